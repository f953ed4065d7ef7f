"""nexoclom_amd: MI355X-native implementation of nexoclom's particle-tracking + image hot path.

Same front door as the reference package (nexoclom/__init__.py:9-14): Input, Output, ModelImage,
SSObject, ModelDensity (data_simulation/ModelDensity.py), LOSResult and LOSResultFitted
(data_simulation/LOSResult*.py), plus CameraImage (perspective images) and ShellMap (density and
zenith column per local time, latitude and altitude), both extensions.  Importing this package touches
neither a database nor the GPU; the HIP library is loaded on first use and there is no CPU
fallback for the integrator or the image kernels.
"""
__version__ = '0.1.0'

from .Input import Input                    # noqa: F401
from .Output import Output                  # noqa: F401
from .ModelImage import ModelImage, ModelResult   # noqa: F401
from .LOSResult import LOSResult, SpacecraftData   # noqa: F401
from .ModelDensity import ModelDensity        # noqa: F401
from .CameraImage import CameraImage          # noqa: F401
from .ShellMap import ShellMap                # noqa: F401
from .LOSResultFitted import LOSResultFitted  # noqa: F401
from .sourcemap import SourceMap              # noqa: F401
from .transient import TransientImages, TransientRadiance, response_matrix   # noqa: F401
from .solarsystem import SSObject, planet_dist    # noqa: F401
from .atomicdata import gValue, RadPresConst, PhotoRate, atomicmass   # noqa: F401
from .input_classes import InputError       # noqa: F401
