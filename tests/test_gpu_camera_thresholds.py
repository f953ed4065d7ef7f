"""k_camera, k_camera_moments, k_camera_cube and k_camera_ages on the GPU, ON the thresholds the
guarded tests (tests/test_gpu_camera.py and the camera scenes of the pixel-moments, pixel-cube and
age-cube tests) keep 1e-9 away from.

include/nexoclom_hip.h defines the camera pass operation by operation in fp64 with one rounding per
operation, so every decision a sample meets -- in front of the camera or not, which pixel, hidden
or not, sunlit or not, finite or dropped -- is a function of its bits, and the kernels are held to
tests/camera_restatement.py exactly on the inputs of tests/threshold_cases.py: brackets (two
adjacent doubles or floats on either side of a decision) and exact hits (the decided quantity equal
to the threshold), among guarded padding, in two arrangements in the wave.  No guard is asserted
here: tests/test_threshold_cases_cpu.py asserts instead, without a GPU, that every bracket and hit
is what it claims to be and that a scalar restatement written from the header agrees with the NumPy
one on every sample.

Asserted: packet counts per pixel and the counters samples, samples_binned and nonfinite equal to
the restatement's exactly; the image at the existing rtol 1e-11 (sums taken in another order); and,
for every bracket, that the two pixels (a pixel border, a frame border) or the two weights (hidden
or not, sunlit or not, finite or dropped) the restatement predicts are the ones found in the
download.  The kernels that share camera_located run the cases of steps 2, 3 and 4; their packet
image, image and counters come from the same download (their own sums have their own tests)."""
import numpy as np
import pytest

from tests import threshold_cases as T
from tests.test_gpu_camera import RTOL, forces, set_camera, tables                       # noqa: F401

pytestmark = pytest.mark.gpu
SHARED_FRONT = [name for name in T.CAMERA_CASES if 'sunlit' not in name]      # steps 2, 3 and 4


def plain(ctx, case):
    ctx.camera_accumulate(*case['cols'])


def moments(ctx, case):
    x, y, z, vy, frac = case['cols']
    vx, vz, _ = T.extra_columns(case)
    ctx.camera_moments_enable()
    ctx.camera_moments_accumulate(x, y, z, vx, vy, vz, frac)


def cube(ctx, case):
    x, y, z, vy, frac = case['cols']
    vx, vz, _ = T.extra_columns(case)
    ctx.camera_cube_enable(3, -1e-3, 1e-3)
    ctx.camera_cube_accumulate(x, y, z, vx, vy, vz, frac)


def ages(ctx, case):
    time = T.extra_columns(case)[2]
    ctx.camera_ages_enable(3, 3000.0, 500.0, 2500.0)
    ctx.camera_ages_accumulate(time, *case['cols'])


def check(ctx, forces, name, accumulate):
    case = T.CASES[name]()
    want, d = T.restated(name)
    quantity, gt = tables(forces, case['kind'])
    set_camera(ctx, case['camera'], forces, quantity, gt)
    accumulate(ctx, case)
    counters = ctx.counters()
    image, counts = ctx.camera_download()
    print(f'{name}: {want.samples} samples, {want.binned} binned, {want.nonfinite} nonfinite; '
          f'{len(case["brackets"])} brackets, {len(case["hits"])} exact hits')
    nz = counts.shape[1]
    # the brackets first, so that a failure names its threshold
    for ia, ib, label, which in case['brackets']:
        pa, pb = int(d['pix'][ia]), int(d['pix'][ib])
        if which in ('ix', 'iz'):
            assert pa != pb
        for i, pix in ((ia, pa), (ib, pb)):
            if d['keep'][i]:
                at = divmod(pix, nz)
                assert counts[at] == want.counts[at], (label, i, at)
                np.testing.assert_allclose(image[at], want.image[at], rtol=RTOL, atol=0,
                                           err_msg=f'{label}, sample {i}, pixel {at}')
    for i, label, *_ in case['hits']:
        if d['keep'][i]:
            at = divmod(int(d['pix'][i]), nz)
            assert counts[at] == want.counts[at], (label, i, at)
    assert np.array_equal(counts, want.counts)
    assert counters['samples'] == want.samples
    assert counters['samples_binned'] == want.binned == want.counts.sum()
    assert counters['nonfinite'] == want.nonfinite
    np.testing.assert_allclose(image, want.image, rtol=RTOL, atol=0)
    return want, d


@pytest.mark.parametrize('name', T.CAMERA_CASES)
def test_camera_on_the_thresholds(ctx, forces, name):
    want, d = check(ctx, forces, name, plain)
    assert want.binned > 0
    if name.startswith('cam_front_finite'):
        assert want.nonfinite == 10 and np.isfinite(want.image).all() and want.image.max() > 1e308


@pytest.mark.parametrize('accumulate', [moments, cube, ages], ids=lambda f: f.__name__)
@pytest.mark.parametrize('name', SHARED_FRONT)
def test_kernels_that_share_the_front(ctx, forces, name, accumulate):
    check(ctx, forces, name, accumulate)
