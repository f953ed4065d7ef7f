"""k_camera against k_image (atomic mode) over the same resident rows: the catalogue of
Input.run(1e6) (1.3e8 float32 rows in HBM), a 512 x 512 radiance image each -- the orthographic
ModelImage frame (8 x 8 R) and a camera 6 R from the planet with a 60 x 60 degree field of view.
The two kernels are alternated in one process, 3 warm-up rounds and 9 timed ones; each round's
figure is the HIP-event time (nxc_last_kernel_ms) summed over the launches.  Prints one JSON line
with the medians, the spread, the binned samples of each (one memory-side atomic request per binned
sample binds both) and the ratio.

    python tools/gpu_exp_camera.py [N]          (default: 1e6)
"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                            # noqa: E402
from nexoclom_amd import CameraImage, Input, ModelImage, hip_api   # noqa: E402
from nexoclom_amd.catalogue import sample_spans                    # noqa: E402

WARMUP, ROUNDS = 3, 9


def spans(inputs, ctx):
    """The row ranges the classes launch over (adjacent slices of a store merged)."""
    return [span for _, span in sample_spans(inputs._catalogue, ctx)]


def main():
    n = float(sys.argv[1]) if len(sys.argv) > 1 else 1e6
    ctx = hip_api.Context(0)
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(n, seed=7, context=ctx)
        # the two classes set their descriptions (and check the whole path once)
        image = ModelImage(inputs, dict(quantity='radiance', dims='512,512', width='8,8'), context=ctx)
        cam = CameraImage(inputs, dict(quantity='radiance', observer='0,-6,0', fov='60,60',
                                       dims='512,512'), context=ctx)
    launches = spans(inputs, ctx)
    rows = sum(s[2] for s in launches)
    ctx.image_mode('atomics')
    times = {'k_image': [], 'k_camera': []}
    binned = {}
    for rnd in range(WARMUP + ROUNDS):
        for name in ('k_image', 'k_camera'):
            ms, hit = 0.0, 0
            for store, first, count in launches:
                if name == 'k_image':
                    ctx.image_accumulate_rows(store, first, count)
                else:
                    ctx.camera_accumulate(rows=(store, first, count))
                ms += ctx.last_kernel_ms()
                hit += ctx.counters()['samples_binned']
            binned[name] = hit
            if rnd >= WARMUP:
                times[name].append(ms)
    ctx.image_mode('auto')
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps(dict(
        npackets=n, rows=rows, launches=len(launches), dims=[512, 512],
        image_packets=float(image.packet_image.sum()), camera_packets=float(cam.packet_image.sum()),
        binned=binned,
        k_image_ms=dict(median=round(med['k_image'], 3), min=round(min(times['k_image']), 3),
                        max=round(max(times['k_image']), 3)),
        k_camera_ms=dict(median=round(med['k_camera'], 3), min=round(min(times['k_camera']), 3),
                         max=round(max(times['k_camera']), 3)),
        ratio=round(med['k_camera']/med['k_image'], 3),
        requests_per_s=dict(k_image=round(binned['k_image']/med['k_image']*1e3, -7),
                            k_camera=round(binned['k_camera']/med['k_camera']*1e3, -7)))), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
