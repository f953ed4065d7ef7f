"""k_image_ages against k_image_cube, k_camera_ages against k_camera_cube, and k_ages_apply against
a streaming copy, over the same resident rows as tools/gpu_exp_image_cube.py: the catalogue of
Input.run(1e6) (1.3e8 float32 rows in HBM), 512 x 512 radiance, 64 bins -- the cube over (-10, 10)
km/s, the age block over (0, 50000) s, the run's endtime.  One process; the two kernels of a
consumer are alternated, 3 warm-up rounds and 9 timed ones; a round's figure is the HIP-event time
(nxc_last_kernel_ms) summed over the launches.  The ages pass reads one column (time) where the
cube's reads two (vx, vz) and makes the same atomic requests, so it should take no longer than the
cube's pass plus the spread of the cube's pass itself: the line says whether it did
(``ages_within_cube_spread``), and nothing is tuned to make it so.

Then k_ages_apply on the image's block (512 x 512 x 66 records) for ne = 1 and ne = 64, 3 warm-up
and 9 timed calls each, against the box's k_stream_copy rate measured in the same run applied to
the bytes the kernel moves (a rate times a byte count, not a timed copy of those bytes): the block
once per epoch chunk (hip_api.ages_apply_plan) plus K, read, and ne x npix records written.  The ratio is reported; no target is set.

One JSON line per measurement, appended to ``--out FILE``.

    python tools/gpu_exp_image_ages.py [--out FILE] [N]          (default: 1e6)
"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import numpy as np                                            # noqa: E402
from gpu_exp_image_moments import ROUNDS, WARMUP, spread      # noqa: E402
from nexoclom_amd import CameraImage, Input, ModelImage, hip_api   # noqa: E402
from nexoclom_amd.catalogue import sample_spans                    # noqa: E402

CUBE_KMS, NBINS = (-10.0, 10.0), 64


def main():
    args = sys.argv[1:]
    out_path = None
    if '--out' in args:
        out_path = args[args.index('--out') + 1]
        del args[args.index('--out'):args.index('--out') + 2]
    n = float(args[0]) if args else 1e6

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(line + '\n')

    ctx = hip_api.Context(0)
    copy_bps = ctx.stream_copy_gbs()*1e9
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    endtime = float(inputs.options.endtime.value)
    image_params = dict(quantity='radiance', dims='512,512', width='8,8')
    camera_params = dict(quantity='radiance', observer='0,-3,0.5', fov='60,45', dims='512,512')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(n, seed=7, context=ctx)
        # the classes check the whole path once and leave their descriptions set, the age block
        # enabled; the cube is an independent state of the handle and is enabled beside it
        cam = CameraImage(inputs, camera_params, context=ctx, ages=(0.0, endtime, NBINS))
        image = ModelImage(inputs, image_params, context=ctx, ages=(0.0, endtime, NBINS))
    cube = (NBINS, CUBE_KMS[0]/image.unit_km, CUBE_KMS[1]/image.unit_km)
    ctx.image_cube_enable(*cube)
    ctx.camera_cube_enable(*cube)
    launches = [span for _, span in sample_spans(inputs._catalogue, ctx)]
    rows = sum(s[2] for s in launches)
    passes = {
        'image': {'k_image_cube': lambda span: ctx.image_cube_accumulate(rows=span),
                  'k_image_ages': lambda span: ctx.image_ages_accumulate(rows=span)},
        'camera': {'k_camera_cube': lambda span: ctx.camera_cube_accumulate(rows=span),
                   'k_camera_ages': lambda span: ctx.camera_ages_accumulate(rows=span)},
    }
    for which, kernels in passes.items():
        times = {name: [] for name in kernels}
        binned = {}
        for rnd in range(WARMUP + ROUNDS):
            for name, accumulate in kernels.items():
                ms, hit = 0.0, 0
                for span in launches:
                    accumulate(span)
                    ms += ctx.last_kernel_ms()
                    hit += ctx.counters()['samples_binned']
                binned[name] = hit
                if rnd >= WARMUP:
                    times[name].append(ms)
        cube_name, ages_name = kernels
        assert len(set(binned.values())) == 1
        med = {name: float(np.median(t)) for name, t in times.items()}
        cube_spread = max(times[cube_name]) - min(times[cube_name])
        download = ctx.image_ages_download if which == 'image' else ctx.camera_ages_download
        sums = download()[..., 0]
        emit({'npackets': n, 'rows': rows, 'launches': len(launches), 'dims': [512, 512],
              'bins': NBINS, 'ages_s': [0.0, endtime], 'consumer': which,
              'binned': binned[ages_name],
              'weight_inside_the_range': round(float(sums[..., 1:-1].sum()/sums.sum()), 4),
              **{name + '_ms': spread(t) for name, t in times.items()},
              'cube_spread_ms': round(cube_spread, 3),
              'ages_over_cube': round(med[ages_name]/med[cube_name], 3),
              'ages_within_cube_spread': med[ages_name] <= med[cube_name] + cube_spread})

    # the contraction: the image's block as the last pass left it, K of ones and a ramp
    npix, planes = 512*512, NBINS + 2
    for ne in (1, 64):
        K = np.ones((planes, ne)) + np.arange(ne)[None, :]/64.0
        times = []
        for rnd in range(WARMUP + ROUNDS):
            ctx.image_ages_apply(K)
            if rnd >= WARMUP:
                times.append(ctx.last_kernel_ms())
        chunks = -(-ne//hip_api.ages_apply_plan(planes, ne)[2])      # epochs per workgroup
        moved = chunks*npix*planes*16 + planes*ne*8 + ne*npix*16
        med = float(np.median(times))
        emit({'kernel': 'k_ages_apply', 'npix': npix, 'planes': planes, 'ne': ne,
              'epoch_chunks': chunks, 'k_ages_apply_ms': spread(times), 'bytes': moved,
              'k_ages_apply_gbs': round(moved/med/1e6, 1),
              'stream_copy_gbs': round(copy_bps/1e9, 1),
              'stream_copy_ms_same_bytes': round(moved/copy_bps*1e3, 3),
              'apply_over_copy': round(med/(moved/copy_bps*1e3), 3)})
    ctx.close()


if __name__ == '__main__':
    main()
