"""k_image_cube against k_image (atomic mode) and k_image_moments, then k_camera_cube against k_camera
and k_camera_moments, over the same resident rows as tools/gpu_exp_image_moments.py: the catalogue
of Input.run(1e6) (1.3e8 float32 rows in HBM), 512 x 512 radiance -- the orthographic ModelImage
frame (8 x 8 R) and a camera at 0,-3,0.5 with a 60 x 45 degree field of view; cube = (-10, 10, 64)
km/s.  One process; the three kernels of a consumer are alternated, 3 warm-up rounds and 9 timed
ones; a round's figure is the HIP-event time (nxc_last_kernel_ms) summed over the launches.  One
JSON line per consumer (appended to ``--out FILE``) with median [min, max] and the two floors of the
cube kernel:

  bytes    20 B per float32 row plus 8 B (vx, vz) per binned sample with w != 0, at the box's
           k_stream_copy rate measured in the same run;
  atomics  two requests per binned sample with w != 0 and one for every other binned sample, at
           the 2.4e10 requests/s of profiles/r01_ubench_atomics.txt.

The samples with w != 0 are counted on the host as in tools/gpu_exp_image_moments.py.  No time is
a gate: the lines say what was measured and which floor is nearer.

    python tools/gpu_exp_image_cube.py [--out FILE] [N]          (default: 1e6)
"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import numpy as np                                            # noqa: E402
from gpu_exp_image_moments import ATOMIC_RPS, ROUNDS, WARMUP, lit_and_binned, spread   # noqa: E402
from nexoclom_amd import CameraImage, Input, ModelImage, hip_api   # noqa: E402
from nexoclom_amd.catalogue import sample_spans                    # noqa: E402

CUBE_KMS, NV = (-10.0, 10.0), 64


def main():
    args = sys.argv[1:]
    out_path = None
    if '--out' in args:
        out_path = args[args.index('--out') + 1]
        del args[args.index('--out'):args.index('--out') + 2]
    n = float(args[0]) if args else 1e6
    ctx = hip_api.Context(0)
    copy_bps = ctx.stream_copy_gbs()*1e9
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    image_params = dict(quantity='radiance', dims='512,512', width='8,8')
    camera_params = dict(quantity='radiance', observer='0,-3,0.5', fov='60,45', dims='512,512')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(n, seed=7, context=ctx)
        # the classes check the whole path once and leave their descriptions set, moments enabled;
        # the cube is an independent state of the handle and is enabled beside them
        cam = CameraImage(inputs, camera_params, context=ctx, moments=True)
        image = ModelImage(inputs, image_params, context=ctx, moments=True)
    cube = (NV, CUBE_KMS[0]/image.unit_km, CUBE_KMS[1]/image.unit_km)
    ctx.image_cube_enable(*cube)
    ctx.camera_cube_enable(*cube)
    launches = [span for _, span in sample_spans(inputs._catalogue, ctx)]
    rows = sum(s[2] for s in launches)
    nonzero = lit_and_binned(launches, image, cam)
    passes = {
        'image': {'k_image': lambda span: ctx.image_accumulate_rows(*span),
                  'k_image_moments': lambda span: ctx.image_moments_accumulate(rows=span),
                  'k_image_cube': lambda span: ctx.image_cube_accumulate(rows=span)},
        'camera': {'k_camera': lambda span: ctx.camera_accumulate(rows=span),
                   'k_camera_moments': lambda span: ctx.camera_moments_accumulate(rows=span),
                   'k_camera_cube': lambda span: ctx.camera_cube_accumulate(rows=span)},
    }
    ctx.image_mode('atomics')
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
        plain_name, moments_name, cube_name = kernels
        assert len(set(binned.values())) == 1
        hits, lit = binned[cube_name], nonzero[which]
        download = ctx.image_cube_download if which == 'image' else ctx.camera_cube_download
        sums = download()[..., 0]
        in_range = float(sums[..., 1:-1].sum()/sums.sum())
        med = {name: float(np.median(t)) for name, t in times.items()}
        floors = dict(bytes_ms=round((20*rows + 8*lit)/copy_bps*1e3, 3),
                      atomics_ms=round((hits + lit)/ATOMIC_RPS*1e3, 3))
        binds = max(floors, key=floors.get)
        line = json.dumps({
            'npackets': n, 'rows': rows, 'launches': len(launches), 'dims': [512, 512],
            'cube_kms': list(CUBE_KMS) + [NV], 'consumer': which, 'binned': hits,
            'binned_nonzero': lit, 'weight_inside_the_range': round(in_range, 4),
            **{name + '_ms': spread(t) for name, t in times.items()},
            'cube_over_plain': round(med[cube_name]/med[plain_name], 3),
            'cube_over_moments': round(med[cube_name]/med[moments_name], 3),
            'between_plain_and_moments': med[plain_name] <= med[cube_name] <= med[moments_name],
            'requests_per_s': round((hits + lit)/med[cube_name]*1e3, 0),
            'stream_copy_gbs': round(copy_bps/1e9, 1), 'floors': floors, 'binding_floor': binds,
            'floor_share_of_kernel_time': round(floors[binds]/med[cube_name], 3)})
        print(line, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(line + '\n')
    ctx.image_mode('auto')
    ctx.close()


if __name__ == '__main__':
    main()
