"""k_image_moments against k_image (atomic mode) and k_camera_moments against k_camera over the same
resident rows: the catalogue of Input.run(1e6) (1.3e8 float32 rows in HBM), 512 x 512 radiance -- the
orthographic ModelImage frame (8 x 8 R) and a camera at 0,-3,0.5 with a 60 x 45 degree field of view.
One process; each pair of kernels is alternated, 3 warm-up rounds and 9 timed ones; a round's figure
is the HIP-event time (nxc_last_kernel_ms) summed over the launches.  One JSON line per pair
(appended to ``--out FILE``) with median [min, max] and the two floors of the moments kernel:

  bytes    20 B per float32 row plus 8 B (vx, vz) per binned sample with w != 0, at the box's
           k_stream_copy rate measured in the same run;
  atomics  one request per binned sample plus two per binned sample with w != 0, at the 2.4e10
           requests/s of profiles/r01_ubench_atomics.txt.

The samples with w != 0 are not a counter of the kernels: they are counted on the host from the
rows' positions (a sample's weight is zero iff it is hidden by the planet or in its shadow: the
stored rows have frac > 0 and the g-values are positive), in float32 -- a floor does not depend on
the few samples within rounding of a limb.

    python tools/gpu_exp_image_moments.py [--out FILE] [N]          (default: 1e6)
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
ATOMIC_RPS = 2.4e10
CHUNK = 1 << 24


def lit_and_binned(launches, image, cam):
    """Binned samples with w != 0 of the image and of the camera, from the rows' positions."""
    M = image.image_rotation().astype(np.float32)
    o = cam.observer.astype(np.float32)
    C = cam.basis.astype(np.float32)
    count = {'image': 0, 'camera': 0}
    for store, first, total in launches:
        for at in range(first, first + total, CHUNK):
            rows, _ = store.download(at, min(CHUNK, first + total - at), index=False)
            x, y, z = rows[1], rows[2], rows[3]
            sunlit = (x*x + z*z > 1) | (y < 0)
            xo, yo, zo = (M[r, 0]*x + M[r, 1]*y + M[r, 2]*z for r in range(3))
            inside = (xo >= image.xedges[0]) & (xo <= image.xedges[-1]) \
                & (zo >= image.zedges[0]) & (zo <= image.zedges[-1])
            count['image'] += int(np.count_nonzero(inside & sunlit & ((xo*xo + zo*zo > 1) | (yo < 0))))
            dx, dy, dz = x - o[0], y - o[1], z - o[2]
            xc, dc, zc = (C[r, 0]*dx + C[r, 1]*dy + C[r, 2]*dz for r in range(3))
            with np.errstate(all='ignore'):
                u, v = xc/dc, zc/dc
            inside = (dc > 0) & (u >= cam.uedges[0]) & (u <= cam.uedges[-1]) \
                & (v >= cam.vedges[0]) & (v <= cam.vedges[-1])
            r2 = dx*dx + dy*dy + dz*dz
            b = -(o[0]*dx + o[1]*dy + o[2]*dz)
            cx, cy, cz = o[1]*z - o[2]*y, o[2]*x - o[0]*z, o[0]*y - o[1]*x
            hidden = (b > 0) & (b < r2) & (cx*cx + cy*cy + cz*cz < r2)
            count['camera'] += int(np.count_nonzero(inside & sunlit & ~hidden))
    return count


def spread(values):
    return dict(median=round(float(np.median(values)), 3), min=round(min(values), 3),
                max=round(max(values), 3))


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
        # the classes check the whole path once and leave their descriptions set, moments enabled
        cam = CameraImage(inputs, camera_params, context=ctx, moments=True)
        image = ModelImage(inputs, image_params, context=ctx, moments=True)
    launches = [span for _, span in sample_spans(inputs._catalogue, ctx)]
    rows = sum(s[2] for s in launches)
    nonzero = lit_and_binned(launches, image, cam)
    passes = {
        'image': (lambda span: ctx.image_accumulate_rows(*span),
                  lambda span: ctx.image_moments_accumulate(rows=span), 'k_image', 'k_image_moments'),
        'camera': (lambda span: ctx.camera_accumulate(rows=span),
                   lambda span: ctx.camera_moments_accumulate(rows=span), 'k_camera',
                   'k_camera_moments'),
    }
    ctx.image_mode('atomics')
    for which, (plain, moments, plain_name, moments_name) in passes.items():
        times = {plain_name: [], moments_name: []}
        binned = {}
        for rnd in range(WARMUP + ROUNDS):
            for name, accumulate in ((plain_name, plain), (moments_name, moments)):
                ms, hit = 0.0, 0
                for span in launches:
                    accumulate(span)
                    ms += ctx.last_kernel_ms()
                    hit += ctx.counters()['samples_binned']
                binned[name] = hit
                if rnd >= WARMUP:
                    times[name].append(ms)
        assert binned[plain_name] == binned[moments_name]
        hits, lit = binned[moments_name], nonzero[which]
        med = float(np.median(times[moments_name]))
        floors = dict(bytes_ms=round((20*rows + 8*lit)/copy_bps*1e3, 3),
                      atomics_ms=round((hits + 2*lit)/ATOMIC_RPS*1e3, 3))
        binds = max(floors, key=floors.get)
        line = json.dumps({
            'npackets': n, 'rows': rows, 'launches': len(launches), 'dims': [512, 512],
            'consumer': which, 'binned': hits, 'binned_nonzero': lit,
            plain_name + '_ms': spread(times[plain_name]),
            moments_name + '_ms': spread(times[moments_name]),
            'ratio': round(med/float(np.median(times[plain_name])), 3),
            'stream_copy_gbs': round(copy_bps/1e9, 1), 'floors': floors, 'binding_floor': binds,
            'floor_share_of_kernel_time': round(floors[binds]/med, 3)})
        print(line, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(line + '\n')
    ctx.image_mode('auto')
    ctx.close()


if __name__ == '__main__':
    main()
