"""The plan of the tiled stored-sample image (nxc_tile_plan.hpp), without a GPU."""
import os
import subprocess

from tests import tile_plan_restatement as TP

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_plan_as_a_host_program(tmp_path):
    """How an image is cut into tiles and the samples into slabs, producers and chunks, and where
    the regions of the chunk scratch lie, is host-only code (nxc_tile_plan.hpp) that nxc_api.hip
    and the kernels share.  tests/tools/tile_plan_check.cpp sweeps images from 1 x 1 to 1100 x
    1100, tiles of 1 to 8192 pixels, image tables around every LDS limit, 1 to 2^31 samples
    (around 2^15 x cap x producers, where the 16-bit chunk numbers force smaller slabs), slab limits
    from 1 up, 1 to 2048 producer slots and both sample widths, and checks what the kernels rely
    on.  Built plainly here; the same file is what is built with -fsanitize=address,undefined.
    The plans it prints for a fixed list of inputs equal those of the Python restatement that the
    GPU tests (test_gpu_image_tiles_edges.py) take their structure from."""
    exe = tmp_path / 'tile_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', 'tile_plan_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout
    lines = done.stdout.strip().split('\n')
    assert lines[-1] == ('577600 geometries (154129 fit, 214465564 pixels mapped), 190158 sample '
                         'plans (27440839 slabs walked, 17802 cut by 16-bit chunk numbers), '
                         '0 unexpected')
    table = [ln for ln in lines[:-1] if ln.startswith('plan ')]
    assert len(table) == len(lines) - 1 == 22
    refused = 0
    for ln in table:
        left, right = ln[5:].split(':')
        nx, nz, tile_pixels, img_bytes, p, limit, slots, width = (int(v) for v in left.split())
        g = TP.geometry(nx, nz, tile_pixels, img_bytes)
        if right.strip() == 'refused':
            assert g is None, ln
            refused += 1
            continue
        s = TP.slabs(g, p, limit, slots, width)
        mine = [g['lg'], g['tile_used'], g['cap'], g['lds_bin'], int(TP.room(img_bytes)), s['slab'],
                s['prod'], s['span'], s['mc'], s['o_sl'], s['o_list'], s['o_n'], s['bytes']]
        assert mine == [int(v) for v in right.split()], ln
    assert refused == 4


def test_restated_pixel_maps_and_list_shapes():
    """The restatement's own helpers: every pixel of a 100 x 8 image in 128 tiles has a place and
    comes back from it; a list of m entries has ceil(m / cap) chunks and a last one of 1..cap."""
    g = TP.geometry(100, 8, 8)
    assert (g['nb'], g['cap'], g['tile_used']) == (128, 64, 8)
    for ix in range(100):
        for iz in range(8):
            b, loc = TP.tile_of(ix, g), TP.place(ix, iz, g)
            assert 0 <= loc < g['tile_used'] and TP.pixel(loc, b, g) == ix*8 + iz
    m = [0, 1, 63, 64, 65, 127, 128, 129]
    assert list(TP.chunks(m, 64)) == [0, 1, 1, 1, 2, 2, 2, 3]
    assert list(TP.last_fill(m, 64)) == [0, 1, 63, 64, 1, 63, 64, 1]
    s = TP.slabs(g, 2*2048 + 1, sample_bytes=8)
    n = TP.lists(g, s, [5]*(2*2048 + 1))
    assert n.shape == (1, 3, 128) and list(n[0, :, 5]) == [2048, 2048, 1] and n.sum() == 4097
