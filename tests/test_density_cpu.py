"""ModelDensity without a GPU: the point index (its neighbour cells cover every ball), the
reference's scaling (ModelDensity.py:56,84-87, the Vpix quirk included) and a run shared by two
ranks.  The device is replaced by a NumPy brute-force stand-in (DensityContext below)."""
import contextlib
import io
import multiprocessing as mp
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest

from tests.density_walk_cases import candidate_cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')


def brute_force(points, dr, x, y, z, frac):
    """(frac sums, counts) per point: the membership rule in fp64, d = q - p,
    (dx*dx + dy*dy) + dz*dz <= dr*dr, over every sample."""
    sums, counts = np.zeros(len(points)), np.zeros(len(points))
    x, y, z, frac = (np.asarray(c, dtype=np.float64) for c in (x, y, z, frac))
    for j, (qx, qy, qz) in enumerate(points):
        dx, dy, dz = qx - x, qy - y, qz - z
        hit = (dx*dx + dy*dy) + dz*dz <= dr*dr
        sums[j], counts[j] = frac[hit].sum(), hit.sum()
    return sums, counts


def _check_cover(points, rows, dr):
    from nexoclom_amd.ModelDensity import DensityIndex
    index = DensityIndex(points, dr)
    assert index.h >= dr*(1 + 2**-20)
    assert int(np.prod(index.dims)) <= 1 << 24
    assert index.cell_start[0] == 0 and index.cell_start[-1] == len(index.points)
    assert np.all(np.diff(index.cell_start) >= 0)
    position = np.empty(len(index.points), dtype=np.int64)     # indexed point -> its cell
    for c in range(len(index.cell_start) - 1):
        position[index.cell_start[c]:index.cell_start[c + 1]] = c
    hits = 0
    for p in rows:
        d = index.points - p
        hit = np.flatnonzero((d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1]) + d[:, 2]*d[:, 2] <= dr*dr)
        if len(hit):
            cells = set(candidate_cells(index, p))
            assert set(position[hit]) <= cells, (p, position[hit], cells)
            hits += len(hit)
    return index, hits


def test_neighbour_cells_cover_every_ball():
    rng = np.random.default_rng(7)
    dr = 0.05
    points = rng.uniform(-1, 1, (400, 3))
    # points on cell faces: the grid's own origin plus whole multiples of the edge
    from nexoclom_amd.ModelDensity import DensityIndex
    probe = DensityIndex(points, dr)
    faces = probe.origin + probe.h*rng.integers(0, 20, (100, 3))
    points = np.concatenate([points, faces, points[:5]])         # duplicates too
    rows = [rng.uniform(-1.1, 1.1, (3000, 3))]
    for axis in range(3):               # rows at +-dr along each axis, and a rounding either side
        for sign in (-1, 1):
            shifted = points.copy()
            shifted[:, axis] += sign*dr
            rows += [shifted, np.nextafter(shifted, shifted + sign), np.nextafter(shifted, 0*shifted)]
    on_sphere = rng.normal(size=(points.shape[0], 3))
    on_sphere *= dr/np.linalg.norm(on_sphere, axis=1)[:, None]
    rows.append(points + on_sphere)
    rows = np.concatenate(rows)
    index, hits = _check_cover(points, rows, dr)
    assert hits > 3000
    # float32 rows, as the stored rows are, widened
    _check_cover(points, rows.astype(np.float32).astype(np.float64), dr)


def test_cell_cap_grows_the_edge_and_still_covers():
    from nexoclom_amd.ModelDensity import DensityIndex
    rng = np.random.default_rng(3)
    dr = 1e-3
    points = np.concatenate([rng.uniform(-50, 50, (300, 3)), rng.uniform(0, 0.01, (200, 3))])
    index, hits = _check_cover(points, np.concatenate([points + rng.normal(0, dr/2, points.shape),
                                                       rng.uniform(0, 0.01, (2000, 3))]), dr)
    assert index.h > 100*dr and hits > 200
    # non-finite points are left out and get nothing
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, 0.5]])
    idx = DensityIndex(bad, 0.1)
    assert list(idx.order) == [2] and len(idx.points) == 1
    assert np.array_equal(idx.scatter(np.array([3.0]), 3), [0, 0, 3.0])
    assert len(DensityIndex(bad[:2], 0.1).points) == 0
    with pytest.raises(ValueError):
        DensityIndex(bad, 0.0)


def _stand_in():
    from tests.oracle_context import OracleContext

    class DensityContext(OracleContext):
        """The density calls of hip_api.Context, by brute force over every sample."""

        def density_set(self, points, cell_start, origin, h, dr, dims):
            self._dpoints, self._ddr = np.array(points, dtype=np.float64).reshape(-1, 3), float(dr)
            self._dsum = np.zeros(len(self._dpoints))
            self._dcount = np.zeros(len(self._dpoints))

        def density_accumulate(self, x=None, y=None, z=None, frac=None, rows=None):
            if rows is not None:
                store, first, count = rows
                r, _ = store.download(first, count, index=False)
                x, y, z, frac = r[1], r[2], r[3], r[7]
            s, c = brute_force(self._dpoints, self._ddr, x, y, z, frac)
            self._dsum += s
            self._dcount += c

        def density_download(self):
            return self._dsum.copy(), self._dcount.copy()
    return DensityContext


def _fake_inputs(runs):
    from nexoclom_amd import Input
    inputs = Input(INPUT)
    inputs._catalogue = runs
    return inputs


def test_formulas_and_scaling():
    """Vpix = 4/3/pi dr^3 in cm^3 (the reference's quirk: not the ball's volume),
    atoms_per_packet = 1e23 / (totalsource / endtime), density = sum(frac) * atoms_per_packet /
    Vpix, packets = the count; totals over the Outputs."""
    from nexoclom_amd import ModelDensity
    X1 = pd.DataFrame({'x': np.float32([1.0, 1.05, 3.0]), 'y': np.float32([0, 0, 0]),
                       'z': np.float32([0, 0, 0]), 'frac': np.float32([0.5, 0.25, 1.0])})
    X2 = pd.DataFrame({'x': [1.0], 'y': [0.02], 'z': [0.0], 'frac': [0.125]})
    runs = [types.SimpleNamespace(X=X1, totalsource=1000., npackets=10, idnum=1, filename='a'),
            types.SimpleNamespace(X=X2, totalsource=500., npackets=5, idnum=2, filename='b')]
    inputs = _fake_inputs(runs)
    endtime = inputs.options.endtime.value
    R_km = inputs.geometry.planet.radius.value
    with contextlib.redirect_stdout(io.StringIO()):
        d = ModelDensity(inputs, [1.0, 3.0, 10.0, np.nan], [0, 0, 0, 0], [0, 0, 0, 0], dr=0.1,
                         context=_stand_in()())
    assert d.type == 'density' and d.unit == 'R_Mercury'
    Vpix = 4/3/np.pi*0.1**3*(R_km*1e5)**3
    assert np.isclose(float(d.Vpix), Vpix, rtol=1e-15)
    assert np.isclose(float(d.Vpix), 4/(3*np.pi)*(0.1*R_km*1e5)**3, rtol=1e-14)
    assert d.totalsource == 1500.
    apc = 1e23/(1500./endtime)
    assert d.atoms_per_packet == apc
    assert np.array_equal(d.packets, [3.0, 1.0, 0.0, 0.0])
    want = np.array([0.5 + 0.25 + 0.125, 1.0, 0., 0.])*apc/Vpix
    np.testing.assert_allclose(d.density, want, rtol=1e-15, atol=0)
    assert d.outid == [1, 2] and d.outputfiles == ['a', 'b'] and float(d.dr) == 0.1
    assert float(d.sourcerate) == 1.0


def test_empty_catalogue_raises():
    from nexoclom_amd import ModelDensity
    with pytest.raises(RuntimeError, match='No packets found'):
        ModelDensity(_fake_inputs([]), [0.], [0.], [0.], context=_stand_in()())


N, SIZE = 1000, 500                      # two Outputs of 500 packets: one per rank


def _points():
    rng = np.random.default_rng(11)
    return rng.uniform(-2, 2, 150), rng.uniform(-2, 2, 150), rng.uniform(-1, 1, 150)


def _worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from nexoclom_amd import Input, ModelDensity
    from nexoclom_amd.distributed import ControlPlane
    cp = ControlPlane(world, rank, timeout=120)
    Ctx = _stand_in()

    def flow(cp_):
        inputs = Input(INPUT)
        inputs.options.endtime = type(inputs.options.endtime)(6000., 's')
        ctx = Ctx()
        with contextlib.redirect_stdout(io.StringIO()):
            inputs.run(N, packs_per_it=SIZE, seed=5, context=ctx, cp=cp_)
            return inputs, ModelDensity(inputs, *_points(), dr=0.2, cp=cp_, reduce='host',
                                        context=ctx)
    inputs, shared = flow(cp)
    assert len(inputs._catalogue) == 1                     # this rank's share
    if rank == 0:
        alone_inputs, alone = flow(None)
        assert len(alone_inputs._catalogue) == 2
        assert alone.packets.sum() > 100
        assert np.array_equal(shared.packets, alone.packets)
        np.testing.assert_allclose(shared.density, alone.density, rtol=1e-12, atol=0)
        assert shared.totalsource == alone.totalsource and shared.npackets == alone.npackets == N
        assert shared.atoms_per_packet == alone.atoms_per_packet
        open(os.path.join(tmpdir, 'ok'), 'w').write('ok')
    cp.barrier()
    cp.close()


def test_two_ranks_equal_one_rank(tmp_path):
    port = 29100 + os.getpid() % 150
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert (tmp_path / 'ok').exists()


def test_density_desc_layout_matches_header():
    import ctypes as C
    from nexoclom_amd import hip_api
    d = hip_api.nxc_density_desc
    # 3 + 2 doubles, 3 + 1 int64, 2 pointers
    assert C.sizeof(d) == 5*8 + 4*8 + 2*8
    assert d.h.offset == 24 and d.dims.offset == 40 and d.n_points.offset == 64
    assert d.points.offset == 72 and d.cell_start.offset == 80
