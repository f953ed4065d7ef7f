"""Generate tests/golden/g12_bounce.npz FROM THE REFERENCE'S OWN bouncepackets().

Build machine only: it needs a checkout of the reference, named by the first argument or by
$NEXOCLOM_REFERENCE.

    python tests/tools/make_bounce_golden.py REFERENCE_CHECKOUT

particle_tracking/bouncepackets.py and initial_state/surface_temperature.py are loaded by path
under empty stub parent packages (neither needs astropy; ``geometry.taa`` is the one-element
ndarray subclass with ``.value`` of make_surface_temperature_golden.py).  The reference's
``bouncepackets(outputs, Ximpcheck, r0, hitplanet)`` is called with a duck ``outputs``:
  randgen.random(n)     hands out, in the reference's draw order (sin altitude, azimuth,
                        probability), the Philox uniforms of np_oracle.philox_uniform_pairs for
                        each row's (packet id, bounce number): stream 0xb0c, blocks 2k and 2k + 1
  surfaceint.v_interp   scipy's .ev of the v(T, p) spline that tests/test_thermal_source_cpu.py
                        pins to the reference's construction
  surfaceint.stickcoef  the reference's closure (SurfaceInteraction.py:15-20) over the loaded
                        reference surface_temperature and the case's A

What the file holds, per case c in tests/bounce_cases.CASES (tests/test_bounce_cpu.py compares
np_oracle.bounce_packets with it bit for bit):
  c_X [n, 8]        states after the step that took the packets below the surface (and a few that
                    stayed above: hit = False)
  c_r0, c_hit [n]   their radii and the reference's hitplanet mask
  c_ids, c_nb [n]   packet ids (consecutive from 0, 2^32 - 100, 2^33 + 5, 2^32) and bounce numbers
                    (0..40 on half of the random rows, 0 elsewhere)
  c_u [3, n]        the three uniforms handed to the reference
  c_out [n, 8]      the reference's rows afterwards
  c_edge [n]        0 for the random rows, else the number of the hand-made edge family
  c_scalars, c_A    taa, accomfactor, temperature-dependent flag, stickcoef; A[3]
  GM, unit_km, seed, edge_names
Edge rows on which the reference asserts or returns a non-finite row are left out (and printed).
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nexoclom_amd.solarsystem import SSObject     # noqa: E402
from tests import bounce_cases as B               # noqa: E402

SEED = 12
N_RANDOM = 400
FIRST_INDEX = (0, 2**32 - 100, 2**33 + 5, 2**32)
EDGE_NAMES = ['random', 'terminator pi/2', 'terminator 3pi/2', 'longitude 0', 'near pole',
              'grazing', 'v_old2 clamped', 'subsolar point', 'night side', 'moving outward',
              'probability in an end interval']


class Angle(np.ndarray):
    @property
    def value(self):
        return np.asarray(self)


def load_reference(ref_root):
    base = os.path.join(ref_root, 'nexoclom')

    def load(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, *path))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
        return module

    for stub in ('nexoclom', 'nexoclom.initial_state', 'nexoclom.particle_tracking'):
        sys.modules[stub] = types.ModuleType(stub)
        sys.modules[stub].__path__ = []
    st = load('nexoclom.initial_state.surface_temperature', 'initial_state', 'surface_temperature.py')
    bp = load('nexoclom.particle_tracking.bouncepackets', 'particle_tracking', 'bouncepackets.py')
    return bp.bouncepackets, st.surface_temperature


class Draws:
    """randgen.random(n): the prepared vectors, one per call."""

    def __init__(self, vectors):
        self.vectors = list(vectors)

    def random(self, n):
        v = self.vectors.pop(0)
        assert len(v) == n
        return v.copy()


def duck_outputs(case, GM, unit_km, u, surface_temperature):
    taa, accom, tempdep, stick, A = case
    geo = types.SimpleNamespace(startpoint='Mercury',
                                taa=np.array([taa], dtype=np.float64).view(Angle),
                                planet=types.SimpleNamespace(
                                    radius=types.SimpleNamespace(value=unit_km)))
    si = types.SimpleNamespace(accomfactor=accom, stickcoef=stick,
                               sticktype='temperature dependent' if tempdep else 'constant', A=A)
    inputs = types.SimpleNamespace(geometry=geo, surfaceinteraction=si)

    def stickcoef(lon, lat):                       # SurfaceInteraction.py:15-20
        tsurf = surface_temperature(inputs.geometry, lon, lat)
        coef = A[0] * np.exp(A[1]*tsurf) + A[2]
        coef[coef > 1.] = 1.
        coef[coef < 0.] = 0.
        return coef

    surfaceint = types.SimpleNamespace(stickcoef=stickcoef)
    if accom != 0:
        surfaceint.v_interp = B.thermal_spline(taa).ev
    return types.SimpleNamespace(GM=GM, inputs=inputs, surfaceint=surfaceint,
                                 randgen=Draws(u if accom != 0 else u[:2]))


def random_rows(rng, n, unit_km):
    depth = 10**rng.uniform(-7, np.log10(3e-2), n)
    pos = B.unit(rng.normal(size=(n, 3)))*(1 - depth)[:, None]
    vel = B.unit(rng.normal(size=(n, 3)))*(rng.uniform(0.3, 4.0, n)/unit_km)[:, None]
    return pos, vel


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NEXOCLOM_REFERENCE')
    if not ref_root:
        sys.exit(__doc__)
    bouncepackets, surface_temperature = load_reference(ref_root)
    mercury = SSObject('Mercury')
    unit_km = float(mercury.radius.value)
    GM = float(mercury.GM.value/(unit_km*1e3)**3)
    out = dict(GM=np.float64(GM), unit_km=np.float64(unit_km), seed=np.int64(SEED),
               edge_names=np.array(EDGE_NAMES))
    for c, (name, case) in enumerate(B.CASES.items()):
        rng = np.random.default_rng(SEED + c)
        pos, vel = random_rows(rng, N_RANDOM, unit_km)
        fam = np.zeros(N_RANDOM, dtype=np.int64)
        edges = B.edge_rows(unit_km)
        pos = np.concatenate([pos, np.array([e[1] for e in edges], dtype=float)])
        vel = np.concatenate([vel, np.array([e[2] for e in edges], dtype=float)])
        fam = np.concatenate([fam, np.array([e[0] for e in edges])])
        n = len(fam)
        # consecutive ids from the case's first index (what a launch gives its packets), straddling
        # the high counter word; bounce numbers 0..40 on half of the random rows, 0 elsewhere (the
        # rows a single-impact launch can reproduce)
        ids = np.uint64(FIRST_INDEX[c]) + np.arange(n, dtype=np.uint64)
        nb = np.zeros(n, dtype=np.int64)
        later = np.nonzero(fam == 0)[0][::2]
        nb[later] = rng.integers(0, 41, len(later))
        nb[later[:4]] = [40, 1, 39, 40]
        # 10: packets whose probability draw falls in the first / last knot interval of ty
        p = B.uniforms(ids, nb, SEED)[2]
        ends = (fam == 0) & (nb == 0) & ((p < 0.01) | (p > 0.99))
        assert (ends & (p < 0.01)).sum() >= 2 and (ends & (p > 0.99)).sum() >= 2
        fam[ends] = 10
        X = np.zeros((n, 8))
        X[:, 0] = rng.uniform(30., 9000., n)
        X[:, 1:4], X[:, 4:7] = pos, vel
        X[:, 7] = 10**rng.uniform(-9.5, 0, n)
        # frac goes through log and exp in every rk5 step: 1 is the value a step hands on unchanged,
        # so the rows a launch can reproduce carry it
        X[nb == 0, 7] = 1.0
        # a few packets that stayed above the surface: not in hitplanet, must come back untouched
        above = np.nonzero(fam == 0)[0][41:81:2]
        X[above, 1:4] *= 1.1
        r0 = np.sqrt((X[:, 1]*X[:, 1] + X[:, 2]*X[:, 2]) + X[:, 3]*X[:, 3])
        hit = (r0 - 1.) < 0
        assert not hit[above].any() and hit.sum() == n - len(above)
        u = B.uniforms(ids, nb, SEED)

        def reference(rows):
            Xr = X[rows].copy()
            bouncepackets(duck_outputs(case, GM, unit_km, u[:, rows][:, hit[rows]],
                                       surface_temperature), Xr, r0[rows], hit[rows])
            return Xr

        keep = np.ones(n, dtype=bool)
        result = np.zeros((n, 8))
        plain = np.nonzero((fam == 0) | (fam == 10))[0]
        result[plain] = reference(plain)
        for row in np.nonzero((fam != 0) & (fam != 10))[0]:
            try:
                with np.errstate(all='ignore'):
                    result[row] = reference(np.array([row]))
                if not np.all(np.isfinite(result[row])):
                    raise AssertionError('non-finite row')
            except AssertionError as exc:
                keep[row] = False
                print(f'{name}: left out {EDGE_NAMES[fam[row]]} row {row}: {exc!r}'[:150])
        assert np.all(np.isfinite(result[keep]))
        for key, value in (('X', X), ('r0', r0), ('hit', hit), ('ids', ids), ('nb', nb),
                           ('out', result), ('edge', fam)):
            out[f'{name}_{key}'] = value[keep]
        out[f'{name}_u'] = u[:, keep]
        out[f'{name}_scalars'] = np.array(case[:4], dtype=np.float64)
        out[f'{name}_A'] = np.array(case[4], dtype=np.float64)
        kept = fam[keep]
        print(f'{name}: {keep.sum()} rows, edge families',
              {EDGE_NAMES[f]: int((kept == f).sum()) for f in np.unique(kept) if f})
    np.savez_compressed(B.GOLDEN, **out)
    print(f'{B.GOLDEN}: {os.path.getsize(B.GOLDEN)} bytes')


if __name__ == '__main__':
    main()
