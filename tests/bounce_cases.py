"""Shared set-up of the surface re-emission tests: the configurations of tests/golden/g12_bounce.npz
and the restatement's view of them (tests/tools/make_bounce_golden.py, tests/test_bounce_cpu.py,
tests/test_gpu_bounce.py)."""
import os
import types

import numpy as np

from nexoclom_amd import surface
from oracle import np_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g12_bounce.npz')
STREAM = 0xb0c
DEFAULT_A = (1.57014, -0.006262, 0.1614157)

# name -> (taa, accomfactor, temperature dependent, stickcoef, A): the two bounce inputfiles of
# tests/inputfiles and the two elastic forms
CASES = {
    'const': (0.5, 0.5, 0, 0.3, (0., 0., 0.)),
    'tempdep': (1.3, 0.2, 1, 0.0, DEFAULT_A),
    'elastic': (1.3, 0.0, 0, 0.0, (0., 0., 0.)),
    'elastic_stick': (0.5, 0.0, 0, 0.4, (0., 0., 0.)),
}

_SPLINES = {}


def geometry(taa):
    return types.SimpleNamespace(startpoint='Mercury', taa=float(taa))


def thermal_spline(taa, species='Na'):
    """The v(T, p) spline of surface.tabulate_thermal_speeds (pinned to the reference's
    construction by tests/test_thermal_source_cpu.py), one per true anomaly."""
    key = (float(taa), species)
    if key not in _SPLINES:
        _SPLINES[key] = surface.tabulate_thermal_speeds(geometry(taa), species)[3]
    return _SPLINES[key]


def config(taa, accomfactor, temp_dependent, stickcoef, A, GM, unit_km, seed, spline=None):
    """The dict np_oracle.bounce_packets and hip_api.Context.set_bounce take."""
    if accomfactor != 0 and spline is None:
        spline = thermal_spline(taa)
    surf = types.SimpleNamespace(v_interp=None if spline is None else spline.ev)
    if spline is None:
        tx, ty, coef = np.zeros(8), np.zeros(8), np.zeros((4, 4))
    else:
        tx, ty, coef = surface.spline_tables(spline)
    return dict(GM=float(GM), unit_km=float(unit_km), accomfactor=float(accomfactor),
                temp_dependent=int(temp_dependent), stickcoef=float(stickcoef),
                A=tuple(float(a) for a in A), t0=surface.NIGHT_SIDE_K,
                t1=float(surface.day_side_t1(geometry(taa))), tpow=0.25, tx=tx, ty=ty, coef=coef,
                seed=int(seed), surf=surf)


def golden_config(g, name):
    """cfg of case ``name`` from the scalars stored in the golden file."""
    taa, accom, tempdep, stick = (g[f'{name}_scalars'][k] for k in range(4))
    return config(taa, accom, int(tempdep), stick, g[f'{name}_A'], float(g['GM']),
                  float(g['unit_km']), int(g['seed']))


def uniforms(ids, nbounce, seed):
    """(sin altitude, azimuth / 2 pi, probability) of packet ``ids`` at bounce numbers ``nbounce``:
    Philox stream 0xb0c, blocks 2k and 2k + 1."""
    ids = np.asarray(ids, dtype=np.uint64)
    nbounce = np.asarray(nbounce, dtype=np.int64)
    u = np.empty((3, len(ids)))
    for k in np.unique(nbounce):
        m = nbounce == k
        u[0, m], u[1, m] = O.philox_uniform_pairs(ids[m], 2*int(k), STREAM, seed)
        u[2, m], _ = O.philox_uniform_pairs(ids[m], 2*int(k) + 1, STREAM, seed)
    return u


def restate(X, cfg, ids, nbounce, hit=None):
    """np_oracle.bounce_packets on copies: rows after the impact."""
    X = np.array(X, dtype=np.float64)
    r0 = np.sqrt((X[:, 1]*X[:, 1] + X[:, 2]*X[:, 2]) + X[:, 3]*X[:, 3])
    hit = (r0 - 1.) < 0 if hit is None else np.asarray(hit, dtype=bool)
    nb = np.array(nbounce, dtype=np.int64)
    O.bounce_packets(X, r0, hit, cfg, np.asarray(ids, dtype=np.uint64), nb)
    return X


def unit(v):
    v = np.asarray(v, dtype=float)
    return v/np.linalg.norm(v, axis=-1, keepdims=True)


def step_to(side, centre, f):
    """A y = k 2^-54 whose impact longitude f(y) is the value next to ``centre`` on ``side`` (or
    ``centre`` itself for side 0).  The longitude is (atan2 + 2 pi) % 2 pi, so its values around a
    terminator are spaced by the doubles around 2.5 pi, and a run of k gives the same one: the
    middle of the run, where a last-bit difference in atan2 does not decide the rounding."""
    ks = sorted(range(-96, 97), key=abs)
    value = next(f(k*2.0**-54) for k in ks if np.sign(f(k*2.0**-54) - centre) == side)
    run = sorted(k for k in ks if f(k*2.0**-54) == value)
    assert run[0] > -96 and run[-1] < 96
    return run[len(run)//2]*2.0**-54


def edge_rows(unit_km):
    """(family, position, velocity) of the hand-made rows.  Velocity components that are exactly 0
    keep their position component through the move back to the surface (x + 0 t = x)."""
    rows = []
    v = 1.5/unit_km
    two_pi = 2*np.pi

    def lon_of(x, y):
        return (np.arctan2(x, -y) + two_pi) % two_pi

    # 1, 2: impact longitude on and next to the terminators on either side: moved back along x,
    # y and z kept
    for fam, sx, centre in ((1, 1.0, np.pi/2), (2, -1.0, 3*np.pi/2)):
        for side in (-1, 0, 1):
            for depth, lat in ((1e-3, 0.0), (1e-5, 0.6)):
                z = np.sin(lat)*(1 - depth)
                xs = sx*np.sqrt(1 - z*z)
                y = step_to(side, centre, lambda yy: lon_of(xs, yy))
                rows.append((fam, [sx*(1 - depth)*np.cos(lat), y, z], [-sx*v, 0.0, 0.0]))
    # 3: longitude 0 / 2 pi: x tiny of either sign, moved back along y
    for x in (0.0, 1e-300, -1e-300, 1e-17, -1e-17, 4e-16, -4e-16, 5e-16, -5e-16, 1e-15, -1e-15):
        rows.append((3, [x, -(1 - 2e-4), 0.0], [0.0, v, 0.0]))
    # 4: latitude +-(pi/2 - small)
    for small in (1e-3, 1e-5, 1e-7, 3e-8):
        for sz in (1.0, -1.0):
            for ang in (0.3, 2.0, 4.0):
                p = np.array([np.sin(small)*np.sin(ang), -np.sin(small)*np.cos(ang),
                              sz*np.cos(small)])*(1 - 1e-4)
                rows.append((4, p, -unit(p)*v))
                rows.append((4, p, [0.3*v, -0.2*v, -sz*v]))
    # 5: grazing: r^2 a few doubles under 1, velocity along the tangent, b^2 - 4ac from 1e-30 up
    for speed in (1e-7, 1e-6, 1e-5, 1e-4, 8e-4):
        for ulps in (1, 3, 40):
            for ang in (0.7, 2.9, 5.5):
                p = np.array([np.sin(ang)*np.cos(0.4), -np.cos(ang)*np.cos(0.4), np.sin(0.4)])
                p = p*(1 - ulps*1.2e-16)
                t = unit(np.cross(p, [0.3, 0.1, 1.0]))
                rows.append((5, p, t*speed))
    # 6: slow and deep: v_old2 < 0 before the clamp
    for speed_km in (0.01, 0.1, 0.5):
        for depth in (1e-2, 3e-2):
            for ang in (0.2, 3.0):
                p = np.array([np.sin(ang), -np.cos(ang), 0.2])
                p = unit(p)*(1 - depth)
                rows.append((6, p, -unit(p)*speed_km/unit_km))
    # 7: the sub-solar point, T = t0 + t1 = tx[nx-4] exactly; 8: the night side, T = t0 = tx[3]
    for depth in (1e-6, 1e-3, 2e-2):
        rows.append((7, [0.0, -(1 - depth), 0.0], [0.0, v, 0.0]))
        for ang in (np.pi, 2.0, 4.5):
            p = np.array([np.sin(ang)*np.cos(0.5), -np.cos(ang)*np.cos(0.5), np.sin(0.5)])
            rows.append((8, p*(1 - depth), -p*v))
    # 9: inside and moving outward
    for depth in (1e-6, 1e-3, 2e-2):
        for ang in (0.1, 1.0, 3.3, 5.0):
            p = np.array([np.sin(ang)*np.cos(-0.3), -np.cos(ang)*np.cos(-0.3), np.sin(-0.3)])
            rows.append((9, p*(1 - depth), unit(p + [0.2, -0.1, 0.3])*v))
    return rows
