"""tests/threshold_cases.py without a GPU: the two restatements themselves on its inputs, the
conditions that make the GPU tests on them meaningful, and the recorded numbers.

1. A scalar restatement of the camera pass and of the shell pass, written from the text of
   include/nexoclom_hip.h as a plain loop over Python floats (math.sqrt, math.atan2, one operation
   per line, independent of the NumPy code), gives the same pixel or cell, record, hidden, sunlit
   and kept flag for every sample of every case, and the same weights bit for bit.
2. Every bracket is two adjacent doubles (adjacent floats in the float32 cases) of one column; the
   named decision differs across it and the other decisions of the sample do not; every exact hit
   has the decided quantity equal to the threshold bit for bit; the numbers per threshold that the
   cases are to hold are there; the padding passes the guards of the guarded tests; the '/pairs'
   variants put the members of a bracket at lanes l and l + 32 of one wave, l in {0, 31}.
3. The recorded numbers.  First guess of bin_index, (int)((e_k - e_0) * (n / (e_n - e_0))), on the
   edges of np.linspace(-tan 25 deg, tan 25 deg, n + 1): wrong at 0 edges for n = 1, 2, 3; at 3 of
   8 for n = 7, 14 of 65 for n = 64, 47 of 1001 for n = 1000 and 2050 of 8193 for n = 8192 -- exact
   edge hits do run the fix-up loops.  A sample meant to sit one ulp inside the limb is not hidden:
   with o = (1, -4, 0) and p = (nextafter(1, 0), 3, 0), cz = 7 - 4 ulp rounds back to 7, so c2 == r2;
   thresholds are found by search, not written down.  Brackets per threshold over all cases (each
   again in the '/pairs' variant): u border 40, v border 32, u frame 8, v frame 8, dc>0 4 (oblique),
   b<r2 16 (12 axis-aligned at |o| = 1, 1.25, 1e3; 4 oblique), c2<r2 12 (8 axis-aligned at
   |o| = 1.25, 1e3; 4 oblique), b>0 8 (axis-aligned at |o| = 1, 1e3; never deciding, see
   tests/threshold_cases.py), w overflows 1, sunlit 4 + 4, mu edge 72 in float64 and 72 in float32,
   |mu|=1 16, altitude record 47; exact hits b == r2 16 and c2 == r2 6, found by the ulp walk."""
import bisect
import math

import numpy as np
import pytest

from tests import threshold_cases as T
from tests.camera_restatement import camera_image
from tests.shell_map_restatement import edges as shell_edges, shell_map
from tests.test_gpu_camera import tables

RTOL = 1e-11
PACKED = [name for name in T.CASES if not name.endswith('/pairs')]
RECORDED_MISSES = {1: 0, 2: 0, 3: 0, 7: 3, 64: 14, 1000: 47, 8192: 2050}
INF = float('inf')


# ---- 1. the scalar restatements ------------------------------------------------------------------------
def div(a, b):
    """a / b as IEEE-754 has it where Python raises"""
    if b != 0.0:
        return a/b
    if a != a or a == 0.0:
        return float('nan')
    return math.copysign(INF, a)*math.copysign(1.0, b)


def finite(v):
    return v == v and abs(v) != INF


def bin_of(v, edges):
    if not (v >= edges[0] and v <= edges[-1]):
        return -1
    if v == edges[-1]:
        return len(edges) - 2
    return bisect.bisect_right(edges, v) - 1


def g_sum(radvel, gt):
    gg = 0.0
    for k, (v_tab, g_tab) in enumerate(gt):
        v_tab, g_tab = [float(v) for v in v_tab], [float(g) for g in g_tab]
        if radvel != radvel:
            g = radvel
        elif radvel <= v_tab[0]:
            g = g_tab[0]
        elif radvel >= v_tab[-1]:
            g = g_tab[-1]
        else:
            j = bisect.bisect_right(v_tab, radvel) - 1
            slope = (g_tab[j + 1] - g_tab[j])/(v_tab[j + 1] - v_tab[j])
            g = slope*(radvel - v_tab[j]) + g_tab[j]
        gg = g if k == 0 else gg + g
    return gg


def is_sunlit(x, y, z):
    s = x*x
    t = z*z
    s = s + t
    return s > 1.0 + 2.0**-52 or y < 0.0


def scalar_camera(case):
    cam = case['camera']
    quantity, gt = tables(T.forces(), case['kind'])
    o = [float(v) for v in cam.o]
    C = [float(v) for v in np.asarray(cam.basis).reshape(9)]
    ue, ve = [float(v) for v in cam.uedges], [float(v) for v in cam.vedges]
    vrplanet, area = float(T.forces().vrplanet), float(cam.area)
    out = []
    for x, y, z, vy, frac in zip(*(c.astype(np.float64).tolist() for c in case['cols'])):
        # 1
        dx = x - o[0]
        dy = y - o[1]
        dz = z - o[2]
        radvel = vy + vrplanet
        xc = (C[0]*dx + C[1]*dy) + C[2]*dz
        dc = (C[3]*dx + C[4]*dy) + C[5]*dz
        zc = (C[6]*dx + C[7]*dy) + C[8]*dz
        # 2, 3
        ix = iz = -1
        if dc > 0.0:
            u = div(xc, dc)
            v = div(zc, dc)
            ix = bin_of(u, ue)
            iz = bin_of(v, ve)
        if ix < 0 or iz < 0:
            bad = (not finite(frac)) or radvel != radvel
            out.append((-1, False, False, False, 0.0, bad))
            continue
        pix = ix*(len(ve) - 1) + iz
        # 4
        r2 = (dx*dx + dy*dy) + dz*dz
        b = -((o[0]*dx + o[1]*dy) + o[2]*dz)
        cx = o[1]*z - o[2]*y
        cy = o[2]*x - o[0]*z
        cz = o[0]*y - o[1]*x
        c2 = (cx*cx + cy*cy) + cz*cz
        hidden = b > 0.0 and b < r2 and c2 < r2
        f = frac*0.0 if hidden else frac
        # 5, 6
        lit = True
        if quantity == 'radiance':
            lit = is_sunlit(x, y, z)
            if not lit:
                f = f*0.0
            w = f*g_sum(radvel, gt)
            w = w/1e6
        else:
            w = f
        if not finite(w) or radvel != radvel:
            out.append((pix, hidden, lit, False, 0.0, True))
            continue
        # 7
        r = math.sqrt(r2)
        foot = dc*dc
        foot = foot*dc
        foot = div(foot, r)
        w = div(w, foot*area)
        # 8
        out.append((pix, hidden, lit, finite(w), w, not finite(w)))
    return out


def scalar_shell(case):
    quantity, gt = tables(T.forces(), case['kind'])
    nlon, nlat = case['grid']
    r_lo, r_hi, nalt = case['alt']
    le, me = ([float(v) for v in e] for e in shell_edges(nlon, nlat))
    inv_dr = float(nalt)/(float(r_hi) - float(r_lo))
    vrplanet = float(T.forces().vrplanet)
    out = []
    for x, y, z, vy, frac in zip(*(c.astype(np.float64).tolist() for c in case['cols'])):
        # 1
        radvel = vy + vrplanet
        r2 = (x*x + y*y) + z*z
        r = math.sqrt(r2)
        mu = div(z, r)
        # 2
        lon = math.atan2(x, -y)
        if lon < 0.0:
            lon = lon + 2*math.pi
        # 3
        ix = bin_of(lon, le)
        iz = bin_of(mu, me)
        if ix < 0 or iz < 0:
            bad = (not finite(frac)) or radvel != radvel
            out.append((-1, -1, False, False, 0.0, 0.0, bad))
            continue
        cell = ix*nlat + iz
        # 4, 5
        f = frac
        lit = True
        if quantity == 'radiance':
            lit = is_sunlit(x, y, z)
            if not lit:
                f = f*0.0
            w = f*g_sum(radvel, gt)
            w = w/1e6
        else:
            w = f
        if not finite(w) or radvel != radvel:
            out.append((cell, -1, lit, False, 0.0, 0.0, True))
            continue
        # 6
        c = div(w, r2)
        if not finite(c):
            out.append((cell, -1, lit, False, 0.0, 0.0, True))
            continue
        # 8
        k = -1
        if w != 0.0:
            t = (r - r_lo)*inv_dr
            if t < 0.0:
                k = 0
            elif t < float(nalt):
                k = 1 + int(t)
            else:
                k = nalt + 1
        out.append((cell, k, lit, True, w, c, False))
    return out


@pytest.mark.parametrize('name', PACKED)
def test_scalar_restatement_agrees(name):
    case = T.CASES[name]()
    res, d = T.restate(case)
    if case['family'] == 'camera':
        rows = scalar_camera(case)
        pix, hidden, lit, keep, w, bad = (np.array(col) for col in zip(*rows))
        located = d['located']
        assert np.array_equal(pix >= 0, located)
        assert np.array_equal(pix[located], d['pix'][located])
        assert np.array_equal(hidden[located], d['hidden'][located])
        assert np.array_equal(lit[located], d['sunlit'][located])
        assert np.array_equal(keep, d['keep'])
        assert np.array_equal(w[keep].view(np.int64), d['w'][keep].view(np.int64))
    else:
        rows = scalar_shell(case)
        cell, k, lit, keep, w, c, bad = (np.array(col) for col in zip(*rows))
        located = d['located']
        assert np.array_equal(cell >= 0, located)
        assert np.array_equal(cell[located], d['cell'][located])
        assert np.array_equal(lit[located], d['sunlit'][located])
        assert np.array_equal(keep, d['keep'])
        assert np.array_equal(k[keep], d['k'][keep])
        assert np.array_equal(w[keep].view(np.int64), d['w'][keep].view(np.int64))
        assert np.array_equal(c[keep].view(np.int64), d['c'][keep].view(np.int64))
    assert int(bad.sum()) == res.nonfinite == d['nonfinite']
    assert int(keep.sum()) == res.binned == res.counts.sum()
    assert res.samples == len(case['cols'][0])


# ---- 2. the conditions -----------------------------------------------------------------------------------
def decisions(case, d):
    """{name: array} of everything a sample's result hangs on"""
    if case['family'] == 'camera':
        with np.errstate(invalid='ignore'):
            out = {k: d[k] for k in ('front', 'ix', 'iz', 'located', 'hidden', 'sunlit', 'keep')}
            where = d['located']                        # step 4 is taken by located samples only
            out.update({'b>0': where & (d['b'] > 0), 'b<r2': where & (d['b'] < d['r2']),
                        'c2<r2': where & (d['c2'] < d['r2'])})
        return out
    out = {k: d[k] for k in ('ix', 'iz', 'sunlit', 'keep', 'filed', 'k')}
    with np.errstate(invalid='ignore'):
        out['|mu|<1'] = np.abs(d['mu']) < 1
    return out


# what else may (and, where it can be read off a result, must) move with the named decision
FOLLOWS = {('camera', 'b<r2'): {'hidden'}, ('camera', 'c2<r2'): {'hidden'},
           ('camera', 'front'): {'ix', 'iz'}, ('shell', 'sunlit'): {'filed', 'k'},
           ('camera', 'ix'): {'located', 'keep'}, ('camera', 'iz'): {'located', 'keep'}}    # the frame


@pytest.mark.parametrize('name', list(T.CASES))
def test_brackets_and_hits(name):
    case = T.CASES[name]()
    res, d = T.restate(case)
    cols = np.array([c.astype(np.float64) for c in case['cols']])
    narrow = np.array(case['cols'])
    dec = decisions(case, d)
    for ia, ib, label, which in case['brackets']:
        same = (cols[:, ia] == cols[:, ib]) | (np.isnan(cols[:, ia]) & np.isnan(cols[:, ib]))
        differ = np.flatnonzero(~same)
        assert len(differ) == 1, (label, ia, ib)
        a, b = narrow[differ[0], ia], narrow[differ[0], ib]
        assert a.dtype == case['dtype'] and np.nextafter(a, b) == b and a != b, (label, a, b)
        assert dec[which][ia] != dec[which][ib], (label, ia, ib)
        free = FOLLOWS.get((case['family'], which), set()) | {which}
        if case['family'] == 'camera' and dec['located'][ia] != dec['located'][ib]:
            assert which in ('ix', 'iz')                # a frame border: step 4 is taken on one side only
            free |= {'b>0', 'b<r2', 'c2<r2', 'hidden'}
        for other, values in dec.items():
            if other not in free:
                assert values[ia] == values[ib], (label, other, ia, ib)
        if which in ('b<r2', 'c2<r2'):
            rest = {'b>0', 'b<r2', 'c2<r2'} - {which}
            assert all(dec[o][ia] and dec[o][ib] for o in rest), label
            assert dec['hidden'][ia] != dec['hidden'][ib] and dec['located'][ia] and dec['located'][ib]
        if which == 'b>0':
            assert dec['b<r2'][ia] and dec['b<r2'][ib] and dec['located'][ia] and dec['located'][ib]
            assert not (dec['c2<r2'][ia] or dec['c2<r2'][ib] or dec['hidden'][ia] or dec['hidden'][ib])
        if which == 'front':
            assert not (dec['located'][ia] or dec['located'][ib])
    for i, label, quantity, value in case['hits']:
        assert d[quantity][i] == value, (label, i, d[quantity][i], value)
    # every threshold sample of the camera's edge cases is where it was meant to be: dc = 1, u = x, v = z
    if name.startswith(('cam_u_', 'cam_v_')):
        own = np.array([i for i, _ in case['marks']])
        assert np.all(d['dc'][own] == 1.0)
        assert np.array_equal(d['u'][own], cols[0, own]) and np.array_equal(d['v'][own], cols[2, own])
        n = int(name.split('_')[2].split('/')[0])
        assert len(case['hits']) == n + 1 and len(case['marks']) == 3*(n + 1)
        outside = own[~d['located'][own]]
        assert len(outside) == 2                        # one ulp below the first edge, one above the last
    # the padding passes the guards of the guarded tests
    pad = tuple(c[case['padding']] for c in case['cols'])
    quantity, gt = tables(T.forces(), case['kind'])
    assert len(pad[0]) >= 300 and len(pad[0]) + case['n_threshold'] == len(cols[0]) <= 25000
    if case['family'] == 'camera':
        cam = case['camera']
        guards = camera_image(*pad, cam.o, cam.basis, cam.uedges, cam.vedges, T.forces().vrplanet, cam.area,
                              quantity, gt)[4:6]
    else:
        guards = shell_map(*pad, T.forces().vrplanet, quantity, gt, *case['grid'], *case['alt'])[7:10]
    assert min(guards) >= T.GUARD
    # the arrangement in the wave
    if name.endswith('/pairs'):
        pairs = set(case['pairs'])
        assert all((ia, ib) in pairs for ia, ib, *_ in case['brackets'])
        for q, (i, j) in enumerate(case['pairs']):
            assert i//64 == j//64 == q and j % 64 == i % 64 + 32 and i % 64 == (0 if q % 2 == 0 else 31)
        twin = T.CASES[name[:-len('/pairs')]]()
        for mine, theirs in zip(case['cols'], twin['cols']):
            assert np.array_equal(np.sort(mine.view(np.uint64 if mine.itemsize == 8 else np.uint32)),
                                  np.sort(theirs.view(np.uint64 if mine.itemsize == 8 else np.uint32)))


def brackets_of(names, label):
    return sum(T.tally(T.CASES[name]()).get(label, [0, 0])[0] for name in names)


def test_the_numbers_per_threshold():
    for cam in ('oblique', 'horizon'):
        for width in ('f64', 'f32'):
            tally = T.tally(T.CASES[f'cam_borders_{cam}_{width}']())
            assert tally['u border'][0] >= 8 and tally['v border'][0] >= 8
            assert tally['u frame'][0] == 2 and tally['v frame'][0] == 2
    assert T.tally(T.CASES['cam_borders_oblique_f64']())['dc>0'][0] >= 4
    axis = ['cam_hidden_axis_1', 'cam_hidden_axis_1.25', 'cam_hidden_axis_1e3']
    for label in ('b<r2', 'c2<r2'):
        assert brackets_of(axis, label) >= 4 and brackets_of(['cam_hidden_oblique'], label) >= 4
    assert brackets_of(['cam_hidden_axis_1'], 'b<r2') >= 1
    assert brackets_of(['cam_hidden_axis_1e3'], 'b<r2') >= 1
    assert brackets_of(['cam_hidden_axis_1e3'], 'c2<r2') >= 1
    assert np.linalg.norm(T.CASES['cam_hidden_axis_1']()['camera'].o) == 1.0
    assert np.linalg.norm(T.CASES['cam_hidden_axis_1e3']()['camera'].o) == 1e3
    assert brackets_of(['cam_hidden_b_axis_1', 'cam_hidden_b_axis_1e3'], 'b>0') >= 4
    for name in axis + ['cam_hidden_oblique']:          # where `<` and `<=` part
        assert T.tally(T.CASES[name]())['b=r2'][1] >= 1
    assert sum(T.tally(T.CASES[name]()).get('c2=r2', [0, 0])[1]
               for name in axis + ['cam_hidden_oblique']) >= 2
    assert brackets_of(['cam_front_finite'], 'w overflows') == 1
    assert brackets_of(['cam_sunlit'], 'sunlit') >= 1 and brackets_of(['shell_sunlit'], 'sunlit') >= 1
    for nlat in (2, 3, 7, 64):
        for width in ('f64', 'f32'):
            assert brackets_of([f'shell_mu_{nlat}_{width}'], 'mu edge') == nlat - 1
        assert T.tally(T.CASES[f'shell_mu_{nlat}_f64']())['|mu|=1'] == [4, 4]
    for nlat in (2, 4, 7):
        assert T.tally(T.CASES[f'shell_mu_hits_{nlat}']())['mu edge'][1] == nlat - 1
    for label, nalt in (('1', 1), ('5', 5), ('33', 33), ('narrow', 4)):
        case = T.CASES[f'shell_alt_{label}']()
        assert T.tally(case)['altitude record'][0] == nalt + 1       # t = 0, the interior integers, t = nalt
        assert len(case['hits']) == 4
    assert T.CASES['shell_alt_narrow']()['alt'] == (2.0, 2.0625, 4)


def test_first_guess_of_bin_index_misses_on_exact_edges():
    misses = T.edge_misses()
    print({n: f'{missed} of {of}' for n, (missed, of) in misses.items()})
    assert {n: missed for n, (missed, _) in misses.items()} == RECORDED_MISSES
    assert all(misses[n][0] >= 1 for n in (7, 64, 1000, 8192))
    for axis in 'uv':                                   # and the cases hold exactly those edges
        for n in T.EDGE_COUNTS:
            cam = T.CASES[f'cam_{axis}_{n}']()['camera']
            e = cam.uedges if axis == 'u' else cam.vedges
            assert np.array_equal(e, np.linspace(-T.TAN25, T.TAN25, n + 1))
            assert len(cam.vedges if axis == 'u' else cam.uedges) - 1 not in (n, 0)


def test_nice_coordinates_are_a_trap():
    """One ulp inside the limb by geometry, not hidden by the arithmetic."""
    o, p = (1.0, -4.0, 0.0), (float(np.nextafter(1.0, 0.0)), 3.0, 0.0)
    cz = o[0]*p[1] - o[1]*p[0]
    assert cz == 7.0
    cam = T.axis_camera(o, half=(2.0, 2.0))
    d = T.cam_eval(cam, 'column', [p])
    assert d['c2'][0] == d['r2'][0] and not d['hidden'][0]


def test_the_camera_front_and_finiteness_case():
    case = T.CASES['cam_front_finite']()
    res, d = T.restate(case)
    by_name = {}
    for i, label in case['marks']:
        by_name.setdefault(label, []).append(i)
    dc_hits = by_name['dc=+-0, +-5e-324']
    assert [bool(v) for v in d['located'][dc_hits]] == [False, False, True, False, False]
    assert not d['keep'][dc_hits].any()
    for label, located, kept in (('boresight dc=5e-324', True, False), ('boresight dc=1e-150', True, False),
                                 ('boresight dc=1e-100', True, True)):
        i = by_name[label][0]
        assert d['located'][i] == located and d['keep'][i] == kept
    w = d['w'][by_name['boresight dc=1e-100'][0]]
    assert 0.999e200 < w < 1.001e200
    a, b = by_name['w overflows']
    assert d['keep'][a] and not d['keep'][b] and d['w'][b] == np.inf and d['w'][a] > 1e308
    for where, located in (('inside', True), ('outside', False), ('behind', False)):
        for what in ('frac', 'vy'):
            i = by_name[f'{what}=NaN {where}'][0]
            assert d['located'][i] == located and not d['keep'][i]
    # 5e-324 twice, 1e-150, the upper member of the bracket, and the six NaN samples
    assert res.nonfinite == 10 and d['keep'][case['padding']].sum() == res.binned - 2


def test_the_sunlit_cases():
    for name in ('cam_sunlit', 'shell_sunlit'):
        case = T.CASES[name]()
        res, d = T.restate(case)
        own = np.array([i for i, _ in case['marks']])
        if name == 'cam_sunlit':
            assert d['located'][own].all() and not d['hidden'][own].any()
        hits = np.array([i for i, *_ in case['hits']])
        assert [bool(v) for v in d['sunlit'][hits]] == [False, False, True, False, True, True, True, True]
        assert set(d['s'][hits]) == {1.0 + 2.0**-52, 1.0 + 2.0**-51}
        # a lit sample weighs enough in its pixel or cell to be missed
        sums = res.image.ravel() if name == 'cam_sunlit' else res.column.ravel()
        where = d['pix'] if name == 'cam_sunlit' else d['cell']
        value = d['w'] if name == 'cam_sunlit' else d['c']
        lit = own[d['sunlit'][own]]
        assert np.all(value[lit] > 1e-6*sums[where[lit]])


def test_a_wrong_hidden_flag_or_record_would_show():
    for name in T.CAMERA_CASES:
        if 'hidden' in name:
            case = T.CASES[name]()
            res, d = T.restate(case)
            for ia, ib, label, which in case['brackets']:
                if which != 'b>0':
                    seen = ia if not d['hidden'][ia] else ib
                    assert d['w'][seen] > 1e-6*res.image.ravel()[d['pix'][seen]] > 0
            for i, label, quantity, value in case['hits']:
                # equality: not hidden, by that inequality alone, and seen in its pixel
                other = d['c2'][i] < d['r2'][i] if quantity == 'b_r2' else d['b'][i] < d['r2'][i]
                assert d[quantity][i] == 0.0 and d['b'][i] > 0 and other and not d['hidden'][i]
                assert d['located'][i] and d['w'][i] > 1e-6*res.image.ravel()[d['pix'][i]] > 0
    for name in T.SHELL_CASES:
        if name.startswith('shell_alt'):
            case = T.CASES[name]()
            res, d = T.restate(case)
            per_cell = res.abs_sums[0, ..., 0].reshape(-1, res.abs_sums.shape[3])
            r_lo, r_hi, nalt = case['alt']
            hits = [i for i, *_ in case['hits']]          # r_lo - 1 ulp, r_lo, r_hi - 1 ulp, r_hi
            assert list(d['r'][hits]) == [np.nextafter(r_lo, 0), r_lo, np.nextafter(r_hi, 0), r_hi]
            assert d['t'][hits[1]] == 0.0 and d['t'][hits[3]] == nalt and d['t'][hits[0]] < 0
            assert list(d['k'][hits]) == [0, 1, nalt, nalt + 1]
            for i, _ in case['marks']:
                # moved to a neighbouring record it changes both by w, far above RTOL * sum |term|
                assert d['filed'][i] and d['w'][i] > 1e6*RTOL*per_cell[d['cell'][i]].sum()


@pytest.mark.parametrize('nlon', [1, 3, 5])
def test_longitudes_do_not_hang_on_the_last_bit_of_atan2(nlon):
    case = T.CASES[f'shell_lon_{nlon}']()
    res, d = T.restate(case)
    lon_edges = shell_edges(nlon, 3)[0]
    want = {'lon=+-0': (0, 0.0), 'lon=-tiny+2pi': (nlon - 1, lon_edges[-1]), 'lon=pi': (None, np.pi),
            'lon=pi/2 or 3pi/2': (None, None), 'pole': (None, None)}
    for i, label in case['marks']:
        if label.startswith('centre'):
            assert np.isnan(d['mu'][i]) and not d['located'][i]
            continue
        ix, lon = want[label]
        assert d['located'][i] and d['keep'][i]
        if ix is not None:
            assert d['ix'][i] == ix and d['lon'][i] == lon        # the seam: exact by Annex F
        elif d['lon'][i] == 0.0:                                  # a pole with atan2(+-0, +0) = +-0
            assert label == 'pole' and d['ix'][i] == 0
        else:
            assert np.min(np.abs(d['lon'][i] - lon_edges[1:-1]), initial=np.inf) >= 1e-3
            assert 1e-3 < d['lon'][i] < 2*np.pi - 1e-3
        if label == 'pole':
            assert abs(d['mu'][i]) == 1.0 and d['iz'][i] in (0, 2) and d['lon'][i] in (0.0, np.pi)
    assert res.nonfinite == 1 and res.binned == res.samples - 2
