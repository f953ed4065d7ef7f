"""Inputs that sit ON the decision thresholds of the camera pass and of the shell pass, built without
a GPU and without a library call, from the arithmetic of tests/camera_restatement.py and
tests/shell_map_restatement.py alone.  The guarded tests (tests/test_gpu_camera.py,
tests/test_gpu_shell_map.py, ...) keep every sample 1e-9 away from every threshold; the cases here
do the opposite, and tests/test_gpu_camera_thresholds.py / tests/test_gpu_shell_thresholds.py hold
the kernels to the restatements exactly on them.

Two constructions:

* ``bracket(decision, lo, hi)`` bisects on the integer ordering of the doubles (or of the float32
  values, widened exactly) between ``lo`` and ``hi`` and returns two ADJACENT values at which
  ``decision`` differs.  ``decision(values)`` puts the values into one coordinate of fixed samples
  and evaluates the restatement (many brackets are bisected at once, one per array element).  A
  kernel that moves the decided quantity by one rounding puts one of the two samples on the other
  side.  A search that cannot succeed raises.
* exact hits: samples whose decided quantity equals the threshold bit for bit, with the two
  nextafter neighbours of the input coordinate; placed where the arithmetic is exact, or found by
  walking one coordinate by ulps (``walk_to``).

Nothing is written down from geometry: every threshold sample is found on, or verified against, the
restatement (tests/test_threshold_cases_cpu.py repeats every condition as an assertion).

Every bracket walks ONE input coordinate, the others fixed, so that its two members are adjacent
doubles of one column.  Where the issue of a decision is a direction in space (the boresight, the
radius) the coordinate that moves the decided quantity most is walked.

Findings about what can be placed at all, and about what no input can tell apart:

* ``b > 0`` can never be the deciding inequality of ``hidden``.  c2 = |o x p|^2 = |o|^2 r2 - b^2,
  so at b = 0 (to within its own sign) c2 >= r2 whenever |o| >= 1, which nxc_camera_set demands:
  the third inequality fails wherever the first is on its threshold; at |o| = 1 exactly the two
  sides are the same rounded sum (c2 == r2).  The 'b>0' brackets are therefore brackets of the
  sign of b with ``b < r2`` true and ``c2 < r2`` false on both sides (asserted), and the sample is
  not hidden on either side: they pin that a kernel does not hide a sample from the first two
  inequalities alone.  A camera that has the planet in view (the 'oblique' one) has b = 0 at right
  angles to it, outside the frame, so those brackets come from axis-aligned cameras that look
  past the planet.  ``c2 < r2`` cannot decide from |o| = 1 either (c2 - r2 = -dc^2 there); its
  axis-aligned brackets are taken from |o| = 1.25 and 1e3, those of ``b < r2`` from 1, 1.25, 1e3.
* A bracket tells a moved quantity, not ``<`` from ``<=``: the cases of ``hidden`` therefore also
  hold samples with b == r2 and with c2 == r2 bit for bit, found by the ulp walk.
* ``dc > 0`` of the 'oblique' camera is bracketed through the camera position along y; no
  coordinate axis lies inside its field of view, so on the positive side u is outside the frame and
  neither member is binned.  The thresholds of ``dc`` that show in a result are the axis-aligned
  ones (dc = 5e-324 is located and then dropped as non-finite, -5e-324 and +-0 are not located).
  ``dc >= 0`` in the kernel would change no result at all: at dc = +-0 u and v are NaN or infinite
  and the sample is outside the frame either way, with the same ``nonfinite`` rule.
* ``t <= nalt`` in step 8 of the shell pass would change no result either: at t == nalt it gives
  1 + (int)t = nalt + 1, the record the definition names.  r = r_hi (t == nalt exactly, asserted) is
  in the cases all the same, with its neighbour one ulp below in record nalt.

An entry of CASES is a function without arguments that returns a dict: ``family`` ('camera' or
'shell'), ``cols`` (x y z vy frac, float64 or float32), ``camera`` (a tests.test_gpu_camera.Camera)
or ``grid`` and ``alt``, ``kind`` (the g-value tables of ``tables``), ``marks`` [(sample index,
threshold name)], ``brackets`` [(index a, index b, name, decision)], ``hits`` [(index, name,
quantity, value)], ``n_threshold`` (the samples that are not padding) and ``padding`` (the indices
of the guarded filler samples).  Every case exists twice: '<name>' holds the threshold samples in
front of the padding; '<name>/pairs' holds the two members of bracket q (and an exact hit and its
lower neighbour) at lanes l and l + 32 of wave q, l = 0 for even q and 31 for odd q, the lanes
image_add_pairs and add_record_pairs pair (a sample's index is its wave * 64 + lane).

``python -m tests.threshold_cases`` prints, per case, the brackets and exact hits per threshold and
the edges at which the first guess of bin_index is wrong."""
import functools

import numpy as np

from tests import helpers as H
from tests.camera_restatement import camera_image, camera_samples
from tests.shell_map_restatement import edges as shell_edges, shell_map, shell_samples
from tests.test_gpu_camera import Camera, camera as named_camera, cloud as camera_cloud, tables
from tests.test_gpu_pixel_moments import cloud as seven_cloud

GUARD = 1e-9
TINY = 5e-324
TAN25 = np.tan(np.radians(25.0))
EDGE_COUNTS = (1, 2, 3, 7, 64, 1000, 8192)


@functools.lru_cache(maxsize=None)
def forces():
    return H.mercury_forces('Na', 1.3)


# ---- adjacent values -------------------------------------------------------------------------------
def _keys(v, dtype):
    """Order-preserving integers of the values of ``dtype`` (+0 and -0 share key 0)."""
    it, low = (np.int64, -2**63) if dtype == np.float64 else (np.int32, -2**31)
    i = np.asarray(v, dtype=dtype).view(it).astype(np.int64)
    return np.where(i >= 0, i, low - i)


def _values(k, dtype):
    k = np.asarray(k, dtype=np.int64)
    if dtype == np.float64:
        return np.where(k >= 0, k, -2**63 - k).view(np.float64)
    return np.where(k >= 0, k, -2**31 - k).astype(np.int32).view(np.float32).astype(np.float64)


def bracket(decision, lo, hi, dtype=np.float64):
    """Arrays (a, b): adjacent values of ``dtype`` (as float64) between lo and hi, a on lo's side,
    with decision(a) == decision(lo) != decision(b) == decision(hi), element by element."""
    lo, hi = np.atleast_1d(np.asarray(lo, dtype=dtype)), np.atleast_1d(np.asarray(hi, dtype=dtype))
    ka, kb = _keys(lo, dtype), _keys(hi, dtype)
    da, db = decision(_values(ka, dtype)), decision(_values(kb, dtype))
    if np.any(da == db):
        raise ValueError(f'bracket: the decision is the same at both ends for {np.flatnonzero(da == db)}')
    def far():                                          # (kb - ka overflows between -40 and 40)
        return (kb > ka + 1) | (ka > kb + 1)
    while np.any(far()):
        mid = np.where(far(), ka//2 + kb//2 + ((ka & 1) + (kb & 1))//2, ka)
        same = decision(_values(mid, dtype)) == da
        ka, kb = np.where(same, mid, ka), np.where(same | ~far(), kb, mid)
    a, b = _values(ka, dtype), _values(kb, dtype)
    if np.any(decision(a) != da) or np.any(decision(b) != db) or np.any(a == b):
        raise ValueError('bracket: the search did not end on two adjacent values that differ')
    return a, b


def walk_to(quantity, target, start, reach=4096):
    """The double nearest ``start`` (by ulps, at most ``reach`` away) at which quantity(value) ==
    target bit for bit; raises when there is none."""
    k0 = int(_keys(start, np.float64))
    ks = k0 + np.concatenate([[0], np.ravel([(s, -s) for s in range(1, reach + 1)])])
    vals = _values(ks, np.float64)
    ok = np.flatnonzero(quantity(vals) == target)
    if not len(ok):
        raise ValueError(f'walk_to: {target!r} is not reached within {reach} ulps of {start!r}')
    return float(vals[ok[0]])


def neighbours(v, dtype=np.float64):
    """(the value below, v, the value above) in ``dtype``"""
    v = dtype(v)
    return float(np.nextafter(v, dtype(-np.inf))), float(v), float(np.nextafter(v, dtype(np.inf)))


def first_guess_misses(edges):
    """Edges e_k at which bin_index's first guess (int)((e_k - e_0) * inv_step), inv_step = n /
    (e_n - e_0), clamped to n - 1, is not the bin of e_k."""
    n = len(edges) - 1
    inv_step = np.float64(n)/(edges[n] - edges[0])
    guess = np.minimum(((edges - edges[0])*inv_step).astype(np.int64), n - 1)
    return int(np.sum(guess != np.minimum(np.arange(n + 1), n - 1)))


# ---- the two restatements on positions ---------------------------------------------------------------
def cam_eval(cam, kind, P, vy=0.003, frac=0.5):
    quantity, gt = tables(forces(), kind)
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    one = np.ones(len(P))
    return camera_samples(P[:, 0], P[:, 1], P[:, 2], vy*one, frac*one, cam.o, cam.basis, cam.uedges,
                          cam.vedges, forces().vrplanet, cam.area, quantity, gt)


def shell_eval(grid, alt, kind, P, vy=0.003, frac=0.5):
    quantity, gt = tables(forces(), kind)
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    one = np.ones(len(P))
    return shell_samples(P[:, 0], P[:, 1], P[:, 2], vy*one, frac*one, forces().vrplanet, quantity, gt,
                         *grid, *alt)


def bracket_coordinate(evaluate, decide, P, coord, lo, hi, dtype=np.float64):
    """One bracket per row of P (m, 3): coordinate ``coord`` of every row walks between lo and hi
    (scalars or (m,)), decide(evaluate(positions)) is the decision.  Returns the two (m, 3) arrays."""
    P = np.array(P, dtype=dtype).astype(np.float64).reshape(-1, 3)

    def put(values):
        Q = P.copy()
        Q[:, coord] = values
        return Q

    lo, hi = np.broadcast_to(lo, len(P)), np.broadcast_to(hi, len(P))
    a, b = bracket(lambda values: decide(evaluate(put(values))), lo, hi, dtype)
    return put(a), put(b)


# ---- a case under construction -----------------------------------------------------------------------
class Build:
    def __init__(self, seed, dtype=np.float64):
        self.rng, self.dtype = np.random.default_rng(seed), dtype
        self.rows, self.marks, self.brackets, self.hits, self.pairs = [], [], [], [], []

    def add(self, p, name, vy=None, frac=None):
        vy = self.rng.uniform(-0.02, 0.02) if vy is None else vy
        frac = self.rng.uniform(0.25, 1.0) if frac is None else frac
        self.rows.append((p[0], p[1], p[2], vy, frac))
        self.marks.append((len(self.rows) - 1, name))
        return len(self.rows) - 1

    def bracket(self, A, B, name, decision):
        """rows of A and B (m, 3) are the members of m brackets of ``decision``"""
        for a, b in zip(np.atleast_2d(A), np.atleast_2d(B)):
            vy, frac = self.rng.uniform(-0.02, 0.02), self.rng.uniform(0.25, 1.0)
            ia, ib = self.add(a, name, vy, frac), self.add(b, name, vy, frac)
            self.brackets.append((ia, ib, name, decision))
            self.pairs.append((ia, ib))

    def hit(self, p, coord, name, quantity, value, sides=True):
        """p is an exact hit of ``quantity`` == value; its neighbours along ``coord`` go with it"""
        below, _, above = neighbours(p[coord])
        i = self.add(p, name)
        self.hits.append((i, name, quantity, value))
        if sides:
            lower, upper = np.array(p, dtype=np.float64), np.array(p, dtype=np.float64)
            lower[coord], upper[coord] = below, above
            self.pairs.append((self.add(lower, name + ' -1ulp'), i))
            self.add(upper, name + ' +1ulp')
        return i

    def columns(self):
        cols = np.array(self.rows, dtype=np.float64).reshape(-1, 5).T
        narrow = cols.astype(self.dtype)
        with np.errstate(invalid='ignore'):
            exact = (narrow[:3].astype(np.float64) == cols[:3]) | np.isnan(cols[:3])
        if not exact.all():
            raise ValueError('a threshold position is not a value of the case\'s type')
        return narrow


def _finish(build, family, kind, padding, arrangement, **scene):
    """Threshold samples + padding, in the order of ``arrangement``."""
    own = build.columns()
    T = own.shape[1]
    cols = np.concatenate([own, np.array([np.asarray(c, dtype=build.dtype) for c in padding])], axis=1)
    N = cols.shape[1]
    order = np.arange(N)
    members = {(i, j) for i, j, *_ in build.brackets}      # the brackets first: each gets a wave
    build.pairs.sort(key=lambda pair: pair not in members)
    if arrangement == 'pairs':
        slots = np.full(N, -1)
        taken = np.zeros(N, dtype=bool)
        for q, (i, j) in enumerate(build.pairs[:N//64]):
            lane = 0 if q % 2 == 0 else 31
            slots[q*64 + lane], slots[q*64 + lane + 32] = i, j
            taken[[i, j]] = True
        slots[slots < 0] = np.flatnonzero(~taken)
        order = slots
    where = np.empty(N, dtype=np.int64)
    where[order] = np.arange(N)
    cols = tuple(np.ascontiguousarray(c[order]) for c in cols)
    return dict(family=family, kind=kind, cols=cols, dtype=build.dtype, n_threshold=T,
                marks=[(int(where[i]), name) for i, name in build.marks],
                brackets=[(int(where[i]), int(where[j]), name, dec) for i, j, name, dec in build.brackets],
                hits=[(int(where[i]), name, q, v) for i, name, q, v in build.hits],
                pairs=[(int(where[i]), int(where[j])) for i, j in build.pairs[:N//64]]
                if arrangement == 'pairs' else [],
                padding=np.sort(where[T:]), **scene)


def _n_padding(build):
    """A few hundred, and enough waves for every bracket to have one of its own (at most 400)."""
    T = len(build.rows)
    return max(300, 64*min(len(build.brackets) + 1, 400) - T)


def camera_padding(cam, kind, n, seed, dtype):
    """n guarded samples of tests/test_gpu_camera.py's cloud() (without its five placed ones)."""
    quantity, gt = tables(forces(), kind)
    for s in range(seed, seed + 50):
        cols = tuple(c[5:] for c in camera_cloud(cam, n + 5, s, dtype))
        res = camera_image(*cols, cam.o, cam.basis, cam.uedges, cam.vedges, forces().vrplanet, cam.area,
                           quantity, gt)
        if res.edge_guard >= GUARD and res.margin_guard >= GUARD:
            return cols
    raise ValueError('no guarded padding found')


def shell_padding(grid, alt, kind, n, seed, dtype):
    """n guarded samples of tests/test_gpu_shell_map.py's five(cloud())."""
    quantity, gt = tables(forces(), kind)
    for s in range(seed, seed + 50):
        seven = seven_cloud(n, s, dtype)
        cols = tuple(seven[k] for k in (0, 1, 2, 4, 6))
        res = shell_map(*cols, forces().vrplanet, quantity, gt, *grid, *alt)
        if min(res.edge_guard, res.margin_guard, res.bin_guard) >= GUARD:
            return cols
    raise ValueError('no guarded padding found')


def camera_case(build, cam, kind, arrangement, seed):
    pad = camera_padding(cam, kind, _n_padding(build), seed, build.dtype)
    return _finish(build, 'camera', kind, pad, arrangement, camera=cam)


def shell_case(build, grid, alt, kind, arrangement, seed):
    pad = shell_padding(grid, alt, kind, _n_padding(build), seed, build.dtype)
    return _finish(build, 'shell', kind, pad, arrangement, grid=tuple(grid), alt=tuple(alt))


# ---- cameras -----------------------------------------------------------------------------------------
def axis_camera(o, half=(TAN25, TAN25), dims=(3, 3)):
    """Right = x, boresight = y, up = z exactly; pix_area_cm2 = 1."""
    cam = Camera(o, (0, 1, 0), (0, 0, 1), (50, 50), dims)
    assert np.array_equal(cam.basis, np.eye(3))
    cam.uedges = np.linspace(-half[0], half[0], dims[0] + 1)
    cam.vedges = np.linspace(-half[1], half[1], dims[1] + 1)
    cam.area = 1.0
    return cam


def cam_front_finite(arrangement):
    """Steps 2 and 6 to 8 with a camera at (2, 0, 0): dc is the sample's own y."""
    cam = axis_camera((2.0, 0.0, 0.0))
    B = Build(201)
    for dc in (0.0, -0.0, TINY, -TINY):
        B.hit((2.0, dc, 0.0), 1, 'dc=+-0, +-5e-324', 'dc', dc, sides=False)
    B.hit((2.0, 0.0, 0.0), 1, 'dc=+-0, +-5e-324', 'dc', 0.0, sides=False)
    for dc in (TINY, 1e-150, 1e-100):                  # located; the first two weigh inf
        B.add((2.0, dc, 0.0), f'boresight dc={dc!r}', frac=1.0)

    def keeps(frac):
        return cam_eval(cam, 'column', np.tile([2.0, 1e-100, 0.0], (len(frac), 1)), frac=frac)['keep']
    lo, hi = bracket(keeps, 1e100, 1e110)
    for f in (lo[0], hi[0]):
        B.add((2.0, 1e-100, 0.0), 'w overflows', vy=0.001, frac=float(f))
    B.brackets.append((len(B.rows) - 2, len(B.rows) - 1, 'w overflows', 'keep'))
    B.pairs.append((len(B.rows) - 2, len(B.rows) - 1))
    for where, p in (('inside', (2.1, 1.0, 0.1)), ('outside', (4.0, 1.0, 0.1)), ('behind', (2.1, -1.0, 0.1))):
        B.add(p, f'frac=NaN {where}', frac=np.nan)
        B.add(p, f'vy=NaN {where}', vy=np.nan)
    return camera_case(B, cam, 'column', arrangement, 210)


def cam_edges(axis, n, arrangement):
    """Step 3 with a camera at (0, -2, 0) and samples at y = -1: dc = 1, u = x, v = z exactly.  A
    sample on every edge of the n-bin axis with its two neighbours; the other axis has m != n bins."""
    m = 3 if axis == 'u' else 2
    m = 5 - m if m == n else m                      # never the same count on both axes
    cam = axis_camera((0.0, -2.0, 0.0), dims=(n, m) if axis == 'u' else (m, n))
    B = Build(300 + n)
    edges, other = (cam.uedges, cam.vedges) if axis == 'u' else (cam.vedges, cam.uedges)
    centres = (other[:-1] + other[1:])/2 + 0.013
    for k, e in enumerate(edges):
        t = centres[k % m]
        p = (e, -1.0, t) if axis == 'u' else (t, -1.0, e)
        B.hit(p, 0 if axis == 'u' else 2, f'{axis} edge', axis, e)
    return camera_case(B, cam, 'column', arrangement, 310 + n)


def cam_borders(name, dtype, arrangement):
    """Step 3 of a named camera of tests/test_gpu_camera.py: brackets across interior pixel borders
    of both axes and across the four frame borders, one coordinate walked per bracket."""
    cam = named_camera(name, (11, 9))
    right, bore, up = cam.basis
    B = Build(400, dtype)

    def evaluate(P):
        return cam_eval(cam, 'column', P)

    for axis, edges, direction, other, other_dir in (('u', cam.uedges, right, cam.vedges, up),
                                                     ('v', cam.vedges, up, cam.uedges, right)):
        coord = int(np.argmax(np.abs(direction)))
        key = 'ix' if axis == 'u' else 'iz'
        n = len(edges) - 1
        for k in range(n + 1):
            t = (other[k % (len(other) - 1)] + other[k % (len(other) - 1) + 1])/2
            depth = 2.0 + 0.37*k
            P = cam.o + depth*(bore + edges[k]*direction + t*other_dir)
            step = 0.3*depth*(edges[1] - edges[0])

            def decide(d, k=k, n=n, key=key):
                return d[key] >= k if k < n else d[key] < 0
            A, Bm = bracket_coordinate(evaluate, decide, P, coord, P[coord] - step, P[coord] + step, dtype)
            what = 'border' if 0 < k < n else 'frame'
            B.bracket(A, Bm, f'{axis} {what}', key)
    if name == 'oblique' and dtype == np.float64:
        P = np.array([cam.o, cam.o, cam.o, cam.o])
        for q in range(4):                              # a few ulps beside the camera
            P[q, 0] = _values(_keys(cam.o[0], np.float64) + 3*q, np.float64)
            P[q, 2] = _values(_keys(cam.o[2], np.float64) - 2*q, np.float64)
        A, Bm = bracket_coordinate(evaluate, lambda d: d['front'], P, 1, cam.o[1] - 0.5, cam.o[1] + 0.5)
        B.bracket(A, Bm, 'dc>0', 'front')
    return camera_case(B, cam, 'column', arrangement, 410)


def _hidden_brackets(B, cam, targets):
    """targets: (inequality, P, coord, lo, hi) -- brackets of that inequality alone; then, walking
    the same coordinate on by ulps from the bracket (and moving another one a little when the walk
    steps over it), a sample with b == r2 or c2 == r2 bit for bit, where `<` and `<=` part."""
    def evaluate(P):
        d = cam_eval(cam, 'column', P)
        return dict(d, **{'b>0': d['b'] > 0, 'b<r2': d['b'] < d['r2'], 'c2<r2': d['c2'] < d['r2']})
    for which, P, coord, lo, hi in targets:
        A, Bm = bracket_coordinate(evaluate, lambda d, which=which: d[which], [P], coord, lo, hi)
        B.bracket(A, Bm, which, which)
        if which == 'b>0':
            continue
        key = 'b_r2' if which == 'b<r2' else 'c2_r2'
        for attempt in range(200):
            Q = A[0].copy()
            Q[(coord + 1) % 3] *= 1 + 1e-3*attempt

            def difference(values, Q=Q):
                R = np.tile(Q, (len(values), 1))
                R[:, coord] = values
                return evaluate(R)[key]
            try:
                Q[coord] = walk_to(difference, 0.0, Q[coord], reach=256)
            except ValueError:
                continue
            B.hit(Q, coord, which.replace('<', '='), key, 0.0)
            break


def cam_hidden_axis(D, arrangement):
    """Step 4 from (0, -D, 0), looking at the planet along +y, 127 degrees wide.  ``b < r2`` decides
    at the point of closest approach of a line through the planet (y walks along the line);
    ``c2 < r2`` decides on the limb behind the planet (x walks across it) -- not from D = 1, where
    c2 - r2 = -(y + D)^2 < 0 for every sample in front of the camera."""
    cam = axis_camera((0.0, -float(D), 0.0), half=(2.0, 2.0), dims=(4, 3))
    B = Build(500)
    targets = []
    for q in range(4):
        rho, z = 0.1 + 0.1*q, 0.05 + 0.05*q
        targets.append(('b<r2', (rho, 0.0, z), 1, -0.6, 0.6))
        if D > 1:
            y = 1.5 + q
            targets.append(('c2<r2', (0.5, y, z), 0, 0.2, 1.9*(y + D)))
    _hidden_brackets(B, cam, targets)
    return camera_case(B, cam, 'column', arrangement, 510)


def cam_hidden_b_axis(D, arrangement):
    """The sign of b from (D, 0, 0), looking along +y past the planet: b = -D (x - D), x walks
    through the camera's own.  (See the module's note: the sample is hidden on neither side.)"""
    cam = axis_camera((float(D), 0.0, 0.0), half=(2.0, 2.0), dims=(5, 3))
    B = Build(540)
    targets = [('b>0', (float(D), 0.7 + 0.9*q, 0.1 + 0.2*q), 0, D - 0.25, D + 0.25) for q in range(4)]
    _hidden_brackets(B, cam, targets)
    return camera_case(B, cam, 'column', arrangement, 550)


def cam_hidden_oblique(arrangement):
    """Step 4 of the 'oblique' camera.  No 'b>0' here: b = 0 lies at right angles to the planet's
    centre, which this camera has 10 degrees off its boresight, outside the field of view."""
    cam = named_camera('oblique', (11, 9))
    B = Build(520)
    o = cam.o
    D = np.linalg.norm(o)
    unit = o/D
    side = np.cross(unit, cam.basis[2])
    side /= np.linalg.norm(side)
    targets = []
    for q in range(4):
        # behind the planet, on the limb as the camera sees it: the coordinate most along `side`
        a = 1.5 + 0.8*q
        limb = -a*unit + (D + a)/np.sqrt(D*D - 1)*side*(1 if q % 2 else -1)
        c = int(np.argmax(np.abs(side)))
        reach = 0.3/abs(side[c])
        targets.append(('c2<r2', limb, c, limb[c] - reach, limb[c] + reach))
        # closest approach of a line through the planet: walk the coordinate most along the line
        near = (0.15 + 0.1*q)*side + 0.1*q*cam.basis[2]
        c = int(np.argmax(np.abs(near - o)))
        targets.append(('b<r2', near, c, near[c] - 0.6, near[c] + 0.6))
    _hidden_brackets(B, cam, targets)
    return camera_case(B, cam, 'column', arrangement, 530)


SUNLIT_XZ = ((1.0, 2.0**-26), (1.0, float(np.sqrt(2.0**-51))))     # s = 1 + 2^-52 and 1 + 2^-51
SUNLIT_Y = (0.0, -0.0, -TINY, 1.0)


def _sunlit_places(B, evaluate):
    """x*x + z*z = 1 + 2^-52 exactly (dark unless y < 0) and the next value up (sunlit), each with
    y in SUNLIT_Y; brackets of the cylinder test on x at z = 0.6."""
    for x, z in SUNLIT_XZ:
        s = x*x + z*z
        for y in SUNLIT_Y:
            B.hit((x, y, z), 1, 's=1+2^-52 and next', 's', s, sides=False)
    P = [(0.8, 0.5, 0.6), (0.8, 0.0, 0.6), (-0.8, 2.5, 0.6), (0.8, 0.25, -0.6)]
    A, Bm = bracket_coordinate(evaluate, lambda d: d['sunlit'], P, 0,
                               [0.5, 0.5, -0.5, 0.5], [1.1, 1.1, -1.1, 1.1])
    B.bracket(A, Bm, 'sunlit', 'sunlit')


def cam_sunlit(arrangement):
    """Step 5 seen from (3, 0, 0): the terminator cylinder edge-on, nothing hidden."""
    cam = Camera((3.0, 0.0, 0.0), None, (0, 0, 1), (90, 90), (5, 3))
    B = Build(600)
    _sunlit_places(B, lambda P: cam_eval(cam, 'constant', P))
    return camera_case(B, cam, 'constant', arrangement, 610)


# ---- shells ------------------------------------------------------------------------------------------
ALT = (1.5, 4.0, 7)


def shell_longitude(nlon, arrangement):
    """The placements whose longitude bin does not hang on the last bit of atan2."""
    grid = (nlon, 3)
    B = Build(700 + nlon)
    for x in (0.0, -0.0):
        B.add((x, -2.0, 0.3), 'lon=+-0')
        B.add((x, 2.0, 0.3), 'lon=pi')
    B.add((-1e-300, -2.0, 0.3), 'lon=-tiny+2pi')
    for y in (0.0, -0.0):
        for x in (1.0, -1.0):
            B.add((2*x, y, 0.3), 'lon=pi/2 or 3pi/2')
    for x in (0.0, -0.0):
        for y in (0.0, -0.0):
            for z in (2.5, -2.5):
                B.add((x, y, z), 'pole')
    B.add((0.0, 0.0, 0.0), 'centre')
    B.add((0.0, 0.0, 0.0), 'centre frac=NaN', frac=np.nan)
    return shell_case(B, grid, ALT, 'column', arrangement, 710)


def _mu_of(x, y):
    def mu(z):
        r2 = (x*x + y*y) + z*z
        with np.errstate(all='ignore'):
            return z/np.sqrt(r2)
    return mu


def shell_mu(nlat, dtype, arrangement):
    """Brackets in z across every interior edge of nlat bands, at fixed x and y; mu = +-1 exactly
    and the first x at which it is not."""
    grid = (3, nlat)
    B = Build(800 + nlat, dtype)

    def evaluate(P):
        return shell_eval(grid, ALT, 'column', P)
    k = np.arange(1, nlat)
    ang = 0.4 + 1.7*(k % 3)                              # longitudes inside the three bins
    rad = 1.2 + 0.05*(k % 40)
    P = np.stack([rad*np.sin(ang), -rad*np.cos(ang), 0*rad], axis=1)
    A, Bm = bracket_coordinate(evaluate, lambda d: d['iz'] >= k, P, 2, -40.0, 40.0, dtype)
    B.bracket(A, Bm, 'mu edge', 'iz')
    if dtype == np.float64:
        for sign in (1.0, -1.0):
            P = [(0.0, -1e-10, sign*1.5), (0.0, -1e-10, sign*3.0)]
            A, Bm = bracket_coordinate(evaluate, lambda d: np.abs(d['mu']) < 1, P, 0, 0.0, 1e-3)
            B.bracket(A, Bm, '|mu|=1', '|mu|<1')
            for ia, *_ in B.brackets[-2:]:                # the member at x = 0's side has mu = +-1
                B.hits.append((ia, '|mu|=1', 'mu', sign))
    return shell_case(B, grid, ALT, 'column', arrangement, 810)


def shell_mu_hits(nlat, arrangement):
    """Samples whose mu equals an interior edge bit for bit, found by walking z by ulps."""
    grid = (3, nlat)
    B = Build(850 + nlat)
    mu_edges = shell_edges(*grid)[1]
    for k in range(1, nlat):
        x, y = 1.3*np.sin(0.4 + 1.7*(k % 3)), -1.3*np.cos(0.4 + 1.7*(k % 3))
        e = mu_edges[k]
        for attempt in range(64):                      # z / r steps over about one mu in eight: if
            xa = x*(1 + 0.003*attempt)                  # the edge is one of them, move x a little
            z0 = e*np.sqrt((xa*xa + y*y)/(1 - e*e))
            try:
                z = walk_to(_mu_of(xa, y), e, z0, reach=64)
            except ValueError:
                continue
            B.hit((xa, y, z), 2, 'mu edge', 'mu', e)
            break
        else:
            raise ValueError(f'no sample with mu == {e!r} found')
    return shell_case(B, grid, ALT, 'column', arrangement, 860)


def shell_altitude(alt, arrangement):
    """r exactly r_lo and r_hi and one ulp below each, on the x axis (lon = pi/2, mu = 0); brackets
    of the record across t = 0, every interior integer and t = nalt, x walked at fixed y and z."""
    grid = (3, 3)
    r_lo, r_hi, nalt = alt
    B = Build(900 + nalt)
    for r in (r_lo, r_hi):
        for v in neighbours(r)[:2]:
            B.hit((v, 0.0, 0.0), 0, 'r=r_lo, r_hi and 1 ulp below', 'r', v, sides=False)

    def evaluate(P):
        return shell_eval(grid, alt, 'column', P)
    j = np.arange(0, nalt + 1)
    y, z = -0.3 - 0.01*(j % 7), 0.4 + 0.01*(j % 5)
    P = np.stack([0*y, y, z], axis=1)
    A, Bm = bracket_coordinate(evaluate, lambda d: d['k'] > j, P, 0, 0.9*r_lo - 0.6, r_hi + 1.0)
    B.bracket(A, Bm, 'altitude record', 'k')
    return shell_case(B, grid, alt, 'column', arrangement, 910)


def shell_sunlit(arrangement):
    grid = (5, 3)
    B = Build(950)
    _sunlit_places(B, lambda P: shell_eval(grid, ALT, 'constant', P))
    return shell_case(B, grid, ALT, 'constant', arrangement, 960)


def shell_finite(arrangement):
    """c = w / r2 at the ends of the exponent range, frac = 1 unless said."""
    grid = (5, 3)
    B = Build(970)
    B.add((1e-160, -1e-160, 1e-160), 'r2 tiny: c overflows', frac=1.0)
    B.add((1e160, -1e160, 1e160), 'r2 overflows: c = 0', frac=1.0)
    B.add((1e150, -1e150, 1e150), 'r2 huge', frac=1.0)
    B.add((1e150, -1e150, 1e150), 'r2 huge: c underflows to 0', frac=1e-30)
    B.add((1e150, -1e150, 1e150), 'r2 huge: c denormal', frac=1e-12)
    B.add((1.0, -2.0, 0.3), 'frac=NaN', frac=np.nan)
    B.add((1.0, -2.0, 0.3), 'vy=NaN', vy=np.nan)
    return shell_case(B, grid, ALT, 'column', arrangement, 980)


# ---- the catalogue -----------------------------------------------------------------------------------
def _both(table):
    out = {}
    for name, make in table.items():
        out[name] = functools.lru_cache(maxsize=None)(functools.partial(make, 'packed'))
        out[name + '/pairs'] = functools.lru_cache(maxsize=None)(functools.partial(make, 'pairs'))
    return out


_TABLE = {'cam_front_finite': cam_front_finite, 'cam_sunlit': cam_sunlit,
          'cam_hidden_axis_1': functools.partial(cam_hidden_axis, 1),
          'cam_hidden_axis_1.25': functools.partial(cam_hidden_axis, 1.25),
          'cam_hidden_axis_1e3': functools.partial(cam_hidden_axis, 1000),
          'cam_hidden_b_axis_1': functools.partial(cam_hidden_b_axis, 1),
          'cam_hidden_b_axis_1e3': functools.partial(cam_hidden_b_axis, 1000),
          'cam_hidden_oblique': cam_hidden_oblique}
for _n in EDGE_COUNTS:
    _TABLE[f'cam_u_{_n}'] = functools.partial(cam_edges, 'u', _n)
    _TABLE[f'cam_v_{_n}'] = functools.partial(cam_edges, 'v', _n)
for _name in ('oblique', 'horizon'):
    _TABLE[f'cam_borders_{_name}_f64'] = functools.partial(cam_borders, _name, np.float64)
    _TABLE[f'cam_borders_{_name}_f32'] = functools.partial(cam_borders, _name, np.float32)
for _n in (1, 3, 5):
    _TABLE[f'shell_lon_{_n}'] = functools.partial(shell_longitude, _n)
for _n in (2, 3, 7, 64):
    _TABLE[f'shell_mu_{_n}_f64'] = functools.partial(shell_mu, _n, np.float64)
    _TABLE[f'shell_mu_{_n}_f32'] = functools.partial(shell_mu, _n, np.float32)
for _n in (2, 4, 7):
    _TABLE[f'shell_mu_hits_{_n}'] = functools.partial(shell_mu_hits, _n)
for _name, _alt in (('1', (1.5, 4.0, 1)), ('5', (1.5, 4.0, 5)), ('33', (1.5, 4.0, 33)),
                    ('narrow', (2.0, 2.0625, 4))):
    _TABLE[f'shell_alt_{_name}'] = functools.partial(shell_altitude, _alt)
_TABLE['shell_sunlit'] = shell_sunlit
_TABLE['shell_finite'] = shell_finite
CASES = _both(_TABLE)
CAMERA_CASES = [name for name in CASES if name.startswith('cam_')]
SHELL_CASES = [name for name in CASES if name.startswith('shell_')]


def restate(case):
    """(the restatement's result, its per-sample intermediates) of a case"""
    quantity, gt = tables(forces(), case['kind'])
    if case['family'] == 'camera':
        cam = case['camera']
        args = (*case['cols'], cam.o, cam.basis, cam.uedges, cam.vedges, forces().vrplanet, cam.area,
                quantity, gt)
        return camera_image(*args), camera_samples(*args)
    args = (*case['cols'], forces().vrplanet, quantity, gt, *case['grid'], *case['alt'])
    return shell_map(*args), shell_samples(*args)


@functools.lru_cache(maxsize=None)
def restated(name):
    """restate(CASES[name]()), computed once and not to be changed"""
    return restate(CASES[name]())


def extra_columns(case, seed=77):
    """Finite vx, vz [R/s] and time [s] columns of the case's type, for the kernels that read them"""
    rng = np.random.default_rng(seed)
    n = len(case['cols'][0])
    return tuple(np.ascontiguousarray(c.astype(case['dtype'])) for c in
                 (rng.normal(size=n)*1e-3, rng.normal(size=n)*1e-3, rng.uniform(0.0, 3000.0, n)))


def tally(case):
    """{threshold name: [brackets, exact hits]}"""
    out = {}
    for *_, name, _ in case['brackets']:
        out.setdefault(name, [0, 0])[0] += 1
    for _, name, *_ in case['hits']:
        out.setdefault(name, [0, 0])[1] += 1
    return out


def edge_misses():
    """{n: (edges at which bin_index's first guess is wrong, edges)} for the camera's edge cases"""
    return {n: (first_guess_misses(np.linspace(-TAN25, TAN25, n + 1)), n + 1) for n in EDGE_COUNTS}


if __name__ == '__main__':
    for n, (missed, of) in edge_misses().items():
        print(f'n = {n}: the first guess of bin_index is wrong at {missed} of {of} edges')
    for case_name in CASES:
        entry = CASES[case_name]()
        counts = ', '.join(f'{name}: {b} brackets, {h} hits' for name, (b, h) in tally(entry).items())
        print(f'{case_name}: {len(entry["cols"][0])} samples ({entry["n_threshold"]} on thresholds, '
              f'{entry["dtype"].__name__}); {counts}')
