"""k_shell (shell_located) and k_shell_moments (shell_located<ShellHit>, the same front) on the GPU, ON the
thresholds the guarded tests (tests/test_gpu_shell_map.py, tests/test_gpu_shell_moments.py) keep
1e-9 away from -- 1e-7 from the seam and 1e-3 from the poles in their case 'seam_and_poles'.

The "ShellMap" definition of include/nexoclom_hip.h is fp64 with one rounding per operation, so the
latitude band, the altitude record, the sunlit flag and what is dropped as non-finite are functions
of a sample's bits, and both kernels are held to tests/shell_map_restatement.py exactly on the
inputs of tests/threshold_cases.py: brackets and exact hits of mu = z / r on every interior edge
and at +-1, of (int)t on every integer and of r at r_lo and r_hi, of the terminator cylinder, of
c = w / r2 at both ends of the exponent range.  The longitude is the one transcendental value: only
placements whose bin does not hang on the last bit of atan2 are used -- the seam through x = +-0
and x = -1e-300 (-tiny + 2 pi is the last edge, inclusive), the axes, and the poles, where
atan2(+-0, +-0) is fixed by C Annex F.  No guard is asserted here: tests/test_threshold_cases_cpu.py
asserts instead, without a GPU, that every bracket and hit is what it claims to be.

Asserted, for both kernels: packet counts per cell and the counters equal to the restatement's
exactly, the column at rtol 1e-11, the planes by compare_planes (a threshold sample in a
neighbouring record fails it: asserted without a GPU), and for every bracket that the two cells the
restatement predicts hold its counts."""
import numpy as np
import pytest

from tests import threshold_cases as T
from tests.test_gpu_shell_map import compare, forces, shell_set                           # noqa: F401

pytestmark = pytest.mark.gpu


def plain(ctx, case):
    ctx.shell_accumulate(*case['cols'])


def moments(ctx, case):
    x, y, z, vy, frac = case['cols']
    vx, vz, _ = T.extra_columns(case)
    ctx.shell_moments_enable()
    ctx.shell_moments_accumulate(x, y, z, vx, vy, vz, frac)


@pytest.mark.parametrize('accumulate', [plain, moments], ids=lambda f: f.__name__)
@pytest.mark.parametrize('name', T.SHELL_CASES)
def test_shell_on_the_thresholds(ctx, forces, name, accumulate):
    case = T.CASES[name]()
    want, d = T.restated(name)
    shell_set(ctx, forces, case['kind'], case['grid'], case['alt'])
    accumulate(ctx, case)
    counters = ctx.counters()
    print(f'{name}: {want.samples} samples, {want.binned} binned, {want.nonfinite} nonfinite; '
          f'{len(case["brackets"])} brackets, {len(case["hits"])} exact hits')
    column, counts, sums = ctx.shell_download()
    nlat = counts.shape[1]
    for ia, ib, label, which in case['brackets']:               # first, so that a failure names it
        if which == 'iz':
            assert d['cell'][ia] != d['cell'][ib]
        if which == 'k':
            assert d['k'][ia] != d['k'][ib] and d['cell'][ia] == d['cell'][ib]
        for i in (ia, ib):
            if d['keep'][i]:
                at = divmod(int(d['cell'][i]), nlat)
                assert counts[at] == want.counts[at], (label, i, at)
            if d['filed'][i]:
                rec = at + (int(d['k'][i]), 0)
                tol = 1e-11*want.abs_sums[(0,) + rec]
                assert abs(sums[(0,) + rec] - want.sums[(0,) + rec]) <= tol, (label, i, rec)
    assert np.isfinite(column).all() and np.isfinite(sums).all()
    compare(ctx, want, counters)
    assert want.binned > 0
