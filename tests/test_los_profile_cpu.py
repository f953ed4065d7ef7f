"""The line-of-sight profile without a GPU: the restatement's identity against the oracle, the host
side of LOSResult(profile=...) (parsing, refusals, a plain result is unchanged) and the host-only
argument check of nxc_los_profile_enable as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import nexoclom_amd
from tests import los_profile_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
NEW_ATTRIBUTES = ('profile', 'profile_below', 'profile_above', 'velocity_edges', 'velocity_axis',
                  'profile_effective_packets', 'velocity', 'velocity_variance',
                  'velocity_dispersion', 'velocity_skewness', 'effective_packets', 'profile_sums',
                  'moment_sums')


def spacecraft(n=5):
    from nexoclom_amd import SpacecraftData
    th = np.linspace(0, 2*np.pi, n, endpoint=False)
    pos = np.stack([2*np.cos(th), -2 + 0*th, 2*np.sin(th)], 1)
    look = -pos/np.linalg.norm(pos, axis=1)[:, None]
    return SpacecraftData(*pos.T, *look.T)


def make_inputs():
    from nexoclom_amd import Input
    return Input(INPUT)


# ---- 1. the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_the_records_sum_to_the_oracles_radiance(f32):
    """Every used pair adds its wtemp to exactly one record of its spectrum, and the used pairs
    are all that adds to the oracle's radiance (no decided pair has a negative weight: asserted in
    the restatement for every case)."""
    c = PC.case('mixed', f32=f32)
    want = c['want']
    assert want.sums.shape == (6, PC.NV + 2, 2) and len(want.pairs) > 2000
    np.testing.assert_allclose(want.sums[..., 0].sum(1), want.radiance, rtol=1e-12, atol=0)
    # ww is the same sum in the records and in the moments; the moments' magnitudes bound them
    np.testing.assert_allclose(want.sums[..., 1].sum(1), want.moments[:, 3], rtol=1e-12, atol=0)
    assert np.all(np.abs(want.moments) <= want.moment_mags)
    hot = want.npackets > 0
    assert np.array_equal(hot, want.radiance > 0) and not want.sums[~hot].any()
    # about a sigma either side: the mean velocity of a hot spectrum lies well inside the range
    u = want.moments[hot, 0]/want.radiance[hot]
    assert np.all((PC.V_LO < u) & (u < PC.V_HI))


def test_the_edge_case_files_every_row_where_the_rule_says():
    for f32 in (False, True):
        c, record = PC.edge_case(f32)
        assert c['want'].bin_guard == 0.0 and c['m'] == 19        # rows sit exactly on edges
        assert sorted(set(record)) == list(range(10))             # every record is met


# ---- 2. the host side of profile= ------------------------------------------------------------------
def test_parse_profile():
    from nexoclom_amd.LOSResult import parse_profile
    assert parse_profile((-10, 10, 64), 512) == (-10.0, 10.0, 64)
    assert parse_profile([0.5, 1.5, np.int64(3)], 1) == (0.5, 1.5, 3)
    with pytest.raises(ValueError) as err:
        parse_profile((-10, 10, 2**21 - 2), 1024)
    assert '2^31' in str(err.value) and 'profile=' in str(err.value)
    assert parse_profile((-10, 10, 2**21 - 3), 1024)[2] == 2**21 - 3


BAD_PROFILES = [(-10, 10), (-10, 10, 64, 1), 'abc', 5, (-10, 10, 2.5), (-10, 10, 64.0), (-10, 10, 0),
                (-10, 10, -4), (10, -10, 4), (5, 5, 3), (np.nan, 1, 4), (0, np.inf, 4),
                (-np.inf, 0, 4), ('a', 1, 4), (-1.7e308, 1.7e308, 4)]


@pytest.mark.parametrize('bad', BAD_PROFILES, ids=[str(b) for b in BAD_PROFILES])
def test_a_bad_profile_is_refused_before_a_context_is_opened(bad):
    """parse_cube's rules with the argument's own name; no context is given and this machine may
    have no device: a ValueError, nothing else."""
    from nexoclom_amd import LOSResult
    with pytest.raises(ValueError) as err:
        LOSResult(spacecraft(), make_inputs(), profile=bad)
    assert 'profile=' in str(err.value) and 'cube=' not in str(err.value)


def test_profile_refuses_cp_and_the_fitted_result_refuses_profile():
    from nexoclom_amd import LOSResult, LOSResultFitted
    sc = spacecraft()
    los = LOSResult(sc, make_inputs(), context=object(), profile=(-10, 10, 8))
    with pytest.raises(NotImplementedError) as err:
        los.simulate_data_from_inputs(sc, cp=object())
    assert 'profile=' in str(err.value) and 'cp=' in str(err.value)
    with pytest.raises(NotImplementedError) as err:
        LOSResultFitted(sc, 'unfit', profile=(-10, 10, 8))
    assert 'profile=' in str(err.value) and 'LOSResultFitted' in str(err.value)


def test_profile_is_keyword_only_and_a_plain_result_has_none_of_it():
    from nexoclom_amd import LOSResult
    sc = spacecraft()
    with pytest.raises(TypeError):
        LOSResult(sc, make_inputs(), None, np.radians(1.), (-10, 10, 8))
    plain = LOSResult(sc, make_inputs())
    with_profile = LOSResult(sc, make_inputs(), profile=(-10, 10, 8))
    for obj in (plain, with_profile):              # they appear with the run, and only with profile=
        assert not any(hasattr(obj, name) for name in NEW_ATTRIBUTES)
    assert set(vars(with_profile)) == set(vars(plain))


def test_a_plain_pass_calls_the_plain_entries():
    """Without profile= compute_iteration hands los_accumulate exactly what it always did."""
    from nexoclom_amd import LOSResult
    from nexoclom_amd.Output import Output

    class Recorder:
        def __init__(self):
            self.calls = []

        def los_accumulate(self, *args, **kwargs):
            self.calls.append((len(args), sorted(kwargs)))
            S = args[8].shape[1]
            return dict(radiance=np.zeros(S), npackets=np.zeros(S, dtype=np.int64), included=None,
                        used=None, n_used=0)

        def counters(self):
            return {'nonfinite': 0}

    import pandas as pd
    out = Output.__new__(Output)
    frame = pd.DataFrame({c: np.linspace(1, 2, 4, dtype=np.float32) for c in PC.COLUMNS})
    out.X, out.X0 = frame, pd.DataFrame()
    out.npackets, out.totalsource = 4, 4.0
    out.vrplanet, out.aplanet = 0.0, 0.4
    sc = spacecraft()
    for profile, names, n_args in ((None, [], 14), ((-10, 10, 8), ['profile', 'vx', 'vz'], 14)):
        ctx = Recorder()
        los = LOSResult(sc, make_inputs(), context=ctx, profile=profile)
        los.compute_iteration(out, sc, profile=profile is not None)
        (count, keywords), = ctx.calls
        assert count == n_args and keywords == sorted(['index', 'n_index', 'used_cap'] + names)


# ---- 3. the C side's argument check, as a host program ------------------------------------------------
def test_argument_check_as_a_host_program(tmp_path):
    """nxc_los_profile_enable's refusals are host-only code (nxc_los_profile_check.hpp);
    tests/tools/los_profile_check.cpp feeds it good arguments, one bad set per refusal, and nv one
    below and at the 2^31 record limit for several numbers of spectra.  Built plainly here; the same
    file is what is built with -fsanitize=address,undefined to check the host code."""
    exe = tmp_path / 'los_profile_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', 'los_profile_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused: ' in line]
    assert len(refused) >= 17 and sum(' accepted' in line for line in lines) >= 6
    for word in ('S must be at least 1', 'nv must be at least 1', 'finite', 'below v_hi',
                 'v_hi - v_lo', '2^31'):
        assert any(word in line for line in refused), word
    assert any(line.startswith('1 spectrum, 2^31 - 1 records accepted') for line in lines)
    assert any(line.startswith('1 spectrum, 2^31 records refused') for line in lines)


def test_the_library_exports_the_five_entry_points():
    from nexoclom_amd import hip_api
    names = [f'nxc_los_profile_{what}' for what in ('enable', 'accumulate', 'accumulate_f32',
                                                    'accumulate_rows', 'download')]
    assert all(name in hip_api.EXPORTS for name in names)
    with open(os.path.join(HERE, '..', 'include', 'nexoclom_hip.h')) as f:
        header = f.read()
    assert 'Line-of-sight profile' in header and all(f'int {name}(' in header for name in names)
    assert 'spacecraft\'s own velocity is NOT subtracted' in header
