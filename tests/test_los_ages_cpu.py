"""The line-of-sight ages without a GPU: the restatement's identities against the oracle, the host
side of LOSResult(ages=...) (parsing, refusals, a plain result is unchanged), transient() and
transient_design() over constructed age sums, and the host-only argument check of
nxc_los_ages_enable as a stand-alone program."""
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import nexoclom_amd
from tests import los_ages_cases as AC

HERE = os.path.dirname(os.path.abspath(__file__))
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
NEW_ATTRIBUTES = ('age_profile', 'age_below', 'age_above', 'age_edges', 'age_axis',
                  'age_effective_packets', 'age_sums')
AGES = (400.0, 2500.0, 7)


def spacecraft(n=5, **columns):
    from nexoclom_amd import SpacecraftData
    th = np.linspace(0, 2*np.pi, n, endpoint=False)
    pos = np.stack([2*np.cos(th), -2 + 0*th, 2*np.sin(th)], 1)
    look = -pos/np.linalg.norm(pos, axis=1)[:, None]
    return SpacecraftData(*pos.T, *look.T, **columns)


def make_inputs():
    from nexoclom_amd import Input
    return Input(INPUT)


# ---- 1. the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_the_planes_sum_to_the_oracles_radiance(f32):
    """Every used pair adds its wtemp to exactly one plane of its spectrum, and the used pairs are
    all that adds to the oracle's radiance; cold spectra have empty records."""
    c = AC.case('mixed', f32=f32)
    want = c['want']
    assert want.sums.shape == (6, AC.NA + 2, 2) and len(want.pairs) > 2000
    np.testing.assert_allclose(want.sums[..., 0].sum(1), want.radiance, rtol=1e-12, atol=0)
    hot = want.npackets > 0
    assert np.array_equal(hot, want.radiance > 0) and 0 < hot.sum() < len(hot)
    assert not want.sums[~hot].any()
    assert np.array_equal(want.sums[..., 0] > 0, want.sums[..., 1] > 0)
    assert set(want.planes) == want.pairs


def test_the_edge_case_files_every_row_where_the_rule_says():
    for f32 in (False, True):
        c, record = AC.edge_case(f32)
        assert c['m'] == 28                                   # every row is seen
        assert sorted(set(record)) == list(range(10))         # every record is met
        assert np.array_equal(c['want'].sums[0, :, 0] > 0, np.bincount(record, minlength=10) > 0)


# ---- 2. the host side of ages= ----------------------------------------------------------------------
def test_parse_los_ages():
    from nexoclom_amd.LOSResult import parse_los_ages
    assert parse_los_ages((0, 3600, 64), 512) == (0.0, 3600.0, 64)
    assert parse_los_ages([0.5, 1.5, np.int64(3)], 1) == (0.5, 1.5, 3)
    with pytest.raises(ValueError) as err:
        parse_los_ages((0, 10, 2**21 - 2), 1024)
    assert '2^31' in str(err.value) and 'ages=' in str(err.value)
    assert parse_los_ages((0, 10, 2**21 - 3), 1024)[2] == 2**21 - 3


BAD_AGES = [(0, 10), (0, 10, 64, 1), 'abc', 5, (0, 10, 2.5), (0, 10, 64.0), (0, 10, 0), (0, 10, -4),
            (10, -10, 4), (5, 5, 3), (np.nan, 1, 4), (0, np.inf, 4), (-np.inf, 0, 4), ('a', 1, 4),
            (-1.7e308, 1.7e308, 4), (0, 10, 2**31)]


@pytest.mark.parametrize('bad', BAD_AGES, ids=[str(b) for b in BAD_AGES])
def test_a_bad_ages_is_refused_before_a_context_is_opened(bad):
    """parse_ages's rules and the record limit; no context is given and this machine may have no
    device: a ValueError, nothing else."""
    from nexoclom_amd import LOSResult
    with pytest.raises(ValueError) as err:
        LOSResult(spacecraft(), make_inputs(), ages=bad)
    assert 'ages=' in str(err.value)


class NoContext:
    """A context that fails the test when anything is asked of it."""

    def __getattr__(self, name):
        raise AssertionError(f'the context was used ({name}) before the refusal')


def test_ages_refuses_profile_cp_adaptive_steps_and_the_fitted_result():
    from nexoclom_amd import LOSResult, LOSResultFitted
    sc = spacecraft()
    with pytest.raises(NotImplementedError) as err:
        LOSResult(sc, make_inputs(), context=NoContext(), ages=AGES, profile=(-10, 10, 8))
    assert 'ages=' in str(err.value) and 'profile=' in str(err.value)
    los = LOSResult(sc, make_inputs(), context=NoContext(), ages=AGES)
    with pytest.raises(NotImplementedError) as err:
        los.simulate_data_from_inputs(sc, cp=object())
    assert 'ages=' in str(err.value) and 'cp=' in str(err.value)
    adaptive = make_inputs()
    adaptive.options.step_size = 0
    with pytest.raises(NotImplementedError) as err:
        LOSResult(sc, adaptive, context=NoContext(), ages=AGES)
    assert 'step_size = 0' in str(err.value)
    LOSResult(sc, adaptive, context=NoContext())              # without ages= such inputs are fine
    with pytest.raises(NotImplementedError) as err:
        LOSResultFitted(sc, 'unfit', ages=AGES)
    assert 'ages=' in str(err.value) and 'LOSResultFitted' in str(err.value)


def test_ages_is_keyword_only_and_a_plain_result_has_none_of_it():
    from nexoclom_amd import LOSResult
    sc = spacecraft()
    with pytest.raises(TypeError):
        LOSResult(sc, make_inputs(), None, np.radians(1.), AGES)
    plain = LOSResult(sc, make_inputs())
    with_ages = LOSResult(sc, make_inputs(), ages=AGES)
    for obj in (plain, with_ages):                 # they appear with the run, and only with ages=
        assert not any(hasattr(obj, name) for name in NEW_ATTRIBUTES)
    assert set(vars(with_ages)) - set(vars(plain)) == {'_ages'}
    for call in (lambda: plain.transient(([0.0], [1.0]), 0.0), lambda: plain.transient_design([0.0], 0.0)):
        with pytest.raises(ValueError, match='ages='):
            call()
    with pytest.raises(ValueError, match='simulate_data_from_inputs'):
        with_ages.transient(([0.0], [1.0]), 0.0)


def test_spacecraft_data_without_time_has_the_columns_it_had():
    from nexoclom_amd.LOSResult import BORESIGHT, POSITION
    assert list(spacecraft().data.columns) == list(POSITION + BORESIGHT)
    three = np.arange(3.0)
    full = spacecraft(3, radiance=three, sigma=three, alttan=three)
    assert list(full.data.columns) == list(POSITION + BORESIGHT) + ['radiance', 'sigma', 'alttan']
    timed = spacecraft(3, time=[10, 20, 30])
    assert list(timed.data.columns) == list(POSITION + BORESIGHT) + ['time']
    assert timed.data['time'].dtype == float and list(timed.data['time']) == [10.0, 20.0, 30.0]
    with pytest.raises(TypeError):
        nexoclom_amd.SpacecraftData(*np.zeros((6, 3)), 'Na', 'synthetic', None, None, None, three)


def test_a_pass_calls_the_entries_of_its_mode():
    """Without ages= compute_iteration hands los_accumulate exactly what it always did; with it,
    the time column and ages=True."""
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

    out = Output.__new__(Output)
    frame = pd.DataFrame({c: np.linspace(1, 2, 4, dtype=np.float32) for c in AC.COLUMNS})
    out.X, out.X0 = frame, pd.DataFrame()
    out.npackets, out.totalsource = 4, 4.0
    out.vrplanet, out.aplanet = 0.0, 0.4
    sc = spacecraft()
    for ages, names in ((None, []), (AGES, ['ages', 'time'])):
        ctx = Recorder()
        los = LOSResult(sc, make_inputs(), context=ctx, ages=ages)
        los.compute_iteration(out, sc, ages=ages is not None)
        (count, keywords), = ctx.calls
        assert count == 14 and keywords == sorted(['index', 'n_index', 'used_cap'] + names)


def test_the_binding_refuses_two_modes_and_ages_without_time():
    """Context.los_accumulate's own refusals come before anything is asked of the library."""
    from nexoclom_amd import hip_api
    ctx = hip_api.Context.__new__(hip_api.Context)            # no device, no handle
    nine = [None]*9
    with pytest.raises(ValueError, match='exclude each other'):
        hip_api.Context.los_accumulate(ctx, *nine, profile=True, ages=True, rows=object())
    with pytest.raises(ValueError, match='needs time'):
        hip_api.Context.los_accumulate(ctx, *nine, *[np.zeros(2)]*5, ages=True)


# ---- 3. transient() and transient_design() -------------------------------------------------------------
def result_with_sums(S=5, nbins=7, seed=3, time=None):
    """A LOSResult as simulate_data_from_inputs leaves it, over constructed age sums: a few records
    empty, one spectrum empty altogether."""
    from nexoclom_amd import LOSResult
    rng = np.random.default_rng(seed)
    sc = spacecraft(S) if time is None else spacecraft(S, time=time)
    sc.data.index = np.arange(50, 50 + S)
    los = LOSResult(sc, make_inputs(), ages=(100.0, 100.0 + 200.0*nbins, nbins))
    n = rng.integers(0, 40, (S, nbins + 2))
    n[-1] = 0
    w = rng.uniform(0.5, 2.0, (S, nbins + 2, 40))*(np.arange(40) < n[..., None])
    los.age_sums = np.stack([w.sum(-1), (w*w).sum(-1)], -1)
    los.atoms_per_packet = 3.7e21
    los._times = None if time is None else np.array(sc.data['time'], dtype=float)
    total = np.zeros(S)
    for k in range(nbins + 2):
        total = total + los.age_sums[:, k, 0]
    los.radiance = pd.Series(total*(los.atoms_per_packet/1e3), index=sc.data.index)
    los._publish_ages(sc.data.index)
    return los


def test_published_attributes():
    los = result_with_sums()
    assert los.age_profile.shape == (5, 7) and los.age_effective_packets.shape == (5, 7)
    for name in ('age_profile', 'age_below', 'age_above', 'age_effective_packets'):
        assert list(getattr(los, name).index) == list(los.radiance.index), name
    np.testing.assert_allclose(los.age_edges, 100.0 + 200.0*np.arange(8), rtol=0, atol=0)
    np.testing.assert_allclose(los.age_axis, 200.0 + 200.0*np.arange(7), rtol=0, atol=0)
    total = los.age_profile.sum(1) + los.age_below + los.age_above
    np.testing.assert_allclose(total.values, los.radiance.values, rtol=1e-12, atol=0)
    assert np.array_equal(los.age_profile.values, los.age_sums[:, 1:-1, 0]*(3.7e21/1e3))
    assert not los.age_effective_packets.values[-1].any()


def test_a_constant_history_of_one_gives_the_ordered_sum_of_the_planes():
    """K == 1 exactly, so radiance[s] is the planes of s added in the order 0 .. nbins + 1 from
    0.0, then scaled: bit for bit, against a loop over the spectra and planes written here."""
    los = result_with_sums(time=[0.0, 1e3, -5e3, 7.77e5, 12.5])
    for history in (([0.0], [1.0]), ([-1e4, 0.0, 333.3, 1e6], [1.0, 1.0, 1.0, 1.0])):
        got = los.transient(history)
        assert got.kernel.shape == (9, 5) and np.all(got.kernel == 1.0)
        assert np.array_equal(got.times, [0.0, 1e3, -5e3, 7.77e5, 12.5])
        want, eff = [], []
        for s in range(5):
            total, ww = 0.0, 0.0
            for k in range(9):
                total = total + float(los.age_sums[s, k, 0])*1.0
                ww = ww + float(los.age_sums[s, k, 1])*(1.0*1.0)
            want.append(total*(3.7e21/1e3))
            eff.append(total*total/ww if ww != 0 else 0.0)
        assert np.array_equal(got.radiance.values, np.array(want))
        assert np.array_equal(got.effective_packets.values, np.array(eff))
        assert np.array_equal(got.radiance.values, los.radiance.values)
        assert list(got.radiance.index) == list(los.radiance.index) == list(got.effective_packets.index)
        assert got.effective_packets.values[-1] == 0.0 and np.all(got.effective_packets.values[:-1] >= 1)


def test_a_step_far_in_the_past_or_the_future():
    """The rate steps from 0 to 1.  Long before every launch time: the steady radiance.  Long after
    the epochs: nothing but the oldest plane's share, at the first node's rate -- 0 -- and with the
    step turned round (1 long ago, 0 since) the outer plane alone."""
    los = result_with_sums()
    scale = 3.7e21/1e3
    steady = los.transient(([-1e9, -1e9 + 1.0], [0.0, 1.0]), 5000.0)
    assert np.array_equal(steady.kernel[:-1], np.ones((8, 5))) and not steady.kernel[-1].any()
    np.testing.assert_allclose(steady.radiance.values,
                               los.radiance.values - los.age_above.values, rtol=1e-12, atol=0)
    never = los.transient(([1e9, 1e9 + 1.0], [0.0, 1.0]), 5000.0)
    assert not never.kernel.any() and not never.radiance.values.any()
    assert not never.effective_packets.values.any()
    long_ago = los.transient(([1e9, 1e9 + 1.0], [1.0, 0.0]), np.full(5, 5000.0))
    assert np.array_equal(long_ago.kernel[:-1], np.ones((8, 5))) and np.all(long_ago.kernel[-1] == 1.0)
    ended = los.transient(([-1e9, -1e9 + 1.0], [1.0, 0.0]), 5000.0)
    assert not ended.kernel[:-1].any() and np.all(ended.kernel[-1] == 1.0)
    assert np.array_equal(ended.radiance.values, los.age_sums[:, -1, 0]*scale)
    assert np.array_equal(ended.radiance.values, los.age_above.values)


def test_times():
    los = result_with_sums()
    for call in (lambda: los.transient(([0.0], [1.0])), lambda: los.transient_design([0.0, 1.0])):
        with pytest.raises(ValueError, match='times'):
            call()
    for bad in ([1.0, 2.0], np.zeros((5, 1)), [0, 1, 2, 3, np.nan], np.inf, 'soon'):
        with pytest.raises(ValueError, match='times'):
            los.transient(([0.0], [1.0]), bad)
    assert np.array_equal(los.transient(([0.0], [1.0]), 7).times, np.full(5, 7.0))
    timed = result_with_sums(time=[1, 2, 3, 4, 5])
    assert np.array_equal(timed.transient(([0.0], [1.0])).times, [1.0, 2.0, 3.0, 4.0, 5.0])
    assert np.array_equal(timed.transient(([0.0], [1.0]), 9.0).times, np.full(5, 9.0))


def test_transient_design():
    """A @ rates against transient((t_nodes, rates)).radiance at J = 4 nodes and 7 bins.  Both are
    sums over the planes of S[s][k] times a K entry; K is linear in the rates up to the rounding of
    its own evaluation: J + 1 linear pieces of at most 8 rounded operations per entry, J entries of
    A per row, then nbins + 2 products and adds -- c = 8 (J + 1)^2 + 2 (nbins + 2) operations, each
    with a relative error of at most 2^-52 of a term no larger than sum_k |S[s][k]| max(rates)."""
    nbins, J = 7, 4
    times = np.array([900.0, 1500.0, 1700.0, 2600.0, 4000.0])
    los = result_with_sums(nbins=nbins, time=times)
    nodes = np.array([-200.0, 450.0, 1100.0, 2450.0])
    A = los.transient_design(nodes)
    assert A.shape == (5, J) and np.all(A >= 0) and not A[-1].any()
    assert A[:-1].any(0).all() and A[0, 3] == 0   # the first epoch lies before the last node's rise
    for j in range(J):
        assert np.array_equal(A[:, j], los.transient((nodes, np.eye(J)[j])).radiance.values)
    # the columns are a partition of one: a constant rate of 1 gives the steady radiance
    np.testing.assert_allclose(A.sum(1), los.radiance.values, rtol=1e-12, atol=0)
    c = 8*(J + 1)**2 + 2*(nbins + 2)
    scale = los.atoms_per_packet/1e3
    for rates in (np.array([0.0, 3.0, 0.5, 1.0]), np.array([2.0, 0.0, 0.0, 7.5]), np.ones(J)):
        direct = los.transient((nodes, rates)).radiance.values
        bound = c*2.0**-52*np.abs(los.age_sums[..., 0]).sum(1)*scale*rates.max()
        err = np.abs(A @ rates - direct)
        print('transient_design: max error over its bound', float(np.max(err[:-1]/bound[:-1])))
        assert np.all(err <= bound)
    assert np.array_equal(los.transient_design(nodes, times), A)
    assert not np.array_equal(los.transient_design(nodes, 0.0), A)


# ---- 4. the C side's argument check, as a host program ------------------------------------------------
@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_argument_check_as_a_host_program(tmp_path, flags):
    """nxc_los_ages_enable's refusals are host-only code (nxc_ages_check.hpp);
    tests/tools/los_ages_check.cpp feeds it good arguments, one bad set per refusal of the header's
    list, and na one below and at the 2^31 record limit for several numbers of spectra.  Built
    plainly and with the host sanitizers; run as its own process."""
    exe = tmp_path / 'los_ages_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'los_ages_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused: ' in line]
    assert len(refused) >= 21 and sum(' accepted' in line for line in lines) >= 8
    for word in ('S must be at least 1', 'na must be at least 1', 't0 must be finite',
                 'a_lo and a_hi must be finite', 'below a_hi', 'a_hi - a_lo',
                 'S * (na + 2) must be below 2^31'):
        assert any(word in line for line in refused), word
    assert any(line.startswith('1 spectrum, 2^31 - 1 records accepted') for line in lines)
    assert any(line.startswith('1 spectrum, 2^31 records refused') for line in lines)


def test_the_library_exports_the_five_entry_points_and_the_header_does_not_drift():
    from nexoclom_amd import hip_api
    from tests import test_abi
    names = [f'nxc_los_ages_{what}' for what in ('enable', 'accumulate', 'accumulate_f32',
                                                 'accumulate_rows', 'download')]
    assert all(name in hip_api.EXPORTS for name in names) and hip_api.ABI_VERSION == 3
    with open(test_abi.HEADER) as f:
        header = f.read()
    assert 'Line-of-sight ages' in header and all(f'int {name}(' in header for name in names)
    assert test_abi.signature_drift(header) == []
    lib = hip_api.load_library()
    assert all(hasattr(lib, name) for name in names)
