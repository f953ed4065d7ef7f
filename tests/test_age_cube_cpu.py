"""The age cube without a GPU: the restatement's bin rule and contraction, transient.py
(response_matrix, parse_ages, ages_from_sums), the refusals of ages= on objects built without a
device, and the host-only checks and LDS plan of nxc_*_ages_* as a stand-alone program under the
host sanitizers."""
import contextlib
import io
import os
import re
import subprocess

import numpy as np
import pytest

import nexoclom_amd
from nexoclom_amd import hip_api
from nexoclom_amd.transient import (TransientImages, ages_from_sums, parse_ages,
                                    response_matrix)
from oracle import np_oracle
from tests.age_cube_restatement import (apply_ordered, apply_plan, camera_ages, image_ages,
                                        planes)

HERE = os.path.dirname(os.path.abspath(__file__))
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
EPS = 2.0**-52


# ---- 1. the restatement ---------------------------------------------------------------------------
def test_the_bin_rule():
    """na = 4 over [60, 180): bins of 30 s.  With t0 = 0 a row time is minus its age, so ages one
    ulp off an edge exist; t0 = 3000 gives the same planes for the ages that exist there."""
    age = np.array([60.0, 90.0, 120.0, 150.0, 180.0,                 # every edge
                    np.nextafter(60.0, 0), np.nextafter(60.0, 1e9),  # one ulp either side of a_lo
                    np.nextafter(90.0, 0), np.nextafter(90.0, 1e9),
                    np.nextafter(180.0, 0), np.nextafter(180.0, 1e9),
                    0.0, 3000.0, -30.0, -1e300, 1e300, np.inf, -np.inf])
    want = [1, 2, 3, 4, 5, 0, 1, 1, 2, 4, 5, 0, 5, 0, 0, 5, 5, 0]
    k, guard = planes(-age, 4, 0.0, 60.0, 180.0)
    assert list(k) == want and guard == 0.0
    whole = np.array([0, 1, 2, 3, 4, 11, 12, 13])
    k, guard = planes(3000.0 - age[whole], 4, 3000.0, 60.0, 180.0)
    assert list(k) == [want[j] for j in whole] and guard == 0.0
    k, _ = planes(np.array([np.nan, 2900.0]), 4, 3000.0, 60.0, 180.0)
    assert list(k) == [5, 2]
    assert planes(np.array([np.nan, 3000.0]), 4, 3000.0, 60.0, 180.0)[1] == np.inf
    assert planes(np.array([2925.0]), 4, 3000.0, 60.0, 180.0)[1] == 0.5
    # float32 times are widened, not the ages narrowed
    t32 = np.array([2940.0, 2910.0, 16777216.0], dtype=np.float32)
    assert list(planes(t32, 4, 3000.0, 60.0, 180.0)[0]) == [1, 2, 0]


@pytest.mark.parametrize('na,m,a_lo', [(1, 7, 0.0), (2, 5, 300.0), (7, 2, 300.0), (64, 0, 300.0),
                                       (64, 1, 0.0), (100, 0, -15.0)])
def test_ages_on_edges_follow_from_integers(na, m, a_lo):
    """Times that are multiples of 30 s and a_hi - a_lo = 30 na 2^m: age a_lo + 30 j is filed
    under bin j >> m, although 1/30 is not a binary fraction -- also from float32 times, which
    are widened exactly."""
    t0 = 3000.0
    j = np.arange(0, 101)
    time = t0 - 30.0*j
    want = np.where(30.0*j < a_lo, 0, np.minimum(1 + (np.floor((30.0*j - a_lo)/30.0).astype(int) >> m),
                                                   na + 1))
    for t in (time, time.astype(np.float32)):
        k, guard = planes(t, na, t0, a_lo, a_lo + 30.0*na*2**m)
        assert np.array_equal(k, want)
        assert guard == (0.5 if a_lo < 0 and m == 0 else 0.0) or m > 0


def cloud(n, seed, extent=6.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = d*rng.uniform(1.0, extent, n)[:, None]
    time = 30.0*rng.integers(0, 101, n)
    return time, p[:, 0], p[:, 1], p[:, 2], rng.normal(size=n)*2.0/2440.53, rng.integers(1, 17, n)/16.0


IMAGE_ARGS = (2e-4, np_oracle.image_rotation(0.7, 0.4), 'column', [], (16, 12), (-4., 4.), (-4., 4.),
              1.0)


@pytest.mark.parametrize('na,a_lo,a_hi', [(1, 0.0, 3840.0), (7, 600.0, 1020.0), (64, 300.0, 2220.0)])
def test_the_planes_sum_to_the_image(na, a_lo, a_hi):
    """Every sample that adds w to image[pix] adds w to exactly one plane of pix; with a pixel of
    1 cm^2 and fractions in sixteenths every sum is exact."""
    cols = cloud(20000, 5)
    res = image_ages(*cols, *IMAGE_ARGS, na, 3000.0, a_lo, a_hi)
    assert res.binned > 5000 and res.sums.shape == (16, 12, na + 2, 2)
    assert np.array_equal(res.sums[..., 0].sum(-1), res.image)
    # (a sample behind the planet is counted and has w == 0: it is filed nowhere)
    assert np.all(res.packets.sum(-1) <= res.counts) and res.packets.sum() > 0.8*res.counts.sum()
    assert np.array_equal(res.sums, res.abs_sums)
    if na == 1:
        assert not res.sums[:, :, [0, -1]].any()          # the range holds every age
    else:
        assert res.sums[:, :, 0, 0].sum() > 0 and res.sums[:, :, -1, 0].sum() > 0
    # float32 times are widened: the same planes
    narrow = image_ages(cols[0].astype(np.float32), *cols[1:], *IMAGE_ARGS, na, 3000.0, a_lo, a_hi)
    assert np.array_equal(narrow.sums, res.sums)

    from nexoclom_amd.CameraImage import camera_basis
    o = np.array([1.5, -6.0, 2.0])
    ue, ve = np.linspace(-0.4, 0.4, 9), np.linspace(-0.3, 0.3, 7)
    cam = camera_ages(*cols, o, camera_basis(-o, (0, 0, 1)), ue, ve, 2e-4, 1.0, 'column', (), na,
                      3000.0, a_lo, a_hi)
    assert cam.binned > 500 and cam.sums.shape == (8, 6, na + 2, 2)
    np.testing.assert_allclose(cam.sums[..., 0].sum(-1), cam.image, rtol=1e-12, atol=0)
    assert np.all(cam.packets.sum(-1) <= cam.counts) and cam.packets.sum() > 0.8*cam.counts.sum()


def test_apply_ordered_is_the_contraction():
    rng = np.random.default_rng(3)
    sums = np.stack([rng.normal(size=(5, 4, 9)), rng.uniform(0, 1, (5, 4, 9))], -1)
    K = rng.normal(size=(9, 6))
    out = apply_ordered(sums, K)
    assert out.shape == (6, 5, 4, 2)
    np.testing.assert_allclose(out[..., 0], np.einsum('xzk,ke->exz', sums[..., 0], K), rtol=0,
                               atol=9*EPS*np.einsum('xzk,ke->exz', np.abs(sums[..., 0]), np.abs(K)).max())
    np.testing.assert_allclose(out[..., 1], np.einsum('xzk,ke->exz', sums[..., 1], K*K), rtol=9*EPS)
    # one pixel by hand, in the order of the planes
    s = 0.0
    for k in range(9):
        s = s + sums[2, 1, k, 0]*K[k, 4]
    assert out[4, 2, 1, 0] == s
    assert np.array_equal(apply_ordered(sums, np.ones((9, 1)))[0, ..., 1] > 0, np.ones((5, 4), bool))


# ---- 2. response_matrix ---------------------------------------------------------------------------
EDGES = 60.0 + 30.0*np.arange(9)            # 8 bins of 30 s from 60 s to 300 s


def test_a_constant_history_gives_ones():
    for history in (([0.0], [1.0]), ([0.0, 100.0], [1.0, 1.0]),
                    ([-500.0, 17.0, 423.0, 1e6], [1.0]*4)):
        K = response_matrix(EDGES, [-1e4, 0.0, 17.0, 250.0, 423.0, 3e7], history)
        assert K.shape == (10, 6) and np.array_equal(K, np.ones((10, 6)))
    K = response_matrix(EDGES, [5.0], ([0.0, 1.0], [0.25, 0.25]))
    assert np.array_equal(K, np.full((10, 1), 0.25))


def test_a_step_gives_the_covered_fraction_of_every_launch_interval():
    """The source switches on at t_s (a ramp one ulp wide): bin k of epoch t_e was launched in
    [t_e - edge[k + 1], t_e - edge[k]], of which the part after t_s counts."""
    t_s = 1000.0
    step = ([t_s, np.nextafter(t_s, np.inf)], [0.0, 1.0])
    epochs = np.array([t_s - 1.0, t_s, t_s + 10.0, t_s + 60.0, t_s + 75.0, t_s + 180.0, t_s + 300.0,
                       t_s + 1e4])
    K = response_matrix(EDGES, epochs, step)
    lo, hi = epochs[None, :] - EDGES[1:, None], epochs[None, :] - EDGES[:-1, None]
    covered = np.clip(hi - t_s, 0.0, 30.0)/30.0
    np.testing.assert_allclose(K[1:-1], covered, rtol=0, atol=1e-12)
    assert np.array_equal(covered[:, 4], [0.5, 0, 0, 0, 0, 0, 0, 0])        # t_e - t_s = 75 s
    assert np.array_equal(covered[:, 5], [1, 1, 1, 1, 0, 0, 0, 0])          # 180 s: four bins
    assert np.array_equal(K[1:-1, 5] == 0, covered[:, 5] == 0)              # wholly before t_s: 0
    assert np.all(lo < hi)
    # row 0: the mean over [t_e - a_lo, t_e]; the last row: the rate long ago
    np.testing.assert_allclose(K[0], np.clip(epochs - t_s, 0.0, 60.0)/60.0, rtol=0, atol=1e-12)
    assert np.array_equal(K[-1], np.zeros(8))
    # a source that switches off instead: the complement, and the first node's rate stays
    off = response_matrix(EDGES, epochs, (step[0], [1.0, 0.0]))
    np.testing.assert_allclose(off[:-1], 1.0 - K[:-1], rtol=0, atol=1e-12)
    assert np.array_equal(off[-1], np.ones(8))


def dense_mean(p, q, nodes, rates, n=200001):
    """Trapezoid quadrature of the piecewise-linear function over [p, q], refined at the nodes."""
    t = np.unique(np.concatenate([np.linspace(p, q, n), np.clip(nodes, p, q)]))
    r = np.interp(t, nodes, rates)
    return np.sum(np.diff(t)*(r[:-1] + r[1:])/2)/(q - p)


def test_against_a_dense_quadrature():
    """Nodes inside bins, on edges and outside every bin; epochs before the first and after the
    last node.  The trapezoid rule is exact on every linear piece once the nodes are grid points,
    so the quadrature's own error is rounding: 2e5 terms of one sign, far below 1e-12 relative."""
    nodes = np.array([-100.0, 40.0, 55.0, 130.0, 131.0, 600.0])
    rates = np.array([0.3, 2.0, 0.0, 0.0, 5.0, 1.5])
    epochs = np.array([-500.0, -100.0, 37.0, 130.0, 250.0, 400.0, 601.0, 5000.0])
    K = response_matrix(EDGES, epochs, (nodes, rates))
    assert K.shape == (10, 8)
    for e, t_e in enumerate(epochs):
        for k in range(8):
            want = dense_mean(t_e - EDGES[k + 1], t_e - EDGES[k], nodes, rates)
            assert abs(K[1 + k, e] - want) <= 1e-12*max(want, 1e-300), (k, e)
        want = dense_mean(t_e - EDGES[0], t_e, nodes, rates)
        assert abs(K[0, e] - want) <= 1e-12*want
    assert np.array_equal(K[-1], np.full(8, 0.3))
    # before the first node everything is the first rate, long after the last the last one
    assert np.array_equal(K[:, 0], np.full(10, 0.3))
    assert np.array_equal(K[:-1, 7], np.full(9, 1.5))
    # a node inside a bin: epoch 250, bin 2 = launches in [100, 130] at rate 0, bin 3 = [70, 100]
    assert K[3, 4] == 0.0 and K[4, 4] == 0.0 and K[5, 4] > 0.0


def test_the_outer_rows():
    nodes, rates = [0.0, 100.0], [2.0, 4.0]
    K = response_matrix([0.0, 50.0, 100.0], [100.0, 150.0], (nodes, rates))
    assert np.array_equal(K[0], [4.0, 4.0])                   # a_lo == 0: the rate at t_e
    assert np.array_equal(K[-1], [2.0, 2.0])                  # the first node's rate
    np.testing.assert_allclose(K[1:-1], [[3.5, 4.0], [2.5, 3.5]], rtol=4*EPS)
    K = response_matrix([20.0, 50.0], [100.0], (nodes, rates))
    np.testing.assert_allclose(K[0], [3.8], rtol=4*EPS)       # the mean over [80, 100]
    assert response_matrix([0.0, 1.0], 5.0, ([0.0], [1.0])).shape == (3, 1)


BAD_HISTORIES = [([0.0, 0.0], [1.0, 1.0]), ([1.0, 0.0], [1.0, 1.0]), ([0.0, np.nan], [1.0, 1.0]),
                 ([0.0, np.inf], [1.0, 1.0]), ([0.0, 1.0], [1.0, -0.5]), ([0.0, 1.0], [1.0, np.nan]),
                 ([0.0, 1.0], [1.0, np.inf]), ([0.0, 1.0], [1.0]), ([], []), 'abc', 5,
                 ([[0.0, 1.0]], [[1.0, 1.0]]), ([0.0, 1.0],)]


@pytest.mark.parametrize('bad', BAD_HISTORIES, ids=[str(b) for b in BAD_HISTORIES])
def test_a_bad_history_is_refused(bad):
    with pytest.raises(ValueError):
        response_matrix(EDGES, [0.0], bad)


def test_bad_epochs_and_edges_are_refused():
    good = ([0.0], [1.0])
    for epochs in ([np.nan], [0.0, np.inf], [], 'abc', [[0.0]]):
        with pytest.raises(ValueError):
            response_matrix(EDGES, epochs, good)
    for edges in ([0.0], [0.0, 0.0], [1.0, 0.0], [0.0, np.nan], [0.0, np.inf], 'abc', [[0.0, 1.0]]):
        with pytest.raises(ValueError):
            response_matrix(edges, [0.0], good)


# ---- 3. the host side of ages= --------------------------------------------------------------------
def test_ages_from_sums():
    sums = np.zeros((2, 3, 5, 2))
    sums[0, 1, :, 0] = [1., 2., 0., 4., 8.]
    sums[0, 1, :, 1] = [1., 2., 0., 4., 16.]
    got = ages_from_sums(sums, 10.0, 0.0, 90.0)
    assert tuple(got) == ('age_cube', 'age_below', 'age_above', 'age_edges', 'age_axis',
                          'age_effective_packets')
    assert got['age_cube'].shape == (2, 3, 3) and got['age_below'].shape == (2, 3)
    assert list(got['age_cube'][0, 1]) == [20., 0., 40.]
    assert got['age_below'][0, 1] == 10. and got['age_above'][0, 1] == 80.
    assert list(got['age_edges']) == [0., 30., 60., 90.]
    assert list(got['age_axis']) == [15., 45., 75.]
    assert list(got['age_effective_packets'][0, 1]) == [2., 0., 4.]
    assert not got['age_cube'][1].any() and not got['age_effective_packets'][1].any()


def test_transient_images():
    sums = np.zeros((2, 3, 2, 2))
    sums[0, 1, 1] = [6.0, 9.0]
    sums[1, 2, 0] = [1.0, 1.0]
    res = TransientImages([5.0, 6.0], np.ones((4, 2)), sums, 10.0)
    assert list(res.epochs) == [5.0, 6.0] and res.images.shape == (2, 3, 2)
    assert res.images[0, 1, 1] == 60.0 and res.effective_packets[0, 1, 1] == 4.0
    assert list(res.light_curve) == [60.0, 10.0]
    assert not res.effective_packets[0, 0].any()


def test_parse_ages():
    assert parse_ages((0, 3000, 100)) == (0.0, 3000.0, 100)
    assert parse_ages([-15.0, 1.5, np.int64(3)]) == (-15.0, 1.5, 3)


BAD_AGES = [(0, 10), (0, 10, 64, 1), 'abc', 5, (0, 10, 2.5), (0, 10, 64.0), (0, 10, 0),
            (0, 10, -4), (10, 0, 4), (5, 5, 3), (np.nan, 1, 4), (0, np.inf, 4), (-np.inf, 0, 4),
            ('a', 1, 4), (-1.7e308, 1.7e308, 4)]


def make_inputs():
    from nexoclom_amd import Input
    return Input(INPUT)


IMAGE = dict(quantity='column', dims='8,6')
CAMERA = dict(quantity='column', observer='0,-3,0.5', fov='40,30', dims='8,6')
AGES = (0, 150, 5)


@pytest.mark.parametrize('bad', BAD_AGES, ids=[str(b) for b in BAD_AGES])
def test_bad_ages_are_refused_before_a_context_is_opened(bad):
    """No context is given and this machine may have no device: a ValueError, nothing else."""
    from nexoclom_amd import CameraImage, ModelImage
    from nexoclom_amd.input_classes import InputError
    with pytest.raises(ValueError):
        parse_ages(bad)
    for build in (lambda: ModelImage(make_inputs(), IMAGE, ages=bad),
                  lambda: make_inputs().produce_image(IMAGE, ages=bad),
                  lambda: CameraImage(make_inputs(), CAMERA, ages=bad)):
        with pytest.raises((ValueError, InputError)) as err:
            build()
        assert 'ages=' in str(err.value)


def test_a_block_with_too_many_records_is_refused_on_the_host():
    from nexoclom_amd import ModelImage
    with pytest.raises(ValueError) as err:
        ModelImage(make_inputs(), dict(quantity='column', dims='4096,4096'), ages=(0, 10, 126))
    assert '2^31' in str(err.value) and 'ages=' in str(err.value)


@pytest.mark.parametrize('kw', [dict(npackets=1000), dict(shard=(0, 10)), dict(moments=True),
                                dict(cube=(-10, 10, 5))])
def test_model_image_refuses_ages_with(kw):
    from nexoclom_amd import ModelImage
    with pytest.raises(NotImplementedError) as err:
        ModelImage(make_inputs(), IMAGE, context=object(), ages=AGES, **kw)
    assert 'ages=' in str(err.value) and next(iter(kw)) in str(err.value)


@pytest.mark.parametrize('kw', [dict(npackets=1000), dict(shard=(0, 10)), dict(cp=object()),
                                dict(moments=True), dict(cube=(-10, 10, 5))])
def test_camera_image_refuses_ages_with(kw):
    from nexoclom_amd import CameraImage
    with pytest.raises(NotImplementedError) as err:
        CameraImage(make_inputs(), CAMERA, context=object(), ages=AGES, **kw)
    assert 'ages=' in str(err.value) and next(iter(kw)) in str(err.value)


@pytest.mark.parametrize('kw', [dict(cp=object()), dict(moments=True), dict(cube=(-10, 10, 5))])
def test_produce_image_refuses_ages_with(kw):
    with pytest.raises(NotImplementedError) as err:
        make_inputs().produce_image(IMAGE, context=object(), ages=AGES, **kw)
    assert 'ages=' in str(err.value) and next(iter(kw)) in str(err.value)


def test_an_adaptive_step_run_is_refused_with_the_reason():
    from nexoclom_amd import CameraImage, ModelImage
    inputs = make_inputs()
    inputs.options.step_size = 0
    for build in (lambda: ModelImage(inputs, IMAGE, context=object(), ages=AGES),
                  lambda: inputs.produce_image(IMAGE, context=object(), ages=AGES),
                  lambda: CameraImage(inputs, CAMERA, context=object(), ages=AGES)):
        with pytest.raises(NotImplementedError) as err:
            build()
        assert 'step_size = 0' in str(err.value) and 'final row' in str(err.value)
        assert 'does not carry the age' in str(err.value)


def test_ages_is_keyword_only_and_an_empty_catalogue_gives_an_empty_block():
    from nexoclom_amd import CameraImage, ModelImage
    with contextlib.redirect_stdout(io.StringIO()):
        image = ModelImage(make_inputs(), IMAGE, context=object(), ages=AGES)
        cam = CameraImage(make_inputs(), CAMERA, context=object(), ages=AGES)
        moon = ModelImage(make_inputs(), IMAGE, context=object(), ages=AGES, slab_rows=5)
        plain = ModelImage(make_inputs(), IMAGE, context=object())
    with pytest.raises(TypeError):
        ModelImage(make_inputs(), IMAGE, False, None, AGES)
    for obj in (image, cam, moon):
        assert obj.ages == (0.0, 150.0, 5)
        assert obj.age_sums.shape == (8, 6, 7, 2) and not obj.age_sums.any()
        assert obj.age_cube.shape == (8, 6, 5) and obj.age_below.shape == (8, 6) == obj.age_above.shape
        assert obj.age_effective_packets.shape == (8, 6, 5) and not obj.age_effective_packets.any()
        assert list(obj.age_edges) == [0, 30, 60, 90, 120, 150]
        assert list(obj.age_axis) == [15, 45, 75, 105, 135]
        assert not hasattr(obj, 'cube_sums') and not hasattr(obj, 'moment_sums')
        # nothing was binned: the transient images are empty, and no device is asked
        res = obj.transient([0.0, 10.0], ([0.0, 5.0], [0.0, 2.0]))
        assert res.images.shape == (2, 8, 6) and not res.images.any()
        assert res.kernel.shape == (7, 2) and list(res.light_curve) == [0.0, 0.0]
        with pytest.raises(ValueError):
            obj.transient([0.0], ([1.0, 0.0], [1.0, 1.0]))
    assert plain.ages is None and not hasattr(plain, 'age_sums') and not hasattr(plain, 'age_axis')
    with pytest.raises(ValueError) as err:
        plain.transient([0.0], ([0.0], [1.0]))
    assert 'ages=' in str(err.value)


# ---- 4. the C side's host-only code, as a program under the sanitizers ----------------------------
def test_argument_check_and_plan_as_a_host_program(tmp_path):
    """nxc_*_ages_enable's and nxc_*_ages_apply's refusals and the LDS plan of k_ages_apply are
    host-only code (nxc_ages_check.hpp); tests/tools/ages_check.cpp feeds it good arguments, one
    bad set per refusal, na one below and at the 2^31 record limit, and the plan at 64 KiB and
    160 KiB.  Built with -fsanitize=address,undefined and run as its own process."""
    exe = tmp_path / 'ages_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'tools', 'ages_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    assert 'runtime error' not in done.stderr and 'Sanitizer' not in done.stderr
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused: ' in line]
    assert len(refused) >= 24 and sum(' accepted' in line for line in lines) >= 9
    for word in ('at least 1', 't0 must be finite', 'a_lo and a_hi must be finite', 'below a_hi',
                 'a_hi - a_lo', '2^31', 'ne must be at least 1', 'K is null', 'not finite'):
        assert any(word in line for line in refused), word
    assert any(line.startswith('1 pixel, 2^31 - 1 records accepted') for line in lines)
    assert any(line.startswith('1 pixel, 2^31 records refused') for line in lines)
    # the plan: every case of the issue at both LDS sizes, and the restatement's copy of the rule
    plans = [re.fullmatch(r'plan lds (\d+) planes (\d+) ne (\d+): stride (\d+) run (\d+) chunk (\d+) '
                          r'bytes (\d+)', line) for line in lines]
    plans = [tuple(int(v) for v in m.groups()) for m in plans if m]
    assert len(plans) == 12
    for lds in (65536, 163840):
        shapes = {(p[1], p[2]) for p in plans if p[0] == lds}
        assert {(3, 1), (66, 1), (66, 1000)} <= shapes and len(shapes) == 6
        most = max(p[1] for p in plans if p[0] == lds)
        assert (most | 1)*16 + most*8 <= lds < ((most + 1) | 1)*16 + (most + 1)*8
    for lds, planes_, ne, stride, run, chunk, nbytes in plans:
        assert (stride, run, chunk) == apply_plan(planes_, ne, lds)
        assert (stride, run, chunk) == hip_api.ages_apply_plan(planes_, ne, lds)
        assert nbytes == run*stride*16 + planes_*chunk*8 <= lds
    assert sum('does not fit' in line for line in lines) == 4
    assert hip_api.ages_apply_plan(2731, 1, 65536) is None and hip_api.ages_apply_plan(3, 0) is None
    assert hip_api.ages_apply_plan(66, 64) == (67, 15, 30)


# The complete text of every refusal of the one check (nxc_ages_check.hpp) per subject, as each
# subject's driver under tests/tools prints it: {driver: {the driver's case: the refusal}}.  Written
# down from what the drivers printed while each subject still had a check header of its own.
REFUSALS = {
    'ages_check': {
        'no pixels': 'age cube: the image has no pixels',
        'na = 0': 'age cube: na must be at least 1',
        't0 NaN': 'age cube: t0 must be finite',
        'a_lo NaN': 'age cube: a_lo and a_hi must be finite',
        'empty range': 'age cube: a_lo must be below a_hi',
        'width overflows': 'age cube: a_hi - a_lo must be finite',
        '1 pixel, 2^31 records': 'age cube: n_pix * (na + 2) must be below 2^31 records',
        'na = INT64_MAX': 'age cube: n_pix * (na + 2) must be below 2^31 records',
        'ne = 0': 'age cube: ne must be at least 1',
        'ne = 2^31': 'age cube: ne must be below 2^31',
        'K null': 'age cube: K is null',
        'K with a NaN at its end': 'age cube: K holds a value that is not finite',
    },
    'density_ages_check': {
        'no points': 'density ages: the index has no points',
        'na = 0': 'density ages: na must be at least 1',
        't0 NaN': 'density ages: t0 must be finite',
        'a_lo NaN': 'density ages: a_lo and a_hi must be finite',
        'empty range': 'density ages: a_lo must be below a_hi',
        'width overflows': 'density ages: a_hi - a_lo must be finite',
        '1 point, 2^31 records': 'density ages: n_points * (na + 2) must be below 2^31 records',
        'n_points = INT64_MAX': 'density ages: n_points * (na + 2) must be below 2^31 records',
    },
    'los_ages_check': {
        'no spectra': 'line-of-sight ages: S must be at least 1',
        'na = 0': 'line-of-sight ages: na must be at least 1',
        't0 NaN': 'line-of-sight ages: t0 must be finite',
        'a_lo NaN': 'line-of-sight ages: a_lo and a_hi must be finite',
        'empty range': 'line-of-sight ages: a_lo must be below a_hi',
        'width overflows': 'line-of-sight ages: a_hi - a_lo must be finite',
        '1 spectrum, 2^31 records': 'line-of-sight ages: S * (na + 2) must be below 2^31 records',
        'S = INT64_MAX': 'line-of-sight ages: S * (na + 2) must be below 2^31 records',
    },
    'shell_ages_check': {
        'no records': 'shell ages: the map has no records',
        'na = 0': 'shell ages: na must be at least 1',
        't0 NaN': 'shell ages: t0 must be finite',
        'a_lo NaN': 'shell ages: a_lo and a_hi must be finite',
        'empty range': 'shell ages: a_lo must be below a_hi',
        'width overflows': 'shell ages: a_hi - a_lo must be finite',
        '1 record, 2^31 age records':
            'shell ages: nlon * nlat * (nalt + 2) * (na + 2) must be below 2^31 records',
        'records = INT64_MAX':
            'shell ages: nlon * nlat * (nalt + 2) * (na + 2) must be below 2^31 records',
    },
}


@pytest.mark.parametrize('driver', sorted(REFUSALS))
def test_every_refusal_text_per_subject(tmp_path, driver):
    """One check composes the refusals of the four subjects from their words (AgesSubject); every
    text is, byte for byte, what the subject's own check said, and no case of a driver is refused
    with a text outside the table."""
    exe = tmp_path / driver
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', driver + '.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    got = dict(line.split(' refused: ', 1) for line in done.stdout.splitlines()
               if ' refused: ' in line)
    for case, text in REFUSALS[driver].items():
        assert got[case] == text, case
    assert set(got.values()) == set(REFUSALS[driver].values())


def test_the_library_exports_the_entry_points():
    from nexoclom_amd import hip_api
    names = [f'nxc_{which}_ages_{what}' for which in ('image', 'camera')
             for what in ('enable', 'accumulate', 'accumulate_f32', 'accumulate_rows', 'download',
                          'apply')]
    assert len(names) == 12 and all(name in hip_api.EXPORTS for name in names)
    lib = hip_api.load_library()
    assert all(hasattr(lib, name) for name in names)
    with open(os.path.join(HERE, '..', 'include', 'nexoclom_hip.h')) as f:
        header = f.read()
    assert 'Age cube' in header and all(f'int {name}(' in header for name in names)
    assert hip_api.ABI_VERSION == 3
