"""The velocity cube without a GPU: the restatement against itself and against the pixel moments,
the host side of cube= (cube_from_sums, the refusals, bad arguments) and the host-only argument
check of nxc_*_cube_enable as a stand-alone program."""
import contextlib
import io
import os
import subprocess

import numpy as np
import pytest

import nexoclom_amd
from nexoclom_amd.ModelImage import cube_from_sums, parse_cube
from oracle import np_oracle
from tests.pixel_cube_restatement import camera_cube, image_cube, planes
from tests.pixel_moments_restatement import image_moments

HERE = os.path.dirname(os.path.abspath(__file__))
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
EPS = 2.0**-52
R_KM = 2440.53


def cloud(n, seed, extent=6.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = d*rng.uniform(1.0, extent, n)[:, None]
    v = rng.normal(size=(n, 3))*2.0/R_KM
    return p[:, 0], p[:, 1], p[:, 2], v[:, 0], v[:, 1], v[:, 2], rng.uniform(0.1, 1.0, n)


IMAGE_ARGS = (2e-4, np_oracle.image_rotation(0.7, 0.4), 'column', [], (16, 12), (-4., 4.), (-4., 4.),
              1.0)


# ---- 1. the restatement ---------------------------------------------------------------------------
def test_the_bin_rule():
    """Planes of hand-picked velocities, nv = 4 over [-2, 2): dv = 1."""
    v = np.array([-2.0, -2.0 - 1e-12, -1.000001, -1.0, 0.0, -0.0, 1.999999, 2.0, 7.0, np.nan,
                  np.inf, -np.inf])
    k, guard = planes(v, 4, -2.0, 2.0)
    assert list(k) == [1, 0, 1, 2, 3, 3, 4, 5, 5, 5, 5, 0]
    assert guard == 0.0                                   # samples sit exactly on edges
    k, guard = planes(np.array([0.25, -0.5]), 4, -2.0, 2.0)
    assert list(k) == [3, 2] and guard == 0.25
    assert planes(np.array([5.0, np.nan]), 4, -2.0, 2.0)[1] == np.inf


@pytest.mark.parametrize('nv,v_lo,v_hi', [(1, -0.01, 0.01), (7, -0.0008, 0.0008), (64, 0.0, 0.0005)])
def test_the_planes_sum_to_the_image(nv, v_lo, v_hi):
    """Every sample that adds w to image[pix] adds w to exactly one plane of pix."""
    cols = cloud(20000, 5)
    res = image_cube(*cols, *IMAGE_ARGS, nv, v_lo, v_hi)
    assert res.binned > 5000 and res.sums.shape == (16, 12, nv + 2, 2)
    np.testing.assert_allclose(res.sums[..., 0].sum(-1), res.image, rtol=1e-12, atol=0)
    np.testing.assert_allclose(res.abs_sums[..., 0].sum(-1), res.image, rtol=1e-12, atol=0)
    if nv == 1:
        assert not res.sums[:, :, [0, -1]].any()          # the range holds every sample
    else:
        assert res.sums[:, :, 0, 0].sum() > 0 and res.sums[:, :, -1, 0].sum() > 0

    from nexoclom_amd.CameraImage import camera_basis
    o = np.array([1.5, -6.0, 2.0])
    ue, ve = np.linspace(-0.4, 0.4, 9), np.linspace(-0.3, 0.3, 7)
    cam = camera_cube(*cols, o, camera_basis(-o, (0, 0, 1)), ue, ve, 2e-4, 1.0, 'column', (), nv,
                      v_lo, v_hi)
    assert cam.binned > 500 and cam.sums.shape == (8, 6, nv + 2, 2)
    np.testing.assert_allclose(cam.sums[..., 0].sum(-1), cam.image, rtol=1e-12, atol=0)


def test_cube_mean_and_variance_against_the_moments():
    """With positive weights (quantity column) and a range that holds every sample, the cube knows
    each sample's velocity v_i only as its bin's centre c_i, |c_i - v_i| <= dv/2.  Per pixel, with
    p_i = w_i / S0 and e_i = c_i - v_i:

      mean      |sum p_i c_i - sum p_i v_i| = |sum p_i e_i| <= dv/2.
      variance  c_i - mean_c = (v_i - mean) + (e_i - e_bar), so
                var_c = var + 2 sum p_i (v_i - mean)(e_i - e_bar) + sum p_i (e_i - e_bar)^2.
                The last sum is the variance of a quantity confined to an interval of length dv,
                which is at most dv^2/4; by Cauchy-Schwarz the middle term is at most
                2 sqrt(var) sqrt(dv^2/4) = dv sqrt(var).  Hence
                |var_c - var| <= dv sqrt(var) + dv^2/4        (equivalently |sigma_c - sigma| <= dv/2).

    A theorem, not a tolerance.  Rounding is allowed for separately: the moments' variance is
    m2/S0 - u^2, each term a sum of n positive terms and a quotient, so it carries at most
    (n + 4) EPS (m2/S0 + u^2); the cube's sums and the bin rule's t carry the same order."""
    nv, v_lo, v_hi = 16, -0.008, 0.008
    dv = (v_hi - v_lo)/nv
    cols = cloud(20000, 7)
    assert np.abs(np.stack(cols[3:6])).max()*np.sqrt(3) < v_hi       # |vlos| <= |v| < v_hi
    res = image_cube(*cols, *IMAGE_ARGS, nv, v_lo, v_hi)
    mom = image_moments(*cols, *IMAGE_ARGS)
    assert not res.sums[:, :, [0, -1]].any()
    lit = res.image > 0
    assert lit.sum() > 150 and np.all(res.sums[..., 0] >= 0)
    S = res.sums[..., 1:-1, 0][lit]
    S0 = res.image[lit]
    centres = v_lo + (np.arange(nv) + 0.5)*dv
    mean_c = (S*centres).sum(-1)/S.sum(-1)
    var_c = (S*(centres - mean_c[:, None])**2).sum(-1)/S.sum(-1)
    u, q2 = mom.sums[..., 0][lit]/S0, mom.sums[..., 1][lit]/S0
    var = q2 - u*u
    n = res.counts.max()
    slack = 4*(n + 4)*EPS*(q2 + u*u + v_hi**2)
    assert np.all(np.abs(mean_c - u) <= dv/2 + 4*(n + 4)*EPS*v_hi)
    assert np.all(np.abs(var_c - var) <= dv*np.sqrt(np.maximum(var, 0)) + dv*dv/4 + slack)
    # the bounds are not idle: binning moves the mean by a fair part of dv/2 somewhere
    assert np.abs(mean_c - u).max() > 0.05*dv


# ---- 2. the host side of cube= --------------------------------------------------------------------
def test_cube_from_sums():
    sums = np.zeros((2, 3, 5, 2))
    sums[0, 1, :, 0] = [1., 2., 0., 4., 8.]
    sums[0, 1, :, 1] = [1., 2., 0., 4., 16.]
    got = cube_from_sums(sums, 10.0, -3.0, 3.0)
    assert tuple(got) == ('cube', 'cube_below', 'cube_above', 'velocity_edges', 'velocity_axis',
                          'cube_effective_packets')
    assert got['cube'].shape == (2, 3, 3) and got['cube_below'].shape == (2, 3)
    assert list(got['cube'][0, 1]) == [20., 0., 40.]
    assert got['cube_below'][0, 1] == 10. and got['cube_above'][0, 1] == 80.
    assert list(got['velocity_edges']) == [-3., -1., 1., 3.]
    assert list(got['velocity_axis']) == [-2., 0., 2.]
    assert list(got['cube_effective_packets'][0, 1]) == [2., 0., 4.]
    assert not got['cube'][1].any() and not got['cube_effective_packets'][1].any()


def test_parse_cube():
    assert parse_cube((-10, 10, 64)) == (-10.0, 10.0, 64)
    assert parse_cube([0.5, 1.5, np.int64(3)]) == (0.5, 1.5, 3)


BAD_CUBES = [(-10, 10), (-10, 10, 64, 1), 'abc', 5, (-10, 10, 2.5), (-10, 10, 64.0), (-10, 10, 0),
             (-10, 10, -4), (10, -10, 4), (5, 5, 3), (np.nan, 1, 4), (0, np.inf, 4), (-np.inf, 0, 4),
             ('a', 1, 4), (-1.7e308, 1.7e308, 4)]


def make_inputs():
    from nexoclom_amd import Input
    return Input(INPUT)


IMAGE = dict(quantity='column', dims='8,6')
CAMERA = dict(quantity='column', observer='0,-3,0.5', fov='40,30', dims='8,6')
CUBE = (-10, 10, 5)


@pytest.mark.parametrize('bad', BAD_CUBES, ids=[str(b) for b in BAD_CUBES])
def test_a_bad_cube_is_refused_before_a_context_is_opened(bad):
    """No context is given and this machine may have no device: a ValueError, nothing else."""
    from nexoclom_amd import CameraImage, ModelImage
    from nexoclom_amd.input_classes import InputError
    with pytest.raises(ValueError):
        parse_cube(bad)
    for build in (lambda: ModelImage(make_inputs(), IMAGE, cube=bad),
                  lambda: make_inputs().produce_image(IMAGE, cube=bad),
                  lambda: CameraImage(make_inputs(), CAMERA, cube=bad)):
        with pytest.raises((ValueError, InputError)) as err:
            build()
        assert 'cube=' in str(err.value)


def test_a_cube_with_too_many_records_is_refused_on_the_host():
    from nexoclom_amd import ModelImage
    with pytest.raises(ValueError) as err:
        ModelImage(make_inputs(), dict(quantity='column', dims='4096,4096'), cube=(-10, 10, 126))
    assert '2^31' in str(err.value)


@pytest.mark.parametrize('kw', [dict(npackets=1000), dict(shard=(0, 10)), dict(moments=True)])
def test_model_image_refuses_cube_with(kw):
    from nexoclom_amd import ModelImage
    with pytest.raises(NotImplementedError) as err:
        ModelImage(make_inputs(), IMAGE, context=object(), cube=CUBE, **kw)
    assert 'cube=' in str(err.value) and next(iter(kw)) in str(err.value)


@pytest.mark.parametrize('kw', [dict(npackets=1000), dict(shard=(0, 10)), dict(cp=object()),
                                dict(moments=True)])
def test_camera_image_refuses_cube_with(kw):
    from nexoclom_amd import CameraImage
    with pytest.raises(NotImplementedError) as err:
        CameraImage(make_inputs(), CAMERA, context=object(), cube=CUBE, **kw)
    assert 'cube=' in str(err.value) and next(iter(kw)) in str(err.value)


@pytest.mark.parametrize('kw', [dict(cp=object()), dict(moments=True)])
def test_produce_image_refuses_cube_with(kw):
    with pytest.raises(NotImplementedError) as err:
        make_inputs().produce_image(IMAGE, context=object(), cube=CUBE, **kw)
    assert 'cube=' in str(err.value) and next(iter(kw)) in str(err.value)


def test_cube_is_keyword_only_and_an_empty_catalogue_gives_an_empty_cube():
    from nexoclom_amd import CameraImage, ModelImage
    with contextlib.redirect_stdout(io.StringIO()):
        image = ModelImage(make_inputs(), IMAGE, context=object(), cube=CUBE)
        cam = CameraImage(make_inputs(), CAMERA, context=object(), cube=CUBE)
        plain = ModelImage(make_inputs(), IMAGE, context=object())
    for obj in (image, cam):
        assert obj.cube_sums.shape == (8, 6, 7, 2) and not obj.cube_sums.any()
        assert obj.cube.shape == (8, 6, 5) and obj.cube_below.shape == (8, 6) == obj.cube_above.shape
        assert obj.cube_effective_packets.shape == (8, 6, 5) and not obj.cube_effective_packets.any()
        np.testing.assert_allclose(obj.velocity_edges, [-10, -6, -2, 2, 6, 10], rtol=4*EPS)
        np.testing.assert_allclose(obj.velocity_axis, [-8, -4, 0, 4, 8], atol=8*EPS*10)
        assert not hasattr(obj, 'moment_sums')
    assert plain.cube is None and not hasattr(plain, 'cube_sums')
    assert not hasattr(plain, 'velocity_axis')


# ---- 3. the C side's argument check, as a host program ------------------------------------------------
def test_argument_check_as_a_host_program(tmp_path):
    """nxc_*_cube_enable's refusals are host-only code (nxc_cube_check.hpp);
    tests/tools/cube_check.cpp feeds it good arguments, one bad set per refusal, and nv one below and
    at the 2^31 record limit for several image sizes.  Built plainly here; the same file is what is
    built with -fsanitize=address,undefined to check the host code."""
    exe = tmp_path / 'cube_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', 'cube_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused: ' in line]
    assert len(refused) >= 16 and sum(' accepted' in line for line in lines) >= 7
    for word in ('at least 1', 'finite', 'below v_hi', 'v_hi - v_lo', '2^31'):
        assert any(word in line for line in refused), word
    assert any(line.startswith('1 pixel, 2^31 - 1 records accepted') for line in lines)
    assert any(line.startswith('1 pixel, 2^31 records refused') for line in lines)


def test_the_library_exports_the_ten_entry_points():
    from nexoclom_amd import hip_api
    names = [f'nxc_{which}_cube_{what}' for which in ('image', 'camera')
             for what in ('enable', 'accumulate', 'accumulate_f32', 'accumulate_rows', 'download')]
    assert all(name in hip_api.EXPORTS for name in names)
    with open(os.path.join(HERE, '..', 'include', 'nexoclom_hip.h')) as f:
        header = f.read()
    assert 'Velocity cube' in header and all(f'int {name}(' in header for name in names)
