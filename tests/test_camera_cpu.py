"""CameraImage without a GPU: the definition (tests/camera_restatement.py, written from
include/nexoclom_hip.h) on hand cases and in its far-field limit against the orthographic
create_image; CameraImage's params and refusals; the host-only check of nxc_camera_desc as a
stand-alone program; the ctypes mirror of the descriptor."""
import contextlib
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle
from tests.camera_restatement import camera_image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')
HEADER = os.path.join(ROOT, 'include', 'nexoclom_hip.h')
UNIT_CM = 2440e5
EYE = np.eye(3)                       # right = +x, boresight = +y, up = +z
G_TABLES = [(np.array([-5e-3, -1e-3, 2e-3, 6e-3]), np.array([3., 7., 5., 2.])),
            (np.array([-4e-3, 0., 4e-3]), np.array([1., 4., 2.]))]


def one(p, o, basis=EYE, quantity='column', frac=0.37, vy=1e-3, dims=(5, 3), half=(0.5, 0.3)):
    ue = np.linspace(-half[0], half[0], dims[0] + 1)
    ve = np.linspace(-half[1], half[1], dims[1] + 1)
    du, dv = 2*half[0]/dims[0], 2*half[1]/dims[1]
    res = camera_image([p[0]], [p[1]], [p[2]], [vy], [frac], o, basis, ue, ve, 2e-4,
                       du*dv*UNIT_CM**2, quantity, G_TABLES)
    return res, du, dv


# ---- 1. hand cases ------------------------------------------------------------------------------
def test_packet_on_the_boresight():
    res, du, dv = one((0., -2., 0.), (0., -5., 0.))
    assert res.samples == 1 and res.binned == 1
    assert res.counts.sum() == 1 and res.counts[2, 1] == 1
    np.testing.assert_allclose(res.image[2, 1], 0.37/(du*dv*3.0**2*UNIT_CM**2), rtol=1e-14, atol=0)


def test_packet_against_a_line_of_sight_cone():
    """The same packet seen by compute_iteration's cone along the camera's boresight: both spread
    its weight over an area at its distance, pi (r sin dphi)^2 there and du dv r^2 here."""
    dphi = np.radians(1.0)
    p, o = (0., -2., 0.), (0., -5., 0.)
    res, du, dv = one(p, o, quantity='radiance')
    samples = {k: np.array([v]) for k, v in zip(('x', 'y', 'z', 'vy', 'frac'), (*p, 1e-3, 0.37))}
    sc = dict(x=np.array([o[0]]), y=np.array([o[1]]), z=np.array([o[2]]),
              xbore=np.array([0.]), ybore=np.array([1.]), zbore=np.array([0.]))
    rad, npack, _, _ = np_oracle.los_iteration(samples, sc, dphi, 20., 2e-4, G_TABLES, UNIT_CM)
    assert npack[0] == 1 and rad[0] > 0
    np.testing.assert_allclose(res.image[2, 1]/rad[0], np.pi*np.sin(dphi)**2/(du*dv),
                               rtol=1e-13, atol=0)


def test_occultation_and_the_half_space_behind_the_camera():
    hidden, _, _ = one((0., 2., 0.), (0., -3., 0.))
    assert hidden.counts[2, 1] == 1 and hidden.binned == 1 and hidden.image[2, 1] == 0.0
    front, _, _ = one((0., -2., 0.), (0., -3., 0.))
    assert front.counts[2, 1] == 1 and front.image[2, 1] > 0
    behind, _, _ = one((0., -4., 0.), (0., -3., 0.))
    assert behind.samples == 1 and behind.binned == 0 and behind.counts.sum() == 0
    # beside the planet, farther away than it: not hidden
    beside, _, _ = one((2.4, 2., 0.), (0., -3., 0.))
    assert beside.binned == 1 and beside.image.sum() > 0


def test_shadow_only_in_radiance():
    from nexoclom_amd.CameraImage import camera_basis
    basis = camera_basis((-1., 0., 0.), (0., 0., 1.))
    p, o = (0.5, 2., 0.), (3., 2., 0.)            # inside the shadow cylinder, in plain view
    dark, _, _ = one(p, o, basis, 'radiance')
    assert dark.counts[2, 1] == 1 and dark.image[2, 1] == 0.0
    column, _, _ = one(p, o, basis, 'column')
    assert column.counts[2, 1] == 1 and column.image[2, 1] > 0
    lit, _, _ = one((1.5, 2., 0.), o, basis, 'radiance')
    assert lit.image[2, 1] > 0


def test_nonfinite_weights_are_dropped():
    res, _, _ = one((0., -2., 0.), (0., -5., 0.), frac=np.inf)
    assert res.binned == 0 and res.counts.sum() == 0


# ---- 2. far-field limit: the orthographic image -----------------------------------------------------
E, D = 10.0, 1e8
FAR_SEED = 3


def far_field_cloud(seed, n=6000):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = np.where(np.arange(n) % 2 == 0, rng.uniform(1.0, 3.0, n), rng.uniform(1.0, E, n))
    p = u*r[:, None]
    return p[:, 0], p[:, 1], p[:, 2], rng.uniform(-4e-3, 5e-3, n), rng.uniform(0.1, 1.0, n)


@pytest.mark.parametrize('quantity', ['column', 'radiance'])
def test_far_field_limit_is_create_image(quantity):
    """A camera at distance D along the observer's line of sight, with the frame scaled by 1/D.
    With d_c = M p + (0, D, 0): u D = x_obs / (1 + y_obs / D) differs from x_obs by at most
    E^2 / D; foot = d_c^3 / r lies between d_c^2 (1 - rho^2 / (2 d_c^2)) and d_c^2 with
    d_c^2 = D^2 (1 + y_obs / D)^2, so foot du dv differs from Apix by at most 2.1 E / D relative; the
    camera's occultation test differs from `inview` only within E^2 / D of the limb."""
    M = np_oracle.image_rotation(0.7, 0.4)
    assert np.all(np.abs(M) > 1e-3)
    x, y, z, vy, frac = far_field_cloud(FAR_SEED)
    dims, width = (24, 17), 24.0
    assert width > 2*E*(1 + E/D)
    xr = zr = (-width/2, width/2)
    xedges = np.linspace(xr[0], xr[1], dims[0] + 1)
    zedges = np.linspace(zr[0], zr[1], dims[1] + 1)
    apix = (width/dims[0])*(width/dims[1])*UNIT_CM**2
    # the condition: nothing within 2 E^2 / D of a bin edge or of the limb
    obs = np.stack([(M[r, 0]*x + M[r, 1]*y) + M[r, 2]*z for r in range(3)])
    tol = 2*E**2/D
    assert np.min(np.abs(obs[0][:, None] - xedges[None, :])) > tol
    assert np.min(np.abs(obs[2][:, None] - zedges[None, :])) > tol
    assert np.min(np.abs(np.hypot(obs[0], obs[2]) - 1.0)) > tol
    assert np.min(np.abs(obs[1])) > tol

    image, counts, _, _ = np_oracle.create_image(x, y, z, vy, frac, 2e-4, M, quantity, G_TABLES,
                                                 dims, xr, zr, apix, matmul=False)
    o = M.T @ np.array([0., -D, 0.])
    cam = camera_image(x, y, z, vy, frac, o, M, xedges/D, zedges/D, 2e-4,
                       (width/dims[0]/D)*(width/dims[1]/D)*UNIT_CM**2, quantity, G_TABLES)
    assert cam.binned == len(x) == counts.sum()
    assert np.array_equal(cam.counts, counts)
    assert np.count_nonzero(image) > 200
    hidden = ~((np.hypot(obs[0], obs[2]) > 1) | (obs[1] < 0))
    assert hidden.sum() > 50                                       # occulted samples take part
    np.testing.assert_allclose(cam.image, image, rtol=3*E/D, atol=0)


# ---- 3. CameraImage: params and refusals --------------------------------------------------------------
def make_inputs():
    from nexoclom_amd import Input
    return Input(INPUT)


def build(params, **kw):
    from nexoclom_amd import CameraImage
    with contextlib.redirect_stdout(io.StringIO()):
        return CameraImage(make_inputs(), params, context=object(), **kw)


GOOD = dict(quantity='column', observer='0,-3,0.5', fov='40,30', dims='8,6')


def test_params_make_the_frame():
    cam = build(GOOD)
    assert cam.image.shape == cam.packet_image.shape == (8, 6) and not cam.image.any()
    np.testing.assert_allclose(cam.basis @ cam.basis.T, np.eye(3), atol=1e-15)
    bore = -np.array([0., -3., 0.5])/np.linalg.norm([0., -3., 0.5])
    np.testing.assert_allclose(cam.basis[1], bore, atol=1e-15)
    np.testing.assert_allclose(np.cross(cam.basis[0], cam.basis[1]), cam.basis[2], atol=1e-15)
    assert cam.basis[2][2] > 0                                   # up is up
    assert len(cam.uedges) == 9 and len(cam.vedges) == 7
    np.testing.assert_allclose(cam.uedges[[0, -1]], [-np.tan(np.radians(20)), np.tan(np.radians(20))])
    np.testing.assert_allclose(cam.vedges[[0, -1]], [-np.tan(np.radians(15)), np.tan(np.radians(15))])
    np.testing.assert_allclose(cam.uedges, -cam.uedges[::-1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(cam.pix_area_cm2, np.diff(cam.uedges)[0]*np.diff(cam.vedges)[0]
                               * (cam.unit_km*1e5)**2)
    # the pixels' solid angles add up to that of the rectangular field of view
    a, b = cam.uedges[-1], cam.vedges[-1]
    np.testing.assert_allclose(cam.pixel_solid_angle.sum(), 4*np.arcsin(a*b/np.sqrt((1+a*a)*(1+b*b))),
                               rtol=2e-3)
    rays = cam.pixel_boresights()
    assert rays.shape == (8, 6, 3)
    np.testing.assert_allclose(np.linalg.norm(rays, axis=2), 1.0, atol=1e-15)
    centre = 0.25*(rays[3, 2] + rays[4, 2] + rays[3, 3] + rays[4, 3])
    np.testing.assert_allclose(centre/np.linalg.norm(centre), bore, atol=1e-12)
    assert cam.totalsource == 0 and cam.atoms_per_packet == 0


def test_explicit_boresight_up_and_defaults():
    cam = build(dict(GOOD, boresight='1,0,0', up='0,1,0'))
    np.testing.assert_allclose(cam.basis, [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-15)
    cam = build({k: v for k, v in GOOD.items() if k != 'dims'})
    assert cam.image.shape == (256, 256)


@pytest.mark.parametrize('change, text', [
    (dict(observer=None), 'observer'),
    (dict(observer='0,-0.5,0.2'), 'outside the planet'),
    (dict(observer='0,-3'), 'observer'),
    (dict(observer='0,0,3'), 'parallel'),                        # boresight -z, up +z
    (dict(boresight='0,2,0', up='0,-1,0'), 'parallel'),
    (dict(boresight='0,0,0'), 'zero vector'),
    (dict(fov=None), 'fov'),
    (dict(fov='180,30'), 'fov'),
    (dict(fov='40,0'), 'fov'),
    (dict(fov='40'), 'fov'),
    (dict(dims='0,6'), 'dims'),
    (dict(dims='8,9000'), 'dims'),
    (dict(dims='8'), 'dims'),
    (dict(quantity='density'), 'quantity'),
])
def test_refused_params(change, text):
    from nexoclom_amd import InputError
    params = {k: v for k, v in dict(GOOD, **change).items() if v is not None}
    with pytest.raises(InputError) as err:
        build(params)
    assert text in str(err.value)


@pytest.mark.parametrize('kw', [dict(npackets=1000), dict(cp=object()), dict(shard=(0, 10)),
                                dict(tiles=True), dict(projection='fisheye'), dict(moons=True)])
def test_out_of_scope_keywords_are_refused(kw):
    with pytest.raises(NotImplementedError):
        build(GOOD, **kw)
    with pytest.raises(NotImplementedError):
        build(dict(GOOD, projection='fisheye'))
    with pytest.raises(TypeError):
        build(GOOD, no_such_keyword=1)


# ---- 4. the C side's refusals, as a host program --------------------------------------------------------
def test_descriptor_check_as_a_host_program(tmp_path):
    """nxc_camera_set's refusals are host-only code (nxc_camera_check.hpp);
    tests/tools/camera_check.cpp feeds it good descriptors and one bad one per refusal.  Built
    plainly here; the same file is what is built with -fsanitize=address,undefined to check the
    host code's memory accesses."""
    exe = tmp_path / 'camera_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', 'camera_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    refused = [line for line in done.stdout.splitlines() if ' refused: ' in line]
    assert len(refused) >= 20
    for word in ('finite', '|o| >= 1', 'orthonormal', 'dims', 'increase', 'symmetric', 'n_lines',
                 'g-value table'):
        assert any(word in line for line in refused), word


# ---- 5. ABI ---------------------------------------------------------------------------------------------
def test_camera_desc_mirror_matches_the_compiled_header(tmp_path):
    from nexoclom_amd import hip_api
    ct = hip_api.nxc_camera_desc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("%zu", sizeof(nxc_camera_desc));']
    lines += [f'printf(" %zu", offsetof(nxc_camera_desc, {field}));' for field, *_ in ct._fields_]
    lines.append('printf("\\n"); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', str(src), '-o', str(exe)])
    size, *offsets = subprocess.check_output([str(exe)], text=True).split()
    assert int(size) == C.sizeof(ct) == 14*8 + 2*4 + 2*8 + 2*8 + 4*8 + 8*8
    assert [int(v) for v in offsets] == [getattr(ct, f).offset for f, *_ in ct._fields_]
    for name in ('nxc_camera_set', 'nxc_camera_accumulate', 'nxc_camera_accumulate_f32',
                 'nxc_camera_accumulate_rows', 'nxc_camera_download'):
        assert name in hip_api.EXPORTS
