"""The device buffers of one handle through a second configuration: set_image, camera_set and
density_set at one size with their moments, cube and spectrum enabled and used, then at a smaller
size on the same Context -- and everything the second configuration downloads must be what a fresh
Context, given only that configuration, downloads.  Nothing here provokes a failure or allocates
anything large: 65 samples (one wave and one lane), 7 x 5 then 3 x 2 pixels, 12 then 3 points.

Comparison rule: packet counts, rows per point and rows per record (a pass with frac = 1 leaves
them in plane 0 of the spectrum) are equal exactly; floating-point sums are held to the bounds of
the consumers' own tests -- 1e-11 * sum |term| for the pixel sums (tests/test_gpu_pixel_moments.py,
tests/test_gpu_pixel_cube.py), (n - 1) 2^-52 sum |term| for the density sums
(tests/density_moments_restatement.py, tests/density_spectrum_restatement.py) -- against the
restatement and, with the same bound, between the two Contexts."""
import numpy as np
import pytest

from nexoclom_amd import hip_api
from nexoclom_amd.ModelDensity import DensityIndex
from tests import density_moments_restatement as moments_restatement
from tests import density_spectrum_restatement as spectrum_restatement
from tests import helpers as H
from tests import test_gpu_density_moments as density_moments
from tests import test_gpu_density_spectrum as density_spectrum
from tests import test_gpu_pixel_cube as cube
from tests import test_gpu_pixel_moments as moments
from tests.test_gpu_pixel_moments import RTOL, dress, tables

pytestmark = pytest.mark.gpu
P = 65
CUBE = (3,) + cube.WIDE
BINS = (4, 1.5e-4, 4.5e-4)
DR = 0.1


def refused(call, entry):
    with pytest.raises(hip_api.HipError) as err:
        call()
    assert err.value.code == hip_api.NXC_ERR_STATE
    assert f'{entry} has not been called' in str(err.value)


def pixel_case(forces, which, dims, seed):
    """The two scenes of one grid, 65 samples inside its frame, and what the restatements say."""
    scene, cube_scene = moments.SCENES[which](forces, dims=dims), cube.SCENES[which](forces, dims=dims)
    rng = np.random.default_rng(seed)
    cols = dress(scene.place(rng.uniform(-0.8, 0.8, P), rng.uniform(-0.8, 0.8, P),
                             rng.uniform(0.0, 1.0, P)), rng)
    quantity, gt = tables(forces, 'two')
    want_m = moments.restate(scene, cols, quantity, gt)
    want_c = cube.restate(cube_scene, cols, quantity, gt, CUBE)
    assert want_m.binned == P == want_c.binned and np.count_nonzero(want_c.sums[..., 1:-1, 0]) > 0
    return scene, cube_scene, cols, quantity, gt, want_m, want_c


def pixels(ctx, forces, which, dims, seed):
    """One configuration of the image or the camera: the set, the refusals before the enables, zeroed
    moments and cube of the new shapes, one pass through each; every download, and what the
    restatements say."""
    scene, cube_scene, cols, quantity, gt, want_m, want_c = pixel_case(forces, which, dims, seed)
    entry = 'nxc_image' if which == 'image' else 'nxc_camera'
    scene.set(ctx, quantity, gt, enable=False)
    refused(lambda: scene.moments(ctx), f'{entry}_moments_enable')
    refused(lambda: cube_scene.download(ctx), f'{entry}_cube_enable')
    scene.enable(ctx)
    cube_scene.enable(ctx, *CUBE)
    zero_m, zero_c = scene.moments(ctx), cube_scene.download(ctx)
    assert zero_m.shape == dims + (4,) and not zero_m.any()
    assert zero_c.shape == dims + (CUBE[0] + 2, 2) and not zero_c.any()
    scene.accumulate(ctx, *cols)
    cube_scene.accumulate(ctx, *cols)
    got = dict(pair=scene.pair(ctx), moments=scene.moments(ctx), cube=cube_scene.download(ctx))

    image, counts = got['pair']                       # two passes added to the pair
    assert counts.shape == dims and np.array_equal(counts, 2*want_m.counts)
    np.testing.assert_allclose(image, 2*want_m.image, rtol=RTOL, atol=0)
    moments.compare_sums(got['moments'], want_m)
    cube.compare_cube(got['cube'], want_c)
    return got, want_m, want_c


def same_pixels(got, fresh, want_m, want_c):
    assert np.array_equal(got['pair'][1], fresh['pair'][1])
    np.testing.assert_allclose(got['pair'][0], fresh['pair'][0], rtol=RTOL, atol=0)
    moments.compare_sums(got['moments'], want_m, reference=fresh['moments'])
    cube.compare_cube(got['cube'], want_c, reference=fresh['cube'])


def density_case(q, seed):
    """q points, 65 rows around them, an all-sky spectrum of four bins, and the restatements."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(-1, 1, (q, 3))
    cols = density_moments.make_rows(
        rng, P, xyz=points[rng.integers(q, size=P)] + rng.normal(0, 0.03, (P, 3)))
    spec = density_spectrum.cone_spec(rng, q, all_sky=True, bins=BINS)
    want_m = moments_restatement.restate(points, DR, *cols)
    want_s = spectrum_restatement.restate(points, DR, *spec, *cols)
    assert want_m.counts.sum() >= P // 2 and want_s.seen.sum() == want_s.counts.sum()
    assert np.count_nonzero(want_s.seen[:, 1:-1].sum(axis=0)) >= 2
    return points, cols, spec, want_m, want_s


def density(ctx, q, seed):
    """One configuration of ModelDensity: q points, the moments, then a four-bin spectrum that is
    switched off and on again; one pass through each, and a third with frac = 1 for the rows per
    record."""
    points, cols, spec, want_m, want_s = density_case(q, seed)
    frames, nv, s_lo, s_hi, cos_half, all_sky = spec
    index = DensityIndex(points, DR)
    ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
    refused(ctx.density_moments_download, 'nxc_density_moments_enable')
    refused(ctx.density_spectrum_download, 'nxc_density_spectrum_enable')

    def spectrum_on():
        ctx.density_spectrum_enable(nv, s_lo, s_hi, cos_half, all_sky, frames[index.order])
        zero = ctx.density_spectrum_download()
        assert zero.shape == (2, q, nv + 2, 2) and not zero.any()

    ctx.density_moments_enable()
    spectrum_on()
    ctx.density_spectrum_enable(0)
    refused(ctx.density_spectrum_download, 'nxc_density_spectrum_enable')
    spectrum_on()
    zero = ctx.density_moments_download()
    assert zero.shape == (q, 10) and not zero.any()

    got = {}
    ctx.density_moments_accumulate(*cols)
    got['moments'], got['s0'], got['counts'] = density_moments.download(ctx, index, q)
    moments_restatement.check(got['moments'], got['s0'], got['counts'], want_m, f'{q} points, moments')
    ctx.density_spectrum_accumulate(*cols)
    got['spectrum'], _, counts = density_spectrum.download(ctx, index, q)
    assert np.array_equal(counts, 2*want_s.counts)
    assert np.all(np.abs(got['spectrum'] - want_s.sums) <= want_s.bound)
    assert not got['spectrum'][:, want_s.seen == 0].any()
    ctx.density_spectrum_enable(0)
    spectrum_on()
    ctx.density_spectrum_accumulate(*density_spectrum.with_unit_frac(cols))
    ones, _, got['passes'] = density_spectrum.download(ctx, index, q)
    got['rows'] = spectrum_restatement.seen_counts(ones)
    assert np.array_equal(got['passes'], 3*want_s.counts)
    assert np.array_equal(got['rows'], want_s.seen)
    return got, want_m, want_s


def same_density(got, fresh, want_m, want_s):
    for exact in ('counts', 'passes', 'rows'):
        assert np.array_equal(got[exact], fresh[exact]), exact
    assert np.all(np.abs(got['s0'] - fresh['s0']) <= want_m.bound_s0)
    assert np.all(np.abs(got['moments'] - fresh['moments']) <= want_m.bound)
    assert np.all(np.abs(got['spectrum'] - fresh['spectrum']) <= want_s.bound)


def second_configuration(ctx, forces):
    return (pixels(ctx, forces, 'image', (3, 2), 12), pixels(ctx, forces, 'camera', (3, 2), 14),
            density(ctx, 3, 16))


def test_a_second_configuration_is_what_a_fresh_context_gives():
    forces = H.mercury_forces('Na', 1.3)
    with hip_api.Context(0) as ctx:
        pixels(ctx, forces, 'image', (7, 5), 11)
        pixels(ctx, forces, 'camera', (7, 5), 13)
        density(ctx, 12, 15)
        again = second_configuration(ctx, forces)
    with hip_api.Context(0) as other:
        fresh = second_configuration(other, forces)
    for (got, *want), (new, *_) in zip(again[:2], fresh[:2]):
        same_pixels(got, new, *want)
    (got, *want), (new, *_) = again[2], fresh[2]
    same_density(got, new, *want)
