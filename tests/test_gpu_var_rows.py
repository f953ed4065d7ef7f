"""nxc_integrate_var_resident + nxc_var_rows_build through hip_api.  The yardstick is the unchanged
nxc_integrate_var on the same upload, its finals filtered (fp64 frac > 0) and narrowed
(astype(float32) / int32) with NumPy: rows, index, kept and total bit for bit."""
import numpy as np
import pytest

from nexoclom_amd import hip_api
from tests import helpers as H

pytestmark = pytest.mark.gpu

RES, EDGE, ENDTIME = 1e-4, 25.0, 3000.0
COUNTS = [1, 63, 64, 65, 255, 256, 257, 3*256 + 17, 5000]
DROPPED = [0.0, -0.0, np.nan, -0.5]
KEPT = [1e-300, 1e-46, 1e-10]                  # 1e-300 and 1e-46 narrow to 0 and are kept
TIE = 1.0 + 2.0**-24                           # halfway between two float32: rounds to even, 1.0


def packets(n, seed, plant='alternate'):
    """n packets with random launch times; planted ones have no time left, so the driver leaves
    their state alone: around the first wave boundary (lanes 56..71) dropped and kept fracs
    alternate, two kept ones carry a position that overflows float32 and a rounding tie."""
    X0 = H.sample_x0(n, seed, ENDTIME)
    X0[:, 0] = np.random.default_rng(seed + 1).random(n)*ENDTIME
    if plant == 'alternate':
        planted = np.arange(max(0, min(n, 64) - 8), min(n, 64 + 8))
        frac = np.array([DROPPED[(i//2) % 4] if i % 2 == 0 else KEPT[(i//2) % 3] for i in planted])
    elif plant == 'none kept':
        planted = np.arange(n)
        frac = np.array([DROPPED[i % 4] for i in planted])
    else:                                      # every packet kept: none flies (and lands)
        planted = np.arange(n)
        frac = np.array([(KEPT + [1.0, 0.5])[i % 5] for i in planted])
    X0[planted, 0] = 0.0
    X0[planted, 7] = frac
    kept = planted[frac > 0]
    if len(kept) > 1:
        X0[kept[0], 1] = 1e39
        X0[kept[1], 2] = TIE
    return X0, planted, frac


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def expected(final, narrow, compress):
    keep = final[:, 7] > 0 if compress else np.ones(len(final), dtype=bool)
    rows = np.vstack([final[keep].T, np.zeros((1, int(keep.sum())))])
    index = np.flatnonzero(keep)
    with np.errstate(over='ignore', under='ignore'):
        return (rows.astype(np.float32) if narrow else rows,
                index.astype(np.int32 if narrow else np.int64), keep)


def prepare(ctx):
    H.set_ctx_forces(ctx, H.mercury_forces('Na', 1.3))
    ctx.set_bounce(None)
    ctx.set_bodies(None)


def check_all_forms(ctx, X0, planted, frac):
    ctx.upload_packets(X0)
    final, hs = ctx.integrate_var(RES, EDGE)                 # the yardstick, on this upload
    want_ctr = ctx.counters()
    assert np.array_equal(bits(final[planted]), bits(X0[planted]))      # left alone
    got_hs = ctx.integrate_var(RES, EDGE, resident=True)
    assert np.array_equal(bits(got_hs), bits(hs))
    assert ctx.counters() == want_ctr
    for narrow in (False, True):
        for compress in (False, True):
            rows, index, keep = expected(final, narrow, compress)
            store, kept = ctx.var_rows_build(narrow=narrow, compress=compress)
            try:
                assert store.total == int(keep.sum()) and store.narrow == narrow
                assert kept.dtype == np.bool_ and np.array_equal(kept, keep)
                if store.total:
                    got_rows, got_index = store.download()
                    assert got_rows.dtype == rows.dtype and got_index.dtype == index.dtype
                    assert np.array_equal(got_index, index)
                    assert np.array_equal(bits(got_rows), bits(rows))
            finally:
                store.free()
    return final


@pytest.mark.parametrize('variant', ['fair', 'plain'])
@pytest.mark.parametrize('n', COUNTS)
def test_rows_equal_filtered_narrowed_finals(ctx, n, variant, monkeypatch):
    monkeypatch.setenv('NXC_TEST_VAR_VARIANT', variant)
    prepare(ctx)
    X0, planted, frac = packets(n, 100 + n)
    final = check_all_forms(ctx, X0, planted, frac)
    if n >= 72:
        keep = final[:, 7] > 0
        assert keep[57:72:2].all() and not keep[56:72:2].any()          # across lanes 63 | 64
        with np.errstate(over='ignore'):
            narrowed = final[keep].astype(np.float32)
        assert np.isinf(narrowed[:, 1]).any() and (narrowed[:, 2] == 1.0).any()
        assert (narrowed[:, 7] == 0).sum() >= 4                         # underflowed, kept


@pytest.mark.parametrize('plant', ['none kept', 'all kept'])
def test_nothing_and_everything_kept(ctx, plant):
    prepare(ctx)
    X0, planted, frac = packets(257, 7, plant)
    final = check_all_forms(ctx, X0, planted, frac)
    assert (final[:, 7] > 0).sum() == (0 if plant == 'none kept' else 257)


def test_build_needs_a_resident_integration_of_these_packets(ctx):
    prepare(ctx)
    X0, _, _ = packets(300, 3)
    ctx.upload_packets(X0)

    def refused():
        with pytest.raises(hip_api.HipError) as err:
            ctx.var_rows_build(narrow=True, compress=True)
        assert err.value.code == hip_api.NXC_ERR_STATE

    refused()                                                # nothing integrated yet
    final, hs = ctx.integrate_var(RES, EDGE)
    refused()                                                # the download form does not count
    ctx.integrate_var(RES, EDGE, resident=True)
    ctx.upload_packets(X0)
    refused()                                                # a later upload
    ctx.integrate_var(RES, EDGE, resident=True)
    ctx.state(X0[:4, 1], X0[:4, 2], X0[:4, 3], X0[:4, 5])   # takes the scratch the finals sit in
    refused()
    # the handle works afterwards
    ctx.integrate_var(RES, EDGE, resident=True)
    store, kept = ctx.var_rows_build(narrow=False, compress=False)
    rows, index = store.download()
    store.free()
    assert kept.all() and np.array_equal(bits(rows[:8]), bits(final.T))
    assert np.array_equal(index, np.arange(300))


@pytest.mark.parametrize('narrow', [False, True])
def test_image_over_the_store_equals_image_over_host_columns(ctx, narrow):
    prepare(ctx)
    f = H.mercury_forces('Na', 1.3)
    X0, _, _ = packets(5000, 11)
    ctx.upload_packets(X0)
    ctx.integrate_var(RES, EDGE, resident=True)
    store, kept = ctx.var_rows_build(narrow=narrow, compress=True)
    rows, _ = store.download()
    im = H.image_setup(f, 'radiance', dims=(64, 64))
    ctx.set_image(im['M'], f.vrplanet, im['apix'], 'radiance', im['xedges'], im['zedges'],
                  im['g_tables'])
    ctx.image_accumulate_rows(store)
    got_image, got_counts = ctx.image_download()
    store.free()
    ctx.image_clear()
    ctx.image_accumulate(*(rows[k] for k in (1, 2, 3, 5, 7)))
    image, counts = ctx.image_download()
    assert counts.sum() > 100 and np.array_equal(got_counts, counts)
    np.testing.assert_allclose(got_image, image, rtol=1e-12, atol=0)
