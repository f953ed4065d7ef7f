"""The moments and cube entries of hip_api.Context for the image and for the camera, without a
GPU: on a library stub that records (symbol, arguments), each method calls the nxc_ symbol of its
own prefix and its download has the shape its docstring gives."""
import ctypes as C
import types

import numpy as np
import pytest

from nexoclom_amd.hip_api import Context


class Library:
    """Every nxc_ symbol succeeds and is recorded with the values of its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        if not symbol.startswith('nxc_'):
            raise AttributeError(symbol)

        def entry(*args):
            self.calls.append((symbol, tuple(getattr(a, 'value', a) for a in args[1:])))
            return 0
        return entry


def context(prefix, shape):
    ctx = Context.__new__(Context)
    ctx.lib, ctx._h = Library(), C.c_void_p()
    ctx.image_shape = None                         # as Context() leaves it until set_image
    if shape is not None:                          # as set_image / camera_set leave it
        setattr(ctx, prefix + '_shape', shape)
    return ctx


def said(ctx):
    calls, ctx.lib.calls = ctx.lib.calls, []
    return calls


@pytest.mark.parametrize('shape', [None, (3, 5)])
@pytest.mark.parametrize('prefix', ['image', 'camera'])
def test_moments_entries_call_their_own_symbols(prefix, shape):
    ctx = context(prefix, shape)
    entry = lambda op: getattr(ctx, f'{prefix}_moments_{op}')            # noqa: E731
    entry('enable')()
    entry('enable')(on=False)
    assert said(ctx) == [(f'nxc_{prefix}_moments_enable', (1,)), (f'nxc_{prefix}_moments_enable', (0,))]
    sums = entry('download')()
    assert sums.shape == (shape or (0, 0)) + (4,) and sums.dtype == np.float64 and not sums.any()
    (symbol, args), = said(ctx)
    assert symbol == f'nxc_{prefix}_moments_download' and len(args) == 1


@pytest.mark.parametrize('nv', [0, 6])
@pytest.mark.parametrize('shape', [None, (3, 5)])
@pytest.mark.parametrize('prefix', ['image', 'camera'])
def test_cube_entries_call_their_own_symbols(prefix, shape, nv):
    ctx = context(prefix, shape)
    entry = lambda op: getattr(ctx, f'{prefix}_cube_{op}')               # noqa: E731
    assert entry('download')().shape == (shape or (0, 0)) + (2, 2)       # no enable yet: nv = 0
    assert said(ctx)[0][0] == f'nxc_{prefix}_cube_download'
    if nv:
        entry('enable')(nv, v_lo=-2.5, v_hi=1.5)
        assert said(ctx) == [(f'nxc_{prefix}_cube_enable', (nv, -2.5, 1.5))]
    else:
        entry('enable')(nv)
        assert said(ctx) == [(f'nxc_{prefix}_cube_enable', (0, 0.0, 0.0))]
    sums = entry('download')()
    assert sums.shape == (shape or (0, 0)) + (nv + 2, 2) and sums.dtype == np.float64
    (symbol, args), = said(ctx)
    assert symbol == f'nxc_{prefix}_cube_download' and len(args) == 1
    # the twin's bin count is its own
    other = 'camera' if prefix == 'image' else 'image'
    assert getattr(ctx, f'{other}_cube_download')().shape == (0, 0, 2, 2)
    assert said(ctx)[0][0] == f'nxc_{other}_cube_download'


@pytest.mark.parametrize('what', ['moments', 'cube'])
@pytest.mark.parametrize('prefix', ['image', 'camera'])
def test_accumulate_entries_call_their_own_symbols(prefix, what):
    ctx = context(prefix, (3, 5))
    accumulate = getattr(ctx, f'{prefix}_{what}_accumulate')
    names = ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac')
    store = types.SimpleNamespace(_r='handle')
    accumulate(rows=(store, 4, 9))
    assert said(ctx) == [(f'nxc_{prefix}_{what}_accumulate_rows', ('handle', 4, 9))]
    for dtype, suffix in ((np.float32, '_f32'), (np.float64, '')):
        accumulate(**{name: np.zeros(11, dtype=dtype) for name in names})
        (symbol, args), = said(ctx)
        assert symbol == f'nxc_{prefix}_{what}_accumulate{suffix}'
        assert args[0] == 11 and len(args) == 1 + len(names)
