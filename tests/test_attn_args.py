"""The attention entries' argument checks: which message each refusal carries and, for inputs that break two rules, which one wins.

No GPU needed: every call here is refused on the host, before any launch (the pointers are dummies that are never dereferenced).
tests/test_attn_long_args.py pins the launch-grid refusal of mbx_attn_fwd / mbx_attn_bwd, tests/test_ragged.py the ragged entry's."""
import os

import pytest

from motionbert_amd.engine import MODE_SPATIAL, MODE_TEMPORAL
from motionbert_amd.hip_ops import MBX_BF16, MBX_F32

P = 8           # a non-null, 8-byte aligned dummy pointer
SHAPE = (2, 9, 17, 8, 64)      # B, T, J, H, hd
HUGE = 1 << 24                 # clips: 2^24 x 17 joints x 8 heads x 2 sequence blocks overflow the launch grid


@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def refused(lib, rc, *parts):
    err = lib.mbx_last_error()
    assert rc != 0, 'the call was not refused'
    for part in parts:
        assert part in err, (part, err)


def fwd(lib, ptrs=(P, P, P), shape=SHAPE, scale=0.125, mode=MODE_TEMPORAL, dtype=MBX_BF16):
    return lib.mbx_attn_fwd(*ptrs, *shape, scale, mode, dtype, None)


def fwd_drop(lib, ptrs=(P, P, P), shape=SHAPE, scale=0.125, mode=MODE_TEMPORAL, dtype=MBX_BF16, p=0.5):
    return lib.mbx_attn_fwd_drop(*ptrs, *shape, scale, mode, dtype, p, 7, None)


def bwd(lib, ptrs=(P,) * 5, shape=SHAPE, mode=MODE_TEMPORAL, dtype=MBX_BF16):
    return lib.mbx_attn_bwd(*ptrs, *shape, 0.125, mode, dtype, None)


def bwd_drop(lib, ptrs=(P,) * 5, shape=SHAPE, mode=MODE_TEMPORAL, dtype=MBX_BF16, p=0.5):
    return lib.mbx_attn_bwd_drop(*ptrs, *shape, 0.125, mode, dtype, p, 7, None)


def bwd_planes(lib, ptrs=(P,) * 6, shape=SHAPE, mode=MODE_TEMPORAL, p=0.0):
    return lib.mbx_attn_bwd_planes(*ptrs, *shape, 0.125, mode, p, 7, None)


def bwd_stats(lib, ptrs=(P,) * 8, shape=SHAPE, mode=MODE_TEMPORAL):
    return lib.mbx_attn_bwd_stats(*ptrs, *shape, 0.125, mode, None)


def with_null(n, k):
    return tuple(None if i == k else P for i in range(n))


def test_null_pointers(lib):
    for k in range(3):
        refused(lib, fwd(lib, ptrs=with_null(3, k)), b'attn_fwd: null pointer')
        refused(lib, fwd_drop(lib, ptrs=with_null(3, k)), b'attn_fwd: null pointer')
    for k in range(5):
        refused(lib, bwd(lib, ptrs=with_null(5, k)), b'attn_bwd: null pointer')
        refused(lib, bwd_drop(lib, ptrs=with_null(5, k)), b'attn_bwd: null pointer')
        refused(lib, bwd_planes(lib, ptrs=with_null(6, k)), b'attn_bwd: null pointer')        # dqkv_hi is the fifth
        refused(lib, bwd_stats(lib, ptrs=with_null(8, k)), b'attn_bwd: null pointer')
    refused(lib, bwd_planes(lib, ptrs=with_null(6, 5)), b'attn_bwd_planes: null pointer')     # dqkv_lo
    for k in (5, 6, 7):                                                                        # bias_f, rsum, part
        refused(lib, bwd_stats(lib, ptrs=with_null(8, k)), b'attn_bwd_stats: null pointer')
    refused(lib, bwd_stats(lib, ptrs=(P,) * 7 + (12,)), b'attn_bwd_stats: part must be 8-byte aligned')


@pytest.mark.parametrize('call,who', [(fwd, b'attn_fwd'), (fwd_drop, b'attn_fwd'), (bwd, b'attn_bwd'), (bwd_drop, b'attn_bwd'),
                                      (bwd_planes, b'attn_bwd'), (bwd_stats, b'attn_bwd')])
def test_shape_head_dim_and_mode(lib, call, who):
    for shape in ((0, 9, 17, 8, 64), (2, 0, 17, 8, 64), (2, 9, -1, 8, 64), (2, 9, 17, 0, 64)):
        refused(lib, call(lib, shape=shape), who + b': bad shape')
    refused(lib, call(lib, shape=(2, 9, 17, 8, 48)), who + b': head dim 48 unsupported (32 or 64)')
    refused(lib, call(lib, mode=2), who + b': unknown mode 2')
    # the order of the shared checks: shape, head dim, mode
    refused(lib, call(lib, shape=(0, 9, 17, 8, 48), mode=5), b'bad shape')
    refused(lib, call(lib, shape=(2, 9, 17, 8, 48), mode=5), b'head dim 48')
    refused(lib, call(lib, shape=(2, 300, 17, 8, 48)), b'head dim 48')       # on the way to the streamed kernels too


@pytest.mark.parametrize('call,who', [(fwd, b'attn_fwd'), (fwd_drop, b'attn_fwd'), (bwd, b'attn_bwd'), (bwd_drop, b'attn_bwd')])
def test_unknown_dtype(lib, call, who):
    refused(lib, call(lib, dtype=2), who + b': unknown dtype 2')
    refused(lib, call(lib, dtype=-1), who + b': unknown dtype -1')
    refused(lib, call(lib, mode=3, dtype=7), b'unknown mode 3')                                   # mode before dtype
    refused(lib, call(lib, shape=(HUGE, 300, 17, 8, 64), dtype=7), b'unknown dtype 7')            # dtype before the grid


@pytest.mark.parametrize('call', [fwd, fwd_drop])
def test_forward_scale_must_be_positive(lib, call):
    refused(lib, call(lib, scale=0.0), b'attn_fwd: scale must be positive', b'got 0')
    refused(lib, call(lib, scale=-0.125), b'attn_fwd: scale must be positive', b'got -0.125')
    refused(lib, call(lib, scale=float('nan')), b'attn_fwd: scale must be positive')
    refused(lib, call(lib, ptrs=(P, None, P), scale=0.0), b'null pointer')                        # null pointer before scale
    refused(lib, call(lib, shape=(0, 9, 17, 8, 48), scale=0.0, mode=9, dtype=9), b'scale must be positive')      # scale before the shape checks


@pytest.mark.parametrize('call,who', [(fwd_drop, b'attn_fwd_drop'), (bwd_drop, b'attn_bwd_drop'), (bwd_planes, b'attn_bwd_planes')])
def test_dropout_rate(lib, call, who):
    refused(lib, call(lib, p=1.0), who + b': dropout rate 1 outside [0, 1)')
    refused(lib, call(lib, p=-0.25), who + b': dropout rate -0.25 outside [0, 1)')
    refused(lib, call(lib, p=float('nan')), who + b': dropout rate')
    # the rate is looked at before anything else but the entry's own pointers
    n = 6 if call is bwd_planes else 5 if call is bwd_drop else 3
    refused(lib, call(lib, ptrs=with_null(n, 0), shape=(0, 9, 17, 8, 48), p=1.0), who + b': dropout rate')


def test_entry_checks_come_before_the_shared_ones(lib):
    refused(lib, bwd_planes(lib, ptrs=with_null(6, 5), p=1.0), b'attn_bwd_planes: null pointer')      # dqkv_lo before the rate
    refused(lib, bwd_planes(lib, ptrs=(None,) * 6, shape=(0, 9, 17, 8, 64)), b'attn_bwd_planes: null pointer')
    refused(lib, bwd_stats(lib, ptrs=(None,) * 8, shape=(0, 9, 17, 8, 64)), b'attn_bwd_stats: null pointer')
    refused(lib, bwd_stats(lib, ptrs=(None,) * 5 + (P, P, 12)), b'part must be 8-byte aligned')        # alignment before the other pointers
    refused(lib, bwd(lib, ptrs=with_null(5, 2), shape=(0, 9, 17, 8, 48), mode=4, dtype=4), b'attn_bwd: null pointer')      # null before bad shape


@pytest.mark.parametrize('dtype', [MBX_F32, MBX_BF16])
def test_streamed_grid_overflow(lib, dtype):
    """L > 256 with more (problem, 256-row block) pairs than a launch grid holds, through every entry and in both modes."""
    temporal, spatial = (HUGE, 300, 17, 8, 64), (HUGE, 17, 300, 8, 32)
    for shape, mode in ((temporal, MODE_TEMPORAL), (spatial, MODE_SPATIAL)):
        refused(lib, fwd(lib, shape=shape, mode=mode, dtype=dtype), b'attn_fwd: 2281701376 problems x 2 sequence blocks exceed the launch grid')
        refused(lib, fwd_drop(lib, shape=shape, mode=mode, dtype=dtype), b'attn_fwd: 2281701376 problems x 2 sequence blocks exceed the launch grid')
        refused(lib, bwd(lib, shape=shape, mode=mode, dtype=dtype), b'attn_bwd: 2281701376 problems x 2 sequence blocks exceed the launch grid')
        refused(lib, bwd_drop(lib, shape=shape, mode=mode, dtype=dtype), b'attn_bwd: 2281701376 problems x 2 sequence blocks exceed the launch grid')
    refused(lib, bwd_planes(lib, shape=temporal), b'attn_bwd: 2281701376 problems', b'exceed the launch grid')
    refused(lib, bwd_planes(lib, shape=temporal, p=0.5), b'attn_bwd: 2281701376 problems', b'exceed the launch grid')
    refused(lib, bwd_stats(lib, shape=temporal), b'attn_bwd: 2281701376 problems', b'exceed the launch grid')
    # the product counts, not the problems alone: 2^21 x 17 x 8 problems fit a grid, their 8 blocks each do not
    refused(lib, fwd(lib, shape=(1 << 21, 2000, 17, 8, 64), dtype=dtype), b'attn_fwd: 285212672 problems x 8 sequence blocks')
