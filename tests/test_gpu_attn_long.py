"""Temporal attention beyond 256 frames on a real MI355X: the streamed kernels (csrc/attention_stream.hip) against the torch
restatement of the kernel set (MockOps, run on the GPU), with the tolerances of test_gpu_kernels.py::test_attention.  Every output
is pre-filled with a sentinel, so a row the kernels never write shows up as an error."""
import pytest
import torch

from motionbert_amd.engine import MODE_TEMPORAL
from tests.mock_ops import MockOps
from tests.test_gpu_kernels import DEV, check, rel, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
J = 17
# one-row tail block (257), ragged tails (300, 777), exact multiples of the 256-row block (512, 1024, 2048), several query blocks
LONG = [(1, 257, 8, 64), (2, 300, 8, 32), (1, 512, 8, 64), (1, 777, 2, 64), (1, 1024, 4, 32), (1, 2048, 2, 64)]


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def _inputs(B, T, H, hd, dt):
    C, M = H * hd, B * T * J
    qkv = rnd(M, 3 * C, seed=1, dtype=dt)
    qkv[:, :C] *= 2.0          # a few dominant keys: large row maxima
    return qkv, rnd(M, C, seed=2, dtype=dt), C, M


def _sections(name, got, ref, C, tol):
    for i, n in enumerate(['dq', 'dk', 'dv']):
        check(f'{name}.{n}', got[:, i * C:(i + 1) * C], ref[:, i * C:(i + 1) * C], tol)


@pytest.mark.parametrize('dt', [torch.float32, BF])
@pytest.mark.parametrize('B,T,H,hd', LONG)
def test_attention_long(ops, dt, B, T, H, hd):
    qkv, do, C, M = _inputs(B, T, H, hd, dt)
    scale = hd ** -0.5
    tag = f'{"f32" if dt == torch.float32 else "bf16"}.B{B}T{T}H{H}d{hd}'
    o, lse = torch.full((M, C), 9.0, device=DEV, dtype=dt), torch.full((M, H), 9.0, device=DEV)
    o2, lse2 = torch.empty(M, C, device=DEV, dtype=dt), torch.empty(M, H, device=DEV)
    ops.attn_fwd(qkv, o, lse, B, T, J, H, scale, MODE_TEMPORAL)
    MockOps().attn_fwd(qkv, o2, lse2, B, T, J, H, scale, MODE_TEMPORAL)
    check(f'attn_long.fwd.o.{tag}', o, o2, 2e-5 if dt == torch.float32 else 1.5e-2)
    check(f'attn_long.fwd.lse.{tag}', lse, lse2, 2e-5 if dt == torch.float32 else 1e-4)
    dq, dq2 = torch.full((M, 3 * C), 9.0, device=DEV, dtype=dt), torch.empty(M, 3 * C, device=DEV, dtype=dt)
    ops.attn_bwd(qkv, o2, do, lse2, dq, B, T, J, H, scale, MODE_TEMPORAL)
    MockOps().attn_bwd(qkv, o2, do, lse2, dq2, B, T, J, H, scale, MODE_TEMPORAL)
    _sections(f'attn_long.bwd.{tag}', dq, dq2, C, 5e-5 if dt == torch.float32 else 2e-2)
    if dt == torch.float32:      # operand planes of the bf16x3 split: bit for bit the split of the fp32 output
        pl = (torch.full((M, 3 * C), 9.0, device=DEV, dtype=BF), torch.full((M, 3 * C), 9.0, device=DEV, dtype=BF))
        ops.attn_bwd(qkv, o2, do, lse2, pl, B, T, J, H, scale, MODE_TEMPORAL)
        hi, lo = ops.split(dq)
        torch.cuda.synchronize()
        assert torch.equal(pl[0].view(torch.int16), hi.view(torch.int16)) and torch.equal(pl[1].view(torch.int16), lo.view(torch.int16)), tag


@pytest.mark.parametrize('dt', [torch.float32, BF])
@pytest.mark.parametrize('T', [300, 512])
def test_attention_long_probability_dropout(ops, dt, T):
    """The mask index runs over the full L (dbase + q L + k): the same masks as the resident kernels and dropmask.py."""
    B, H, hd = 1, 4, 64
    qkv, do, C, M = _inputs(B, T, H, hd, dt)
    scale = hd ** -0.5
    drop = (0.1, 0x1234567890ABCDEF)
    tag = f'{"f32" if dt == torch.float32 else "bf16"}.T{T}'
    o, lse = torch.full((M, C), 9.0, device=DEV, dtype=dt), torch.full((M, H), 9.0, device=DEV)
    o2, lse2, o0 = torch.empty(M, C, device=DEV, dtype=dt), torch.empty(M, H, device=DEV), torch.empty(M, C, device=DEV, dtype=dt)
    ops.attn_fwd(qkv, o, lse, B, T, J, H, scale, MODE_TEMPORAL, drop=drop)
    ops.attn_fwd(qkv, o0, torch.empty_like(lse), B, T, J, H, scale, MODE_TEMPORAL)
    MockOps().attn_fwd(qkv, o2, lse2, B, T, J, H, scale, MODE_TEMPORAL, drop=drop)
    check(f'attn_long_drop.fwd.o.{tag}', o, o2, 2e-5 if dt == torch.float32 else 1.5e-2)
    check(f'attn_long_drop.fwd.lse.{tag}', lse, lse2, 2e-5 if dt == torch.float32 else 1e-4)
    assert rel(o.float(), o0.float()) > 0.05, 'the mask must change the output'
    dq, dq2 = torch.full((M, 3 * C), 9.0, device=DEV, dtype=dt), torch.empty(M, 3 * C, device=DEV, dtype=dt)
    ops.attn_bwd(qkv, o2, do, lse2, dq, B, T, J, H, scale, MODE_TEMPORAL, drop=drop)
    MockOps().attn_bwd(qkv, o2, do, lse2, dq2, B, T, J, H, scale, MODE_TEMPORAL, drop=drop)
    _sections(f'attn_long_drop.bwd.{tag}', dq, dq2, C, 5e-5 if dt == torch.float32 else 2e-2)


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('T', [300, 512])
def test_attn_bwd_stats_long(ops, T, hd):
    """The row-dot form the folded LayerNorm backward calls (bf16 training): dqkv identical to mbx_attn_bwd, and per (token, head)
    the dots of the rounded dqkv with rsum and (qkv - bias_f) -- the reconstruction of test_gpu_fold.py::test_attn_bwd_stats."""
    B, H = 1, 4
    C, M = H * hd, B * T * J
    qkv, do = rnd(M, 3 * C, seed=1, dtype=BF), rnd(M, C, seed=2, dtype=BF)
    o, lse = torch.empty(M, C, device=DEV, dtype=BF), torch.empty(M, H, device=DEV)
    scale = hd ** -0.5
    ops.attn_fwd(qkv, o, lse, B, T, J, H, scale, MODE_TEMPORAL)
    bias_f, rsum = rnd(3 * C, seed=3, scale=0.3), rnd(3 * C, seed=4)
    d0, d1 = torch.empty(M, 3 * C, device=DEV, dtype=BF), torch.full((M, 3 * C), 9.0, device=DEV, dtype=BF)
    part = torch.full((2 * H, M, 2), 7.0, device=DEV)
    ops.attn_bwd(qkv, o, do, lse, d0, B, T, J, H, scale, MODE_TEMPORAL)
    ops.attn_bwd_stats(qkv, o, do, lse, d1, bias_f, rsum, part, B, T, J, H, scale, MODE_TEMPORAL)
    torch.cuda.synchronize()
    tag = f'T{T}.hd{hd}'
    assert torch.equal(d0, d1), f'attn_bwd_stats_long.{tag}: dqkv differs from mbx_attn_bwd'
    d = d1.float().reshape(M, 3, H, hd)
    rb, bb = rsum.to(BF).float(), bias_f.to(BF).float()
    y = (qkv.float() - bb).reshape(M, 3, H, hd)
    t1, t2 = (d * rb.reshape(1, 3, H, hd)).sum(3), (d * y).sum(3)
    own = torch.stack([torch.stack([t1[:, 0], t1[:, 1] + t1[:, 2]], -1), torch.stack([t2[:, 0], t2[:, 1] + t2[:, 2]], -1)], -1)
    check(f'attn_bwd_stats_long.part.{tag}', part, own.reshape(M, 2 * H, 2).transpose(0, 1), 1e-4)
