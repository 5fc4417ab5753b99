"""The serial ends of the training step on a real MI355X: the re-gridded embedding backward (one block per frame index and channel
group, one finalize launch for dpos / dw / db), the head kernels with several rows in flight per wave, and the embedding that
normalises its own rows (mbx_embed_ln_fwd).

References: torch in float64 on the same inputs, and oracle.torch_ops.MockOps for the op definitions.  Tolerances (relative L2 over the
whole tensor) are those tests/test_gpu_kernels.py gives the same quantities: 2e-5 for fp32 outputs, 5e-5 for gradients that are sums of
per-block partial rows, 4e-3 for bf16 outputs, 1e-6 for embed_fwd.  Every float reduction has a fixed order: two calls give the same
bits, and the bf16-pair form of the embedding backward gives the bits of the call on the pair's fp32 sum.

Shapes are the smallest at which the new grids can go wrong: see the lists below."""
import pytest
import torch

from oracle.torch_ops import MockOps

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 7.0


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def check(name, got, ref, tol):
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all(), f'{name}: non-finite output'
    e = rel(got, ref)
    print(f'{name}: rel-l2 {e:.3e} (tol {tol:.0e})')
    assert e < tol, f'{name}: rel-l2 {e:.3e} >= {tol:.1e}'


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


# ------------------------------------------------------------------------------------------------------------------ embedding backward
# (B, T, J, C, Din): one clip / one frame; a clip count that divides no slice count (3 clips over 16 slices, 9 over 8); more clips
# than the eight loads in flight; C/4 = 16 < 64 lanes with fewer joints than slices (every joint split by clip); C/4 = 256 with
# dim_in 4.  A block is 1024 threads: 256 quads x 4 slices at C = 1024, 128 x 8 at C = 512, 64 x 16 below (17 joints: one whole
# round and one joint split by clip).
EMBED_SHAPES = [(1, 1, 17, 512, 3), (3, 2, 17, 256, 3), (9, 5, 17, 512, 3), (2, 9, 5, 64, 2), (17, 3, 17, 1024, 4)]
MAXLEN = 12      # rows of temp_embed / dtemp; the binding zeroes dtemp first, the kernel writes rows < T
EMBED_NAMES = ['dw', 'db', 'dpos', 'dtemp', 'dx']


def embed_outs(B, T, J, C, Din, with_dx):
    shapes = [(C, Din), (C,), (1, J, C), (1, MAXLEN, 1, C)] + ([(B, T, J, Din)] if with_dx else [])
    outs = [torch.full(s, SENTINEL, device=DEV) for s in shapes]
    return outs if with_dx else outs + [None]


def embed_ref64(dh, x, w, B, T, J, C, Din):
    d = dh.double()
    d4 = d.reshape(B, T, J, C)
    dtemp = torch.zeros(1, MAXLEN, 1, C, device=DEV, dtype=torch.float64)
    dtemp[0, :T, 0] = d4.sum((0, 2))
    return [d.t() @ x.double().reshape(-1, Din), d.sum(0), d4.sum((0, 1)).reshape(1, J, C), dtemp, (d @ w.double()).reshape(B, T, J, Din)]


@pytest.mark.parametrize('with_dx', [True, False])
@pytest.mark.parametrize('B,T,J,C,Din', EMBED_SHAPES)
def test_embed_bwd(ops, B, T, J, C, Din, with_dx):
    M = B * T * J
    tag = f'B{B}.T{T}.J{J}.C{C}.Din{Din}.dx{int(with_dx)}'
    x, w = rnd(B, T, J, Din, seed=1), rnd(C, Din, seed=2)
    dh = rnd(M, C, seed=3)
    ref = embed_ref64(dh, x, w, B, T, J, C, Din)
    got = embed_outs(B, T, J, C, Din, with_dx)
    ops.embed_bwd(dh, x, w, *got, B, T, J)
    mock = embed_outs(B, T, J, C, Din, with_dx)
    MockOps().embed_bwd(dh, x, w, *mock, B, T, J)
    for n, a, m, r in zip(EMBED_NAMES, got, mock, ref):
        if a is None:
            continue
        if n == 'dtemp':
            assert bool((a[0, T:] == 0).all()), f'embed_bwd.dtemp.{tag}: rows >= T written'
        check(f'embed_bwd.{n}.{tag}', a, r, 2e-5)
        check(f'embed_bwd.{n}.vs_mock.{tag}', a, m, 2e-5)
    again = embed_outs(B, T, J, C, Din, with_dx)
    ops.embed_bwd(dh, x, w, *again, B, T, J)
    torch.cuda.synchronize()
    for n, a, o in zip(EMBED_NAMES, got, again):
        assert a is None or torch.equal(a, o), f'embed_bwd.{n}.{tag}: two calls differ'
    # the incoming gradient as a bf16 pair: the bits of the call on the pair's fp32 sum
    dh_a, dh_b = rnd(M, C, seed=4, dtype=torch.bfloat16), rnd(M, C, seed=5, dtype=torch.bfloat16, scale=0.3)
    dsum = dh_a.float() + dh_b.float()
    pair, single, pair2 = (embed_outs(B, T, J, C, Din, with_dx) for _ in range(3))
    ops.embed_bwd_pair(dh_a, dh_b, x, w, *pair, B, T, J)
    ops.embed_bwd(dsum, x, w, *single, B, T, J)
    ops.embed_bwd_pair(dh_a, dh_b, x, w, *pair2, B, T, J)
    torch.cuda.synchronize()
    ref = embed_ref64(dsum, x, w, B, T, J, C, Din)
    for n, a, o, a2, r in zip(EMBED_NAMES, pair, single, pair2, ref):
        if a is None:
            continue
        assert torch.equal(a, o), f'embed_bwd_pair.{n}.{tag}: not the bits of embed_bwd on the fp32 sum'
        assert torch.equal(a, a2), f'embed_bwd_pair.{n}.{tag}: two calls differ'
        check(f'embed_bwd_pair.{n}.{tag}', a, r, 2e-5)


# ------------------------------------------------------------------------------------------------------------------------------ head
# M = 1 and 5: fewer rows than one iteration of one wave holds in flight (4 forward, 6 backward); 4099: a ragged last group of rows
# and waves without any.  R = 64: a quarter of the lanes own a slot; R = 512: two slots per lane.  36867 rows: more than one pass of
# the grid (2048 blocks x 4 waves x 4 rows forward, 1024 x 4 x 6 backward).
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('D', [1, 3, 8])
@pytest.mark.parametrize('R', [64, 512])
@pytest.mark.parametrize('M', [1, 5, 4099])
def test_head(ops, M, R, D, dt):
    head_case(ops, M, R, D, dt)


@pytest.mark.parametrize('R,dt', [(64, torch.bfloat16), (512, torch.float32)], ids=['R64-bf16', 'R512-f32'])
def test_head_more_than_one_pass(ops, R, dt):
    head_case(ops, 36867, R, 3, dt)


def head_case(ops, M, R, D, dt):
    tag = f'M{M}.R{R}.D{D}.{"bf16" if dt == torch.bfloat16 else "f32"}'
    rep, w, b = torch.tanh(rnd(M, R, seed=1)), rnd(D, R, seed=2, scale=0.1), rnd(D, seed=3)
    out, out2 = torch.full((M, D), SENTINEL, device=DEV), torch.full((M, D), SENTINEL, device=DEV)
    ops.head_fwd(rep, w, b, out)
    ops.head_fwd(rep, w, b, out2)
    check(f'head_fwd.{tag}', out, rep.double() @ w.double().t() + b.double(), 2e-5)
    mock = torch.empty(M, D, device=DEV)
    MockOps().head_fwd(rep, w, b, mock)
    check(f'head_fwd.vs_mock.{tag}', out, mock, 2e-5)
    assert torch.equal(out, out2), f'head_fwd.{tag}: two calls differ'
    dout = rnd(M, D, seed=4)
    mk = lambda: [torch.full((M, R), SENTINEL, device=DEV, dtype=dt), torch.full((D, R), SENTINEL, device=DEV), torch.full((D,), SENTINEL, device=DEV)]
    a, a2 = mk(), mk()
    ops.head_bwd(dout, rep, w, *a)
    ops.head_bwd(dout, rep, w, *a2)
    ref = [(dout.double() @ w.double()) * (1 - rep.double() * rep.double()), dout.double().t() @ rep.double(), dout.double().sum(0)]
    for n, u, u2, r, tol in zip(['dpre', 'dw', 'db'], a, a2, ref, [4e-3 if dt == torch.bfloat16 else 2e-5, 5e-5, 5e-5]):
        check(f'head_bwd.{n}.{tag}', u, r, tol)
        assert torch.equal(u, u2), f'head_bwd.{n}.{tag}: two calls differ'


# ------------------------------------------------------------------------------------------- embedding + normalisation of its own rows
# (B, T, J, C): one frame of one clip at C = 512 (two slots per lane); C = 256 (one full slot); C = 64 (a quarter of the lanes) with
# M = 105 rows: no multiple of the four rows of a block
@pytest.mark.parametrize('B,T,J,C', [(1, 1, 17, 512), (2, 9, 17, 256), (3, 7, 5, 64)])
def test_embed_ln_fwd(ops, B, T, J, C):
    M, Din, eps = B * T * J, 3, 1e-6
    x, w, b = rnd(B, T, J, Din, seed=1), rnd(C, Din, seed=2), rnd(C, seed=3)
    pos, temp = rnd(1, J, C, seed=4), rnd(1, MAXLEN, 1, C, seed=5)
    mk = lambda: [torch.full((M, C), SENTINEL, device=DEV), torch.full((M, C), SENTINEL, device=DEV, dtype=torch.bfloat16),
                  torch.full((M,), SENTINEL, device=DEV), torch.full((M,), SENTINEL, device=DEV)]
    two, one = mk(), mk()
    ops.embed_fwd(x, w, b, pos, temp, two[0], B, T, J)
    ops.layernorm_fwd(two[0], None, None, eps, *two[1:])
    ops.embed_ln_fwd(x, w, b, pos, temp, eps, *one, B, T, J)
    torch.cuda.synchronize()
    for n, u, v in zip(['h', 'xhat', 'mean', 'rstd'], one, two):
        assert torch.equal(u, v), f'embed_ln_fwd.{n}.B{B}.T{T}.J{J}.C{C}: not the bits of embed_fwd + layernorm_fwd'
    h64 = x.double() @ w.double().t() + b.double() + pos.double().reshape(1, 1, J, C) + temp.double()[:, :T]
    check(f'embed_ln_fwd.h.C{C}', one[0], h64.reshape(M, C), 1e-6)
    mu = h64.reshape(M, C).mean(-1, keepdim=True)
    rs = torch.rsqrt(((h64.reshape(M, C) - mu) ** 2).mean(-1, keepdim=True) + eps)
    check(f'embed_ln_fwd.xhat.C{C}', one[1], (h64.reshape(M, C) - mu) * rs, 4e-3)
    check(f'embed_ln_fwd.rstd.C{C}', one[3], rs.reshape(M), 2e-5)
