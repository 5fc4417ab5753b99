"""References, rounding models and gates for the kernels of csrc/elementwise.hip between the GEMMs and the loss: embedding, LayerNorm, adaptive
fusion (plain and with its fused LayerNorms), regression head, tanh backward, average.  Plain module, no fixtures, any device:
tests/test_gpu_row_parity.py applies it to the kernels on the GPU, tests/test_rowerr.py applies the same gates to seeded corruptions of the
restatements on the CPU.

  *_ref64   the exact operation in float64 from the same fp32 / bf16 bits
  *_model   the kernel's formula in torch fp32, in the kernel's operation order; bf16 exactly where the kernel rounds to bf16
  *_bound   worst-case elementwise bounds (gate A), derived where they are defined from the operation count.  gam(n) = n U / (1 - n U) is
            the standard bound for n successive roundings; a sum in which no term passes through more than L additions is off by at most
            gam(L) sum |terms|, whatever the order
  the launch geometry (grid caps, rows per wave, LDS slices) is restated from the launchers so that the bounds of the reduced outputs follow
  the summation structure: per-thread chain, LDS fold, block_fold_store, steperr.colsum_chain"""
import torch

from tests import localerr as LE
from tests import steperr as SE
from tests.steperr import f32  # noqa: F401  (the value a C float argument takes; the callers pass eps through it)

U = LE.U32
BF = torch.bfloat16
F32 = torch.float32
GUARD = 64                    # elements of guard band behind every output
LN_BLOCKS, FUSE_BLOCKS, HEAD_BWD_BLOCKS, ROW_BLOCKS = 1024, 2048, 1024, 2048      # grid caps of the launchers (blocks of 4 waves)


def gam(n):
    return n * U / (1.0 - n * U)


def cdiv(a, b):
    return -(-a // b)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ the bf16 copies
def bf16_store(x32):
    """store4<bf16_t> (mbx_common.h): pack_bf2 converts a float pair with __builtin_convertvector, which is v_cvt_pk_bf16_f32 on gfx950:
    round to nearest, ties to even -- the rounding of torch's fp32 -> bfloat16 conversion."""
    return x32.to(BF)


def bf16_trunc(x32):
    """the corruption of tests/test_rowerr.py: round toward zero (drop the low 16 bits)"""
    return (x32.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def split_planes(o32):
    """store4_planes / split_bf16_kernel: hi = bf16(o), lo = bf16(o - hi), the subtraction in fp32 (it is exact)"""
    hi = bf16_store(o32)
    return hi, bf16_store(o32 - hi.float())


# ------------------------------------------------------------------------------------------------ sentinels
def guarded(shape, dtype, device):
    """(payload view, whole buffer): NaN everywhere, GUARD elements behind the payload"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), float('nan'), dtype=dtype, device=device)
    return buf[:n].view(*shape), buf


def guard_intact(buf):
    """the guard band still holds the NaN bit pattern it was filled with"""
    ref = torch.full((GUARD,), float('nan'), dtype=buf.dtype, device=buf.device)
    return same_bits(buf[-GUARD:], ref)


# ------------------------------------------------------------------------------------------------ geometry of the row kernels
def vpl_for(C):
    return 1 if C <= 256 else 2 if C <= 512 else 4 if C <= 1024 else 8


def row_chain(C, per_slot=4):
    """additions an element passes through in a one-wave row reduction: per_slot per float4 slot of the lane (VPL slots), 6 wave levels"""
    return per_slot * vpl_for(C) + 6


def grid_rows(M, cap):
    """(blocks, most rows one wave walks) of the `row = blockIdx * 4 + wave; row += gridDim * 4` kernels"""
    grid = min(cdiv(M, 4), cap)
    return grid, cdiv(M, 4 * grid)


def colsum_vec(stride, col0, ncols):
    """launch_colsum2's choice: colsum4_kernel<16> (True) or the scalar colsum_kernel (False)"""
    assert ncols // 4 < 64 * 512, 'colsum4_kernel<64> has another chain: not restated here'
    return ncols % 4 == 0 and col0 % 4 == 0 and stride % 4 == 0


def lanes(t, C):
    """[M, C] -> [M, VPL, 64, 4]: slot k of lane l holds channels (k * 64 + l) * 4 .. + 3 (ROW_C); zeros past C, as the kernels' registers"""
    vpl = vpl_for(C)
    return torch.nn.functional.pad(t, (0, vpl * 256 - C)).reshape(t.shape[0], vpl, 64, 4)


def fma32(a, b, c):
    """fmaf in torch: the product of two fp32 values is exact in float64, the sum rounds once to 53 bits and once more to fp32 (a double
    rounding that differs from the fused operation only within 2^-29 of a tie)"""
    return (a.double() * b.double() + c.double()).float()


def wave_tree(v):
    """wave_sum (mbx_common.h) of per-lane values [M, 64]: the DPP butterfly adds lane pairs, quads, halves of a row, rows, and the two
    row_bcast steps add (R0 + R1) and (R2 + R3) and then those: a balanced tree over the lanes in their order.  fp32 addition commutes, so
    the tree is the result, bit for bit."""
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


# ------------------------------------------------------------------------------------------------ gate B on rows
def gate_rows(got, ref64, model):
    """SE.gate_units with a row of C values as the unit, and per_unit_excess on the same grid.
    Returns (g, m, px, ok, message); ok <=> worst <= 2 x model worst, every unit within 2 err_m + 2 mean, <= MAX_EXEMPT on the floor."""
    cols = got.shape[-1]
    got, ref64, model = got.reshape(-1, cols), ref64.reshape(-1, cols), model.reshape(-1, cols)
    g = LE.unit_errors(got, ref64, 1, cols, full=True)
    m = LE.unit_errors(model, ref64, 1, cols, full=True)
    px = LE.per_unit_excess(g, m, 1, cols)
    ok = m['exempt'] <= LE.MAX_EXEMPT and g['worst'] <= 2.0 * m['worst'] and px['excess'] <= 1.0
    return g, m, px, ok, (f'kernel {g["worst"]:.3e} vs 2 x model {m["worst"]:.3e} at row {g["row"]}; per-unit excess {px["excess"]:.3f} at row '
                          f'{px["row"]} ({px["n_over"]} over); {m["exempt"]:.2%} of the rows on the floor')


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def ln_inputs(M, C, seed, device, offset=0.0, affine=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * (0.5 + torch.randn(M, 1, generator=g).abs()) + offset
    gamma = (1.0 + 0.2 * torch.randn(C, generator=g)) if affine else None
    beta = 0.3 * torch.randn(C, generator=g) if affine else None
    return x.to(device), (gamma.to(device) if affine else None), (beta.to(device) if affine else None)


def ln_fwd_ref64(x, gamma, beta, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    v = x - mu
    rs = 1.0 / torch.sqrt((v * v).mean(-1, keepdim=True) + eps)
    y = v * rs
    if gamma is not None:
        y = y * gamma.double() + beta.double()
    return y, mu[:, 0], rs[:, 0]


def ln_fwd_model(x, gamma, beta, eps, dtype, stats_shift=None):
    """ln_fwd_row in torch fp32 in the kernel's order: per lane s += (v0 + v1) + (v2 + v3) over its slots, wave_sum, mu = s * (1 / C);
    v = x - mu; per lane q = fma(v, v, q) over its slots and elements, wave_sum, rs = 1 / sqrt(q * (1 / C) + eps); y = fma(v rs, gamma, beta),
    rounded to `dtype`.  The row sum decides the error of a row with a large common offset (every element inherits the mean's error), so
    the model follows its order exactly.  stats_shift = s: the corruption of tests/test_rowerr.py -- rows >= s take the mean and rstd
    of row - s."""
    M, C = x.shape
    invC = torch.ones((), dtype=F32, device=x.device) / float(C)
    L = lanes(x, C)
    s = torch.zeros(M, 64, dtype=F32, device=x.device)
    for k in range(L.shape[1]):
        s = s + ((L[:, k, :, 0] + L[:, k, :, 1]) + (L[:, k, :, 2] + L[:, k, :, 3]))
    mu = (wave_tree(s) * invC)[:, None]
    if stats_shift is not None:
        mu = torch.cat([mu[:stats_shift], mu[:M - stats_shift]])
    v = x - mu
    V = lanes(v, C)
    q = torch.zeros(M, 64, dtype=F32, device=x.device)
    for k in range(V.shape[1]):
        for i in range(4):
            q = fma32(V[:, k, :, i], V[:, k, :, i], q)
    rs = (1.0 / torch.sqrt(wave_tree(q) * invC + eps))[:, None]
    if stats_shift is not None:
        rs = torch.cat([rs[:stats_shift], rs[:M - stats_shift]])
    y = v * rs
    if gamma is not None:
        y = fma32(y, gamma, beta)
    return y.to(dtype), mu[:, 0], rs[:, 0]


def ln_stat_bounds(x, eps):
    """Gate A, absolute, for mean and rstd of ln_fwd_row.
      mean  the row sum: (v0 + v1) + (v2 + v3) per slot (2 additions), one addition per slot into s, 6 wave levels: L = 3 VPL + 6 additions at
            most per element; 1 / C is rounded, the product is rounded:  |mean - mu| <= gam(L + 2) sum |x| / C
      rstd  v_i = fl(x_i - mean) carries U |v_i|; sum (x_i - mean)^2 = sum (x_i - mu)^2 + C dmu^2 exactly, dmu the bound above; the fma chain
            (4 per slot, 6 wave levels) and the squares' two relative roundings: gam(4 VPL + 8) of a sum of non-negative terms; then the product with
            the rounded 1 / C, the addition of eps, the root (halves what came before) and the reciprocal:
            |rstd - rs| <= rs (0.5 (gam(4 VPL + 11) + dmu^2 / (var + eps)) + 2 U) (1 + 4 U)"""
    C = x.shape[-1]
    x64 = x.double()
    _, mu, rs = ln_fwd_ref64(x, None, None, eps)
    bm = gam(row_chain(C, 3) + 2) * x64.abs().sum(-1) / C
    rel = 0.5 * (gam(row_chain(C, 4) + 5) + bm * bm * rs * rs) + 2 * U
    return bm, rs * rel * (1 + 4 * U)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_bwd_ref64(dy_t, x, mean, rstd, gamma, dres, extra, drop_row=None):
    """(dx, dgamma, dbeta) in float64 from the fp32 / bf16 bits; mean and rstd are INPUTS (the fp32 values the forward stored)"""
    d, xh = dy_t.double(), (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    keep = torch.ones(d.shape[0], 1, dtype=d.dtype, device=d.device)
    if drop_row is not None:
        keep[drop_row] = 0
    dg, db = (d * xh * keep).sum(0), (d * keep).sum(0)
    dd = d * gamma.double()
    r = rstd.double()[:, None] * (dd - dd.mean(-1, keepdim=True) - xh * (dd * xh).mean(-1, keepdim=True))
    for t in (dres, extra):
        if t is not None:
            r = r + t.double()
    return r, dg, db


def ln_bwd_model(dy_t, x, mean, rstd, gamma, dres, extra, drop_row=None):
    """ln_bwd_row in torch fp32.  drop_row: the corruption of tests/test_rowerr.py -- that row is missing from dgamma and dbeta."""
    C = x.shape[-1]
    invC = torch.ones((), dtype=F32, device=x.device) / float(C)
    d, xh = dy_t.float(), (x - mean[:, None]) * rstd[:, None]
    keep = torch.ones(d.shape[0], 1, dtype=F32, device=d.device)
    if drop_row is not None:
        keep[drop_row] = 0
    dg, db = (d * xh * keep).sum(0), (d * keep).sum(0)
    dd = d * gamma
    s1, s2 = dd.sum(-1, keepdim=True) * invC, (dd * xh).sum(-1, keepdim=True) * invC
    r = rstd[:, None] * (dd - s1 - xh * s2)
    if dres is not None:
        r = r + dres
    if extra is not None:
        r = r + extra
    return r, dg, db


def ln_bwd_param_bounds(dy_t, x, mean, rstd):
    """Gate A for dgamma / dbeta along ln_bwd_kernel's summation: a wave accumulates its rows (at most ceil(M / (4 grid)) of them) in
    registers, block_fold_store adds the 4 waves, (l0 + l1) + (l2 + l3): 2 additions, colsum4_kernel<16> folds the `grid` partial rows.
    A dgamma term is d * xh with xh = fl(fl(x - mean) rstd): 2 roundings, the product itself is inside the fma.
        |dgamma - exact| <= gam(rows + 2 + colsum_chain(grid) + 2) sum_m |d xh|        |dbeta - exact| <= gam(rows + 2 + chain) sum_m |d|"""
    M, C = x.shape
    grid, rows = grid_rows(M, LN_BLOCKS)
    assert colsum_vec(2 * C, 0, 2 * C)
    L = rows + 2 + SE.colsum_chain(grid, True)
    d = dy_t.double().abs()
    xh = ((x.double() - mean.double()[:, None]) * rstd.double()[:, None]).abs()
    return gam(L + 2) * (d * xh).sum(0), gam(L) * d.sum(0)


# ------------------------------------------------------------------------------------------------ embedding forward
def embed_inputs(B, T, J, Din, C, seed, device, maxlen=None):
    """pos [1, J, C] and temp [1, maxlen, 1, C] (maxlen = T + 3 rows, more than the kernel may read) with a distinct offset per row, so that a
    wrong j or t index is a wrong value"""
    g = torch.Generator().manual_seed(seed)
    maxlen = T + 3 if maxlen is None else maxlen
    x = torch.randn(B * T * J, Din, generator=g)
    w = torch.randn(C, Din, generator=g) * 0.5
    b = torch.randn(C, generator=g) * 0.1
    pos = torch.randn(1, J, C, generator=g) * 0.1 + torch.arange(J).reshape(1, J, 1) * 0.25
    temp = torch.randn(1, maxlen, 1, C, generator=g) * 0.1 - torch.arange(maxlen).reshape(1, maxlen, 1, 1) * 0.125
    return [t.to(device) for t in (x, w, b, pos, temp)]


def embed_fwd_ref64(x, w, b, pos, temp, B, T, J):
    C = w.shape[0]
    y = x.double().reshape(B, T, J, -1) @ w.double().t() + b.double() + pos.double().reshape(1, 1, J, C) + temp.double().reshape(1, -1, 1, C)[:, :T]
    return y.reshape(B * T * J, C)


def embed_fwd_model(x, w, b, pos, temp, B, T, J, wrap_bug=False):
    """the fma chain over k from 0, then ((a + b) + pos) + temp.  wrap_bug: the corruption of tests/test_rowerr.py -- the first row after a
    clip wrap (t = 0, j = 0 of every clip but the first) takes temp[t_prev + 1] = temp[T] instead of temp[0]."""
    C, Din = w.shape
    x4 = x.reshape(B, T, J, Din)
    a = torch.zeros(B, T, J, C, dtype=F32, device=x.device)
    for k in range(Din):
        a = x4[..., k:k + 1] * w[:, k] + a
    tt = temp.reshape(1, -1, 1, C)[:, :T].expand(B, T, J, C).clone()
    if wrap_bug:
        tt[1:, 0, 0] = temp.reshape(-1, C)[T]
    return (((a + b) + pos.reshape(1, 1, J, C)) + tt).reshape(B * T * J, C)


def embed_fwd_bound(x, w, b, pos, temp, B, T, J):
    """Gate A: Din fma roundings and three additions, every partial sum bounded by |x| . |w| + |b| + |pos| + |temp|:  gam(Din + 3) x that"""
    C, Din = w.shape
    mag = (x.double().abs().reshape(B, T, J, Din) @ w.double().abs().t() + b.double().abs() + pos.double().abs().reshape(1, 1, J, C)
           + temp.double().abs().reshape(1, -1, 1, C)[:, :T])
    return gam(Din + 3) * mag.reshape(B * T * J, C)


def clip_edges(t2d, B, T, J):
    """[M, C] -> ([B, C] first row of every clip, [B, C] last row of every clip)"""
    t3 = t2d.reshape(B, T * J, -1)
    return t3[:, 0], t3[:, -1]


# ------------------------------------------------------------------------------------------------ embedding backward
def embed_slices(C):
    """(channel quads, LDS clip slices) of embed_bwd_kernel"""
    nq = C // 4
    return nq, max(256 // nq, 1)


def _embed_keep(B, T, J, C, drop_slice, dtype, device):
    keep = torch.ones(B, T, J, 1, dtype=dtype, device=device)
    if drop_slice is not None:
        t, sl = drop_slice
        keep[sl::embed_slices(C)[1], t] = 0
    return keep


def embed_bwd_ref64(dh, x, w, B, T, J, drop_slice=None):
    """dict(dw [C, Din], db [C], dpos [J, C], dtemp [T, C], dx [M, Din]) in float64"""
    C, Din = w.shape
    d = dh.double()
    dk = (d.reshape(B, T, J, C) * _embed_keep(B, T, J, C, drop_slice, d.dtype, d.device))
    return dict(dw=dk.reshape(-1, C).t() @ x.double().reshape(-1, Din), db=dk.sum((0, 1, 2)), dpos=dk.sum((0, 1)),
                dtemp=d.reshape(B, T, J, C).sum((0, 2)), dx=d @ w.double())


def embed_bwd_model(dh, x, w, B, T, J, drop_slice=None):
    """the same sums in torch fp32.  drop_slice = (t, sl): the corruption of tests/test_rowerr.py -- in frame block t the clips b = sl mod ns of
    one LDS slice are missing from dpos, dw and db."""
    C, Din = w.shape
    dk = dh.reshape(B, T, J, C) * _embed_keep(B, T, J, C, drop_slice, F32, dh.device)
    return dict(dw=dk.reshape(-1, C).t() @ x.reshape(-1, Din), db=dk.sum((0, 1, 2)), dpos=dk.sum((0, 1)),
                dtemp=dh.reshape(B, T, J, C).sum((0, 2)), dx=dh @ w)


def embed_bwd_bounds(dh, x, w, B, T, J):
    """Gate A along embed_bwd_kernel (one block per frame t; thread = channel quad x clip slice): a slice adds its per = ceil(B / ns) clips
    in one fma chain (the masked clips of the last group add exact zeros), slice 0 folds the ns slices through LDS (ns - 1 additions), adds
    the J joints into `at` (dtemp, db), and colsum4_kernel<16> folds the T partial rows (dpos, dw, db):
        dtemp  gam(per + ns - 1 + J)              sum_{b, j} |dh|
        dpos   gam(per + ns - 1 + chain(T))       sum_{b, t} |dh|
        db     gam(per + ns - 1 + J + chain(T))   sum |dh|
        dw     gam(J per + ns - 1 + chain(T))     sum |dh| |x|        (one chain over the joints and the clips; the products are inside the fma)
        dx     gam(ceil(C / 64) + 6)              sum_c |dh| |w|      (embed_bwd_dx_kernel: a lane's fma chain, 6 wave levels)"""
    C, Din = w.shape
    nq, ns = embed_slices(C)
    per, fold = cdiv(B, ns), ns - 1
    stride = J * C + C * Din + C
    assert colsum_vec(stride, 0, J * C) and colsum_vec(stride, J * C, C * Din) and colsum_vec(stride, J * C + C * Din, C)
    ch = SE.colsum_chain(T, True)
    a = dh.double().abs()
    a4 = a.reshape(B, T, J, C)
    return dict(dtemp=gam(per + fold + J) * a4.sum((0, 2)), dpos=gam(per + fold + ch) * a4.sum((0, 1)),
                db=gam(per + fold + J + ch) * a4.sum((0, 1, 2)), dw=gam(J * per + fold + ch) * (a.t() @ x.double().abs().reshape(-1, Din)),
                dx=gam(cdiv(C, 64) + 6) * (a @ w.double().abs()))


# ------------------------------------------------------------------------------------------------ adaptive fusion forward
def fuse_inputs(M, C, seed, device, wscale=None):
    """plain Gaussian rows; logits of standard deviation 0.5, so that no alpha is small enough to put a row of d_st / d_ts on gate B's floor"""
    g = torch.Generator().manual_seed(seed)
    x_st, x_ts = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    w = torch.randn(2, 2 * C, generator=g) * (wscale if wscale is not None else 0.5 * (2 * C) ** -0.5)
    b = torch.randn(2, generator=g) * 0.1
    return [t.to(device) for t in (x_st, x_ts, w, b)]


def fuse_plant_logit_gaps(x_st, x_ts, w, b, rows, gaps):
    """move row rows[i] of x_st along w[0, :C] - w[1, :C] (the gradient of l0 - l1 in x_st) so that l0 - l1 = gaps[i] (up to fp32 rounding)"""
    C = x_st.shape[1]
    gdir = (w[0, :C] - w[1, :C]).double()
    cat = torch.cat([x_st, x_ts], -1).double()
    l = cat @ w.double().t() + b.double()
    for r, gap in zip(rows, gaps):
        k = (gap - float(l[r, 0] - l[r, 1])) / float(gdir @ gdir)
        x_st[r] = (x_st[r].double() + k * gdir).float()
    return x_st


def fuse_fwd_ref64(x_st, x_ts, w, b):
    """(out, alpha, logits, amp): amp = |x| . |w| + |b| bounds every partial sum of a logit"""
    cat = torch.cat([x_st, x_ts], -1).double()
    l = cat @ w.double().t() + b.double()
    amp = cat.abs() @ w.double().abs().t() + b.double().abs()
    alpha = torch.softmax(l, -1)
    return x_st.double() * alpha[:, 0:1] + x_ts.double() * alpha[:, 1:2], alpha, l, amp


def fuse_logits_model(x_st, x_ts, w, b):
    """the two logits in fuse_fwd_kernel's order: per lane l = fma(a, w_s, fma(t, w_t, l)) over its slots and elements, wave_sum, + bias.
    A logit's error moves every element of the fused row together, so the model follows the order exactly."""
    M, C = x_st.shape
    A, T_ = lanes(x_st, C), lanes(x_ts, C)
    out = []
    for j in (0, 1):
        Ws, Wt = lanes(w[j:j + 1, :C], C)[0], lanes(w[j:j + 1, C:], C)[0]
        l = torch.zeros(M, 64, dtype=F32, device=x_st.device)
        for k in range(A.shape[1]):
            for i in range(4):
                l = fma32(A[:, k, :, i], Ws[k, :, i], fma32(T_[:, k, :, i], Wt[k, :, i], l))
        out.append(wave_tree(l) + b[j])
    return torch.stack(out, -1)


def fuse_fwd_model(x_st, x_ts, w, b, swap_row=None):
    """fuse_fwd_kernel in torch fp32 with torch.exp for __expf: e = exp(l - max), inv = 1 / (e0 + e1), alpha = e inv,
    out = fma(x_st, a0, x_ts a1).  swap_row: the corruption of tests/test_rowerr.py -- alpha0 and alpha1 exchanged on that row."""
    l = fuse_logits_model(x_st, x_ts, w, b)
    e = torch.exp(l - l.max(-1, keepdim=True).values)
    alpha = e * (1.0 / (e[:, 0:1] + e[:, 1:2]))
    if swap_row is not None:
        alpha[swap_row] = alpha[swap_row].flip(0)
    return fma32(x_st, alpha[:, 0:1], x_ts * alpha[:, 1:2]), alpha


def fuse_alpha_bound(amp64, C, model_alpha, alpha64):
    """Gate A, absolute, per row.  A logit is a lane's chain of 2 fma per element (8 per slot), 6 wave levels and the bias: off by at most
    gam(8 VPL + 7) amp.  alpha0 = sigma(l0 - l1), |sigma'| = alpha (1 - alpha) <= 1 / 4 everywhere, so the logit errors move alpha by at most
    (e0 + e1) / 4.  The rest (exponential, reciprocal, product) is taken from the fp32 model, which uses torch.exp: 2 x its worst error
    against float64 over the rows of the case.  No accuracy of __expf is assumed."""
    el = gam(row_chain(C, 8) + 1) * amp64
    return 0.25 * el.sum(-1, keepdim=True) + 2.0 * float((model_alpha.double() - alpha64).abs().max())


# ------------------------------------------------------------------------------------------------ adaptive fusion backward
def _block_keep(M, cap, drop_block, dtype, device):
    keep = torch.ones(M, 1, dtype=dtype, device=device)
    if drop_block is not None:
        grid, _ = grid_rows(M, cap)
        rows = torch.arange(M, device=device)
        keep[(rows // 4) % grid == drop_block] = 0
    return keep


def fuse_bwd_ref64(dh, x_st, x_ts, alpha, w, drop_block=None):
    """(d_st, d_ts, dw [2, 2C], db [2], dl [M, 2], da [M, 2]) in float64; alpha is an INPUT (fp32 bits)"""
    C = x_st.shape[1]
    d, a, t, al, w64 = dh.double(), x_st.double(), x_ts.double(), alpha.double(), w.double()
    da = torch.stack([(d * a).sum(-1), (d * t).sum(-1)], -1)
    dl = al * (da - (da * al).sum(-1, keepdim=True))
    dlk = dl * _block_keep(d.shape[0], FUSE_BLOCKS, drop_block, d.dtype, d.device)
    dcat = dl @ w64
    return d * al[:, 0:1] + dcat[:, :C], d * al[:, 1:2] + dcat[:, C:], dlk.t() @ torch.cat([a, t], -1), dlk.sum(0), dl, da


def fuse_bwd_model(dh, x_st, x_ts, alpha, w, drop_block=None, dot_fma=None):
    """fuse_bwd_kernel in torch fp32 in the kernel's order: per lane da_i = fma(dh, x_i, da_i) over its slots and elements, wave_sum;
    dot = da0 a0 + da1 a1 as hipcc compiles it (VPL = 1: two packed products and an addition, not contracted; VPL >= 2: fma(da0, a0, da1 a1)),
    dl = alpha (da - dot),
    d_st = fma(dh, a0, fma(dl0, w0s, dl1 w1s)).  da - dot cancels (da_i - dot = a_j (da_i - da_j)), so the roundings of da and dot move
    dl, and with it every element of the row, together: the model follows their order exactly (as ln_fwd_model does for the mean).
    dot_fma: which of the two forms of `dot` (None: the one hipcc 7 compiles at this width).  The source leaves the choice to the compiler's
    contraction, so the GPU test does not rely on it: fuse_bwd_dot_form() reads the form off the kernel's own output.
    drop_block: the corruption of tests/test_rowerr.py -- that block's partial row (its rows' terms) is missing from dw and db."""
    M, C = x_st.shape
    D, A, T_ = lanes(dh, C), lanes(x_st, C), lanes(x_ts, C)
    d0 = torch.zeros(M, 64, dtype=F32, device=dh.device)
    d1 = torch.zeros(M, 64, dtype=F32, device=dh.device)
    for k in range(D.shape[1]):
        for i in range(4):
            d0 = fma32(D[:, k, :, i], A[:, k, :, i], d0)
            d1 = fma32(D[:, k, :, i], T_[:, k, :, i], d1)
    da = torch.stack([wave_tree(d0), wave_tree(d1)], -1)
    if dot_fma is None:
        dot_fma = vpl_for(C) > 1
    if dot_fma:
        dot = fma32(da[:, 0:1], alpha[:, 0:1], da[:, 1:2] * alpha[:, 1:2])
    else:
        dot = da[:, 0:1] * alpha[:, 0:1] + da[:, 1:2] * alpha[:, 1:2]
    dl = alpha * (da - dot)
    dlk = dl * _block_keep(M, FUSE_BLOCKS, drop_block, F32, dh.device)
    r_st = fma32(dh, alpha[:, 0:1], fma32(dl[:, 0:1], w[0, :C], dl[:, 1:2] * w[1, :C]))
    r_ts = fma32(dh, alpha[:, 1:2], fma32(dl[:, 0:1], w[0, C:], dl[:, 1:2] * w[1, C:]))
    return r_st, r_ts, dlk.t() @ torch.cat([x_st, x_ts], -1), dlk.sum(0)


def fuse_bwd_dot_form(d_st, dh, x_st, x_ts, alpha, w):
    """(dot_fma, model outputs): which form of `dot` the kernel that produced d_st was compiled with -- the model whose d_st agrees with it
    in more elements, bit for bit.  The two forms differ by one rounding of a per-row scalar; this identifies the kernel that runs (as
    localerr.attn_bwd_ref has one variant per kernel), it does not widen the gate: the kernel is then judged against that one model."""
    cand = {f: fuse_bwd_model(dh, x_st, x_ts, alpha, w, dot_fma=f) for f in (False, True)}
    agree = {f: int((bits(d_st) == bits(m[0])).sum()) for f, m in cand.items()}
    f = agree[True] > agree[False]
    return f, cand[f], agree


def fuse_bwd_param_bounds(dh, x_st, x_ts, alpha, w):
    """Gate A for the fusion dw / db along fuse_bwd_kernel's summation.  Per row, with E_i = gam(4 VPL + 6) sum |dh x_i| the error of the
    row dot da_i (one fma per element, 6 wave levels):
        dot = da0 a0 + da1 a1      |ddot| <= a0 E0 + a1 E1 + gam(3) (|da0 a0| + |da1 a1|)
        dl_i = a_i (da_i - dot)    |ddl_i| <= a_i (E_i + |ddot|) (1 + 2 U) + gam(2) |dl_i|
    A wave accumulates dl_i x over its rows (at most ceil(M / (4 grid)), products inside the fma), block_fold_store adds the 4 waves
    (2 additions), the colsum folds the `grid` partial rows (dw: colsum4_kernel<16>; db: 2 columns, the scalar colsum_kernel):
        |dw - exact| <= (1 + gam(L)) sum_m |ddl| |x| + gam(L) sum_m |dl x|,  L = rows + 2 + colsum_chain(grid)"""
    M, C = x_st.shape
    d, a, t, al = dh.double(), x_st.double(), x_ts.double(), alpha.double()
    cat = torch.cat([a, t], -1).abs()
    E = gam(row_chain(C, 4)) * torch.stack([(d * a).abs().sum(-1), (d * t).abs().sum(-1)], -1)
    da = torch.stack([(d * a).sum(-1), (d * t).sum(-1)], -1)
    ddot = (al * E).sum(-1, keepdim=True) + gam(3) * (da * al).abs().sum(-1, keepdim=True)
    dl = al * (da - (da * al).sum(-1, keepdim=True))
    ddl = al * (E + ddot) * (1 + 2 * U) + gam(2) * dl.abs()
    grid, rows = grid_rows(M, FUSE_BLOCKS)
    n = 4 * C + 4
    assert colsum_vec(n, 0, 4 * C) and not colsum_vec(n, 4 * C, 2)
    Lw, Lb = rows + 2 + SE.colsum_chain(grid, True), rows + 2 + SE.colsum_chain(grid, False)
    return (1 + gam(Lw)) * (ddl.t() @ cat) + gam(Lw) * (dl.abs().t() @ cat), (1 + gam(Lb)) * ddl.sum(0) + gam(Lb) * dl.abs().sum(0)


# ------------------------------------------------------------------------------------------------ head, tanh backward, average
def head_inputs(M, R, D, seed, device):
    """rep = tanh(.) with a few entries exactly +1, -1 and 0"""
    g = torch.Generator().manual_seed(seed)
    rep = torch.tanh(torch.randn(M, R, generator=g) * 1.5)
    flat = rep.reshape(-1)
    n = flat.numel()
    for i, v in ((0, 1.0), (n // 3, -1.0), (n // 2, 0.0), (n - 1, 1.0), (n - 2, -1.0), (min(n - 1, 5), 0.0)):
        flat[i] = v
    w = torch.randn(D, R, generator=g) * R ** -0.5
    b = torch.randn(D, generator=g) * 0.1
    dout = torch.randn(M, D, generator=g)
    return [t.to(device) for t in (rep, w, b, dout)]


def head_fwd_ref64(rep, w, b):
    return rep.double() @ w.double().t() + b.double()


def head_fwd_model(rep, w, b):
    return rep @ w.t() + b


def head_fwd_bound(rep, w, b):
    """Gate A: a lane's fma chain (4 per slot), 6 wave levels, the bias: gam(4 VPL + 7) (|rep| . |w| + |b|)"""
    return gam(row_chain(rep.shape[1], 4) + 1) * (rep.double().abs() @ w.double().abs().t() + b.double().abs())


def tanh_factor_err(rep64):
    """|fl(1 - r r) - (1 - r^2)|, with or without contraction into one fma: U r^2 + U |1 - r^2| at most (exactly 0 at r = +-1 and r = 0)"""
    return U * (rep64 * rep64 + (1.0 - rep64 * rep64).abs())


def head_bwd_ref64(dout, rep, w):
    """(dpre [M, R], dw [D, R], db [D]) in float64"""
    o = dout.double() @ w.double()
    return o * (1.0 - rep.double() ** 2), dout.double().t() @ rep.double(), dout.double().sum(0)


def head_bwd_model(dout, rep, w, dtype):
    return ((dout @ w) * (1.0 - rep * rep)).to(dtype), dout.t() @ rep, dout.sum(0)


def head_dpre_bound(dout, rep, w, r):
    """Gate A for dpre = (dout . w) (1 - rep^2) rounded to T (r = 2^-8 for bf16, 2^-24 for fp32): o is a chain of Dout fma
    (gam(Dout) |dout| . |w|), the factor carries tanh_factor_err, the product one rounding, the store r:
        r |x| + (1 + r) (gam(Dout) amp (|1 - rep^2| + 2 U) + |o| tanh_factor_err + U |x|) (1 + 2 U)"""
    D = w.shape[0]
    r64 = rep.double()
    o, amp = dout.double() @ w.double(), dout.double().abs() @ w.double().abs()
    x = o * (1.0 - r64 * r64)
    return r * x.abs() + (1 + r) * (gam(D) * amp * ((1.0 - r64 * r64).abs() + 2 * U) + o.abs() * tanh_factor_err(r64) + U * x.abs()) * (1 + 2 * U)


def head_bwd_param_bounds(dout, rep, M, R, D):
    """Gate A for the head dw / db along head_bwd_kernel: a wave accumulates dout * rep over its rows (products inside the fma), block_fold_store
    (2 additions), the colsum over `grid` partial rows (dw: vector; db: vector where Dout % 4 == 0, else scalar)"""
    grid, rows = grid_rows(M, HEAD_BWD_BLOCKS)
    n = D * R + 8
    assert colsum_vec(n, 0, D * R)
    Lw = rows + 2 + SE.colsum_chain(grid, True)
    Lb = rows + 2 + SE.colsum_chain(grid, colsum_vec(n, D * R, D))
    return gam(Lw) * (dout.double().abs().t() @ rep.double().abs()), gam(Lb) * dout.double().abs().sum(0)


def tanh_bwd_ref64(drep, rep):
    return drep.double() * (1.0 - rep.double() ** 2)


def tanh_bwd_model(drep, rep, dtype):
    return (drep * (1.0 - rep * rep)).to(dtype)


def tanh_bwd_bound(drep, rep, r):
    """Gate A: r |x| + (1 + r) (|drep| tanh_factor_err + U |x|) (1 + 2 U)"""
    x = tanh_bwd_ref64(drep, rep)
    return r * x.abs() + (1 + r) * (drep.double().abs() * tanh_factor_err(rep.double()) + U * x.abs()) * (1 + 2 * U)


def average_bound(u, v):
    """Gate A: one rounding of the sum; the halving is exact above the subnormals (2^-150 covers them)"""
    return U * (u.double() + v.double()).abs() * 0.5 + 2.0 ** -150


def average_bwd_bound(dh):
    """Gate A: dh * 0.5 is exact above the subnormals"""
    return torch.full_like(dh.double(), 2.0 ** -150)


# ------------------------------------------------------------------------------------------------ what the old gate saw
def old_gate(name, bad, ref, old_tol):
    """one line: the whole-tensor relative L2 of a corruption next to the tolerance tests/test_gpu_kernels.py holds the same output to"""
    r = LE.rel(torch.nan_to_num(bad.double(), nan=0.0), ref.double())
    return f'{name}: global rel-l2 {r:.2e} against the old tolerance {old_tol:.0e} -> the old gate {"fails it too" if r > old_tol else "LETS IT THROUGH"}'
