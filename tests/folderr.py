"""References, restatements and gates for the weight-fold, unfold and operand-split kernels of csrc/elementwise.hip: mbx_prep_weights,
mbx_fold_norm_weights, mbx_lnbwd_rowc, mbx_unfold_norm_grads, mbx_split_bf16, mbx_gelu_fwd.  Plain module, no fixtures, any device:
tests/test_gpu_fold_parity.py applies it to the kernels on the GPU, tests/test_folderr.py applies the same gates to the restatements and
to the seeded CORRUPTIONS of them on the CPU.

  *_ref64   the exact operation in float64 from the same fp32 / bf16 bits
  *_model   the kernel's formula in torch fp32 in the kernel's operation order.  Every one of these kernels has a fixed order, so where the
            output is a copy, a product or a short chain the model IS the expected output, bit for bit
  *_bounds  worst-case elementwise bounds for the reduced outputs: a sum in which no term passes through more than L additions is off by
            at most gam(L) sum |terms| (rowerr.gam), whatever the order.  L is counted from the kernel next to each bound
  `corrupt` one of CORRUPTIONS: a named defect planted in a model (never in a kernel), which the gates must see

fmaf is restated by rowerr.fma32, whose float64 intermediate rounds twice.  The two roundings differ from the fused one only where the
float64 sum lands exactly on the midpoint of two fp32 neighbours; fma_ties counts those elements.  Where the count is 0 the model is the
kernel's result without exception; where it is not, at most TIE_CAP of the elements may differ."""
import math

import torch

from tests import localerr as LE
from tests import rowerr as RE
from tests import steperr as SE
from tests.rowerr import BF, F32, U, cdiv, gam

TIE_CAP = 1e-4                # share of the elements of a bit-equal output that may differ where fma32's double rounding can bite
CORRUPTIONS = ('rsum_unrounded', 'bias_from_previous', 'wt_ragged_column_lost', 'lo_from_truncated_hi', 'rowc_odd_block_dropped',
               'rowc_invc_of_k', 'dgamma_after_update', 'dbeta_db_beta', 'dgamma_ragged_block_lost', 'rsum_one_row_one_step',
               'second_pass_skipped')

# (N, K) of one launch: max_n = 1536 and max_k = 1024 come from different descriptors, so the grid (sized by both) has blocks past
# tk * tn of every descriptor, in either direction; ragged tiles in N, in K, in both; a descriptor smaller than one tile
DESC_SET = ((1536, 512), (64, 1024), (200, 72), (65, 33), (33, 95), (3, 5))
DESC_BIAS = (True, False, True, False, True, False)      # one launch mixes descriptors with and without a bias
DESC_SINGLE = ((64, 64),)
ROWC_CASES = ((1, 1, 192), (2, 255, 512), (3, 256, 192), (3, 257, 512), (25, 257, 192), (16, 257, 512), (1, 4131, 512), (2, 1, 512),
              (16, 256, 192), (25, 4131, 512), (25, 1, 192), (3, 4131, 192), (16, 255, 192), (2, 4131, 192))      # (nb, M, C)
UNFOLD_SHAPES = ((1536, 512), (64, 64), (65, 64), (63, 65), (200, 72), (130, 6), (1, 4))      # (N, K)
UNFOLD_VEC = (True, True, True, False, True, False, True)       # colsum4_kernel<16> or the scalar colsum_kernel
GRID_CAP = 256 * 16           # clamp_grid(.., 256 * 16) of mbx_split_bf16 and mbx_gelu_fwd, blocks of 256 threads, one float4 each
FLAT_N = (4, 1028, 4 * 256 * 4096 + 8)        # one vector; a second, partial block; one vector pair past the capped grid
SPLIT_PLANT = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.375, 2.0 ** -120)         # as test_gpu_kernels.test_split_bf16_bits
GELU_PLANT = (-9.0, -6.0, -0.75, -0.0, 0.0, 0.75, 6.0, 9.0, 5.5, -5.5, 1e-30, -1e-30)       # test_gelu_fwd's eight, +-5.5, +-1e-30
GELU_BIN = 0.5
GELU_MULT = 4.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def nan_like(shape, dtype, device):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device=device)


def fma_ties(a, b, c):
    """elements of fma32(a, b, c) whose float64 intermediate sits exactly on an fp32 midpoint (29 low bits 1 0...0): the only ones where
    the double rounding can differ from fmaf -- and only where that float64 sum was itself rounded (TwoSum's error term is not 0): a
    sum that is exact in float64, as after a cancellation, is a true tie, which both round to even."""
    p, c64 = a.double() * b.double(), c.double()          # the product of two fp32 values is exact in float64
    d = (p + c64).contiguous()
    t = d - p
    err = (p - (d - t)) + (c64 - t)
    return int((((d.view(torch.int64) & (2 ** 29 - 1)) == 2 ** 28) & (err != 0)).sum())


class Tally:
    """fma32 with the ties counted"""

    def __init__(self):
        self.ties = 0

    def fma(self, a, b, c):
        self.ties += fma_ties(a, b, c)
        return RE.fma32(a, b, c)


def diff_count(got, want):
    """(elements whose bits differ, flat index of the first)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = (RE.bits(got) != RE.bits(want)).reshape(-1)
    n = int(bad.sum())
    return n, (int(torch.nonzero(bad)[0]) if n else -1)


def tie_gate(got, want, ties):
    """bit-equality with the documented exception: (ok, differing elements, first).  ties == 0: no exception at all."""
    n, first = diff_count(got, want)
    return n == 0 or (ties > 0 and n < TIE_CAP * got.numel()), n, first


def bound_gate(got, ref64, bound64):
    """LE.bound_check on a vector or a matrix"""
    cols = got.shape[-1] if got.dim() > 1 else 1
    return LE.bound_check(got.reshape(-1, cols), ref64.reshape(-1, cols), bound64.reshape(-1, cols))


# ------------------------------------------------------------------------------------------------ prep_weights
PREP_KINDS = {'f32': (0, F32), 'bf16': (1, BF), 'lo': (2, BF)}        # kind -> (dtype code of the C ABI, output type)


def prep_inputs(shapes, seed, device):
    """fp32 weights of scale 3 with the values of SPLIT_PLANT (next to bf16 ties, an exact bf16, a remainder below the subnormals) where
    they fit"""
    g = _gen(seed)
    out = []
    for N, K in shapes:
        w = torch.randn(N, K, generator=g) * 3.0
        n = min(N * K, len(SPLIT_PLANT))
        w.view(-1)[:n] = torch.tensor(SPLIT_PLANT[:n])
        out.append(w.to(device))
    return out


def cvt(v32, kind, corrupt=None):
    """Cvt<T>::from_f of prep_weights_kernel: float, bf16 (nearest even), BfLo = bf16(v - float(bf16(v))) with the subtraction in fp32"""
    if kind == 'f32':
        return v32.clone()
    if kind == 'bf16':
        return RE.bf16_store(v32)
    if corrupt == 'lo_from_truncated_hi':
        return RE.bf16_store(v32 - RE.bf16_trunc(v32).float())
    return RE.split_planes(v32)[1]


def tiled_t(vt, N, corrupt=None):
    """the [K, N] output as the kernel leaves a NaN-filled buffer.  wt_ragged_column_lost: `n0 + cx < N` against N rounded down to the
    tile, so the columns of the ragged last tile are never written"""
    if corrupt != 'wt_ragged_column_lost':
        return vt
    out = nan_like(vt.shape, vt.dtype, vt.device)
    out[:, :N // 32 * 32] = vt[:, :N // 32 * 32]
    return out


def prep_model(w, kind, need_t, corrupt=None):
    """(dst_n [N, K], dst_t [K, N] or None) = (T(w), T(w^T))"""
    return cvt(w, kind, corrupt), (tiled_t(cvt(w.t().contiguous(), kind, corrupt), w.shape[0], corrupt) if need_t else None)


# ------------------------------------------------------------------------------------------------ fold_norm_weights
def fold_inputs(shapes, bias_on, seed, device):
    """per descriptor dict(w, b or None, gamma, beta): w of scale 0.05, gamma = 1 + 0.3 randn with one entry exactly 0.0 and one negative
    (+-0 columns in W', whose sign bit must match), beta of scale 0.2"""
    g = _gen(seed)
    out = []
    for (N, K), has_b in zip(shapes, bias_on):
        w = torch.randn(N, K, generator=g) * 0.05
        b = torch.randn(N, generator=g) if has_b else None
        gamma = 1.0 + 0.3 * torch.randn(K, generator=g)
        gamma[K // 3] = 0.0
        gamma[(2 * K) // 3] = -gamma[(2 * K) // 3].abs() - 0.5
        beta = 0.2 * torch.randn(K, generator=g)
        out.append(dict(w=w.to(device), b=None if b is None else b.to(device), gamma=gamma.to(device), beta=beta.to(device)))
    return out


def fold_w_model(d, need_t, corrupt=None):
    """fold_weights_kernel: W' = bf16(fp32(w gamma)) and its transpose"""
    v = d['w'] * d['gamma']
    return RE.bf16_store(v), (tiled_t(RE.bf16_store(v.t().contiguous()), v.shape[0], corrupt) if need_t else None)


def _lane_chain(t):
    """[N, K] -> [N, ceil(K / 64), 64]: step j of lane l holds k = j * 64 + l (fold_rows_kernel's `k = lane; k += 64`); zeros past K, which
    neither an fma nor an addition sees (the accumulators start at +0 and never become -0)"""
    N, K = t.shape
    n = cdiv(K, 64)
    return torch.nn.functional.pad(t, (0, n * 64 - K)).reshape(N, n, 64)


def fold_rows_ref64(d):
    """(bias_f, rsum) in float64: b + sum_k w beta, and the sum of the ROUNDED folded weights"""
    w64 = d['w'].double()
    bf = (w64 * d['beta'].double()).sum(1)
    if d['b'] is not None:
        bf = bf + d['b'].double()
    return bf, RE.bf16_store(d['w'] * d['gamma']).double().sum(1)


def fold_rows_model(d, corrupt=None, prev=None, row=0):
    """fold_rows_kernel, one wave per row: per lane sb = fmaf(w, beta, sb) and sr += float(bf16(w gamma)) over k = lane, lane + 64, ..,
    wave_sum of each, bias_f = (bias or 0) + sb.  Returns (bias_f, rsum, ties).
    rsum_unrounded: sr from the fp32 product; bias_from_previous: a bias-less descriptor adds the bias of `prev` (the descriptor before
    it); rsum_one_row_one_step: rsum[row] off by one bf16 step of the row's largest |W'|."""
    w, gamma, beta, b = d['w'], d['gamma'], d['beta'], d['b']
    N, K = w.shape
    t = Tally()
    v = w * gamma
    W, Wf = _lane_chain(w), _lane_chain(v if corrupt == 'rsum_unrounded' else RE.bf16_store(v).float())
    Bt = _lane_chain(beta[None])[0]
    sb = torch.zeros(N, 64, dtype=F32, device=w.device)
    sr = torch.zeros(N, 64, dtype=F32, device=w.device)
    for j in range(W.shape[1]):
        sb = t.fma(W[:, j], Bt[j], sb)
        sr = sr + Wf[:, j]
    if b is None and corrupt == 'bias_from_previous':
        b = prev['b'][:N]
    bias_f = (b if b is not None else torch.zeros(N, dtype=F32, device=w.device)) + RE.wave_tree(sb)
    rsum = RE.wave_tree(sr)
    if corrupt == 'rsum_one_row_one_step':
        rsum = rsum.clone()
        rsum[row] += bf16_step(RE.bf16_store(v)[row].float().abs().max())
    return bias_f, rsum, t.ties


def bf16_step(x):
    """the distance between the bf16 neighbours of |x|: 2^(e - 7)"""
    return 2.0 ** (math.floor(math.log2(float(x))) - 7)


def fold_rows_bounds(d):
    """a term enters its lane's chain of n = ceil(K / 64) steps and then the 6 levels of wave_sum: at most L = n + 6 roundings.
        |rsum - exact|   <= gam(L) sum_k |W'|                     (the terms are the exact bf16 values)
        |bias_f - exact| <= gam(L + 1) (sum_k |w beta| + |b|)     (the products are inside the fma; one more addition for the bias)"""
    w64 = d['w'].double()
    L = cdiv(d['w'].shape[1], 64) + 6
    mb = (w64 * d['beta'].double()).abs().sum(1)
    if d['b'] is not None:
        mb = mb + d['b'].double().abs()
    return gam(L + 1) * mb, gam(L) * RE.bf16_store(d['w'] * d['gamma']).double().abs().sum(1)


# ------------------------------------------------------------------------------------------------ lnbwd_rowc
def rowc_inputs(nb, M, seed, device):
    g = _gen(seed)
    part = torch.randn(nb, M, 2, generator=g)
    rstd = torch.randn(M, generator=g).abs() + 0.1
    return part.to(device), rstd.to(device)


def rowc_ref64(part, rstd, C):
    s = part.double().sum(0)
    rs = rstd.double()
    return torch.stack([rs, rs * s[:, 0] / C, rs * s[:, 1] / C, torch.zeros_like(rs)], -1)


def rowc_sanity_bound(part, rstd, C):
    """what the restatement itself may be off by: ceil(nb / 2) chain steps, p + q, two products, the rounded 1 / C"""
    nb = part.shape[0]
    b = gam(cdiv(nb, 2) + 4) * rstd.double()[:, None] * part.double().abs().sum(0) / C
    return torch.cat([torch.zeros_like(b[:, :1]), b, torch.zeros_like(b[:, :1])], -1)


def rowc_model(part, rstd, C, corrupt=None, K=None):
    """lnbwd_rowc_kernel: p sums the blocks 0, 2, 4, .. in order, q the blocks 1, 3, ..; an odd last block goes into p;
    rowc = (rs, (rs (p1 + q1)) invC, (rs (p2 + q2)) invC, 0) with invC = 1.0f / (float)C.  No multiply is followed by an addition, so
    there is nothing for the compiler to contract.  rowc_odd_block_dropped; rowc_invc_of_k: 1 / K of the GEMM instead of 1 / C."""
    nb, M, _ = part.shape
    p = torch.zeros(M, 2, dtype=F32, device=part.device)
    q = torch.zeros(M, 2, dtype=F32, device=part.device)
    b = 0
    while b + 1 < nb:
        p, q = p + part[b], q + part[b + 1]
        b += 2
    if b < nb and corrupt != 'rowc_odd_block_dropped':
        p = p + part[b]
    invC = torch.ones((), dtype=F32, device=part.device) / float(K if corrupt == 'rowc_invc_of_k' else C)
    s = p + q
    return torch.stack([rstd, (rstd * s[:, 0]) * invC, (rstd * s[:, 1]) * invC, torch.zeros_like(rstd)], -1)


# ------------------------------------------------------------------------------------------------ unfold_norm_grads
def unfold_vec(K):
    """launch_colsum2(ws, nblk, 2K, 0, 2K, dgamma, dbeta, split = K): the vector kernel needs ncols, col0, stride AND split to be multiples
    of 4.  colsum_vec states the first three; the second call states `split % 4 == 0` as the offset of the second output"""
    return RE.colsum_vec(2 * K, 0, 2 * K) and RE.colsum_vec(2 * K, K, K)


def unfold_inputs(N, K, seed, device):
    """dw' [N, K], db [N] with one exact zero row, w, gamma, beta with one exact zero"""
    g = _gen(seed)
    dwp, db, w = torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(N, K, generator=g) * 0.05
    gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    db[N // 2] = 0.0
    beta[K // 2] = 0.0
    return [t.to(device) for t in (dwp, db, w, gamma, beta)]


def unfold_ref64(dwp, db, w, gamma, beta):
    """(dw, dgamma, dbeta) in float64; dgamma from dw' as it is BEFORE the in-place update (dwp is never written here)"""
    d, w64 = dwp.double(), w.double()
    return gamma.double() * d + db.double()[:, None] * beta.double(), (w64 * d).sum(0), (w64 * db.double()[:, None]).sum(0)


def colsum_model(part, vec):
    """launch_colsum2 over part [nparts, cols] in the kernels' order.
    colsum4_kernel<16>: part lane pl of 16 walks i = pl, pl + 16, ..; while i + 48 < nparts four accumulators take i, i + 16, i + 32, i + 48;
    the rest goes into a0; (a0 + a1) + (a2 + a3); lane 0 adds the 16 part lanes in order.
    colsum_kernel: the same with 4 groups, and (r0 + r1) + (r2 + r3) at the end."""
    nparts, cols = part.shape
    PL = 16 if vec else 4
    red = []
    for pl in range(PL):
        a = [torch.zeros(cols, dtype=F32, device=part.device) for _ in range(4)]
        i = pl
        while i + 3 * PL < nparts:
            for j in range(4):
                a[j] = a[j] + part[i + j * PL]
            i += 4 * PL
        while i < nparts:
            a[0] = a[0] + part[i]
            i += PL
        red.append((a[0] + a[1]) + (a[2] + a[3]))
    if not vec:
        return (red[0] + red[1]) + (red[2] + red[3])
    t = red[0]
    for q in range(1, PL):
        t = t + red[q]
    return t


def unfold_model(dwp, db, w, gamma, beta, corrupt=None):
    """unfold_norm_grads_kernel + launch_colsum2.  A block is 64 rows x 64 columns; thread (tx, ty) owns column k and the rows
    n = nb0 + ty + 4 i, i < 16: ag = fmaf(w, dw', ag), ab = fmaf(w, db, ab), dw = fmaf(gamma, dw', fp32(db beta)); the four ty are folded
    through LDS, (r0 + r1) + (r2 + r3); the ceil(N / 64) partial rows [dgamma K | dbeta K] go through the colsum.
    Returns (dw, dgamma, dbeta, ties of dw, ties of the chains).
    dgamma_after_update: ag reads the updated dw; dbeta_db_beta: ab = sum db beta; dgamma_ragged_block_lost: the last block's partial
    dgamma row is missing where N is no multiple of 64."""
    N, K = dwp.shape
    td, tc = Tally(), Tally()
    dw = td.fma(gamma[None, :], dwp, db[:, None] * beta[None, :])
    nblk = cdiv(N, 64)

    def blocks(t):      # [N, X] -> [nblk, 16 (i), 4 (ty), X]
        return torch.nn.functional.pad(t, (0, 0, 0, nblk * 64 - N)).reshape(nblk, 16, 4, t.shape[1])
    S, W, D = blocks(dw if corrupt == 'dgamma_after_update' else dwp), blocks(w), blocks(db[:, None])
    ag = torch.zeros(nblk, 4, K, dtype=F32, device=dwp.device)
    ab = torch.zeros(nblk, 4, K, dtype=F32, device=dwp.device)
    for i in range(16):
        ag = tc.fma(W[:, i], S[:, i], ag)
        ab = tc.fma(D[:, i].expand(nblk, 4, K), beta.expand(nblk, 4, K), ab) if corrupt == 'dbeta_db_beta' else tc.fma(W[:, i], D[:, i], ab)
    pg = (ag[:, 0] + ag[:, 1]) + (ag[:, 2] + ag[:, 3])
    pb = (ab[:, 0] + ab[:, 1]) + (ab[:, 2] + ab[:, 3])
    if corrupt == 'dgamma_ragged_block_lost' and N % 64:
        pg[-1] = 0
    out = colsum_model(torch.cat([pg, pb], 1), unfold_vec(K))
    return dw, out[:K].clone(), out[K:].clone(), td.ties, tc.ties


def unfold_chain(N, K):
    """16 fma of the thread, 2 additions of the LDS fold, the colsum's chain over ceil(N / 64) partial rows"""
    return 16 + 2 + SE.colsum_chain(cdiv(N, 64), unfold_vec(K))


def unfold_bounds(dwp, db, w):
    """|dgamma - exact| <= gam(L) sum_n |w dw'|,  |dbeta - exact| <= gam(L) sum_n |w db|,  L = unfold_chain (the products are inside the fma)"""
    L = unfold_chain(*dwp.shape)
    w64 = w.double().abs()
    return gam(L) * (w64 * dwp.double().abs()).sum(0), gam(L) * (w64 * db.double().abs()[:, None]).sum(0)


# ------------------------------------------------------------------------------------------------ split_bf16, gelu_fwd
def first_pass(n):
    """elements the first pass of the grid-stride loop covers: min(ceil(n4 / 256), GRID_CAP) blocks x 256 threads x 4 elements"""
    return min(min(cdiv(n // 4, 256), GRID_CAP) * 1024, n)


def skip_second_pass(out, corrupt):
    """second_pass_skipped: what lies past the first pass stays as the NaN the buffer was filled with"""
    if corrupt == 'second_pass_skipped':
        out = out.clone()
        out[first_pass(out.numel()):] = float('nan')
    return out


def split_inputs(n, seed, device):
    x = torch.randn(n, generator=_gen(seed)) * 3.0
    x[:4] = torch.tensor(SPLIT_PLANT)
    return x.to(device)


def split_model(x, corrupt=None):
    hi, lo = RE.split_planes(x)
    return skip_second_pass(hi, corrupt), skip_second_pass(lo, corrupt)


def gelu_inputs(n, dtype, seed, device):
    """scale 2 with as many of GELU_PLANT as fit (all twelve from 1028 elements on)"""
    u = torch.randn(n, generator=_gen(seed)) * 2.0
    k = min(n, len(GELU_PLANT))
    u[:k] = torch.tensor(GELU_PLANT[:k])
    return u.to(dtype).to(device)


def gelu_ref64(u):
    return LE.gelu64(u.double())


def gelu_model(u, corrupt=None):
    """gelu_fwd_kernel: fp32 erf form of the same bits, one rounding to the output type"""
    return skip_second_pass(torch.nn.functional.gelu(u.float()).to(u.dtype), corrupt)


def gelu_gate(got, ref64, model, u):
    """The gate for rounded outputs, per unit: a unit is one 4-element vector (the kernel loads and stores four at a time), its error the
    largest |x - ref64| of the four.  Units are binned by max |u| in bins of GELU_BIN; a unit must stay within
        max(GELU_MULT x the worst error of the MODEL over the units of its bin,  r x the bin's largest |gelu|)
    r the unit roundoff of the output type.  A non-finite output makes its unit's error infinite.
    Returns dict(ratio, unit, bin, n_over, bins = {bin: (units, kernel worst, model worst, floor, kernel / model)})."""
    r = LE.R_BF16 if got.dtype == BF else LE.R_F32

    def unit_max(t):
        t = torch.where(torch.isfinite(t), t, torch.full_like(t, float('inf')))
        return t.reshape(-1, 4).max(1).values
    eg, em = unit_max((got.double() - ref64).abs()), unit_max((model.double() - ref64).abs())
    b = torch.floor(unit_max(u.double().abs()) / GELU_BIN).long()
    nbin = int(b.max()) + 1
    zero = torch.zeros(nbin, dtype=torch.float64, device=got.device)
    m_bin, g_bin = zero.scatter_reduce(0, b, em, 'amax'), zero.scatter_reduce(0, b, eg, 'amax')
    floor = r * zero.scatter_reduce(0, b, unit_max(ref64.abs()), 'amax')
    limit = torch.maximum(GELU_MULT * m_bin, floor)
    ratio = eg / limit[b].clamp_min(1e-300)
    ratio = torch.where(eg == 0, torch.zeros_like(ratio), ratio)
    k = int(ratio.argmax())
    cnt = torch.bincount(b, minlength=nbin)
    bins = {int(i): (int(cnt[i]), float(g_bin[i]), float(m_bin[i]), float(floor[i]), float(g_bin[i] / m_bin[i]) if m_bin[i] > 0 else float('inf') if g_bin[i] > 0 else 0.0)
            for i in range(nbin) if cnt[i] > 0}
    return dict(ratio=float(ratio[k]), unit=k, bin=int(b[k]), n_over=int((ratio > 1.0).sum()), bins=bins)
