"""Local (per-unit) error metrics for the kernel parity tests.

The per-kernel tests decide with a relative L2 norm over the whole output.  That number tells the error LEVEL; it cannot see a defect
with small SUPPORT (a fragment, a row, one wave's tile), which is how a software-pipelined kernel fails ("Row-owner kernels
for dim_feat 256 -- the bug worth recording").  This module holds the second line of metrics:

  unit_errors        relative L2 per unit (row, (row, head) slice, 32 x 32 MFMA tile, 16-byte fragment, 32-row wave block), worst value
                     WITH its coordinates
  locate             which workgroup tile / wave tile / stream tile a coordinate belongs to, from the geometry the kernel sources state
  elementwise_bound  worst-case bound for an output that sees ONE rounding after an fp32 accumulation; used with no margin
  attn_*             float64 restatements of the attention entries: the exact result and the rounding model (bf16 exactly where the
                     kernels round), so that a kernel is gated against the error the number format forces, not against a tuned number
  mlp_ref            the same pair for the fused MLP forward (the hidden passes through bf16 once)

Plain module: no fixtures, runs on whatever device its tensors live on (tests/test_localerr.py uses it on the CPU,
tests/test_gpu_local_parity.py on the GPU)."""
import math

import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
R_BF16 = 2.0 ** -8        # half a bf16 step relative to the value (8 significand bits): |T(x) - x| <= 2^-8 |x|
R_F32 = 2.0 ** -24
SLAB = 32768              # rows of a float64 product held at once (as tools/rows_soak.py)
FLOOR_FRAC = 0.05         # a unit's denominator is floored at this fraction of the RMS unit norm of the reference
MAX_EXEMPT = 1e-3         # at most 0.1 % of the units of a tensor may sit on that floor


def worst_row(got, ref):
    """max over rows of |got - ref| / |ref|: a handful of wrong rows among 264,384 does not move a relative L2 over all of them (round 6:
    a token fragment read before it had landed; the thresholds are those of tools/rows_soak.py)"""
    g, r = got.float(), ref.float()
    return float(((g - r).norm(dim=-1) / r.norm(dim=-1)).max())


def bf16_round(x):
    """float64 -> the nearest bf16 (ties to even, through fp32: double rounding is impossible to hit short of 2^-29 ties), as float64"""
    return x.float().to(torch.bfloat16).double()


def slabs(M, step=SLAB):
    for r0 in range(0, M, step):
        yield r0, min(M, r0 + step)


# ------------------------------------------------------------------------------------------------ per-unit relative L2
def unit_errors(got, ref64, unit_rows, unit_cols, floor_frac=FLOOR_FRAC, valid=None, full=False):
    """Relative L2 error of every (unit_rows x unit_cols) block of a 2-D output against a float64 reference; ragged last blocks are
    kept (they are the ragged tails of the kernels).  The denominator of a unit is floored at `floor_frac` x the RMS norm a unit of its
    element count has in the reference (root mean square per element x sqrt(elements of the unit): a ragged block is measured against
    blocks of its own size), so that a unit whose exact value is near zero does not decide; `exempt` is the share of units on that
    floor.  A non-finite value in `got` makes its unit's error infinite.  valid: 0 / 1 tensor of the same shape marking padding
    the caller added (it does not count as elements).

    Returns dict(worst, row, col, unit=(i, j), mean, exempt, n_units): `row`, `col` are the first row / column of the worst unit.
    full: also `err` (every unit's error, flat) and `grid` = (flat index -> unit number i * ncols + j, ncols) for per_unit_excess."""
    assert got.dim() == 2 and got.shape == ref64.shape, (got.shape, ref64.shape)
    M, N = got.shape
    d = got.double() - ref64
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    nr, nc = -(-M // unit_rows), -(-N // unit_cols)

    def blocksum(t, square=True):
        t = t * t if square else t
        if N % unit_cols:
            t = torch.nn.functional.pad(t, (0, nc * unit_cols - N))
        t = t.reshape(M, nc, unit_cols).sum(-1)
        if M % unit_rows:
            t = torch.nn.functional.pad(t, (0, 0, 0, nr * unit_rows - M))
        return t.reshape(nr, unit_rows, nc).sum(1)

    e2, r2 = blocksum(d), blocksum(ref64.double())
    cnt = blocksum(torch.ones_like(d) if valid is None else valid.double(), square=False)
    floor2 = (floor_frac ** 2) * float(r2.sum() / cnt.sum()) * cnt
    live = cnt > 0
    e2, r2, floor2 = e2[live].reshape(-1), r2[live].reshape(-1), floor2[live].reshape(-1)
    err = torch.sqrt(e2 / torch.maximum(r2, floor2).clamp_min(1e-300))
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    k = int(torch.nonzero(live.reshape(-1))[int(err.argmax())])
    i, j = k // nc, k % nc
    err_k = float(err.max())
    fin = err[torch.isfinite(err)]
    res = dict(worst=err_k, row=i * unit_rows, col=j * unit_cols, unit=(i, j),
               mean=float(fin.mean()) if fin.numel() else float('inf'), exempt=float((r2 < floor2).double().mean()), n_units=int(live.sum()))
    if full:
        res['err'], res['grid'] = err, (torch.nonzero(live.reshape(-1)).reshape(-1), nc)
    return res


def per_unit_excess(g, m, unit_rows, unit_cols):
    """The per-unit gate for outputs rounded inside the kernel, from two unit_errors(..., full=True) results on the same grid (g: kernel
    against exact, m: rounding model against exact):  err_g(u) <= 2 err_m(u) + 2 mean(err_m)  for EVERY unit u.  Worst-against-worst
    alone lets one ill-conditioned unit of the model (a (row, head) of dq whose exact value nearly cancels carries 20-30 x the mean
    relative error in the model itself) set the gate for all the others; here each unit answers for itself.  Why these terms: kernel and
    model are two realisations of the same roundings, so a unit's two errors share their scale, not their value -- 2 x covers the spread
    of a unit whose error is many independent roundings; a unit dominated by a handful of roundings (one effective key) has a relative
    error of at most a few bf16 half-steps, 2^-8 each, i.e. of the order of the mean, which the additive term covers.
    Returns dict(excess = max over units of err_g / (2 err_m + 2 mean), row, col of that unit)."""
    ratio = g['err'] / (2.0 * m['err'] + 2.0 * m['mean'])
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
    k = int(ratio.argmax())
    idx, nc = g['grid']
    u = int(idx[k])
    return dict(excess=float(ratio[k]), row=(u // nc) * unit_rows, col=(u % nc) * unit_cols, n_over=int((ratio > 1.0).sum()))


UNITS = {'row': lambda N, hd=None: (1, N), 'row_head': lambda N, hd=None: (1, hd), 'tile': lambda N, hd=None: (32, 32),
         'frag': lambda N, hd=None: (1, 8), 'wave_rows': lambda N, hd=None: (32, N)}


def unit_shape(unit, N, hd=None):
    """'row' | 'row_head' (hd columns) | 'tile' (MFMA 32 x 32) | 'frag' (8 elements: one 16-byte store) | 'wave_rows' (32 whole rows)"""
    return UNITS[unit](N, hd)


# ------------------------------------------------------------------------------------------------ where a coordinate lives
# (rows, cols) of the workgroup tile and of one wave's tile, from the constants at the top of the kernel sources.  cols = None: the
# workgroup / wave owns complete rows.
GEOMETRY = {
    'pp256': dict(wg=(256, 256), wave=(128, 64)),        # gemm_nt_pp256_kernel (gemm_pipe.hip): 8 waves, 2 x 4
    'pipe': dict(wg=(256, 128), wave=(64, 64)),          # gemm_nt_pipe_kernel: 8 waves, 4 x 2
    'tn256': dict(wg=(256, 256), wave=(128, 64)),        # gemm_tn_pipe256_kernel: the tile is over (N, K) of dW
    'tn': dict(wg=(256, 128), wave=(64, 64)),            # gemm_tn_pipe_kernel
    'rows_nk': dict(wg=(128, None), wave=(32, None)),    # gemm_rows.hip: R_BM = 128 token rows, 4 waves x 32 rows, K resident
    'rows_n': dict(wg=(128, None), wave=(32, None)),     # gemm_rows_n.hip: RN_BM = 128, N resident
    'mlp': dict(wg=(128, None), wave=(32, None)),        # mlp_fused.hip: F_BM = 128 (4 waves x 32)
    'attn': dict(wave=(32, None)),                       # attention.hip: a 32-row query (key) block per wave; `row` is the sequence index
    'attn_stream': dict(wg=(256, None), wave=(32, None), stream_tile=64),   # attention_stream.hip: MBX_STREAM_BLOCK / _TILE
}
BK = 32     # one k-step of the tile kernels


def locate(row, col, geometry):
    """Which workgroup tile and wave tile (and, streamed attention: which 256-row block, 32-row wave block, 64-row stream tile) the
    element (row, col) falls in -- a pipeline defect should be readable from which wave or stage the worst unit belongs to.  For the
    attention geometries `row` is the index inside the sequence (frame for temporal, joint for spatial)."""
    g = GEOMETRY[geometry]
    out = dict(geometry=geometry, row=int(row), col=int(col))
    if 'wg' in g:
        br, bc = g['wg']
        out['wg'] = (row // br, col // bc if bc else 0)
        r_in, c_in = row % br, (col % bc if bc else col)
    else:
        r_in, c_in = row, col
    wr, wc = g['wave']
    out['wave'] = (r_in // wr, c_in // wc if wc else 0)
    out['row_in_wave'] = r_in % wr
    out['mfma_tile'] = (row // 32, col // 32)
    if 'stream_tile' in g:
        out['stream_tile'] = row // g['stream_tile']
    return out


def where(u, geometry, seq_row=None):
    """One line for a failure message from a unit_errors() / bound_check() result.  seq_row: maps a token row to the index inside its
    sequence (attention: the geometry is over the sequence index)."""
    if seq_row is not None:
        return (f"worst {u.get('worst', u.get('ratio')):.3e} at token row {u['row']}, col {u['col']} -> "
                f"{locate(seq_row(u['row']), u['col'], geometry)}")
    return f"worst {u.get('worst', u.get('ratio')):.3e} at row {u['row']}, col {u['col']} -> {locate(u['row'], u['col'], geometry)}"


# ------------------------------------------------------------------------------------------------ one final rounding: elementwise
GELU_LIP = 1.13           # sup |gelu'| = Phi(u) + u phi(u) at u = sqrt 2: 1.1290
ERF_ABS = 3e-7            # gelu_fast.h: |erf error| <= 1.5e-7 (7.1.26 forms) and <= 3e-7 (7.1.28 form, gelu_fast2)
GELU_EVAL_ABS = 7e-7      # gelu_fast.h: "fp32 evaluation error 7e-7 absolute" of gelu_fast2


def elementwise_bound(x64, amp64, K, r, lip=1.0, ops=1, eabs=0.0, mag64=None):
    """Worst-case |got - x| for an output x = f(sum_k a_k w_k [+ ...]) that is accumulated in fp32 and rounded ONCE to the output type:

        |got - x| <= r |x| + (1 + r) (lip (K 2^-24 amp + ops 2^-24 mag) + eabs)

    x64   the float64 value computed from the same operand bits
    amp64 |a| . |w|^T: the fp32 accumulation of K exact bf16 products is off by at most K 2^-24 of it (each partial sum is bounded by it)
    mag64 a bound on every intermediate of the epilogue (amp + |bias| + ...; default amp): each of the `ops` further fp32 operations
          adds at most 2^-24 of it
    r     2^-8 for a bf16 output (half a step relative to the value), 2^-24 for an fp32 one
    lip   Lipschitz constant of the epilogue in the accumulator
    eabs  absolute error of the epilogue's own function evaluation (e.g. what gelu_fast.h states), may be a tensor
    The (1 + r) carries the rounding of the PERTURBED value.  No margin is added by the callers."""
    mag = amp64 if mag64 is None else mag64
    return r * x64.abs() + (1.0 + r) * (lip * (K * U32 * amp64 + ops * U32 * mag) + eabs)


def tn_splits(M, N, K, x3=False):
    """Token splits of the weight gradient: an independent restatement of the split count in the launch plan of the pipelined kernels
    (tn_plan_pipe -> tnp_splits, gemm_pipe.hip; TnPlan, mbx_common.h) with its tile constants (256 x 256 tiles and
    32-token chunks where N, K >= 256, else 256 x 128 and 64-token chunks; X3 walks three passes of chunks).  The test checks it against the
    library's workspace size wherever that size determines it."""
    big = N >= 256 and K >= 256          # (tnp_splits takes the tile shape from N, K alone, also for X3)
    bn, bk, bms = (256, 256, 32) if big else (256, 128, 64)
    tiles = -(-N // bn) * -(-K // bk)
    nchunks = (3 if x3 else 1) * -(-M // bms)
    s = 0
    for w in range(1, 5):
        if (256 * w) % tiles == 0 and ((256 * w) // tiles) % 8 == 0 and (256 * w) // tiles <= 128:
            s = (256 * w) // tiles
            break
    if s == 0 and big:
        best = 1e30
        for c in range(8, 257, 8):
            rounds, cps = (tiles * c + 255) // 256, (nchunks + c - 1) // c
            cost = rounds * cps + c * N * K * 8.0 / 4e6
            if cost < best:
                best, s = cost, c
    if s == 0:
        s = min(128, ((512 // tiles + 7) // 8) * 8)
    return max(1, min(s, nchunks))


def split_sum_bound(x64, amp64, n_terms, splits, r=R_F32, slack=64):
    """The weight gradient's structure (gemm_pipe.hip, mbx_launch_gemm_tn_pipe / _x3): the n_terms token products are divided over `splits`
    workgroups per output tile, each accumulating its ceil(n_terms / splits) (+ one chunk of at most `slack` tokens of rounding-up)
    products in fp32, and the `splits` partial tiles are summed in fp32 by a column-sum pass:

        |got - x| <= r |x| + (1 + r) (ceil(n_terms / splits) + slack + splits) 2^-24 amp"""
    per = -(-n_terms // splits) + slack
    return r * x64.abs() + (1.0 + r) * (per + splits) * U32 * amp64


def bound_check(got, x64, bound64):
    """max over elements of |got - x| / bound (must be <= 1), its coordinates, and the number of violations; non-finite counts."""
    d = (got.double() - x64).abs()
    ratio = d / bound64.clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
    k = int(ratio.argmax())
    N = got.shape[-1]
    return dict(ratio=float(ratio.reshape(-1)[k]), row=k // N, col=k % N, violations=int((ratio > 1.0).sum()))


def gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad64(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def gelu_eabs(u64):
    """absolute error of the fast erf-GELU forms of gelu_fast.h at pre-activation u: |u| / 2 x the erf error + the stated evaluation error"""
    return 0.5 * u64.abs() * ERF_ABS + GELU_EVAL_ABS


def gelu_grad_eabs(u64):
    """gelu' = (1 + erf) / 2 + u phi(u) from the 7.1.26 parts: half the erf error, the Gaussian (v_exp_f32, 1 ulp, times |u| / sqrt(2 pi)) and
    ten fp32 operations on values <= 1.13"""
    return 0.5 * ERF_ABS + (2.0 * u64.abs() * 0.4 + 10 * 1.13) * U32


# ------------------------------------------------------------------------------------------------ global rel-L2 (the existing gate)
def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def scaled_global(rel_small, n_small, n_large):
    """What a defect of FIXED support that gives `rel_small` over n_small elements gives over n_large elements of the same statistics:
    the error norm stays, the reference norm grows with sqrt(elements)."""
    return rel_small * math.sqrt(n_small / n_large)


# ------------------------------------------------------------------------------------------------ attention in float64
def _qkv5(qkv, B, T, J, H):
    C = qkv.shape[-1] // 3
    q5 = qkv.double().reshape(B, T, J, 3, H, C // H)
    return q5[:, :, :, 0], q5[:, :, :, 1], q5[:, :, :, 2]


def _seq_first(x, mode_temporal):
    """[B,T,J,H,d] -> [problems..., L, d]: temporal [B,J,H,T,d], spatial [B,T,H,J,d]"""
    return x.permute(0, 2, 3, 1, 4) if mode_temporal else x.permute(0, 1, 3, 2, 4)


def _seq_back(x, mode_temporal):
    return x.permute(0, 3, 1, 2, 4) if mode_temporal else x.permute(0, 1, 3, 2, 4)


def attn_mask(B, T, J, H, temporal, drop, device):
    """keep / (1 - p) over the reference's attn tensor, in this module's problem-major layout ([B,J,H,T,T] temporal -- the reference's
    is [B,H,J,T,T] -- and [B,T,H,J,J] spatial); None without dropout.  drop = (p, seed) or (p, seed, clips): the B clips given are the
    clips of those numbers in a LARGER batch, over whose attention tensor the mask index runs (tests/test_gpu_big_rows.py)"""
    if drop is None or drop[0] <= 0:
        return None
    from motionbert_amd.dropmask import keep, mask_like
    if len(drop) > 2:
        per = H * J * T * T if temporal else T * H * J * J      # elements of one clip: the batch index is outermost in both layouts
        idx = torch.tensor(list(drop[2]), dtype=torch.int64, device=device)[:, None] * per + torch.arange(per, dtype=torch.int64, device=device)[None, :]
        m = (keep(idx, drop[0], drop[1]).float() / (1.0 - drop[0])).double()      # (in fp32 first, as mask_like on an fp32 tensor)
        return m.reshape(B, H, J, T, T).permute(0, 2, 1, 3, 4) if temporal else m.reshape(B, T, H, J, J)
    if temporal:
        return mask_like(torch.empty(B, H, J, T, T, device=device), drop[0], drop[1]).permute(0, 2, 1, 3, 4).double()
    return mask_like(torch.empty(B, T, H, J, J, device=device), drop[0], drop[1]).double()


def attn_fwd_ref(qkv, B, T, J, H, scale, temporal, model, drop=None, skip=None):
    """o [M, C] and lse [M, H] in float64 from the bf16 operand bits.

    model = False: the exact softmax(q k^T scale) v.
    model = True : the roundings of attn_fwd_kernel (attention.hip) / the streamed forward: the probabilities relative to the row
                   maximum, p = exp(s - max), go to bf16 before the P.V MFMA (MmaCols: pack_bf2 of the B operand) while the row sum is
                   taken from the unrounded fp32 p; o = acc / l is rounded to bf16 once (store_rowfrag).  lse is not rounded.
    skip = (problem index tuple, query block (q0, q1), key tile (k0, k1)): test_localerr.py's corruption -- those keys are left out of
                   those queries' softmax."""
    q, k, v = (_seq_first(t, temporal) for t in _qkv5(qkv, B, T, J, H))
    s = (q @ k.transpose(-1, -2)) * scale
    if skip is not None:
        idx, (q0, q1), (k0, k1) = skip
        s[idx + (slice(q0, q1), slice(k0, k1))] = float('-inf')
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    mk = attn_mask(B, T, J, H, temporal, drop, qkv.device)
    pm = p if mk is None else p * mk          # the mask multiplier is applied in fp32, before the pack
    if model:
        pm = bf16_round(pm)
    o = (pm @ v) / l
    if model:
        o = bf16_round(o)
    M = qkv.shape[0]
    o = _seq_back(o, temporal).reshape(M, -1)
    lse = (lse.permute(0, 3, 1, 2) if temporal else lse.permute(0, 1, 3, 2)).reshape(M, H)
    return o, lse


def attn_bwd_ref(qkv, o, do, lse, B, T, J, H, scale, temporal, model, drop=None, delta_rows=None, variant='fused'):
    """dqkv [M, 3C] in float64.  lse is the float64 log-sum-exp of the rows; o, do the bf16 tensors the kernel reads.

    model = False: the exact gradient of softmax attention for the probabilities exp(s - lse) and delta = rowsum(dO o64) with o64 the
                   UNROUNDED output (what autograd computes).
    model = True : the roundings of the bf16 backward kernels, which differ (`variant`):
        'fused'  attn_bwd_fused_kernel (attention.hip:700-751; 32 < L <= 256 without dropout): delta = rowsum(dO o) from the bf16 o; P goes
                 to bf16 before the P^T.dO MFMA (dV); dS / scale = p (dP - delta) goes to bf16 before the dS.K and dS^T.Q MFMAs and the
                 softmax scale is applied to the fp32 accumulators (:710, :751)
        'split'  attn_bwd_dq_kernel / attn_bwd_dkv_kernel (attention.hip:194-216, :312; dropout with L > 32) and the streamed pair
                 (attention_stream.hip:232-262, :395): delta from the bf16 o as above; dS = p (dP - delta) scale is rounded WITH the scale
        'small'  attn_bwd_small_kernel (attention.hip:439-454, :484-487; L <= 32): delta = rowsum(P o dP) in fp32 from the fragments -- o is
                 not read at all -- and dS = p (dP - delta) scale is rounded with the scale
                 dq / dk / dv are rounded to bf16 once in every variant.
    o: for model = False pass the float64 exact output.  delta_rows = (src, dst): test_localerr.py's corruption -- token row dst takes
                   the delta of token row src."""
    q, k, v = (_seq_first(t, temporal) for t in _qkv5(qkv, B, T, J, H))
    hd = q.shape[-1]
    M = qkv.shape[0]
    do5 = do.double().reshape(B, T, J, H, hd)
    l4 = lse.double().reshape(B, T, J, H)
    ll = (l4.permute(0, 2, 3, 1) if temporal else l4.permute(0, 1, 3, 2))[..., None]
    dos = _seq_first(do5, temporal)
    p = torch.exp((q @ k.transpose(-1, -2)) * scale - ll)
    dp = dos @ v.transpose(-1, -2)
    mk = attn_mask(B, T, J, H, temporal, drop, qkv.device)
    pd = p
    if mk is not None:
        dp, pd = dp * mk, p * mk
    if model and variant == 'small':
        dl = (p * dp).sum(-1, keepdim=True)                              # problem-major [..., L, 1]
        if delta_rows is not None:
            raise ValueError('delta_rows is a corruption of the kernels that read delta per token row')
    else:
        delta = (do5 * o.double().reshape(B, T, J, H, hd)).sum(-1)        # [B,T,J,H]
        if delta_rows is not None:
            dflat = delta.reshape(M, H).clone()
            dflat[delta_rows[1]] = dflat[delta_rows[0]]
            delta = dflat.reshape(B, T, J, H)
        dl = (delta.permute(0, 2, 3, 1) if temporal else delta.permute(0, 1, 3, 2))[..., None]
    ds = p * (dp - dl)
    if model and variant == 'fused':
        ds, pd = bf16_round(ds), bf16_round(pd)
        dq, dk = (ds @ k) * scale, (ds.transpose(-1, -2) @ q) * scale
    else:
        ds = ds * scale
        if model:
            ds, pd = bf16_round(ds), bf16_round(pd)
        dq, dk = ds @ k, ds.transpose(-1, -2) @ q
    dv = pd.transpose(-1, -2) @ dos
    out = torch.stack([_seq_back(t, temporal) for t in (dq, dk, dv)], 3).reshape(M, -1)      # [B,T,J,3,H,hd]
    return bf16_round(out) if model else out


def attn_stats_ref(dqkv, qkv, bias_f, rsum, H):
    """part [2H, M, 2] of mbx_attn_bwd_stats from a given (rounded) dqkv: per (token, head) the dots with rsum and (qkv - bias_f) over the
    head's q columns (role 0) and its k + v columns (role 1); both vectors enter as bf16 (packed-bf16 dot products, attention_common.h)."""
    M = dqkv.shape[0]
    rb, bb = bf16_round(rsum.double()), bf16_round(bias_f.double())
    d = dqkv.double().reshape(M, 3, H, -1)
    y = (qkv.double() - bb).reshape(M, 3, H, -1)
    t1, t2 = (d * rb.reshape(1, 3, H, -1)).sum(3), (d * y).sum(3)
    amp = (d.abs() * rb.abs().reshape(1, 3, H, -1)).sum(3), (d.abs() * y.abs()).sum(3)
    f = lambda t: torch.stack([torch.stack([t[0][:, 0], t[0][:, 1] + t[0][:, 2]], -1), torch.stack([t[1][:, 0], t[1][:, 1] + t[1][:, 2]], -1)], -1)
    return f((t1, t2)).reshape(M, 2 * H, 2).transpose(0, 1), f(amp).reshape(M, 2 * H, 2).transpose(0, 1)


# ------------------------------------------------------------------------------------------------ the fused MLP in float64
def mlp_ref(a, w1, b1, w2, b2, resid, model, r0=0, r1=None):
    """y = resid + gelu(a . W1^T + b1) . W2^T + b2 for rows r0:r1, float64, operand bits as given (a: the normalised bf16 operand).
    model = True: the hidden gelu(.) passes through bf16 once (mlp_fused.hip packs it for the second MFMA; tests/mock_ops.py states the
    same in fp32).  The fp32 output y sees no further rounding worth modelling (2^-24)."""
    sl = slice(r0, r1)
    g = gelu64(a[sl].double() @ w1.double().t() + b1.double())
    if model:
        g = bf16_round(g)
    return resid[sl].double() + g @ w2.double().t() + b2.double()


def row_abs_rel_check(got, ref64, abs_tol64, rel_tol):
    """per-row fp32 statistics (lse, mean, rstd, part): max of |got - ref| / (abs_tol + rel_tol |ref|) and where"""
    d = (got.double() - ref64).abs() / (abs_tol64 + rel_tol * ref64.abs()).clamp_min(1e-300)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    k = int(d.argmax())
    n = got.shape[-1] if got.dim() > 1 else 1
    return dict(ratio=float(d.reshape(-1)[k]), row=k // n, col=k % n)
