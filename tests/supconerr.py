"""Reference, rounding model, bounds and inputs for the one-shot kernels (csrc/oneshot.hip): mbx_supcon_loss (lib/model/loss_supcon.py:57-98 with
contrast_mode 'all', optionally through F.normalize) and mbx_nn_cosine (train_action_1shot.py:58-69).  Plain module, no fixtures:
tests/test_gpu_oneshot.py applies it to the kernels on the GPU, tests/test_supconerr.py to seeded corruptions of the restatement on the CPU.

  supcon_ref64 / nn_ref64   torch restatements in float64 from the same fp32 bits, gradient by autograd, normalisation inside the reference
                            (pinned to the reference's own loss_supcon.py by tests/golden/supcon.npz, tools/mint_supcon.py)
  supcon_model              the kernels' formula in torch fp32, in their operation order
  supcon_bounds             first-order worst-case bounds: of the loss, and per anchor row of dfeat as a max-norm
  nn_sim_bound              first-order worst-case bound of every similarity mbx_nn_cosine compares
  supcon_inputs / nn_inputs seeded inputs whose values are exact in fp32

The temperatures enter the kernel as fp32: the float64 reference takes the SAME fp32 values (f32(0.1), not 0.1)."""
import math

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of fp32
KC = 32                   # OS_KC of oneshot.hip: a dot product starts a new fma chain every 32 columns
MAX_SPLIT = 128           # SC_MAX_SPLIT: workgroups of the Gram pass
U_EXP = 4 * U             # expf / logf within 2 ulp (the HIP math library documents 1 ulp for both)
NORM_EPS = 1e-12          # F.normalize
COS_EPS = 1e-8            # F.cosine_similarity


def f32(v):
    return float(np.float32(v))


def quant(x, bits):
    return torch.round(x * 2.0 ** bits) / 2.0 ** bits


def split_plan(D):
    """(chunks per split, splits) of the Gram pass: sc_cps / sc_nsplit of oneshot.hip"""
    chunks = (D + KC - 1) // KC
    cps = (chunks + MAX_SPLIT - 1) // MAX_SPLIT
    return cps, (chunks + cps - 1) // cps


def row_labels(labels, n_views):
    return labels.reshape(-1).repeat_interleave(n_views)


# ------------------------------------------------------------------------------------------------ float64 restatements
def supcon_terms64(x, lab, t, tb):
    """loss_supcon.py:68-96 on rows x [A,D] (float64, may require grad) with row labels lab [A]; the mean over the anchors does not
    depend on their order, so the rows stay in memory order (the reference stacks them view by view)."""
    A = x.shape[0]
    S = (x @ x.T) / t
    a = S - S.max(1, keepdim=True).values.detach()
    other = ~torch.eye(A, dtype=torch.bool, device=x.device)
    logp = a - torch.log((torch.exp(a) * other).sum(1, keepdim=True))
    pos = ((lab[:, None] == lab[None, :]) & other).to(x.dtype)
    return (-(t / tb) * (pos * logp).sum(1) / pos.sum(1)).mean()


def supcon_ref64(feat, labels, tau, tau_b, normalize, gscale=1.0):
    """(loss, dfeat) in float64 for feat [bsz,n_views,D] fp32 bits; dfeat = gscale * d loss / d feat by autograd"""
    bsz, nv, D = feat.shape
    z = feat.double().detach().requires_grad_(True)
    x = z.reshape(bsz * nv, D)
    if normalize:
        x = torch.nn.functional.normalize(x, dim=-1, eps=NORM_EPS)
    loss = supcon_terms64(x, row_labels(labels, nv), f32(tau), f32(tau_b))
    (loss * gscale).backward()
    return loss.detach(), z.grad


def nn_ref64(anchors, anchor_labels, test, test_labels=None, chunk=256):
    """train_action_1shot.py:61-68 in float64, the broadcast taken `chunk` test rows at a time: (pred index [N], sims [M,N], predicted
    labels [N], accuracy or None)"""
    a = anchors.double().unsqueeze(1)
    sims = torch.cat([torch.nn.functional.cosine_similarity(a, test[n:n + chunk].double().unsqueeze(0), dim=-1)
                      for n in range(0, test.shape[0], chunk)], dim=1)
    idx = torch.argmax(sims, dim=0)
    pred = anchor_labels[idx]
    acc = None if test_labels is None else float((pred == test_labels).double().mean())
    return idx, sims, pred, acc


# ------------------------------------------------------------------------------------------------ the kernels in torch fp32
CORRUPTIONS = ('diag_in_den', 'self_positive', 'no_ratio', 'no_transpose', 'no_projection', 'labels_mod')


def blocked_gram(z):
    """sum_k z_ik z_jk the way supcon_gram_kernel and supcon_row_kernel add it: per 32 columns from zero, chunks in order inside a split,
    splits in order (a chunk's 32 products are one fp32 matmul here: the kernel's is an fma chain in column order)"""
    A, D = z.shape
    cps, nsplit = split_plan(D)
    dot = torch.zeros(A, A, dtype=torch.float32, device=z.device)
    for s in range(nsplit):
        tot = torch.zeros_like(dot)
        for q in range(cps):
            k0 = (s * cps + q) * KC
            if k0 >= D:
                break
            c = z[:, k0:k0 + KC]
            tot = tot + c @ c.T
        dot = dot + tot
    return dot


def supcon_model(feat, labels, tau, tau_b, normalize, gscale=1.0, corrupt=None):
    """mbx_supcon_loss in torch fp32, operation by operation: (loss, dfeat).  corrupt (tests/test_supconerr.py): 'diag_in_den' the diagonal
    stays in the denominator, 'self_positive' the anchor counts among its positives, 'no_ratio' tau / tau_b dropped, 'no_transpose' only
    G applied (an anchor's part as a contrast of the others is lost), 'no_projection' the x (x . g) term of the normalisation's backward
    missing, 'labels_mod' row r labelled labels[r % bsz] instead of labels[r / n_views]."""
    assert corrupt is None or corrupt in CORRUPTIONS
    bsz, nv, D = feat.shape
    A = bsz * nv
    dev = feat.device
    z = feat.float().reshape(A, D)
    t = torch.tensor(f32(tau), dtype=torch.float32, device=dev)
    ratio = t / torch.tensor(f32(tau_b), dtype=torch.float32, device=dev)
    if corrupt == 'no_ratio':
        ratio = torch.ones_like(ratio)
    dot = blocked_gram(z)
    nrm = torch.sqrt(torch.diagonal(dot))
    inv = 1.0 / torch.clamp_min(nrm, f32(NORM_EPS)) if normalize else torch.ones(A, dtype=torch.float32, device=dev)
    S = ((dot * inv[:, None]) * inv[None, :]) / t if normalize else dot / t
    a = S - S.max(1, keepdim=True).values
    eye = torch.eye(A, dtype=torch.bool, device=dev)
    other = ~eye if corrupt != 'diag_in_den' else torch.ones_like(eye)
    e = torch.exp(a) * other
    den = e.sum(1, keepdim=True)
    lse = torch.log(den)
    r = torch.arange(A, device=dev)
    lab = labels.reshape(-1)[r % bsz if corrupt == 'labels_mod' else r // nv]
    pos = ((lab[:, None] == lab[None, :]) & (~eye if corrupt != 'self_positive' else torch.ones_like(eye))).float()
    n = pos.sum(1, keepdim=True)
    loss = (-ratio * ((pos * (a - lse)).sum(1, keepdim=True) / n)).sum() / A
    G = (ratio / A) * (e / den - pos * (1.0 / n))
    W = (G + G.T) / t if corrupt != 'no_transpose' else G / t
    x = z * inv[:, None] if normalize else z
    g = W @ x
    if normalize:
        xg = (x * g).sum(1, keepdim=True)
        inner = torch.where((nrm < f32(NORM_EPS))[:, None], g, g - x * xg) if corrupt != 'no_projection' else g
        g = inner * inv[:, None]
    return loss, (gscale * g).reshape(bsz, nv, D)


# ------------------------------------------------------------------------------------------------ error bounds
def supcon_bounds(feat, labels, tau, tau_b, normalize, gscale=1.0):
    """First-order worst case of mbx_supcon_loss against float64: (loss bound, row bound [A]); |loss - ref| <= loss bound and
    max_k |dfeat[i,k] - ref[i,k]| <= row bound[i].  Correctly rounded +, *, /, sqrt, fma; expf and logf within U_EXP relative.  Every
    quantity below is the float64 value, E_q the bound of the fp32 q's distance from it.
      dot   a product z_ik z_jk passes at most 32 additions of its chunk's fma chain, cps chunk additions and nsplit split additions:
            E_dot = c U sum_k |z_ik z_jk|, c = 32 + cps + nsplit
      norm  the diagonal of dot (all terms positive: relative c U), the root (half of it, + U), the reciprocal (+ U): r_inv = c U / 2 + 2 U,
            which also covers a clamped row (1e-12 as fp32, then the reciprocal: 2 U)
      S     normalised ((dot inv_i) inv_j) / tau: E_S = (E_dot + |dot| (r_inv_i + r_inv_j + 2 U)) inv_i inv_j / tau + U |S|; else E_dot / tau + U |S|
      m     the maximum of perturbed values moves by at most the largest perturbation of the row: E_m = max_j E_S
      a     S - m: E_a = E_S + E_m + U |a|;   e = exp(a): E_e = e (E_a + U_EXP)
      den   128 lanes in a fixed tree of 7 levels: E_den = sum_j E_e + 8 U den;   lse = log den: E_lse = E_den / den + U_EXP |lse|
      lp    a - lse: E_lp = E_a + E_lse + U |lp|;   sp = sum over the positives, the same tree: E_sp = sum E_lp + 8 U sum |lp|
      row   -ratio (sp / n): ratio = tau / tau_b is one division, then a division and a product: E_row = ratio E_sp / n + 3 U |row|
      loss  tree over 128 rows and the division by A: E_loss = (sum E_row + 8 U sum |row|) / A + U |loss|
      p     e / den: E_p = E_e / den + p E_den / den + U p;   q = [pos] (1 / n): E_q = 2 U q
      G     (ratio / A) (p - q): E_G = (ratio / A) (E_p + E_q + U |p - q|) + 3 U |G|;   W = (G + G^T) / tau: E_W = (E_G + E_G^T) / tau + 2 U |W|
      x     z inv under normalize: E_x = |x| (r_inv + U), else exact
      g     a chain of A fmas over j: E_g = E_W |x| + |W| E_x + A U (|W| |x|)
      plain dfeat = gscale g: E = |gscale| (E_g + U |g|)
      norm. xg = x . g: ceil(D / 256) fmas per thread, a wave tree, three additions: E_xg = sum_k (E_x |g| + |x| E_g) + (ceil(D / 256) + 10) U sum_k |x g|
            inner = g - x xg: E_in = E_g + E_x |xg| + |x| E_xg + U |x xg| + U |inner|   (a clamped row: inner = g, E_in = E_g)
            dfeat = gscale (inner inv): E = |gscale| inv (E_in + |inner| (r_inv + 2 U))"""
    bsz, nv, D = feat.shape
    A = bsz * nv
    z = feat.double().reshape(A, D)
    t, tb = f32(tau), f32(tau_b)
    ratio = t / tb
    cps, nsplit = split_plan(D)
    c = KC + cps + nsplit
    az = z.abs()
    dot = z @ z.T
    E_dot = c * U * (az @ az.T)
    if normalize:
        nrm = z.norm(dim=-1)
        inv = 1.0 / nrm.clamp_min(NORM_EPS)
        r_inv = c * U / 2 + 2 * U
        ii = inv[:, None] * inv[None, :]
        S = dot * ii / t
        E_S = (E_dot + dot.abs() * (2 * r_inv + 2 * U)) * ii / t + U * S.abs()
        x = z * inv[:, None]
        E_x = x.abs() * (r_inv + U)
    else:
        S = dot / t
        E_S = E_dot / t + U * S.abs()
        x, E_x = z, torch.zeros_like(z)
    a = S - S.max(1, keepdim=True).values
    E_a = E_S + E_S.max(1, keepdim=True).values + U * a.abs()
    other = (~torch.eye(A, dtype=torch.bool, device=z.device)).double()
    e = torch.exp(a) * other
    E_e = e * (E_a + U_EXP)
    den = e.sum(1, keepdim=True)
    E_den = E_e.sum(1, keepdim=True) + 8 * U * den
    lse = torch.log(den)
    E_lse = E_den / den + U_EXP * lse.abs()
    lp = a - lse
    E_lp = E_a + E_lse + U * lp.abs()
    lab = row_labels(labels, nv)
    pos = (lab[:, None] == lab[None, :]).double() * other
    n = pos.sum(1, keepdim=True)
    E_sp = (pos * E_lp).sum(1, keepdim=True) + 8 * U * (pos * lp.abs()).sum(1, keepdim=True)
    row = -ratio * (pos * lp).sum(1, keepdim=True) / n
    E_row = ratio * E_sp / n + 3 * U * row.abs()
    loss = row.mean()
    E_loss = (E_row.sum() + 8 * U * row.abs().sum()) / A + U * loss.abs()
    p = e / den
    E_p = E_e / den + p * E_den / den + U * p
    q = pos / n
    G = (ratio / A) * (p - q)
    E_G = (ratio / A) * (E_p + 2 * U * q + U * (p - q).abs()) + 3 * U * G.abs()
    W = (G + G.T) / t
    E_W = (E_G + E_G.T) / t + 2 * U * W.abs()
    g = W @ x
    E_g = E_W @ x.abs() + W.abs() @ E_x + A * U * (W.abs() @ x.abs())
    gs = abs(float(gscale))
    if not normalize:
        return E_loss, gs * (E_g + U * g.abs()).max(1).values
    xg = (x * g).sum(1, keepdim=True)
    E_xg = (E_x * g.abs() + x.abs() * E_g).sum(1, keepdim=True) + (math.ceil(D / 256) + 10) * U * (x * g).abs().sum(1, keepdim=True)
    clamped = (nrm < NORM_EPS)[:, None]
    inner = torch.where(clamped, g, g - x * xg)
    E_in = torch.where(clamped, E_g, E_g + E_x * xg.abs() + x.abs() * E_xg + U * (x * xg).abs() + U * inner.abs())
    E = gs * inv[:, None] * (E_in + inner.abs() * (r_inv + 2 * U))
    return E_loss, E.max(1).values


def nn_sim_bound(anchors, test):
    """First-order worst case [M,N] of the similarity mbx_nn_cosine forms, against float64.
      dot   a product passes at most 32 additions of its chunk's fma chain and ceil(D / 32) chunk additions: E_dot = c U sum_k |a_k t_k|
      norm  per column residue a chain of ceil(D / 32) fmas, then 32 additions in column order (the same c); the root halves the relative
            error (+ U); a clamped norm is 1e-8 as fp32 (U): r = c U / 2 + U
      sim   dot / (|a| |t|): the product and the division, U each: E = E_dot / (|a| |t|) + |sim| (r_a + r_t + 2 U)"""
    a, t = anchors.double(), test.double()
    D = a.shape[1]
    c = KC + math.ceil(D / KC)
    na, nt = a.norm(dim=-1).clamp_min(COS_EPS), t.norm(dim=-1).clamp_min(COS_EPS)
    den = na[:, None] * nt[None, :]
    r = c * U / 2 + U
    return c * U * (a.abs() @ t.abs().T) / den + (a @ t.T).abs() / den * (2 * r + 2 * U)


# ------------------------------------------------------------------------------------------------ gates
def supcon_gate(got_loss, got_d, ref_loss, ref_d, b_loss, b_row):
    """(loss ratio, worst row ratio, ok): |loss - ref| / bound and max over the rows of max_k |d - ref| / row bound; both <= 1 to pass.
    A row whose bound is 0 (possible only if its gradient is exactly 0 in every precision) must match exactly."""
    A = b_row.shape[0]
    dl = abs(float(got_loss.double() - ref_loss))
    rl = dl / float(b_loss) if float(b_loss) > 0 else (0.0 if dl == 0 else math.inf)
    err = (got_d.double().reshape(A, -1) - ref_d.reshape(A, -1)).abs().max(1).values
    rr = torch.where(b_row > 0, err / b_row.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ok = bool(np.isfinite(float(got_loss))) and bool(torch.isfinite(got_d).all()) and rl <= 1.0 and float(rr.max()) <= 1.0
    return rl, float(rr.max()), ok


# ------------------------------------------------------------------------------------------------ inputs
def group_labels(sizes, seed):
    """labels with the given class sizes, in a seeded order"""
    lab = torch.cat([torch.full((s,), c, dtype=torch.int64) for c, s in enumerate(sizes)])
    return lab[torch.randperm(len(lab), generator=torch.Generator().manual_seed(seed))]


def supcon_inputs(bsz, n_views, D, seed, device='cpu', spread=None):
    """feat [bsz,n_views,D]: a class direction plus noise, on a 2^-12 grid, scaled by the power of two next to 1 / sqrt(D) so that the rows
    have norms near 1 as a trained embedding's have (every value exact in fp32).  spread = (lo, hi): row r is scaled by a power of two
    between lo and hi (norms over several decades, for `normalize`).  Labels come from CASE_LABELS."""
    g = torch.Generator().manual_seed(seed)
    lab = CASE_LABELS[(bsz, n_views, D)](seed)
    mu = torch.randn(int(lab.max()) + 1, D, generator=g)
    x = quant(0.7 * mu[lab][:, None, :] + torch.randn(bsz, n_views, D, generator=g), 12) * 2.0 ** -round(math.log2(math.sqrt(D)))
    if spread is not None:
        lo, hi = math.log2(spread[0]), math.log2(spread[1])
        ex = torch.round(torch.linspace(lo, hi, bsz * n_views)).reshape(bsz, n_views, 1)
        x = x * 2.0 ** ex
    return x.float().to(device), lab.to(device)


# (bsz, n_views, D) of the GPU test -> labels(seed).  With n_views = 1 every class needs two samples; with 2 views a class of one will do.
CASE_LABELS = {
    (2, 1, 1): lambda seed: torch.zeros(2, dtype=torch.int64),
    (3, 2, 5): lambda seed: group_labels((2, 1), seed),
    (17, 2, 129): lambda seed: group_labels((1, 2, 5, 9), seed),
    (32, 1, 2048): lambda seed: group_labels((2,) * 16, seed),
    (64, 2, 64): lambda seed: group_labels((1, 3, 4, 8, 16, 32), seed),
    (128, 1, 4096): lambda seed: group_labels((2,) * 16 + (4,) * 8 + (8,) * 4 + (32,), seed),
    # small cases of the CPU tests
    (4, 2, 8): lambda seed: group_labels((2, 2), seed),
    (6, 2, 33): lambda seed: torch.tensor([0, 1, 2, 2, 1, 0]),
}
FIXTURE_TAUS = (0.1, 0.07)                      # tests/golden/supcon.npz: the trainer's temperature, the class's default base temperature


def case_seed(shape):
    """the seed of a case of tests/golden/supcon.npz (tools/mint_supcon.py) and of the GPU test"""
    return 2100 + 7 * shape[0] + 3 * shape[1] + shape[2]


def fixture_rows(A, D):
    """anchor rows whose gradient the fixture keeps: all, or the first and last four of a case of more than 16384 elements"""
    return torch.arange(A) if A * D <= 16384 else torch.cat([torch.arange(4), torch.arange(A - 4, A)])


GPU_SHAPES = ((2, 1, 1), (3, 2, 5), (17, 2, 129), (32, 1, 2048), (64, 2, 64), (128, 1, 4096))
TAUS = ((0.1, 0.07), (0.07, 0.07))            # (temperature, base temperature): the trainer's (args.temp, the class default) and the defaults


def nn_inputs(M, N, D, seed, noise, device='cpu'):
    """exemplars: M unit-ish rows (randn / sqrt(D) on a grid); test row n = exemplar (n mod M) + noise * randn / sqrt(D): (anchors [M,D],
    anchor labels [M], test [N,D], test labels [N]).  Labels are 100 + 3 index, so that a label is never an index."""
    g = torch.Generator().manual_seed(seed)
    s = 2.0 ** -round(math.log2(math.sqrt(D)))
    a = quant(torch.randn(M, D, generator=g), 12) * s
    own = torch.arange(N) % M
    t = a[own] + quant(noise * torch.randn(N, D, generator=g), 12) * s
    al = (100 + 3 * torch.arange(M)).to(torch.int32)
    return a.float().to(device), al.to(device), t.float().to(device), al[own].to(device)


NN_SHAPES = ((1, 1, 1), (3, 5, 7), (65, 130, 129), (20, 257, 2048), (20, 4096, 2048))
# |noise| / |exemplar| per case.  Another exemplar's similarity to a test row is about N(0, 1 / D) and the row's own 1 / sqrt(1 + noise^2): the
# noise is scaled to D and M so that the nearest exemplar is the planted one for most rows of every case, and at M = 20, D = 2048 so that the
# float64 accuracy lies in [0.5, 0.9] (the clustered cases); test_supconerr.py asserts NN_ACCURACY on the float64 reference alone.
NN_NOISE = {(1, 1, 1): 0.5, (3, 5, 7): 0.5, (65, 130, 129): 2.0, (20, 257, 2048): 16.0, (20, 4096, 2048): 16.0}
NN_ACCURACY = {(1, 1, 1): (1.0, 1.0), (3, 5, 7): (0.6, 1.0), (65, 130, 129): (0.6, 1.0), (20, 257, 2048): (0.5, 0.9), (20, 4096, 2048): (0.5, 0.9)}
MAX_UNDER_MARGIN = 0.02   # at most 2 % of the rows may have a float64 top-two margin below twice the similarity bound


def nn_margin(sims, bound):
    """float64 top-two margin of every test row [N] and the rows that are units of the exact gate: margin > 2 x the largest bound among the
    row's similarities (M = 1: every row)"""
    if sims.shape[0] == 1:
        return torch.full((sims.shape[1],), math.inf, dtype=torch.float64, device=sims.device), torch.ones(sims.shape[1], dtype=torch.bool, device=sims.device)
    top = torch.topk(sims, 2, dim=0).values
    margin = top[0] - top[1]
    return margin, margin > 2 * bound.max(0).values
