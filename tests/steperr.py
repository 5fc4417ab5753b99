"""References, rounding models and gates for the kernels of csrc/train_step.hip (pose loss, 2D loss, AdamW, dropout / DropPath, the
ActionNet pooling).  Plain module, no fixtures: tests/test_gpu_step_parity.py applies it to the kernels on the GPU, tests/test_steperr.py
applies the same gates to seeded corruptions of the restatements on the CPU.

  *_ref64    the exact operation in float64 from the same fp32 bits
  *_model    the kernel's documented formula in torch fp32, in the kernel's operation order (the "rounding model" of gate B)
  *_bound    worst-case elementwise bounds (gate A), derived where they are defined
  gate_units gate B: the worst unit of got-vs-float64 within 2 x the worst unit of model-vs-float64; at most LE.MAX_EXEMPT of the units on the floor"""
import math

import torch

from motionbert_amd import dropmask
from tests import localerr as LE

U = LE.U32


def f32(x):
    """the value a C float argument takes"""
    return float(torch.tensor(x, dtype=torch.float32))


def quant(x, bits):
    return torch.round(x * 2.0 ** bits) / 2.0 ** bits


# ------------------------------------------------------------------------------------------------ gate B
def gate_units(got, ref64, model, cols, floor_frac=LE.FLOOR_FRAC):
    """got, ref64, model: [units, cols].  Returns (g, m, ok, message); ok <=> worst(got) <= 2 worst(model) and the floor exempts <= 0.1 %."""
    g, m = LE.unit_errors(got, ref64, 1, cols, floor_frac=floor_frac), LE.unit_errors(model, ref64, 1, cols, floor_frac=floor_frac)
    ok = m['exempt'] <= LE.MAX_EXEMPT and g['worst'] <= 2.0 * m['worst']
    return g, m, ok, f'kernel {g["worst"]:.3e} vs 2 x model {m["worst"]:.3e} at unit {g["row"]}; {m["exempt"]:.2%} of the units on the floor'


def boundary_pairs(x, B, T):
    """[B, T, ...] -> [B, 2 * rest]: the last frame of clip b next to the first frame of clip (b + 1) % B -- the two frames that must not
    exchange a velocity term"""
    x = x.reshape(B, T, -1)
    return torch.cat([x[:, T - 1], x[torch.arange(1, B + 1) % B, 0]], -1)


# ------------------------------------------------------------------------------------------------ pose loss
def pose_inputs(B, T, J, seed, device, plant=True):
    """gt skeleton-scaled with the root joint exactly 0, pred = gt + noise.  gt lies on a 2^-10 grid and the noise on a 2^-16 grid, so that
    pred - gt and the frame differences are exact in fp32 AND in float64: a planted zero norm is zero in both, whatever the order of the
    subtractions.  Planted (clips with T >= 7, J > 1): clip b % 8 == 0 a frame with pred == gt in every joint; b % 8 == 1 two consecutive
    frames with identical residuals (zero velocity norm); every clip one isolated joint with pred == gt."""
    g = torch.Generator().manual_seed(seed)
    gt = quant(torch.randn(B, T, J, 3, generator=g) * 0.3, 10)
    gt[:, :, 0] = 0
    noise = quant(torch.randn(B, T, J, 3, generator=g) * 0.03, 16)
    noise = torch.where(noise == 0, torch.full_like(noise, 2.0 ** -16), noise)
    if plant and T >= 7 and J > 1:
        for b in range(B):
            if b % 8 == 0:
                noise[b, 2] = 0
            if b % 8 == 1:
                noise[b, 5] = noise[b, 4]
            noise[b, (b * 5 + 3) % T if (b * 5 + 3) % T != 2 else 3, 1 + b % (J - 1)] = 0
    return (gt + noise).to(device), gt.to(device)


def pose_ref64(pred, gt, ls, lv, gscale):
    """float64 autograd of the restated reference losses (tests/test_gpu_train.py, pinned to the real reference by tests/golden)"""
    from tests.test_gpu_train import _ref_losses
    p = pred.double().detach().requires_grad_(True)
    r = _ref_losses(p, gt.double(), ls, lv)
    (r[3] * gscale).backward()
    return torch.stack([v.detach() for v in r]), p.grad


def _norm3(x):      # norm3 of train_step.hip: sqrt(fma(x, x, fma(y, y, z z)))
    return torch.sqrt(x[..., 0] * x[..., 0] + (x[..., 1] * x[..., 1] + x[..., 2] * x[..., 2]))


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def pose_model(pred, gt, ls, lv, gscale, leak=None):
    """pose_loss_kernel in torch fp32, operation by operation (sums over the joints of a frame with torch.sum for the wave reduction).
    leak = b: the corruption of tests/test_steperr.py -- the last frame of clip b takes a velocity term from the first frame of clip b + 1."""
    B, T, J, _ = pred.shape
    one = torch.ones((), dtype=torch.float32, device=pred.device)
    inv_n = one / float(B * T * J)
    inv_nv = one / float(B * (T - 1) * J) if T > 1 else one * 0
    zero = torch.zeros((), dtype=torch.float32, device=pred.device)
    r = pred - gt
    n1 = _norm3(r)
    i1 = torch.where(n1 > 0, 1.0 / n1, zero)
    grad = r * i1[..., None] * inv_n
    a, b = _dot3(gt, pred).sum(-1)[..., None, None], _dot3(pred, pred).sum(-1)[..., None, None]
    s = a / b
    q = s * pred - gt
    n2 = _norm3(q)
    e = q * torch.where(n2 > 0, 1.0 / n2, zero)[..., None]
    c = _dot3(e, pred).sum(-1)[..., None, None]
    k1, k2 = c / b, 2.0 * a * c / (b * b)
    grad = grad + (ls * inv_n) * (s * e + k1 * gt - k2 * pred)
    if T > 1:
        d = (pred[:, 1:] - pred[:, :-1]) - (gt[:, 1:] - gt[:, :-1])
        n3 = _norm3(d)
        u = d * torch.where(n3 > 0, (lv * inv_nv) / n3, zero)[..., None]
        grad[:, 1:] += u
        grad[:, :-1] -= u
        if leak is not None:
            dx = (pred[leak + 1, 0] - pred[leak, T - 1]) - (gt[leak + 1, 0] - gt[leak, T - 1])
            nx = _norm3(dx)
            grad[leak, T - 1] -= dx * torch.where(nx > 0, (lv * inv_nv) / nx, zero)[..., None]
    return gscale * grad


def colsum_chain(nparts, vec):
    """the longest chain of fp32 additions a partial passes through in mbx_launch_colsum (elementwise.hip).  colsum4_kernel<16> (ncols = stride
    = 4): 16 part lanes, each ceil(nparts / 16) partials over 4 accumulators, (a0 + a1) + (a2 + a3), then 15 serial additions over the
    part lanes.  colsum_kernel (ncols = 1): 4 groups, 4 accumulators each, two levels, two levels."""
    if vec:
        return -(-(-(-nparts // 16)) // 4) + 2 + 15
    return -(-(-(-nparts // 4)) // 4) + 2 + 2


def pose_loss_bounds(pred, gt, ls, lv):
    """Gate A for the four scalars {mpjpe, n_mpjpe, velocity, total}: first-order worst case of pose_loss_kernel + colsum4_kernel<16>.
    correctly rounded +, *, /, sqrt, fma (hipcc's default); |.| below are float64 values from the same bits.
      mpjpe     r_c = p_c - g_c: one rounding, U (|p_c| + |g_c|); norm3: three fma roundings on the sum of squares (half each after the root)
                and the root: <= 3 U n1 <= 3 U A1, A1 = |(|p| + |g|)|_2  ->  per joint 4 U A1
      n_mpjpe   a, b: per lane 3 products + 2 additions, 6 tree levels: 9 U (sum |g||p|), 9 U b; s = a / b: |ds| <= |s| (9 U sum|g||p| / |a| + 10 U);
                q_c = s p_c - g_c: two roundings on |s p_c| + |g_c|; norm3 as above  ->  per joint |ds| |p|_2 + 5 U A2, A2 = |(|s||p| + |g|)|_2
      velocity  d_c = (p_t - p_t-1) - (g_t - g_t-1): three roundings, each <= U A3c, A3c = |p_t| + |p_t-1| + |g_t| + |g_t-1|; norm3  ->  5 U A3
      per frame the wave sum (6 levels) and the product with 1 / n (the reciprocal, the product): 8 U x the frame's partial
      total     s1 + ls s2 + lv s3: four more roundings on |s1| + ls |s2| + lv |s3|
      colsum    chain x U x sum |partials| (all partials are >= 0)
    Returns a float64 tensor of 4 bounds."""
    B, T, J, _ = pred.shape
    p, g = pred.double(), gt.double()
    n, nv = B * T * J, max(B * (T - 1) * J, 1)
    chain = colsum_chain(B * T, True)
    nrm = lambda x: x.norm(dim=-1)
    n1 = nrm(p - g)
    e1 = 4 * U * nrm(p.abs() + g.abs())
    a, b = (g * p).sum((-1, -2), keepdim=True), (p * p).sum((-1, -2), keepdim=True)
    aa = (g.abs() * p.abs()).sum((-1, -2), keepdim=True)
    s = a / b
    ds = s.abs() * (9 * U * aa / a.abs().clamp_min(1e-300) + 10 * U)
    n2 = nrm(s * p - g)
    e2 = ds[..., 0] * nrm(p) + 5 * U * nrm(s.abs() * p.abs() + g.abs())
    out = []
    parts = []
    for val, err, cnt in ((n1, e1, n), (n2, e2, n)):
        parts.append(val.sum() / cnt)
        out.append((err.sum() + 8 * U * val.sum()) / cnt)
    if T > 1:
        n3 = nrm((p[:, 1:] - p[:, :-1]) - (g[:, 1:] - g[:, :-1]))
        e3 = 5 * U * nrm(p[:, 1:].abs() + p[:, :-1].abs() + g[:, 1:].abs() + g[:, :-1].abs())
        parts.append(n3.sum() / nv)
        out.append((e3.sum() + 8 * U * n3.sum()) / nv)
    else:
        parts.append(n1.sum() * 0)
        out.append(n1.sum() * 0)
    mag = parts[0] + ls * parts[1] + lv * parts[2]
    out.append(out[0] + ls * out[1] + lv * out[2] + 4 * U * mag)
    parts.append(mag)
    return torch.stack([(o + chain * U * q) * (1 + U) for o, q in zip(out, parts)])


# ------------------------------------------------------------------------------------------------ 2D loss
def loss2d_inputs(B, T, J, seed, device):
    """batch [B,T,J,3]: x, y and the confidence in channel 2 (a tenth of them exactly 0 where J > 1); pred [B,T,J,3]"""
    g = torch.Generator().manual_seed(seed)
    batch = torch.randn(B, T, J, 3, generator=g) * 0.4
    conf = torch.rand(B, T, J, generator=g)
    zero = torch.rand(B, T, J, generator=g) < 0.1
    if J == 1:      # a frame is one joint: a zero confidence would make the whole unit's gradient 0 (it would sit on the floor of gate B)
        zero[:] = False
    batch[..., 2] = torch.where(zero, torch.zeros_like(conf), 0.05 + conf)
    pred = batch + torch.randn(B, T, J, 3, generator=g) * 0.05
    return pred.to(device), batch.to(device)


def loss2d_ref64(pred, target, conf, gscale):
    from tests.test_gpu_train import _ref_loss_2d
    p = pred.double().detach().requires_grad_(True)
    r = _ref_loss_2d(p, target.double(), conf.double()[..., None])
    (r * gscale).backward()
    return r.detach(), p.grad


def loss2d_model(pred, target, conf, gscale):
    """loss_2d_kernel in torch fp32"""
    B, T, J, _ = pred.shape
    one = torch.ones((), dtype=torch.float32, device=pred.device)
    inv_n = one / float(B * T * J)
    r = (pred[..., :2] - target[..., :2]) * conf[..., None]
    nrm = torch.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1])
    inv = torch.where(nrm > 0, conf * inv_n / nrm, one * 0)
    out = torch.zeros_like(pred)
    out[..., :2] = gscale * (r * inv[..., None])
    return out


def loss2d_bound(pred, target, conf):
    """Gate A for the scalar: r_c = (p_c - t_c) conf: two roundings on (|p_c| + |t_c|) |conf|; the norm: two fma roundings (half each after the
    root) and the root, <= 3 U nrm <= 3 U A, A = |conf| |(|p| + |t|)|_2  ->  per joint 5 U A; the wave sum and the product with 1 / n: 8 U x
    the frame's partial; colsum_kernel's chain x U x the sum of the (non-negative) partials."""
    B, T, J, _ = pred.shape
    p, t, c = pred.double()[..., :2], target.double()[..., :2], conf.double()
    nrm = ((p - t) * c[..., None]).norm(dim=-1)
    amp = c.abs() * (p.abs() + t.abs()).norm(dim=-1)
    n = B * T * J
    return ((5 * U * amp.sum() + 8 * U * nrm.sum()) / n + colsum_chain(B * T, False) * U * nrm.sum() / n) * (1 + U)


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_ref64(p, g, m, v, t, lr, b1, b2, eps, wd):
    """one step in float64; lr, b1, b2, eps, wd are the float32-rounded values the C ABI receives, 1 - b^t is formed in Python doubles"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p * (1.0 - lr * wd) - (lr / bc1) * m2 / (v2.sqrt() / math.sqrt(bc2) + eps), m2, v2


def adamw_model(p, g, m, v, t, lr, b1, b2, eps, wd, skip_last=False):
    """adamw_kernel in torch fp32: the bias corrections from fp32 pow, step = lr / bc1, rs2 = rsqrt(bc2), decay = 1 - lr wd, adamw_one's order.
    skip_last: the corruption of tests/test_steperr.py -- the last scalar of the range is not updated."""
    k = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)
    b1, b2, eps, lr, wd, t = k(b1), k(b2), k(eps), k(lr), k(wd), k(float(t))
    bc1, bc2 = 1.0 - torch.pow(b1, t), 1.0 - torch.pow(b2, t)
    step, rs2, decay = lr / bc1, torch.rsqrt(bc2), 1.0 - lr * wd
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    p2 = p * decay - step * m2 / (torch.sqrt(v2) * rs2 + eps)
    if skip_last:
        p2[-1], m2[-1], v2[-1] = p[-1], m[-1], v[-1]
    return p2, m2, v2


def adamw_moment_bounds(g, m2_64, v2_64, b1, b2):
    """Gate A.  1 - b is exact in fp32 for b in [0.5, 1) (Sterbenz).  m = fma(b1, m, (1 - b1) g): the product (1 - b1) g rounds once, the fma
    once: U |(1 - b1) g| + U |m|.  v = fma(b2, v, ((1 - b2) g) g): the product of THREE factors rounds twice, the fma once: 2 U (1 - b2) g^2 + U v."""
    g = g.double()
    return ((U * ((1.0 - b1) * g).abs() + U * m2_64.abs()) * (1 + U), (2 * U * (1.0 - b2) * g * g + U * v2_64.abs()) * (1 + 2 * U))


def adamw_gate_elements(got, ref64, model, floor_frac):
    return gate_units(got.reshape(-1, 1), ref64.reshape(-1, 1), model.reshape(-1, 1), 1, floor_frac=floor_frac)


# ------------------------------------------------------------------------------------------------ dropout / DropPath
def scale32(p):
    """1.0f / (1.0f - p) as the kernels form it (two correctly rounded fp32 operations), as a Python float"""
    one = torch.ones((), dtype=torch.float32)
    return float(one / (one - torch.tensor(p, dtype=torch.float32)))


def keep_range(i0, i1, p, seed, device):
    """bool keep decision of the flat element indices i0 .. i1 - 1 (dropmask.keep; p = 0 keeps everything)"""
    if p <= 0:
        return torch.ones(i1 - i0, dtype=torch.bool, device=device)
    return dropmask.keep(torch.arange(i0, i1, dtype=torch.int64, device=device), p, seed)


def branch_keep(r0, r1, C, rps, p, seed, pp, seed_path, device, rps_off=0):
    """[r1 - r0, C] bool: element mask on row * C + col AND the DropPath mask on row // rps.  rps_off: the corruption of
    tests/test_steperr.py (the DropPath index taken as row // (rps + 1))."""
    ke = keep_range(r0 * C, r1 * C, p, seed, device).reshape(r1 - r0, C)
    if pp <= 0:
        return ke
    rows = torch.arange(r0, r1, dtype=torch.int64, device=device)
    return ke & dropmask.keep(rows // (rps + rps_off), pp, seed_path)[:, None]


def branch_mult32(p, pp):
    """the fp32 multiplier of a kept element in branch_drop_kernel: m = (1 / (1 - pp)) * (1 / (1 - p)), one fp32 product"""
    return float(torch.tensor(scale32(pp), dtype=torch.float32) * torch.tensor(scale32(p), dtype=torch.float32))


def mask_mismatch(kernel_keep, want_keep):
    """number of elements whose keep decision differs, and the first of them (flat index in the slab)"""
    bad = kernel_keep != want_keep
    n = int(bad.sum())
    return n, (int(torch.nonzero(bad.reshape(-1))[0]) if n else -1)


def kept_fraction_ok(kept, n, p):
    """|kept / n - (1 - p)| within 4 sigma, sigma = sqrt(p (1 - p) / n)"""
    return abs(kept / n - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / n)
