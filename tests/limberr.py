"""Reference, rounding model, bounds and inputs for mbx_pose_loss_full (csrc/train_step.hip): the seven 3D losses of the reference's training
step (train.py:177-199, lib/model/loss.py:56-203), their weighted total and its gradient.  Derived the way tests/steperr.py derives pose_ref64,
pose_model and pose_loss_bounds, which supply the first three terms here.  Plain module, no fixtures: tests/test_gpu_limb_loss.py applies it to the
kernel on the GPU, tests/test_limberr.py to seeded corruptions of the restatement on the CPU.

  terms64 / full_ref64   the seven reference losses restated with torch ops, in float64 from the same fp32 bits, gradient by autograd
                         (pinned to the reference's own loss.py by tests/golden/pose_loss_full.npz)
  full_model             the kernels' formula in torch fp32, in their operation order (the rounding model of the per-frame gate)
  full_loss_bounds       first-order worst-case bounds of the eight scalars
  limb_inputs            seeded inputs, frames resampled until limb lengths and angles are well conditioned
  ambiguous_frames       frames in which the argument of a sign() is smaller than its fp32 error bound: the gradient there may differ by a whole
                         term between two correct evaluations, so they are no units of the per-frame gate"""
import math

import torch

from tests import localerr as LE
from tests import steperr as SE

U = LE.U32
NAMES = ('mpjpe', 'n_mpjpe', 'velocity', 'lv', 'lg', 'angle', 'angle_velocity', 'total')
# lib/model/loss.py:103-108 and :159-176 (lists of names: which joints a limb joins, which limbs an angle lies between)
LIMBS = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15), (15, 16))
ANGLES = ((0, 3), (0, 6), (3, 6), (0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 10), (7, 13), (8, 13), (10, 13), (7, 8), (8, 9), (10, 11), (11, 12),
          (13, 14), (14, 15))
CLAMP64 = 1.0 - 1e-7                   # the reference clamps the cosine to [-1 + 1e-7, 1 - 1e-7]
CLAMP32 = SE.f32(1.0 - 1e-7)           # ... which an fp32 tensor is compared with as 1 - 2^-23
COS_EPS = 1e-8                         # F.cosine_similarity's eps
MIN_LIMB = 0.05                        # limb_inputs: every limb longer than this fraction of the mean limb length
MAX_COS = 0.99                         # limb_inputs: every |cos| at most this
MAX_AMBIGUOUS = 1e-3                   # at most 0.1 % of the frames may be left out of the per-frame gate


def _idx(pairs, side, device):
    return torch.tensor([p[side] for p in pairs], dtype=torch.int64, device=device)


def limb_vecs(x, limbs=LIMBS):
    return x[:, :, _idx(limbs, 0, x.device)] - x[:, :, _idx(limbs, 1, x.device)]


# ------------------------------------------------------------------------------------------------ float64 restatement
def limb_lens(x, limbs=LIMBS):
    """loss.py:98-112"""
    return torch.norm(limb_vecs(x, limbs), dim=-1)


def angles(x, limbs=LIMBS, clamp=CLAMP64):
    """loss.py:148-182"""
    v = limb_vecs(x, limbs)
    cos = torch.nn.functional.cosine_similarity(v[:, :, _idx(ANGLES, 0, x.device)], v[:, :, _idx(ANGLES, 1, x.device)], dim=-1)
    return torch.acos(cos.clamp(-clamp, clamp))


def terms64(pred, gt):
    """the seven losses (train.py:178-184) of float64 pred (may require grad) and gt, as a list of 0-dim tensors"""
    from tests.test_gpu_train import _ref_losses
    T = pred.shape[1]
    zero = pred.sum() * 0
    l1, l2, l3, _ = _ref_losses(pred, gt, 0.0, 0.0)
    lp, lg = limb_lens(pred), limb_lens(gt)
    lv = torch.mean(torch.var(lp, dim=1)) if T > 1 else zero                                   # loss.py:114-123
    llg = torch.mean(torch.abs(lp - lg))                                                       # :125-131 (nn.L1Loss)
    ap, ag = angles(pred), angles(gt)
    a = torch.mean(torch.abs(ap - ag))                                                         # :184-190
    av = torch.mean(torch.abs((ap[:, 1:] - ap[:, :-1]) - (ag[:, 1:] - ag[:, :-1]))) if T > 1 else zero      # :192-203
    return [l1, l2, l3, lv, llg, a, av]


def weights7(lam6):
    return (1.0,) + tuple(float(v) for v in lam6)


def full_ref64(pred, gt, lam6, gscale):
    """(losses [8], dpred) in float64: train.py:185-191 and autograd"""
    p = pred.double().detach().requires_grad_(True)
    t = terms64(p, gt.double())
    total = sum(w * v for w, v in zip(weights7(lam6), t))
    (total * gscale).backward()
    return torch.stack([v.detach() for v in t] + [total.detach()]), p.grad


# ------------------------------------------------------------------------------------------------ the kernels in torch fp32
def _sign(x):
    return torch.sign(x)      # sign(0) = 0, as sign0 of train_step.hip


def _angle_parts(v, clamp_mask=True):
    """limb_angle of train_step.hip for every angle of v [B,T,16,3]"""
    u, w = v[:, :, _idx(ANGLES, 0, v.device)], v[:, :, _idx(ANGLES, 1, v.device)]
    eps = torch.tensor(COS_EPS, dtype=v.dtype, device=v.device)
    c = torch.tensor(CLAMP32, dtype=v.dtype, device=v.device)
    nu, nw = SE._norm3(u), SE._norm3(w)
    iu, iw = 1.0 / torch.maximum(nu, eps), 1.0 / torch.maximum(nw, eps)
    uh, wh = u * iu[..., None], w * iw[..., None]
    cs = SE._dot3(uh, wh)
    cl = torch.minimum(torch.maximum(cs, -c), c)
    inside = (cs >= -c) & (cs <= c) if clamp_mask else torch.ones_like(cs, dtype=torch.bool)
    zero = torch.zeros((), dtype=v.dtype, device=v.device)
    dth = torch.where(inside, -1.0 / torch.sqrt((1.0 - cl) * (1.0 + cl)), zero)
    return dict(th=torch.acos(cl), uh=uh, wh=wh, iu=iu, iw=iw, pu=torch.where(nu >= eps, cs, zero), pw=torch.where(nw >= eps, cs, zero), dth=dth)


def full_model(pred, gt, lam6, gscale, corrupt=None):
    """mbx_pose_loss_full in torch fp32, operation by operation: (losses [8], dpred).  The first three terms are steperr.pose_model.  The
    per-clip mean follows limb_mean_kernel's order (four phases over t, (0 + 1) + (2 + 3)); the limb and joint gradients are added in the
    order of the kernel's slot lists (angles ascending, first limb before second; limbs ascending, first joint before second).  The sums
    of the eight scalars use torch.sum (the kernel's order is a wave reduction and a column sum: covered by full_loss_bounds).
    corrupt -- tests/test_limberr.py: 'limb_table' one wrong limb-table entry, 'var_T' 1 / T instead of 1 / (T - 1), 'leak' the last frame
    of clip 0 takes an angle-velocity term from the first frame of clip 1, 'clamp_mask' a clamped cosine still passes a gradient."""
    ls, lv, llv, llg, la, lav = (float(v) for v in lam6)
    B, T, J, _ = pred.shape
    dev = pred.device
    limbs = LIMBS if corrupt != 'limb_table' else LIMBS[:5] + ((5, 7),) + LIMBS[6:]
    one = torch.ones((), dtype=torch.float32, device=dev)
    zero = one * 0
    grad = SE.pose_model(pred, gt, ls, lv, 1.0)
    inv_l, inv_a = one / float(B * T * 16), one / float(B * T * 18)
    inv_var = one / float(((T - 1) if corrupt != 'var_T' else T) * B * 16) if T > 1 else zero
    inv_av = one / float(B * (T - 1) * 18) if T > 1 else zero
    vp, vg = limb_vecs(pred, limbs), limb_vecs(gt, limbs)
    lp, lg = SE._norm3(vp), SE._norm3(vg)
    acc4 = [torch.zeros(B, 16, dtype=torch.float32, device=dev) for _ in range(4)]
    for t in range(T):
        acc4[t % 4] = acc4[t % 4] + lp[:, t]
    mean = ((acc4[0] + acc4[1]) + (acc4[2] + acc4[3])) / float(T)
    dm, dlg = lp - mean[:, None], lp - lg
    ap, ag = _angle_parts(vp, clamp_mask=corrupt != 'clamp_mask'), _angle_parts(vg)
    tp, tg = ap['th'], ag['th']
    da = tp - tg
    d = (tp[:, 1:] - tp[:, :-1]) - (tg[:, 1:] - tg[:, :-1])
    z1 = torch.zeros(B, 1, 18, dtype=torch.float32, device=dev)
    dprev, dnext = torch.cat([z1, d], 1), torch.cat([d, z1], 1)
    if corrupt == 'leak' and B > 1:
        dnext[0, T - 1] = (tp[1, 0] - tp[0, T - 1]) - (tg[1, 0] - tg[0, T - 1])
    # ---- the eight scalars
    l3 = [v.float() for v in _losses3_fp32(pred, gt)]
    s = l3 + [(dm * dm).sum() * inv_var, dlg.abs().sum() * inv_l, da.abs().sum() * inv_a, dprev.abs().sum() * inv_av]
    total = s[0] + ls * s[1] + lv * s[2] + llv * s[3] + llg * s[4] + la * s[5] + lav * s[6]
    losses = torch.stack(s + [total])
    # ---- the gradient
    if any(v != 0.0 for v in (llv, llg, la, lav)):
        gc = ((la * inv_a) * _sign(da) + (lav * inv_av) * (_sign(dprev) - _sign(dnext))) * ap['dth']
        slot_u = gc[..., None] * (ap['wh'] - ap['pu'][..., None] * ap['uh']) * ap['iu'][..., None]
        slot_w = gc[..., None] * (ap['uh'] - ap['pw'][..., None] * ap['wh']) * ap['iw'][..., None]
        il = torch.where(lp > 0, 1.0 / lp, zero)
        gl = ((llv * inv_var) * 2.0 * dm + (llg * inv_l) * _sign(dlg)) * il
        acc = gl[..., None] * vp
        for k, (i, j) in enumerate(ANGLES):
            acc[:, :, i] += slot_u[:, :, k]
            acc[:, :, j] += slot_w[:, :, k]
        e = torch.zeros_like(pred)
        for l, (a, b) in enumerate(limbs):
            e[:, :, a] += acc[:, :, l]
            e[:, :, b] -= acc[:, :, l]
        grad = grad + e
    return losses, gscale * grad


def _losses3_fp32(pred, gt):
    from tests.test_gpu_train import _ref_losses
    return _ref_losses(pred, gt, 0.0, 0.0)[:3]


# ------------------------------------------------------------------------------------------------ error bounds
def _limb_err(x64):
    """len = norm3(x[a] - x[b]) in fp32, |.| from float64.  v_c = x_a - x_b: one rounding, U |v_c|, which moves the length by at most U len;
    norm3: three fma roundings on the sum of squares (half each after the root) and the root, 2.5 U len  ->  |d len| <= 4 U len"""
    ln = limb_lens(x64)
    return ln, 4 * U * ln


def _angle_err(x64):
    """theta = acos(uh . wh) in fp32.  uh_c = u_c * (1 / len): u_c carries U, len 4 U (above), the reciprocal U, the product U: 7 U |uh_c|, and
    the same for wh_c.  cos = uh_0 wh_0 + uh_1 wh_1 + uh_2 wh_2: each product 14 U from its factors and U of its own, two additions of at most
    U A each, A = sum_c |uh_c wh_c|  ->  |d cos| <= 17 U A.  acos: |d theta| <= |d cos| / sqrt(1 - cos^2) + 4 U theta (acosf within 2 ulp =
    4 U relative, the accuracy the HIP math library documents is 1 ulp; torch's CPU acosf is within 1 ulp).  First order: meaningful where
    the cosine is inside the clamp and away from +-1, which limb_inputs ensures."""
    v = limb_vecs(x64)
    u, w = v[:, :, _idx(ANGLES, 0, x64.device)], v[:, :, _idx(ANGLES, 1, x64.device)]
    uh, wh = u / u.norm(dim=-1, keepdim=True).clamp_min(COS_EPS), w / w.norm(dim=-1, keepdim=True).clamp_min(COS_EPS)
    cos = (uh * wh).sum(-1).clamp(-CLAMP64, CLAMP64)
    th = torch.acos(cos)
    return th, 17 * U * (uh * wh).abs().sum(-1) / torch.sqrt(1.0 - cos * cos) + 4 * U * th


def _sign_args(pred, gt):
    """the three families of sign() arguments in float64 with the fp32 error bound of each: [(value, bound)] for len_p - len_g [B,T,16],
    theta_p - theta_g [B,T,18] and the angle-velocity difference [B,T-1,18] (None for T = 1).  A difference of two fp32 values adds one
    rounding, U |difference|."""
    p, g = pred.double(), gt.double()
    lp, elp = _limb_err(p)
    lg, elg = _limb_err(g)
    tp, etp = _angle_err(p)
    tg, etg = _angle_err(g)
    out = [(lp - lg, elp + elg), (tp - tg, etp + etg)]
    if p.shape[1] > 1:
        vp, vg = tp[:, 1:] - tp[:, :-1], tg[:, 1:] - tg[:, :-1]
        out.append((vp - vg, etp[:, 1:] + etp[:, :-1] + etg[:, 1:] + etg[:, :-1] + U * (vp.abs() + vg.abs())))
    else:
        out.append(None)
    return out, (lp, elp)


def full_loss_bounds(pred, gt, lam6):
    """First-order worst case for the eight scalars of mbx_pose_loss_full; float64 tensor [8].  correctly rounded +, *, /, sqrt, fma.
      mpjpe, n_mpjpe, velocity   steperr.pose_loss_bounds (the same device function, the same column sum)
      lg      |len_p - len_g|: the two lengths (4 U each, _limb_err), the difference U |d|
      lv      mean_t len: limb_mean_kernel adds ceil(T / 4) lengths per phase, two more additions and the division: (ceil(T / 4) + 3) U mean, on
              top of the lengths' own 4 U  ->  E_m = (ceil(T / 4) + 7) U mean;  dm = len - mean: 4 U len + E_m + U |dm|;  dm^2: 2 |dm| |d dm| + U dm^2
      angle   |theta_p - theta_g|: the two angles (_angle_err), the difference U |d|
      av      |(theta_p,t - theta_p,t-1) - (theta_g,t - theta_g,t-1)|: four angles, the inner differences U each, the outer U |d|
      per frame the wave sum (6 levels) and the product with 1 / n (the reciprocal, the product): 8 U x the frame's partial
      colsum  chain x U x the sum of the (non-negative) partials, per column
      total   the per-frame total is formed from the frame's seven rounded partials: sum_i lambda_i bound_i, eight more roundings on
              mag = sum_i lambda_i value_i, and the total column's own column sum: (8 + chain) U mag"""
    B, T, J, _ = pred.shape
    lam7 = weights7(lam6)
    b3 = SE.pose_loss_bounds(pred, gt, lam7[1], lam7[2])
    chain = SE.colsum_chain(B * T, True)
    args, (lp, elp) = _sign_args(pred, gt)
    vals = [v.detach() for v in terms64(pred.double(), gt.double())]
    zero = vals[0] * 0
    n_l, n_a = B * T * 16, B * T * 18
    fin = lambda err_sum, val_sum, n: ((err_sum + 8 * U * val_sum) / n + chain * U * val_sum / n) * (1 + U)
    (dl, el), (da, ea), vel = args
    b_lg = fin((el + U * dl.abs()).sum(), dl.abs().sum(), n_l)
    b_a = fin((ea + U * da.abs()).sum(), da.abs().sum(), n_a)
    if T > 1:
        m = lp.mean(1, keepdim=True)
        dm = lp - m
        e_dm = elp + (math.ceil(T / 4) + 7) * U * m + U * dm.abs()
        b_lv = fin((2 * dm.abs() * e_dm + U * dm * dm).sum(), (dm * dm).sum(), (T - 1) * B * 16)
        dv, ev = vel
        b_av = fin((ev + U * dv.abs()).sum(), dv.abs().sum(), B * (T - 1) * 18)
    else:
        b_lv = b_av = zero
    b7 = [b3[0], b3[1], b3[2], b_lv, b_lg, b_a, b_av]
    mag = sum(w * v for w, v in zip(lam7, vals))
    b_total = (sum(w * b for w, b in zip(lam7, b7)) + (8 + chain) * U * mag) * (1 + U)
    return torch.stack([b.double() for b in b7] + [b_total.double()])


def ambiguous_frames(pred, gt):
    """bool [B * T]: frames with a sign() argument below its fp32 error bound (an angle-velocity difference belongs to both of its frames)"""
    B, T = pred.shape[:2]
    args, _ = _sign_args(pred, gt)
    amb = torch.zeros(B, T, dtype=torch.bool, device=pred.device)
    for v, e in args[:2]:
        amb |= (v.abs() < e).any(-1)
    if args[2] is not None:
        a = (args[2][0].abs() < args[2][1]).any(-1)
        amb[:, 1:] |= a
        amb[:, :-1] |= a
    return amb.reshape(-1)


# ------------------------------------------------------------------------------------------------ inputs
def conditioned(pred, gt):
    """bool [frames]: every limb of pred and of gt longer than MIN_LIMB x the mean limb length of its tensor, every |cos| <= MAX_COS
    (pred, gt [B,T,17,3] or [N,1,17,3])"""
    ok = None
    for x in (pred.double(), gt.double()):
        ln = limb_lens(x)
        v = limb_vecs(x)
        cos = torch.nn.functional.cosine_similarity(v[:, :, _idx(ANGLES, 0, x.device)], v[:, :, _idx(ANGLES, 1, x.device)], dim=-1)
        k = (ln > MIN_LIMB * ln.mean()).all(-1) & (cos.abs() <= MAX_COS).all(-1)
        ok = k if ok is None else ok & k
    return ok.reshape(-1)


def limb_inputs(B, T, seed, device, noise=0.1):
    """gt skeleton-scaled on a 2^-10 grid with the root joint exactly 0, pred = gt + noise on a 2^-16 grid (both exact in fp32); frames that
    miss `conditioned` are drawn again until none does: the conditioning of acos and of 1 / len is then bounded and the rounding model is a
    fair yardstick.  The frames of a clip are independent draws."""
    g = torch.Generator().manual_seed(seed)

    def draw(n):
        gt = SE.quant(torch.randn(n, 1, 17, 3, generator=g) * 0.3, 10)
        gt[:, :, 0] = 0
        return gt + SE.quant(torch.randn(n, 1, 17, 3, generator=g) * noise, 16), gt

    pred, gt = draw(B * T)
    for _ in range(100):
        bad = ~conditioned(pred, gt)
        if not bool(bad.any()):
            return pred.reshape(B, T, 17, 3).to(device), gt.reshape(B, T, 17, 3).to(device)
        pred[bad], gt[bad] = draw(int(bad.sum()))
    raise RuntimeError('limb_inputs: resampling did not converge')


def plant_collinear(pred, gt, b, t, tilt=0.0):
    """In frame (b, t): joint 1 of pred and gt at (-0.5, 0, 0), pred = gt except joint 2 at (-1, tilt, 0).  Limbs 0 (joints 0 - 1) and 1
    (joints 1 - 2) of pred are then (0.5, 0, 0) and (0.5, -tilt, 0): with tilt = 0 exactly parallel AND exactly computed in any precision
    (length 0.5, unit vector (1, 0, 0), cosine 1), so the clamp is active whatever the rounding; with 0 < tilt <= 2^-13 the cosine is still
    beyond 1 - 1e-7 but the limbs are not parallel, so a dropped clamp mask shows as a gradient of ordinary size.  In a clip of one frame
    joint 0 of that frame then has an exactly zero gradient: pred = gt in every joint its other limbs and angles touch, the root is 0,
    and the one angle whose sign is not 0 is the clamped one."""
    gt[b, t, 1] = torch.tensor([-0.5, 0.0, 0.0], dtype=gt.dtype, device=gt.device)
    pred[b, t] = gt[b, t]
    pred[b, t, 2] = torch.tensor([-1.0, tilt, 0.0], dtype=gt.dtype, device=gt.device)
    return pred, gt


def gate_frames(got, ref64, model, B, T, keep):
    """the per-frame gate (steperr.gate_units with its floor) over the frames `keep`, and the per-clip-boundary-pair gate over the pairs
    whose two frames are both kept: ((g, m, ok, msg) frame, (g, m, ok, msg) pair or None when no pair is left)"""
    F = B * T
    f = SE.gate_units(got.reshape(F, -1)[keep], ref64.reshape(F, -1)[keep], model.reshape(F, -1)[keep], 51)
    k2 = keep.reshape(B, T)
    pk = k2[:, T - 1] & k2[torch.arange(1, B + 1, device=keep.device) % B, 0]
    if not bool(pk.any()):
        return f, None
    bp = lambda x: SE.boundary_pairs(x, B, T)[pk]
    return f, SE.gate_units(bp(got), bp(ref64), bp(model), 102)


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
LAMBDAS = (0.5, 20.0, 0.25, 0.5, 0.125, 2.0)          # scale, velocity, lv, lg, a, av: all nonzero, all exact in fp32
LAMBDAS_BASE = (0.5, 20.0, 0.0, 0.0, 0.0, 0.0)        # the four new ones at zero: "log like the reference"
GPU_SHAPES = ((1, 1), (3, 1), (2, 2), (5, 7), (3, 65), (2, 243), (64, 243))
# seeds for which the float64 reference alone leaves at most MAX_AMBIGUOUS of the frames out (tests/test_limberr.py checks every one)
SEEDS = {(1, 1): 1001, (3, 1): 3001, (2, 2): 2002, (5, 7): 5007, (3, 65): 3065, (2, 243): 2243, (64, 243): 64244}
