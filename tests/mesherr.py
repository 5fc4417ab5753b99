"""Restatements, inputs and gates for the mesh-recovery kernels (csrc/mesh.hip): mbx_rot6d_theta_fwd / _bwd (lib/model/model_mesh.py:63,74),
mbx_mesh_param_loss (lib/model/loss_mesh.py:49-68) and mbx_mesh_errors (lib/utils/utils_mesh.py:333-438).  Plain module, no fixtures:
tests/test_gpu_mesh.py applies it to the kernels on the GPU, tests/test_mesherr.py to seeded corruptions on the CPU, tools/mint_mesh.py
pins it to the reference's own code at 1e-12 (tests/golden/mesh.npz).

  rot_chain / rot_chain_grad     the 6D -> rotation matrix -> quaternion -> axis-angle chain in torch, in the dtype of its input (float64: the
                                 restatement; float32: a model of the kernel), gradient by autograd
  param_losses / param_loss_grad the three parameter losses and d(weighted sum) / d pred_theta, likewise
  mesh_errors64                  the five per-frame error rows in numpy float64, SVD as the reference takes it
  rot_inputs / theta_inputs / err_inputs   seeded inputs (not stored in the fixture)
  stat / gate32 / GATE64         the gates

Gates of the fp32 kernels: the yardstick is the reference's own code in float32 on the CPU against the same code in float64, per output
array, as  stat = max |error| / max |float64 value|  (recorded in the fixture as `.ref32`).  The device gets 4 x that: a factor 2 for
hardware sin / cos / atan2 / rsqrt paths documented at 2 ulp where the CPU's are 1 and for fma contraction in another order, a factor 2
for comparing maxima over different rounding patterns; never less than 8 fp32 ulps (arrays on which the reference happens to round
exactly).  Gate of the fp64 kernel: 1e-10 relative per frame and per aggregate, the gate of mbx_pose_errors (tests/eval_fixture.py).

The L1 loss has a kink where a predicted and a target matrix element agree: its subgradient jumps by 2 there, and float32 and float64
can land on different sides.  theta_inputs therefore keeps every such difference either exactly 0 (planted: equal rows, joints that are
zero on both sides) or above 1e-4.

One corruption of the issue's list cannot be built for quat2mat: its second normalisation divides a quaternion (cos h, sin h a / |a + 1e-8|)
whose norm differs from 1 by at most 1e-8 relative wherever sin h is not itself below 1e-8, so dropping it changes nothing a float32
gate can see, in the value or in the gradient.  'no_second_norm' drops the second normalisation of rot6d_to_rotmat instead (b2), which the
rescaled and sheared inputs do make visible."""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -23
FLOOR = 8 * EPS32         # 8 fp32 ulps, relative to the largest float64 value of the array
GATE64 = 1e-10
H36M_17_TO_14 = (1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15, 16)
ERR_ROWS = ('mpve', 'mpjpe_17j', 'mpjpe', 'pa_mpjpe_17j', 'pa_mpjpe')      # rows of mbx_mesh_errors; 'mpjpe' / 'pa_mpjpe' are the 14-joint ones

CORRUPTIONS = ('untransposed', 'wrong_case', 'no_eps', 'no_second_norm', 'mse_for_l1', 'norm72', 'subset_off_by_one', 'no_reflection_fix',
               'mpve_no_root')
ROT_CORRUPTIONS = ('untransposed', 'wrong_case', 'no_second_norm')
LOSS_CORRUPTIONS = ('no_eps', 'mse_for_l1', 'norm72')
ERR_CORRUPTIONS = ('subset_off_by_one', 'no_reflection_fix', 'mpve_no_root')


# ------------------------------------------------------------------------------------------------ rotation chain
def rot_cases(m, wrong=False):
    """the mask case 0 .. 3 of rotation_matrix_to_quaternion for m = R^T [M,3,3]; wrong: the third mask compares m00 < m11 (sign lost)"""
    d2 = m[:, 2, 2] < 1e-6
    d0_d1 = m[:, 0, 0] > m[:, 1, 1]
    d0_nd1 = m[:, 0, 0] < (m[:, 1, 1] if wrong else -m[:, 1, 1])
    return torch.where(d2, torch.where(d0_d1, 0, 1), torch.where(d0_nd1, 2, 3))


def rot_chain(x6, corrupt=None):
    """(rotmat [M,3,3], aa [M,3]) of x6 [M,6] in x6's dtype.  corrupt: 'untransposed' the quaternion step reads R instead of R^T,
    'wrong_case' the third mask loses its minus sign (m00 < m11), so joints of case 3 are divided by case 2's small trace term: the same
    rotation in exact arithmetic, ill-conditioned in fp32 -- what the four cases exist to avoid; 'no_second_norm' b2 is left unnormalised."""
    assert corrupt is None or corrupt in ROT_CORRUPTIONS
    x = x6.reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = a1 / a1.norm(dim=1, keepdim=True).clamp_min(1e-6)
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = u if corrupt == 'no_second_norm' else u / u.norm(dim=1, keepdim=True).clamp_min(1e-6)
    b3 = torch.linalg.cross(b1, b2, dim=1)
    R = torch.stack([b1, b2, b3], dim=-1)
    m = R if corrupt == 'untransposed' else R.transpose(1, 2)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[:, i, j] for i in range(3) for j in range(3)]
    t = [1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22, 1 + m00 + m11 + m22]
    qs = [torch.stack([m12 - m21, t[0], m01 + m10, m20 + m02], -1), torch.stack([m20 - m02, m01 + m10, t[1], m12 + m21], -1),
          torch.stack([m01 - m10, m20 + m02, m12 + m21, t[2]], -1), torch.stack([t[3], m12 - m21, m20 - m02, m01 - m10], -1)]
    case = rot_cases(m.detach(), wrong=corrupt == 'wrong_case')
    qsel = sum(torch.where((case == c)[:, None], qs[c], torch.zeros_like(qs[c])) for c in range(4))
    tsel = sum(torch.where(case == c, t[c], torch.zeros_like(t[c])) for c in range(4))
    q = qsel / torch.sqrt(tsel)[:, None] * 0.5
    s2 = (q[:, 1:] ** 2).sum(1)
    pos = s2 > 0
    s = torch.sqrt(torch.where(pos, s2, torch.ones_like(s2)))          # sin^2 == 0: k = 2 takes over; its gradient is the continuous extension
    c = q[:, 0]
    tt = 2.0 * torch.where(c < 0, torch.atan2(-s, -c), torch.atan2(s, c))
    k = torch.where(pos, tt / s, torch.full_like(s, 2.0))
    aa = q[:, 1:] * k[:, None]
    aa = torch.where(torch.isnan(aa), torch.zeros_like(aa), aa)
    return R, aa


def rot_chain_grad(x6, drot, daa, dtype, corrupt=None):
    """(rotmat, aa, dx6) in `dtype` from the fp32 bits of x6 and the cotangents"""
    x = x6.detach().clone().to(dtype).requires_grad_(True)
    R, aa = rot_chain(x, corrupt)
    ((R.reshape(-1, 9) * drot.to(dtype)).sum() + (aa * daa.to(dtype)).sum()).backward()
    return R.detach().reshape(-1, 9), aa.detach(), x.grad


def axis_angle_matrix64(axis, angle):
    """Rodrigues' formula in float64: axis [M,3] unit, angle [M]"""
    K = torch.zeros(len(angle), 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    return torch.eye(3, dtype=torch.float64) + torch.sin(angle)[:, None, None] * K + (1 - torch.cos(angle))[:, None, None] * (K @ K)


def rot_inputs(M, seed):
    """x6 [M,6] fp32 and cotangents drot [M,9], daa [M,3] fp32.  Rotations by an angle uniform in [0.05, pi - 0.05] about a uniform axis; the
    first column is rescaled by [0.5, 2], the second rescaled by [0.5, 2] and sheared along the first by [-0.5, 0.5], so that both
    normalisations and the projection do work.  With M >= 72 every quaternion case occurs (asserted)."""
    g = torch.Generator().manual_seed(seed)
    axis = torch.randn(M, 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    angle = 0.05 + (math.pi - 0.1) * torch.rand(M, generator=g, dtype=torch.float64)
    R = axis_angle_matrix64(axis, angle)
    sc = 0.5 + 1.5 * torch.rand(M, 2, generator=g, dtype=torch.float64)
    sh = torch.rand(M, generator=g, dtype=torch.float64) - 0.5
    a1 = R[:, :, 0] * sc[:, :1]
    a2 = R[:, :, 1] * sc[:, 1:] + sh[:, None] * R[:, :, 0]
    x6 = torch.stack([a1, a2], dim=-1).reshape(M, 6).float()
    drot = torch.randn(M, 9, generator=g).float()
    daa = torch.randn(M, 3, generator=g).float()
    if M >= 72:
        counts = torch.bincount(rot_cases(rot_chain(x6.double())[0].transpose(1, 2)), minlength=4)
        assert int(counts.min()) >= 1, f'rot_inputs({M}, {seed}): quaternion cases {counts.tolist()}'
    return x6, drot, daa


ROT_M = (1, 72, 264, 24 * 2048)


def rot_seed(M):
    return 4100 + M % 997


def fixture_rows(n, width, limit=16384):
    """rows of an [n, width] gradient the fixture keeps: all, or the first and last 32 of an array of more than `limit` elements"""
    return np.arange(n) if n * width <= limit else np.concatenate([np.arange(32), np.arange(n - 32, n)])


# ------------------------------------------------------------------------------------------------ parameter losses
def rodrigues(a, corrupt=None):
    """batch_rodrigues (utils_mesh.py:8-51) of a [N,3] -> [N,9].  corrupt 'no_eps': the + 1e-8 inside the norm is dropped."""
    n = (a + (0.0 if corrupt == 'no_eps' else 1e-8)).norm(dim=1, keepdim=True)
    h = n * 0.5
    q = torch.cat([torch.cos(h), torch.sin(h) * (a / n)], dim=1)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz, 2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], dim=1)


def param_losses(pred, gt, loss_type, corrupt=None):
    """(loss_pose, loss_shape, loss_norm) of pred, gt [F,82] in their dtype.  loss_type 0 MSE, 1 L1.  corrupt: 'no_eps' (rodrigues),
    'mse_for_l1' the squared difference whatever loss_type says, 'norm72' loss_norm over the pose part only."""
    assert corrupt is None or corrupt in LOSS_CORRUPTIONS
    crit = (lambda d: (d * d).mean()) if loss_type == 0 or corrupt == 'mse_for_l1' else (lambda d: d.abs().mean())
    Rp = rodrigues(pred[:, :72].reshape(-1, 3), corrupt)
    Rg = rodrigues(gt[:, :72].reshape(-1, 3), corrupt)
    return crit(Rp - Rg), crit(pred[:, 72:] - gt[:, 72:]), (pred[:, :72] if corrupt == 'norm72' else pred).norm(dim=-1).mean()


def param_loss_grad(pred, gt, loss_type, lambdas3, dtype, corrupt=None):
    """(losses [3], dtheta [F,82]) in `dtype`; dtheta = d (sum lambda_i loss_i) / d pred"""
    p = pred.detach().clone().to(dtype).requires_grad_(True)
    ls = param_losses(p, gt.to(dtype), loss_type, corrupt)
    sum(float(np.float32(l)) * v for l, v in zip(lambdas3, ls)).backward()
    return torch.stack([v.detach() for v in ls]), p.grad


LOSS_F = (1, 3, 33, 2048)
LAMBDAS3 = (1.0, 0.5, 0.25)       # lambda_pose, lambda_shape, lambda_norm of the fixture: all three terms in play, exact in fp32
KINK = 1e-4


def loss_seed(F):
    return 5200 + F % 991


def theta_inputs(F, seed):
    """pred, gt [F,82] fp32.  Pose joints are axis-angle vectors of length up to about 2.5; about one joint in eight is exactly zero on
    the target side and one in sixteen on the prediction's (SMPL targets are full of zero joints: without the + 1e-8 those are 0 / 0).
    With F >= 3, target row 1 equals the prediction's.  Every difference of two rotation-matrix elements is exactly 0 or above KINK."""
    g = torch.Generator().manual_seed(seed)

    def joints(n):
        return (0.8 * torch.randn(n, 3, generator=g)).float()
    pp, pg = joints(F * 24), joints(F * 24)
    pg[torch.rand(F * 24, generator=g) < 0.125] = 0.0
    pp[torch.rand(F * 24, generator=g) < 0.0625] = 0.0
    for _ in range(64):
        d = (rodrigues(pp.double()) - rodrigues(pg.double())).abs()
        bad = ((d > 0) & (d < KINK)).any(1)
        if not bool(bad.any()):
            break
        pp[bad] = joints(int(bad.sum()))
    else:
        raise AssertionError('theta_inputs: could not move every difference off the kink')
    pred = torch.cat([pp.reshape(F, 72), torch.randn(F, 10, generator=g).float()], 1)
    gt = torch.cat([pg.reshape(F, 72), torch.randn(F, 10, generator=g).float()], 1)
    if F >= 3:
        gt[1] = pred[1]
    return pred.contiguous(), gt.contiguous()


# ------------------------------------------------------------------------------------------------ mesh errors
def rigid_align64(A, B, corrupt=None):
    """rigid_align (utils_mesh.py:333-355) of A onto B, [n,3] float64.  corrupt 'no_reflection_fix': the det < 0 branch is left out."""
    n = A.shape[0]
    ca, cb = A.mean(0), B.mean(0)
    H = (A - ca).T @ (B - cb) / n
    U, s, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0 and corrupt != 'no_reflection_fix':
        s = s.copy()
        Vt = Vt.copy()
        s[-1] = -s[-1]
        Vt[2] = -Vt[2]
        R = Vt.T @ U.T
    with np.errstate(divide='ignore', invalid='ignore'):
        c = 1 / np.var(A, axis=0).sum() * np.sum(s)
        return (c * R @ A.T).T + (cb - c * R @ ca)


def mesh_errors64(vp, vg, kp, kg, corrupt=None):
    """err [5,F] float64, rows ERR_ROWS, of verts [F,V,3] (or None) and joints [F,17,3] (numpy, any float dtype).  corrupt:
    'subset_off_by_one' the 14 joints are (0 .. 5, 7, 9 .. 15), 'no_reflection_fix' (rigid_align64), 'mpve_no_root' raw vertices."""
    assert corrupt is None or corrupt in ERR_CORRUPTIONS
    kp, kg = np.asarray(kp, np.float64), np.asarray(kg, np.float64)
    F = kp.shape[0]
    err = np.full((5, F), np.nan)
    if vp is not None:
        a, b = np.asarray(vp, np.float64), np.asarray(vg, np.float64)
        if corrupt != 'mpve_no_root':
            a, b = a - kp[:, :1], b - kg[:, :1]
        err[0] = np.sqrt(((a - b) ** 2).sum(-1)).mean(-1)
    p17, g17 = kp - kp[:, :1], kg - kg[:, :1]
    idx = [j - 1 for j in H36M_17_TO_14] if corrupt == 'subset_off_by_one' else list(H36M_17_TO_14)
    p14, g14 = p17[:, idx], g17[:, idx]
    err[1] = np.sqrt(((p17 - g17) ** 2).sum(-1)).mean(-1)
    err[2] = np.sqrt(((p14 - g14) ** 2).sum(-1)).mean(-1)
    for f in range(F):
        err[3, f] = np.sqrt(((rigid_align64(p17[f], g17[f], corrupt) - g17[f]) ** 2).sum(-1)).mean()
        err[4, f] = np.sqrt(((rigid_align64(p14[f], g14[f], corrupt) - g14[f]) ** 2).sum(-1)).mean()
    return err


def aggregate(err):
    """evaluate_mesh's dict from the per-frame rows"""
    return {k: float(np.mean(err[i])) for i, k in enumerate(ERR_ROWS)}


ERR_CASES = ((1, 6890), (5, 6890), (37, 6890), (3, 7))       # (F, V)
PLANTED = {(37, 6890): (0, 1, 2), (3, 7): (0, 1, 2)}         # frames: prediction == target, mirrored prediction, zero-extent prediction


def err_seed(case):
    return 6300 + 11 * case[0] + case[1] % 977


def err_inputs(F, V, seed):
    """verts_p, verts_g [F,V,3], kp_p, kp_g [F,17,3] fp32, millimetre-sized: the prediction is the target turned by up to 0.3 rad, scaled
    by [0.9, 1.1], shifted and perturbed by 20 mm noise.  Cases in PLANTED have frame 0 equal to its target, frame 1 mirrored in x
    (the best orthogonal map is a reflection: rigid_align's det < 0 branch) and frame 2 with all predicted joints in one point."""
    g = torch.Generator().manual_seed(seed)
    vg = 300.0 * torch.randn(F, V, 3, generator=g, dtype=torch.float64)
    kg = 300.0 * torch.randn(F, 17, 3, generator=g, dtype=torch.float64)
    axis = torch.randn(F, 3, generator=g, dtype=torch.float64)
    R = axis_angle_matrix64(axis / axis.norm(dim=1, keepdim=True), 0.3 * torch.rand(F, generator=g, dtype=torch.float64))
    sc = (0.9 + 0.2 * torch.rand(F, 1, 1, generator=g, dtype=torch.float64))
    t = 100.0 * torch.randn(F, 1, 3, generator=g, dtype=torch.float64)
    vp = sc * (vg @ R.transpose(1, 2)) + t + 20.0 * torch.randn(F, V, 3, generator=g, dtype=torch.float64)
    kp = sc * (kg @ R.transpose(1, 2)) + t + 20.0 * torch.randn(F, 17, 3, generator=g, dtype=torch.float64)
    if (F, V) in PLANTED:
        same, mirror, flat = PLANTED[(F, V)]
        vp[same], kp[same] = vg[same], kg[same]
        kp[mirror] = kg[mirror] * torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64) + 5.0 * torch.randn(17, 3, generator=g, dtype=torch.float64)
        kp[flat] = kp[flat, :1]
    return vp.float().contiguous(), vg.float().contiguous(), kp.float().contiguous(), kg.float().contiguous()


# ------------------------------------------------------------------------------------------------ gates
def stat(got, ref64):
    """max |got - ref| / max |ref| (an array that is exactly zero in float64 must be matched exactly)"""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, np.float64)
    ref = np.asarray(ref64.detach().cpu() if torch.is_tensor(ref64) else ref64, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return math.inf
    err, top = float(np.max(np.abs(got - ref))) if got.size else 0.0, float(np.max(np.abs(ref))) if ref.size else 0.0
    return err / top if top > 0 else (0.0 if err == 0 else math.inf)


def gate32(ref32_stat):
    return max(4.0 * float(ref32_stat), FLOOR)


def err_ratio(got, ref):
    """worst |got - ref| / (GATE64 |ref|) over the entries; NaN must sit exactly where the reference's is, and an exact 0 (a prediction
    equal to its target) is matched to GATE64 of a millimetre"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return math.inf
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - ref[ok]) / (GATE64 * np.maximum(np.abs(ref[ok]), 1.0))))


# ------------------------------------------------------------------------------------------------ the fp64 kernel's own algebra
def _align_model(A, B, corrupt=None):
    """mean |aligned_j - B_j| the way mbx_mesh_errors forms it (csrc/pose_solve.h): right vectors from the eigen-decomposition of H^T H
    (the kernel: 8 Jacobi sweeps; tests/procerr.py models those), u_i = H v_i / s_i for the two leading ones, with the kernel's guard for a
    rank-one H (procerr.rank_one_guard), the third pair as cross products, the signed third singular value u2 . H v2.
    A = prediction, B = target, [n,3] float64."""
    with np.errstate(divide='ignore', invalid='ignore'):
        Y0, X0 = A - A.mean(0), B - B.mean(0)
        nx, ny = (X0 ** 2).sum(), (Y0 ** 2).sum()
        H = X0.T @ Y0 / ny
        if not np.isfinite(H).all():
            return np.nan
        if nx == 0.0:
            return float(np.sqrt((X0 ** 2).sum(-1)).mean())
        w, V = np.linalg.eigh(H.T @ H)
        v0, v1 = V[:, 2], V[:, 1]
        v2 = np.cross(v0, v1)
        u0 = H @ v0
        s0 = np.linalg.norm(u0)
        u0 = u0 / s0
        u1 = H @ v1
        u1 = u1 - (u0 @ u1) * u0
        from tests import procerr                # (procerr reads rigid_align64 from this module)
        u1, s1 = procerr.rank_one_guard(u0, u1, s0, np.linalg.norm(u1))
        u2 = np.cross(u0, u1)
        s2 = u2 @ (H @ v2)
        if corrupt == 'no_reflection_fix' and s2 < 0:
            s2, v2 = -s2, -v2
        R = np.outer(v0, u0) + np.outer(v1, u1) + np.outer(v2, u2)
        return float(np.sqrt(((Y0 @ ((s0 + s1 + s2) * R) - X0) ** 2).sum(-1)).mean())


def mesh_errors_model(vp, vg, kp, kg, corrupt=None):
    """mbx_mesh_errors in numpy float64 with the kernel's decomposition; the three plain rows are mesh_errors64's"""
    err = mesh_errors64(vp, vg, kp, kg, corrupt if corrupt != 'no_reflection_fix' else None)
    kp, kg = np.asarray(kp, np.float64), np.asarray(kg, np.float64)
    p17, g17 = kp - kp[:, :1], kg - kg[:, :1]
    idx = [j - 1 for j in H36M_17_TO_14] if corrupt == 'subset_off_by_one' else list(H36M_17_TO_14)
    for f in range(kp.shape[0]):
        err[3, f] = _align_model(p17[f], g17[f], corrupt)
        err[4, f] = _align_model(p17[f][idx], g17[f][idx], corrupt)
    return err


# ------------------------------------------------------------------------------------------------ a kernel provider in torch (CPU tests)
class TorchOps:
    """The mesh entries of the kernel provider (and pose_loss_full) on CPU tensors, from the float64 restatements: same argument lists as
    HipOps, results rounded to the outputs' dtype.  `calls` counts the entries used."""

    def __init__(self):
        self.calls = {}

    def _count(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def rot6d_theta_fwd(self, x6, rotmat, aa):
        self._count('rot6d_theta_fwd')
        R, a = rot_chain(x6.double())
        if rotmat is not None:
            rotmat.copy_(R.reshape(rotmat.shape))
        if aa is not None:
            aa.copy_(a)

    def rot6d_theta_bwd(self, x6, drotmat, daa, dx6):
        self._count('rot6d_theta_bwd')
        M = x6.shape[0]
        dr = torch.zeros(M, 9, dtype=torch.float64) if drotmat is None else drotmat.double().reshape(M, 9)
        da = torch.zeros(M, 3, dtype=torch.float64) if daa is None else daa.double()
        with torch.enable_grad():             # (called from inside a backward)
            dx6.copy_(rot_chain_grad(x6, dr, da, torch.float64)[2])

    def mesh_param_loss(self, pred_theta, gt_theta, loss_type, lambdas3, losses, dtheta, grad_scale=1.0):
        self._count('mesh_param_loss')
        with torch.enable_grad():
            ls, d = param_loss_grad(pred_theta, gt_theta, int(loss_type), lambdas3, torch.float64)
        losses[:3] = ls.float()
        losses[3] = float(sum(float(l) * float(v) for l, v in zip(lambdas3, ls)))
        if dtheta is not None:
            dtheta.copy_(grad_scale * (d if d is not None else torch.zeros_like(pred_theta, dtype=torch.float64)))

    def mesh_errors(self, verts_p, verts_g, kp_p, kp_g, err):
        self._count('mesh_errors')
        err.copy_(torch.from_numpy(mesh_errors64(None if verts_p is None else verts_p.numpy(), None if verts_g is None else verts_g.numpy(),
                                                 kp_p.numpy(), kp_g.numpy())))

    def pose_loss_full(self, pred, gt, lambdas6, losses, dpred, grad_scale=1.0):
        self._count('pose_loss_full')
        from tests import limberr
        with torch.enable_grad():
            ls, d = limberr.full_ref64(pred, gt, lambdas6, grad_scale)
        losses.copy_(ls)
        if dpred is not None:
            dpred.copy_(d)


# ------------------------------------------------------------------------------------------------ stand-ins for the end-to-end tests
class StandInSMPL(torch.nn.Module):
    """A fixed differentiable map from (betas [F,10], 24 rotation matrices) to V vertices, called as the reference calls its SMPL layer:
    every vertex is a blend (fixed weights over the 24 joints) of the rotated shaped template.  Not a body model; it has SMPL's call
    signature, returns `.vertices` in metres and makes every rotation matrix and every beta matter."""

    def __init__(self, V=64, seed=7):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer('template', 0.3 * torch.randn(V, 3, generator=g))
        self.register_buffer('shapedirs', 0.02 * torch.randn(V, 3, 10, generator=g))
        self.register_buffer('weights', torch.softmax(2.0 * torch.randn(V, 24, generator=g), dim=1))
        self.J_regressor_h36m = torch.softmax(torch.randn(17, V, generator=g), dim=1)

    def forward(self, betas, body_pose, global_orient, pose2rot=False):
        import types
        assert not pose2rot
        R = torch.cat([global_orient, body_pose], dim=1)                               # [F,24,3,3]
        shaped = self.template[None] + torch.einsum('vck,fk->fvc', self.shapedirs, betas)
        verts = torch.einsum('vj,fjcd,fvd->fvc', self.weights, R, shaped)
        return types.SimpleNamespace(vertices=verts)


def mean_params(seed=8):
    """(init_pose [1,144], init_shape [1,10]): 6D columns of moderate rotations, small betas"""
    g = torch.Generator().manual_seed(seed)
    axis = torch.randn(24, 3, generator=g, dtype=torch.float64)
    R = axis_angle_matrix64(axis / axis.norm(dim=1, keepdim=True), 0.2 + 1.5 * torch.rand(24, generator=g, dtype=torch.float64))
    return torch.stack([R[:, :, 0], R[:, :, 1]], dim=-1).reshape(1, 144).float(), (0.3 * torch.randn(1, 10, generator=g)).float()


def plain_head_forward(head, feat):
    """SMPLRegressor.forward with the rotation chain written in plain torch operations (rot_chain), in the dtype of `feat`"""
    N, T = feat.shape[:2]
    NT = N * T
    feat = feat.reshape(N, T, -1)
    fp = head.relu1(head.bn1(head.fc1(head.dropout(feat.reshape(NT, -1)))))
    fs = head.relu2(head.bn2(head.fc2(head.dropout(head.pool2(feat.permute(0, 2, 1)).reshape(N, -1)))))
    pose = head.head_pose(fp) + head.init_pose.expand(NT, -1)
    shape = (head.head_shape(fs) + head.init_shape.expand(N, -1)).expand(T, N, -1).permute(1, 0, 2).reshape(NT, -1)
    R, aa = rot_chain(pose.reshape(-1, 6))
    R = R.reshape(NT, 24, 3, 3)
    verts = head.smpl(betas=shape, body_pose=R[:, 1:], global_orient=R[:, 0].unsqueeze(1), pose2rot=False).vertices * 1000.0
    kp = torch.matmul(head.J_regressor.to(verts)[None].expand(NT, -1, -1), verts)
    return [{'theta': torch.cat([aa.reshape(NT, 72), shape], dim=1).reshape(N, T, -1), 'verts': verts.reshape(N, T, -1, 3),
             'kp_3d': kp.reshape(N, T, -1, 3)}]


class Lambdas:
    """the ten weights as train_mesh.py reads them from its config (values: configs/mesh/MB_train_pw3d.yaml's, with lambda_3d off 1 and the
    terms the config switches off switched on, so that every term and the lambda_3d handling are in play)"""
    lambda_3d, lambda_scale, lambda_3dv, lambda_lv, lambda_lg, lambda_a, lambda_av = 0.5, 0.25, 10.0, 0.125, 0.5, 1.0, 2.0
    lambda_shape, lambda_pose, lambda_norm = 0.5, 1000.0, 20.0


def mesh_targets(N, T, V, seed):
    """a target dict: theta [N,T,82], kp_3d [N,T,17,3], verts [N,T,V,3] (millimetres)"""
    g = torch.Generator().manual_seed(seed)
    theta = torch.cat([0.5 * torch.randn(N, T, 72, generator=g), torch.randn(N, T, 10, generator=g)], -1)
    return {'theta': theta, 'kp_3d': 200.0 * torch.randn(N, T, 17, 3, generator=g), 'verts': 200.0 * torch.randn(N, T, V, 3, generator=g)}
