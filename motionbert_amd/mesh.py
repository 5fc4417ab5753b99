"""Mesh recovery on the device (reference `train_mesh.py`, `lib/model/model_mesh.py`, `lib/model/loss_mesh.py`, `lib/utils/utils_mesh.py`;
configs `configs/mesh/*.yaml`).  The SMPL layer is injected as in the reference: the project's own `motionbert_amd.smpl.SMPLLayer` (fused device
skinning, built from the user's SMPL arrays) or any module with the reference's call signature (`smplx`); everything around it is here:

    rot6d_to_rotmat_theta(x6)       the head's rotation chain 6D -> rotation matrix -> quaternion -> axis-angle as ONE kernel forward and ONE
                                    backward (`mbx_rot6d_theta_fwd / _bwd`; about 120 small torch kernels each way in the reference).
    SMPLRegressor / MeshRegressor   model_mesh.py:9-101 with the reference's parameter and buffer names; `smpl`, `init_pose`, `init_shape` and
                                    `J_regressor` are injected.
    MeshLoss(loss_type, lambdas)    loss_mesh.py:7-68: the reference's dict of ten losses as 0-dim device tensors; the seven joint terms from
                                    one `mbx_pose_loss_full`, the three parameter terms from one `mbx_mesh_param_loss`.
    MeshStep(model, ...)            the optimizer step of train_mesh.py:165-203 (a `train.TwoGroupStep`), no host synchronisation; the ten losses, the total and
                                    the step's MPJPE / MPVE stay in a device log tensor.
    MeshEvaluator()                 `update(output, batch_gt)` per test batch (`mbx_mesh_errors` into device buffers), `finish()` returns
                                    `evaluate_mesh`'s dict and is the only host synchronisation: no vertex ever goes to the host.
    compute_error / compute_error_frames   the reference's signatures (utils_mesh.py:357-393) on the same kernel.
    flip_thetas_batch(thetas)       utils_mesh.py:486-513 on a tensor, bit for bit.
    mesh_targets(smpl, pose, shape) the ground-truth stage of `MotionSMPL.__getitem__` (lib/data/dataset_mesh.py:63-97) for a batch of clips on the
                                    device, one `mbx_mesh_gt`: the clip flip of the 2D input and of theta, SMPL from axis-angle, the H36M joints,
                                    both root subtractions.  `motionbert_amd.data.PackedMesh` feeds it from packed arrays.
    flip_average(model, smpl, x)    the flip evaluation of train_mesh.py:83-108: the mean of the model's output and the flipped-back output of
                                    the flipped input, for `MeshEvaluator.update`.

Not here: the 49-joint map of `utils_smpl.SMPL`, rendering, a DDP variant of the step.  `infer_wild_mesh.py` (with its scale fit and camera
placement) is `motionbert_amd.wild.infer_mesh`.

There is no CPU path: without an injected kernel provider (`ops=`), tensors that are not on a ROCm device raise.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import hip_ops
from .smpl import _MOVE, SMPLLayer, rodrigues
from .train import TwoGroupStep

LOSS_KEYS = ('loss_3d_pos', 'loss_3d_scale', 'loss_3d_velocity', 'loss_lv', 'loss_lg', 'loss_a', 'loss_av', 'loss_shape', 'loss_pose', 'loss_norm')
LAMBDA_NAMES = ('lambda_3d', 'lambda_scale', 'lambda_3dv', 'lambda_lv', 'lambda_lg', 'lambda_a', 'lambda_av', 'lambda_shape', 'lambda_pose',
                'lambda_norm')      # train_mesh.py:180-189, in the order of LOSS_KEYS
ERROR_KEYS = ('mpve', 'mpjpe_17j', 'mpjpe', 'pa_mpjpe_17j', 'pa_mpjpe')      # rows of mbx_mesh_errors; 'mpjpe' / 'pa_mpjpe' use the 14 joints
LOSS_TYPES = {'MSE': 0, 'L1': 1}


# ---------------------------------------------------------------------------------------------------------------- rotation chain
class _Rot6dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ops, x6):
        x = x6.detach().contiguous().float()
        M = x.shape[0]
        rotmat = torch.empty(M, 9, dtype=torch.float32, device=x.device)
        aa = torch.empty(M, 3, dtype=torch.float32, device=x.device)
        if M:
            ops.rot6d_theta_fwd(x, rotmat, aa)
        ctx.ops, ctx.x = ops, x
        ctx.set_materialize_grads(False)
        return rotmat.view(M, 3, 3), aa

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, drotmat, daa):
        x = ctx.x
        dx = torch.zeros_like(x)
        if x.shape[0] and (drotmat is not None or daa is not None):
            dr = None if drotmat is None else drotmat.contiguous().float().reshape(-1, 9)
            da = None if daa is None else daa.contiguous().float()
            ctx.ops.rot6d_theta_bwd(x, dr, da, dx)
        return None, dx


def rot6d_to_rotmat_theta(x6: torch.Tensor, ops=None):
    """`(rotmat [M,3,3], aa [M,3])` of x6 [M,6] (or [..., 6k], flattened as the reference's `view(-1, 3, 2)` flattens it):
    `rot6d_to_rotmat(x6)` and `rotation_matrix_to_angle_axis(rotmat)` of utils_mesh.py, differentiable with respect to x6 through
    either output.  The gradient is autograd's of the reference, except at an exact identity (sin^2 == 0), where the reference gives
    NaN and this the continuous extension `d aa = 2 d q_xyz` (include/mbx.h)."""
    if x6.numel() % 6 != 0:
        raise ValueError(f'rot6d_to_rotmat_theta needs a multiple of 6 elements, got {tuple(x6.shape)}')
    if not x6.dtype.is_floating_point:
        raise ValueError(f'rot6d_to_rotmat_theta needs a floating-point tensor, got {x6.dtype}')
    ops = hip_ops.provider(ops, 'motionbert_amd.mesh.rot6d_to_rotmat_theta', x6)
    return _Rot6dFn.apply(ops, x6.reshape(-1, 6))


# ---------------------------------------------------------------------------------------------------------------- model
class SMPLRegressor(nn.Module):
    """model_mesh.py:9-80 with the SMPL layer injected.  `smpl`: any nn.Module called as `smpl(betas=, body_pose=, global_orient=,
    pose2rot=False)` that returns an object with `.vertices` [F,V,3] in metres; `init_pose` [1,144] / `init_shape` [1,10]: the mean
    parameters (`smpl_mean_params`); `J_regressor` [17,V]: `smpl.J_regressor_h36m`.  Parameter and buffer names are the reference's
    (`fc1 / fc2 / bn1 / bn2 / head_pose / head_shape`, `init_pose`, `init_shape`, `smpl.*`): with the reference's `SMPL` injected its
    checkpoints load with `strict=True`.  `J_regressor` is a plain attribute as in the reference (it is `smpl`'s buffer there).
    The Linear / BatchNorm layers are torch modules; the rotation chain is `rot6d_to_rotmat_theta`."""

    def __init__(self, smpl, init_pose, init_shape, J_regressor, dim_rep=512, num_joints=17, hidden_dim=2048, dropout_ratio=0., ops=None):
        super().__init__()
        param_pose_dim = 24 * 6
        self.dropout = nn.Dropout(p=dropout_ratio)
        self.fc1 = nn.Linear(num_joints * dim_rep, hidden_dim)
        self.pool2 = nn.AdaptiveAvgPool2d((None, 1))
        self.fc2 = nn.Linear(num_joints * dim_rep, hidden_dim)
        self.bn1 = nn.BatchNorm1d(hidden_dim, momentum=0.1)
        self.bn2 = nn.BatchNorm1d(hidden_dim, momentum=0.1)
        self.relu1 = nn.ReLU(inplace=True)
        self.relu2 = nn.ReLU(inplace=True)
        self.head_pose = nn.Linear(hidden_dim, param_pose_dim)
        self.head_shape = nn.Linear(hidden_dim, 10)
        nn.init.xavier_uniform_(self.head_pose.weight, gain=0.01)
        nn.init.xavier_uniform_(self.head_shape.weight, gain=0.01)
        self.smpl = smpl
        init_pose, init_shape = torch.as_tensor(init_pose), torch.as_tensor(init_shape)
        if init_pose.numel() != param_pose_dim or init_shape.numel() != 10:
            raise ValueError(f'init_pose needs 144 elements and init_shape 10, got {tuple(init_pose.shape)} / {tuple(init_shape.shape)}')
        self.register_buffer('init_pose', init_pose.reshape(1, param_pose_dim).clone())
        self.register_buffer('init_shape', init_shape.reshape(1, 10).float().clone())
        J_regressor = torch.as_tensor(J_regressor)
        if J_regressor.dim() != 2 or J_regressor.shape[0] != 17:
            raise ValueError(f'J_regressor needs to be [17, V], got {tuple(J_regressor.shape)}')
        self.J_regressor = J_regressor
        self.ops = ops

    def _regressor(self, device, dtype):
        if self.J_regressor.device != device or self.J_regressor.dtype != dtype:
            self.J_regressor = self.J_regressor.to(device=device, dtype=dtype)    # once, not per forward as the reference moves it: a host copy per step
        return self.J_regressor

    def forward_params(self, feat):
        """The head without SMPL: feat [N,T,J,C] -> `(rotmat [NT,24,3,3], shape [NT,10], theta [NT,82])`, the parameters `forward` hands to
        the SMPL layer and its `theta` (24 axis-angle joints | shape).  `wild.infer_mesh` feeds them to one `mbx_wild_mesh` launch."""
        N, T, J, C = feat.shape
        NT = N * T
        feat = feat.reshape(N, T, -1)
        feat_pose = self.relu1(self.bn1(self.fc1(self.dropout(feat.reshape(NT, -1)))))          # (NT, hidden)
        feat_shape = self.pool2(feat.permute(0, 2, 1)).reshape(N, -1)                           # mean over T: (N, J*C)
        feat_shape = self.relu2(self.bn2(self.fc2(self.dropout(feat_shape))))                   # (N, hidden)
        pred_pose = self.head_pose(feat_pose) + self.init_pose.expand(NT, -1)
        pred_shape = self.head_shape(feat_shape) + self.init_shape.expand(N, -1)
        pred_shape = pred_shape.expand(T, N, -1).permute(1, 0, 2).reshape(NT, -1)
        rotmat, aa = rot6d_to_rotmat_theta(pred_pose.float(), ops=self.ops)
        rotmat, aa = rotmat.to(pred_pose.dtype), aa.to(pred_pose.dtype)                         # (the kernels are fp32)
        return rotmat.view(NT, 24, 3, 3), pred_shape, torch.cat([aa.reshape(NT, 72), pred_shape], dim=1)

    def forward(self, feat, init_pose=None, init_shape=None):
        NT = feat.shape[0] * feat.shape[1]
        pred_rotmat, pred_shape, theta = self.forward_params(feat)
        if isinstance(self.smpl, SMPLLayer):
            # the project's own layer: vertices in millimetres and the 17 regressed joints from one fused launch (no [NT,V,3] product
            # with 1000 and no batched [17,V] matmul; their gradients come back through mbx_smpl_bwd)
            verts, kp = self.smpl.forward_kp(pred_shape, pred_rotmat, self._regressor(pred_shape.device, torch.float32), 1000.0, ops=self.ops)
            return [{'theta': theta, 'verts': verts.to(theta.dtype), 'kp_3d': kp.to(theta.dtype)}]
        pred_output = self.smpl(betas=pred_shape, body_pose=pred_rotmat[:, 1:], global_orient=pred_rotmat[:, 0].unsqueeze(1), pose2rot=False)
        pred_vertices = pred_output.vertices * 1000.0
        pred_joints = torch.matmul(self._regressor(pred_vertices.device, pred_vertices.dtype)[None].expand(NT, -1, -1), pred_vertices)
        return [{'theta': theta,                                                    # (N*T, 72+10)
                 'verts': pred_vertices,                                            # (N*T, V, 3)
                 'kp_3d': pred_joints}]                                             # (N*T, 17, 3)


class MeshRegressor(nn.Module):
    """model_mesh.py:82-101: `MeshRegressor(backbone, head)` with a ready `SMPLRegressor`, or `MeshRegressor(backbone, smpl=, init_pose=,
    init_shape=, J_regressor=, dim_rep=, num_joints=, hidden_dim=, dropout_ratio=)` (the reference's default dropout_ratio 0.5).
    forward: x [N,T,17,3] -> a list with one dict `theta` [N,T,82] / `verts` [N,T,V,3] / `kp_3d` [N,T,17,3]."""

    def __init__(self, backbone, head=None, dim_rep=512, num_joints=17, hidden_dim=2048, dropout_ratio=0.5, **head_args):
        super().__init__()
        self.backbone = backbone
        self.feat_J = num_joints
        if head is None:
            head = SMPLRegressor(dim_rep=dim_rep, num_joints=num_joints, hidden_dim=hidden_dim, dropout_ratio=dropout_ratio, **head_args)
        elif head_args:
            raise ValueError(f'MeshRegressor: a ready head and head arguments {sorted(head_args)} exclude each other')
        self.head = head

    def forward(self, x, init_pose=None, init_shape=None, n_iter=3):
        N, T, J, C = x.shape
        feat = self.backbone.get_representation(x).reshape([N, T, self.feat_J, -1])
        smpl_output = self.head(feat)
        for s in smpl_output:
            s['theta'] = s['theta'].reshape(N, T, -1)
            s['verts'] = s['verts'].reshape(N, T, -1, 3)
            s['kp_3d'] = s['kp_3d'].reshape(N, T, -1, 3)
        return smpl_output


# ---------------------------------------------------------------------------------------------------------------- loss
def _joint_call(ops, kp, gt, lam6, want_grad):
    losses = torch.empty(8, dtype=torch.float32, device=kp.device)
    d = torch.empty_like(kp) if want_grad else None
    ops.pose_loss_full(kp, gt, lam6, losses, d)
    return losses, d


def _param_call(ops, loss_type, theta, gt_theta, lam3, want_grad):
    losses = torch.empty(4, dtype=torch.float32, device=theta.device)
    d = torch.empty_like(theta) if want_grad else None
    ops.mesh_param_loss(theta, gt_theta, loss_type, lam3, losses, d)
    return losses, d


def _log10(joint, param):
    """the ten values in the order of LOSS_KEYS from mbx_pose_loss_full's [8] and mbx_mesh_param_loss's [4] = pose, shape, norm, sum"""
    return torch.cat([joint[:7], param[1:2], param[0:1], param[2:3]])


class _MeshTotalFn(torch.autograd.Function):
    """total = sum lambda_i loss_i and the log; both cotangents come out of the two forward calls"""

    @staticmethod
    def forward(ctx, ops, kp, gt_kp, theta, gt_theta, lam10, loss_type):
        l3d, lam6 = lam10[0], lam10[1:7]
        lam3 = (lam10[8], lam10[7], lam10[9])                         # the kernel's order: pose, shape, norm
        gk, gth = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if l3d != 0.0:
            # mbx_pose_loss_full fixes the weight of loss_mpjpe at 1: the other six lambdas are divided by lambda_3d and the total and
            # the cotangent multiplied by it
            joint, dk = _joint_call(ops, kp, gt_kp, tuple(v / l3d for v in lam6), gk)
            jtotal = joint[7] * l3d
            if dk is not None:
                dk = dk * l3d
        else:
            # lambda_3d == 0: (mpjpe + sum lambda_k term_k) - mpjpe, two calls
            joint, dk = _joint_call(ops, kp, gt_kp, lam6, gk)
            if dk is not None:
                dk = dk - _joint_call(ops, kp, gt_kp, (0.0,) * 6, True)[1]
            jtotal = joint[7] - joint[0]
        param, dth = _param_call(ops, loss_type, theta, gt_theta, lam3, gth)
        ctx.dk, ctx.dth = dk, dth
        log = _log10(joint, param)
        ctx.mark_non_differentiable(log)
        return jtotal + param[3], log

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dtotal, _dlog):
        dk, dth = ctx.dk, ctx.dth
        ctx.dk = ctx.dth = None
        return None, (dk * dtotal if dk is not None else None), None, (dth * dtotal if dth is not None else None), None, None, None


class _MeshTermsFn(torch.autograd.Function):
    """the ten losses as ten differentiable outputs: backward runs one kernel call per output that received a cotangent (the joint terms
    2 .. 7 one more, shared: the kernel's total always carries loss_mpjpe with weight 1, which is subtracted again)"""

    @staticmethod
    def forward(ctx, ops, kp, gt_kp, theta, gt_theta, loss_type):
        joint, _ = _joint_call(ops, kp, gt_kp, (0.0,) * 6, False)
        param, _ = _param_call(ops, loss_type, theta, gt_theta, (0.0, 0.0, 0.0), False)
        ctx.ops, ctx.loss_type = ops, loss_type
        ctx.save_for_backward(kp, gt_kp, theta, gt_theta)
        ctx.set_materialize_grads(False)
        return tuple(_log10(joint, param).unbind(0))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        kp, gt_kp, theta, gt_theta = ctx.saved_tensors
        ops = ctx.ops
        dk = dth = None
        if ctx.needs_input_grad[1] and any(v is not None for v in g[:7]):
            base = _joint_call(ops, kp, gt_kp, (0.0,) * 6, True)[1]
            dk = base * g[0] if g[0] is not None else torch.zeros_like(kp)
            for k in range(1, 7):
                if g[k] is not None:
                    e = tuple(1.0 if i == k - 1 else 0.0 for i in range(6))
                    dk = dk + (_joint_call(ops, kp, gt_kp, e, True)[1] - base) * g[k]
        if ctx.needs_input_grad[3] and any(v is not None for v in g[7:]):
            dth = torch.zeros_like(theta)
            for slot, k in ((0, 8), (1, 7), (2, 9)):             # kernel slot (pose, shape, norm) <- position in LOSS_KEYS
                if g[k] is not None:
                    e = tuple(1.0 if i == slot else 0.0 for i in range(3))
                    dth = dth + _param_call(ops, ctx.loss_type, theta, gt_theta, e, True)[1] * g[k]
        return None, dk, None, dth, None, None


def _lambdas10(lambdas):
    if isinstance(lambdas, dict):
        return tuple(float(lambdas[n]) for n in LAMBDA_NAMES)
    return tuple(float(getattr(lambdas, n)) for n in LAMBDA_NAMES)


class MeshLoss(nn.Module):
    """loss_mesh.py:7-68.  `forward(smpl_output, data_gt)` returns the reference's dict of ten 0-dim device tensors (`loss_3d_pos`,
    `loss_3d_scale`, `loss_3d_velocity`, `loss_lv`, `loss_lg`, `loss_a`, `loss_av`, `loss_shape`, `loss_pose`, `loss_norm`) from
    `smpl_output[-1]['theta' / 'kp_3d']` [N,T,82] / [N,T,17,3] and `data_gt['theta' / 'kp_3d']`.

    With `lambdas` (an object or dict carrying `lambda_3d, lambda_scale, lambda_3dv, lambda_lv, lambda_lg, lambda_a, lambda_av, lambda_shape,
    lambda_pose, lambda_norm` as train_mesh.py:180-189 reads them) the dict also has `total`, the trainer's weighted sum.  Only `total` is
    differentiable then: its gradient comes out of the same two kernel calls that computed the values, and the ten entries are the log.
    `mbx_pose_loss_full` fixes the weight of `loss_3d_pos` at 1; `lambda_3d` is honoured by handing the kernel the six other joint
    lambdas divided by `lambda_3d` and multiplying its total and its cotangent by `lambda_3d`.  With `lambda_3d == 0` the kernel is
    called twice (with the lambdas, and with all of them 0) and the `loss_3d_pos` part is subtracted.

    Without `lambdas` every entry is individually differentiable, so the reference's own weighting line works unchanged; backward
    then costs one kernel call per entry that is used."""

    def __init__(self, loss_type='MSE', lambdas=None, device='cuda', ops=None):
        super().__init__()
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type must be 'MSE' or 'L1', got {loss_type!r}")
        self.loss_type, self.device, self.ops = loss_type, device, ops
        self.lambdas = None if lambdas is None else _lambdas10(lambdas)

    def forward(self, smpl_output, data_gt):
        preds = smpl_output[-1]
        theta, kp = preds['theta'], preds['kp_3d']
        gt_theta, gt_kp = data_gt['theta'], data_gt['kp_3d']
        if theta.dim() != 3 or theta.shape[-1] != 82 or theta.shape[0] * theta.shape[1] < 1 or tuple(gt_theta.shape) != tuple(theta.shape):
            raise ValueError(f'theta [N,T,82] expected for prediction and target, got {tuple(theta.shape)} / {tuple(gt_theta.shape)}')
        if tuple(kp.shape) != tuple(theta.shape[:2]) + (17, 3) or tuple(gt_kp.shape) != tuple(kp.shape):
            raise ValueError(f'kp_3d [N,T,17,3] expected for prediction and target, got {tuple(kp.shape)} / {tuple(gt_kp.shape)}')
        ops = hip_ops.provider(self.ops, 'motionbert_amd.mesh.MeshLoss', theta, kp, gt_theta, gt_kp)
        kp_local = (kp - kp[:, :, 0:1, :]).float().contiguous()                    # loss_mesh.py:36-37
        gt_local = (gt_kp - gt_kp[:, :, 0:1, :]).detach().float().contiguous()
        th = theta.reshape(-1, 82).float().contiguous()
        gth = gt_theta.reshape(-1, 82).detach().float().contiguous()
        t = LOSS_TYPES[self.loss_type]
        if self.lambdas is None:
            return dict(zip(LOSS_KEYS, _MeshTermsFn.apply(ops, kp_local, gt_local, th, gth, t)))
        total, log = _MeshTotalFn.apply(ops, kp_local, gt_local, th, gth, self.lambdas, t)
        out = dict(zip(LOSS_KEYS, log.unbind(0)))
        out['total'] = total
        return out


# ---------------------------------------------------------------------------------------------------------------- errors
def _frames(output, target):
    out = output[0] if isinstance(output, (list, tuple)) else output
    kp_p, kp_g = out['kp_3d'], target['kp_3d']
    if kp_p.shape[-2:] != (17, 3) or tuple(kp_g.shape) != tuple(kp_p.shape):
        raise ValueError(f'kp_3d [...,17,3] expected for prediction and target, got {tuple(kp_p.shape)} / {tuple(kp_g.shape)}')
    vp, vg = out.get('verts'), target.get('verts')
    if (vp is None) != (vg is None):
        raise ValueError('verts must be given for prediction and target, or for neither')
    F = kp_p.numel() // 51
    if vp is not None:
        if vp.shape[-1] != 3 or tuple(vg.shape) != tuple(vp.shape) or vp.numel() % (3 * max(F, 1)) != 0 or (F and vp.numel() == 0):
            raise ValueError(f'verts [...,V,3] with the frames of kp_3d expected for prediction and target, got {tuple(vp.shape)} / {tuple(vg.shape)}')
        V = vp.shape[-2]
        vp, vg = vp.detach().reshape(-1, V, 3).float().contiguous(), vg.detach().reshape(-1, V, 3).float().contiguous()
        if vp.shape[0] != F:
            raise ValueError(f'verts have {vp.shape[0]} frames, kp_3d {F}')
    return vp, vg, kp_p.detach().reshape(-1, 17, 3).float().contiguous(), kp_g.detach().reshape(-1, 17, 3).float().contiguous()


def mesh_errors(output, target, ops=None) -> torch.Tensor:
    """err [5,F] float64 on the device, rows ERROR_KEYS, for `output` (the model's list, or its dict) and `target` (dict): `verts`
    [...,V,3] (optional on both) and `kp_3d` [...,17,3].  Without `verts` the `mpve` row is NaN."""
    vp, vg, kp, kg = _frames(output, target)
    ops = hip_ops.provider(ops, 'motionbert_amd.mesh.mesh_errors', vp, vg, kp, kg)
    err = torch.empty(5, kp.shape[0], dtype=torch.float64, device=kp.device)
    if kp.shape[0]:
        ops.mesh_errors(vp, vg, kp, kg, err)
    return err


def compute_error_frames(output, target, ops=None):
    """utils_mesh.py:376-393: `(mpjpes [F], mpves [F])`, the 17-joint MPJPE and the MPVE per frame -- float64 tensors on the device (the
    reference returns fp32 on the host, which is a synchronisation)."""
    err = mesh_errors(output, target, ops)
    return err[1], err[0]


def compute_error(output, target, ops=None):
    """utils_mesh.py:357-374: `(mpjpe, mpve)` as 0-dim device tensors, the means of `compute_error_frames`."""
    mpjpes, mpves = compute_error_frames(output, target, ops)
    return mpjpes.mean(), mpves.mean()


class MeshEvaluator:
    """`evaluate_mesh` (utils_mesh.py:395-438) accumulated on the device.

        ev = MeshEvaluator()
        for batch_input, batch_gt in test_loader: ev.update(model(batch_input.cuda()), batch_gt)      # batch_gt's tensors on the device
        errors = ev.finish()       # {'mpve', 'mpjpe', 'pa_mpjpe', 'mpjpe_17j', 'pa_mpjpe_17j'}: the one host synchronisation

    `update` runs `mbx_mesh_errors` on the batch and keeps its [5, frames] float64 result on the device (40 bytes per frame where the
    reference keeps 165 KB per frame on the host); it returns that result.  `finish` averages every row over all frames seen."""

    def __init__(self, ops=None):
        hip_ops.evaluator_provider(ops, None, 'motionbert_amd.mesh.MeshEvaluator')
        self.ops = ops                      # (stays None without an injected provider: every update() then checks where its tensors are)
        self.reset()

    def reset(self):
        self.rows = []
        self.count = 0

    def update(self, output, batch_gt) -> torch.Tensor:
        err = mesh_errors(output, batch_gt, self.ops)
        self.rows.append(err)
        self.count += err.shape[1]
        return err

    def frames(self) -> torch.Tensor:
        """[5, frames seen] on the device"""
        if not self.rows:
            raise RuntimeError('no update() yet')
        return torch.cat(self.rows, dim=1)

    def finish(self) -> dict:
        if self.count == 0:
            raise RuntimeError('finish() before any update()')
        mean = self.frames().mean(dim=1).cpu().tolist()
        return {k: mean[ERROR_KEYS.index(k)] for k in ('mpve', 'mpjpe', 'pa_mpjpe', 'mpjpe_17j', 'pa_mpjpe_17j')}


# ---------------------------------------------------------------------------------------------------------------- flip evaluation
THETA_FLIP_PERM = (0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22)     # utils_mesh.py:503, as a permutation
JOINT_FLIP_PERM = (0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13)                                   # flip_data, utils_data.py:61-65


def flip_thetas_batch(thetas: torch.Tensor) -> torch.Tensor:
    """utils_mesh.py:486-513: thetas [N,F,72] axis-angle -> the pose of the mirrored body: the y and z components of every joint negated,
    left and right joints swapped.  A new tensor; bit-equal to the reference's."""
    if thetas.dim() != 3 or thetas.shape[-1] != 72:
        raise ValueError(f'thetas [N,F,72] expected, got {tuple(thetas.shape)}')
    t = thetas.reshape(*thetas.shape[:2], 24, 3)
    sign = torch.tensor([1.0, -1.0, -1.0], dtype=thetas.dtype, device=thetas.device)
    return (t * sign).index_select(2, torch.tensor(THETA_FLIP_PERM, device=thetas.device)).reshape(*thetas.shape[:2], 72)


def flip_input(x: torch.Tensor) -> torch.Tensor:
    """`flip_data` (utils_data.py:54-66) of [..., 17, D]: x negated, left and right joints swapped; a new tensor"""
    f = x.index_select(-2, torch.tensor(JOINT_FLIP_PERM, device=x.device)).clone()
    f[..., 0] = -f[..., 0]
    return f


def flip_average(model, smpl, batch_input: torch.Tensor, output=None):
    """train_mesh.py:83-108 (`args.flip`): the model on the flipped input, its thetas flipped back, SMPL with `pose2rot=True`, the joint
    regression, and per key the mean with the model's output on the input itself (`output`: that output where the caller already has it).
    Returns the list with one dict `theta` [N,T,82] / `verts` [N,T,V,3] / `kp_3d` [N,T,17,3] that `MeshEvaluator.update` takes.  With an
    `SMPLLayer` the vertices and joints of the flipped pass come from one fused launch; any other `smpl` is called as the reference calls it."""
    with torch.no_grad():
        if output is None:
            output = model(batch_input)
        N, T = batch_input.shape[:2]
        flipped = model(flip_input(batch_input))[0]
        pose = flip_thetas_batch(flipped['theta'][:, :, :72]).reshape(-1, 72)
        shape = flipped['theta'][:, :, 72:].reshape(-1, 10)
        Q = smpl.J_regressor_h36m
        if isinstance(smpl, SMPLLayer):
            rot = rodrigues(pose.reshape(-1, 3).float()).view(N * T, 24, 3, 3)
            verts, kp = smpl.forward_kp(shape.float().contiguous(), rot, Q, 1000.0)
        else:
            verts = smpl(betas=shape, body_pose=pose[:, 3:], global_orient=pose[:, :3], pose2rot=True).vertices.detach() * 1000.0
            kp = torch.matmul(Q.to(verts)[None].expand(verts.shape[0], -1, -1), verts)
        back = {'theta': torch.cat([pose.reshape(N, T, -1), shape.reshape(N, T, -1)], dim=-1), 'verts': verts.reshape(N, T, -1, 3),
                'kp_3d': kp.reshape(N, T, -1, 3)}
        return [{k: (output[0][k] + back[k].to(output[0][k].dtype)) * 0.5 for k in flipped}]


# ---------------------------------------------------------------------------------------------------------------- targets
TARGET_KEYS = ('theta', 'kp_3d', 'verts')


def mesh_targets(smpl, pose, shape, motion_2d=None, flip=None, seed=None, flip_prob=0.5, want=TARGET_KEYS, return_flips=False, ops=None):
    """`(motion_2d_out or None, {'theta': [N,T,82], 'kp_3d': [N,T,17,3], 'verts': [N,T,V,3]})`: what `MotionSMPL.__getitem__` returns for
    every clip of a batch, from pose [N,T,72] (axis-angle), shape [N,T,10] and the 2D input motion_2d [N,T,17,3] (optional), in one
    `mbx_mesh_gt` on the device.  `smpl`: an `SMPLLayer` with `J_regressor_h36m`.  Millimetres (`* 1000`), root = the regressed joint 0.

    `flip`: None / False no clip is flipped (the test split); True every clip is flipped with probability `flip_prob`, drawn on the device
    from `seed` (default: 62 bits from torch's CPU generator) and the clip's index; a [N] bool / uint8 tensor flips the clips it marks.  A
    flipped clip has `flip_data` applied to its 2D input and `flip_thetas` to its pose before SMPL.  `want`: the keys to compute (a subset of
    'theta', 'kp_3d', 'verts'; with `motion_2d` or `return_flips` it may be empty).  `return_flips=True` appends the flags used ([N] uint8).
    No autograd, no host synchronisation; fp32."""
    if not isinstance(smpl, SMPLLayer):
        raise TypeError('mesh_targets needs an SMPLLayer')
    Q = smpl.J_regressor_h36m
    if Q is None:
        raise ValueError('mesh_targets needs the model\'s J_regressor_h36m (the layer has none)')
    want = tuple(want)
    if any(k not in TARGET_KEYS for k in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a subset of {TARGET_KEYS}, got {want}')
    if not want and motion_2d is None and not return_flips:
        raise ValueError('mesh_targets: nothing to compute (empty want, no motion_2d, return_flips off)')
    if pose.dim() != 3 or pose.shape[2] != 72 or pose.shape[1] < 1:
        raise ValueError(f'pose [N,T,72] expected, got {tuple(pose.shape)}')
    N, T = pose.shape[:2]
    if tuple(shape.shape) != (N, T, 10):
        raise ValueError(f'shape [{N},{T},10] expected, got {tuple(shape.shape)}')
    if motion_2d is not None and tuple(motion_2d.shape) != (N, T, 17, 3):
        raise ValueError(f'motion_2d [{N},{T},17,3] expected, got {tuple(motion_2d.shape)}')
    flags = None
    if torch.is_tensor(flip):
        if tuple(flip.shape) != (N,) or flip.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'flip [{N}] bool or uint8 expected, got {tuple(flip.shape)} {flip.dtype}')
        flags = flip
    elif flip is not None and not isinstance(flip, bool):
        raise ValueError(f'flip must be None, a bool or a [N] tensor, got {flip!r}')
    if not 0.0 <= float(flip_prob) <= 1.0:
        raise ValueError(f'flip_prob must lie in [0, 1], got {flip_prob}')
    ops = hip_ops.provider(ops, 'motionbert_amd.mesh.mesh_targets', pose, shape, motion_2d, flags, smpl.v_template, move=_MOVE)
    dev = pose.device
    if any(t is not None and t.device != dev for t in (shape, motion_2d, flags, smpl.v_template)):
        raise ValueError(f'mesh_targets: the layer and every tensor must be on one device (pose is on {dev})')
    prob = 0.0
    if flip is True:
        prob = float(flip_prob)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    with torch.no_grad():
        pose, shape = pose.detach().float().contiguous(), shape.detach().float().contiguous()
        m2d = None if motion_2d is None else motion_2d.detach().float().contiguous()
        if flags is not None:
            flags = flags.detach().to(torch.uint8).contiguous()
        if Q.dtype != torch.float32 or not Q.is_contiguous():
            Q = Q.float().contiguous()
        K, V = Q.shape[0], smpl.num_vertices
        if not N:
            out = {'theta': pose.new_empty(0, T, 82), 'kp_3d': pose.new_empty(0, T, K, 3), 'verts': pose.new_empty(0, T, V, 3)}
            res = (None if m2d is None else torch.empty_like(m2d), {k: out[k] for k in want})
            return res + (torch.empty(0, dtype=torch.uint8, device=dev),) if return_flips else res
        x2d = None if m2d is None else torch.empty_like(m2d)
        out = {}
        if 'theta' in want:
            out['theta'] = torch.empty(N, T, 82, dtype=torch.float32, device=dev)
        if 'kp_3d' in want:
            out['kp_3d'] = torch.empty(N, T, K, 3, dtype=torch.float32, device=dev)
        if 'verts' in want:
            out['verts'] = torch.empty(N, T, V, 3, dtype=torch.float32, device=dev)
        used = torch.empty(N, dtype=torch.uint8, device=dev) if return_flips else None
        ops.mesh_gt(smpl.model_tensors(), Q, pose, shape, m2d, flags, 0 if seed is None else int(seed), prob, 1000.0, x2d, out.get('theta'),
                    out.get('kp_3d'), out.get('verts'), used, ws=smpl.workspace(ops, 'gt', N * T, K, dev))
    res = (x2d, {k: out[k] for k in want})
    return res + (used,) if return_flips else res


# ---------------------------------------------------------------------------------------------------------------- step
LOG_KEYS = LOSS_KEYS + ('total', 'mpjpe', 'mpve')


class MeshStep(TwoGroupStep):
    """One optimizer step of train_mesh.py:165-203: forward, `MeshLoss` with the trainer's lambdas, `compute_error`, backward, and the two
    AdamW groups of `train.TwoGroupStep` (:316-321).  `batch_gt`: dict with `theta` [N,T,82], `kp_3d` [N,T,17,3], `verts` [N,T,V,3] on the device.
    Returns the log: a device tensor [13] in the order of LOG_KEYS (the ten losses, the weighted total, the step's mean 17-joint MPJPE and
    MPVE); nothing is synchronised with the host (the reference ends every step with eleven `.item()` calls and a `.cpu()`).
    Single-process only."""

    def __init__(self, model, lr_backbone: float = 5e-5, lr_head: float = 5e-4, weight_decay: float = 0.01, lambdas=None,
                 loss_type: str = 'L1', ops=None):
        if lambdas is None:
            raise ValueError('MeshStep needs the trainer\'s lambdas (lambda_3d ... lambda_norm)')
        self.ops = ops
        self.criterion = MeshLoss(loss_type=loss_type, lambdas=lambdas, ops=ops)
        super().__init__(model, lr_backbone, lr_head, weight_decay)

    def __call__(self, batch_input: torch.Tensor, batch_gt: dict) -> torch.Tensor:
        output = self.model(batch_input)
        self.zero_grad()
        losses = self.criterion(output, batch_gt)
        with torch.no_grad():
            mpjpe, mpve = compute_error(output, batch_gt, self.ops)
        losses['total'].backward()
        self.step()
        return torch.cat([torch.stack([losses[k].detach() for k in LOSS_KEYS + ('total',)]).double(), torch.stack([mpjpe, mpve])])
