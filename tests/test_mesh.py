"""motionbert_amd.mesh on the CPU with a torch kernel provider injected through `ops=` (tests/mesherr.TorchOps: the float64 restatements):
names, shapes, bookkeeping, the lambda_3d handling and the refusals.  The kernels themselves: tests/test_gpu_mesh.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import mesherr as ME

DIM_REP, HIDDEN, V = 8, 16, 64


class Backbone(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, DIM_REP)

    def get_representation(self, x):
        return torch.tanh(self.lin(x))


def regressor(ops, seed=3, dropout=0.0):
    from motionbert_amd.mesh import MeshRegressor
    torch.manual_seed(seed)
    smpl = ME.StandInSMPL(V)
    pose, shape = ME.mean_params()
    return MeshRegressor(Backbone(), smpl=smpl, init_pose=pose, init_shape=shape, J_regressor=smpl.J_regressor_h36m, dim_rep=DIM_REP,
                         hidden_dim=HIDDEN, dropout_ratio=dropout, ops=ops)


def test_state_dict_keys_shapes_and_initialisation():
    ops = ME.TorchOps()
    net = regressor(ops)
    head = sorted(k for k in net.state_dict() if not k.startswith('backbone.'))
    bn = ['bias', 'num_batches_tracked', 'running_mean', 'running_var', 'weight']
    want = sorted(['head.%s.%s' % (m, p) for m in ('fc1', 'fc2', 'head_pose', 'head_shape') for p in ('weight', 'bias')] +
                  ['head.%s.%s' % (m, p) for m in ('bn1', 'bn2') for p in bn] + ['head.init_pose', 'head.init_shape'] +
                  ['head.smpl.' + n for n in ('template', 'shapedirs', 'weights')])
    assert head == want
    assert sorted(k for k in net.state_dict() if k.startswith('backbone.')) == ['backbone.lin.bias', 'backbone.lin.weight']
    assert net.head.fc1.weight.shape == (HIDDEN, 17 * DIM_REP) and net.head.head_pose.weight.shape == (144, HIDDEN)
    assert net.head.init_pose.shape == (1, 144) and net.head.init_shape.shape == (1, 10)
    for lin in (net.head.head_pose, net.head.head_shape):      # xavier_uniform_(gain=0.01), model_mesh.py:23-24
        bound = 0.01 * math.sqrt(6.0 / sum(lin.weight.shape))
        assert 0.5 * bound < float(lin.weight.detach().abs().max()) <= bound
    other = regressor(ops, seed=4)
    other.load_state_dict(net.state_dict(), strict=True)
    out = net.train()(torch.randn(2, 5, 17, 3))
    assert isinstance(out, list) and len(out) == 1 and sorted(out[0]) == ['kp_3d', 'theta', 'verts']
    assert out[0]['theta'].shape == (2, 5, 82) and out[0]['verts'].shape == (2, 5, V, 3) and out[0]['kp_3d'].shape == (2, 5, 17, 3)
    assert bool((out[0]['theta'][:, :, 72:] == out[0]['theta'][:, :1, 72:]).all()), 'one shape per clip'
    assert ops.calls == {'rot6d_theta_fwd': 1}


def test_forward_and_gradient_match_the_plain_torch_head():
    ops = ME.TorchOps()
    net = regressor(ops).double().train()
    x = torch.randn(2, 3, 17, 3, dtype=torch.float64)
    out = net(x)[0]
    w = {k: torch.randn_like(v) for k, v in out.items()}
    sum((out[k] * w[k]).sum() for k in out).backward()
    got = {n: p.grad.clone() for n, p in net.named_parameters()}
    net.zero_grad()
    ref = ME.plain_head_forward(net.head, net.backbone.get_representation(x).reshape(2, 3, 17, -1))[0]
    sum((ref[k] * w[k].double()).sum() for k in ref).backward()
    for k in out:                      # the provider rounds the chain's outputs to fp32
        assert float((out[k] - ref[k]).detach().abs().max()) <= 1e-6 * float(ref[k].detach().abs().max()), k
    grads = dict(net.named_parameters())
    for n in ('head.head_pose.weight', 'head.head_pose.bias', 'head.head_shape.weight', 'head.fc1.weight', 'head.fc2.weight', 'backbone.lin.weight'):
        assert float((got[n] - grads[n].grad).abs().max()) <= 1e-5 * float(grads[n].grad.abs().max()), n      # (fc biases: BatchNorm cancels them)
    assert ops.calls['rot6d_theta_bwd'] == 1


def outputs_and_targets(seed=5, N=2, T=4):
    g = torch.Generator().manual_seed(seed + 1000)
    tgt = ME.mesh_targets(N, T, V, seed)
    out = [{'theta': (tgt['theta'] + 0.2 * torch.randn(N, T, 82, generator=g)).requires_grad_(True),
            'kp_3d': (tgt['kp_3d'] + 30.0 * torch.randn(N, T, 17, 3, generator=g)).requires_grad_(True),
            'verts': tgt['verts'] + 30.0 * torch.randn(N, T, V, 3, generator=g)}]
    return out, tgt


@pytest.mark.parametrize('loss_type', ('MSE', 'L1'))
def test_mesh_loss_dict_and_values(loss_type):
    from motionbert_amd.mesh import LOSS_KEYS, MeshLoss
    from tests import limberr
    out, tgt = outputs_and_targets()
    d = MeshLoss(loss_type=loss_type, ops=ME.TorchOps())(out, tgt)
    assert tuple(d) == LOSS_KEYS == ('loss_3d_pos', 'loss_3d_scale', 'loss_3d_velocity', 'loss_lv', 'loss_lg', 'loss_a', 'loss_av', 'loss_shape',
                                     'loss_pose', 'loss_norm')
    assert all(v.shape == () and v.requires_grad for v in d.values())
    kp, gk = out[0]['kp_3d'].detach().double(), tgt['kp_3d'].double()
    seven = limberr.terms64(kp - kp[:, :, :1], gk - gk[:, :, :1])
    lp, ls, ln = ME.param_losses(out[0]['theta'].detach().double().reshape(-1, 82), tgt['theta'].double().reshape(-1, 82), ('MSE', 'L1').index(loss_type))
    for k, ref in zip(LOSS_KEYS, seven + [ls, lp, ln]):
        assert float(d[k].detach()) == pytest.approx(float(ref), rel=1e-6), k
    with pytest.raises(ValueError, match='MSE'):
        MeshLoss(loss_type='huber')


@pytest.mark.parametrize('lambda_3d', (0.5, 1.0, 0.0))
def test_total_honours_lambda_3d_and_every_other_lambda(lambda_3d):
    from motionbert_amd.mesh import LAMBDA_NAMES, LOSS_KEYS, MeshLoss

    class L(ME.Lambdas):
        pass
    L.lambda_3d = lambda_3d
    ops = ME.TorchOps()
    out, tgt = outputs_and_targets()
    d = MeshLoss(loss_type='L1', lambdas=L, ops=ops)(out, tgt)
    assert tuple(d) == LOSS_KEYS + ('total',)
    assert d['total'].requires_grad and not any(d[k].requires_grad for k in LOSS_KEYS)
    assert ops.calls == ({'pose_loss_full': 1, 'mesh_param_loss': 1} if lambda_3d else {'pose_loss_full': 2, 'mesh_param_loss': 1})
    d['total'].backward()
    assert ops.calls['mesh_param_loss'] == 1, 'the cotangents came out of the forward calls'
    got = (out[0]['kp_3d'].grad.clone(), out[0]['theta'].grad.clone())
    out[0]['kp_3d'].grad = out[0]['theta'].grad = None
    # the reference's own weighting line on the individually differentiable entries
    e = MeshLoss(loss_type='L1', ops=ME.TorchOps())(out, tgt)
    total = sum(getattr(L, n) * e[k] for n, k in zip(LAMBDA_NAMES, LOSS_KEYS))
    total.backward()
    assert float(d['total']) == pytest.approx(float(total), rel=1e-5)
    for a, b in zip(got, (out[0]['kp_3d'].grad, out[0]['theta'].grad)):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    # a dict of lambdas serves as well
    d2 = MeshLoss(loss_type='L1', lambdas={n: getattr(L, n) for n in LAMBDA_NAMES}, ops=ME.TorchOps())(out, tgt)
    assert float(d2['total']) == float(d['total'])


def test_entries_are_individually_differentiable_at_one_call_per_used_term():
    from motionbert_amd.mesh import MeshLoss
    ops = ME.TorchOps()
    out, tgt = outputs_and_targets()
    d = MeshLoss(loss_type='MSE', ops=ops)(out, tgt)
    before = dict(ops.calls)
    (d['loss_pose'] + 2.0 * d['loss_3d_pos']).backward()
    assert ops.calls['mesh_param_loss'] - before['mesh_param_loss'] == 1 and ops.calls['pose_loss_full'] - before['pose_loss_full'] == 1
    th = out[0]['theta'].detach().double().reshape(-1, 82)
    _, want = ME.param_loss_grad(th.float(), tgt['theta'].reshape(-1, 82), 0, (1.0, 0.0, 0.0), torch.float64)
    assert float((out[0]['theta'].grad.reshape(-1, 82) - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert float(out[0]['theta'].grad[..., 72:].abs().max()) == 0.0, 'loss_pose alone does not reach the shape'


def test_evaluator_over_three_batches_equals_one_call():
    from motionbert_amd.mesh import MeshEvaluator, compute_error, compute_error_frames
    ops = ME.TorchOps()
    out, tgt = outputs_and_targets(N=6, T=2)
    out = [{k: v.detach() for k, v in out[0].items()}]
    ev = MeshEvaluator(ops=ops)
    with pytest.raises(RuntimeError, match='before any update'):
        ev.finish()
    for lo, hi in ((0, 1), (1, 4), (4, 6)):
        r = ev.update([{k: v[lo:hi] for k, v in out[0].items()}], {k: v[lo:hi] for k, v in tgt.items()})
        assert r.shape == (5, 2 * (hi - lo)) and r.dtype == torch.float64
    got = ev.finish()
    assert ev.count == 12 and tuple(got) == ('mpve', 'mpjpe', 'pa_mpjpe', 'mpjpe_17j', 'pa_mpjpe_17j')
    ref = ME.aggregate(ME.mesh_errors64(out[0]['verts'].reshape(-1, V, 3).numpy(), tgt['verts'].reshape(-1, V, 3).numpy(),
                                        out[0]['kp_3d'].reshape(-1, 17, 3).numpy(), tgt['kp_3d'].reshape(-1, 17, 3).numpy()))
    for k in got:
        assert got[k] == pytest.approx(ref[k], rel=1e-12), k
    mpjpes, mpves = compute_error_frames(out, tgt, ops=ops)
    assert mpjpes.shape == (12,) and mpves.shape == (12,)
    mpjpe, mpve = compute_error(out, tgt, ops=ops)
    assert float(mpjpe) == pytest.approx(ref['mpjpe_17j'], rel=1e-12) and float(mpve) == pytest.approx(ref['mpve'], rel=1e-12)
    # joints only: the MPVE row is NaN
    only = ev.__class__(ops=ops)
    only.update({'kp_3d': out[0]['kp_3d']}, {'kp_3d': tgt['kp_3d']})
    res = only.finish()
    assert math.isnan(res['mpve']) and res['pa_mpjpe'] == pytest.approx(ref['pa_mpjpe'], rel=1e-12)


def test_refusals():
    from motionbert_amd.mesh import MeshLoss, MeshRegressor, MeshStep, SMPLRegressor, compute_error, rot6d_to_rotmat_theta
    ops = ME.TorchOps()
    with pytest.raises(RuntimeError, match='no CPU path'):
        rot6d_to_rotmat_theta(torch.zeros(4, 6))
    with pytest.raises(ValueError, match='multiple of 6'):
        rot6d_to_rotmat_theta(torch.zeros(4, 5), ops=ops)
    with pytest.raises(ValueError, match='floating-point'):
        rot6d_to_rotmat_theta(torch.zeros(4, 6, dtype=torch.int64), ops=ops)
    out, tgt = outputs_and_targets()
    with pytest.raises(RuntimeError, match='no CPU path'):
        MeshLoss()(out, tgt)
    with pytest.raises(RuntimeError, match='no CPU path'):
        compute_error(out, tgt)
    with pytest.raises(ValueError, match=r'theta \[N,T,82\]'):
        MeshLoss(ops=ops)([{'theta': out[0]['theta'][..., :72], 'kp_3d': out[0]['kp_3d']}], tgt)
    with pytest.raises(ValueError, match=r'kp_3d \[N,T,17,3\]'):
        MeshLoss(ops=ops)([{'theta': out[0]['theta'], 'kp_3d': out[0]['kp_3d'][:, :, :16]}], tgt)
    with pytest.raises(ValueError, match='kp_3d'):
        compute_error([{'kp_3d': out[0]['kp_3d'][:, :, :16]}], tgt, ops=ops)
    with pytest.raises(ValueError, match='verts'):
        compute_error([{'kp_3d': out[0]['kp_3d'], 'verts': out[0]['verts']}], {'kp_3d': tgt['kp_3d']}, ops=ops)
    with pytest.raises(AttributeError):
        MeshLoss(lambdas=object(), ops=ops)
    smpl = ME.StandInSMPL(V)
    pose, shape = ME.mean_params()
    with pytest.raises(ValueError, match='144'):
        SMPLRegressor(smpl, pose[:, :72], shape, smpl.J_regressor_h36m)
    with pytest.raises(ValueError, match='J_regressor'):
        SMPLRegressor(smpl, pose, shape, smpl.J_regressor_h36m[:14])
    head = SMPLRegressor(smpl, pose, shape, smpl.J_regressor_h36m, dim_rep=DIM_REP, hidden_dim=HIDDEN)
    with pytest.raises(ValueError, match='exclude'):
        MeshRegressor(Backbone(), head, smpl=smpl)
    with pytest.raises(ValueError, match='lambdas'):
        MeshStep(MeshRegressor(Backbone(), head))


# ------------------------------------------------------------------------------------------------ the C entry points' argument checks
@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_argument_errors_are_reported_not_crashed(lib):
    p = C.c_void_p(4096)            # never dereferenced: every check below fails before a launch
    assert lib.mbx_version() >= 110
    assert lib.mbx_rot6d_theta_fwd(None, p, p, 4, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_rot6d_theta_fwd(p, None, None, 4, None) != 0 and b'at least one' in lib.mbx_last_error()
    assert lib.mbx_rot6d_theta_fwd(p, p, p, -1, None) != 0 and b'joint count' in lib.mbx_last_error()
    assert lib.mbx_rot6d_theta_fwd(None, None, None, 0, None) == 0, 'M = 0 is a no-op'
    assert lib.mbx_rot6d_theta_fwd(C.c_void_p(4098), p, p, 4, None) != 0 and b'aligned' in lib.mbx_last_error()
    assert lib.mbx_rot6d_theta_bwd(p, None, None, None, 4, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_rot6d_theta_bwd(p, None, None, p, 4, None) != 0 and b'alias' in lib.mbx_last_error()
    q = C.c_void_p(8192)
    assert lib.mbx_mesh_param_loss(p, p, 2, 1.0, 1.0, 1.0, 1.0, p, None, 4, p, None) != 0 and b'loss_type' in lib.mbx_last_error()
    assert lib.mbx_mesh_param_loss(p, p, 1, 1.0, 1.0, 1.0, 1.0, p, None, 0, p, None) != 0 and b'frame count' in lib.mbx_last_error()
    assert lib.mbx_mesh_param_loss(p, q, 1, 1.0, 1.0, 1.0, 1.0, p, q, 4, p, None) != 0 and b'alias' in lib.mbx_last_error()
    assert lib.mbx_mesh_param_loss(p, None, 1, 1.0, 1.0, 1.0, 1.0, p, None, 4, p, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_mesh_param_loss_ws(0) == 0 and lib.mbx_mesh_param_loss_ws(2048) >= 256 * 3 * 4
    assert lib.mbx_mesh_errors(p, p, None, p, p, 4, 7, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_mesh_errors(p, None, p, p, p, 4, 7, None) != 0 and b'both' in lib.mbx_last_error()
    assert lib.mbx_mesh_errors(p, p, p, p, p, 4, 0, None) != 0 and b'vertex count' in lib.mbx_last_error()
    assert lib.mbx_mesh_errors(p, p, p, p, C.c_void_p(4100), 4, 7, None) != 0 and b'aligned' in lib.mbx_last_error()
    assert lib.mbx_mesh_errors(None, None, None, None, None, 0, 7, None) == 0, 'F = 0 is a no-op'


def test_binding_refuses_wrong_layouts_before_the_library_is_called():
    from motionbert_amd import hip_ops

    class Lib:                      # no symbol may be reached
        pass
    ops = hip_ops.HipOps(lib=Lib())
    x, R, aa = torch.zeros(4, 6), torch.zeros(4, 9), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match=r'x6 \[M,6\]'):
        ops.rot6d_theta_fwd(torch.zeros(4, 5), R, aa)
    with pytest.raises(RuntimeError, match='at least one output'):
        ops.rot6d_theta_fwd(x, None, None)
    with pytest.raises(RuntimeError, match='rotmat must be a contiguous'):
        ops.rot6d_theta_fwd(x, torch.zeros(4, 8), aa)
    with pytest.raises(RuntimeError, match='aa must be a contiguous'):
        ops.rot6d_theta_fwd(x, R, aa.double())
    with pytest.raises(RuntimeError, match='x6 must be a contiguous'):
        ops.rot6d_theta_fwd(torch.zeros(6, 4).T, R, aa)
    with pytest.raises(RuntimeError, match='must not alias'):
        ops.rot6d_theta_bwd(x, R, aa, x)
    with pytest.raises(RuntimeError, match='daa must be a contiguous'):
        ops.rot6d_theta_bwd(x, R, torch.zeros(3, 3), torch.zeros(4, 6))
    th, losses = torch.zeros(3, 82), torch.zeros(4)
    with pytest.raises(RuntimeError, match='mesh_param_loss needs'):
        ops.mesh_param_loss(torch.zeros(3, 72), torch.zeros(3, 72), 1, (1, 1, 1), losses, None)
    with pytest.raises(RuntimeError, match='mesh_param_loss needs'):
        ops.mesh_param_loss(th, th.clone(), 1, (1, 1), losses, None)
    with pytest.raises(RuntimeError, match='loss_type'):
        ops.mesh_param_loss(th, th.clone(), 2, (1, 1, 1), losses, None)
    with pytest.raises(RuntimeError, match='losses must be a contiguous'):
        ops.mesh_param_loss(th, th.clone(), 1, (1, 1, 1), torch.zeros(3), None)
    with pytest.raises(RuntimeError, match='dtheta must be a contiguous'):
        ops.mesh_param_loss(th, th.clone(), 1, (1, 1, 1), losses, torch.zeros(3, 82, dtype=torch.float64))
    kp, err = torch.zeros(3, 17, 3), torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r'kp_p, kp_g \[F,17,3\]'):
        ops.mesh_errors(None, None, torch.zeros(3, 14, 3), torch.zeros(3, 14, 3), err)
    with pytest.raises(RuntimeError, match='both'):
        ops.mesh_errors(torch.zeros(3, 7, 3), None, kp, kp, err)
    with pytest.raises(RuntimeError, match='mesh_errors needs verts'):
        ops.mesh_errors(torch.zeros(2, 7, 3), torch.zeros(2, 7, 3), kp, kp, err)
    with pytest.raises(RuntimeError, match='err must be a contiguous'):
        ops.mesh_errors(None, None, kp, kp, torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match='verts_p must be a contiguous'):
        ops.mesh_errors(torch.zeros(3, 3, 7).transpose(1, 2), torch.zeros(3, 7, 3), kp, kp, err)
