"""The mesh-recovery kernels on a real MI355X (csrc/mesh.hip): mbx_rot6d_theta_fwd / _bwd, mbx_mesh_param_loss and mbx_mesh_errors against
float64 (tests/mesherr.py: restatements pinned to the reference by tests/golden/mesh.npz, inputs, gates; its own checks on the CPU:
tests/test_mesherr.py), then MeshRegressor + MeshLoss, MeshStep and MeshEvaluator end to end.

Gates, none of them a number read off a kernel.  fp32 kernels: max |error| / max |float64 value| per output array at most 4 x what the
reference's own code shows in float32 on the CPU against itself in float64 (the `.ref32` entries of the fixture), never less than 8 fp32
ulps.  fp64 kernel: 1e-10 relative per frame and per aggregate.  Every measured ratio goes to mesh_parity.json / .txt in the directory
MBX_REPORT_DIR names (default reports/).

Measured on the MI355X (profiles/mesh_parity.txt): see that file; every ratio below 1."""
import copy
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from tests import mesherr as ME
from tests.helpers import build_model, load_golden, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64 = torch.float32, torch.float64
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'mesh_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'mesh_parity.txt'), 'w') as f:
        f.write('mesh kernels against float64: measured statistic / gate per case and output (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + '  '.join(f'{n} {v:.4g}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


@pytest.fixture(scope='module')
def fx():
    return load_golden('mesh')[0]


def bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int64)


def guarded(*shape, dtype=F32, pad=64):
    """a NaN-filled output inside a larger NaN-filled buffer: (the output, a check that nothing around it was written)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), math.nan, dtype=dtype, device=DEV)

    def untouched():
        return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all())
    return buf[pad:pad + n].view(*shape), untouched


def ratio(tag, name, got, ref64, gate):
    s = ME.stat(got, ref64)
    r = s / gate
    print(f'{tag} {name}: stat {s:.3e} gate {gate:.3e} ratio {r:.4f}')
    REPORT.setdefault(tag, {})[name] = r
    return r


# ------------------------------------------------------------------------------------------------ rotation chain
@pytest.mark.parametrize('M', ME.ROT_M)
def test_rotation_chain_against_float64_and_the_fixture(ops, fx, M):
    x6, drot, daa = ME.rot_inputs(M, ME.rot_seed(M))
    ref = ME.rot_chain_grad(x6, drot, daa, F64)
    rows = fx[f'rot.{M}.rows']
    for name, r in zip(('rotmat', 'aa', 'dx6'), ref):
        assert ME.stat(r[rows], fx[f'rot.{M}.{name}']) <= 1e-12, name
    x, dr, da = x6.to(DEV), drot.to(DEV), daa.to(DEV)
    (R, okR), (aa, oka), (dx, okd) = guarded(M, 9), guarded(M, 3), guarded(M, 6)
    ops.rot6d_theta_fwd(x, R, aa)
    ops.rot6d_theta_bwd(x, dr, da, dx)
    torch.cuda.synchronize()
    assert okR() and oka() and okd(), 'a kernel wrote outside its output'
    worst = max(ratio(f'rot.{M}', n, g, r, ME.gate32(fx[f'rot.{M}.{n}.ref32'])) for n, g, r in zip(('rotmat', 'aa', 'dx6'), (R, aa, dx), ref))
    # either output and either cotangent may be NULL; two calls give the same bits
    R2, aa2, dx2 = torch.full_like(R, math.nan), torch.full_like(aa, math.nan), torch.full_like(dx, math.nan)
    ops.rot6d_theta_fwd(x, R2, None)
    ops.rot6d_theta_fwd(x, None, aa2)
    ops.rot6d_theta_bwd(x, dr, da, dx2)
    assert torch.equal(bits(R2), bits(R)) and torch.equal(bits(aa2), bits(aa)) and torch.equal(bits(dx2), bits(dx))
    d_r, d_a = torch.full_like(dx, math.nan), torch.full_like(dx, math.nan)
    ops.rot6d_theta_bwd(x, dr, None, d_r)
    ops.rot6d_theta_bwd(x, None, da, d_a)
    zero = torch.zeros_like(drot)
    only_r = ME.rot_chain_grad(x6, drot, torch.zeros_like(daa), F64)[2]
    only_a = ME.rot_chain_grad(x6, zero, daa, F64)[2]
    g = ME.gate32(fx[f'rot.{M}.dx6.ref32'])
    worst = max(worst, ratio(f'rot.{M}', 'dx6_rotmat_only', d_r, only_r, g), ratio(f'rot.{M}', 'dx6_aa_only', d_a, only_a, g))
    assert worst <= 1.0


def planted_rows():
    c = 1e-6
    return torch.tensor([[1, 0, 0, 1, 0, 0],            # identity
                         [0, 0, 0, 0, 0, 0],            # all zero: both normalisations clamp, R = 0
                         [1, 0, 0, -1, 0, 0],           # pi about x
                         [-1, 0, 0, 1, 0, 0],           # pi about y
                         [-1, 0, 0, -1, 0, 0],          # pi about z
                         [1, 0, 0, 2 * c, 0, 1],        # about x, R[2,2] = 2e-6: above the mask's eps
                         [1, 0, 0, 0.5 * c, 0, 1],      # R[2,2] = 5e-7: below it
                         [1, 0, 0, -c, 0, 1]], dtype=F32)


def test_rotation_chain_planted_rows(ops):
    x6 = planted_rows()
    R64, aa64 = ME.rot_chain(x6.double())
    case = ME.rot_cases(R64.transpose(1, 2)).tolist()
    assert case == [3, 1, 0, 1, 2, 3, 0, 0], case          # the planted rows reach every mask case, on both sides of eps
    x = x6.to(DEV)
    R, aa = torch.full((8, 9), math.nan, device=DEV), torch.full((8, 3), math.nan, device=DEV)
    ops.rot6d_theta_fwd(x, R, aa)
    aa, R = aa.cpu(), R.cpu()
    pi = float(np.float32(math.pi))
    print(aa)
    assert torch.equal(aa[0], torch.zeros(3)) and torch.equal(R[0], torch.eye(3).reshape(9))
    assert torch.equal(R[1], torch.zeros(9)) and aa[1].tolist() == [0.0, pi, 0.0]
    assert aa[2].tolist() == [pi, 0.0, 0.0] and aa[3].tolist() == [0.0, pi, 0.0] and aa[4].tolist() == [0.0, 0.0, pi]
    assert ME.stat(aa[5:], aa64[5:]) <= ME.FLOOR and ME.stat(R, R64.reshape(8, 9)) <= ME.FLOOR


def test_rotation_chain_gradient_at_the_identity_is_finite(ops):
    x6 = planted_rows()[:1].repeat(5, 1)
    x6[1:] += 0.25 * torch.randn(4, 6, generator=torch.Generator().manual_seed(5))           # identity, then ordinary rows around it
    drot, daa = torch.randn(5, 9, generator=torch.Generator().manual_seed(6)), torch.randn(5, 3, generator=torch.Generator().manual_seed(7))
    want = ME.rot_chain_grad(x6, drot, daa, F64)[2]           # rot_chain takes k = 2 at sin^2 == 0: d aa = 2 d q_xyz, pulled back
    assert bool(torch.isfinite(want).all()) and float(want[0].abs().max()) > 0
    dx = torch.full((5, 6), math.nan, device=DEV)
    ops.rot6d_theta_bwd(x6.to(DEV), drot.to(DEV), daa.to(DEV), dx)
    assert bool(torch.isfinite(dx).all())
    assert ratio('rot.identity', 'dx6', dx, want, ME.FLOOR) <= 1.0


def test_rot6d_function_differentiates_through_either_output(ops, fx):
    from motionbert_amd.mesh import rot6d_to_rotmat_theta
    x6, drot, daa = ME.rot_inputs(72, ME.rot_seed(72))
    x = x6.to(DEV).requires_grad_(True)
    R, aa = rot6d_to_rotmat_theta(x.reshape(3, 144))
    assert R.shape == (72, 3, 3) and aa.shape == (72, 3)
    (aa * daa.to(DEV)).sum().backward()
    want = ME.rot_chain_grad(x6, torch.zeros_like(drot), daa, F64)[2]
    assert ratio('rot.function', 'dx6_aa_only', x.grad, want, ME.gate32(fx['rot.72.dx6.ref32'])) <= 1.0


# ------------------------------------------------------------------------------------------------ parameter losses
@pytest.mark.parametrize('F', ME.LOSS_F)
@pytest.mark.parametrize('t', (0, 1))
def test_parameter_losses_against_float64_and_the_fixture(ops, fx, F, t):
    pred, gt = ME.theta_inputs(F, ME.loss_seed(F))
    rl, rd = ME.param_loss_grad(pred, gt, t, ME.LAMBDAS3, F64)
    assert float(((rl - torch.from_numpy(fx[f'loss.{F}.t{t}.losses'])).abs() / rl.abs()).max()) <= 1e-12
    assert ME.stat(rd[fx[f'loss.{F}.rows']], fx[f'loss.{F}.t{t}.dtheta']) <= 1e-12
    p, g = pred.to(DEV), gt.to(DEV)
    (losses, okl), (d, okd) = guarded(4), guarded(F, 82)
    ops.mesh_param_loss(p, g, t, ME.LAMBDAS3, losses, d)
    torch.cuda.synchronize()
    assert okl() and okd(), 'a kernel wrote outside its output'
    tag = f'loss.{F}.t{t}'
    worst = 0.0
    for i, n in enumerate(('loss_pose', 'loss_shape', 'loss_norm')):
        worst = max(worst, ratio(tag, n, losses[i:i + 1], rl[i:i + 1], ME.gate32(fx[f'{tag}.losses.ref32'][i])))
    total = sum(float(np.float32(l)) * v for l, v in zip(ME.LAMBDAS3, rl))
    worst = max(worst, ratio(tag, 'total', losses[3:4], total.reshape(1), ME.gate32(float(fx[f'{tag}.losses.ref32'].max()))))
    worst = max(worst, ratio(tag, 'dtheta', d, rd, ME.gate32(fx[f'{tag}.dtheta.ref32'])))
    # without dtheta: the same loss bits; a second call: the same bits; grad_scale scales
    l2, d2, d3 = torch.full_like(losses, math.nan), torch.full_like(d, math.nan), torch.full_like(d, math.nan)
    ops.mesh_param_loss(p, g, t, ME.LAMBDAS3, l2, None)
    assert torch.equal(bits(l2), bits(losses))
    ops.mesh_param_loss(p, g, t, ME.LAMBDAS3, l2, d2)
    assert torch.equal(bits(l2), bits(losses)) and torch.equal(bits(d2), bits(d))
    ops.mesh_param_loss(p, g, t, ME.LAMBDAS3, l2, d3, grad_scale=4.0)
    assert torch.equal(bits(d3), bits(d * 4.0))
    if F >= 3:
        # row 1 of the target is the prediction: pose and shape differences are exactly 0, and so is their (sub)gradient
        ops.mesh_param_loss(p, g, t, (1.0, 1.0, 0.0), l2, d2)
        assert float(d2[1].abs().max()) == 0.0 and float(d2[0].abs().max()) > 0.0
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ mesh errors
@pytest.mark.parametrize('case', ME.ERR_CASES)
def test_mesh_errors_against_float64_and_the_fixture(ops, fx, case):
    F, V = case
    vp, vg, kp, kg = ME.err_inputs(F, V, ME.err_seed(case))
    ref = ME.mesh_errors64(vp.numpy(), vg.numpy(), kp.numpy(), kg.numpy())
    if V == 6890:
        assert ME.err_ratio(ref, fx['err.%d.%d.rows' % case]) <= 1e-12 / ME.GATE64
    dvp, dvg, dkp, dkg = vp.to(DEV), vg.to(DEV), kp.to(DEV), kg.to(DEV)
    err, ok = guarded(5, F, dtype=F64)
    ops.mesh_errors(dvp, dvg, dkp, dkg, err)
    torch.cuda.synchronize()
    assert ok(), 'the kernel wrote outside its output'
    got = err.cpu().numpy()
    tag = 'err.%d.%d' % case
    r_frames = ME.err_ratio(got, ref)
    agg, ragg = ME.aggregate(got), ME.aggregate(ref)
    r_agg = ME.err_ratio([agg[k] for k in ME.ERR_ROWS], [ragg[k] for k in ME.ERR_ROWS])
    if V == 6890:
        r_agg = max(r_agg, ME.err_ratio([agg[k] for k in ME.ERR_ROWS], fx['err.%d.%d.dict' % case]))
    print(f'{tag}: per frame error / gate {r_frames:.3e}, aggregates {r_agg:.3e}')
    REPORT[tag] = dict(frames=r_frames, aggregates=r_agg)
    if case in ME.PLANTED:
        same, mirror, flat = ME.PLANTED[case]
        assert np.all(got[:3, same] == 0.0) and np.all(got[3:, same] < 1e-10), 'prediction equal to its target'
        assert np.isnan(got[3:, flat]).all() and int(np.isnan(got).sum()) == 2, 'NaN exactly where the reference has it'
        assert np.all(got[3:, mirror] > 1.0), 'a mirrored pose cannot be aligned by a rotation'
    # the same bits twice; without vertices the MPVE row is NaN and the joint rows keep their bits
    e2, e3 = torch.full_like(err, math.nan), torch.full_like(err, math.nan)
    ops.mesh_errors(dvp, dvg, dkp, dkg, e2)
    ops.mesh_errors(None, None, dkp, dkg, e3)
    assert torch.equal(bits(e2), bits(err))
    assert bool(torch.isnan(e3[0]).all()) and torch.equal(bits(e3[1:]), bits(err[1:]))
    assert r_frames <= 1.0 and r_agg <= 1.0


def test_mesh_errors_on_a_batch_cut_out_of_a_larger_buffer(ops):
    """frames 1 .. 3 of a buffer: at V = 7 frame bases are 84 bytes apart, 4-byte aligned only"""
    case = (5, 7)
    vp, vg, kp, kg = [a.to(DEV) for a in ME.err_inputs(*case, 77)]
    whole, part = torch.empty(5, 5, dtype=F64, device=DEV), torch.empty(5, 3, dtype=F64, device=DEV)
    ops.mesh_errors(vp, vg, kp, kg, whole)
    ops.mesh_errors(vp[1:4], vg[1:4], kp[1:4], kg[1:4], part)
    assert vp[1:4].data_ptr() % 8 != 0 and torch.equal(bits(part), bits(whole[:, 1:4].contiguous()))


# ------------------------------------------------------------------------------------------------ end to end
CFG = dict(dim_in=3, dim_out=3, dim_feat=128, dim_rep=128, depth=2, num_heads=4, mlp_ratio=4, num_joints=17, maxlen=243)
HIDDEN, V = 256, 64


def mesh_net(seed=31):
    from motionbert_amd.mesh import MeshRegressor
    torch.manual_seed(seed)
    smpl = ME.StandInSMPL(V)
    pose, shape = ME.mean_params()
    net = MeshRegressor(build_model(CFG), smpl=smpl, init_pose=pose, init_shape=shape, J_regressor=smpl.J_regressor_h36m, dim_rep=128,
                        hidden_dim=HIDDEN, dropout_ratio=0.).to(DEV)
    net.backbone.precision = 'fp32'
    return net


def clips(n, T, seed):
    return torch.stack([make_input(1, T, 17, seed + i)[0] for i in range(n)]).to(DEV)           # [n, T, 17, 3]


def targets(N, T, seed):
    return {k: v.to(DEV) for k, v in ME.mesh_targets(N, T, V, seed).items()}


def restated_total(out, tgt, lam, loss_type):
    """train_mesh.py:180-189 on an output dict, in plain torch operations and the dtype of the output"""
    from motionbert_amd.mesh import LAMBDA_NAMES
    from tests import limberr
    kp, gk = out['kp_3d'], tgt['kp_3d'].to(out['kp_3d'].dtype)
    seven = limberr.terms64(kp - kp[:, :, :1], gk - gk[:, :, :1])
    lp, ls, ln = ME.param_losses(out['theta'].reshape(-1, 82), tgt['theta'].to(kp.dtype).reshape(-1, 82), ('MSE', 'L1').index(loss_type))
    return sum(float(getattr(lam, n)) * v for n, v in zip(LAMBDA_NAMES, seven + [ls, lp, ln]))


def test_head_and_loss_gradients_match_the_plain_torch_head():
    from motionbert_amd.mesh import MeshLoss
    net = mesh_net().train()
    N, T = 2, 6
    x, tgt = clips(N, T, 300), targets(N, T, 41)
    with torch.no_grad():
        out0 = net(x)[0]
        tgt['theta'] = out0['theta'] + 0.1 * torch.randn_like(out0['theta'])             # targets near the prediction, as in training
        tgt['kp_3d'] = out0['kp_3d'] + 20.0 * torch.randn_like(out0['kp_3d'])
        feat = net.backbone.get_representation(x).reshape(N, T, 17, -1)
    heads = {d: copy.deepcopy(net.head).to(d) for d in (F32, F64)}
    for h in heads.values():
        h.J_regressor = h.J_regressor.to(DEV)
    grads = {}
    for d, h in heads.items():
        o = ME.plain_head_forward(h, feat.to(d))[0]
        restated_total(o, tgt, ME.Lambdas, 'L1').backward()
        grads[d] = {n: p.grad.double() for n, p in h.named_parameters()}
    flat = net.head(feat)[0]
    losses = MeshLoss(loss_type='L1', lambdas=ME.Lambdas)([{k: v.reshape(N, T, *v.shape[1:]) for k, v in flat.items()}], tgt)
    losses['total'].backward()
    worst = 0.0
    for n in ('head_pose.weight', 'head_pose.bias', 'fc1.weight', 'head_shape.weight'):
        gate = ME.gate32(ME.stat(grads[F32][n], grads[F64][n]))
        worst = max(worst, ratio('e2e.grad', n, dict(net.head.named_parameters())[n].grad, grads[F64][n], gate))
    assert worst <= 1.0


def snapshot(step):
    keep = {k: v.clone() for k, v in step.model.state_dict().items()}
    opts = [(o.flat.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.state_t.clone()) for o in (step.opt_backbone, step.opt_head)]
    return keep, opts


def restore(step, snap):
    keep, opts = snap
    with torch.no_grad():
        for k, v in step.model.state_dict().items():
            v.copy_(keep[k])
        for o, (a, b, c, d) in zip((step.opt_backbone, step.opt_head), opts):
            o.flat.copy_(a); o.exp_avg.copy_(b); o.exp_avg_sq.copy_(c); o.state_t.copy_(d)


def test_mesh_step_eager_and_captured_give_the_same_bits():
    from motionbert_amd.mesh import LOG_KEYS, MeshStep
    N, T = 2, 6
    x, tgt = clips(N, T, 400), targets(N, T, 43)
    steps = [MeshStep(mesh_net(seed=33).train(), lr_backbone=1e-4, lr_head=1e-3, weight_decay=0.01, lambdas=ME.Lambdas, loss_type='L1')
             for _ in range(2)]
    eager, graphed = steps
    for a, b in zip(eager.model.state_dict().values(), graphed.model.state_dict().values()):
        assert torch.equal(a, b)
    first = eager.model.head.fc1.weight.detach().clone()
    log_e = eager(x, tgt)
    assert log_e.shape == (len(LOG_KEYS),) and log_e.is_cuda and not log_e.requires_grad and bool(torch.isfinite(log_e).all())
    assert not torch.equal(first, eager.model.head.fc1.weight), 'the step moved the head'
    # warm-up on a side stream without touching the training state, then one captured step, replayed once
    snap = snapshot(graphed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed(x, tgt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore(graphed, snap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log_g = graphed(x, tgt)
    torch.cuda.synchronize()
    restore(graphed, snap)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(log_g), bits(log_e)), (log_g.tolist(), log_e.tolist())
    for (k, a), b in zip(eager.model.state_dict().items(), graphed.model.state_dict().values()):
        assert torch.equal(a, b), k
    lr = (eager.opt_backbone.lr, eager.opt_head.lr)
    eager.decay(0.5)
    assert (eager.opt_backbone.lr, eager.opt_head.lr) == (lr[0] * 0.5, lr[1] * 0.5)


def test_mesh_evaluator_over_three_batches_equals_one_call():
    from motionbert_amd.mesh import MeshEvaluator, compute_error
    net = mesh_net(seed=35).eval()
    N, T = 7, 3
    x, tgt = clips(N, T, 500), targets(N, T, 45)
    with torch.no_grad():
        out = net(x)
    ev = MeshEvaluator()
    for lo, hi in ((0, 2), (2, 3), (3, 7)):
        ev.update([{k: v[lo:hi] for k, v in out[0].items()}], {k: v[lo:hi] for k, v in tgt.items()})
    one = MeshEvaluator()
    whole = one.update(out, tgt)
    assert ev.count == N * T and torch.equal(bits(ev.frames()), bits(whole))
    got, ref = ev.finish(), one.finish()
    assert got == ref and tuple(got) == ('mpve', 'mpjpe', 'pa_mpjpe', 'mpjpe_17j', 'pa_mpjpe_17j')
    want = ME.aggregate(ME.mesh_errors64(out[0]['verts'].reshape(-1, V, 3).cpu().numpy(), tgt['verts'].reshape(-1, V, 3).cpu().numpy(),
                                         out[0]['kp_3d'].reshape(-1, 17, 3).cpu().numpy(), tgt['kp_3d'].reshape(-1, 17, 3).cpu().numpy()))
    r = ME.err_ratio([got[k] for k in ME.ERR_ROWS], [want[k] for k in ME.ERR_ROWS])
    REPORT['e2e.evaluator'] = dict(aggregates=r)
    assert r <= 1.0
    mpjpe, mpve = compute_error(out, tgt)
    assert mpjpe.is_cuda and float(mpjpe) == pytest.approx(want['mpjpe_17j'], rel=1e-10) and float(mpve) == pytest.approx(want['mpve'], rel=1e-10)
