"""The SMPL kernels on a real MI355X (csrc/smpl.hip): mbx_smpl_fwd / mbx_smpl_bwd / mbx_smpl_pack against float64 (tests/smplerr.py: the
restated equations, the plain smplx-style path, inputs, gates; its own checks on the CPU: tests/test_smplerr.py), then SMPLLayer through
autograd, MeshRegressor + MeshLoss, MeshStep and the flip evaluation with the layer in place.

Gate, not a number read off a kernel: per fp32 output array, max |error| / max |float64 value| at most 4 x what the plain path shows in
float32 on the CPU against itself in float64 on the same inputs, never less than 8 fp32 ulps.  Every measured ratio goes to
smpl_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/).

Shapes: the kernels tile 64 vertices; the forward 32 frames per workgroup (8 per wave), the backward 16 (4 per wave) and at most 8 vertex
splits.  CASES has every (F, V) of F in {1, 2, 31, 33, 130} x V in {1, 63, 65, 257} with K in {0, 14, 17} and sparse / dense weights
rotating through them, then the tile edges those leave out (F = 15, 16, 17, 32; V = 64; 8 and 9 vertex tiles) and the real V = 6890.

Measured on the MI355X (profiles/smpl_parity.txt): every ratio below 1; the largest is drot at V = 1 (0.87: every joint sits on the one
vertex and d A_rot - d A_t J^T cancels seven to one), at most 0.42 for V >= 63.  A first run, with the shape and pose offsets added into a
running value of template size, had drot at 1.018 of its gate for F = 31, V = 1: the offsets are summed from zero since (smpl_vposed)."""
import copy
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd.smpl import SMPLLayer, SMPLModel
from tests import mesherr as ME
from tests import smplerr as SE
from tests.helpers import build_model, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64 = torch.float32, torch.float64
REPORT = {}

FS, VS, KS = (1, 2, 31, 33, 130), (1, 63, 65, 257), (0, 14, 17)
CASES = [(F, V, KS[(i + j) % 3], (i + j) % 2 == 1) for i, F in enumerate(FS) for j, V in enumerate(VS)]
CASES += [(15, 64, 17, False), (16, 64, 14, True), (17, 513, 17, False), (32, 512, 14, False), (3, 6890, 17, False)]


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'smpl_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'smpl_parity.txt'), 'w') as f:
        f.write('SMPL kernels against float64: measured statistic / gate per case and output (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + '  '.join(f'{n} {v:.4g}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int64)


def guarded(*shape, dtype=F32, pad=64):
    """a NaN-filled output inside a larger NaN-filled buffer: (the output, a check that nothing around it was written)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), math.nan, dtype=dtype, device=DEV)

    def untouched():
        return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all())
    return buf[pad:pad + n].view(*shape), untouched


def device_model(ops, model):
    md = model.tensors(DEV)
    md['packed_t'] = torch.full((3 * model.V, 224), math.nan, device=DEV)
    ops.smpl_pack(md['shapedirs'], md['posedirs'], md['packed_t'])
    return md


def ratios(tag, got, ref64, gate):
    rep = REPORT.setdefault(tag, {})
    worst = SE.worst_ratio({k: (None if v is None else v.detach().cpu()) for k, v in got.items()}, ref64, gate, rep)
    print(tag, ' '.join(f'{k} {v:.3f}' for k, v in sorted(rep.items())))
    return worst


@pytest.mark.parametrize('F,V,K,dense', CASES)
def test_forward_and_backward_against_float64(ops, F, V, K, dense):
    model = SMPLModel.synthetic(V, 1000 + V, dense)
    inp = SE.inputs(F, V, K, 2000 + 7 * F + V, model)
    scale = 1000.0 if K else 1.0
    md = device_model(ops, model)
    want_pt = torch.cat([model.posedirs.t(), model.shapedirs.reshape(3 * V, 10), torch.zeros(3 * V, 7)], 1)
    assert torch.equal(md['packed_t'].cpu(), want_pt), 'mbx_smpl_pack'
    d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
    rot = d['rot'].reshape(F, 24, 9)
    tag = f'F{F}.V{V}.K{K}.{"dense" if dense else "sparse"}'
    # ---- everything at once, into guarded buffers
    r64, gate = SE.gates(model, inp, scale)
    (verts, okv), (joints, okj), (drot, okr), (db, okb) = guarded(F, V, 3), guarded(F, 24, 3), guarded(F, 24, 9), guarded(F, 10)
    kp, okk = guarded(F, K, 3) if K else (None, lambda: True)
    ops.smpl_fwd(md, d['Q'], d['betas'], rot, scale, verts, kp, joints)
    ops.smpl_bwd(md, d['Q'], d['betas'], rot, scale, d['dverts'], d['dkp'], d['djoints'], drot, db)
    torch.cuda.synchronize()
    assert okv() and okj() and okr() and okb() and okk(), 'a kernel wrote outside its output'
    worst = ratios(tag, dict(verts=verts, kp=kp, joints=joints, drot=drot, dbetas=db), r64, gate)
    # ---- the same bits twice
    v2, j2, dr2, db2 = torch.full_like(verts, math.nan), torch.full_like(joints, math.nan), torch.full_like(drot, math.nan), torch.full_like(db, math.nan)
    k2 = None if kp is None else torch.full_like(kp, math.nan)
    ops.smpl_fwd(md, d['Q'], d['betas'], rot, scale, v2, k2, j2)
    ops.smpl_bwd(md, d['Q'], d['betas'], rot, scale, d['dverts'], d['dkp'], d['djoints'], dr2, db2)
    assert torch.equal(bits(v2), bits(verts)) and torch.equal(bits(j2), bits(joints)) and (kp is None or torch.equal(bits(k2), bits(kp)))
    assert torch.equal(bits(dr2), bits(drot)) and torch.equal(bits(db2), bits(db))
    # ---- each output alone gives the bits of the full call
    for name in ('verts', 'kp', 'joints'):
        if name == 'kp' and not K:
            continue
        out = {n: None for n in ('verts', 'kp', 'joints')}
        out[name], ok = guarded(*dict(verts=(F, V, 3), kp=(F, K, 3), joints=(F, 24, 3))[name])
        ops.smpl_fwd(md, d['Q'], d['betas'], rot, scale, out['verts'], out['kp'], out['joints'])
        torch.cuda.synchronize()
        assert ok() and torch.equal(bits(out[name]), bits(dict(verts=verts, kp=kp, joints=joints)[name])), name
    # ---- one cotangent at a time
    for use in (('dverts',), ('dkp',)):
        if use == ('dkp',) and not K:
            continue
        r1, g1 = SE.gates(model, inp, scale, use)
        dr1, db1 = torch.full_like(drot, math.nan), torch.full_like(db, math.nan)
        ops.smpl_bwd(md, d['Q'], d['betas'], rot, scale, d['dverts'] if use == ('dverts',) else None, d['dkp'] if use == ('dkp',) else None, None, dr1, db1)
        worst = max(worst, ratios(tag + '.' + use[0], dict(drot=dr1, dbetas=db1), r1, {k: g1[k] for k in ('drot', 'dbetas')}))
    assert worst <= 1.0


def test_refusals(ops):
    model = SMPLModel.synthetic(7, 1)
    md = device_model(ops, model)
    b, r = torch.zeros(2, 10, device=DEV), torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(2, 24, 1).contiguous()
    verts, kp = torch.zeros(2, 7, 3, device=DEV), torch.zeros(2, 17, 3, device=DEV)
    Q = model.J_regressor_h36m.to(DEV)
    small = torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match='workspace'):
        ops.smpl_fwd(md, Q, b, r, 1.0, verts, kp, None, ws=small)
    with pytest.raises(RuntimeError, match='workspace'):
        ops.smpl_bwd(md, Q, b, r, 1.0, verts, kp, None, torch.zeros_like(r), torch.zeros_like(b), ws=small)
    bad = list(model.parents)
    bad[9] = 11
    with pytest.raises(RuntimeError, match='forward-ordered'):
        ops.smpl_fwd({**md, 'parents': bad}, Q, b, r, 1.0, verts, kp, None)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.smpl_fwd(md, Q, b, r.cpu(), 1.0, verts, kp, None)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.smpl_fwd(md, Q, b, r, 1.0, verts.transpose(0, 1).contiguous().transpose(0, 1), kp, None)
    # F = 0 is a no-op
    ops.smpl_fwd(md, Q, b[:0], r[:0], 1.0, verts[:0], kp[:0], None)
    ops.smpl_bwd(md, Q, b[:0], r[:0], 1.0, verts[:0], kp[:0], None, torch.zeros_like(r[:0]), torch.zeros_like(b[:0]))
    torch.cuda.synchronize()


def test_layer_through_autograd_against_float64():
    model = SMPLModel.synthetic(257, 55)
    layer = SMPLLayer(model).to(DEV)
    inp = SE.inputs(5, 257, 17, 77, model)
    betas, rot = inp['betas'].to(DEV).requires_grad_(True), inp['rot'].to(DEV).requires_grad_(True)
    out = layer(betas=betas, body_pose=rot[:, 1:], global_orient=rot[:, 0].unsqueeze(1), pose2rot=False)
    assert out.vertices.shape == (5, 257, 3) and out.joints.shape == (5, 24, 3)
    ((out.vertices * inp['dverts'].to(DEV)).sum() + (out.joints * inp['djoints'].to(DEV)).sum()).backward()
    r64, gate = SE.gates(model, {**inp, 'Q': None, 'dkp': None}, 1.0, use=('dverts', 'djoints'))
    worst = ratios('layer.autograd', dict(verts=out.vertices, joints=out.joints, drot=rot.grad, dbetas=betas.grad), r64, gate)
    # forward_kp, scale 1000: the head's call
    betas.grad = rot.grad = None
    verts, kp = layer.forward_kp(betas, rot, scale=1000.0)
    ((verts * inp['dverts'].to(DEV)).sum() + (kp * inp['dkp'].to(DEV)).sum()).backward()
    r64, gate = SE.gates(model, inp, 1000.0, use=('dverts', 'dkp'))
    worst = max(worst, ratios('layer.forward_kp', dict(verts=verts, kp=kp, drot=rot.grad, dbetas=betas.grad), r64,
                              {k: gate[k] for k in ('verts', 'kp', 'drot', 'dbetas')}))
    # pose2rot
    aa = (0.6 * torch.randn(5, 72, generator=torch.Generator().manual_seed(3)))
    o2 = layer(betas=betas.detach(), body_pose=aa[:, 3:].to(DEV), global_orient=aa[:, :3].to(DEV), pose2rot=True)
    plain = SE.PlainSMPL(model)
    p64 = plain(betas=inp['betas'].double(), body_pose=aa.double()[:, 3:], global_orient=aa.double()[:, :3], pose2rot=True)
    p32 = plain(betas=inp['betas'], body_pose=aa[:, 3:], global_orient=aa[:, :3], pose2rot=True)
    worst = max(worst, ratios('layer.pose2rot', dict(verts=o2.vertices, joints=o2.joints), dict(verts=p64.vertices, joints=p64.joints),
                              dict(verts=SE.gate32(SE.stat(p32.vertices, p64.vertices)), joints=SE.gate32(SE.stat(p32.joints, p64.joints)))))
    assert worst <= 1.0
    with pytest.raises(RuntimeError, match='no CPU path'):
        SMPLLayer(model)(betas=inp['betas'], body_pose=inp['rot'][:, 1:], global_orient=inp['rot'][:, :1])


# ------------------------------------------------------------------------------------------------ end to end
CFG = dict(dim_in=3, dim_out=3, dim_feat=128, dim_rep=128, depth=2, num_heads=4, mlp_ratio=4, num_joints=17, maxlen=243)
HIDDEN, V = 256, 65
MODEL = SMPLModel.synthetic(V, 91)


def mesh_net(seed=31):
    from motionbert_amd.mesh import MeshRegressor
    torch.manual_seed(seed)
    smpl = SMPLLayer(MODEL)
    pose, shape = ME.mean_params()
    net = MeshRegressor(build_model(CFG), smpl=smpl, init_pose=pose, init_shape=shape, J_regressor=smpl.J_regressor_h36m, dim_rep=128,
                        hidden_dim=HIDDEN, dropout_ratio=0.).to(DEV)
    net.backbone.precision = 'fp32'
    return net


def clips(n, T, seed):
    return torch.stack([make_input(1, T, 17, seed + i)[0] for i in range(n)]).to(DEV)


def targets(N, T, seed):
    return {k: v.to(DEV) for k, v in ME.mesh_targets(N, T, V, seed).items()}


def test_head_and_loss_gradients_match_the_float64_plain_path():
    """test_gpu_mesh.py's end-to-end rule: a parameter gradient may be 4 x as far from the float64 plain path as the float32 plain path is"""
    from motionbert_amd.mesh import MeshLoss
    from tests.test_gpu_mesh import restated_total
    net = mesh_net().train()
    N, T = 2, 3
    x, tgt = clips(N, T, 300), targets(N, T, 41)
    with torch.no_grad():
        out0 = net(x)[0]
        tgt['theta'] = out0['theta'] + 0.1 * torch.randn_like(out0['theta'])
        tgt['kp_3d'] = out0['kp_3d'] + 20.0 * torch.randn_like(out0['kp_3d'])
        feat = net.backbone.get_representation(x).reshape(N, T, 17, -1)
    grads = {}
    for d in (F32, F64):
        h = copy.deepcopy(net.head).to(d)
        h.smpl = SE.PlainSMPL(MODEL)
        h.J_regressor = h.J_regressor.to(device=DEV, dtype=d)
        o = ME.plain_head_forward(h, feat.to(d))[0]
        restated_total(o, tgt, ME.Lambdas, 'L1').backward()
        grads[d] = {n: p.grad.double() for n, p in h.named_parameters()}
    flat = net.head(feat)[0]
    losses = MeshLoss(loss_type='L1', lambdas=ME.Lambdas)([{k: v.reshape(N, T, *v.shape[1:]) for k, v in flat.items()}], tgt)
    losses['total'].backward()
    worst = 0.0
    for n in ('head_pose.weight', 'head_pose.bias', 'fc1.weight', 'head_shape.weight'):
        gate = ME.gate32(ME.stat(grads[F32][n], grads[F64][n]))
        s = ME.stat(dict(net.head.named_parameters())[n].grad, grads[F64][n])
        print(f'e2e.grad {n}: stat {s:.3e} gate {gate:.3e}')
        REPORT.setdefault('e2e.grad', {})[n] = s / gate
        worst = max(worst, s / gate)
    assert worst <= 1.0


def test_mesh_step_eager_and_captured_give_the_same_bits_over_three_steps():
    from motionbert_amd.mesh import LOG_KEYS, MeshStep
    from tests.test_gpu_mesh import restore, snapshot
    N, T = 2, 3
    x, tgt = clips(N, T, 400), targets(N, T, 43)
    eager, graphed = [MeshStep(mesh_net(seed=33).train(), lr_backbone=1e-4, lr_head=1e-3, weight_decay=0.01, lambdas=ME.Lambdas, loss_type='L1')
                      for _ in range(2)]
    logs_e = [eager(x, tgt).clone() for _ in range(3)]
    assert logs_e[0].shape == (len(LOG_KEYS),) and bool(torch.isfinite(torch.stack(logs_e)).all()) and not torch.equal(logs_e[0], logs_e[2])
    snap = snapshot(graphed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed(x, tgt)                       # warm-up: the layer's workspaces and packed table exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore(graphed, snap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log_g = graphed(x, tgt)
    torch.cuda.synchronize()
    restore(graphed, snap)
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(log_g), bits(logs_e[i])), (i, log_g.tolist(), logs_e[i].tolist())
    for (k, a), b in zip(eager.model.state_dict().items(), graphed.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_flip_average_into_the_evaluator_against_float64():
    from motionbert_amd.mesh import MeshEvaluator, flip_average, flip_input, flip_thetas_batch
    net = mesh_net(seed=35).eval()
    N, T = 3, 3
    x, tgt = clips(N, T, 500), targets(N, T, 45)
    got = flip_average(net, net.head.smpl, x)
    with torch.no_grad():
        out, fl = net(x)[0], net(flip_input(x))[0]
    pose = flip_thetas_batch(fl['theta'][:, :, :72]).double().cpu().reshape(-1, 72)
    shape = fl['theta'][:, :, 72:].double().cpu().reshape(-1, 10)
    plain = SE.PlainSMPL(MODEL)
    v64 = plain(betas=shape, body_pose=pose[:, 3:], global_orient=pose[:, :3], pose2rot=True).vertices * 1000.0
    v32 = plain(betas=shape.float(), body_pose=pose.float()[:, 3:], global_orient=pose.float()[:, :3], pose2rot=True).vertices * 1000.0
    kp64 = MODEL.J_regressor_h36m.double() @ v64
    want_v = (out['verts'].double().cpu() + v64.reshape(N, T, V, 3)) * 0.5
    want_k = (out['kp_3d'].double().cpu() + kp64.reshape(N, T, 17, 3)) * 0.5
    gate = SE.gate32(SE.stat(v32, v64))
    worst = max(ratios('flip.average', dict(verts=got[0]['verts'], kp=got[0]['kp_3d']), dict(verts=want_v, kp=want_k), dict(verts=gate, kp=gate)), 0.0)
    assert worst <= 1.0
    ev = MeshEvaluator()
    ev.update(got, tgt)
    res = ev.finish()
    ref = ME.aggregate(ME.mesh_errors64(want_v.reshape(-1, V, 3).numpy(), tgt['verts'].reshape(-1, V, 3).cpu().numpy(),
                                        want_k.reshape(-1, 17, 3).numpy(), tgt['kp_3d'].reshape(-1, 17, 3).cpu().numpy()))
    # a vertex or joint moves by at most gate x max |value| (above); a mean of distances then moves by at most sqrt(3) times that, the
    # aligned ones by a small multiple of it (the similarity fit is smooth in the 17 joints): 4 x as the margin
    tol = 4.0 * math.sqrt(3.0) * gate * float(want_v.abs().max())
    for k in ref:
        print(f'flip.evaluator {k}: {res[k]:.6f} against {ref[k]:.6f} (tolerance {tol:.2e})')
        assert abs(res[k] - ref[k]) <= tol, k
