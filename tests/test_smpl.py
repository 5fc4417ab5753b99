"""motionbert_amd.smpl and the SMPL parts of motionbert_amd.mesh on the CPU with the fp32 mock of the kernels injected through `ops=`
(tests/smplerr.MockOps): constructors, call signature, shapes, bookkeeping, the flip evaluation and the refusals.  The kernels themselves:
tests/test_gpu_smpl.py."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from motionbert_amd.smpl import SMPL_PARENTS, SMPLLayer, SMPLModel
from tests import mesherr as ME
from tests import smplerr as SE
from tests.helpers import load_golden
from tests.test_mesh import Backbone, DIM_REP, HIDDEN

F32, F64 = torch.float32, torch.float64
V = 65


# ------------------------------------------------------------------------------------------------ SMPLModel
def test_synthetic_model_is_a_valid_body_model():
    for dense in (False, True):
        m = SMPLModel.synthetic(V, 3, dense_weights=dense)
        assert m.V == V and m.parents == SMPL_PARENTS and m.parents[0] == -1
        assert m.v_template.shape == (V, 3) and m.shapedirs.shape == (V, 3, 10) and m.posedirs.shape == (207, 3 * V)
        assert m.J_regressor.shape == (24, V) and m.lbs_weights.shape == (V, 24) and m.J_regressor_h36m.shape == (17, V)
        assert m.Jt.shape == (24, 3) and m.Jd.shape == (24, 3, 10) and all(t.dtype == F32 for t in (m.v_template, m.Jt, m.Jd, m.lbs_weights))
        nz = (m.lbs_weights != 0).sum(1)
        assert int(nz.max()) <= (24 if dense else 4) and (dense or int(nz.min()) >= 1)
        assert float((m.lbs_weights.double().sum(1) - 1).abs().max()) <= 1e-6 and float(m.lbs_weights.min()) >= 0
        assert float((m.J_regressor.double().sum(1) - 1).abs().max()) <= 1e-6 and float(m.J_regressor.min()) >= 0
        assert SE.stat(m.Jt, m.J_regressor.double() @ m.v_template.double()) <= 2.0 ** -23
    assert torch.equal(SMPLModel.synthetic(V, 3).posedirs, SMPLModel.synthetic(V, 3).posedirs)
    assert not torch.equal(SMPLModel.synthetic(V, 3).posedirs, SMPLModel.synthetic(V, 4).posedirs)


def test_npz_and_module_constructors_round_trip(tmp_path):
    m = SMPLModel.synthetic(V, 5)
    path = str(tmp_path / 'model.npz')
    m.to_npz(path)
    a = SMPLModel.from_npz(path)
    layer = SMPLLayer(m)
    b = SMPLModel.from_module(layer)                                    # duck-typed: the layer has smplx's attribute names
    for other in (a, b):
        for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'lbs_weights', 'Jt', 'Jd', 'J_regressor_h36m'):
            assert torch.equal(getattr(other, k), getattr(m, k)), k
        assert other.parents == m.parents
    # the layout of the model files: posedirs [V,3,207], 300 shape components, kintree_table with 2^32 - 1 for the root, `weights`
    files = dict(v_template=m.v_template.numpy(), shapedirs=np.concatenate([m.shapedirs.numpy(), np.ones((V, 3, 290), np.float32)], 2),
                 posedirs=m.posedirs.numpy().T.reshape(V, 3, 207), J_regressor=m.J_regressor.numpy(), weights=m.lbs_weights.numpy(),
                 kintree_table=np.stack([np.asarray((2 ** 32 - 1,) + m.parents[1:], np.int64), np.arange(24)]))
    np.savez(str(tmp_path / 'files.npz'), **files)
    c = SMPLModel.from_npz(str(tmp_path / 'files.npz'))
    assert torch.equal(c.posedirs, m.posedirs) and torch.equal(c.shapedirs, m.shapedirs) and c.parents == m.parents and c.J_regressor_h36m is None


def test_model_refusals(tmp_path):
    m = SMPLModel.synthetic(7, 1)
    args = dict(v_template=m.v_template, shapedirs=m.shapedirs, posedirs=m.posedirs, J_regressor=m.J_regressor, parents=m.parents,
                lbs_weights=m.lbs_weights, J_regressor_h36m=m.J_regressor_h36m)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            SMPLModel(**{**args, **kw})
    bad('v_template', v_template=torch.zeros(0, 3))
    bad('v_template', v_template=torch.zeros(7, 2))
    bad('shapedirs', shapedirs=torch.zeros(7, 3, 9))
    bad('posedirs', posedirs=torch.zeros(206, 21))
    bad('J_regressor needs', J_regressor=torch.zeros(23, 7))
    bad('lbs_weights', lbs_weights=torch.zeros(24, 7))
    bad('24 entries', parents=m.parents[:23])
    bad('forward-ordered', parents=m.parents[:5] + (7,) + m.parents[6:])
    bad('forward-ordered', parents=m.parents[:5] + (5,) + m.parents[6:])
    bad('J_regressor_h36m', J_regressor_h36m=torch.zeros(33, 7))
    bad('J_regressor_h36m', J_regressor_h36m=torch.zeros(17, 6))
    bad('non-finite', v_template=torch.full((7, 3), float('nan')))
    np.savez(str(tmp_path / 'short.npz'), v_template=m.v_template.numpy())
    with pytest.raises(ValueError, match='missing'):
        SMPLModel.from_npz(str(tmp_path / 'short.npz'))
    with pytest.raises(ValueError, match='has no'):
        SMPLModel.from_module(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError, match='SMPLModel'):
        SMPLLayer(torch.nn.Linear(2, 2))


# ------------------------------------------------------------------------------------------------ SMPLLayer
def test_layer_call_signature_shapes_and_gradients():
    m = SMPLModel.synthetic(V, 7)
    ops = SE.MockOps()
    layer = SMPLLayer(m, ops=ops)
    inp = SE.inputs(3, V, 0, 17)
    betas, rot = inp['betas'].clone().requires_grad_(True), inp['rot'].clone().requires_grad_(True)
    out = layer(betas=betas, body_pose=rot[:, 1:], global_orient=rot[:, 0].unsqueeze(1), pose2rot=False)
    assert out.vertices.shape == (3, V, 3) and out.joints.shape == (3, 24, 3) and out.vertices.requires_grad
    ((out.vertices * inp['dverts']).sum() + (out.joints * inp['djoints']).sum()).backward()
    r64, gate = SE.gates(m, inp, 1.0, use=('dverts', 'djoints'))
    got = dict(verts=out.vertices.detach(), joints=out.joints.detach(), drot=rot.grad, dbetas=betas.grad)
    assert SE.worst_ratio(got, r64, gate) <= 1.0
    assert ops.calls == {'smpl_fwd': 1, 'smpl_pack': 1, 'smpl_bwd': 1}
    layer(betas=betas, body_pose=rot[:, 1:], global_orient=rot[:, :1]).vertices.sum().backward()
    assert ops.calls == {'smpl_fwd': 2, 'smpl_pack': 1, 'smpl_bwd': 2}, 'the packed table is built once'
    with pytest.raises(ValueError, match='betas'):
        layer(betas=betas[:, :9], body_pose=rot[:, 1:], global_orient=rot[:, :1])
    with pytest.raises(ValueError, match='24 rotation matrices'):
        layer(betas=betas, body_pose=rot[:, 2:], global_orient=rot[:, :1])
    with pytest.raises(RuntimeError, match='no CPU path'):
        SMPLLayer(m)(betas=betas, body_pose=rot[:, 1:], global_orient=rot[:, :1])
    empty = layer(betas=betas[:0], body_pose=rot[:0, 1:], global_orient=rot[:0, :1])
    assert empty.vertices.shape == (0, V, 3) and empty.joints.shape == (0, 24, 3)


def test_layer_pose2rot_takes_axis_angle():
    m = SMPLModel.synthetic(V, 7)
    layer = SMPLLayer(m, ops=SE.MockOps())
    g = torch.Generator().manual_seed(2)
    aa = (0.6 * torch.randn(2, 72, generator=g)).requires_grad_(True)
    betas = torch.randn(2, 10, generator=g)
    out = layer(betas=betas, body_pose=aa[:, 3:], global_orient=aa[:, :3], pose2rot=True)
    ref = SE.PlainSMPL(m)(betas=betas.double(), body_pose=aa.detach().double()[:, 3:], global_orient=aa.detach().double()[:, :3], pose2rot=True)
    ref32 = SE.PlainSMPL(m)(betas=betas, body_pose=aa.detach()[:, 3:], global_orient=aa.detach()[:, :3], pose2rot=True)
    assert SE.stat(out.vertices, ref.vertices) <= SE.gate32(SE.stat(ref32.vertices, ref.vertices))
    assert SE.stat(out.joints, ref.joints) <= SE.gate32(SE.stat(ref32.joints, ref.joints))
    out.vertices.sum().backward()
    assert aa.grad is not None and bool(torch.isfinite(aa.grad).all()) and float(aa.grad.abs().max()) > 0
    with pytest.raises(ValueError, match='axis-angle'):
        layer(betas=betas, body_pose=aa[:, 6:], global_orient=aa[:, :3], pose2rot=True)


def test_state_dict_round_trip_rebuilds_the_derived_arrays():
    a, b = SMPLLayer(SMPLModel.synthetic(V, 7), ops=SE.MockOps()), SMPLLayer(SMPLModel.synthetic(V, 8), ops=SE.MockOps())
    assert sorted(a.state_dict()) == ['J_regressor', 'J_regressor_h36m', 'lbs_weights', 'parents', 'posedirs', 'shapedirs', 'v_template']
    inp = SE.inputs(2, V, 0, 3)
    call = lambda l: l(betas=inp['betas'], body_pose=inp['rot'][:, 1:], global_orient=inp['rot'][:, :1])      # noqa: E731
    assert not torch.equal(call(a).joints, call(b).joints)
    b.load_state_dict(a.state_dict(), strict=True)
    assert torch.equal(b.Jt, a.Jt) and torch.equal(b.Jd, a.Jd)
    assert torch.equal(call(a).vertices, call(b).vertices) and torch.equal(call(a).joints, call(b).joints)
    c = copy.deepcopy(a).double().float()
    assert torch.equal(call(c).vertices, call(a).vertices)
    assert a.J_regressor_h36m.shape == (17, V)


# ------------------------------------------------------------------------------------------------ the head around the layer
def regressor(smpl, ops, seed=3):
    from motionbert_amd.mesh import MeshRegressor
    torch.manual_seed(seed)
    pose, shape = ME.mean_params()
    return MeshRegressor(Backbone(), smpl=smpl, init_pose=pose, init_shape=shape, J_regressor=smpl.J_regressor_h36m, dim_rep=DIM_REP,
                         hidden_dim=HIDDEN, dropout_ratio=0.0, ops=ops)


def test_head_with_the_layer_matches_the_plain_head_within_the_gates():
    m = SMPLModel.synthetic(V, 9)
    ops = SE.MockOps()
    net = regressor(SMPLLayer(m, ops=ops), ops).train()
    stand_in = regressor(ME.StandInSMPL(V), ops).train()
    x = torch.randn(2, 3, 17, 3, generator=torch.Generator().manual_seed(4))
    out, other = net(x), stand_in(x)
    assert sorted(out[0]) == sorted(other[0]) == ['kp_3d', 'theta', 'verts']
    assert {k: v.shape for k, v in out[0].items()} == {k: v.shape for k, v in other[0].items()}
    assert ops.calls['smpl_fwd'] == 1
    w = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(5)) for k, v in out[0].items()}
    sum((out[0][k] * w[k]).sum() for k in w).backward()
    assert ops.calls['smpl_bwd'] == 1
    feat = net.backbone.get_representation(x).reshape(2, 3, 17, -1).detach()
    res = {}
    for d in (F32, F64):
        head = copy.deepcopy(net.head).to(d)
        head.zero_grad()
        head.smpl = SE.PlainSMPL(m)
        head.J_regressor = head.J_regressor.to(d)
        o = ME.plain_head_forward(head, feat.to(d))[0]
        sum((o[k] * w[k].to(d)).sum() for k in w).backward()
        res[d] = ({k: v.detach() for k, v in o.items()}, {n: p.grad for n, p in head.named_parameters()})
    for k in ('verts', 'kp_3d', 'theta'):
        assert SE.stat(out[0][k].detach(), res[F64][0][k]) <= SE.gate32(SE.stat(res[F32][0][k], res[F64][0][k])), k
    grads = dict(net.head.named_parameters())
    for n in ('head_pose.weight', 'head_pose.bias', 'head_shape.weight', 'fc1.weight', 'fc2.weight'):
        assert SE.stat(grads[n].grad, res[F64][1][n]) <= SE.gate32(SE.stat(res[F32][1][n], res[F64][1][n])), n


# ------------------------------------------------------------------------------------------------ flip evaluation
def test_flip_thetas_batch_is_bit_equal_to_the_reference():
    from motionbert_amd.mesh import flip_thetas_batch
    fx = load_golden('smpl_flip')[0]
    n = len([k for k in fx.files if k.startswith('in.')])
    assert n >= 3
    for i in range(n):
        x = torch.from_numpy(fx[f'in.{i}'])
        keep = x.clone()
        y = flip_thetas_batch(x)
        assert y.dtype == x.dtype and y.numpy().tobytes() == fx[f'out.{i}'].tobytes(), i
        assert torch.equal(x, keep), 'the input is left alone'
        assert torch.equal(flip_thetas_batch(y), x), 'an involution'
    with pytest.raises(ValueError, match='72'):
        flip_thetas_batch(torch.zeros(2, 3, 69))


def test_flip_average_against_its_float64_restatement():
    from motionbert_amd.mesh import MeshEvaluator, flip_average
    m = SMPLModel.synthetic(V, 9)
    ops = SE.MockOps()
    layer = SMPLLayer(m, ops=ops)
    net = regressor(layer, ops).eval()
    x = torch.randn(2, 3, 17, 3, generator=torch.Generator().manual_seed(6))
    got = flip_average(net, layer, x)
    assert sorted(got[0]) == ['kp_3d', 'theta', 'verts'] and got[0]['verts'].shape == (2, 3, V, 3) and not got[0]['verts'].requires_grad
    # train_mesh.py:83-108 restated in float64 from the model's two outputs
    with torch.no_grad():
        out = net(x)[0]
        xf = x.clone()
        xf[..., 0] *= -1
        left, right = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
        xf[..., left + right, :] = xf[..., right + left, :]
        fl = net(xf)[0]
    pose = fl['theta'][:, :, :72].double().reshape(2, 3, 24, 3).clone()
    pose[..., 1:] *= -1
    for a, b in ((1, 2), (4, 5), (7, 8), (10, 11), (13, 14), (16, 17), (18, 19), (20, 21), (22, 23)):
        pose[:, :, [a, b]] = pose[:, :, [b, a]]
    pose, shape = pose.reshape(-1, 72), fl['theta'][:, :, 72:].double().reshape(-1, 10)
    verts = SE.PlainSMPL(m)(betas=shape, body_pose=pose[:, 3:], global_orient=pose[:, :3], pose2rot=True).vertices * 1000.0
    kp = m.J_regressor_h36m.double() @ verts
    want = {'theta': (out['theta'].double() + torch.cat([pose, shape], 1).reshape(2, 3, 82)) * 0.5,
            'verts': (out['verts'].double() + verts.reshape(2, 3, V, 3)) * 0.5, 'kp_3d': (out['kp_3d'].double() + kp.reshape(2, 3, 17, 3)) * 0.5}
    for k in want:
        assert SE.stat(got[0][k], want[k]) <= 4e-6, k                 # fp32 model outputs averaged: a few fp32 roundings of millimetre values
    tgt = ME.mesh_targets(2, 3, V, 7)
    ev = MeshEvaluator(ops=ops)
    ev.update(got, tgt)
    ref = ME.aggregate(ME.mesh_errors64(want['verts'].reshape(-1, V, 3).numpy(), tgt['verts'].reshape(-1, V, 3).numpy(),
                                        want['kp_3d'].reshape(-1, 17, 3).numpy(), tgt['kp_3d'].reshape(-1, 17, 3).numpy()))
    res = ev.finish()
    for k in ref:
        assert res[k] == pytest.approx(ref[k], rel=1e-5), k
    # a layer that is not the project's own is called as the reference calls it
    plain = flip_average(net, SE.PlainSMPL(m), x)
    for k in want:
        assert SE.stat(plain[0][k], want[k]) <= 4e-6, k


# ------------------------------------------------------------------------------------------------ header, binding, library
@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_header_binding_and_version_agree(lib):
    from motionbert_amd import hip_ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'mbx.h')).read()
    assert lib.mbx_version() >= 120
    for name in ('mbx_smpl_pack', 'mbx_smpl_fwd_ws', 'mbx_smpl_bwd_ws', 'mbx_smpl_fwd', 'mbx_smpl_bwd'):
        decl = re.search(r'\b%s\(([^;]*)\);' % name, header)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(hip_ops.SIGNATURES[name][1]), name
        assert hasattr(lib, name)


def test_library_refusals_are_reported_not_crashed(lib):
    p = C.c_void_p(4096)            # never dereferenced: every check below fails before a launch
    ok = (C.c_int * 24)(*SMPL_PARENTS)
    big = C.c_size_t(1 << 40)

    def fwd(parents=ok, K=17, F=4, V=65, verts=p, kp=p, ws=p, wsb=big, Q=p, rot=p):
        return lib.mbx_smpl_fwd(p, p, p, p, p, parents, p, Q, K, p, rot, 1.0, verts, kp, p, F, V, ws, wsb, None)

    def bwd(parents=ok, K=17, F=4, V=65, wsb=big, drot=C.c_void_p(8192), dkp=p, Q=p):
        return lib.mbx_smpl_bwd(p, p, p, p, p, p, parents, p, Q, K, p, p, 1.0, p, dkp, None, drot, C.c_void_p(12288), F, V, p, wsb, None)
    for call in (fwd, bwd):
        assert call(V=0) != 0 and b'V >= 1' in lib.mbx_last_error()
        assert call(K=33) != 0 and b'K <= 32' in lib.mbx_last_error()
        bad = list(SMPL_PARENTS)
        bad[5] = 7
        assert call(parents=(C.c_int * 24)(*bad)) != 0 and b'forward-ordered' in lib.mbx_last_error()
        bad = list(SMPL_PARENTS)
        bad[0] = 0
        assert call(parents=(C.c_int * 24)(*bad)) != 0 and b'parents[0]' in lib.mbx_last_error()
        assert call(wsb=C.c_size_t(1024)) != 0 and b'workspace' in lib.mbx_last_error()
        assert call(F=0) == 0, 'F = 0 is a no-op'
        assert call(F=-1) != 0
    assert fwd(verts=None, kp=None, F=0) == 0
    assert lib.mbx_smpl_fwd(p, p, p, p, p, ok, p, None, 0, p, p, 1.0, None, None, None, 4, 65, p, big, None) != 0 and b'no output' in lib.mbx_last_error()
    assert fwd(Q=None) != 0 and b'regressor' in lib.mbx_last_error()
    assert fwd(rot=C.c_void_p(4098)) != 0 and b'aligned' in lib.mbx_last_error()
    assert bwd(drot=p) != 0 and b'alias' in lib.mbx_last_error()
    assert bwd(Q=None) != 0 and b'regressor' in lib.mbx_last_error()
    assert lib.mbx_smpl_fwd_ws(0, 65, 17) == 0 and lib.mbx_smpl_fwd_ws(4, 0, 17) == 0 and lib.mbx_smpl_bwd_ws(4, 65, 33) == 0
    assert lib.mbx_smpl_fwd_ws(2048, 6890, 17) >= 108 * 2048 * 51 * 4 and lib.mbx_smpl_fwd_ws(2048, 6890, 0) < 8 << 20
    assert lib.mbx_smpl_bwd_ws(2048, 6890, 17) >= 9 * 2048 * 512 * 4
    assert lib.mbx_smpl_pack(p, p, p, 0, None) != 0 and b'vertex count' in lib.mbx_last_error()
    assert lib.mbx_smpl_pack(p, None, p, 4, None) != 0 and b'null' in lib.mbx_last_error()


def test_binding_refuses_wrong_layouts_before_the_library_is_called():
    from motionbert_amd import hip_ops

    class Lib:                      # no symbol may be reached
        pass
    ops = hip_ops.HipOps(lib=Lib())
    m = SMPLModel.synthetic(7, 1)
    md = m.tensors()
    md['packed_t'] = torch.zeros(21, 224)
    b, r = torch.zeros(3, 10), torch.zeros(3, 24, 9)
    verts, kp, joints, Q = torch.zeros(3, 7, 3), torch.zeros(3, 17, 3), torch.zeros(3, 24, 3), m.J_regressor_h36m
    ws = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no output'):
        ops.smpl_fwd(md, Q, b, r, 1.0, None, None, None, ws=ws)
    with pytest.raises(RuntimeError, match=r'betas \[F,10\]'):
        ops.smpl_fwd(md, Q, torch.zeros(3, 9), r, 1.0, verts, kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match=r'betas \[F,10\]'):
        ops.smpl_fwd(md, Q, b, torch.zeros(2, 24, 9), 1.0, verts, kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match='rotmat must be a contiguous'):
        ops.smpl_fwd(md, Q, b, torch.zeros(3, 9, 24).transpose(1, 2), 1.0, verts, kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match='betas must be a contiguous'):
        ops.smpl_fwd(md, Q, b.double(), r, 1.0, verts, kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match='verts must be a contiguous'):
        ops.smpl_fwd(md, Q, b, r, 1.0, torch.zeros(3, 8, 3), kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match='kp must be a contiguous'):
        ops.smpl_fwd(md, Q, b, r, 1.0, verts, torch.zeros(3, 14, 3), joints, ws=ws)
    with pytest.raises(RuntimeError, match='kp needs the regressor'):
        ops.smpl_fwd(md, None, b, r, 1.0, verts, torch.zeros(3, 0, 3), joints, ws=ws)
    with pytest.raises(RuntimeError, match=r'Q \[1 <= K <= 32'):
        ops.smpl_fwd(md, torch.zeros(33, 7), b, r, 1.0, verts, None, joints, ws=ws)
    with pytest.raises(RuntimeError, match=r'Q \[1 <= K <= 32'):
        ops.smpl_fwd(md, torch.zeros(17, 8), b, r, 1.0, verts, None, joints, ws=ws)
    with pytest.raises(RuntimeError, match='posedirs must be a contiguous'):
        ops.smpl_fwd({**md, 'posedirs': md['posedirs'][:, :20]}, Q, b, r, 1.0, verts, kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match='lbs_weights must be a contiguous'):
        ops.smpl_fwd({**md, 'lbs_weights': md['lbs_weights'].t().contiguous().t()}, Q, b, r, 1.0, verts, kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match='24 parents'):
        ops.smpl_fwd({**md, 'parents': m.parents[:20]}, Q, b, r, 1.0, verts, kp, joints, ws=ws)
    with pytest.raises(RuntimeError, match='ws must be a contiguous'):
        ops.smpl_fwd(md, Q, b, r, 1.0, verts, kp, joints, ws=torch.zeros(64))
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='must be a contiguous'):
            ops.smpl_fwd(md, Q, b.cuda(), r, 1.0, verts, kp, joints, ws=ws)
    db, dr = torch.zeros(3, 10), torch.zeros(3, 24, 9)
    with pytest.raises(RuntimeError, match='packed_t'):
        ops.smpl_bwd({k: v for k, v in md.items() if k != 'packed_t'}, Q, b, r, 1.0, verts, kp, None, dr, db, ws=ws)
    with pytest.raises(RuntimeError, match='packed_t must be a contiguous'):
        ops.smpl_bwd({**md, 'packed_t': torch.zeros(21, 207)}, Q, b, r, 1.0, verts, kp, None, dr, db, ws=ws)
    with pytest.raises(RuntimeError, match='drotmat and dbetas'):
        ops.smpl_bwd(md, Q, b, r, 1.0, verts, kp, None, None, db, ws=ws)
    with pytest.raises(RuntimeError, match='dverts must be a contiguous'):
        ops.smpl_bwd(md, Q, b, r, 1.0, verts[:, :, :2], kp, None, dr, db, ws=ws)
    with pytest.raises(RuntimeError, match='dkp needs the regressor'):
        ops.smpl_bwd(md, None, b, r, 1.0, verts, kp, None, dr, db, ws=ws)
    with pytest.raises(RuntimeError, match='djoints must be a contiguous'):
        ops.smpl_bwd(md, Q, b, r, 1.0, verts, kp, torch.zeros(3, 23, 3), dr, db, ws=ws)
    with pytest.raises(RuntimeError, match='drotmat must be a contiguous'):
        ops.smpl_bwd(md, Q, b, r, 1.0, verts, kp, None, dr.double(), db, ws=ws)
    with pytest.raises(RuntimeError, match=r'shapedirs \[V >= 1,3,10\]'):
        ops.smpl_pack(torch.zeros(7, 30), md['posedirs'], md['packed_t'])
    with pytest.raises(RuntimeError, match='packed_t must be a contiguous'):
        ops.smpl_pack(md['shapedirs'], md['posedirs'], torch.zeros(21, 207))
