"""motionbert_amd.wild.infer_mesh / solve_scale / place on the CPU with the kernel provider of tests/wildmesherr.py injected: the loop of
infer_wild_mesh.py:99-154 end to end against its restatement, the batching, the dict form and the argument errors.  The kernels
themselves: tests/test_gpu_wild_mesh.py."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from motionbert_amd import wild
from motionbert_amd.smpl import SMPLLayer, SMPLModel
from tests import smplerr as SE
from tests import wilderr as WE
from tests import wildmesherr as WM
from tests.test_smpl import regressor

V, CLIP = 65, WE.CLIP_LEN
VID = (1920, 1080)
TOL = 2e-5        # fp32 outputs of the same equations at another batch size: a few fp32 roundings of millimetre values


def setup(corrupt=None):
    ops = WM.WildMeshOps(corrupt)
    layer = SMPLLayer(SMPLModel.synthetic(V, 9), ops=ops)
    net = regressor(layer, ops).eval()
    # the mean parameters alone give the same pose to every frame; real weights spread them
    with torch.no_grad():
        net.head.head_pose.weight.mul_(40.0)
        net.head.head_shape.weight.mul_(40.0)
    return ops, layer, net


def ref_motion(F, seed):
    r = np.random.RandomState(seed)
    return r.normal(0, 0.25, (1, 17, 3)) + r.normal(0, 0.03, (F, 17, 3)) + np.cumsum(r.normal(0, 0.02, (F, 1, 3)), axis=0)


def restated(net, layer, kp, pixel, flip, ref=None, scale=None):
    motion = WE.input_ref(kp, VID if pixel else None, None if pixel else [1, 1])[0]
    return WM.reference_loop(net, layer, motion, CLIP, flip, ref, scale)


@pytest.mark.parametrize('flip', [True, False])
@pytest.mark.parametrize('pixel', [True, False])
@pytest.mark.parametrize('with_ref', [True, False])
def test_infer_mesh_against_the_restated_loop(flip, pixel, with_ref):
    ops, layer, net = setup()
    kp = WE.detections(2 * CLIP + 4, 8601)
    ref = ref_motion(len(kp), 8602) if with_ref else None
    got = wild.infer_mesh(net, layer, kp, clip_len=CLIP, vid_size=VID, pixel=pixel, flip=flip, ref_3d=ref, want=('verts', 'kp_3d', 'theta'), ops=ops)
    assert sorted(got) == sorted(['verts', 'kp_3d', 'theta'] + (['scale'] if with_ref else []))
    assert got['verts'].shape == (len(kp), V, 3) and got['kp_3d'].shape == (len(kp), 17, 3) and got['theta'].shape == (len(kp), 82)
    assert all(got[k].dtype == np.float32 and np.isfinite(got[k]).all() for k in ('verts', 'kp_3d', 'theta'))
    want_v, want_k = restated(net, layer, kp, pixel, flip, ref, got.get('scale'))
    assert SE.stat(got['kp_3d'], want_k) <= TOL
    assert SE.stat(got['verts'], want_v) <= TOL
    if with_ref:
        row = WM.fit_row(ref, want_k)                       # the restated fit on the restated keypoints
        assert row[5] >= 1 and abs(got['scale'] - row[0]) <= 1e-4 * abs(row[0])
        assert ops.calls['scale_fit'] == 1 and ops.calls['wild_mesh_place'] == 1
    assert ops.mesh_calls == [(2, CLIP, flip), (1, 4, flip)]         # the full clips in one batch, the tail in its own


def test_batch_size_does_not_change_the_result():
    res = {}
    for mb in (1, 2, 64):
        ops, layer, net = setup()
        kp = WE.detections(3 * CLIP + 2, 8603)
        res[mb] = wild.infer_mesh(net, layer, kp, clip_len=CLIP, max_batch=mb, ops=ops)
        assert ops.mesh_calls == {1: [(1, CLIP, True)] * 3, 2: [(2, CLIP, True), (1, CLIP, True)], 64: [(3, CLIP, True)]}[mb] + [(1, 2, True)]
    for mb in (2, 64):
        for k in ('verts', 'kp_3d'):
            assert SE.stat(res[mb][k], res[1][k]) <= TOL, (mb, k)


def test_dict_form_pools_the_tracks():
    ops, layer, net = setup()
    tracks, _ = WE.persons()
    refs = OrderedDict((k, ref_motion(len(v), 8610 + k)) for k, v in tracks.items())
    got = wild.infer_mesh(net, layer, tracks, clip_len=CLIP, ref_3d=refs, max_batch=2, ops=ops)
    assert list(got) == list(tracks)
    # full clips of all tracks pooled (7: two, 1: one), then the tails by length (3: 5 frames, 1: 1 frame)
    assert ops.mesh_calls == [(2, CLIP, True), (1, CLIP, True), (1, 5, True), (1, 1, True)]
    assert ops.calls['scale_fit'] == 1 and ops.calls['wild_mesh_place'] == 1
    for k, kp in tracks.items():
        ops1, layer1, net1 = setup()
        one = wild.infer_mesh(net1, layer1, kp, clip_len=CLIP, ref_3d=refs[k], ops=ops1)
        assert got[k]['verts'].shape == (len(kp), V, 3)
        assert abs(got[k]['scale'] - one['scale']) <= 1e-6 * abs(one['scale'])
        for name in ('verts', 'kp_3d'):
            assert SE.stat(got[k][name], one[name]) <= TOL, (k, name)


def test_to_host_false_returns_tensors_and_want_selects():
    ops, layer, net = setup()
    kp = WE.detections(CLIP + 1, 8604)
    got = wild.infer_mesh(net, layer, kp, clip_len=CLIP, want=('kp_3d',), to_host=False, ops=ops)
    assert list(got) == ['kp_3d'] and isinstance(got['kp_3d'], torch.Tensor)
    got = wild.infer_mesh(net, layer, kp, clip_len=CLIP, want=('verts',), ref_3d=ref_motion(len(kp), 1), to_host=False, ops=ops)
    assert sorted(got) == ['scale', 'verts'] and isinstance(got['scale'], float)
    wrapped = torch.nn.DataParallel(net) if hasattr(torch.nn, 'DataParallel') else net
    again = wild.infer_mesh(wrapped, layer, kp, clip_len=CLIP, want=('kp_3d',), ops=ops)
    assert again['kp_3d'].shape == (len(kp), 17, 3)


def test_solve_scale_and_place():
    ops = WM.WildMeshOps()
    ref, kp = WM.fit_problem('p340')
    s, t, obj, it = wild.solve_scale(ref, kp, ops=ops)
    s0, t0, o0, _ = WM.fit_ref('p340')
    assert abs(s - s0) <= 1e-10 * s0 and abs(obj - o0) <= 1e-10 * o0 and t.shape == (3,) and it >= 2
    ref2, kp2, lens = WM.pool_problem()
    with pytest.raises(ValueError, match='track 1 has no frames'):
        wild.solve_scale(ref2, kp2, seq_lens=lens, ops=ops)
    rows = wild.solve_scale(np.concatenate([ref, ref]), np.concatenate([kp, kp]), seq_lens=[20, 20], ops=ops)
    assert len(rows) == 2 and rows[0][0] == rows[1][0] == s
    with pytest.raises(ValueError, match='without extent'):
        wild.solve_scale(*WM.no_extent_problem(), ops=ops)
    verts, k, r, lens, fit = WM.place_problem(V)
    want = WM.place_eq(verts, k, r, fit[:, 0], lens)
    for f in (torch.from_numpy(fit), [(fit[0, 0], None, 0.0, 3), (fit[1, 0], None, 0.0, 3)]):
        v = torch.from_numpy(verts.copy())
        assert wild.place(v, k, r, f, seq_lens=lens, ops=ops) is v
        assert WE.differing(v.numpy(), want) == 0


def test_argument_errors():
    ops, layer, net = setup()
    kp = WE.detections(CLIP, 8605)
    with pytest.raises(ValueError, match='want'):
        wild.infer_mesh(net, layer, kp, clip_len=CLIP, want=('verts', 'joints'), ops=ops)
    with pytest.raises(ValueError, match='want'):
        wild.infer_mesh(net, layer, kp, clip_len=CLIP, want=(), ops=ops)
    with pytest.raises(ValueError, match='vid_size'):
        wild.infer_mesh(net, layer, kp, clip_len=CLIP, pixel=True, ops=ops)
    with pytest.raises(ValueError, match='>= 1'):
        wild.infer_mesh(net, layer, kp, clip_len=0, ops=ops)
    with pytest.raises(ValueError, match=r'reference motion \[9,17,3\]'):
        wild.infer_mesh(net, layer, kp, clip_len=CLIP, ref_3d=np.zeros((8, 17, 3)), ops=ops)
    with pytest.raises(ValueError, match='dict matching the tracks'):
        wild.infer_mesh(net, layer, {0: kp}, clip_len=CLIP, ref_3d=np.zeros((9, 17, 3)), ops=ops)
    with pytest.raises(ValueError, match='has the tracks'):
        wild.infer_mesh(net, layer, {0: kp}, clip_len=CLIP, ref_3d={1: np.zeros((9, 17, 3))}, ops=ops)
    with pytest.raises(TypeError, match='SMPLLayer'):
        wild.infer_mesh(net, SE.PlainSMPL(SMPLModel.synthetic(V, 9)), kp, clip_len=CLIP, ops=ops)
    foreign = regressor(SE.PlainSMPL(SMPLModel.synthetic(V, 9)), ops)
    with pytest.raises(TypeError, match='flip_average'):
        wild.infer_mesh(foreign, layer, kp, clip_len=CLIP, ops=ops)
    with pytest.raises(TypeError, match='MeshRegressor'):
        wild.infer_mesh(net.backbone, layer, kp, clip_len=CLIP, ops=ops)
    with pytest.raises(ValueError, match='track 0 has a reference motion without extent'):
        wild.infer_mesh(net, layer, kp, clip_len=CLIP, ref_3d=np.ones((9, 17, 3)), ops=ops)
    with pytest.raises(ValueError, match='in place'):
        wild.place(np.zeros((2, 3, 3), np.float32), np.zeros((2, 17, 3)), np.zeros((2, 17, 3)), (1.0, None, 0.0, 2), ops=ops)
    with pytest.raises(RuntimeError, match='no CPU path'):
        wild.infer_mesh(net, layer, kp, clip_len=CLIP)


def test_a_corrupted_provider_is_seen_end_to_end():
    """the end-to-end comparison is no tautology: the paired stage without its 0.5 fails it"""
    ops, layer, net = setup('pair_without_half')
    kp = WE.detections(CLIP + 3, 8606)
    got = wild.infer_mesh(net, layer, kp, clip_len=CLIP, ops=ops)
    want_v, want_k = restated(net, layer, kp, False, True)
    assert SE.stat(got['verts'], want_v) > 0.1 and SE.stat(got['kp_3d'], want_k) > 0.1
