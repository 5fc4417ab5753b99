"""The mesh data path on the CPU: `pack_mesh` against the reference-minted fixture (tests/golden/mesh_gt.npz), `PackedMesh` and
`mesh_targets` with the torch mock provider of tests/meshgterr.py, and their argument errors."""
import os
import pickle

import numpy as np
import pytest
import torch

from motionbert_amd.data import PackedMesh, pack_mesh
from motionbert_amd.mesh import mesh_targets
from motionbert_amd.smpl import SMPLLayer, SMPLModel
from tests import meshgterr as GE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh_gt.npz')
V = 33
MODEL = SMPLModel.synthetic(V, 3200)


@pytest.fixture(scope='module')
def fx():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def layer():
    return SMPLLayer(MODEL)


def write_pickle(tmp_path, dataset):
    path = str(tmp_path / f'{dataset}.pkl')
    with open(path, 'wb') as f:
        pickle.dump(GE.make_pickle(dataset, GE.PACK_SEED[dataset]), f)
    return path


@pytest.mark.parametrize('dataset,clip_len,data_stride', GE.PACK_CASES)
def test_pack_mesh_reproduces_the_reference_bit_for_bit(fx, tmp_path, dataset, clip_len, data_stride):
    path = write_pickle(tmp_path, dataset)
    for split in ('train', 'test'):
        prefix = str(tmp_path / f'{dataset}_{split}')
        meta = pack_mesh(path, dataset, split, clip_len, data_stride, prefix)
        for name in ('motion2d', 'pose', 'shape'):
            got, want = np.load(f'{prefix}.{name}.npy'), fx[f'pack.{dataset}.{split}.{name}']
            assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), (dataset, split, name)
        assert meta['n'] == len(fx[f'pack.{dataset}.{split}.pose']) and meta['clip_len'] == (1 if dataset == 'coco' else clip_len)


def test_pack_mesh_argument_errors(tmp_path):
    path = write_pickle(tmp_path, 'pw3d')
    with pytest.raises(ValueError, match='sample_stride'):
        pack_mesh(path, 'pw3d', 'train', 8, 4, str(tmp_path / 'x'), sample_stride=2)
    with pytest.raises(ValueError, match='undefined'):
        pack_mesh(path, 'agora', 'train', 8, 4, str(tmp_path / 'x'))
    with pytest.raises(ValueError, match='data_split'):
        pack_mesh(path, 'pw3d', 'val', 8, 4, str(tmp_path / 'x'))
    bad = GE.make_pickle('h36m', 1)
    bad['train']['camera_name'][3] = '12345678'
    with open(tmp_path / 'bad.pkl', 'wb') as f:
        pickle.dump(bad, f)
    with pytest.raises(ValueError, match='invalid camera name'):
        pack_mesh(str(tmp_path / 'bad.pkl'), 'h36m', 'train', 8, 4, str(tmp_path / 'x'))


@pytest.fixture(scope='module')
def packed(tmp_path_factory):
    root = tmp_path_factory.mktemp('mesh')
    path = write_pickle(root, 'h36m')
    prefix = str(root / 'h36m_train')
    pack_mesh(path, 'h36m', 'train', 8, 4, prefix)
    return prefix


def collect(ds, **kw):
    return [(x, gt) for x, gt in ds.batches(**kw)]


def test_packed_mesh_yields_what_the_step_and_the_evaluator_take(layer, packed):
    ds = PackedMesh(packed, layer, device='cpu', ops=GE.MockOps())
    assert len(ds) == 7
    got = collect(ds, batch_size=3, shuffle=True, epoch=1, seed=5)
    assert [x.shape[0] for x, _ in got] == [3, 3, 1]
    for x, gt in got:
        B = x.shape[0]
        assert tuple(gt) == ('theta', 'kp_3d', 'verts')
        assert x.shape == (B, 8, 17, 3) and gt['theta'].shape == (B, 8, 82) and gt['kp_3d'].shape == (B, 8, 17, 3) and gt['verts'].shape == (B, 8, V, 3)
        assert all(t.dtype == torch.float32 and not t.requires_grad for t in (x, *gt.values()))
        assert float(x[..., 2].min()) >= 0 and float(x[..., 2].max()) <= 1 and bool((gt['kp_3d'][:, :, 0] == 0).all())
    assert [x.shape[0] for x, _ in collect(ds, batch_size=3, drop_last=True)] == [3, 3]
    # the targets are the float64 definition's, within its gate
    x, gt = got[0]
    ref64, gate = GE.gates(MODEL, gt['theta'])
    assert GE.check(gt, None, None, None, ref64, gate) == []
    # MeshLoss and the evaluator take the pair as it is
    from motionbert_amd.mesh import MeshEvaluator, MeshLoss
    from tests import mesherr as ME
    out = [{k: v + 1.0 for k, v in gt.items()}]
    losses = MeshLoss(loss_type='L1', lambdas=ME.Lambdas, ops=GE.MockOps())(out, gt)
    assert bool(torch.isfinite(losses['total']))
    ev = MeshEvaluator(ops=GE.MockOps())
    ev.update(out, gt)
    assert set(ev.finish()) == {'mpve', 'mpjpe', 'pa_mpjpe', 'mpjpe_17j', 'pa_mpjpe_17j'}


def test_packed_mesh_flips_in_training_only_and_reproducibly(layer, packed):
    stored = np.load(packed + '.motion2d.npy')
    pose = np.load(packed + '.pose.npy')
    test = PackedMesh(packed, layer, device='cpu', train=False, ops=GE.MockOps())
    for e in range(3):
        for (x, gt), idx in zip(test.batches(batch_size=4, shuffle=False, epoch=e, seed=9), ([0, 1, 2, 3], [4, 5, 6])):
            want = stored[idx].copy()
            want[..., 2] = np.clip(want[..., 2], 0, 1)
            assert x.numpy().tobytes() == want.tobytes() and gt['theta'][..., :72].numpy().tobytes() == pose[idx].tobytes()
    off = PackedMesh(packed, layer, device='cpu', train=True, flip=False, ops=GE.MockOps())
    assert all(gt['theta'][..., :72].numpy().tobytes() == pose[i].tobytes()
               for (x, gt), i in zip(off.batches(batch_size=4, shuffle=False), ([0, 1, 2, 3], [4, 5, 6])))
    train = PackedMesh(packed, layer, device='cpu', train=True, ops=GE.MockOps())
    flipped = 0
    for e in range(4):
        a, b = collect(train, batch_size=4, shuffle=True, epoch=e, seed=9, rank=0, world=1), collect(train, batch_size=4, shuffle=True, epoch=e, seed=9)
        for (xa, ga), (xb, gb) in zip(a, b):
            assert torch.equal(xa, xb) and all(torch.equal(ga[k], gb[k]) for k in ga)
        order = np.sort(np.random.default_rng([9, e]).permutation(7)[:4])
        flipped += int((a[0][1]['theta'][:, 0, 1] != torch.from_numpy(pose[order][:, 0, 1])).sum())
    assert 0 < flipped < 16, 'four epochs of four clips: some flipped, not all'
    other = collect(train, batch_size=4, shuffle=True, epoch=0, seed=10)
    mine = collect(train, batch_size=4, shuffle=True, epoch=0, seed=9)
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(other, mine))


def test_two_ranks_partition_an_epoch(layer, packed):
    shape = np.load(packed + '.shape.npy')
    ds = PackedMesh(packed, layer, device='cpu', train=True, ops=GE.MockOps())
    seen = []
    for rank in (0, 1):
        rows = torch.cat([gt['theta'][:, 0, 72:] for _, gt in ds.batches(batch_size=2, shuffle=True, epoch=2, seed=3, rank=rank, world=2)])
        assert rows.shape[0] == 4                                                   # ceil(7 / 2): equal shares, one clip wrapped around
        seen += [int(np.flatnonzero((shape[:, 0] == r.numpy()).all(1))[0]) for r in rows]
    assert sorted(set(seen)) == list(range(7)) and len(seen) == 8


def test_mesh_targets_argument_errors(layer):
    pose, shape, m2d = GE.inputs(2, 3, 4)
    ops = GE.MockOps()
    bare = SMPLModel.synthetic(V, 1)
    bare.J_regressor_h36m = None
    with pytest.raises(ValueError, match='J_regressor_h36m'):
        mesh_targets(SMPLLayer(bare), pose, shape, ops=ops)
    with pytest.raises(TypeError, match='SMPLLayer'):
        mesh_targets(object(), pose, shape, ops=ops)
    with pytest.raises(ValueError, match=r'pose \[N,T,72\]'):
        mesh_targets(layer, pose[..., :69], shape, ops=ops)
    with pytest.raises(ValueError, match='shape'):
        mesh_targets(layer, pose, shape[:1], ops=ops)
    with pytest.raises(ValueError, match='motion_2d'):
        mesh_targets(layer, pose, shape, m2d[:, :, :16], ops=ops)
    with pytest.raises(ValueError, match='flip'):
        mesh_targets(layer, pose, shape, flip=torch.ones(3, dtype=torch.uint8), ops=ops)
    with pytest.raises(ValueError, match='flip'):
        mesh_targets(layer, pose, shape, flip=torch.ones(2), ops=ops)
    with pytest.raises(ValueError, match='flip_prob'):
        mesh_targets(layer, pose, shape, flip=True, flip_prob=1.5, ops=ops)
    with pytest.raises(ValueError, match='want'):
        mesh_targets(layer, pose, shape, want=('theta', 'joints'), ops=ops)
    with pytest.raises(ValueError, match='nothing to compute'):
        mesh_targets(layer, pose, shape, want=(), ops=ops)
    with pytest.raises(RuntimeError, match='no CPU path'):
        mesh_targets(layer, pose, shape)
    assert ops.calls == {}


def test_mesh_targets_want_and_flags(layer):
    pose, shape, m2d = GE.inputs(2, 3, 4)
    ops = GE.MockOps()
    x, out = mesh_targets(layer, pose, shape, ops=ops, want=('kp_3d',))
    assert x is None and tuple(out) == ('kp_3d',)
    x, out, used = mesh_targets(layer, pose, shape, m2d, flip=torch.tensor([True, False]), want=(), return_flips=True, ops=ops)
    assert out == {} and used.tolist() == [1, 0] and x.shape == m2d.shape
    _, _, used = mesh_targets(layer, pose, shape, flip=True, seed=77, want=('theta',), return_flips=True, ops=ops)
    assert used.tolist() == GE.drawn_flags(77, 2, 0.5).tolist()
    _, _, used = mesh_targets(layer, pose, shape, flip=True, flip_prob=1.0, want=('theta',), return_flips=True, ops=ops)
    assert used.tolist() == [1, 1]
    x, out = mesh_targets(layer, pose[:0], shape[:0], m2d[:0], ops=ops)
    assert x.shape == (0, 3, 17, 3) and x.data_ptr() != m2d.data_ptr() and out['verts'].shape == (0, 3, V, 3) and ops.calls['mesh_gt'] == 4


# ------------------------------------------------------------------------------------------------ header, binding, library
@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_library_refusals_are_reported_not_crashed(lib):
    import ctypes as C
    from motionbert_amd.smpl import SMPL_PARENTS
    assert lib.mbx_version() >= 140
    p, q = C.c_void_p(4096), C.c_void_p(8192)            # never dereferenced: every check below fails before a launch
    ok = (C.c_int * 24)(*SMPL_PARENTS)
    big = C.c_size_t(1 << 40)

    def gt(pose=p, shape=p, m2d=p, flips=None, prob=0.5, vt=p, parents=ok, Q=p, K=17, x2d=q, theta=q, kp=q, verts=q, used=q, N=2, T=3, V=65,
           ws=p, wsb=big):
        return lib.mbx_mesh_gt(pose, shape, m2d, flips, 7, prob, vt, p, p, p, p, parents, p, Q, K, 1000.0, x2d, theta, kp, verts, used, N, T, V,
                               ws, wsb, None)
    assert gt(V=0) != 0 and b'V >= 1' in lib.mbx_last_error()
    assert gt(K=33) != 0 and b'K <= 32' in lib.mbx_last_error()
    assert gt(K=0) != 0 and b'1 <= K' in lib.mbx_last_error()
    assert gt(T=0) != 0 and b'T >= 1' in lib.mbx_last_error()
    assert gt(N=1 << 19, T=4) != 0 and b'2^20' in lib.mbx_last_error()
    bad = list(SMPL_PARENTS)
    bad[5] = 7
    assert gt(parents=(C.c_int * 24)(*bad)) != 0 and b'forward-ordered' in lib.mbx_last_error()
    assert gt(x2d=None, theta=None, kp=None, verts=None, used=None) != 0 and b'no output' in lib.mbx_last_error()
    assert gt(prob=1.5) != 0 and b'flip_prob' in lib.mbx_last_error()
    assert gt(pose=None) != 0 and b'null' in lib.mbx_last_error()
    assert gt(m2d=None) != 0 and b'motion_2d' in lib.mbx_last_error()
    assert gt(m2d=q) != 0 and b'alias' in lib.mbx_last_error()
    assert gt(vt=None) != 0 and b'null' in lib.mbx_last_error()
    assert gt(Q=None) != 0 and b'null' in lib.mbx_last_error()
    assert gt(ws=None) != 0 and b'null' in lib.mbx_last_error()
    assert gt(wsb=C.c_size_t(1024)) != 0 and b'workspace' in lib.mbx_last_error()
    assert gt(pose=C.c_void_p(4098)) != 0 and b'aligned' in lib.mbx_last_error()
    assert gt(verts=C.c_void_p(8194)) != 0 and b'aligned' in lib.mbx_last_error()
    assert gt(ws=C.c_void_p(4100)) != 0 and b'aligned' in lib.mbx_last_error()
    assert gt(N=0) == 0                                   # F = 0 returns at once
    assert lib.mbx_mesh_gt_ws(6, 65, 17) >= lib.mbx_smpl_fwd_ws(6, 65, 17) + 6 * 216 * 4 and lib.mbx_mesh_gt_ws(0, 65, 17) == 0
