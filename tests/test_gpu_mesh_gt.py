"""The mesh targets on a real MI355X (mbx_mesh_gt in csrc/smpl.hip, motionbert_amd.mesh.mesh_targets, motionbert_amd.data.PackedMesh) against
tests/meshgterr.py: `theta`, `x2d` and the flags bit for bit against the restated flips (pinned to the reference's own functions by
tests/golden/mesh_gt.npz), `kp_3d` and `verts` against the float64 plain path.

Gate, not a number read off a kernel: per fp32 output array, max |error| / max |float64 value| at most 4 x what the plain path shows in
float32 on the CPU against itself in float64 on the same inputs, never less than 8 fp32 ulps.  Every measured ratio goes to
mesh_gt_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/).

Shapes: the forward tiles 64 vertices x 32 frames, 8 per wave; the flag belongs to the clip, the prepare kernel handles 4 frames per
workgroup, the centring kernel 8 frames x 2048 vertices.  CASES crosses (N, T) in {(1,1), (2,1), (11,3), (5,7), (3,16), (33,1)} with V in
{1, 63, 65, 257}, K = 17, sparse and dense weights alternating and the four flip patterns rotating; then K = 1 (kp_3d exactly zero) and
the real V = 6890 (four centring chunks, the last one partial).  Every case carries the planted rows of meshgterr.inputs.

Measured on the MI355X (profiles/mesh_gt_parity.txt): every ratio below 1; the largest are kp_3d at 0.80 and verts at 0.50, both for one clip
of one frame with V = 65 (every other case: at most 0.45 and 0.31); both are exactly 0 where the float64 value is (V = 1, K = 1).  The two
end-to-end step ratios are 0: target errors of this size average out of a loss over 12,000 elements, so that check sees gross errors only."""
import json
import math
import os
import pickle
import time

import numpy as np
import pytest
import torch

from motionbert_amd.smpl import SMPLLayer, SMPLModel
from tests import mesherr as ME
from tests import meshgterr as GE
from tests import smplerr as SE
from tests.helpers import build_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = torch.float32
REPORT = {}

NTS, VS = ((1, 1), (2, 1), (11, 3), (5, 7), (3, 16), (33, 1)), (1, 63, 65, 257)
FLIPS = GE.PATTERNS + ('drawn',)
CASES = [(N, T, V, 17, (i + j) % 2 == 1, FLIPS[(i + j) % 4]) for i, (N, T) in enumerate(NTS) for j, V in enumerate(VS)]
CASES += [(5, 7, 65, 1, False, 'alternating'), (2, 2, 6890, 17, False, 'alternating')]


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'mesh_gt_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'mesh_gt_parity.txt'), 'w') as f:
        f.write('mesh targets against float64: measured statistic / gate per case and output (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + '  '.join(f'{n} {v:.4g}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def bits(t):
    return t.view(torch.int32)


def guarded(*shape, dtype=F32, pad=64):
    """an output filled with NaN (uint8: 0xAB) inside a larger buffer filled alike: (the output, a check that nothing around it was written)"""
    n = int(np.prod(shape))
    fill = math.nan if dtype == F32 else 0xAB
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)

    def untouched():
        edge = torch.cat([buf[:pad], buf[pad + n:]])
        return bool(torch.isnan(edge).all()) if dtype == F32 else bool((edge == 0xAB).all())
    return buf[pad:pad + n].view(*shape), untouched


def rotations(ops, ws, F, V, K):
    """[F,24,9]: the rotation matrices a call with kp_3d or verts left in its workspace.  Test-only knowledge of csrc/smpl.hip's layout, which
    include/mbx.h does not promise: the forward's workspace (mbx_smpl_fwd_ws less its 256 spare bytes), then the matrices."""
    off = int(ops.lib.mbx_smpl_fwd_ws(F, V, K)) - 256
    return ws[off:off + F * 216 * 4].view(F32).view(F, 24, 9).clone()


def run(ops, md, Q, dev, flags, seed, N, T, V, K, ws, names=('x2d', 'theta', 'kp_3d', 'verts', 'flips_used')):
    shapes = dict(x2d=(N, T, 17, 3), theta=(N, T, 82), kp_3d=(N, T, K, 3), verts=(N, T, V, 3), flips_used=(N,))
    out, oks = {}, []
    for n in names:
        out[n], ok = guarded(*shapes[n], dtype=torch.uint8 if n == 'flips_used' else F32)
        oks.append(ok)
    ops.mesh_gt(md, Q, dev['pose'], dev['shape'], dev['m2d'], flags, seed, 0.5, GE.SCALE, out.get('x2d'), out.get('theta'), out.get('kp_3d'),
                out.get('verts'), out.get('flips_used'), ws=ws)
    torch.cuda.synchronize()
    assert all(ok() for ok in oks), 'a kernel wrote outside its output'
    return out


@pytest.mark.parametrize('N,T,V,K,dense,pattern', CASES)
def test_targets_against_the_reference(ops, N, T, V, K, dense, pattern):
    F = N * T
    model = SMPLModel.synthetic(V, 1000 + V, dense)
    md = model.tensors(DEV)
    Q = model.J_regressor_h36m[:K].contiguous()
    seed = 3000 + 17 * N + T + V
    pose, shape, m2d = GE.inputs(N, T, seed)
    want_flags = GE.drawn_flags(seed, N, 0.5) if pattern == 'drawn' else GE.flip_pattern(N, pattern)
    want_x2d, want_theta = GE.exact_targets(pose.numpy(), shape.numpy(), m2d.numpy(), want_flags.numpy())
    ref64, gate = GE.gates(model, want_theta, Q)
    dev = dict(pose=pose.to(DEV), shape=shape.to(DEV), m2d=m2d.to(DEV))
    flags = None if pattern == 'drawn' else want_flags.to(DEV)
    Qd = Q.to(DEV)
    ws = ops.mesh_gt_ws(F, V, K, DEV)
    tag = f'N{N}.T{T}.V{V}.K{K}.{"dense" if dense else "sparse"}.{pattern}'
    got = run(ops, md, Qd, dev, flags, seed, N, T, V, K, ws)
    rep = REPORT.setdefault(tag, {})
    failed = GE.check(got, want_x2d, want_theta, want_flags, ref64, gate, rep)
    print(tag, ' '.join(f'{k} {v:.3f}' for k, v in sorted(rep.items())))
    assert failed == [], failed
    assert bool(torch.isfinite(got['verts']).all()) and bool(torch.isfinite(got['kp_3d']).all())
    assert bool((got['kp_3d'][:, :, 0] == 0).all()), 'the root joint is the origin'
    if K == 1:
        assert torch.equal(got['kp_3d'], torch.zeros_like(got['kp_3d']))
    # ---- all-zero rotation vectors give the identity exactly: joints 22 and 23 everywhere and, with F > 1, the whole last frame
    rot = rotations(ops, ws, F, V, K)
    eye = torch.eye(3, device=DEV).reshape(9)
    assert bool(torch.isfinite(rot).all()) and bool((rot[:, 22:] == eye).all())
    if F > 1:
        assert bool((rot[F - 1] == eye).all())
        # the rest pose: the template plus the shape offsets through the identity chain, centred
        rest64 = GE.body_targets(model, torch.cat([torch.zeros(1, 1, 72), shape.reshape(F, 10)[F - 1].reshape(1, 1, 10)], -1), torch.float64, Q)[1]
        assert SE.stat(got['verts'].reshape(F, V, 3)[F - 1:].cpu(), rest64.reshape(1, V, 3)) <= gate['verts']
    # ---- mbx_smpl_fwd on the same rotations: scale x from the same kernels, the root from the same fixed-order sum
    v, k = torch.full((F, V, 3), math.nan, device=DEV), torch.full((F, K, 3), math.nan, device=DEV)
    ops.smpl_fwd(md, Qd, dev['shape'].reshape(F, 10), rot, GE.SCALE, v, k, None)
    assert torch.equal(bits(v - k[:, :1]), bits(got['verts'].reshape(F, V, 3))), 'verts differ from smpl_fwd verts - kp[:, :1]'
    assert torch.equal(bits(k - k[:, :1]), bits(got['kp_3d'].reshape(F, K, 3))), 'kp_3d differs from smpl_fwd kp - kp[:, :1]'
    # ---- the same bits twice
    again = run(ops, md, Qd, dev, flags, seed, N, T, V, K, ws)
    for n in ('x2d', 'theta', 'kp_3d', 'verts'):
        assert torch.equal(bits(again[n]), bits(got[n])), n
    assert torch.equal(again['flips_used'], got['flips_used'])
    # ---- verts alone (the vertex kernel then forms the root's partials only) and kp_3d alone give the bits of the full call
    for n in ('verts', 'kp_3d'):
        one = run(ops, md, Qd, dev, flags, seed, N, T, V, K, ws, names=(n,))
        assert torch.equal(bits(one[n]), bits(got[n])), n + ' alone'


def test_every_combination_of_outputs(ops):
    from motionbert_amd.mesh import mesh_targets
    N, T, V = 3, 5, 65
    layer = SMPLLayer(SMPLModel.synthetic(V, 61)).to(DEV)
    pose, shape, m2d = [a.to(DEV) for a in GE.inputs(N, T, 62)]
    flags = GE.flip_pattern(N, 'alternating').to(DEV)
    x_full, full, used = mesh_targets(layer, pose, shape, m2d, flip=flags, return_flips=True)
    assert torch.equal(used, flags) and tuple(full) == ('theta', 'kp_3d', 'verts')
    keys = ('theta', 'kp_3d', 'verts')
    for mask in range(8):
        want = tuple(k for i, k in enumerate(keys) if mask >> i & 1)
        for with_2d in (True, False):
            if not want and not with_2d:
                continue
            x, out = mesh_targets(layer, pose, shape, m2d if with_2d else None, flip=flags.bool(), want=want)
            assert tuple(out) == want and (x is None) == (not with_2d)
            assert x is None or torch.equal(bits(x), bits(x_full))
            for k in want:
                assert torch.equal(bits(out[k]), bits(full[k])), (want, with_2d, k)
    assert not full['verts'].requires_grad and full['verts'].dtype == F32
    # None / False: no flips
    for flip in (None, False):
        _, out, used = mesh_targets(layer, pose, shape, flip=flip, want=('theta',), return_flips=True)
        assert int(used.sum()) == 0 and torch.equal(bits(out['theta'][..., :72]), bits(pose))
    with pytest.raises(RuntimeError, match='no CPU path'):
        mesh_targets(layer, pose.cpu(), shape, m2d)


def test_drawn_flags_follow_the_seed_and_the_probability(ops):
    from motionbert_amd.mesh import mesh_targets
    N = 4096
    layer = SMPLLayer(SMPLModel.synthetic(1, 63)).to(DEV)
    g = torch.Generator().manual_seed(64)
    pose, shape = (0.5 * torch.randn(N, 1, 72, generator=g)).to(DEV), torch.randn(N, 1, 10, generator=g).to(DEV)
    a = mesh_targets(layer, pose, shape, flip=True, seed=1234, want=('theta',), return_flips=True)
    b = mesh_targets(layer, pose, shape, flip=True, seed=1234, want=('theta',), return_flips=True)
    c = mesh_targets(layer, pose, shape, flip=True, seed=1235, want=('theta',), return_flips=True)
    assert torch.equal(a[2], b[2]) and torch.equal(bits(a[1]['theta']), bits(b[1]['theta'])) and not torch.equal(a[2], c[2])
    assert torch.equal(a[2].cpu(), GE.drawn_flags(1234, N, 0.5)), 'the draw is the counter-based hash of (seed, clip index)'
    count = int(a[2].sum())
    print('flipped', count, 'of', N)
    REPORT['drawn.4096'] = dict(flipped=count)
    assert abs(count - 2048) <= 160                 # five standard deviations of the binomial
    flipped = a[2].bool()
    assert bool((a[1]['theta'][flipped][:, 0, 1] == -pose[flipped][:, 0, 1]).all()) and torch.equal(a[1]['theta'][~flipped][..., :72], pose[~flipped])
    torch.manual_seed(5)
    d = mesh_targets(layer, pose, shape, flip=True, want=('theta',), return_flips=True)
    torch.manual_seed(5)
    e = mesh_targets(layer, pose, shape, flip=True, want=('theta',), return_flips=True)
    assert torch.equal(d[2], e[2]) and 0 < int(d[2].sum()) < N, 'the default seed comes from torch\'s CPU generator'


def test_more_frames_than_a_grid_y_carries(ops):
    """8 x 65,535 = 524,280 frames is where a centring grid with its frame blocks on y would end: past it the last frames must be centred
    like the first.  A frame's result does not depend on the batch around it, so the last clips equal a call on them alone bit for bit."""
    from motionbert_amd.mesh import mesh_targets
    N, V, tail = 8 * 65535 + 24, 2, 40
    layer = SMPLLayer(SMPLModel.synthetic(V, 65)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(66)
    pose, shape = 0.5 * torch.randn(N, 1, 72, generator=g, device=DEV), torch.randn(N, 1, 10, generator=g, device=DEV)
    _, big = mesh_targets(layer, pose, shape, want=('kp_3d', 'verts'))
    _, small = mesh_targets(layer, pose[N - tail:], shape[N - tail:], want=('kp_3d', 'verts'))
    for k in ('kp_3d', 'verts'):
        assert bool(torch.isfinite(big[k]).all()) and torch.equal(bits(big[k][N - tail:]), bits(small[k])), k
    assert bool((big['kp_3d'][:, :, 0] == 0).all()) and float(small['verts'].abs().max()) > 1.0
    del big, pose, shape
    layer._ws.clear()
    torch.cuda.empty_cache()


def test_refusals(ops):
    model = SMPLModel.synthetic(7, 1)
    md = model.tensors(DEV)
    Q = model.J_regressor_h36m.to(DEV)
    pose, shape, m2d = [a.to(DEV) for a in GE.inputs(2, 2, 3)]
    theta, verts = torch.zeros(2, 2, 82, device=DEV), torch.zeros(2, 2, 7, 3, device=DEV)
    with pytest.raises(RuntimeError, match='workspace'):
        ops.mesh_gt(md, Q, pose, shape, None, None, 0, 0.0, 1000.0, None, theta, None, verts, None, ws=torch.zeros(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='no output'):
        ops.mesh_gt(md, Q, pose, shape, m2d, None, 0, 0.0, 1000.0, None, None, None, None, None)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.mesh_gt(md, Q, pose.cpu(), shape, None, None, 0, 0.0, 1000.0, None, theta, None, None, None)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.mesh_gt(md, Q, pose, shape, None, torch.zeros(2, device=DEV), 0, 0.0, 1000.0, None, theta, None, None, None)
    with pytest.raises(RuntimeError, match='alias'):
        ops.mesh_gt(md, Q, pose, shape, m2d, None, 0, 0.0, 1000.0, m2d, theta, None, None, None)
    ops.mesh_gt(md, Q, pose[:0], shape[:0], None, None, 0, 0.0, 1000.0, None, theta[:0], None, verts[:0], None)       # F = 0 is a no-op
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
CFG = dict(dim_in=3, dim_out=3, dim_feat=128, dim_rep=128, depth=2, num_heads=4, mlp_ratio=4, num_joints=17, maxlen=243)
HIDDEN, V = 256, 257
MODEL = SMPLModel.synthetic(V, 93)


def mesh_net(seed=31):
    from motionbert_amd.mesh import MeshRegressor
    torch.manual_seed(seed)
    smpl = SMPLLayer(MODEL)
    pose, shape = ME.mean_params()
    net = MeshRegressor(build_model(CFG), smpl=smpl, init_pose=pose, init_shape=shape, J_regressor=smpl.J_regressor_h36m, dim_rep=128,
                        hidden_dim=HIDDEN, dropout_ratio=0.).to(DEV)
    net.backbone.precision = 'fp32'
    return net


@pytest.fixture(scope='module')
def packed(tmp_path_factory):
    """the synthetic 3DPW detection file of meshgterr.make_pickle, packed: 4 training and 3 test clips of 8 frames"""
    from motionbert_amd.data import pack_mesh
    root = tmp_path_factory.mktemp('mesh_gt')
    path = str(root / 'pw3d.pkl')
    with open(path, 'wb') as f:
        pickle.dump(GE.make_pickle('pw3d', GE.PACK_SEED['pw3d']), f)
    for split in ('train', 'test'):
        pack_mesh(path, 'pw3d', split, 8, 4, str(root / split))
    return str(root)


def reference_targets(gt, dtype):
    """the targets of a batch from the plain path in `dtype` on the batch's own theta (exact), rounded to fp32 on the device"""
    kp, verts = GE.body_targets(MODEL, gt['theta'].cpu(), dtype)
    return {'theta': gt['theta'], 'kp_3d': kp.float().to(DEV), 'verts': verts.float().to(DEV)}


def test_packed_mesh_into_the_step_for_two_steps(packed):
    """The loss of a step on the device's targets equals the loss on targets built by the float64 plain path within the standing gate of
    tests/mesherr.py: 4 x what targets built by the same path in float32 show, never less than 8 fp32 ulps.  All three losses come from
    the same forward output, so nothing but the targets differs."""
    from motionbert_amd.data import PackedMesh
    from motionbert_amd.mesh import LOG_KEYS, MeshLoss, MeshStep
    net = mesh_net(seed=37).train()
    step = MeshStep(net, lr_backbone=1e-4, lr_head=1e-3, weight_decay=0.01, lambdas=ME.Lambdas, loss_type='L1')
    crit = MeshLoss(loss_type='L1', lambdas=ME.Lambdas)
    ds = PackedMesh(os.path.join(packed, 'train'), net.head.smpl, device=DEV, train=True)
    logs = []
    for k, (x, gt) in enumerate(ds.batches(batch_size=2, shuffle=True, epoch=0, seed=21)):
        assert x.shape == (2, 8, 17, 3) and x.is_cuda and gt['verts'].shape == (2, 8, V, 3) and gt['kp_3d'].shape == (2, 8, 17, 3)
        out = net(x)
        total = {name: float(crit(out, tgt)['total'].detach()) for name, tgt in (('device', gt), ('f64', reference_targets(gt, torch.float64)),
                                                                        ('f32', reference_targets(gt, torch.float32)))}
        gate = ME.gate32(abs(total['f32'] - total['f64']) / abs(total['f64']))
        s = abs(total['device'] - total['f64']) / abs(total['f64'])
        print(f'e2e.step{k}: total {total["device"]:.6f} against {total["f64"]:.6f}: stat {s:.3e} gate {gate:.3e}')
        REPORT.setdefault('e2e.step', {})[f'total{k}'] = s / gate
        log = step(x, gt)
        assert log.shape == (len(LOG_KEYS),) and bool(torch.isfinite(log).all())
        assert s <= gate
        assert abs(float(log[LOG_KEYS.index('total')]) - total['device']) <= ME.FLOOR * abs(total['device']), 'the step computes this loss'
        logs.append(log.clone())
    assert len(logs) == 2 and not torch.equal(logs[0], logs[1])


def test_packed_mesh_into_the_evaluator(packed):
    from motionbert_amd.data import PackedMesh
    from motionbert_amd.mesh import MeshEvaluator
    net = mesh_net(seed=39).eval()
    ds = PackedMesh(os.path.join(packed, 'test'), net.head.smpl, device=DEV, train=False)
    stored = np.load(os.path.join(packed, 'test.pose.npy'))
    ev, outs, refs, seen = MeshEvaluator(), [], [], 0
    for epoch in range(2):                      # train=False never flips, whatever the epoch and seed
        for x, gt in ds.batches(batch_size=2, shuffle=False, epoch=epoch, seed=epoch):
            assert torch.equal(gt['theta'][..., :72].cpu(), torch.from_numpy(stored[seen % 3:seen % 3 + x.shape[0]]))
            seen += x.shape[0]
            if epoch:
                continue
            with torch.no_grad():
                out = net(x)
            ev.update(out, gt)
            outs.append({k: v.double().cpu() for k, v in out[0].items()})
            refs.append(dict(zip(('kp_3d', 'verts'), GE.body_targets(MODEL, gt['theta'].cpu(), torch.float64))))
    assert seen == 6 and ev.count == 24
    res = ev.finish()
    cat = lambda rows, k, w: torch.cat([r[k] for r in rows]).reshape(-1, w, 3).numpy()      # noqa: E731
    ref = ME.aggregate(ME.mesh_errors64(cat(outs, 'verts', V), cat(refs, 'verts', V), cat(outs, 'kp_3d', 17), cat(refs, 'kp_3d', 17)))
    # the gate of test_gpu_smpl.py's evaluator test: a target vertex or joint is off by at most gate x max |value|; a mean of distances
    # then moves by at most sqrt(3) times that, the aligned ones by a small multiple of it: 4 x as the margin
    theta = torch.cat([torch.from_numpy(stored), torch.from_numpy(np.load(os.path.join(packed, 'test.shape.npy')))], -1)
    ref64, gate = GE.gates(MODEL, theta)
    tol = 4.0 * math.sqrt(3.0) * gate['verts'] * float(ref64['verts'].abs().max())
    for k in ref:
        print(f'e2e.evaluator {k}: {res[k]:.6f} against {ref[k]:.6f} (tolerance {tol:.2e})')
        REPORT.setdefault('e2e.evaluator', {})[k] = abs(res[k] - ref[k]) / tol
        assert abs(res[k] - ref[k]) <= tol, k
