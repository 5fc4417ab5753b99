"""In-the-wild mesh recovery on a real MI355X (mbx_wild_mesh in csrc/smpl.hip, mbx_scale_fit and mbx_wild_mesh_place in csrc/wild.hip,
motionbert_amd.wild.infer_mesh): the gates of tests/wildmesherr.py (its own checks on the CPU: tests/test_wildmesherr.py,
tests/test_wild_mesh.py) applied to the kernels.

Gates.  mbx_wild_mesh, single pass: equal bits with SMPLLayer.forward_kp on the same inputs, stitched; theta and mbx_wild_mesh_place: equal
bits with the numpy restatement; pair mode: per array max |error| / max |float64 value| at most 4 x what the float32 plain path shows against
itself in float64 on the same inputs (floor 8 fp32 ulps), computed on the CPU when the test runs.  mbx_scale_fit: (a) the float64 objective
of its (s, t) no greater than the reference's own best fun (tests/golden/wild_mesh.npz) plus N 2^-53 relative; (b) scale, t and objective
within 1e-10 of the float64 IRLS run to 1e-16; (c) pooled and single-track calls give equal bits.  Outputs are NaN-filled beforehand and
guard rows checked.  `infer_mesh` against `mesh.flip_average` on the very batches the run formed: the pair-mode gate.  What was measured
goes to wild_mesh_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import os
import time
from collections import OrderedDict

import numpy as np
import pytest
import torch

from motionbert_amd.smpl import SMPLLayer, SMPLModel
from tests import mesherr as ME
from tests import smplerr as SE
from tests import wilderr as WE
from tests import wildmesherr as WM
from tests.helpers import build_model, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
L = WE.CLIP_LEN
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


def _fmt(v):
    return f'{v:.4g}' if isinstance(v, float) else str(v)


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'wild_mesh_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'wild_mesh_parity.txt'), 'w') as f:
        f.write('in-the-wild mesh recovery.  mesh.* / infer.*: error as a share of its gate (4 x the float32 plain path against float64, floor 8 ulps;\n'
                '<= 1 passes; head-room = 1 / share), `differing`: elements whose bits differ (0 passes).  fit.*: `b` = worst of scale / t / objective\n'
                'against the float64 IRLS run to 1e-16, as a share of 1e-10 (<= 1 passes); `a` = (objective - the reference\'s best fun) over the rounding\n'
                'bound N 2^-53 (<= 1 passes; negative: below the reference\'s best); `below_reference`: that margin, relative.\n')
        for k in sorted(REPORT):
            f.write(f'{k:34s} ' + '  '.join(f'{n} {_fmt(v)}' for n, v in sorted(REPORT[k].items()) if v is not None) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


@pytest.fixture(scope='module')
def fixture():
    return WM.load_fixture()


# ------------------------------------------------------------------------------------------------ mbx_wild_mesh
# V = 65: one full vertex tile plus one vertex; 3 x 3 frames: less than a workgroup's; 4 x 8 = 32 frames: exactly the frames of one
# workgroup in single-pass mode (4 waves x 8) and of two in pair mode (4 waves x 4)
@pytest.mark.parametrize('V,n,T', [(65, 3, 3), (65, 4, 8), (6890, 3, 3), (6890, 4, 8)])
def test_wild_mesh_kernels(ops, V, n, T):
    case = WM.mesh_case(V, n, T, 8700 + V % 100 + n)
    assert sorted(case['dst']) != list(case['dst']) and case['F'] > n * T          # out of order, with a gap
    rep = {}
    failed = WM.mesh_gate_run(ops, DEV, case, rep)
    REPORT[f'mesh.V{V}.{n}x{T}'] = dict(rep, failed=len(failed))
    print(V, n, T, rep, failed)
    assert failed == []


def test_wild_mesh_is_repeatable_and_leaves_unknown_clips_alone(ops):
    case = WM.mesh_case(65, 3, 3, 8710)
    layer = SMPLLayer(case['model']).to(DEV)
    a, b = WM.run_mesh(ops, DEV, layer, case, True), WM.run_mesh(ops, DEV, layer, case, True)
    assert all(WE.differing(a[k], b[k]) == 0 for k in ('verts', 'kp', 'theta'))
    # a device entry that does not fit (the host's dst_max says otherwise) skips its clip: nothing is written out of bounds
    bad = dict(case, dst=case['dst'].copy())
    bad['dst'][int(np.argmin(case['dst']))] = -5
    c = WM.run_mesh(ops, DEV, layer, bad, True)
    lost = int(case['dst'].min())
    assert c['clean'] and np.isnan(c['verts'][lost:lost + 3]).all() and np.isnan(c['kp'][lost:lost + 3]).all() and np.isnan(c['theta'][lost:lost + 3]).all()
    keep = np.ones(case['F'], bool)
    keep[lost:lost + 3] = False
    assert all(WE.differing(a[k][keep], c[k][keep]) == 0 for k in ('verts', 'kp', 'theta'))
    REPORT['mesh.repeat'] = dict(differing=0)


# ------------------------------------------------------------------------------------------------ mbx_scale_fit, mbx_wild_mesh_place
def test_scale_fit(ops, fixture):
    rep = {}
    failed = WM.fit_gate_run(ops, DEV, fixture, WM.PROBLEMS + (WM.LARGE,), rep)
    for k, v in rep.items():
        REPORT[k] = {n: (float(x) if x is not None else None) for n, x in v.items()}
    print(rep, failed)
    assert failed == []
    for name in WM.FIXTURE_PROBLEMS:
        assert rep[f'fit.{name}']['a'] is not None


@pytest.mark.parametrize('V', [65, 6890])
def test_place_equals_the_restatement_bit_for_bit(ops, V):
    d = WM.place_gate_run(ops, DEV, V)
    REPORT[f'place.V{V}'] = dict(differing=d)
    assert d == 0


# ------------------------------------------------------------------------------------------------ infer_mesh
@pytest.fixture(scope='module')
def net():
    from motionbert_amd.mesh import MeshRegressor
    zt, cfg = load_golden('tiny_trained')
    m = build_model(cfg)
    m.load_state_dict({k[2:]: torch.from_numpy(zt[k]) for k in zt.files if k.startswith('w.')}, strict=True)
    m.precision = 'fp32'
    assert m.maxlen >= L
    torch.manual_seed(41)
    smpl = SMPLLayer(SMPLModel.synthetic(6890, 9))
    pose, shape = ME.mean_params()
    net = MeshRegressor(m, smpl=smpl, init_pose=pose, init_shape=shape, J_regressor=smpl.J_regressor_h36m, dim_rep=m.dim_rep, hidden_dim=64,
                        dropout_ratio=0.)
    with torch.no_grad():
        net.head.head_pose.weight.mul_(40.0)               # the mean parameters alone give every frame the same pose
        net.head.head_shape.weight.mul_(40.0)
    return net.to(DEV).eval()


class _Recording(torch.nn.Module):
    """records the batches the backbone saw"""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []
        self.maxlen = inner.maxlen

    def get_representation(self, x):
        self.seen.append(x.detach().clone())
        return self.inner.get_representation(x)


def _ref_motion(F, seed):
    r = np.random.RandomState(seed)
    return r.normal(0, 0.25, (1, 17, 3)) + r.normal(0, 0.03, (F, 17, 3)) + np.cumsum(r.normal(0, 0.02, (F, 1, 3)), axis=0)


@pytest.mark.parametrize('pixel', [False, True])
def test_infer_mesh_against_flip_average_on_its_own_batches(net, pixel):
    from motionbert_amd import wild
    from motionbert_amd.mesh import flip_average
    kp = WE.detections(2 * L + 4, 8720)
    smpl = net.head.smpl
    backbone = net.backbone
    rec = _Recording(backbone)
    net.backbone = rec
    try:
        got = wild.infer_mesh(net, smpl, kp, clip_len=L, vid_size=(1920, 1080), pixel=pixel, want=('verts', 'kp_3d', 'theta'))
    finally:
        net.backbone = backbone
    batches = rec.seen[0::2]                               # x, flip_input(x) alternate
    assert [tuple(b.shape[:2]) for b in batches] == [(2, L), (1, 4)] and len(rec.seen) == 4
    want = {k: [] for k in ('verts', 'kp_3d', 'theta')}
    params = dict(rot_a=[], betas_a=[], theta_a=[], theta_b=[])
    with torch.no_grad():
        for x, xf in zip(batches, rec.seen[1::2]):
            out = flip_average(net, smpl, x)[0]
            for k in want:
                want[k].append(out[k].reshape((-1,) + out[k].shape[2:]))
            n, T = x.shape[:2]
            ra, ba, ta = net.head.forward_params(backbone.get_representation(x).reshape(n, T, 17, -1))
            tb = net.head.forward_params(backbone.get_representation(xf).reshape(n, T, 17, -1))[2]
            for k, v in zip(params, (ra, ba, ta, tb)):
                params[k].append(v.float().cpu())
    want = {k: torch.cat(v).cpu().numpy() for k, v in want.items()}          # the batches are consecutive clips in frame order
    case = {k: torch.cat(v) for k, v in params.items()}
    model = SMPLModel.synthetic(6890, 9)
    ref64, gate = WM.pair_gates(model, case)
    rep = dict(verts_vs_flip_average=SE.stat(got['verts'], want['verts'].astype(np.float64)) / gate['verts'],
               kp_vs_flip_average=SE.stat(got['kp_3d'], want['kp_3d'].astype(np.float64)) / gate['kp'],
               verts_vs_float64=SE.stat(got['verts'], ref64['verts']) / gate['verts'], kp_vs_float64=SE.stat(got['kp_3d'], ref64['kp']) / gate['kp'],
               theta_differing=WE.differing(got['theta'], WM.theta_pair(case['theta_a'].numpy(), case['theta_b'].numpy())[0]))
    REPORT[f'infer.pixel{int(pixel)}'] = rep
    print(rep)
    assert all(v <= 1.0 for k, v in rep.items() if k != 'theta_differing') and rep['theta_differing'] == 0, rep


def test_infer_mesh_dict_form_equals_single_track_runs(net):
    from motionbert_amd import wild
    its, keys = WE.persons_cases()
    tracks = WE.case_kp(dict(items=its, focus=None), by_track=True)
    refs = OrderedDict((k, _ref_motion(len(v), 8730 + k)) for k, v in tracks.items())
    smpl = net.head.smpl
    # max_batch 2: the pooled run forms the batches the single-track runs form
    both = wild.infer_mesh(net, smpl, tracks, clip_len=L, ref_3d=refs, max_batch=2)
    assert list(both) == keys
    worst = 0
    for k in keys:
        one = wild.infer_mesh(net, smpl, tracks[k], clip_len=L, ref_3d=refs[k], max_batch=2)
        worst = max(worst, WE.differing(both[k]['verts'], one['verts']), WE.differing(both[k]['kp_3d'], one['kp_3d']),
                    int(np.float64(both[k]['scale']).tobytes() != np.float64(one['scale']).tobytes()))
        assert np.isfinite(one['verts']).all() and one['scale'] > 0
    REPORT['infer.dict'] = dict(differing=worst)
    assert worst == 0
    # device tensors on request, DataParallel-wrapped model, single pass
    dp = torch.nn.DataParallel(net, device_ids=[0])
    dev = wild.infer_mesh(dp, smpl, tracks[keys[1]], clip_len=L, flip=False, to_host=False)
    assert dev['verts'].is_cuda and dev['verts'].shape == (len(tracks[keys[1]]), 6890, 3)
    host = wild.infer_mesh(net, smpl, tracks[keys[1]], clip_len=L, flip=False)
    assert WE.differing(dev['verts'].cpu().numpy(), host['verts']) == 0
    with pytest.raises(ValueError, match='maxlen'):
        wild.infer_mesh(net, smpl, tracks[keys[1]], clip_len=net.backbone.maxlen + 1)
