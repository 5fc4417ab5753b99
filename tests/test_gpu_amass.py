"""mbx_amass_joints (csrc/amass.hip) on the GPU against tests/amasserr.py: the float64 gate per case, run-to-run bits, frame independence,
the camera flag, and pack_amass end to end.  Synthetic models with V = 65: the vertices are folded away, V only shapes the pair list.
The worst error / gate per case goes to amass_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import os
import re
import time

import numpy as np
import pytest
import torch

from motionbert_amd import amass as AM
from motionbert_amd import hip_ops
from motionbert_amd.data import _split_clips
from tests import amasserr as AE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}


def _tile():
    with open(os.path.join(ROOT, 'include', 'mbx.h')) as f:
        return int(re.search(r'#define MBX_AMASS_TILE (\d+)', f.read()).group(1))


TILE = _tile()
FRAMES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
MODELS = ('few', 'sparse', 'dense')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = os.environ.get('MBX_REPORT_DIR') or os.path.join(ROOT, 'reports')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'amass_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, tile=TILE, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'amass_parity.txt'), 'w') as f:
        f.write('mbx_amass_joints against plain_lbs_h in float64: worst error / gate per case (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + ' '.join(f'{o}={v:.4f}' if isinstance(v, float) else f'{o}={v}' for o, v in sorted(REPORT[k].items())) + '\n')


@pytest.fixture(scope='module')
def models():
    m = dict(few=AM.SMPLHModel.synthetic(65, 8750, regressor_support=1), sparse=AM.SMPLHModel.synthetic(65, 8751),
             dense=AM.SMPLHModel.synthetic(65, 8752, dense_weights=True))
    assert m['few'].Np <= 17 * 4 and (3 * m['few'].Np) % 16 != 0          # few pairs, and a last block of rows that is not full
    assert m['few'].Np < m['sparse'].Np <= m['dense'].Np == 17 * 52
    return m


def _run(model, inp, camera=False, fma=False):
    d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
    if fma:
        kp = torch.empty(inp['poses'].shape[0], model.K, 3, dtype=torch.float32, device=DEV)
        hip_ops.get().amass_joints(model.tensors(torch.device(DEV)), d['poses'], d['betas'], d['dmpls'], d['trans'], kp, camera=camera, fma=True)
        return kp.cpu()
    return AM.amass_joints(model, d['poses'], d['betas'], d['dmpls'], d['trans'], camera=camera).cpu()


def _case(mi, fi):
    """the options of a (model, F) case: shared and per-frame betas, dmpls and trans present and null, camera off and on each occur with
    every model among the fifteen cases"""
    n = mi * len(FRAMES) + fi
    return dict(per_frame_betas=bool(n & 1), dmpls=bool(n & 2) or n == 0, trans=not (n & 4)), bool(n % 3 == 1)


@pytest.mark.parametrize('F', FRAMES)
@pytest.mark.parametrize('name', MODELS)
def test_gate_bits_and_frame_independence(models, name, F):
    model = models[name]
    opts, camera = _case(MODELS.index(name), FRAMES.index(F))
    inp = AE.inputs(F, 8760 + 7 * F + MODELS.index(name), max_angle=3.1, trans_scale=3.0, **opts)      # angles from exactly 0 up to near pi
    ref, gate = AE.gates(model, inp, camera)
    got = _run(model, inp, camera)
    ratio = AE.stat(got, ref) / gate
    print(f'{name} Np={model.Np} F={F} {opts} camera={camera}: stat / gate = {ratio:.4f} (gate {gate:.3e})')
    REPORT[f'{name} Np={model.Np} F={F}'] = dict(ratio=ratio, camera=int(camera), **{k: int(v) for k, v in opts.items()})
    assert ratio <= 1.0
    assert torch.equal(got, _run(model, inp, camera))                       # two runs, the same bits
    singles = torch.cat([_run(model, {k: (v if v is None or (k == 'betas' and v.dim() == 1) else v[f:f + 1]) for k, v in inp.items()}, camera)
                         for f in range(F)])
    assert torch.equal(got, singles)                                        # a frame does not depend on the frames it shares a launch with
    plain = got if not camera else _run(model, inp, False)
    cam = (plain.numpy()[..., [0, 2, 1]] * np.array([1, -1, 1], np.float32)) * np.float32(0.298)
    assert np.array_equal(cam, _run(model, inp, True).numpy())              # the camera flag = numpy's two operations on the unflagged output


@pytest.mark.parametrize('name', MODELS)
def test_vector_unit_product_is_inside_the_gate(models, name):
    model = models[name]
    inp = AE.inputs(TILE + 2, 8770, max_angle=3.1, trans_scale=1.0)
    ref, gate = AE.gates(model, inp, True)
    ratio = AE.stat(_run(model, inp, True, fma=True), ref) / gate
    REPORT[f'{name} Np={model.Np} F={TILE + 2} fma'] = dict(ratio=ratio)
    assert ratio <= 1.0


def test_pack_amass_on_the_device(tmp_path):
    tree = str(tmp_path / 'tree')
    AE.write_tree(tree)
    models = AE.tree_models()
    kw = dict(n_frames=9, data_stride=3, max_len=12)
    a, b = str(tmp_path / 'gpu'), str(tmp_path / 'mock')
    meta = AM.pack_amass(tree, models, a, chunk=4, **kw)
    assert meta == AM.pack_amass(tree, models, b, ops=AE.MockOps(), **kw)
    assert open(a + '.json', 'rb').read() == open(b + '.json', 'rb').read()                   # indices, shapes, meta: bit equality
    la, lb = np.load(a + '.label.npy'), np.load(b + '.label.npy')
    assert la.shape == lb.shape and la.dtype == lb.dtype == np.float32
    assert open(a + '.label.npy', 'rb').read(128) == open(b + '.label.npy', 'rb').read(128)   # the .npy header
    seqs, _ = AM.read_amass(tree)
    refs, gate, vid_list, nvid = [], 0.0, [], 0
    for s in seqs:
        inp = dict(poses=torch.from_numpy(s['poses']).float(), betas=torch.from_numpy(s['betas'][:16]).float(),
                   dmpls=torch.from_numpy(s['dmpls'][:, :8]).float(), trans=torch.from_numpy(s['trans']).float())
        r, g = AE.gates(models[AM.pick_gender(s['gender'])], inp, camera=True)
        refs.append(r.numpy())
        gate = max(gate, g)
        for lo, hi in AM.slice_table(len(s['poses']), 12):
            if hi > lo:
                vid_list += [nvid] * (hi - lo)
                nvid += 1
    want = np.concatenate(refs)[np.stack(_split_clips(vid_list, 9, 3, np.random.RandomState(0)))]
    ratio = AE.stat(la, want) / gate
    REPORT['pack_amass tiny tree'] = dict(ratio=ratio, clips=int(la.shape[0]))
    assert ratio <= 1.0
