"""In-the-wild inference on a real MI355X (csrc/wild.hip, motionbert_amd/wild.py): mbx_wild_input against the reference's own output
(tests/golden/wild.npz, tools/mint_wild.py), mbx_wild_output and `wild.infer` against the restatements of tests/wilderr.py (its own
checks on the CPU: tests/test_wilderr.py, tests/test_wild.py).

Gates.  Both kernels: EQUAL BITS, outputs NaN-filled beforehand, guard rows around them untouched (wilderr's module docstring says why
bit equality is the right gate).  `infer` against the output stage restated in numpy on the very network outputs it used: equal bits.
`infer` against the reference's batch-1 loop (infer_wild.py:66-88: two forwards and flip_data per clip) through the same model: the
network runs at another batch size and the flip is folded into one forward, so the gate is the one tests/test_gpu_augment.py:76 applies to
that comparison, 1e-6 absolute on normalised output, times min(w, h) / 2 in pixel mode.  What was measured goes to wild_parity.json / .txt
in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import wilderr as WE
from tests.helpers import build_model, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
L = WE.CLIP_LEN
VID = (1920, 1080)
GATE = 1e-6
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'wild_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'wild_parity.txt'), 'w') as f:
        f.write('in-the-wild inference: elements whose bits differ from the reference / the restatement (0 passes), and the worst\n'
                f'absolute difference of wild.infer from the batch-1 loop of infer_wild.py as a share of its gate {GATE:g} (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + '  '.join(f'{n} {v:.4g}' if isinstance(v, float) else f'{n} {v}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


@pytest.fixture(scope='module')
def fixture():
    return WE.load_fixture()


@pytest.fixture(scope='module')
def cases():
    return WE.input_cases()


@pytest.fixture(scope='module')
def model():
    zt, cfg = load_golden('tiny_trained')
    m = build_model(cfg)
    m.load_state_dict({k[2:]: torch.from_numpy(zt[k]) for k in zt.files if k.startswith('w.')}, strict=True)
    m.precision = 'fp32'
    assert m.maxlen >= L
    return m.to(DEV).eval()


# ------------------------------------------------------------------------------------------------ mbx_wild_input
@pytest.mark.parametrize('name', list(WE.input_cases()))
def test_wild_input_equals_the_reference_bit_for_bit(ops, fixture, cases, name):
    res = WE.input_check(ops, DEV, cases[name], fixture[f'in.{name}.out'], fixture[f'in.{name}.box'])
    print(name, res)
    REPORT['input.' + name] = {k: int(v) for k, v in res.items()}
    assert WE.passes(res), (name, res)


def test_wild_input_tracks_in_one_call(ops, fixture):
    """three interleaved persons as one call: every track its own box; and a track without frames between them"""
    its, keys = WE.persons_cases()
    tracks = WE.case_kp(dict(items=its, focus=None), by_track=True)
    kp = np.concatenate(list(tracks.values()))
    lens = [len(tracks[keys[0]]), 0, len(tracks[keys[1]]), len(tracks[keys[2]])]
    for mode, vid, rng in (('crop', None, [1, 1]), ('pixel', VID, None)):
        y, box, clean = WE.run_input(ops, DEV, kp, lens, vid, rng)
        d_out = WE.differing(y, np.concatenate([fixture[f'in.persons.{mode}.focus{k}.out'] for k in keys]))
        d_box = WE.differing(box[[0, 2, 3]], np.stack([fixture[f'in.persons.{mode}.focus{k}.box'] for k in keys]))
        REPORT['input.tracks.' + mode] = dict(out=d_out, box=d_box, clean=int(clean))
        assert d_out == 0 and d_box == 0 and clean and box[1].tolist() == [0, 0, 0, 0]
    # many chunks per track and more tracks than one wave has lanes: the long case repeated, every copy its own track
    case = fixture['in.chunk.%d.first.out' % (2 * WE.CHUNK + 1)]
    one = WE.case_kp(WE.input_cases()['chunk.%d.first' % (2 * WE.CHUNK + 1)])
    S = 70
    y, box, clean = WE.run_input(ops, DEV, np.concatenate([one] * S), [len(one)] * S, None, [1, 1])
    d_out = WE.differing(y, np.concatenate([case] * S))
    REPORT['input.tracks.70'] = dict(out=d_out, clean=int(clean))
    assert d_out == 0 and clean and WE.differing(box, np.stack([fixture['in.chunk.%d.first.box' % (2 * WE.CHUNK + 1)]] * S)) == 0


# ------------------------------------------------------------------------------------------------ mbx_wild_output
@pytest.mark.parametrize('name', list(WE.output_cases()))
def test_wild_output_equals_the_restatement_bit_for_bit(ops, name):
    res = WE.output_check(ops, DEV, WE.output_cases()[name])
    print(name, res)
    REPORT['output.' + name] = {k: int(v) for k, v in res.items()}
    assert res == dict(out=0, clean=True, pred_kept=True), (name, res)


# ------------------------------------------------------------------------------------------------ wild.infer
class Recorder:
    """the model, with every network input and output of the run kept"""

    def __init__(self, model):
        self.model, self.num_joints, self.maxlen, self.seen = model, model.num_joints, model.maxlen, []

    def parameters(self):
        return self.model.parameters()

    def eval(self):
        self.model.eval()
        return self

    def forward(self, x, return_rep=False):
        out = self.model.forward(x, return_rep=return_rep)
        self.seen.append((x.clone(), out.clone()))
        return out

    __call__ = forward


def _restated_output(plan_batches, seen, F, rootrel, gt_2d, vid_size):
    """the output stage of infer_wild.py:81-96 in numpy on the recorded network outputs, stitched by the plan"""
    out = np.full((F, 17, 3), np.nan, dtype=np.float32)
    for offs, (x, pred) in zip(plan_batches, seen):
        p = WE.output_eq(pred.cpu().numpy(), x.cpu().numpy(), rootrel, gt_2d)
        for i, o in enumerate(offs):
            out[o:o + p.shape[1]] = p[i]
    return WE.pixel_eq(out, vid_size) if vid_size else out


@pytest.mark.parametrize('flip,rootrel,gt_2d,no_conf,pixel', [(True, False, False, False, False), (False, True, True, False, False),
                                                              (True, False, False, False, True), (True, True, True, False, True),
                                                              (False, False, True, False, True)])
def test_infer_with_the_real_model(model, flip, rootrel, gt_2d, no_conf, pixel):
    from motionbert_amd import wild
    tag = f'flip{int(flip)}.rootrel{int(rootrel)}.gt2d{int(gt_2d)}.pixel{int(pixel)}'
    F, mb = 4 * L + 3, 3
    kp = WE.detections(F, 8600)
    rec = Recorder(model)
    got = wild.infer(rec, kp, clip_len=L, vid_size=VID, pixel=pixel, flip=flip, rootrel=rootrel, gt_2d=gt_2d, no_conf=no_conf, max_batch=mb)
    assert isinstance(got, np.ndarray) and got.shape == (F, 17, 3) and got.dtype == np.float32 and np.isfinite(got).all()
    batches = [offs[b:b + mb] for _, offs in wild.clip_plan([F], L) for b in range(0, len(offs), mb)]
    assert [tuple(x.shape[:2]) for x, _ in rec.seen] == [(3, L), (1, L), (1, 3)]
    # (a) the output stage, restated, on the very outputs the run used: equal bits
    d = WE.differing(got, _restated_output(batches, rec.seen, F, rootrel, gt_2d, VID if pixel else None))
    # (b) the reference's loop through the same model: batch 1, two forwards, flip_data
    motion = WE.input_ref(kp, VID if pixel else None, None if pixel else [1, 1])[0]
    assert WE.differing(torch.cat([x.reshape(-1, 17, 3) for x, _ in rec.seen]).cpu().numpy(), motion) == 0      # the network saw read_input's bits
    want = WE.reference_loop(model, motion, L, flip, rootrel, gt_2d, no_conf, VID if pixel else None, device=DEV)
    assert want.shape == got.shape and float(want[..., 2].std()) > 1e-3                                        # a network output, not a constant
    gate = GATE * (min(VID) / 2.0 if pixel else 1.0)
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f'{tag}: output stage {d} differing elements; worst difference from the batch-1 loop {worst:.3e} (gate {gate:.3e})')
    REPORT['infer.' + tag] = dict(output_stage=d, loop_share=worst / gate, loop_worst=worst)
    assert d == 0
    assert worst <= gate, (tag, worst, gate)


def test_infer_dict_form_equals_single_track_calls(model):
    from motionbert_amd import wild
    its, keys = WE.persons_cases()
    tracks = WE.case_kp(dict(items=its, focus=None), by_track=True)
    # max_batch 2: the pooled run forms the batches the single-track runs form; 64: the three full clips of two persons share one batch
    for pixel, mb in ((False, 2), (True, 2), (False, 64), (True, 64)):
        both = wild.infer(model, tracks, clip_len=L, vid_size=VID, pixel=pixel, max_batch=mb)
        assert list(both) == keys
        worst = 0
        for k in keys:
            single = wild.infer(model, tracks[k], clip_len=L, vid_size=VID, pixel=pixel, max_batch=mb)
            worst = max(worst, WE.differing(both[k], single))
        REPORT[f'infer.dict.pixel{int(pixel)}.max_batch{mb}'] = dict(differing=worst)
        assert worst == 0, (pixel, mb, worst)
    # a DataParallel-wrapped model and device-resident detections
    dp = torch.nn.DataParallel(model, device_ids=[0])
    k = keys[1]
    a = wild.infer(dp, torch.from_numpy(tracks[k]).to(DEV), clip_len=L, flip=False)
    assert WE.differing(a, wild.infer(model, tracks[k], clip_len=L, flip=False)) == 0
    with pytest.raises(ValueError, match='maxlen'):
        wild.infer(model, tracks[k], clip_len=model.maxlen + 1)
