"""tests/actionerr.py on the CPU: its float64 restatements against the reference's own code (tests/golden/action.npz, tools/mint_action.py),
`data.pack_action` against the reference's `ActionDataset.motions`, the gates against seeded corruptions, and the conditions the input
cases must meet for the GPU parity test to mean what it says."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import actionerr as AE
from tests.helpers import GOLDEN


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'action.npz'))


@pytest.fixture(scope='module')
def cases():
    return AE.input_cases()


# ------------------------------------------------------------------------------------------------ the restatements are the reference
def test_input_restatement_reproduces_the_reference(fixture, cases):
    """random_move + crop_scale of the reference on float64 inputs, every case, every kept frame: 1e-12"""
    assert len(cases) == len(AE.INPUT_SHAPES) + 5
    for name, (x, flags, _) in cases.items():
        p = torch.from_numpy(fixture[name + '.params'])
        ref, zeroed, _ = AE.action_input_ref64(x, p, flags)
        want = torch.from_numpy(fixture[name + '.out'])
        got = ref[:, :, torch.from_numpy(fixture[name + '.frames'])]
        assert got.shape == want.shape, name
        err = float((got - want).abs().max())
        print(f'{name}: max |restatement - reference| {err:.3e}')
        assert err <= 1e-12, (name, err)
        wz = (want == 0).reshape(len(want), -1).all(1)
        assert torch.equal(wz, zeroed | (ref == 0).reshape(len(ref), -1).all(1)), name


def test_xent_restatement_reproduces_the_reference(fixture):
    """CrossEntropyLoss, its autograd gradient and accuracy(topk=(1, 5)) of the reference: 1e-12, hit counts exactly"""
    for shape in AE.XENT_SHAPES:
        z, lab = AE.logit_inputs(*shape, AE.xent_seed(shape))
        r = AE.xent_topk_ref64(z, lab)
        tag = 'xe.%d.%d' % shape
        assert abs(float(r['loss']) - float(fixture[tag + '.loss'])) <= 1e-12 * max(1.0, abs(float(fixture[tag + '.loss']))), tag
        rows = torch.from_numpy(fixture[tag + '.rows'])
        assert float((r['d'][rows] - torch.from_numpy(fixture[tag + '.dlogits'])).abs().max()) <= 1e-12, tag
        n = shape[0]
        acc = fixture[tag + '.acc']                       # percent, computed by the reference in float32
        assert [round(float(a) * n / 100) for a in acc] == [r['hit1'], r['hit5']], tag
        assert np.allclose([100.0 * r['hit1'] / n, 100.0 * r['hit5'] / n], acc, rtol=1e-6, atol=0), tag
    hits = [AE.xent_topk_ref64(*AE.logit_inputs(*s, AE.xent_seed(s))) for s in AE.XENT_SHAPES]
    assert any(0 < h['hit1'] < h['hit5'] < len(h['rank']) for h in hits), 'the fixture needs a case with top-1 hits, further top-5 hits and misses'


def test_pack_action_reproduces_the_reference_bit_for_bit(fixture, tmp_path):
    from motionbert_amd import data
    anns = []
    for i in range(len(AE.ANN_FRAMES)):
        label, total, h, w = (int(v) for v in fixture[f'ann.{i}.meta'])
        anns.append(dict(frame_dir='S%03d' % i, label=label, total_frames=total, img_shape=(h, w), keypoint=fixture[f'ann.{i}.keypoint'],
                         keypoint_score=fixture[f'ann.{i}.keypoint_score']))
    made = AE.annotations()
    assert all(np.array_equal(a['keypoint'], b['keypoint']) and np.array_equal(a['keypoint_score'], b['keypoint_score']) for a, b in zip(anns, made))
    pkl = str(tmp_path / 'ntu.pkl')
    with open(pkl, 'wb') as f:
        pickle.dump(AE.annotation_file(anns), f)
    for split in AE.ANN_SPLITS:
        prefix = str(tmp_path / split)
        meta = data.pack_action(pkl, split, AE.ANN_N_FRAMES, prefix)
        motion, label = np.load(prefix + '.motion.npy'), np.load(prefix + '.label.npy')
        want = fixture[f'ann.{split}.motions']
        assert motion.dtype == np.float32 and motion.shape == want.shape == (len(AE.ANN_SPLITS[split]), 2, AE.ANN_N_FRAMES, 17, 3)
        assert motion.tobytes() == want.tobytes(), split
        assert np.array_equal(label, fixture[f'ann.{split}.labels']) and label.dtype == np.int64
        assert meta['n'] == len(want) and meta['train'] == ('train' in split)
    # the train split draws, the validation split does not; single-person samples get an all-zero second person
    tr, va = fixture['ann.xsub_train.motions'], fixture['ann.xsub_val.motions']
    assert not np.array_equal(tr[3], va[2]), 'sample 5 is in both splits: resampled at random in one, evenly in the other'
    assert not tr[0, 1].any() and tr[1, 1].any()
    with pytest.raises(ValueError, match='no split'):
        data.pack_action(pkl, 'xview_train', AE.ANN_N_FRAMES, str(tmp_path / 'x'))
    # check_split=False: every sample, drawn as a training split (NTURGBD1Shot's constructor)
    meta = data.pack_action(pkl, 'anything', AE.ANN_N_FRAMES, str(tmp_path / 'all'), check_split=False)
    assert meta['n'] == len(AE.ANN_FRAMES) and meta['train']


# ------------------------------------------------------------------------------------------------ the gates
def test_float32_equations_and_the_torch_provider_pass_every_gate(fixture, cases):
    ops = AE.TorchActionOps()
    for name, (x, flags, crop) in cases.items():
        p = AE.case_params(fixture, name)
        y32 = AE.action_input_eq(x, p, flags, torch.float32)[0]
        share, same, _ = AE.input_gate(y32, x, p, flags)
        assert same and share <= 1 / AE.FACTOR + 1e-12, (name, share)
        y = torch.empty_like(x)
        ops.action_input(x, y, p, None, AE.RANGES + (crop,), flags, 0)
        share, same, _ = AE.input_gate(y, x, p, flags)
        assert same and share <= 0.5, (name, share)
    for z, lab in [AE.logit_inputs(*s, AE.xent_seed(s)) for s in AE.XENT_SHAPES] + [AE.planted_logits(), AE.bad_label_logits()]:
        r32 = AE.xent_topk_eq(z, lab, torch.float32, 1.0)
        got = AE.xent_check(torch.stack([r32['loss'], torch.tensor(float(r32['hit1'])), torch.tensor(float(r32['hit5']))]), r32['d'], z, lab)
        assert got['exact'] and got['loss'] <= 1 and got['grad'] <= 1 / AE.FACTOR + 1e-12, got


@pytest.mark.parametrize('corrupt', AE.INPUT_CORRUPTIONS)
def test_every_input_corruption_fails_a_gate(fixture, cases, corrupt):
    """a float32 evaluation with one thing wrong, through the gate the kernel goes through: at least one case must fail"""
    failed = []
    for name, (x, flags, _) in cases.items():
        p = AE.case_params(fixture, name)
        bad = AE.action_input_eq(x, p, flags, torch.float32, corrupt)[0]
        share, same, _ = AE.input_gate(bad, x, p, flags)
        if share > 1 or not same:
            failed.append((name, share, same))
    print(corrupt, failed)
    assert failed, f'{corrupt}: no case notices'
    expect = {'second_person_still': 'in.2.2.243', 'no_end_point': 'in.2.2.2', 'box_over_all': 'in.2.2.243', 'div_ratio': 'in.clip',
              'conf_unclipped': 'in.planted', 'threshold_3': 'in.planted'}[corrupt]
    assert expect in [f[0] for f in failed], (corrupt, failed)


@pytest.mark.parametrize('corrupt', AE.XENT_CORRUPTIONS)
def test_every_loss_corruption_fails_a_gate(corrupt):
    failed = []
    for tag, (z, lab) in [('seeded', AE.logit_inputs(32, 60, AE.xent_seed((32, 60)))), ('planted', AE.planted_logits())]:
        bad = AE.xent_topk_eq(z, lab, torch.float32, 1.0, corrupt)
        got = AE.xent_check(torch.stack([bad['loss'], torch.tensor(float(bad['hit1'])), torch.tensor(float(bad['hit5']))]), bad['d'], z, lab)
        if not got['exact'] or got['loss'] > 1 or got['grad'] > 1:
            failed.append(tag)
    assert failed == {'no_div_n': ['seeded', 'planted'], 'ge_rank': ['planted']}[corrupt], (corrupt, failed)


def test_gate_floors_are_positive_where_float32_is_exact():
    """a row float32 gets exactly (two equal scores: softmax 1/2, loss log 2 both ways) still has a gate, and it is the floor"""
    z, lab = torch.zeros(1, 2), torch.tensor([0])
    _, g_row, g_mean, g_d = AE.xent_gates(z, lab)
    assert float(g_row[0]) == AE.FLOOR and g_mean > 0 and float(g_d[0]) == AE.FLOOR * 0.5
    x = torch.zeros(1, 1, 1, 4, 3)
    x[0, 0, 0, :, :2] = torch.tensor([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]])
    x[..., 2] = 1.0
    p = torch.tensor([[0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    y32 = AE.action_input_eq(x, p, 3, torch.float32)[0]
    assert torch.equal(y32.double(), AE.action_input_ref64(x, p, 3)[0])
    share, same, _ = AE.input_gate(y32 + 4 * AE.EPS32, x, p, 3)
    assert same and 0 < share <= 1


# ------------------------------------------------------------------------------------------------ what the cases must be
def test_input_cases_meet_their_conditions(fixture, cases):
    for name, (x, flags, crop) in cases.items():
        p = AE.case_params(fixture, name)
        if flags & AE.MOVE:
            for k, (a, b) in enumerate((AE.RANGES[0], AE.RANGES[1], AE.RANGES[2], AE.RANGES[2])):
                assert bool(((p[:, 2 * k:2 * k + 2] >= a) & (p[:, 2 * k:2 * k + 2] <= b)).all()), name
        assert bool(((p[:, 8] >= crop[0]) & (p[:, 8] <= crop[1])).all()), name
        if flags & AE.CROP:
            frac = AE.clipped_fraction(x, p, flags)
            print(f'{name}: {100 * frac:.2f} % of the coordinates are clipped')
            assert frac >= 0.05 if name == 'in.clip' else frac <= 0.01, (name, frac)
    x, flags, _ = cases['in.planted']
    y, zeroed, _ = AE.action_input_ref64(x, AE.case_params(fixture, 'in.planted'), flags)
    assert zeroed.tolist() == [True, True, False, True, False, False, False], 'all-zero confidence, 3 valid, 4 valid, coincident, ...'
    assert int((x[1, ..., 2] != 0).sum()) == 3 and int((x[2, ..., 2] != 0).sum()) == 4
    assert not x[4, 1].any() and bool(y[4, 1, ..., :2].abs().max() > 0), 'the all-zero second person is moved off the origin'
    assert float(x[5, ..., 2].max()) == 1.5 and float(y[5, ..., 2].max()) == 1.0 and float(y[5, ..., 2].min()) == -1.0
    x, flags, _ = cases['in.2.2.243']
    assert int((x[..., 2] == 0).sum()) >= 4, 'undetected joints outside the box: what box_over_all gets wrong'
    # seeded draws: inside the ranges, the kernel's arithmetic restated
    d = AE.draw_params(64, 12345, AE.CROP_CLIP)
    for k in range(9):
        a, b = AE.RANGES[k // 2] if k < 4 else AE.RANGES[2] if k < 8 else AE.CROP_CLIP
        assert float(d[:, k].min()) >= np.float32(a) and float(d[:, k].max()) <= np.float32(b) and len(torch.unique(d[:, k])) > 32


def test_planted_logits_are_what_they_claim():
    z, lab = AE.planted_logits()
    r = AE.xent_topk_ref64(z, lab)
    rank = r['rank'].tolist()
    assert rank[:2] + rank[3:8] == [0, z.shape[1] - 1, 4, 5, 0, 1, 5] and rank[2] >= 1
    assert float(r['row_loss'][1]) > 160 and float(r['row_loss'][2]) > 9000 and bool(torch.isfinite(r['row_loss']).all())
    zb, lb = AE.bad_label_logits()
    rb = AE.xent_topk_ref64(zb, lb)
    assert torch.isnan(rb['row_loss']).tolist() == [True, False, True, False] and bool(torch.isnan(rb['loss']))
    assert torch.isnan(rb['d']).all(1).tolist() == [True, False, True, False]
