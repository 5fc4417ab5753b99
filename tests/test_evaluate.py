"""Host logic of motionbert_amd.evaluate without a GPU: the frame -> slots table, the block list, the coverage cases and the
aggregation order, against fixture (b) of tests/golden/eval_h36m.npz (minted from the reference by tools/make_eval_golden.py).
The kernels are replaced by the numpy provider of tests/eval_fixture.py (LAPACK SVD, the reference's own route); the kernels themselves are pinned
in tests/test_gpu_evaluate.py."""
import numpy as np
import pytest
import torch

from tests import eval_fixture as FX
from tests.eval_fixture import NumpyOps


@pytest.fixture(scope='module')
def fx():
    z = FX.load()
    return z, FX.part_b(z)


def test_frame_table_lists_every_covering_clip_once_in_clip_order(fx):
    from motionbert_amd.evaluate import build_frame_csr
    _, b = fx
    split = b['split']
    F, T = len(b['actions']), split.shape[1]
    keep = np.ones(len(split), bool)
    keep[3] = False
    row_ptr, slots = build_frame_csr(split, keep, F)
    want = [[] for _ in range(F)]
    for c in range(len(split)):
        if keep[c]:
            last = {int(f): t for t, f in enumerate(split[c])}          # a repeated frame counts once, with its last listing
            for f, t in last.items():
                want[f].append(c * T + t)
    assert row_ptr.dtype == np.int32 and slots.dtype == np.int32 and row_ptr[0] == 0 and row_ptr[-1] == len(slots)
    for f in range(F):
        assert slots[row_ptr[f]:row_ptr[f + 1]].tolist() == sorted(want[f]), f
    assert any(len(set(c.tolist())) < T for c in split), 'the fixture should hold a resampled clip with repeated frames'
    with pytest.raises(ValueError):
        build_frame_csr(split, keep, int(split.max()))      # a clip frame outside the test set


def test_block_list_and_coverage(fx):
    z, b = fx
    ev = FX.make_evaluator(b, (0, 1, 0), ops=NumpyOps())
    blocked_clip = np.array([str(b['sources'][f])[:-6] == 's_09_act_05_subact_02' for f in b['split'][:, 0]])
    assert blocked_clip.any() and np.array_equal(ev.keep_clip, ~blocked_clip)
    rows = np.diff(ev.row_ptr_host)
    blocked_frame = np.array([str(s)[:-6] == 's_09_act_05_subact_02' for s in b['sources']])
    assert (rows[blocked_frame] == 0).all() and (b['cover'][blocked_frame] > 0).any()      # covered, but only by blocked clips
    assert {0, 1, 2, 3} <= set(rows[~blocked_frame].tolist())                                # frames covered zero, one, three times
    assert ev.action_names == b['action_names'] == sorted(set(b['actions'].tolist()))
    _, _, count = FX.expected(z, (0, 1, 0))
    assert [int((rows[(b['actions'] == a)] > 0).sum()) for a in ev.action_names] == count.tolist()
    everything = FX.make_evaluator(b, (0, 1, 0), ops=NumpyOps(), block_list=())
    assert everything.keep_clip.all() and (np.diff(everything.row_ptr_host) > 0).sum() == (b['cover'] > 0).sum()


@pytest.mark.parametrize('case', FX.CASES)
def test_host_logic_matches_the_reference_aggregation(fx, case):
    z, b = fx
    ev = FX.make_evaluator(b, case, ops=NumpyOps())
    e1, e2, per = FX.run_split(ev, b, 'cpu')
    ref_per, ref_sum, ref_count = FX.expected(z, case)
    got = np.array([[per[a][0] for a in ev.action_names], [per[a][1] for a in ev.action_names]])
    print(case, 'per-action', FX.rel_err(got, ref_per), 'summary', FX.rel_err([e1, e2], ref_sum))
    assert ev.count.tolist() == ref_count.tolist()
    assert FX.rel_err(got, ref_per) < FX.GATE and FX.rel_err([e1, e2], ref_sum) < FX.GATE
    assert e1 == pytest.approx(got[0].mean(), rel=1e-15) and e2 == pytest.approx(got[1].mean(), rel=1e-15)      # mean over actions, not frames
    frames_mean = float(np.sum(got[0] * ref_count) / ref_count.sum())
    assert abs(frames_mean - e1) > 1e-6 * e1


def test_update_order_and_finish_guard(fx):
    _, b = fx
    ev = FX.make_evaluator(b, (1, 1, 1), ops=NumpyOps())
    model = FX.FixedOutputs(torch.from_numpy(b['outputs']))
    ev.update(model, torch.from_numpy(b['x'][:5]))
    with pytest.raises(RuntimeError, match='5 of 16'):
        ev.finish()
    with pytest.raises(ValueError):
        ev.update(model, torch.from_numpy(b['x'][:12]))


def test_cpu_tensors_are_refused():
    import motionbert_amd
    from motionbert_amd.evaluate import evaluate, pose_errors
    assert motionbert_amd.pose_errors is pose_errors and motionbert_amd.H36MEvaluator is not None
    p = torch.zeros(4, 17, 3)
    with pytest.raises(RuntimeError, match='ROCm device'):
        pose_errors(p, p)
    with pytest.raises(RuntimeError, match='ROCm device'):
        pose_errors(p.view(2, 2, 17, 3), p.view(2, 2, 17, 3), hw=torch.ones(2, 2))
    with pytest.raises(RuntimeError, match='ROCm device'):
        evaluate(None, torch.nn.Linear(3, 3), [], None)
    with pytest.raises(ValueError):
        pose_errors(p, p[:, :16], ops=NumpyOps())
