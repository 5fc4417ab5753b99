"""The host logic of the action-recognition task layer on the CPU, with the kernel provider of tests/actionerr.py injected: the PackedAction
stream, ActionEvaluator / validate against the reference's meters (tests/golden/action.npz), the meters of ActionStep(fused_loss=True), and
the argument errors of the two C entries on the library loaded without a GPU."""
import gc
import os
import pickle
import threading

import numpy as np
import pytest
import torch

from motionbert_amd import action, augment, data, hip_ops, train
from tests import actionerr as AE
from tests.helpers import GOLDEN


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'action.npz'))


@pytest.fixture(scope='module')
def packed(tmp_path_factory):
    d = tmp_path_factory.mktemp('ntu')
    pkl = str(d / 'ntu.pkl')
    with open(pkl, 'wb') as f:
        pickle.dump(AE.annotation_file(AE.annotations()), f)
    prefix = str(d / 'all')
    meta = data.pack_action(pkl, 'all', AE.ANN_N_FRAMES, prefix, check_split=False)
    return prefix, meta


# ------------------------------------------------------------------------------------------------ PackedAction
def test_packed_action_stream_shapes_labels_and_device_stage(packed):
    prefix, meta = packed
    assert meta['n'] == 6 and meta['clip_shape'] == [2, 27, 17, 3]
    ops = AE.TorchActionOps()
    ds = data.PackedAction(prefix, device='cpu', ops=ops)
    assert len(ds) == 6
    got = list(ds.batches(4, shuffle=True, epoch=3, seed=11))
    assert [tuple(b.shape) for b, _ in got] == [(4, 2, 27, 17, 3), (2, 2, 27, 17, 3)]
    assert all(b.dtype == torch.float32 and l.dtype == torch.int64 and l.shape == (len(b),) for b, l in got)
    assert [c[0] for c in ops.calls] == ['action_input', 'action_input'] and all(c[2] == 3 and not c[4] for c in ops.calls)
    assert [c[3] for c in ops.calls] == [ds.batch_seed(11, 3, 0, 0), ds.batch_seed(11, 3, 0, 1)] and ops.calls[0][3] != ops.calls[1][3]
    idx = data.shard_indices(6, True, 3, 11, 0, 1)
    motions, labels = np.load(prefix + '.motion.npy'), np.load(prefix + '.label.npy')
    for k, (b, l) in enumerate(got):
        rows = np.sort(idx[4 * k:4 * k + 4])
        assert l.tolist() == labels[rows].tolist()
        want = augment.action_input(torch.from_numpy(motions[rows]), seed=ds.batch_seed(11, 3, 0, k), ops=AE.TorchActionOps())
        assert torch.equal(b, want)
        assert float(b[..., :2].abs().max()) <= 1.0
    assert len(list(ds.batches(4, drop_last=True))) == 1


def test_packed_action_is_deterministic_from_the_seed_and_sharded(packed):
    prefix, _ = packed
    ds = data.PackedAction(prefix, device='cpu', ops=AE.TorchActionOps())
    a = list(ds.batches(3, shuffle=True, epoch=1, seed=4))
    b = list(ds.batches(3, shuffle=True, epoch=1, seed=4))
    assert all(torch.equal(x, y) and torch.equal(l, m) for (x, l), (y, m) in zip(a, b))
    c = list(ds.batches(6, shuffle=False, epoch=1, seed=4))
    d = list(ds.batches(6, shuffle=False, epoch=2, seed=4))
    assert torch.equal(c[0][1], d[0][1]) and not torch.equal(c[0][0], d[0][0]), 'the same clips with other draws in another epoch'
    parts = [list(ds.batches(2, shuffle=True, epoch=0, seed=9, rank=r, world=4)) for r in range(4)]
    assert all(sum(len(l) for _, l in p) == 2 for p in parts), 'equal shares: ceil(6 / 4) clips per rank'
    seeds = {ds.batch_seed(9, 0, r, 0) for r in range(4)}
    assert len(seeds) == 4
    # validation: no move; scale_range None and no move: the stored clips as they are, no launch
    ops = AE.TorchActionOps()
    val = data.PackedAction(prefix, device='cpu', train=False, ops=ops)
    list(val.batches(6, shuffle=False))
    assert ops.calls[0][2] == AE.CROP
    ops = AE.TorchActionOps()
    raw = data.PackedAction(prefix, device='cpu', random_move=False, scale_range=None, ops=ops)
    (b, _), = list(raw.batches(6, shuffle=False))
    assert not ops.calls and torch.equal(b, torch.from_numpy(np.load(prefix + '.motion.npy')))


def test_packed_action_abandoned_epoch_releases_the_loader_thread(packed):
    prefix, _ = packed
    ds = data.PackedAction(prefix, device='cpu', ring=2, ops=AE.TorchActionOps())
    before = threading.active_count()
    for _ in range(3):
        it = ds.batches(1, shuffle=False)
        next(it)
        it.close()
        for k, _b in enumerate(ds.batches(1, shuffle=False)):
            if k == 1:
                break
        gc.collect()
    with pytest.raises(ZeroDivisionError):
        for _b in ds.batches(1, shuffle=False):
            1 / 0
    gc.collect()
    assert threading.active_count() == before
    assert sum(len(l) for _, l in ds.batches(4, shuffle=False)) == 6


def test_both_packed_classes_use_the_one_stream_helper():
    import inspect
    for cls in (data.PackedMotion3D, data.PackedAction):
        src = inspect.getsource(cls.batches)
        assert 'pinned_batches(' in src and 'threading.Thread' not in src and 'pin_memory' not in src, cls.__name__
    assert data.PackedAction.batches.__code__.co_names.count('shard_indices') == 1


def test_action_input_entry_checks_its_arguments():
    x = AE.motion_inputs(2, 2, 5, 17, 1)
    ops = AE.TorchActionOps()
    y, used = augment.action_input(x, seed=3, return_params=True, ops=ops)
    assert torch.equal(used, AE.draw_params(2, 3)) and y.shape == x.shape
    assert torch.equal(augment.action_input(x, params=used, ops=ops), y)
    with pytest.raises(ValueError, match=r'\[N,M,T,J,3\]'):
        augment.action_input(x[0], ops=ops)
    with pytest.raises(ValueError, match=r'params must be \[2, 9\]'):
        augment.action_input(x, params=used[:1], ops=ops)
    with pytest.raises(ValueError, match='lo > hi'):
        augment.action_input(x, angle_range=(5, -5), ops=ops)
    with pytest.raises(RuntimeError, match=r'motionbert_amd\.augment\.action_input runs on the ROCm device'):
        augment.action_input(x)


# ------------------------------------------------------------------------------------------------ evaluation
class TableModel(torch.nn.Module):
    """stands in for ActionNet: a 'clip' is its index into a table of scores"""

    def __init__(self, table):
        super().__init__()
        self.table = torch.nn.Parameter(table)

    def forward(self, idx):
        return self.table[idx.long()]


def _two_batches():
    za, la = AE.logit_inputs(2, 60, AE.xent_seed((2, 60)))
    zb, lb = AE.logit_inputs(32, 60, AE.xent_seed((32, 60)))
    return TableModel(torch.cat([za, zb])), [(torch.arange(2), la), (torch.arange(2, 34), lb)]


def test_evaluator_and_validate_against_the_reference_meters(fixture):
    """the reference's validate(): three AverageMeters updated with (batch value, batch size); batch values from the reference's own
    CrossEntropyLoss and accuracy() in the fixture"""
    model, loader = _two_batches()
    n = np.asarray([2.0, 32.0])
    loss = np.asarray([float(fixture['xe.2.60.loss']), float(fixture['xe.32.60.loss'])])
    acc = np.stack([fixture['xe.2.60.acc'], fixture['xe.32.60.acc']])
    want = (float((loss * n).sum() / n.sum()), float((acc[:, 0] * n).sum() / n.sum()), float((acc[:, 1] * n).sum() / n.sum()))
    ops = AE.TorchActionOps()
    model.train()
    got = action.validate(loader, model, torch.nn.CrossEntropyLoss(), ops=ops)
    assert not model.training and all(isinstance(v, float) for v in got)
    assert abs(got[0] - want[0]) <= 1e-6 * want[0] and abs(got[1] - want[1]) <= 1e-4 and abs(got[2] - want[2]) <= 1e-4, (got, want)
    assert [c[0] for c in ops.calls] == ['xent_topk'] * 2 and all(not c[2] and c[3] for c in ops.calls), 'no gradient, the meter passed in'
    ev = action.ActionEvaluator(ops=AE.TorchActionOps())
    with pytest.raises(RuntimeError, match='before any update'):
        ev.finish()
    scores = ev.update(model, *loader[0])
    assert scores.shape == (2, 60) and not scores.requires_grad
    one = ev.finish()
    assert abs(one[0] - loss[0]) <= 1e-6 * loss[0]
    ev.reset()
    assert float(ev.meter.abs().sum()) == 0
    with pytest.raises(ValueError, match='plain nn.CrossEntropyLoss'):
        action.validate(loader, model, torch.nn.CrossEntropyLoss(label_smoothing=0.1), ops=ops)
    with pytest.raises(RuntimeError, match=r'motionbert_amd\.action\.validate runs on the ROCm device'):
        action.validate(loader, model)
    with pytest.raises(RuntimeError, match=r'motionbert_amd\.action\.ActionEvaluator runs on the ROCm device'):
        action.ActionEvaluator(device='cpu')


def test_cross_entropy_topk_values_gradient_and_argument_checks():
    z, lab = AE.logit_inputs(33, 120, AE.xent_seed((33, 120)))
    zz = z.clone().requires_grad_(True)
    acc = torch.zeros(4, dtype=torch.float64)
    loss, values = action.cross_entropy_topk(zz, lab, acc=acc, ops=AE.TorchActionOps())
    (3.0 * loss).backward()
    ref = z.clone().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(ref, lab)
    (3.0 * want).backward()
    assert loss.dim() == 0 and torch.allclose(loss, want, rtol=1e-6) and torch.allclose(zz.grad, ref.grad, rtol=1e-5, atol=1e-8)
    r = AE.xent_topk_ref64(z, lab)
    assert values.tolist()[1:] == [float(r['hit1']), float(r['hit5'])] and acc.tolist()[1:] == [float(r['hit1']), float(r['hit5']), 33.0]
    for bad, msg in ((lambda: action.cross_entropy_topk(z[0], lab), r'scores \[N,C\]'), (lambda: action.cross_entropy_topk(z, lab.float()), 'integers'),
                     (lambda: action.cross_entropy_topk(torch.zeros(2, 4097), lab[:2]), '4096 classes'),
                     (lambda: action.cross_entropy_topk(z, lab, acc=torch.zeros(4)), 'float64')):
        with pytest.raises(ValueError, match=msg):
            bad()
    with pytest.raises(RuntimeError, match=r'motionbert_amd\.action\.cross_entropy_topk runs on the ROCm device'):
        action.cross_entropy_topk(z, lab)


# ------------------------------------------------------------------------------------------------ the step
class _Step(train.ActionStep):
    """ActionStep without the flat optimizers (they need the device): the loss path and the meters are the class's own"""

    def __init__(self, model, ops, fused_loss=True):
        self.model, self.ddp, self.fused_loss, self.ops, self.meter, self.steps = model, None, fused_loss, ops, None, 0

    def zero_grad(self):
        self.model.zero_grad(set_to_none=True)

    def step(self):
        self.steps += 1


def test_action_step_fused_loss_meters():
    model, loader = _two_batches()
    ops = AE.TorchActionOps()
    step = _Step(model, ops)
    with pytest.raises(RuntimeError, match='before any step'):
        step.meters()
    total = np.zeros(4)
    for idx, lab in loader:
        loss, out = step(idx, lab)
        r = AE.xent_topk_ref64(model.table.detach()[idx], lab)
        assert loss.dim() == 0 and not loss.requires_grad and out.shape == (len(idx), 60) and not out.requires_grad
        assert abs(float(loss) - float(r['loss'])) <= 1e-6 * float(r['loss'])
        ref = model.table.detach().clone().requires_grad_(True)
        torch.nn.functional.cross_entropy(ref[idx], lab).backward()
        assert torch.allclose(model.table.grad, ref.grad, rtol=1e-5, atol=1e-8), 'the gradient reaches the parameters'
        total += [float(r['row_loss'].sum()), r['hit1'], r['hit5'], len(idx)]
    assert step.steps == 2 and [c[0] for c in ops.calls] == ['xent_topk'] * 2 and all(c[2] and c[3] for c in ops.calls)
    got = step.meters()
    assert np.allclose(got, [total[0] / 34, 100 * total[1] / 34, 100 * total[2] / 34], rtol=1e-12)
    step.reset_meters()
    with pytest.raises(RuntimeError, match='before any step'):
        step.meters()
    plain = _Step(model, None, fused_loss=False)
    loss, _ = plain(*loader[0])
    assert plain.meter is None and abs(float(loss) - float(AE.xent_topk_ref64(model.table.detach()[:2], loader[0][1])['loss'])) < 1e-5
    with pytest.raises(RuntimeError, match='fused_loss=True'):
        plain.meters()
    import inspect
    assert inspect.signature(train.ActionStep.__init__).parameters['fused_loss'].default is False


# ------------------------------------------------------------------------------------------------ the C entries without a GPU
def test_abi_argument_errors_without_a_gpu():
    """validation happens before any launch, so this is safe without a GPU"""
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 130
    err = lambda: lib.mbx_last_error().decode()                                           # noqa: E731
    r = (-10.0, 10.0, 0.9, 1.1, -0.1, 0.1, 1.0, 1.0)
    assert lib.mbx_action_input(None, None, 1, 1, 1, 17, None, None, *r, 3, 0, None) != 0 and 'null' in err()
    for shape in ((0, 2, 27, 17), (1, 0, 27, 17), (1, 2, 0, 17), (1, 2, 27, 0), (1, 2, 27, 33)):
        assert lib.mbx_action_input(8, 8, *shape, None, None, *r, 3, 0, None) != 0 and 'bad shape' in err(), shape
    for k in range(4):
        bad = list(r)
        bad[2 * k], bad[2 * k + 1] = bad[2 * k + 1] + 1.0, bad[2 * k]
        assert lib.mbx_action_input(8, 8, 1, 2, 27, 17, None, None, *bad, 3, 0, None) != 0 and 'lo > hi' in err(), k
    assert lib.mbx_action_input(8, 8, 1, 2, 27, 17, None, None, *r, 4, 0, None) != 0 and 'flags' in err()
    assert lib.mbx_xent_topk(None, None, 1, 5, 1.0, None, None, None, None) != 0 and 'null' in err()
    for n, c in ((0, 5), (65537, 5), (1, 0), (1, 4097)):
        assert lib.mbx_xent_topk(8, 8, n, c, 1.0, 8, None, None, None) != 0 and 'bad shape' in err(), (n, c)
