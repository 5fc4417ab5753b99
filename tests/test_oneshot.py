"""Host logic of motionbert_amd.oneshot and data.m_per_class_batches without a GPU: a torch provider (tests/oneshot_fixture.py) stands in
for libmbx.so; the C entry points' argument checks run for real (they return before any launch)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import supconerr as SC
from tests.oneshot_fixture import TableModel, TorchOneShotOps


# ------------------------------------------------------------------------------------------------ supcon_loss
def test_supcon_loss_flattens_trailing_dimensions_and_differentiates():
    from motionbert_amd.oneshot import supcon_loss
    ops = TorchOneShotOps()
    feat, lab = SC.supcon_inputs(4, 2, 8, 3)
    a = feat.reshape(4, 2, 2, 4).clone().requires_grad_(True)
    loss = supcon_loss(a, lab, temperature=0.1, ops=ops)
    assert loss.shape == () and ops.calls == [('supcon_loss', (4, 2, 8), False, True)]
    (loss * 2.5).backward()
    rl, rd = SC.supcon_ref64(feat, lab, 0.1, 0.07, False, 2.5)
    assert abs(float(loss.detach()) - float(rl)) < 1e-6 and a.grad.shape == (4, 2, 2, 4)
    assert float((a.grad.reshape(4, 2, 8).double() - rd).abs().max()) < 1e-6 * float(rd.abs().max())
    with torch.no_grad():
        supcon_loss(feat, lab.reshape(4, 1), normalize=True, ops=ops)                      # labels [bsz, 1] as the reference takes them
    assert ops.calls[-1] == ('supcon_loss', (4, 2, 8), True, False), 'no gradient buffer without a graph'


def test_supcon_loss_without_labels_is_simclr():
    from motionbert_amd.oneshot import supcon_loss
    ops = TorchOneShotOps()
    feat, _ = SC.supcon_inputs(4, 2, 8, 4)
    got = supcon_loss(feat, ops=ops)
    ref, _ = SC.supcon_ref64(feat, torch.arange(4), 0.07, 0.07, False)
    assert abs(float(got) - float(ref)) < 1e-6 * abs(float(ref))
    assert math.isnan(float(supcon_loss(feat[:, :1], ops=ops))), 'one view, every sample its own class: no anchor has a positive'


def test_supcon_loss_refusals():
    from motionbert_amd.oneshot import supcon_loss
    ops = TorchOneShotOps()
    f = torch.zeros(4, 2, 8)
    with pytest.raises(ValueError, match='at least 3 dimensions'):
        supcon_loss(f[:, 0], torch.arange(4), ops=ops)
    with pytest.raises(ValueError, match='Num of labels'):
        supcon_loss(f, torch.arange(5), ops=ops)
    with pytest.raises(ValueError, match='integers'):
        supcon_loss(f, torch.zeros(4), ops=ops)
    with pytest.raises(ValueError, match='anchors'):
        supcon_loss(torch.zeros(65, 2, 8), torch.arange(65), ops=ops)
    with pytest.raises(ValueError, match='anchors'):
        supcon_loss(torch.zeros(1, 1, 8), torch.arange(1), ops=ops)
    with pytest.raises(ValueError, match='temperature'):
        supcon_loss(f, torch.arange(4), temperature=0.0, ops=ops)
    with pytest.raises(TypeError):
        supcon_loss(f, torch.arange(4), mask=torch.eye(4), ops=ops)                         # not offered
    assert ops.calls == []
    with pytest.raises(RuntimeError, match='no CPU path'):
        supcon_loss(f, torch.arange(4))


# ------------------------------------------------------------------------------------------------ evaluator
def test_evaluator_bookkeeping():
    from motionbert_amd.oneshot import OneShotEvaluator, validate
    a, al, t, tl = SC.nn_inputs(5, 23, 16, 9, 2.0)
    _, _, pred, acc = SC.nn_ref64(a, al, t, tl)
    ops = TorchOneShotOps()
    ev = OneShotEvaluator(ops=ops)
    model = TableModel(t)
    with pytest.raises(RuntimeError, match='set_anchors'):
        ev.update(model, torch.arange(3), tl[:3])
    ev.set_anchors(a, al)
    with pytest.raises(RuntimeError, match='before any update'):
        ev.finish()
    got = [ev.update(model, torch.arange(lo, hi), tl[lo:hi]) for lo, hi in ((0, 7), (7, 8), (8, 23))]
    assert torch.equal(torch.cat(got), pred) and ev.count == 23 and model.evals == 3
    assert ev.finish() == acc and [c[0] for c in ops.calls] == ['nn_cosine'] * 3
    ev.update(model, torch.arange(0), tl[:0])                                               # an empty batch: no call, nothing counted
    assert ev.count == 23 and len(ops.calls) == 3
    ev.reset()
    assert ev.count == 0 and int(ev.hits) == 0 and ev.anchors is not None
    with pytest.raises(ValueError, match='labels'):
        ev.update(model, torch.arange(3), tl[:2])
    # exemplars through a loader, and the reference's validate()
    anchors = TableModel(a)
    ev2 = OneShotEvaluator(ops=ops)
    ev2.set_anchors(anchors, [(torch.arange(0, 2), al[0:2]), (torch.arange(2, 5), al[2:5])])
    assert torch.equal(ev2.anchors, a) and torch.equal(ev2.anchor_labels, al) and anchors.evals == 1
    both = TableModel(torch.cat([a, t]))
    out = validate([(torch.arange(0, 5), al)], [(torch.arange(5, 15), tl[:10]), (torch.arange(15, 28), tl[10:])], both, ops=ops)
    assert isinstance(out, torch.Tensor) and out.shape == () and float(out) == pytest.approx(acc)
    with pytest.raises(RuntimeError, match='no CPU path'):
        validate([], [], torch.nn.Linear(2, 2))


# ------------------------------------------------------------------------------------------------ sampler
def test_m_per_class_batches_properties():
    from motionbert_amd.data import m_per_class_batches
    sizes = [1, 3, 5, 2, 2, 9, 2, 4, 2, 2]
    labels = np.repeat(np.arange(10) * 7, sizes)
    labels = labels[np.random.default_rng(0).permutation(len(labels))]
    for m, bs in ((2, 8), (4, 8), (2, 20)):
        batches = m_per_class_batches(labels, m, bs, length=5 * bs + 3, seed=11)
        assert len(batches) == 5
        for b in batches:
            assert b.dtype == np.int64 and b.shape == (bs,) and b.min() >= 0 and b.max() < len(labels)
            cls, cnt = np.unique(labels[b], return_counts=True)
            assert len(cls) == bs // m and (cnt == m).all(), 'batch_size / m distinct classes, m samples each'
            for c in cls:                                                                   # with repetition only where the class is short
                idx = b[labels[b] == c]
                have = int((labels == c).sum())
                assert len(set(idx.tolist())) == m if have >= m else len(set(idx.tolist())) <= have
            lab = torch.from_numpy(labels[b])
            same = (lab[:, None] == lab[None, :]).sum(1) - 1
            assert int(same.min()) >= 1, 'no anchor without a positive'
        again = m_per_class_batches(labels, m, bs, length=5 * bs + 3, seed=11)
        assert all(np.array_equal(x, y) for x, y in zip(batches, again)), 'a function of the seed'
        other = m_per_class_batches(labels, m, bs, length=5 * bs + 3, seed=12)
        assert any(not np.array_equal(x, y) for x, y in zip(batches, other))
    assert len(m_per_class_batches(labels, 2, 8)) == len(labels) // 8
    # the loss of such a batch is finite; of a batch drawn without the guarantee it need not be
    feat = torch.randn(8, 1, 4, generator=torch.Generator().manual_seed(1))
    b = m_per_class_batches(labels, 2, 8, seed=3)[0]
    assert math.isfinite(float(SC.supcon_ref64(feat, torch.from_numpy(labels[b]), 0.1, 0.07, True)[0]))
    for bad in (dict(m=1, batch_size=8), dict(m=3, batch_size=8), dict(m=2, batch_size=22), dict(m=4, batch_size=2)):
        with pytest.raises(ValueError):
            m_per_class_batches(labels, **bad)


# ------------------------------------------------------------------------------------------------ the C entry points' argument checks
@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_argument_errors_are_reported_not_crashed(lib):
    p = C.c_void_p(4096)            # never dereferenced: every check below fails before a launch
    assert lib.mbx_supcon_loss(None, None, 4, 2, 8, 0.1, 0.07, 0, 1.0, None, None, None, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_supcon_loss(p, p, 65, 2, 8, 0.1, 0.07, 0, 1.0, p, None, p, None) != 0
    assert b'130 anchors' in lib.mbx_last_error() and b'<= 128' in lib.mbx_last_error()
    assert lib.mbx_supcon_loss(p, p, 1, 1, 8, 0.1, 0.07, 0, 1.0, p, None, p, None) != 0 and b'anchors' in lib.mbx_last_error()
    assert lib.mbx_supcon_loss(p, p, 4, 2, 0, 0.1, 0.07, 0, 1.0, p, None, p, None) != 0 and b'bad shape' in lib.mbx_last_error()
    assert lib.mbx_supcon_loss(p, p, 4, 2, 8, 0.0, 0.07, 0, 1.0, p, None, p, None) != 0 and b'temperature' in lib.mbx_last_error()
    assert lib.mbx_supcon_loss(p, p, 4, 2, 8, 0.1, -1.0, 0, 1.0, p, None, p, None) != 0 and b'temperature' in lib.mbx_last_error()
    assert lib.mbx_supcon_loss_ws(128, 4096) >= (128 + 1) * 128 * 128 * 4 and lib.mbx_supcon_loss_ws(8, 1) > 0
    assert lib.mbx_supcon_loss_ws(129, 8) == 0 and lib.mbx_supcon_loss_ws(1, 8) == 0 and lib.mbx_supcon_loss_ws(8, 0) == 0
    assert lib.mbx_nn_cosine(p, p, 0, p, None, 4, 8, p, None, None, None) != 0 and b'exemplar' in lib.mbx_last_error()
    assert lib.mbx_nn_cosine(p, p, 3, p, None, 4, 0, p, None, None, None) != 0 and b'bad shape' in lib.mbx_last_error()
    assert lib.mbx_nn_cosine(p, p, 3, p, None, -1, 8, p, None, None, None) != 0 and b'row count' in lib.mbx_last_error()
    assert lib.mbx_nn_cosine(None, p, 3, p, None, 4, 8, p, None, None, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_nn_cosine(p, p, 3, p, p, 4, 8, p, None, None, None) != 0 and b'hit counter' in lib.mbx_last_error()
    assert lib.mbx_nn_cosine(None, None, 3, None, None, 0, 8, None, None, None, None) == 0, 'N = 0 is a no-op'


def test_binding_refuses_wrong_dtypes_before_the_library_is_called():
    from motionbert_amd import hip_ops

    class Lib:                      # no symbol may be reached
        pass
    ops = hip_ops.HipOps(lib=Lib())
    f, lab, loss = torch.zeros(4, 2, 8), torch.zeros(4, dtype=torch.int32), torch.zeros(1)
    with pytest.raises(RuntimeError, match='labels must be a contiguous torch.int32'):
        ops.supcon_loss(f, lab.long(), 0.1, 0.07, False, loss, None)
    with pytest.raises(RuntimeError, match='feat must be a contiguous'):
        ops.supcon_loss(torch.zeros(4, 2, 16)[:, :, ::2], lab, 0.1, 0.07, False, loss, None)             # a strided view
    with pytest.raises(RuntimeError, match='dfeat must be a contiguous'):
        ops.supcon_loss(f, lab, 0.1, 0.07, False, loss, torch.zeros(4, 2, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='dfeat must be a contiguous'):
        ops.supcon_loss(f, lab, 0.1, 0.07, False, loss, torch.zeros(4, 2, 7))
    with pytest.raises(RuntimeError, match='loss must be a contiguous'):
        ops.supcon_loss(f, lab, 0.1, 0.07, False, torch.zeros(2), None)
    with pytest.raises(RuntimeError, match=r'feat \[bsz,n_views,D\]'):
        ops.supcon_loss(f[0], lab, 0.1, 0.07, False, loss, None)
    a, al, t, pred = torch.zeros(3, 8), torch.zeros(3, dtype=torch.int32), torch.zeros(5, 8), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='nn_cosine needs'):
        ops.nn_cosine(a, al, torch.zeros(5, 7), None, pred, None, None)
    with pytest.raises(RuntimeError, match='test must be a contiguous'):
        ops.nn_cosine(a, al, torch.zeros(8, 5).T, None, pred, None, None)
    with pytest.raises(RuntimeError, match='anchors must be a contiguous'):
        ops.nn_cosine(a.double(), al, t, None, pred, None, None)
    with pytest.raises(RuntimeError, match='best_sim must be a contiguous'):
        ops.nn_cosine(a, al, t, None, pred, torch.zeros(4), None)
    with pytest.raises(RuntimeError, match='pred_label must be a contiguous'):
        ops.nn_cosine(a, al, t, None, pred.long(), None, None)
    with pytest.raises(RuntimeError, match='hits must be a contiguous'):
        ops.nn_cosine(a, al, t, pred, pred, None, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='hit counter'):
        ops.nn_cosine(a, al, t, pred, pred, None, None)
