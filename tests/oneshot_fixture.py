"""A torch kernel provider for the host logic of motionbert_amd.oneshot (tests/test_oneshot.py): the two kernel entries answered by the
float64 restatements of tests/supconerr.py, with the call counts the bookkeeping tests look at.  Never part of the product."""
import torch

from tests import supconerr as SC


class TorchOneShotOps:
    def __init__(self):
        self.calls = []

    def supcon_loss(self, feat, labels, temperature, base_temperature, normalize, loss, dfeat, grad_scale=1.0):
        assert feat.dim() == 3 and feat.dtype == torch.float32 and feat.is_contiguous() and labels.dtype == torch.int32
        self.calls.append(('supcon_loss', tuple(feat.shape), bool(normalize), dfeat is not None))
        with torch.enable_grad():      # an autograd.Function's forward runs with the graph switched off
            l, d = SC.supcon_ref64(feat, labels, temperature, base_temperature, normalize, grad_scale)
        loss[0] = l.float()
        if dfeat is not None:
            dfeat.copy_(d.float())

    def nn_cosine(self, anchors, anchor_labels, test, test_labels, pred_label, best_sim, hits):
        assert anchors.dtype == torch.float32 and test.dtype == torch.float32 and anchor_labels.dtype == torch.int32
        self.calls.append(('nn_cosine', tuple(anchors.shape), tuple(test.shape)))
        idx, sims, pred, _ = SC.nn_ref64(anchors, anchor_labels, test)
        pred_label.copy_(pred)
        if best_sim is not None:
            best_sim.copy_(sims.max(0).values.float())
        if test_labels is not None:
            hits += int((pred == test_labels).sum())


class TableModel:
    """Stands in for ActionNet: a 'clip' is its index into a table of embeddings."""

    def __init__(self, table):
        self.table, self.evals = table, 0

    def eval(self):
        self.evals += 1
        return self

    def __call__(self, idx):
        return self.table[idx.long()]
