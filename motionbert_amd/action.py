"""Drop-in `ActionNet` (reference `lib/model/model_action.py`) on top of the HIP backbone.

Same constructor, same sub-module names and therefore the same `state_dict` keys as the reference (`backbone.*`,
`head.fc1.*`, `head.bn.*`, `head.fc2.*`; checkpoints store them with a `module.` prefix under `'model'`,
train_action.py:96-104).  The difference is where the first three operations of the head run: the reference materialises
`get_representation(x)` -- `[N, M, T, 17, 512]` fp32, 541 MB at N = 32 -- drops it out element-wise, and averages it over
T and over the M persons; here `DSTformer.get_pooled_representation` does all three inside the backbone's tail kernels
(forward: one pass over the representation; backward: fused with the tail's tanh'), so the head module only sees the
`[N, 17 * 512]` feature.  `fc1 / BatchNorm1d / ReLU / fc2` are ordinary torch modules (17.9 M
parameters, two small GEMMs): under data parallelism pass the head as `extra=` to `DistributedDSTformer`.

Around the model (reference `train_action.py:40-66,172-188`):

    cross_entropy_topk(scores, labels)   `CrossEntropyLoss()`, its gradient and the top-1 / top-5 hit counts of `accuracy(topk=(1, 5))` in one
                                         launch of `mbx_xent_topk`; nothing comes back to the host.
    ActionEvaluator(...)                 `update(model, batch, labels)` per validation batch, `finish()` -> (loss, top-1 %, top-5 %): the
                                         reference's three AverageMeters as one fp64 device meter and ONE host synchronisation.
    validate(test_loader, model, criterion)   the reference's signature and return order.

There is no CPU path: without an injected kernel provider, tensors that are not on a ROCm device raise (`hip_ops.provider`).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops


class _PooledHead(nn.Module):
    def pooled(self, backbone, x):
        N, M, T, J, C = x.shape
        feat = backbone.get_pooled_representation(x.reshape(N * M, T, J, C), persons=M, dropout=self.dropout.p)
        return feat.reshape(N, -1)                                   # (N, J*C)


class ActionHeadClassification(_PooledHead):
    """model_action.py:6-29: dropout -> mean over T -> mean over M -> fc1 -> BatchNorm1d -> ReLU -> fc2."""

    def __init__(self, dropout_ratio=0., dim_rep=512, num_classes=60, num_joints=17, hidden_dim=2048):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout_ratio)
        self.bn = nn.BatchNorm1d(hidden_dim, momentum=0.1)
        self.relu = nn.ReLU(inplace=True)
        self.fc1 = nn.Linear(dim_rep * num_joints, hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, num_classes)

    def forward(self, feat):
        return self.fc2(self.relu(self.bn(self.fc1(feat))))


class ActionHeadEmbed(_PooledHead):
    """model_action.py:31-49: dropout -> means -> fc1 -> L2 normalisation (one-shot recognition)."""

    def __init__(self, dropout_ratio=0., dim_rep=512, num_joints=17, hidden_dim=2048):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout_ratio)
        self.fc1 = nn.Linear(dim_rep * num_joints, hidden_dim)

    def forward(self, feat):
        return F.normalize(self.fc1(feat), dim=-1)


class ActionNet(nn.Module):
    def __init__(self, backbone, dim_rep=512, num_classes=60, dropout_ratio=0., version='class', hidden_dim=2048, num_joints=17):
        super().__init__()
        self.backbone = backbone
        self.feat_J = num_joints
        if version == 'class':
            self.head = ActionHeadClassification(dropout_ratio=dropout_ratio, dim_rep=dim_rep, num_classes=num_classes, num_joints=num_joints)
        elif version == 'embed':
            self.head = ActionHeadEmbed(dropout_ratio=dropout_ratio, dim_rep=dim_rep, hidden_dim=hidden_dim, num_joints=num_joints)
        else:
            raise Exception('Version Error.')

    def forward(self, x):
        """x: (N, M, T, 17, 3) -> class scores (N, num_classes) / embeddings (N, hidden_dim)."""
        return self.head(self.head.pooled(self.backbone, x))


def cross_entropy_topk(scores: torch.Tensor, labels: torch.Tensor, acc: Optional[torch.Tensor] = None, ops=None):
    """`(loss, values)` for scores [N,C] and integer labels [N]: `loss` = `nn.CrossEntropyLoss()(scores, labels)` (train_action.py:55,180) as
    a 0-dim device tensor, differentiable with respect to `scores` (the gradient was computed in the same launch); `values` =
    [loss, top-1 hits, top-5 hits] (device, fp32 counts, no host synchronisation) -- `accuracy(output, target, topk=(1, 5))`
    (lib/utils/learning.py:25-37) is `values[1:] * 100 / N`.  A row is a top-k hit iff fewer than k columns beat the target's, a column
    with an equal score beating it only from a lower index.  `acc` [4] fp64 on the device, if given, is ADDED to: [sum of row losses, top-1
    hits, top-5 hits, rows].  1 <= N <= 65536, 1 <= C <= 4096; no `ignore_index`, no label smoothing."""
    from .train import _FusedLossFn
    if scores.dim() != 2 or labels.reshape(-1).shape[0] != scores.shape[0]:
        raise ValueError(f'scores [N,C] and labels [N] expected, got {tuple(scores.shape)} / {tuple(labels.shape)}')
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f'labels must be integers, got {labels.dtype}')
    if not (1 <= scores.shape[0] <= 65536 and 1 <= scores.shape[1] <= 4096):
        raise ValueError(f'cross_entropy_topk supports 1 <= N <= 65536 rows and 1 <= C <= 4096 classes, got {tuple(scores.shape)}')
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() != 4 or acc.device != scores.device):
        raise ValueError('acc must be 4 float64 values on the device of the scores')
    ops = hip_ops.provider(ops, 'motionbert_amd.action.cross_entropy_topk', scores, labels, move='scores and labels')
    lab = labels.detach().reshape(-1).to(device=scores.device, dtype=torch.int32).contiguous()
    return _FusedLossFn.apply(lambda x, values, dx: ops.xent_topk(x, lab, values, dx, acc), 3, 0, scores)


class ActionEvaluator:
    """The validation loop of train_action.py:40-66 with its three meters on the device.

        ev = ActionEvaluator()
        for batch, labels in test_loader: ev.update(model, batch.cuda(), labels)
        loss, top1, top5 = ev.finish()

    `update` runs an eval-mode no-grad forward and `mbx_xent_topk` into an fp64 meter [sum of row losses, top-1 hits, top-5 hits, rows] and returns
    the scores; `finish()` is the only host synchronisation.  The averages are weighted by rows, as the reference's
    `AverageMeter.update(value, batch_size)` weights them.  `ops`: kernel provider (default: libmbx.so, tensors on the ROCm device)."""

    def __init__(self, ops=None, device=None):
        self.ops, self.device = hip_ops.evaluator_provider(ops, device, 'motionbert_amd.action.ActionEvaluator')
        self.reset()

    def reset(self):
        self.meter = torch.zeros(4, dtype=torch.float64, device=self.device)

    def update(self, model, batch: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        if hasattr(model, 'eval'):
            model.eval()
        with torch.no_grad():
            scores = model(batch.to(self.device)).float().contiguous()
            if scores.shape[0]:
                cross_entropy_topk(scores, torch.as_tensor(labels).to(self.device), acc=self.meter, ops=self.ops)
        return scores

    def finish(self):
        """(loss_avg, top-1 %, top-5 %) over the rows seen since the constructor / reset(): the one host synchronisation."""
        total, h1, h5, rows = self.meter.cpu().tolist()
        if rows == 0:
            raise RuntimeError('finish() before any update()')
        return total / rows, 100.0 * h1 / rows, 100.0 * h5 / rows


def validate(test_loader, model, criterion=None, ops=None, device=None):
    """Drop-in for the reference's `validate(test_loader, model, criterion)` (train_action.py:40-66): `(loss_avg, top-1 %, top-5 %)` as
    Python floats (the reference returns the two accuracies as 0-dim tensors).  `criterion` is accepted for the signature's sake and must
    be None or a plain `nn.CrossEntropyLoss()`: that is the loss `mbx_xent_topk` computes."""
    if criterion is not None:
        c = criterion.module if hasattr(criterion, 'module') else criterion
        if (not isinstance(c, nn.CrossEntropyLoss) or c.weight is not None or c.reduction != 'mean' or c.ignore_index != -100
                or getattr(c, 'label_smoothing', 0.0) != 0.0):
            raise ValueError('motionbert_amd.action.validate computes a plain nn.CrossEntropyLoss(); pass that or None')
    if ops is None and device is None:
        device = hip_ops.model_device(model, 'motionbert_amd.action.validate')
    ev = ActionEvaluator(ops=ops, device=device)
    for batch, labels in test_loader:
        ev.update(model, batch, labels)
    return ev.finish()
