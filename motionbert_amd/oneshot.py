"""One-shot action recognition on the device (reference `train_action_1shot.py`, `lib/model/loss_supcon.py`; configs
`configs/action/MB_train_NTU120_oneshot.yaml`, `MB_ft_NTU120_oneshot.yaml`: model_version embed, hidden_dim 2048, temp 0.1, n_views 2).

The reference's loss runs about 15 small torch kernels on a 32 x 32 logit matrix, and its `validate()` (train_action_1shot.py:58-69)
builds the `[M, N, hidden]` broadcast for `F.cosine_similarity` -- M * N * 2048 * 4 bytes for a result of one integer per clip.  Here:

    supcon_loss(features, labels, ...)   SupConLoss.forward with contrast_mode 'all' and its gradient in one call of `mbx_supcon_loss`,
                                         optionally through the head's L2 normalisation; the loss stays on the device.
    OneShotStep(model, ...)              the optimizer step of train_action_1shot.py:186-198, a `train.TwoGroupStep` like `train.ActionStep`.
    OneShotEvaluator(...)                exemplars once, then `update(model, batch, labels)` per test batch (`mbx_nn_cosine` into device
                                         buffers); `finish()` returns the accuracy and is the only host synchronisation.
    validate(anchor_loader, test_loader, model)   the reference's signature and return value.

`mask=` and `contrast_mode='one'` of the reference's loss are not offered (the trainer uses neither).  The step is single-process: the
reference computes the loss over the gathered batch, and a per-rank loss would be a different objective.

There is no CPU path: without an injected kernel provider, tensors that are not on a ROCm device raise (`hip_ops.provider`).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import hip_ops
from .train import TwoGroupStep, _FusedLossFn


def supcon_loss(features: torch.Tensor, labels: Optional[torch.Tensor] = None, temperature: float = 0.07, base_temperature: float = 0.07,
                normalize: bool = False, ops=None) -> torch.Tensor:
    """`SupConLoss(temperature, 'all', base_temperature)(features, labels)` (loss_supcon.py:21-98) as a 0-dim device tensor,
    differentiable with respect to `features`; the gradient was computed in the same call.

    features [bsz, n_views, ...] (trailing dimensions are flattened as the reference flattens them); labels [bsz] integers, or None
    for SimCLR: every sample its own class, `labels = arange(bsz)` -- with n_views = 1 no anchor has a positive then and the loss is
    NaN, as the reference's is.  `normalize=True`: `features` is the embedding BEFORE `F.normalize(dim=-1)`; the loss is taken of
    the normalised rows and the gradient comes back with respect to the rows that were passed."""
    if features.dim() < 3:
        raise ValueError('`features` needs to be [bsz, n_views, ...], at least 3 dimensions are required')
    bsz, n_views = features.shape[0], features.shape[1]
    feat = features.reshape(bsz, n_views, -1)
    if labels is None:
        labels = torch.arange(bsz, device=features.device)
    labels = labels.reshape(-1)
    if labels.shape[0] != bsz:
        raise ValueError('Num of labels does not match num of features')
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f'labels must be integers, got {labels.dtype}')
    if not (2 <= bsz * n_views <= 128):
        raise ValueError(f'supcon_loss supports 2 <= bsz * n_views <= 128 anchors, got {bsz} x {n_views}')
    if feat.shape[2] < 1:
        raise ValueError('features have no elements per view')
    if not (temperature > 0 and base_temperature > 0):
        raise ValueError(f'temperature {temperature} and base_temperature {base_temperature} must be > 0')
    ops = hip_ops.provider(ops, 'motionbert_amd.oneshot.supcon_loss', features, labels)
    lab = labels.detach().to(device=features.device, dtype=torch.int32).contiguous()
    t, bt, norm = float(temperature), float(base_temperature), bool(normalize)
    return _FusedLossFn.apply(lambda x, loss, dx: ops.supcon_loss(x, lab, t, bt, norm, loss, dx), 1, 0, feat)[0]


class OneShotStep(TwoGroupStep):
    """One optimizer step of train_action_1shot.py:186-198: embeddings of batch [N,M,T,17,3], reshaped to [N, -1, hidden]
    (N * n_views samples arrive as N rows of one view), SupCon loss at `temperature`, backward, and the two AdamW groups of
    `train.TwoGroupStep` (:156-161).  The head's `fc1` output goes into the loss un-normalised: `mbx_supcon_loss` normalises the rows itself
    and hands back the cotangent of `fc1`'s output, so F.normalize and its backward never run as torch kernels.
    Returns `loss.detach()` (device tensor, no host synchronisation).  Single-process only."""

    def __init__(self, model, temperature: float = 0.1, lr_backbone: float = 1e-4, lr_head: float = 1e-3, weight_decay: float = 0.01, ops=None):
        if not hasattr(model.head, 'fc1') or hasattr(model.head, 'fc2'):
            raise ValueError("OneShotStep needs ActionNet(version='embed')")
        self.temperature, self.ops = float(temperature), ops
        super().__init__(model, lr_backbone, lr_head, weight_decay)

    def __call__(self, batch_input: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        head = self.model.head
        z = head.fc1(head.pooled(self.model.backbone, batch_input))           # [N, hidden], before F.normalize
        self.zero_grad()
        loss = supcon_loss(z.reshape(len(batch_input), -1, z.shape[-1]), labels, temperature=self.temperature, normalize=True, ops=self.ops)
        loss.backward()
        self.step()
        return loss.detach()


def _embed(model, batch):
    with torch.no_grad():
        return model(batch)


class OneShotEvaluator:
    """1-nearest-neighbour accuracy by cosine similarity (train_action_1shot.py:58-69), accumulated on the device.

        ev = OneShotEvaluator()
        ev.set_anchors(model, anchor_loader)          # or ev.set_anchors(feats [M,D], labels [M])
        for batch, labels in test_loader: ev.update(model, batch.cuda(), labels)
        acc = ev.finish()

    `update` runs an eval-mode no-grad forward and `mbx_nn_cosine` and returns the batch's predictions; the hit count stays on the device and `finish()`
    is the only host synchronisation.  `ops`: kernel provider (default: libmbx.so, tensors on the ROCm device)."""

    def __init__(self, ops=None, device=None):
        self.ops, self.device = hip_ops.evaluator_provider(ops, device, 'motionbert_amd.oneshot.OneShotEvaluator')
        self.anchors = self.anchor_labels = None
        self.reset()

    def reset(self):
        """Forget the test rows seen so far (the exemplars stay)."""
        self.hits = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.count = 0

    def set_anchors(self, a, b):
        """`set_anchors(model, loader)`: the exemplar embeddings of every `(batch, labels)` of the loader; or
        `set_anchors(feats [M,D], labels [M])`."""
        if isinstance(a, torch.Tensor):
            feats, labels = a, torch.as_tensor(b)
        else:
            a.eval()
            fs, ls = [], []
            for batch, lab in b:
                fs.append(_embed(a, batch.to(self.device)))
                ls.append(torch.as_tensor(lab))
            if not fs:
                raise ValueError('set_anchors: the exemplar loader is empty')
            feats, labels = torch.cat(fs), torch.cat(ls)
        if feats.dim() != 2 or feats.shape[0] < 1 or labels.reshape(-1).shape[0] != feats.shape[0]:
            raise ValueError(f'exemplars [M,D] with M >= 1 and labels [M] expected, got {tuple(feats.shape)} / {tuple(labels.shape)}')
        self.anchors = feats.detach().to(self.device).float().contiguous()
        self.anchor_labels = labels.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        self.reset()

    def update(self, model, batch: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """Embeds `batch` (eval mode, no grad), classifies its rows and counts the hits.  Returns the predicted labels (device, i32)."""
        if self.anchors is None:
            raise RuntimeError('update() before set_anchors()')
        if hasattr(model, 'eval'):
            model.eval()
        feats = _embed(model, batch.to(self.device)).float().contiguous()
        lab = torch.as_tensor(labels).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if feats.dim() != 2 or feats.shape[1] != self.anchors.shape[1] or lab.shape[0] != feats.shape[0]:
            raise ValueError(f'embeddings [n,{self.anchors.shape[1]}] and labels [n] expected, got {tuple(feats.shape)} / {tuple(lab.shape)}')
        pred = torch.empty(feats.shape[0], dtype=torch.int32, device=self.device)
        if feats.shape[0]:
            self.ops.nn_cosine(self.anchors, self.anchor_labels, feats, lab, pred, None, self.hits)
        self.count += feats.shape[0]
        return pred

    def finish(self) -> float:
        """Accuracy over the test rows seen since set_anchors() / reset(): the one host synchronisation."""
        if self.count == 0:
            raise RuntimeError('finish() before any update()')
        return int(self.hits.cpu()[0]) / self.count


def validate(anchor_loader, test_loader, model, ops=None, device=None):
    """Drop-in for the reference's `validate(anchor_loader, test_loader, model)` (train_action_1shot.py:58-69): the 1-NN accuracy of
    the test split against the exemplars, as a 0-dim tensor like the reference's `sum(pred == labels) / len(pred)`."""
    if ops is None and device is None:
        device = hip_ops.model_device(model, 'motionbert_amd.oneshot.validate')
    ev = OneShotEvaluator(ops=ops, device=device)
    ev.set_anchors(model, anchor_loader)
    for batch, labels in test_loader:
        ev.update(model, batch, labels)
    return torch.tensor(ev.finish())
