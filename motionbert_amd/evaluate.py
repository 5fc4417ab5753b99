"""H36M evaluation on the device: Protocol #1 (MPJPE) and Protocol #2 (Procrustes MPJPE) of train.py:56-153.

The reference copies every prediction to the host, walks the test clips in a Python loop, runs a batched numpy SVD over every
frame (lib/model/loss.py:16-51) and accumulates per-frame errors with fancy indexing.  Here the predictions never leave the
device: `mbx_pose_errors` turns a batch of network outputs into per-frame errors (fp64) right after the forward, and
`mbx_eval_reduce` does the aggregation -- mean over the clips that cover a test frame, mean over the frames of an action, mean
over the actions -- in a fixed summation order.  `finish()` is the only host synchronisation of an evaluation epoch.

    pose_errors(pred, gt, ...)          per-frame (e1, e2); on [N,J,3] inputs the device form of loss.mpjpe / loss.p_mpjpe
    H36MEvaluator(...)                  update(model, batch) per batch, finish() -> (e1_mm, e2_mm, {action: (e1, e2)})
    evaluate(args, model, loader, dr)   the reference's signature and return triple, for a caller that has its DataReaderH36M

Degenerate frames: a frame whose prediction or ground truth has zero extent (all joints equal) makes the alignment divide 0 by 0,
here as in the reference: its e2 is NaN.  The aggregation keeps a test frame when its mean e1 is > 0 (train.py:132), which drops
frames that were never covered, frames whose e1 is exactly 0 and frames whose e1 is NaN; a NaN e2 next to a positive e1 reaches
the action mean, exactly as it does in the reference.

There is no CPU path: tensors that are not on a ROCm device raise.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip_ops

#: train.py:109-111: test sources left out of both protocols
BLOCK_LIST = ('s_09_act_05_subact_02', 's_09_act_10_subact_02', 's_09_act_13_subact_01')


def _f32(t: Optional[torch.Tensor]):
    return None if t is None else t.contiguous().float()


def pose_errors(pred: torch.Tensor, gt: torch.Tensor, *, hw: Optional[torch.Tensor] = None, factor: Optional[torch.Tensor] = None,
                rootrel: bool = False, gt_2d_input: Optional[torch.Tensor] = None, ops=None,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-frame MPJPE and Procrustes MPJPE (fp64 device tensors, no host synchronisation).

    pred, gt [N,T,J,3] (or [N,J,3]: N single frames).  In the reference's order: `rootrel` zeroes joint 0 of pred; `gt_2d_input`
    (the model input [N,T,J,>=2]) replaces x and y of pred; `hw` [N,2] = (res_w, res_h) per clip denormalises pred
    (datareader_h36m.py:125-136); `factor` [N,T] scales it; both poses are made root-relative; then lib/model/loss.py:8-51.
    Without hw / factor / rootrel this is loss.mpjpe and loss.p_mpjpe of the root-relative poses, as train.py:124-127 calls them
    (p_mpjpe does not see the root shift; mpjpe equals loss.mpjpe(pred, gt) when joint 0 of both poses is at the same point).
    `ops`: kernel provider (default: libmbx.so).  `out`: (e1, e2) fp64 tensors to write into."""
    single = pred.dim() == 3
    if single:
        pred, gt = pred.unsqueeze(1), gt.unsqueeze(1)
        gt_2d_input = None if gt_2d_input is None else gt_2d_input.unsqueeze(1)
        factor = None if factor is None else factor.reshape(-1, 1)
    if pred.dim() != 4 or pred.shape[-1] != 3 or gt.shape != pred.shape:
        raise ValueError(f'pose_errors needs pred, gt [N,T,J,3] or [N,J,3], got {tuple(pred.shape)} / {tuple(gt.shape)}')
    N, T, J, _ = pred.shape
    if hw is not None and tuple(hw.shape) != (N, 2):
        raise ValueError(f'hw must be [N,2] = (res_w, res_h) per clip, got {tuple(hw.shape)}')
    if factor is not None and factor.numel() != N * T:
        raise ValueError(f'factor must be [N,T], got {tuple(factor.shape)}')
    if gt_2d_input is not None and (gt_2d_input.dim() != 4 or tuple(gt_2d_input.shape[:3]) != (N, T, J) or gt_2d_input.shape[-1] < 2):
        raise ValueError(f'gt_2d_input must be [N,T,J,>=2], got {tuple(gt_2d_input.shape)}')
    ops = hip_ops.provider(ops, 'motionbert_amd.evaluate.pose_errors', pred, gt, hw, factor, gt_2d_input)
    if out is None:
        e1 = torch.empty(N, T, dtype=torch.float64, device=pred.device)
        e2 = torch.empty(N, T, dtype=torch.float64, device=pred.device)
    else:
        e1, e2 = out
        if any(e.dtype != torch.float64 or e.numel() != N * T or not e.is_contiguous() or e.device != pred.device for e in (e1, e2)):
            raise ValueError('out must be two contiguous fp64 tensors of N*T elements on the device of pred')
    if N * T:
        ops.pose_errors(_f32(pred), _f32(gt), _f32(hw), _f32(factor), _f32(gt_2d_input), bool(rootrel), e1, e2)
    return (e1.reshape(N), e2.reshape(N)) if single else (e1, e2)


def build_frame_csr(frame_clips: np.ndarray, keep_clip: np.ndarray, n_frames: int) -> Tuple[np.ndarray, np.ndarray]:
    """(row_ptr [F+1], slots [nnz]) int32: for every test frame the slots clip * T + t of the kept clips that cover it, in clip order.
    A clip that lists a frame twice (split_clips resamples a source shorter than the clip, utils_data.py:106-109) counts once, with
    its LAST listing: that is what `e1_all[frame_list] += err1` (train.py:128-130) does with a repeated index."""
    frame_clips = np.asarray(frame_clips, dtype=np.int64)
    Nc, T = frame_clips.shape
    if frame_clips.size and (frame_clips.min() < 0 or frame_clips.max() >= n_frames):
        raise ValueError('frame_clips holds a frame index outside the test set')
    clip = np.repeat(np.arange(Nc, dtype=np.int64), T)
    slot = np.arange(Nc * T, dtype=np.int64)
    frame = frame_clips.reshape(-1)
    on = np.repeat(np.asarray(keep_clip, dtype=bool), T)
    clip, slot, frame = clip[on], slot[on], frame[on]
    _, first_rev = np.unique((clip * n_frames + frame)[::-1], return_index=True)      # first in reversed order = last listing
    sel = np.sort(len(slot) - 1 - first_rev)
    slot, frame = slot[sel], frame[sel]                                               # still in clip order
    order = np.argsort(frame, kind='stable')
    row_ptr = np.zeros(n_frames + 1, dtype=np.int64)
    np.cumsum(np.bincount(frame, minlength=n_frames), out=row_ptr[1:])
    if Nc * T >= 2 ** 31:
        raise ValueError('too many clip frames for 32-bit slots')
    return row_ptr.astype(np.int32), slot[order].astype(np.int32)


class H36MEvaluator:
    """Protocol #1 / #2 over a test split, accumulated on the device batch by batch.

    gt_clips [Nc,T,J,3], factor_clips [Nc,T], frame_clips [Nc,T] (test-frame index of every clip frame) are the reference's
    `gts[split_id_test]`, `factors[split_id_test]`, `frames[split_id_test]`; hw_clips [Nc,2] = DataReaderH36M.get_hw() (None: the
    predictions are not denormalised); actions [F] and sources [F] are the per-test-frame lists of the dataset (train.py:86-97).
    A clip's source is that of its first frame without the 6-character camera suffix (train.py:113).

    The constructor builds the frame -> slots table and the action table once and moves them to `device`; `update(model, batch)`
    must see the clips in order; `finish()` is the only call that synchronises."""

    def __init__(self, gt_clips, factor_clips, frame_clips, hw_clips, actions, sources, *, rootrel: bool, flip: bool, gt_2d: bool = False,
                 no_conf: bool = False, block_list: Sequence[str] = BLOCK_LIST, ops=None, device=None):
        ops, device = hip_ops.evaluator_provider(ops, device, 'motionbert_amd.evaluate.H36MEvaluator')
        self.ops, self.device = ops, device
        self.rootrel, self.flip, self.gt_2d, self.no_conf = bool(rootrel), bool(flip), bool(gt_2d), bool(no_conf)
        gt_clips = np.asarray(gt_clips)
        frame_clips = np.asarray(frame_clips, dtype=np.int64)
        actions, sources = np.asarray(actions), np.asarray(sources)
        if gt_clips.ndim != 4 or gt_clips.shape[-1] != 3 or frame_clips.shape != gt_clips.shape[:2]:
            raise ValueError(f'gt_clips [Nc,T,J,3] / frame_clips [Nc,T] expected, got {gt_clips.shape} / {frame_clips.shape}')
        self.n_clips, self.T, self.J, _ = gt_clips.shape
        if len(actions) != len(sources):
            raise ValueError('actions and sources are per test frame and must have the same length')
        self.n_frames = len(actions)
        self.action_names = sorted(set(actions.tolist()))
        action_id = np.searchsorted(np.array(self.action_names), actions).astype(np.int32)
        blocked = set(block_list)
        self.keep_clip = np.array([str(sources[f])[:-6] not in blocked for f in frame_clips[:, 0]], dtype=bool) if self.n_clips else np.zeros(0, bool)
        row_ptr, slots = build_frame_csr(frame_clips, self.keep_clip, self.n_frames)
        self.row_ptr_host, self.slots_host = row_ptr, slots

        def dev(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)
        self.gt = dev(gt_clips, torch.float32)
        self.factor = None if factor_clips is None else dev(np.asarray(factor_clips).reshape(self.n_clips, self.T), torch.float32)
        self.hw = None if hw_clips is None else dev(np.asarray(hw_clips).reshape(self.n_clips, 2), torch.float32)
        self.row_ptr, self.slots, self.action_id = dev(row_ptr, torch.int32), dev(slots, torch.int32), dev(action_id, torch.int32)
        self.e1 = torch.zeros(self.n_clips, self.T, dtype=torch.float64, device=device)
        self.e2 = torch.zeros(self.n_clips, self.T, dtype=torch.float64, device=device)
        A = len(self.action_names)
        self.per_action = torch.empty(2, A, dtype=torch.float64, device=device)
        self.summary = torch.empty(2, dtype=torch.float64, device=device)
        self.count = torch.empty(A, dtype=torch.int32, device=device)
        self.cursor = 0

    def reset(self):
        self.cursor = 0

    def update(self, model, batch_input: torch.Tensor) -> torch.Tensor:
        """Forward of the next len(batch_input) clips (flip test-time augmentation when `flip`), their errors into the slots of
        those clips.  Returns the raw network output of the batch (a fresh tensor the caller may write into)."""
        if self.device.type == 'cuda':
            hip_ops.provider(None, 'motionbert_amd.evaluate.H36MEvaluator.update', batch_input)
        n0, n1 = self.cursor, self.cursor + batch_input.shape[0]
        if n1 > self.n_clips:
            raise ValueError(f'update() was given clips {n0}..{n1 - 1} of a split of {self.n_clips}')
        x = batch_input[..., :2] if self.no_conf else batch_input                   # train.py:65-66
        if self.flip:
            from .augment import flip_tta
            pred = flip_tta(model, x)                                               # train.py:67-72
        else:
            with torch.no_grad():
                pred = model(x)
        if n1 > n0:
            pose_errors(pred, self.gt[n0:n1], hw=None if self.hw is None else self.hw[n0:n1],
                        factor=None if self.factor is None else self.factor[n0:n1], rootrel=self.rootrel,
                        gt_2d_input=batch_input if self.gt_2d else None, ops=self.ops, out=(self.e1[n0:n1], self.e2[n0:n1]))
        self.cursor = n1
        return pred

    def finish(self) -> Tuple[float, float, Dict[str, Tuple[float, float]]]:
        """(e1_mm, e2_mm, {action: (e1_mm, e2_mm)}) over the clips seen so far (all of them for the reference's numbers)."""
        if self.cursor != self.n_clips:
            raise RuntimeError(f'finish() after {self.cursor} of {self.n_clips} clips: the slots of the others hold no errors yet')
        self.ops.eval_reduce(self.e1, self.e2, self.row_ptr, self.slots, self.action_id, len(self.action_names), self.per_action,
                             self.summary, self.count)
        per = self.per_action.cpu().numpy()                                         # the one synchronisation
        summ = self.summary.cpu().numpy()
        return float(summ[0]), float(summ[1]), {a: (float(per[0, i]), float(per[1, i])) for i, a in enumerate(self.action_names)}


def denormalize(results: np.ndarray, hw_clips: np.ndarray) -> np.ndarray:
    """DataReaderH36M.denormalize (datareader_h36m.py:125-136) on [Nc,T,J,3] fp32 predictions, in place, without the 17-joint
    reshape: xy = (xy + [1, h/w]) w/2, z = z w/2 with (w, h) = hw_clips[clip]."""
    hw = np.asarray(hw_clips, dtype=np.float64)
    assert len(results) == len(hw)
    w, h = hw[:, 0].reshape(-1, 1, 1, 1), hw[:, 1].reshape(-1, 1, 1, 1)
    results[..., :2] = (results[..., :2] + np.concatenate([np.ones_like(w), h / w], axis=-1)) * w / 2
    results[..., 2:] = results[..., 2:] * w / 2
    return results


def evaluate(args, model_pos, test_loader, datareader):
    """Drop-in for the reference's `evaluate(args, model_pos, test_loader, datareader)` (train.py:56-153): returns
    (e1, e2, results_all).  `datareader` is read through its public side only: `dt_dataset['test']`, `get_split_id()` and
    `get_hw()`.  `results_all` [Nc,T,J,3] fp32 is the denormalised prediction (after rootrel / gt_2d), copied to the host once at
    the end; the reference additionally leaves the 2.5D factor multiplied into the clips of unblocked sources, a side effect of
    `pred *= factor` on a view (train.py:120-121), which is not reproduced.  The per-action numbers are not printed: use
    H36MEvaluator.finish() for them."""
    device = hip_ops.model_device(model_pos, 'motionbert_amd.evaluate.evaluate')
    model_pos.eval()
    _, split_id_test = datareader.get_split_id()
    test = datareader.dt_dataset['test']
    actions, sources = np.array(test['action']), np.array(test['source'])
    factors, gts = np.array(test['2.5d_factor']), np.array(test['joints_2.5d_image'])
    split = np.stack([np.asarray(s, dtype=np.int64) for s in split_id_test]) if len(split_id_test) else np.zeros((0, 1), np.int64)
    hw = np.asarray(datareader.get_hw())
    rootrel, gt_2d = bool(getattr(args, 'rootrel', False)), bool(getattr(args, 'gt_2d', False))
    with torch.cuda.device(device):
        ev = H36MEvaluator(gts[split], factors[split], split, hw, actions, sources, rootrel=rootrel, flip=bool(getattr(args, 'flip', False)),
                           gt_2d=gt_2d, no_conf=bool(getattr(args, 'no_conf', False)), device=device)
        preds = []
        for batch_input, _ in test_loader:
            batch_input = batch_input.to(device)
            pred = ev.update(model_pos, batch_input)
            if rootrel:
                pred[:, :, 0, :] = 0                                                # train.py:75-76
            if gt_2d:
                pred[..., :2] = batch_input[..., :2]                                # train.py:80-81
            preds.append(pred)
        assert ev.cursor == ev.n_clips, (ev.cursor, ev.n_clips)                     # train.py:98
        e1, e2, _ = ev.finish()
        results_all = torch.cat(preds).cpu().numpy() if preds else np.zeros((0, ev.T, ev.J, 3), np.float32)
    return e1, e2, denormalize(results_all, hw)
