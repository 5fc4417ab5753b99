"""In-the-wild inference on the device: AlphaPose detections in, 3D poses out (reference `infer_wild.py:56-97` +
`lib/data/dataset_wild.py`, without the video reader and the renderer).

    kp = read_alphapose('alphapose-results.json', focus=1)           # [F,26,3] float64, host
    poses = infer(model, kp)                                          # [F,17,3] float32, numpy
    tracks = read_alphapose('alphapose-results.json', by_track=True)  # idx -> [F_idx,26,3]
    poses = infer(model, tracks, vid_size=(1920, 1080), pixel=True)   # idx -> [F_idx,17,3], every tracked person in one pass
    tracks, frame_ids = read_alphapose('alphapose-results.json', by_track=True, frames=True)      # + idx -> the video frame of every row:
                                                                      # render.scene_table / render_scene / video.scene_video draw them all

The reference runs one clip per forward at batch 1, two forwards per clip for the flip, two deep copies in `flip_data`, a `.cpu()` per
clip, a numpy input stage on the host and one person per run (`--focus`).  Here the detections are uploaded once, `mbx_wild_input`
(halpe2h36m + pixel / crop normalisation, float64 arithmetic in the reference's order: its bits) writes the network input of every
track, the clips of all tracks are pooled into batches (`clip_plan`: full clips together, tails grouped by equal length), every batch is
one `flip_tta` forward, `mbx_wild_output` writes each batch straight into its rows of ONE stitched result, and one device-to-host copy
ends the run.

    read_alphapose   the JSON part of `read_input` (dataset_wild.py:67-76); host only
    wild_input       halpe2h36m + normalisation (:77-86) on the device
    clip_plan        the clips of `WildDetDataset` (:94-102) pooled over tracks; host only
    ragged_plan      the same clips in frame order, cut into batches of whole clips of any length (`infer(batching='ragged')`); host only
    wild_output      infer_wild.py:81-96 for one batch of clips
    infer            the loop of infer_wild.py:56-97

Mesh recovery in the wild (reference `infer_wild_mesh.py:42-56,99-154`) shares the input stage, the plan and the batching:

    meshes = infer_mesh(model, smpl, kp, ref_3d=X3D)                  # {'verts': [F,V,3] mm, 'kp_3d': [F,17,3], 'scale': float}

    infer_mesh       the loop of infer_wild_mesh.py:108-146: per batch the backbone and the head's parameters for x and flip_data(x), and ONE
                     `mbx_wild_mesh` launch that evaluates SMPL for both parameter sets and writes their mean into the stitched rows
    solve_scale      infer_wild_mesh.py:42-56 as one `mbx_scale_fit` launch: the convex fit solved by iteratively reweighted least squares
                     where the reference runs 400 starts of `scipy.optimize.least_squares` on the host
    place            infer_wild_mesh.py:153-154 in place (`mbx_wild_mesh_place`)

There is no CPU path: without an injected kernel provider (`ops=`) the tensors live on the ROCm device and libmbx.so does the work."""
from __future__ import annotations

import json
import math
import os
from collections import OrderedDict
from contextlib import nullcontext as _nullcontext
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip_ops

#: frames per chunk of the box reduction (MBX_WILD_CHUNK in include/mbx.h); a chunk never spans tracks
CHUNK_FRAMES = 64
PIXEL, CROP = 1, 2                       # flags of mbx_wild_input
ROOTREL, GT_2D, OUT_PIXEL = 1, 2, 4      # flags of mbx_wild_output


# ---------------------------------------------------------------------------------------------------------------- host: the JSON
def _frame_id(image_id, json_path, n) -> int:
    """the video frame an AlphaPose item belongs to: its `image_id` as an int, or the decimal file stem of a string"""
    if isinstance(image_id, int) and not isinstance(image_id, bool):
        return image_id
    if isinstance(image_id, str):
        stem = os.path.splitext(os.path.basename(image_id))[0]
        if stem.isascii() and stem.isdigit():
            return int(stem)
    raise ValueError(f'{json_path}: item {n} has image_id {image_id!r}; an int or a file name with a decimal stem expected')


def read_alphapose(json_path, focus=None, by_track: bool = False, frames: bool = False):
    """The detections of an AlphaPose result file (Halpe-26): items in file order, `keypoints` reshaped to [-1,3], float64
    (dataset_wild.py:67-76).  `focus`: only the items with that `idx`, as the reference filters.  Returns [F,26,3]; with
    `by_track=True` an ordered dict idx -> [F_idx,26,3], the keys in order of first appearance, file order inside a track.
    ValueError on a joint count other than 26, on non-finite values and on an empty selection.
    `frames=True` returns `(detections, frame_ids)`: the video frame of every row, int64 [F] (with `by_track=True` a dict idx -> int64
    [F_idx]), from each item's `image_id`: an int, or a string whose file stem is a decimal number ('17.jpg' -> 17).  ValueError, naming the
    item, on any other `image_id` and where the frame ids of a track do not rise strictly in file order.  It is what `render.scene_table`
    takes to put every track of a crowd back into the frames of the video."""
    with open(json_path, 'r') as f:
        results = json.load(f)
    tracks: Dict[object, List[np.ndarray]] = OrderedDict()
    ids: Dict[object, List[int]] = OrderedDict()
    for n, item in enumerate(results):
        if focus is not None and item['idx'] != focus:
            continue
        kpts = np.array(item['keypoints'], dtype=np.float64).reshape([-1, 3])
        if kpts.shape[0] != 26:
            raise ValueError(f'{json_path}: item {n} has {kpts.shape[0]} joints; Halpe-26 detections expected')
        if not np.isfinite(kpts).all():
            raise ValueError(f'{json_path}: item {n} has non-finite keypoints')
        tracks.setdefault(item['idx'] if by_track else None, []).append(kpts)
        if frames:
            seen = ids.setdefault(item['idx'] if by_track else None, [])
            frame = _frame_id(item.get('image_id'), json_path, n)
            if seen and frame <= seen[-1]:
                raise ValueError(f'{json_path}: item {n} is frame {frame} after frame {seen[-1]} of the same track; frame ids must rise strictly')
            seen.append(frame)
    if not tracks:
        raise ValueError(f'{json_path}: no detections' + ('' if focus is None else f' with idx == {focus!r}'))
    if by_track:
        det = OrderedDict((k, np.stack(v)) for k, v in tracks.items())
        return (det, OrderedDict((k, np.asarray(v, dtype=np.int64)) for k, v in ids.items())) if frames else det
    return (np.stack(tracks[None]), np.asarray(ids[None], dtype=np.int64)) if frames else np.stack(tracks[None])


# ---------------------------------------------------------------------------------------------------------------- host: plans
def _check_lens(seq_lens, F=None) -> List[int]:
    lens = [int(v) for v in seq_lens]
    if not lens or any(v < 0 for v in lens):
        raise ValueError(f'seq_lens must be a non-empty list of track lengths >= 0, got {list(seq_lens)}')
    if F is not None and sum(lens) != F:
        raise ValueError(f'seq_lens {lens} sum to {sum(lens)}, not to the {F} frames given')
    return lens


def chunk_table(seq_lens) -> Tuple[np.ndarray, np.ndarray]:
    """(chunk_tab [n_chunks,3] int32 = (track, first frame, frames), seq_chunk_ptr [S+1] int32) for mbx_wild_input: every track cut into
    chunks of at most CHUNK_FRAMES frames; a chunk never spans tracks."""
    lens = _check_lens(seq_lens)
    rows, ptr, start = [], [0], 0
    for s, n in enumerate(lens):
        for f0 in range(0, n, CHUNK_FRAMES):
            rows.append((s, start + f0, min(CHUNK_FRAMES, n - f0)))
        ptr.append(len(rows))
        start += n
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3), np.asarray(ptr, dtype=np.int32)


def clip_plan(seq_lens, clip_len: int) -> List[Tuple[int, List[int]]]:
    """The reference's clips (`WildDetDataset.__len__ / __getitem__`: ceil(F / clip_len) per track, the last one shorter) pooled over the
    tracks of `seq_lens`: a list of groups `(T, [frame offsets])`.  The full clips of all tracks come first, as one group in frame order; then
    the tails, grouped by equal length in order of first appearance.  A clip's offset is its first row in the frame-major arrays of all
    tracks one after another: where it is read from the network input and where its poses go in the result."""
    lens = _check_lens(seq_lens)
    clip_len = int(clip_len)
    if clip_len < 1:
        raise ValueError(f'clip_len must be >= 1, got {clip_len}')
    full: List[int] = []
    tails: Dict[int, List[int]] = OrderedDict()
    start = 0
    for n in lens:
        for i in range(math.ceil(n / clip_len)):
            st, end = i * clip_len, min((i + 1) * clip_len, n)
            if end - st == clip_len:
                full.append(start + st)
            else:
                tails.setdefault(end - st, []).append(start + st)
        start += n
    return ([(clip_len, full)] if full else []) + list(tails.items())


def ragged_plan(seq_lens, clip_len: int, max_frames: int) -> List[Tuple[int, List[int]]]:
    """The same clips as `clip_plan` (ceil(F / clip_len) per track, the last one shorter), kept in frame order and cut into ragged
    batches: a list of `(first row, [clip lengths])`.  A batch holds whole consecutive clips, as many as fit into `max_frames` frames
    (>= clip_len), so it is the view `y[first row : first row + sum(clip lengths)]` of the frame-major arrays of all tracks one after
    another; a clip never spans tracks, and every frame lies in exactly one clip of one batch."""
    lens = _check_lens(seq_lens)
    clip_len, max_frames = int(clip_len), int(max_frames)
    if clip_len < 1 or max_frames < clip_len:
        raise ValueError(f'clip_len must be >= 1 and max_frames >= clip_len, got {clip_len} and {max_frames}')
    plan: List[Tuple[int, List[int]]] = []
    row0, cur, start = 0, [], 0
    for n in lens:
        for st in range(0, n, clip_len):
            c = min(clip_len, n - st)
            if cur and sum(cur) + c > max_frames:
                plan.append((row0, cur))
                row0, cur = start + st, []
            cur.append(c)
        start += n
    if cur:
        plan.append((row0, cur))
    return plan


# ---------------------------------------------------------------------------------------------------------------- device stages
def _provider(ops, where: str, t):
    """(ops, device): an injected provider keeps the tensors where they are (the host for arrays); otherwise libmbx.so on the ROCm device"""
    if ops is not None:
        return ops, (t.device if isinstance(t, torch.Tensor) else torch.device('cpu'))
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return hip_ops.get(), t.device
    if not torch.cuda.is_available():
        raise RuntimeError(f'{where} runs on the ROCm device; there is no CPU path')
    return hip_ops.get(), torch.device('cuda', torch.cuda.current_device())


def _on(dev):
    return torch.cuda.device(dev) if dev.type == 'cuda' else _nullcontext()


def _pixel_consts(vid_size):
    w, h = vid_size
    if not (w > 0 and h > 0):
        raise ValueError(f'vid_size must be (w, h) > 0, got {vid_size!r}')
    return float(np.float64(w) / 2.0), float(np.float64(h) / 2.0), float(min(w, h) / 2.0)      # dataset_wild.py:79-81


def wild_input(kp, vid_size=None, scale_range=None, seq_lens=None, channels: int = 3, return_box: bool = False, ops=None):
    """`halpe2h36m` + the normalisation of `read_input` (dataset_wild.py:77-86) on the device, bit for bit.  kp [F,26,3] float64 (tensor or
    array; uploaded once) -> [F,17,channels] float32 on the device.  `seq_lens`: track lengths summing to F (default: one track); every
    track gets its own crop box.

    Pixel mode, `vid_size=(w, h)`: (xy - (w, h) / 2) / (min(w, h) / 2).  Crop mode, `scale_range=[r, r]`: `crop_scale` over the whole track
    -- the box over the joints whose mapped confidence is != 0; fewer than 4 of them, or scale == 0, gives an all-zero track (all three
    channels); every channel clipped to [-1, 1]; joints without confidence are still transformed.  With both, pixel mode runs first, as in
    the reference; with neither, ValueError (the reference dies with UnboundLocalError).  A range with lo != hi draws a random ratio per
    call: that belongs to training and is refused.  `channels=2` drops the confidence (args.no_conf), written directly.  Rows are
    clip-contiguous: clip i of a track is the view `y[start + i * clip_len : start + (i + 1) * clip_len]`.
    `return_box=True`: `(y, box)` with box [S,4] float64 = (xs, ys, scale, valid joints) per track, (0, 0, 0, valid joints) for a zeroed
    one: crop-mode xy map back through  (v / 2 + 0.5) * scale + (xs, ys)."""
    if not vid_size and not scale_range:
        raise ValueError('wild_input needs vid_size (pixel mode), scale_range (crop mode) or both')
    if channels not in (2, 3):
        raise ValueError(f'channels must be 2 or 3, got {channels}')
    flags, half_w, half_h, pix_scale, ratio = 0, 0.0, 0.0, 1.0, 1.0
    if vid_size:
        flags |= PIXEL
        half_w, half_h, pix_scale = _pixel_consts(vid_size)
    if scale_range:
        lo, hi = scale_range
        if lo != hi:
            raise ValueError(f'scale_range {list(scale_range)} draws a random crop ratio: that is a training augmentation; inference passes [r, r] '
                             f'(the reference: [1, 1])')
        flags |= CROP
        ratio = float(lo)
    ops, dev = _provider(ops, 'motionbert_amd.wild.wild_input', kp)
    if not isinstance(kp, torch.Tensor):
        kp = torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float64))
    if kp.dim() != 3 or tuple(kp.shape[1:]) != (26, 3):
        raise ValueError(f'expected Halpe-26 detections [F,26,3], got {tuple(kp.shape)}')
    F = kp.shape[0]
    lens = _check_lens([F] if seq_lens is None else seq_lens, F)
    kp = kp.to(device=dev, dtype=torch.float64).contiguous()
    y = torch.empty(F, 17, channels, dtype=torch.float32, device=dev)
    box = torch.zeros(len(lens), 4, dtype=torch.float64, device=dev) if return_box else None
    if F:
        tab, ptr = chunk_table(lens)
        both = torch.from_numpy(np.concatenate([tab.reshape(-1), ptr])).to(dev)               # one upload
        with _on(dev):
            ops.wild_input(kp, both[:tab.size].view(-1, 3), both[tab.size:], half_w, half_h, pix_scale, ratio, flags, y, box)
    return (y, box) if return_box else y


def _out_flags(rootrel, gt_2d, vid_size):
    flags, half_w, half_h, pix_scale = (ROOTREL if rootrel else 0) | (GT_2D if gt_2d else 0), 0.0, 0.0, 1.0
    if vid_size:
        flags |= OUT_PIXEL
        half_w, half_h, pix_scale = _pixel_consts(vid_size)        # infer_wild.py:95-96: min(vid_size) / 2.0 and np.array(vid_size) / 2.0
    return flags, half_w, half_h, pix_scale


def wild_output(pred: torch.Tensor, dst: torch.Tensor, dst_frames: Sequence[int], x: Optional[torch.Tensor] = None, rootrel: bool = False,
                gt_2d: bool = False, vid_size=None, ops=None):
    """The output stage of infer_wild.py:81-96 for a batch: pred [n,T,17,3] float32 (not modified; the reference writes in place) goes to
    rows dst_frames[i] .. dst_frames[i] + T - 1 of dst [F,17,3] float32 (`dst_frames`: host integers).  `rootrel`: joint 0 of every frame
    is 0; otherwise only [clip, frame 0, joint 0, z] is (a quirk of the reference, kept).  `gt_2d`: xy from the network input x
    [n,T,17,2|3].  `vid_size=(w, h)`: pixel coordinates in numpy's arithmetic there -- the float32 product p * float32(min(w, h) / 2),
    and for xy that product widened to float64, (w, h) / 2 added, the sum rounded to float32.  Returns dst."""
    if pred.dim() != 4 or tuple(pred.shape[2:]) != (17, 3):
        raise ValueError(f'expected pred [n,T,17,3], got {tuple(pred.shape)}')
    n, T = pred.shape[:2]
    frames = [int(v) for v in dst_frames]
    if len(frames) != n:
        raise ValueError(f'{n} clips but {len(frames)} destination offsets')
    if dst.dim() != 3 or tuple(dst.shape[1:]) != (17, 3) or dst.dtype != torch.float32 or not dst.is_contiguous():
        raise ValueError(f'expected a contiguous float32 dst [F,17,3], got {tuple(dst.shape)} {dst.dtype}')
    if any(not 0 <= v <= dst.shape[0] - T for v in frames):
        raise ValueError(f'a clip of {T} frames at one of the offsets {frames} does not fit dst [{dst.shape[0]},17,3]')
    if gt_2d and x is None:
        raise ValueError('gt_2d takes xy from the network input: pass x')
    ops = hip_ops.provider(ops, 'motionbert_amd.wild.wild_output', pred, dst, x, move='pred, dst and x')
    flags, half_w, half_h, pix_scale = _out_flags(rootrel, gt_2d, vid_size)
    if n:
        table = torch.tensor(frames, dtype=torch.int32).to(pred.device)
        with _on(pred.device):
            ops.wild_output(pred.contiguous().float(), None if x is None else x.contiguous().float(), table, max(frames), flags, pix_scale, half_w,
                            half_h, dst)
    return dst


def _tracks(kp_or_tracks):
    """(kp, lens or None, keys or None) of one person's detections or of a dict idx -> [F_idx,26,3]: the tracks one after another"""
    if not isinstance(kp_or_tracks, dict):
        return kp_or_tracks, None, None
    if not kp_or_tracks:
        raise ValueError('no tracks')
    keys = list(kp_or_tracks)
    parts = [kp_or_tracks[k] for k in keys]
    for k, p in zip(keys, parts):
        if len(p.shape) != 3 or tuple(p.shape[1:]) != (26, 3):
            raise ValueError(f'track {k!r}: expected Halpe-26 detections [F,26,3], got {tuple(p.shape)}')
    lens = [int(p.shape[0]) for p in parts]
    if all(isinstance(p, torch.Tensor) for p in parts):
        kp = torch.cat([p.to(torch.float64) for p in parts])
    else:
        kp = np.concatenate([np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p, dtype=np.float64) for p in parts])
    return kp, lens, keys


def _batches(plan, max_batch):
    """(T, offsets) of every network call: each group of the plan in parts of at most max_batch clips"""
    for T, offs in plan:
        for b0 in range(0, len(offs), max_batch):
            yield T, offs[b0:b0 + max_batch]


def _clips(y, part, T):
    """[n,T,17,C]: the clips of y at the offsets `part` (consecutive clips: a view)"""
    n = len(part)
    if all(part[i + 1] - part[i] == T for i in range(n - 1)):
        return y[part[0]:part[0] + n * T].view(n, T, 17, y.shape[2])
    return torch.stack([y[o:o + T] for o in part])


def infer(model, kp_or_tracks, *, clip_len: int = 243, vid_size=None, pixel: bool = False, flip: bool = True, rootrel: bool = False,
          gt_2d: bool = False, no_conf: bool = False, max_batch: int = 64, batching: str = 'equal', ops=None):
    """The loop of infer_wild.py:56-97.  `kp_or_tracks`: [F,26,3] detections of one person (array or tensor) -> numpy [F,17,3] float32, or
    a dict idx -> [F_idx,26,3] (`read_alphapose(by_track=True)`) -> a dict idx -> [F_idx,17,3], every person in the same pass.

    Input stage as infer_wild.py:56-61: `pixel=True` means `vid_size` without a crop, otherwise `scale_range=[1, 1]`.  The full clips of
    all tracks go in batches of at most `max_batch`, each group of equal-length tail clips in batches of its own.  The network call is
    `flip_tta(model, x)` (`flip`) or `model(x)`, under no_grad and eval(); `rootrel`, `gt_2d`, `no_conf` are the config switches of the
    same names.  Every batch goes through `mbx_wild_output` into its rows of one [F,17,3] device tensor; one device-to-host copy ends the
    run.  A DataParallel-wrapped or a bare model is accepted; `clip_len > model.maxlen` raises.

    `batching='ragged'`: clips of DIFFERENT lengths share a network call (`ragged_plan`: whole consecutive clips in frame order, at most
    `max_batch * clip_len` frames per batch).  Every batch is a view of the input stage's output, one `forward_ragged` (through `flip_tta`
    with `flip`) and one `mbx_wild_output_ragged`; the clip tables of the whole run are uploaded once.  A scene of many short tracks then
    takes ceil(frames / (max_batch clip_len)) network calls instead of one per distinct tail length.  `clip_len <= 256`."""
    net = model.module if hasattr(model, 'module') else model
    clip_len, max_batch = int(clip_len), int(max_batch)
    if clip_len < 1 or max_batch < 1:
        raise ValueError(f'clip_len and max_batch must be >= 1, got {clip_len} and {max_batch}')
    if batching not in ('equal', 'ragged'):
        raise ValueError(f"batching must be 'equal' or 'ragged', got {batching!r}")
    if batching == 'ragged' and clip_len > 256:
        raise ValueError(f"batching='ragged' takes clips of at most 256 frames, got clip_len = {clip_len}")
    if batching == 'ragged' and not hasattr(net, 'forward_ragged'):
        raise TypeError("batching='ragged' needs a model with forward_ragged")
    maxlen = getattr(net, 'maxlen', None)
    if maxlen is not None and clip_len > maxlen:
        raise ValueError(f'clip_len {clip_len} is longer than the model takes (maxlen = {maxlen})')
    if pixel and not vid_size:
        raise ValueError('pixel=True needs vid_size=(w, h)')
    kp, lens, keys = _tracks(kp_or_tracks)
    as_dict = keys is not None
    if ops is None and not isinstance(kp, torch.Tensor):
        dev = hip_ops.model_device(net, 'motionbert_amd.wild.infer')
        kp = torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float64)).to(dev)             # the one upload
    y = wild_input(kp, vid_size=vid_size if pixel else None, scale_range=None if pixel else [1, 1], seq_lens=lens,
                   channels=2 if no_conf else 3, ops=ops)
    F, dev = y.shape[0], y.device
    lens = [F] if lens is None else lens
    out = torch.empty(F, 17, 3, dtype=torch.float32, device=dev)
    prov = hip_ops.provider(ops, 'motionbert_amd.wild.infer', y)
    flags, half_w, half_h, pix_scale = _out_flags(rootrel, gt_2d, vid_size if pixel else None)
    plan = clip_plan(lens, clip_len) if batching == 'equal' else []
    offsets = [o for _, offs in plan for o in offs]
    table = torch.tensor(offsets, dtype=torch.int32).to(dev) if offsets else None              # every batch's destinations, one upload
    if hasattr(model, 'eval'):
        model.eval()
    from .augment import flip_tta
    if batching == 'ragged':
        _infer_ragged(net, y, out, ragged_plan(lens, clip_len, max_batch * clip_len), flip, gt_2d, prov, flags, pix_scale, half_w, half_h)
    at = 0
    with torch.no_grad(), _on(dev):
        for T, part in _batches(plan, max_batch):
            n = len(part)
            x = _clips(y, part, T)
            pred = flip_tta(net, x) if flip else model(x)                                      # infer_wild.py:73-80
            prov.wild_output(pred.contiguous().float(), x if gt_2d else None, table[at:at + n], max(part), flags, pix_scale, half_w, half_h, out)
            at += n
    res = out.cpu().numpy()                                                                    # the one device-to-host copy
    if not as_dict:
        return res
    ends = np.cumsum(lens)
    return OrderedDict((k, res[e - n:e]) for k, e, n in zip(keys, ends, lens))


def _infer_ragged(net, y, out, plan, flip, gt_2d, prov, flags, pix_scale, half_w, half_h):
    """the batches of `ragged_plan` through the network and `wild_output_ragged`; the tables of all batches go up in one copy"""
    from .augment import flip_tta
    from .model import ragged_tables
    if not plan:
        return
    dev = y.device
    tabs = [ragged_tables(cl)[0] for _, cl in plan]               # firsts count from the batch's own first row
    frame_t = np.concatenate([ragged_tables(cl)[1] for _, cl in plan])
    n_tab = sum(t.size for t in tabs)
    both = torch.from_numpy(np.concatenate([t.reshape(-1) for t in tabs] + [frame_t])).to(dev)      # one upload
    at = 0
    with torch.no_grad(), _on(dev):
        for (row0, cl), tab in zip(plan, tabs):
            Fb = int(tab[:, 1].sum())
            x = y[row0:row0 + Fb]                                 # a view: whole consecutive clips
            ft = both[n_tab + row0:n_tab + row0 + Fb]
            tables = (both[at:at + tab.size].view(-1, 2), ft)
            at += tab.size
            pred = flip_tta(net, x, clip_lens=cl, tables=tables) if flip else net.forward_ragged(x, cl, tables=tables)
            prov.wild_output_ragged(pred.contiguous().float(), x if gt_2d else None, ft, row0, flags, pix_scale, half_w, half_h, out)


# ---------------------------------------------------------------------------------------------------------------- mesh recovery
_MOVE_MESH = 'the model and the SMPL layer'
FIT_STATUS = {-1: 'has no frames', -2: 'has a reference motion without extent', -3: 'did not converge (mbx_scale_fit iteration cap)'}


def _seq_ptr(lens, dev):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(dev)


def _as_ref(ref_3d, F, dev):
    if not isinstance(ref_3d, torch.Tensor):
        ref_3d = torch.from_numpy(np.ascontiguousarray(ref_3d, dtype=np.float64))
    if ref_3d.dim() != 3 or tuple(ref_3d.shape) != (F, 17, 3):
        raise ValueError(f'expected a reference motion [{F},17,3], got {tuple(ref_3d.shape)}')
    return ref_3d.to(device=dev, dtype=torch.float64).contiguous()


def _fit_rows(fit_host, keys):
    """[(scale, t [3], objective, iterations)] of fit [S,6] on the host; ValueError naming the track on a status"""
    rows = []
    for s, row in enumerate(np.asarray(fit_host, dtype=np.float64).reshape(-1, 6)):
        if not row[5] >= 1:
            raise ValueError(f'solve_scale: track {keys[s] if keys is not None else s!r} {FIT_STATUS.get(int(row[5]) if row[5] == row[5] else 0, "gave no fit")}')
        rows.append((float(row[0]), row[1:4].copy(), float(row[4]), int(row[5])))
    return rows


def _scale_fit(ref, kp, lens, prov):
    fit = torch.empty(len(lens), 6, dtype=torch.float64, device=kp.device)
    with _on(kp.device):
        prov.scale_fit(ref, kp, _seq_ptr(lens, kp.device), fit)
    return fit


def solve_scale(ref_3d, kp_3d, seq_lens=None, ops=None):
    """`solve_scale` of infer_wild_mesh.py:42-56 on the device: the scale and translation that minimise
    mean_i |scale x_i + t - y_i| for x = ref_3d - ref_3d[:, :1] (float64) and y = kp_3d - kp_3d[:, :1] (float32, as numpy forms it),
    by iteratively reweighted least squares in one `mbx_scale_fit` launch (the objective is convex: the reference's 400 starts look
    for an optimum that is unique).  ref_3d [F,17,3] (array or tensor), kp_3d [F,17,3] float32.  Returns `(scale, t [3], objective,
    iterations)`; with `seq_lens` (track lengths summing to F) a list of them, one fit per track.  ValueError naming the track when it
    has no frames, its reference motion has no extent, or the iteration did not converge."""
    if not isinstance(kp_3d, torch.Tensor):
        kp_3d = torch.from_numpy(np.ascontiguousarray(kp_3d, dtype=np.float32))
    if kp_3d.dim() != 3 or tuple(kp_3d.shape[1:]) != (17, 3):
        raise ValueError(f'expected keypoints [F,17,3], got {tuple(kp_3d.shape)}')
    prov, dev = _provider(ops, 'motionbert_amd.wild.solve_scale', kp_3d)
    F = kp_3d.shape[0]
    lens = _check_lens([F] if seq_lens is None else seq_lens, F)
    kp = kp_3d.to(device=dev, dtype=torch.float32).contiguous()
    rows = _fit_rows(_scale_fit(_as_ref(ref_3d, F, dev), kp, lens, prov).cpu().numpy(), None)
    return rows[0] if seq_lens is None else rows


def place(verts, kp_3d, ref_3d, fit, seq_lens=None, ops=None):
    """infer_wild_mesh.py:153-154 in place: verts [F,V,3] float32 (a tensor, modified and returned) = verts - kp_3d[:, :1] + ref_3d[:, :1]
    * scale, in numpy 2's arithmetic (the float32 difference added to the float64 root_cam), rounded to float32 once.  `fit`: what
    `solve_scale` returned (one tuple, or with `seq_lens` the list of them), or the [S,6] float64 tensor of `mbx_scale_fit`."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 3 or verts.shape[2] != 3 or verts.dtype != torch.float32 or not verts.is_contiguous():
        raise ValueError('place needs verts as a contiguous float32 tensor [F,V,3] (it is modified in place)')
    F = verts.shape[0]
    if not isinstance(kp_3d, torch.Tensor):
        kp_3d = torch.from_numpy(np.ascontiguousarray(kp_3d, dtype=np.float32))
    if kp_3d.dim() != 3 or kp_3d.shape[0] != F or kp_3d.shape[2] != 3:
        raise ValueError(f'expected keypoints [{F},K,3], got {tuple(kp_3d.shape)}')
    prov = hip_ops.provider(ops, 'motionbert_amd.wild.place', verts, move='verts')
    dev = verts.device
    lens = _check_lens([F] if seq_lens is None else seq_lens, F)
    if isinstance(fit, torch.Tensor):
        table = fit.to(device=dev, dtype=torch.float64).contiguous()
    else:
        rows = fit if isinstance(fit, list) else [fit]
        table = torch.zeros(len(rows), 6, dtype=torch.float64)
        table[:, 0] = torch.tensor([float(r[0]) for r in rows], dtype=torch.float64)
        table = table.to(dev)
    if tuple(table.shape) != (len(lens), 6):
        raise ValueError(f'{len(lens)} tracks but fits of shape {tuple(table.shape)}')
    if F:
        with _on(dev):
            prov.wild_mesh_place(verts, kp_3d.to(device=dev, dtype=torch.float32).contiguous(), _as_ref(ref_3d, F, dev), _seq_ptr(lens, dev), table)
    return verts


MESH_KEYS = ('verts', 'kp_3d', 'theta')


def infer_mesh(model, smpl, kp_or_tracks, *, clip_len: int = 243, vid_size=None, pixel: bool = False, flip: bool = True, ref_3d=None,
               max_batch: int = 64, want=('verts', 'kp_3d'), to_host: bool = True, ops=None):
    """The loop of infer_wild_mesh.py:99-154.  `model`: a `mesh.MeshRegressor` (bare or DataParallel-wrapped) whose head's `smpl` is an
    `SMPLLayer`; `smpl`: that layer (with `J_regressor_h36m`).  `kp_or_tracks` as `infer` takes it: [F,26,3] detections of one person ->
    a dict `verts` [F,V,3] (millimetres) / `kp_3d` [F,17,3] (/ `theta` [F,82] when `want` names it), or a dict idx -> detections -> a dict
    idx -> such a dict, every person in the same pass.

    Input stage, clip plan and batching are `infer`'s.  Per batch the backbone and `head.forward_params` run on x and (`flip`) on
    `mesh.flip_input(x)`, and ONE `mbx_wild_mesh` launch evaluates SMPL for both parameter sets and writes the mean (lines 115-141) into
    the batch's rows of the stitched results: the vertices of the single passes never exist in memory.  `ref_3d` ([F,17,3], or a dict
    matching the tracks): the reference motion of `--ref_3d_motion_path`; then `solve_scale` (one `mbx_scale_fit` for all tracks) and the
    placement of lines 148-154 (`mbx_wild_mesh_place`) follow on the device, and the result gains `scale`.  `to_host=False` returns device
    tensors (the vertices of a long video are hundreds of MB).  Host reads: the results at the end, and the fits when `ref_3d` is given."""
    from .mesh import flip_input
    from .smpl import SMPLLayer
    net = model.module if hasattr(model, 'module') else model
    head = getattr(net, 'head', None)
    if head is None or not hasattr(head, 'forward_params') or not hasattr(net, 'backbone'):
        raise TypeError('infer_mesh needs a mesh.MeshRegressor (a backbone and a head with forward_params)')
    if not isinstance(smpl, SMPLLayer) or not isinstance(head.smpl, SMPLLayer):
        raise TypeError('infer_mesh needs an SMPLLayer, as `smpl` and in the head; mesh.flip_average is the route for other layers')
    Q = smpl.J_regressor_h36m
    if Q is None:
        raise ValueError('infer_mesh needs the layer\'s J_regressor_h36m (it has none)')
    want = tuple(want)
    if not want or any(k not in MESH_KEYS for k in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a non-empty subset of {MESH_KEYS}, got {want}')
    clip_len, max_batch = int(clip_len), int(max_batch)
    if clip_len < 1 or max_batch < 1:
        raise ValueError(f'clip_len and max_batch must be >= 1, got {clip_len} and {max_batch}')
    maxlen = getattr(net.backbone, 'maxlen', getattr(net, 'maxlen', None))
    if maxlen is not None and clip_len > maxlen:
        raise ValueError(f'clip_len {clip_len} is longer than the model takes (maxlen = {maxlen})')
    if pixel and not vid_size:
        raise ValueError('pixel=True needs vid_size=(w, h)')
    kp, lens, keys = _tracks(kp_or_tracks)
    if ref_3d is not None and (keys is not None) != isinstance(ref_3d, dict):
        raise ValueError('ref_3d must be a dict matching the tracks where the detections are one, an array otherwise')
    if isinstance(ref_3d, dict):
        if list(ref_3d) != keys:
            raise ValueError(f'ref_3d has the tracks {list(ref_3d)}, the detections {keys}')
        for k, n in zip(keys, lens):
            if tuple(ref_3d[k].shape) != (n, 17, 3):
                raise ValueError(f'track {k!r}: expected a reference motion [{n},17,3], got {tuple(ref_3d[k].shape)}')
        ref_3d = np.concatenate([np.asarray(ref_3d[k].cpu() if isinstance(ref_3d[k], torch.Tensor) else ref_3d[k], dtype=np.float64) for k in keys])
    if ops is None and not isinstance(kp, torch.Tensor):
        dev = hip_ops.model_device(net, 'motionbert_amd.wild.infer_mesh')
        kp = torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float64)).to(dev)             # the one upload
    y = wild_input(kp, vid_size=vid_size if pixel else None, scale_range=None if pixel else [1, 1], seq_lens=lens, ops=ops)     # :99-104
    F, dev = y.shape[0], y.device
    lens = [F] if lens is None else lens
    ref = None if ref_3d is None else _as_ref(ref_3d, F, dev)
    prov = hip_ops.provider(ops, 'motionbert_amd.wild.infer_mesh', y, smpl.v_template, move=_MOVE_MESH)
    if Q.device != dev or Q.dtype != torch.float32 or not Q.is_contiguous():
        Q = Q.to(device=dev, dtype=torch.float32).contiguous()
    K, V = Q.shape[0], smpl.num_vertices
    verts = torch.empty(F, V, 3, dtype=torch.float32, device=dev) if 'verts' in want else None
    kp3d = torch.empty(F, K, 3, dtype=torch.float32, device=dev) if ('kp_3d' in want or ref is not None) else None
    theta = torch.empty(F, 82, dtype=torch.float32, device=dev) if 'theta' in want else None
    plan = clip_plan(lens, clip_len)
    offsets = [o for _, offs in plan for o in offs]
    table = torch.tensor(offsets, dtype=torch.int32).to(dev) if offsets else None              # every batch's destinations, one upload
    if hasattr(model, 'eval'):
        model.eval()
    tensors = smpl.model_tensors()

    def params(x):
        n, T = x.shape[:2]
        rot, shape, th = head.forward_params(net.backbone.get_representation(x).reshape([n, T, 17, -1]))
        return rot.float().contiguous(), shape.float().contiguous(), th.float().contiguous()

    at = 0
    with torch.no_grad(), _on(dev):
        for T, part in _batches(plan, max_batch):
            n = len(part)
            x = _clips(y, part, T)
            rot_a, shape_a, theta_a = params(x)                                                # :115
            theta_b = params(flip_input(x))[2] if flip else None                               # :116-117
            prov.wild_mesh(tensors, Q, rot_a, shape_a, theta_a if theta is not None else None, theta_b, 1000.0, table[at:at + n], max(part), T,
                           verts, kp3d, theta)                                                 # :118-141, stitched
            at += n
    out = {'verts': verts, 'kp_3d': kp3d if 'kp_3d' in want else None, 'theta': theta}
    fits = None
    if ref is not None:                                                                        # :148-154
        fit = _scale_fit(ref, kp3d, lens, prov)
        if verts is not None and F:
            with _on(dev):
                prov.wild_mesh_place(verts, kp3d, ref, _seq_ptr(lens, dev), fit)
        fits = _fit_rows(fit.cpu().numpy(), keys)
    out = {k: (v.cpu().numpy() if to_host else v) for k, v in out.items() if v is not None}
    if keys is None:
        if fits is not None:
            out['scale'] = fits[0][0]
        return out
    res, end = OrderedDict(), 0
    for i, (k, n) in enumerate(zip(keys, lens)):
        res[k] = {name: v[end:end + n] for name, v in out.items()}
        if fits is not None:
            res[k]['scale'] = fits[i][0]
        end += n
    return res

