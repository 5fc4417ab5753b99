"""An input pipeline that can feed the GPU (reference `lib/data/dataset_motion_3d.py:33-67`,
`train.py:219-240`, on-disk format of `tools/convert_h36m.py`: one `%08d.pkl` = {"data_input", "data_label"} per clip).

The reference unpickles one ~99 KB file per clip per access from 12 DataLoader workers, augments per clip in numpy and
collates on the host.  At 8 x 1,000 clips/s that is ~0.8 GB/s of pickle parsing.  Here:

  pack_motion3d()      one-off: the per-clip pickles of a (data_root, subsets, split) become two dense arrays
                       `<prefix>.input.npy` / `<prefix>.label.npy` [N, T, 17, 3] float32 (plain .npy: np.load(mmap_mode='r')).
  PackedMotion3D       memory-maps them.  A batch is one `np.take` of B rows (contiguous 49.6 KB each) straight into a slot
                       of a pinned ring buffer, filled by ONE background thread, copied to the device on a side stream while the
                       previous batch trains; nothing is parsed, nothing is collated.
  on the device        everything `MotionDataset3D.__getitem__` did per clip on the host: random flip of input and label
                       (`flip_data`, utils_data.py:54-66), the synthetic / gt_2d input (`x, y` of the label + confidence 1,
                       dataset_motion_3d.py:49-53), `crop_scale_3d` (utils_data.py:31-52) -- batched torch ops.
  pack_action / PackedAction, pack_mesh / PackedMesh   the same scheme for the NTU annotation file (lib/data/dataset_action.py) and for the
                       mesh detection files (lib/data/dataset_mesh.py); their `__getitem__` stages are HIP kernels (`mbx_action_input`,
                       `mbx_mesh_gt`: the SMPL ground truth is computed on the device, nothing of vertex size crosses the host link).
  pack_posetrack / pack_instav / PackedMotion2D   the same scheme for the two 2D sets of pre-training (lib/data/dataset_motion_2d.py); their
                       `__getitem__` stage and the 2D front end of the training step are one launch of `mbx_motion2d_input`.
  sharding             `rank` / `world`: every rank walks the same per-epoch permutation and takes a strided, equally sized
                       share (what DistributedSampler does), so the N ranks of the data-parallel run never exchange data.
"""
from __future__ import annotations

import json
import os
import pickle
import queue
import threading
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from .augment import FLIP_PERM


def pack_motion3d(data_root: str, subset_list: Sequence[str], data_split: str, out_prefix: str) -> dict:
    """Convert the reference's per-clip pickle tree `<data_root>/<subset>/<split>/*.pkl` (file order = the reference's
    `sorted(os.listdir(...))`, dataset_motion_3d.py:19-25) into two dense .npy arrays.  Returns the metadata dict."""
    files = []
    for subset in subset_list:
        d = os.path.join(data_root, subset, data_split)
        files += [os.path.join(d, f) for f in sorted(os.listdir(d))]
    if not files:
        raise ValueError(f'no clips under {data_root} {list(subset_list)} {data_split}')
    with open(files[0], 'rb') as f:
        first = pickle.load(f)
    shape = tuple(np.asarray(first['data_label']).shape)
    has_input = first['data_input'] is not None
    lab = np.lib.format.open_memmap(out_prefix + '.label.npy', mode='w+', dtype=np.float32, shape=(len(files),) + shape)
    inp = np.lib.format.open_memmap(out_prefix + '.input.npy', mode='w+', dtype=np.float32, shape=(len(files),) + shape) if has_input else None
    for i, path in enumerate(files):
        with open(path, 'rb') as f:
            m = pickle.load(f)
        lab[i] = np.asarray(m['data_label'], dtype=np.float32)
        if has_input:
            if m['data_input'] is None:
                raise ValueError(f'{path}: data_input missing (the first clip had one)')
            inp[i] = np.asarray(m['data_input'], dtype=np.float32)
    lab.flush()
    if inp is not None:
        inp.flush()
    meta = dict(n=len(files), clip_shape=list(shape), has_input=bool(has_input), split=data_split, subsets=list(subset_list))
    with open(out_prefix + '.json', 'w') as f:
        json.dump(meta, f)
    return meta


def flip_batch(x: torch.Tensor, which: torch.Tensor) -> torch.Tensor:
    """`flip_data` (utils_data.py:54-66) applied to the clips of the batch where `which` [B] is True."""
    perm = torch.as_tensor(FLIP_PERM, device=x.device)
    f = x.index_select(-2, perm).clone()
    f[..., 0] = -f[..., 0]
    return torch.where(which.view(-1, *([1] * (x.dim() - 1))), f, x)


def crop_scale_3d_batch(motion: torch.Tensor, ratio: torch.Tensor) -> torch.Tensor:
    """`crop_scale_3d` (utils_data.py:31-52) for a batch [B,T,17,3] with one random `ratio` [B] per clip."""
    lo = motion[..., :2].amin(dim=(1, 2))            # [B,2]: xmin, ymin
    hi = motion[..., :2].amax(dim=(1, 2))
    scale = (hi - lo).amax(dim=1) / ratio             # max(xmax-xmin, ymax-ymin) / ratio
    ok = scale != 0
    s = torch.where(ok, scale, torch.ones_like(scale)).view(-1, 1, 1)
    xs = ((lo + hi) - scale.view(-1, 1)) / 2          # [B,2]
    out = motion.clone()
    out[..., :2] = (motion[..., :2] - xs.view(-1, 1, 1, 2)) / s.unsqueeze(-1)
    out[..., 2] = (motion[..., 2] - motion[:, 0:1, 0:1, 2]) / s      # z relative to the first frame's root (:38), same scale
    out = (out - 0.5) * 2
    return torch.where(ok.view(-1, 1, 1, 1), out, torch.zeros_like(out))


def shard_indices(n: int, shuffle: bool, epoch: int, seed: int, rank: int, world: int) -> np.ndarray:
    """The clips of rank `rank` in epoch `epoch`: every rank walks the same permutation and takes a strided share, padded by
    wrap-around to ceil(n / world) clips (what DistributedSampler does).  EQUAL shares are what keeps data-parallel ranks in
    lock-step when the loaders of a pre-training epoch have different lengths (train.py:325-330; `pretrain_epoch_plan`): every
    rank issues the same number of steps per loader, so the gradient all-reduces pair up."""
    order = np.random.default_rng([seed, epoch]).permutation(n) if shuffle else np.arange(n)
    per = -(-n // world)
    return np.resize(order, per * world)[rank::world]


def pinned_batches(arrays, chunks, batch_size: int, device, ring: int = 3):
    """The asynchronous batch stream under `PackedMotion3D.batches` and `PackedAction.batches`: for every index array of `chunks` a tuple
    with one DEVICE tensor per array of `arrays` (numpy arrays or memory maps with the same first dimension; any dtype), holding the
    chunk's rows in ascending index order.  ONE background thread gathers the rows (`np.take`) into a ring of pinned slots, the copy to
    the device runs on a side stream while the previous batch is in use, and the loader thread and the slots are released when the
    generator is closed, exhausted or abandoned.  On a host `device` the tensors are clones of the slots."""
    device = torch.device(device)
    cuda = device.type == 'cuda'
    ring = max(2, int(ring))
    slots = [tuple(torch.empty((batch_size,) + tuple(a.shape[1:]), dtype=torch.from_numpy(np.empty(0, dtype=a.dtype)).dtype, pin_memory=cuda)
                   for a in arrays) for _ in range(ring)]
    free, ready = queue.Queue(), queue.Queue(maxsize=ring)
    for s in range(ring):
        free.put(s)

    stop = threading.Event()

    def producer():                                   # ONE host thread: row gather from the page cache into pinned memory
        try:
            for ch in chunks:
                s = free.get()
                if s is None or stop.is_set():        # the consumer went away (break / exception): see the finally below
                    return
                srt = np.sort(ch)                     # ascending file offsets; the batch is a set, order inside it is irrelevant
                for a, slot in zip(arrays, slots[s]):
                    np.take(a, srt, axis=0, out=slot.numpy()[:len(ch)])
                ready.put((s, len(ch)))
            ready.put(None)
        except Exception as e:                        # surface loader errors in the consumer
            ready.put(e)
    th = threading.Thread(target=producer, daemon=True)
    th.start()
    copy_stream = torch.cuda.Stream(device) if cuda else None
    pending = None                                    # (slot, device tensors, event) of the batch in flight
    try:
        while True:
            item = ready.get()
            if isinstance(item, Exception):
                raise item
            nxt = None
            if item is not None:
                s, nb = item
                if cuda:
                    with torch.cuda.stream(copy_stream):
                        dev = tuple(t[:nb].to(device, non_blocking=True) for t in slots[s])
                        ev = torch.cuda.Event()
                        ev.record(copy_stream)
                else:
                    dev, ev = tuple(t[:nb].clone() for t in slots[s]), None
                nxt = (s, dev, ev)
            if pending is not None:
                s0, dev0, ev0 = pending
                if ev0 is not None:
                    torch.cuda.current_stream(device).wait_event(ev0)      # the copy finished before compute touches it ...
                    ev0.synchronize()                                       # ... and before the host refills the pinned slot
                    for t in dev0:
                        t.record_stream(torch.cuda.current_stream(device))
                free.put(s0)
                pending = nxt
                yield dev0
            else:
                pending = nxt
            if item is None:
                break
    finally:
        # also reached when the consumer abandons the generator (break, exception in the training loop, GeneratorExit):
        # release the loader thread -- it may sit in free.get() or in ready.put() on a full queue -- and the pinned slots
        stop.set()
        free.put(None)
        while th.is_alive():
            try:
                ready.get(timeout=0.05)
            except queue.Empty:
                pass
        th.join()
        if pending is not None and pending[2] is not None:
            pending[2].synchronize()                   # an H2D copy still reading a pinned slot must finish before it is freed


class PackedMotion3D:
    """Memory-mapped packed clips + an asynchronous batch stream.

        ds = PackedMotion3D(prefix, device='cuda', flip=True, synthetic=False, gt_2d=False, scale_range=None)
        for x2d, gt3d in ds.batches(64, shuffle=True, epoch=e, rank=r, world=w):   # device tensors [B,T,17,3]
            ...
    `data_split` semantics follow MotionDataset3D.__getitem__ (dataset_motion_3d.py:42-67): with train=True the input is the
    stored 2D detection with a random flip of input AND label (or, synthetic / gt_2d, the augmented label's x, y + confidence
    1); with train=False the stored input (gt_2d: the label's x, y + confidence 1), no augmentation."""

    def __init__(self, prefix: str, device='cuda', train: bool = True, flip: bool = True, synthetic: bool = False, gt_2d: bool = False,
                 scale_range: Optional[Tuple[float, float]] = None, ring: int = 3):
        with open(prefix + '.json') as f:
            self.meta = json.load(f)
        self.label = np.load(prefix + '.label.npy', mmap_mode='r')
        self.input = np.load(prefix + '.input.npy', mmap_mode='r') if self.meta['has_input'] else None
        self.device = torch.device(device)
        self.train, self.flip, self.synthetic, self.gt_2d, self.scale_range = train, flip, synthetic, gt_2d, scale_range
        self.ring = max(2, int(ring))
        if self.input is None and not (synthetic or gt_2d):
            raise ValueError('Training illegal.')       # dataset_motion_3d.py:59 (no 2D detections and not synthetic / gt_2d)

    def __len__(self):
        return int(self.meta['n'])

    def epoch_indices(self, shuffle: bool, epoch: int, seed: int, rank: int, world: int) -> np.ndarray:
        return shard_indices(len(self), shuffle, epoch, seed, rank, world)

    def _device_stage(self, inp, lab, gen):
        """What MotionDataset3D.__getitem__ did per clip on the host, batched on the device."""
        B = lab.shape[0]
        if not self.train:
            if self.gt_2d:
                inp = torch.cat([lab[..., :2], torch.ones_like(lab[..., :1])], -1)
            return inp, lab
        if self.synthetic or self.gt_2d:
            if self.scale_range is not None:             # Augmenter3D.augment3D (augmentation.py:93-98)
                lo, hi = self.scale_range
                ratio = torch.rand(B, generator=gen, device=lab.device) * (hi - lo) + lo
                lab = crop_scale_3d_batch(lab, ratio)
            if self.flip:
                lab = flip_batch(lab, torch.rand(B, generator=gen, device=lab.device) > 0.5)
            inp = torch.cat([lab[..., :2], torch.ones_like(lab[..., :1])], -1)       # GT x, y and c = 1 (:51-53)
            return inp, lab
        if self.flip:
            which = torch.rand(B, generator=gen, device=lab.device) > 0.5                  # :56-58: input and label together
            inp, lab = flip_batch(inp, which), flip_batch(lab, which)
        return inp, lab

    def batches(self, batch_size: int, shuffle: bool = True, epoch: int = 0, seed: int = 0, rank: int = 0, world: int = 1,
                drop_last: bool = False) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        idx = self.epoch_indices(shuffle, epoch, seed, rank, world)
        chunks = [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]
        if drop_last and chunks and len(chunks[-1]) < batch_size:
            chunks.pop()
        if not chunks:
            return
        need_inp = self.input is not None and not (self.synthetic or self.gt_2d)     # otherwise the input is derived from the label
        gen = torch.Generator(device=self.device)
        gen.manual_seed((seed * 1000003 + epoch) * 8191 + rank)
        stream = pinned_batches([self.label, self.input] if need_inp else [self.label], chunks, batch_size, self.device, self.ring)
        try:
            for got in stream:
                yield self._device_stage(got[1] if need_inp else None, got[0], gen)
        finally:
            stream.close()                                # the consumer went away: release the loader thread and the pinned slots now


# ---------------------------------------------------------------------------------------------------------------
# action recognition (lib/data/dataset_action.py): the NTU annotation file, packed once
# ---------------------------------------------------------------------------------------------------------------
#: coco2h36m (dataset_action.py:31-74): H36M joint <- one COCO joint, or the mean of two; joint 7 (belly) is the mean of H36M 0 and 8
_COCO_SINGLE = {1: 12, 2: 14, 3: 16, 4: 11, 5: 13, 6: 15, 9: 0, 11: 5, 12: 7, 13: 9, 14: 6, 15: 8, 16: 10}
_COCO_PAIR = {0: (11, 12), 8: (5, 6), 10: (1, 2)}


def _ntu_camera(x, img_shape):
    """make_cam (dataset_action.py:19-29): pixels -> [-1, 1] along the longer image side"""
    h, w = img_shape
    return x / (w if w >= h else h) * 2 - 1


def _ntu_track(x):
    """human_tracking (dataset_action.py:114-128): the two detections of a frame swap names whenever person 0 of the previous frame is
    nearer to person 1 of this one (summed joint distances); x [M,T,V,C]"""
    if x.shape[0] == 1:
        return x
    keep = np.sum(np.linalg.norm(x[0, 1:] - x[0, :-1], axis=-1), axis=-1)
    swap = np.sum(np.linalg.norm(x[0, 1:] - x[1, :-1], axis=-1), axis=-1)
    sel = (np.cumsum(keep > swap) % 2)[:, None, None]
    out = np.zeros(x.shape)
    out[:, 0] = x[:, 0]
    out[0, 1:] = x[1, 1:] * sel + x[0, 1:] * (1 - sel)
    out[1, 1:] = x[0, 1:] * sel + x[1, 1:] * (1 - sel)
    return out


def _ntu_to_h36m(x):
    """coco2h36m (dataset_action.py:31-74) for x [M,T,17,C]"""
    y = np.zeros(x.shape)
    for j, c in _COCO_SINGLE.items():
        y[:, :, j] = x[:, :, c]
    for j, (a, b) in _COCO_PAIR.items():
        y[:, :, j] = (x[:, :, a] + x[:, :, b]) * 0.5
    y[:, :, 7] = (y[:, :, 0] + y[:, :, 8]) * 0.5
    return y


def _ntu_frames(ori_len: int, target_len: int, rng) -> np.ndarray:
    """resample (utils_data.py:68-89, replay=False): `target_len` frame indices spread over the clip; with `rng` (a training split) each
    one is jittered inside its interval -- or, for a clip shorter than the target, rounded down or up at random."""
    if rng is None:
        return np.linspace(0, ori_len, num=target_len, endpoint=False, dtype=int)
    even = np.linspace(0, ori_len, num=target_len, endpoint=False)
    if ori_len < target_len:
        sel = rng.randint(2, size=even.shape)
        ids = np.sort(sel * np.floor(even) + (1 - sel) * np.ceil(even))
    else:
        ids = rng.random_sample(even.shape) * (even[1] - even[0]) + even
    return np.clip(ids, a_min=0, a_max=ori_len - 1).astype(np.uint32)


def pack_action(pkl_path: str, data_split: str, n_frames: int, out_prefix: str, check_split: bool = True) -> dict:
    """The one-off host work of `ActionDataset.__init__` (dataset_action.py:130-160) for the annotation pickle of NTU RGB+D
    ({'split': {name: [frame_dir]}, 'annotations': [{'frame_dir', 'label', 'total_frames', 'img_shape', 'keypoint' [M,T0,17,2],
    'keypoint_score' [M,T0,17]}]}): camera normalisation, tracking, COCO -> H36M joints, resampling to `n_frames`, and an all-zero second
    person for single-person samples.  Writes `<prefix>.motion.npy` [N,2,n_frames,17,3] float32, `<prefix>.label.npy` [N] int64 and
    `<prefix>.json`; returns the metadata.

    A split whose name contains 'train' (or any, with check_split=False), and not 'oneshot', is resampled with random numbers: they
    come from `np.random.RandomState(0)` in sample order, which is what the reference's `np.random.seed(0)` amounts to, so the array
    equals the reference's `dataset.motions` bit for bit."""
    with open(pkl_path, 'rb') as f:
        dataset = pickle.load(f)
    members = None
    if check_split:
        if data_split not in dataset['split']:
            raise ValueError(f'{pkl_path} has no split {data_split!r} (it has {sorted(dataset["split"])})')
        members = set(dataset['split'][data_split])
    is_train = ('train' in data_split or not check_split) and 'oneshot' not in data_split
    rng = np.random.RandomState(0) if is_train else None
    motions, labels = [], []
    for sample in dataset['annotations']:
        if members is not None and sample['frame_dir'] not in members:
            continue
        ids = _ntu_frames(sample['total_frames'], n_frames, rng)
        cam = _ntu_to_h36m(_ntu_track(_ntu_camera(sample['keypoint'], sample['img_shape'])))
        motion = np.concatenate((cam[:, ids], sample['keypoint_score'][..., None][:, ids]), axis=-1)
        if motion.shape[0] == 1:
            motion = np.concatenate((motion, np.zeros(motion.shape)), axis=0)
        if motion.shape[0] != 2:
            raise ValueError(f'{sample["frame_dir"]}: {motion.shape[0]} persons (the reference stacks samples of exactly two)')
        motions.append(motion.astype(np.float32))
        labels.append(int(sample['label']))
    if not motions:
        raise ValueError(f'{pkl_path}: split {data_split!r} is empty')
    np.save(out_prefix + '.motion.npy', np.stack(motions))
    np.save(out_prefix + '.label.npy', np.asarray(labels, dtype=np.int64))
    meta = dict(n=len(motions), clip_shape=[2, int(n_frames), 17, 3], split=data_split, train=bool(is_train))
    with open(out_prefix + '.json', 'w') as f:
        json.dump(meta, f)
    return meta


class PackedAction:
    """The packed NTU clips of `pack_action` + the asynchronous batch stream of `pinned_batches` + `NTURGBD.__getitem__` on the device.

        ds = PackedAction(prefix, device='cuda', train=True, random_move=True, scale_range=(1, 1))
        for batch, labels in ds.batches(32, shuffle=True, epoch=e, rank=r, world=w):    # [B,2,T,17,3] f32, [B] int64, on the device
            ...
    Every batch has been through `augment.action_input` (`mbx_action_input`: random_move + crop_scale in one launch) with a seed derived
    from (seed, epoch, rank, batch index): an epoch is reproducible, and no two batches of a run share their draws.  `random_move` and
    `scale_range` are the reference's arguments (dataset_action.py:170-182; `scale_range=None` skips crop_scale); `train=False` is the
    validation loader of train_action.py:133 (`random_move=False`).  `ops`: kernel provider for host tensors (tests)."""

    def __init__(self, prefix: str, device='cuda', train: bool = True, random_move: bool = True, scale_range: Optional[Tuple[float, float]] = (1, 1),
                 ring: int = 3, ops=None):
        with open(prefix + '.json') as f:
            self.meta = json.load(f)
        self.motion = np.load(prefix + '.motion.npy', mmap_mode='r')
        self.label = np.load(prefix + '.label.npy')
        if len(self.motion) != len(self.label):
            raise ValueError(f'{prefix}: {len(self.motion)} clips but {len(self.label)} labels')
        self.device = torch.device(device)
        self.train, self.random_move, self.scale_range = bool(train), bool(random_move) and bool(train), scale_range
        self.ring, self.ops = max(2, int(ring)), ops

    def __len__(self):
        return len(self.label)

    @staticmethod
    def batch_seed(seed: int, epoch: int, rank: int, batch: int) -> int:
        return (((seed * 1000003 + epoch) * 8191 + rank) * 65537 + batch) % (1 << 63)

    def batches(self, batch_size: int, shuffle: bool = True, epoch: int = 0, seed: int = 0, rank: int = 0, world: int = 1,
                drop_last: bool = False) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        from .augment import action_input
        idx = shard_indices(len(self), shuffle, epoch, seed, rank, world)
        chunks = [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]
        if drop_last and chunks and len(chunks[-1]) < batch_size:
            chunks.pop()
        if not chunks:
            return
        stream = pinned_batches([self.motion, self.label], chunks, batch_size, self.device, self.ring)
        try:
            for k, (motion, labels) in enumerate(stream):
                if self.random_move or self.scale_range:
                    motion = action_input(motion, random_move=self.random_move, scale_range=self.scale_range,
                                          seed=self.batch_seed(seed, epoch, rank, k), ops=self.ops)
                yield motion, labels
        finally:
            stream.close()


# ---------------------------------------------------------------------------------------------------------------
# mesh recovery (lib/data/dataset_mesh.py): the detection pickles of H36M / 3DPW / COCO, packed once
# ---------------------------------------------------------------------------------------------------------------
#: DataReaderH36M.read_2d (datareader_h36m.py:29-44): camera name -> (res_w, res_h)
_H36M_RES = {'54138969': (1000, 1002), '60457274': (1000, 1002), '55011271': (1000, 1000), '58860488': (1000, 1000)}
_MESH_RES = {'coco': (640, 640), 'pw3d': (1920, 1920)}      # dataset_mesh.py:28,30


def _split_clips(vid_list, n_frames: int, data_stride: int, rng) -> list:
    """split_clips (utils_data.py:91-112): windows of `n_frames` every `data_stride` frames inside one source; a source that is over
    before it filled a window is resampled to `n_frames` (`resample` with its random rounding, here from `rng`), the last source excepted"""
    result, saved, st, i = [], set(), 0, 0
    while i < len(vid_list):
        i += 1
        if i - st == n_frames:
            result.append(np.arange(st, i))
            saved.add(vid_list[i - 1])
            st += data_stride
        if i == len(vid_list):
            break
        if vid_list[i] != vid_list[i - 1]:
            if vid_list[i - 1] not in saved:
                result.append(_ntu_frames(i - st, n_frames, rng).astype(np.int64) + st)
                saved.add(vid_list[i - 1])
            st = i
    return result


def _mesh_read_2d(part: dict, dataset: str, has_confidence: bool) -> np.ndarray:
    """read_2d of DataReaderH36M (datareader_h36m.py:25-58) / DataReaderMesh (datareader_mesh.py:19-40) for one split: [frames,17,3] with
    the reference's roundings (the division and the factor 2 in float32, the offset subtracted in float64)"""
    xy = np.asarray(part['joint_2d'])[:, :, :2].astype(np.float32)
    if dataset == 'h36m':
        names = list(part['camera_name'])
        bad = [i for i, c in enumerate(names) if c not in _H36M_RES]
        if bad:
            raise ValueError(f'{bad[0]} data item has an invalid camera name')
        if len(names) != len(xy):
            raise ValueError(f'{len(names)} camera names for {len(xy)} frames')
        res = np.asarray([_H36M_RES[c] for c in names], dtype=np.float64).reshape(-1, 2)
        off = np.stack([np.ones(len(names)), res[:, 1] / res[:, 0]], axis=1)[:, None, :]
        xy = ((xy / 1000 * 2).astype(np.float64) - off).astype(np.float32)          # res_w is 1000 for every camera
    else:
        res_w, res_h = _MESH_RES[dataset]
        xy = xy / res_w * 2 - np.asarray([1, res_h / res_w])
    if has_confidence:
        conf = np.asarray(part['confidence']).astype(np.float32)
        if conf.ndim == 2:
            conf = conf[:, :, None]
    else:
        conf = np.ones(xy.shape)[:, :, 0:1]
    return np.concatenate((xy, conf), axis=2)


def pack_mesh(pkl_path: str, dataset: str, data_split: str, clip_len: int, data_stride: int, out_prefix: str, sample_stride: int = 1) -> dict:
    """The one-off host work of `SMPLDataset.__init__` (dataset_mesh.py:19-49) for the detection pickle of `dataset` in {'h36m', 'pw3d',
    'coco'} ({'train' / 'test': {'joint_2d' [frames,17,>=2], 'confidence', 'source', 'smpl_pose' [frames,72], 'smpl_shape' [frames,10]} and,
    for h36m, 'camera_name'}): `read_2d` of the data set's reader with its resolution, `split_clips` with the `n_frames` and strides of
    dataset_mesh.py:25-30 (coco: single frames; the test split: stride = clip_len), and the SMPL parameters of every clip.  Writes
    `<prefix>.motion2d.npy` [N,T,17,3], `<prefix>.pose.npy` [N,T,72], `<prefix>.shape.npy` [N,T,10] (float32) and `<prefix>.json`; returns
    the metadata.  The arrays equal the reference's `motion_2d` / `motion_smpl_3d` bit for bit (the clip of the confidence and the flip
    belong to `__getitem__`: `mesh.mesh_targets`): the random rounding of a short source's resampling comes from
    `np.random.RandomState(0)`, drawn for the train split first, which is what the reference's `np.random.seed(0)` amounts to.

    `sample_stride` other than 1 raises: the reference's camera loop indexes the unstrided list, and no config uses it."""
    if dataset not in ('h36m', 'pw3d', 'coco'):
        raise ValueError('Mesh dataset undefined.')                 # dataset_mesh.py:32
    if data_split not in ('train', 'test'):
        raise ValueError(f"data_split must be 'train' or 'test', got {data_split!r}")
    if sample_stride != 1:
        raise ValueError(f'sample_stride = {sample_stride}: only 1 is supported (the reference reads camera names unstrided)')
    with open(pkl_path, 'rb') as f:
        dt = pickle.load(f)
    n_frames = 1 if dataset == 'coco' else int(clip_len)
    strides = {'train': 1 if dataset == 'coco' else int(data_stride), 'test': 1 if dataset == 'coco' else int(clip_len)}
    rng = np.random.RandomState(0)
    ids = {split: _split_clips(dt[split]['source'], n_frames, strides[split], rng) for split in ('train', 'test')}[data_split]
    if not ids:
        raise ValueError(f'{pkl_path}: split {data_split!r} has no clip of {n_frames} frames')
    ids = np.stack(ids)
    part = dt[data_split]
    motion = _mesh_read_2d(part, dataset, dataset != 'h36m' or 'confidence' in dt['train'])[ids].astype(np.float32)
    pose = np.asarray(part['smpl_pose'])[ids].astype(np.float32)
    shape = np.asarray(part['smpl_shape'])[ids].astype(np.float32)
    if pose.shape != ids.shape + (72,) or shape.shape != ids.shape + (10,):
        raise ValueError(f'{pkl_path}: smpl_pose [frames,72] and smpl_shape [frames,10] expected, clips are {pose.shape} / {shape.shape}')
    np.save(out_prefix + '.motion2d.npy', motion)
    np.save(out_prefix + '.pose.npy', pose)
    np.save(out_prefix + '.shape.npy', shape)
    meta = dict(n=int(len(ids)), clip_len=int(n_frames), dataset=dataset, split=data_split, data_stride=int(strides[data_split]))
    with open(out_prefix + '.json', 'w') as f:
        json.dump(meta, f)
    return meta


class PackedMesh:
    """The packed clips of `pack_mesh` + the asynchronous batch stream of `pinned_batches` + `MotionSMPL.__getitem__` on the device.

        ds = PackedMesh(prefix, smpl, device='cuda', train=True, flip=True)          # smpl: an SMPLLayer on the device
        for batch_input, batch_gt in ds.batches(128, shuffle=True, epoch=e, rank=r, world=w):
            ...          # [B,T,17,3] and {'theta' [B,T,82], 'kp_3d' [B,T,17,3], 'verts' [B,T,V,3]} on the device: MeshStep / MeshEvaluator take them
    About 1 MB per batch crosses the host link (2D input, pose, shape); every batch goes through `mesh.mesh_targets` (`mbx_mesh_gt`: clip
    flip, SMPL, H36M joints, root subtraction) with a seed derived from (seed, epoch, rank, batch index) as `PackedAction` derives it.
    `train=False` (the test split) never flips.  `ops`: kernel provider for host tensors (tests)."""

    def __init__(self, prefix: str, smpl, device='cuda', train: bool = True, flip: bool = True, ring: int = 3, ops=None):
        with open(prefix + '.json') as f:
            self.meta = json.load(f)
        self.motion_2d = np.load(prefix + '.motion2d.npy', mmap_mode='r')
        self.pose = np.load(prefix + '.pose.npy', mmap_mode='r')
        self.shape = np.load(prefix + '.shape.npy', mmap_mode='r')
        if not len(self.motion_2d) == len(self.pose) == len(self.shape):
            raise ValueError(f'{prefix}: {len(self.motion_2d)} / {len(self.pose)} / {len(self.shape)} clips in the three arrays')
        self.smpl = smpl
        self.device = torch.device(device)
        self.train, self.flip = bool(train), bool(flip) and bool(train)
        self.ring, self.ops = max(2, int(ring)), ops

    def __len__(self):
        return len(self.pose)

    def batches(self, batch_size: int, shuffle: bool = True, epoch: int = 0, seed: int = 0, rank: int = 0, world: int = 1,
                drop_last: bool = False) -> Iterator[Tuple[torch.Tensor, dict]]:
        from .mesh import mesh_targets
        idx = shard_indices(len(self), shuffle, epoch, seed, rank, world)
        chunks = [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]
        if drop_last and chunks and len(chunks[-1]) < batch_size:
            chunks.pop()
        if not chunks:
            return
        stream = pinned_batches([self.motion_2d, self.pose, self.shape], chunks, batch_size, self.device, self.ring)
        try:
            for k, (motion_2d, pose, shape) in enumerate(stream):
                yield mesh_targets(self.smpl, pose, shape, motion_2d, flip=self.flip, seed=PackedAction.batch_seed(seed, epoch, rank, k),
                                   ops=self.ops)
        finally:
            stream.close()


# ---------------------------------------------------------------------------------------------------------------
# the 2D half of pre-training (lib/data/dataset_motion_2d.py): PoseTrack and InstaVariety, packed once
# ---------------------------------------------------------------------------------------------------------------
#: posetrack2h36m (dataset_motion_2d.py:14-74): H36M joint <- one PoseTrack joint; the root is the mean of the hips, the belly the mean of
#: root and neck, and their confidences the minimum of the two
_POSETRACK_SINGLE = {1: 12, 2: 14, 3: 16, 4: 11, 5: 13, 6: 15, 8: 1, 9: 0, 10: 2, 11: 5, 12: 7, 13: 9, 14: 6, 15: 8, 16: 10}


def _posetrack_to_h36m(x):
    """posetrack2h36m (dataset_motion_2d.py:54-74) for x [T,17,C]"""
    y = np.zeros(x.shape)
    for j, c in _POSETRACK_SINGLE.items():
        y[:, j] = x[:, c]
    y[:, 0] = (x[:, 11] + x[:, 12]) * 0.5
    y[:, 7] = (y[:, 0] + y[:, 8]) * 0.5
    y[:, 0, 2] = np.minimum(x[:, 11, 2], x[:, 12, 2])
    y[:, 7, 2] = np.minimum(y[:, 0, 2], y[:, 8, 2])
    return y


def _crop_scale_host(motion, scale_range, rng):
    """crop_scale (utils_data.py:7-29) for one clip in numpy's own arithmetic, the ratio from `rng` -- drawn, as there, only once four valid
    joints were found"""
    valid = motion[motion[..., 2] != 0][:, :2]
    if len(valid) < 4:
        return np.zeros(motion.shape)
    xmin, xmax, ymin, ymax = min(valid[:, 0]), max(valid[:, 0]), min(valid[:, 1]), max(valid[:, 1])
    ratio = rng.uniform(low=scale_range[0], high=scale_range[1], size=1)[0]
    scale = max(xmax - xmin, ymax - ymin) * ratio
    if scale == 0:
        return np.zeros(motion.shape)
    result = motion.copy()
    result[..., :2] = (motion[..., :2] - [(xmin + xmax - scale) / 2, (ymin + ymax - scale) / 2]) / scale
    result[..., :2] = (result[..., :2] - 0.5) * 2
    return np.clip(result, -1, 1)


def pack_posetrack(annot_dir: str, out_prefix: str, scale_range=(0.25, 1), seed: int = 0) -> dict:
    """The whole of `PoseTrackDataset2D.__init__` (dataset_motion_2d.py:78-110) for the annotation files of `annot_dir` (the reference
    reads `data/motion2d/posetrack18_annotations/train/`): the tracks of every file in `sorted(os.listdir)` order, the first 30 frames of a
    track of at least 30, the `<= 306` filter on the summed confidence, `crop_scale(scale_range)`, `posetrack2h36m`, zeroing of the joints
    with confidence 0, and the filter that keeps the tracks whose root is visible in all 30 frames.  Writes `<prefix>.motion2d.npy`
    [N,30,17,3] float32 (what `torch.FloatTensor` makes of the reference's array) and `<prefix>.json`; returns the metadata.

    The crop ratios come from `np.random.RandomState(seed)` in motion order, which is what the reference's `np.random.seed(seed)` amounts
    to: the array equals the reference's `motions_2d` bit for bit.  The crop is drawn ONCE, here, as in the reference (its `__getitem__`
    only flips): `PackedMotion2D(kind='posetrack')`."""
    files = sorted(os.listdir(annot_dir))
    if not files:
        raise ValueError(f'no annotation files under {annot_dir}')
    rng = np.random.RandomState(seed)
    tracks = []
    for name in files:
        with open(os.path.join(annot_dir, name), 'r') as f:
            annots = json.load(f)['annotations']
        by_track = {}                                  # insertion order = first appearance, as the reference's defaultdict keeps it
        for a in annots:
            by_track.setdefault(a['track_id'], []).append(np.array(a['keypoints']).reshape(-1, 3))
        tracks += list(by_track.values())
    kept = []
    for track in tracks:
        if len(track) < 30:
            continue
        motion = np.array(track[:30])
        if np.sum(motion[:, :, 2]) <= 306:            # valid joint num threshold
            continue
        motion = _posetrack_to_h36m(_crop_scale_host(motion, scale_range, rng))
        motion[motion[:, :, 2] == 0] = 0
        if np.sum(motion[:, 0, 2]) < 30:
            continue                                   # root all visible (needed for framewise rootrel)
        kept.append(motion)
    if not kept:
        raise ValueError(f'{annot_dir}: no track passed the filters')
    np.save(out_prefix + '.motion2d.npy', np.array(kept).astype(np.float32))
    meta = dict(n=len(kept), clip_shape=[30, 17, 3], kind='posetrack', scale_range=[float(scale_range[0]), float(scale_range[1])], seed=int(seed))
    with open(out_prefix + '.json', 'w') as f:
        json.dump(meta, f)
    return meta


def pack_instav(motion_npy: str, id_npy: str, out_prefix: str, n_frames: int = 81, data_stride: int = 27, valid_threshold: float = 0.0,
                seed: int = 0) -> dict:
    """The whole of `InstaVDataset2D.__init__` (dataset_motion_2d.py:124-133) for `motion_all.npy` [frames,17,3] and `id_all.npy` [frames]:
    `split_clips(id_all, n_frames, data_stride)` with the random rounding of a short video's resampling from `np.random.RandomState(seed)`
    (the reference's `np.random.seed(seed)`), then the clips whose first root confidence is above `valid_threshold`.  Writes the clips
    materialised, `<prefix>.motion2d.npy` [N,n_frames,17,3] float32, and `<prefix>.json`; returns the metadata.  The per-clip stage of
    `__getitem__` (crop, zeroing, flip) is `mbx_motion2d_input`: `PackedMotion2D(kind='instav')`."""
    motion_all, id_all = np.load(motion_npy, mmap_mode='r'), np.load(id_npy)
    if len(motion_all) != len(id_all):
        raise ValueError(f'{len(motion_all)} frames but {len(id_all)} video ids')
    ids = _split_clips(id_all, int(n_frames), int(data_stride), np.random.RandomState(seed))
    if not ids:
        raise ValueError(f'{motion_npy}: no clip of {n_frames} frames')
    ids = np.stack(ids).astype(np.int64)
    ids = ids[np.asarray(motion_all[ids[:, 0], 0, 2]) > valid_threshold]
    if not len(ids):
        raise ValueError(f'{motion_npy}: no clip passed the valid_threshold filter')
    out = np.lib.format.open_memmap(out_prefix + '.motion2d.npy', mode='w+', dtype=np.float32, shape=(len(ids), int(n_frames)) + tuple(motion_all.shape[1:]))
    for i, row in enumerate(ids):
        out[i] = motion_all[row]
    out.flush()
    meta = dict(n=int(len(ids)), clip_shape=[int(n_frames)] + list(motion_all.shape[1:]), kind='instav', data_stride=int(data_stride), seed=int(seed))
    with open(out_prefix + '.json', 'w') as f:
        json.dump(meta, f)
    return meta


class PackedMotion2D:
    """The packed clips of `pack_posetrack` / `pack_instav` + the asynchronous batch stream of `pinned_batches` + the data sets'
    `__getitem__` on the device, and optionally the 2D front end of the pre-training step in the same launch.

        ds = PackedMotion2D(prefix, device='cuda', kind='instav', flip=True, scale_range=(0.25, 1))
        for motion_2d, target in ds.batches(64, epoch=e, rank=r, world=w):        # [B,T,17,3] twice (the same tensor): the reference's loader
            ...
        for x_aug, gt, conf in ds.batches(64, epoch=e, front=step, has_gt=False): # what PretrainStep.step_prepared takes
            ...
    kind='instav': crop_scale(scale_range) with a ratio per clip and batch, zeroing of unseen joints, random flip (dataset_motion_2d.py:
    139-147).  kind='posetrack': the flip only (:116-121; its crop happened once, at pack time).  Every batch is ONE launch of
    `mbx_motion2d_input` with a seed derived from (seed, epoch, rank, batch index) as `PackedAction` derives it.  With `front=step` (a
    `PretrainStep`) the same launch also writes the target, the confidence and the augmented input of train.py:162-172 with the step's
    `rootrel`, `mask` and `noise` (noise only if `has_gt`); a step with `no_conf` is refused (the reference cannot form `conf` there either).
    `ops`: kernel provider for host tensors (tests)."""

    def __init__(self, prefix: str, device='cuda', kind: str = 'instav', flip: bool = True, scale_range: Optional[Tuple[float, float]] = (0.25, 1),
                 ring: int = 3, ops=None):
        if kind not in ('instav', 'posetrack'):
            raise ValueError(f"kind must be 'instav' or 'posetrack', got {kind!r}")
        with open(prefix + '.json') as f:
            self.meta = json.load(f)
        self.motion_2d = np.load(prefix + '.motion2d.npy', mmap_mode='r')
        self.device = torch.device(device)
        self.kind, self.flip = kind, bool(flip)
        self.scale_range = tuple(scale_range) if (kind == 'instav' and scale_range) else None
        self.ring, self.ops = max(2, int(ring)), ops

    def __len__(self):
        return len(self.motion_2d)

    def batches(self, batch_size: int, shuffle: bool = True, epoch: int = 0, seed: int = 0, rank: int = 0, world: int = 1,
                drop_last: bool = False, front=None, has_gt: bool = True):
        from .augment import motion2d_input
        if front is not None and front.no_conf:
            raise ValueError('PackedMotion2D: a step with no_conf has no 2D front end (conf = batch_input[..., 2:] would be empty)')
        idx = shard_indices(len(self), shuffle, epoch, seed, rank, world)
        chunks = [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]
        if drop_last and chunks and len(chunks[-1]) < batch_size:
            chunks.pop()
        if not chunks:
            return
        stage = dict(scale_range=self.scale_range, zero_unseen=self.kind == 'instav', flip_prob=0.5 if self.flip else 0.0, ops=self.ops)
        stream = pinned_batches([self.motion_2d], chunks, batch_size, self.device, self.ring)
        try:
            for k, (motion,) in enumerate(stream):
                s = PackedAction.batch_seed(seed, epoch, rank, k)
                if front is None:
                    data = motion2d_input(motion, want=('data',), seed=s, **stage)['data']
                    yield data, data
                else:
                    out = motion2d_input(motion, want=('x_aug', 'gt', 'conf'), seed=s, aug=front.aug, noise=bool(front.noise and has_gt),
                                         mask=bool(front.mask), rootrel=bool(front.rootrel), **stage)
                    yield out['x_aug'], out['gt'], out['conf']
        finally:
            stream.close()


def m_per_class_batches(labels, m: int, batch_size: int, length: Optional[int] = None, seed: int = 0):
    """Index batches for one-shot training (train_action_1shot.py:145: `MPerClassSampler(labels, m=n_views, batch_size, length_before_new_iter)`
    of pytorch_metric_learning, which this package does not depend on).  Returns a list of `length // batch_size` int64 arrays (a
    `batch_sampler` for a DataLoader); `length` defaults to len(labels).

    Every batch holds `batch_size / m` DISTINCT classes with exactly `m` samples each, laid out class by class; a class with fewer than
    `m` samples is sampled with repetition, a larger one without.  With m >= 2 no anchor of the supervised-contrastive loss is ever
    without a positive -- the guarantee MPerClassSampler is used for (a lonely anchor makes the loss NaN).  The draw order of that
    library is NOT reproduced: the batches are a function of (labels, m, batch_size, length, seed) alone."""
    labels = np.asarray(labels).reshape(-1)
    if m < 2:
        raise ValueError(f'm = {m}: an anchor needs at least one positive in its batch (m >= 2)')
    if batch_size < m or batch_size % m:
        raise ValueError(f'batch_size {batch_size} must be a positive multiple of m = {m}')
    classes, inverse = np.unique(labels, return_inverse=True)
    per_batch = batch_size // m
    if len(classes) < per_batch:
        raise ValueError(f'{len(classes)} classes cannot fill {per_batch} distinct classes per batch')
    members = [np.flatnonzero(inverse == c) for c in range(len(classes))]
    length = len(labels) if length is None else int(length)
    rng = np.random.default_rng(seed)
    batches = []
    for _ in range(length // batch_size):
        out = []
        for c in rng.choice(len(classes), size=per_batch, replace=False):
            out.append(rng.choice(members[c], size=m, replace=len(members[c]) < m))
        batches.append(np.concatenate(out).astype(np.int64))
    return batches
