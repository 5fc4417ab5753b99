"""Restatements, inputs and gates for in-the-wild inference (csrc/wild.hip, motionbert_amd/wild.py).  Plain module, no fixtures:
tests/test_gpu_wild.py applies it to the kernels on the GPU, tests/test_wilderr.py to seeded corruptions on the CPU, tests/test_wild.py runs
`wild.infer` on the CPU stand-ins, tools/mint_wild.py pins the input stage to the reference's own `lib.data.dataset_wild` bit for bit
(tests/golden/wild.npz).

  halpe2h36m / input_eq / input_ref   dataset_wild.py:15-65 and :77-86 (with lib/utils/utils_data.py:7-29) in numpy, in a chosen dtype
                                      (float64: the restatement; float32: a corruption)
  output_eq / pixel_eq / reference_loop   infer_wild.py:81-88, :93-96 and the whole loop :63-96.  `infer_wild.py` CANNOT be imported: it
                                      parses arguments, loads a checkpoint and opens a video at import and needs `imageio`.  These three
                                      are therefore a numpy / torch restatement with line references, NOT the reference's own code; only
                                      the input stage is pinned to the reference by the fixture.
  detections / items / input_cases / output_cases   seeded inputs; the JSON files are written into a temporary directory and not stored
  NumpyWildOps                        `wild_input` / `wild_output` of the kernel provider on CPU tensors, with seeded corruptions
  FixedNet                            a network stand-in whose output is an element-wise function of its input (batch size cannot matter)
  input_check / output_check          the gates: EQUAL BITS, outputs NaN-filled beforehand, guard rows around them untouched

Gates.  Every operation of both stages is a single correctly rounded IEEE operation (+, -, *, /, min, max, a conversion) in a fixed order,
so a correct implementation reproduces the reference's bits: the gate is bit equality, on the float32 output and on the float64 box.
Coordinates are float32 detections widened to float64, as AlphaPose's JSON holds them: they carry fractional digits, and the same
equations in float32 do NOT give the same bits (the 'float32' corruption proves it)."""
import json
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle.augment_oracle import flip_data

CLIP_LEN = 9                    # of the tests (tiny_trained has maxlen 9 too)
CHUNK = 64                      # motionbert_amd.wild.CHUNK_FRAMES, asserted in tests/test_wilderr.py
MAP = [19, 12, 14, 16, 11, 13, 15, None, 18, 0, 17, 5, 7, 9, 6, 8, 10]       # dataset_wild.py:48-64
PIXEL, CROP = 1, 2
ROOTREL, GT_2D, OUT_PIXEL = 1, 2, 4

INPUT_CORRUPTIONS = ('box_over_all', 'threshold_le4', 'map_row', 'conf7_pair', 'float32', 'wh_swapped', 'max_wh')
OUTPUT_CORRUPTIONS = ('clip_dropped', 'root_z_per_track', 'gt2d_wrong_clip')
CORRUPTIONS = INPUT_CORRUPTIONS + OUTPUT_CORRUPTIONS


# ------------------------------------------------------------------------------------------------ input stage
def halpe2h36m(x, corrupt=None):
    """dataset_wild.py:46-65"""
    T, V, C = x.shape
    y = np.zeros([T, 17, C], dtype=x.dtype)
    for j, v in enumerate(MAP):
        if v is not None:
            y[:, j, :] = x[:, v, :]
    y[:, 7, :] = (x[:, 18, :] + x[:, 19, :]) * x.dtype.type(0.5)
    if corrupt == 'map_row':
        y[:, 12, :] = x[:, 8, :]                     # LElbow takes RElbow
    if corrupt == 'conf7_pair':
        y[:, 7, 2] = (x[:, 17, 2] + x[:, 18, 2]) * x.dtype.type(0.5)
    return y


def crop_scale_eq(motion, ratio, corrupt=None):
    """utils_data.py:7-29 with the drawn ratio as an argument -> (result, box = (xs, ys, scale, valid joints); (0, 0, 0, n) where the
    reference returns zeros)"""
    t = motion.dtype.type
    valid = motion[..., 2] != 0
    n = float(valid.sum())
    sel = np.ones_like(valid) if corrupt == 'box_over_all' else valid
    coords = motion[sel][:, :2]
    if (n <= 4 if corrupt == 'threshold_le4' else n < 4):
        return np.zeros(motion.shape, dtype=motion.dtype), np.array([0.0, 0.0, 0.0, n])
    xmin, xmax, ymin, ymax = coords[:, 0].min(), coords[:, 0].max(), coords[:, 1].min(), coords[:, 1].max()
    scale = max(xmax - xmin, ymax - ymin) * t(ratio)
    if scale == 0:
        return np.zeros(motion.shape, dtype=motion.dtype), np.array([0.0, 0.0, 0.0, n])
    xs = (xmin + xmax - scale) / t(2)
    ys = (ymin + ymax - scale) / t(2)
    result = motion.copy()
    result[..., :2] = (motion[..., :2] - np.array([xs, ys], dtype=motion.dtype)) / scale
    result[..., :2] = (result[..., :2] - t(0.5)) * t(2)
    result = np.clip(result, t(-1), t(1))
    return result, np.array([xs, ys, scale, n], dtype=np.float64)


def input_eq(kp, half_w, half_h, pix_scale, ratio, flags, dtype=np.float64, corrupt=None):
    """one track: kp [F,26,3] -> (float32 [F,17,3], box [4] float64), dataset_wild.py:77-86 with the constants of :79-81 as arguments"""
    assert corrupt is None or corrupt in INPUT_CORRUPTIONS
    if corrupt == 'float32':
        dtype = np.float32
    if corrupt == 'wh_swapped':
        half_w, half_h = half_h, half_w
    if corrupt == 'max_wh':
        pix_scale = max(half_w, half_h)
    t = np.dtype(dtype).type
    m = halpe2h36m(np.asarray(kp).astype(dtype), corrupt)
    if flags & PIXEL:
        m[:, :, :2] = m[:, :, :2] - np.array([half_w, half_h], dtype=dtype)
        m[:, :, :2] = m[:, :, :2] / t(pix_scale)
    box = None
    if flags & CROP:
        m, box = crop_scale_eq(m, ratio, corrupt)
    else:
        box = crop_scale_eq(m, 1.0, corrupt)[1]
    return m.astype(np.float32), box


def consts(vid_size):
    if not vid_size:
        return 0.0, 0.0, 1.0
    w, h = vid_size
    half = np.array([w, h]) / 2.0
    return float(half[0]), float(half[1]), min(w, h) / 2.0


def input_ref(kp, vid_size, scale_range, seq_lens=None, corrupt=None):
    """(float32 [F,17,3], box [S,4]) of kp [F,26,3] as `read_input(json, vid_size, scale_range, focus)` normalises it, per track"""
    flags = (PIXEL if vid_size else 0) | (CROP if scale_range else 0)
    assert flags and (not scale_range or scale_range[0] == scale_range[1])
    hw, hh, ps = consts(vid_size)
    outs, boxes, at = [], [], 0
    for n in ([len(kp)] if seq_lens is None else seq_lens):
        o, b = input_eq(kp[at:at + n], hw, hh, ps, scale_range[0] if scale_range else 1.0, flags, corrupt=corrupt)
        outs.append(o)
        boxes.append(b)
        at += n
    return np.concatenate(outs), np.stack(boxes)


# ------------------------------------------------------------------------------------------------ seeded detections
def detections(F, seed, w=1920, h=1080):
    """[F,26,3] float64 holding float32 values (AlphaPose writes float32 detections as decimal text that json.load reads back exactly):
    a skeleton of 26 joints around a centre that walks through the middle of a w x h image, confidences in [0.3, 1)"""
    r = np.random.RandomState(seed)
    centre = np.array([w * 0.5, h * 0.5]) + np.cumsum(r.normal(0, 1.5, (F, 1, 2)), axis=0)
    pose = r.normal(0, 0.11 * min(w, h), (1, 26, 2)) + r.normal(0, 2.0, (F, 26, 2))
    xy = np.clip(centre + pose, [0.3 * w, 0.2 * h], [0.7 * w, 0.8 * h])
    conf = r.uniform(0.3, 1.0, (F, 26, 1))
    return np.concatenate([xy, conf], -1).astype(np.float32).astype(np.float64)


def items(tracks, order=None):
    """the item list of an AlphaPose result file for tracks {idx: [F,26,3]}; `order`: a list of (idx, frame) (default: track after track)"""
    order = order or [(k, f) for k, v in tracks.items() for f in range(len(v))]
    return [dict(image_id='%d.jpg' % f, category_id=1, keypoints=[float(v) for v in tracks[k][f].reshape(-1)], score=2.5, idx=k) for k, f in order]


def write_json(path, item_list):
    with open(path, 'w') as f:
        json.dump(item_list, f)
    return path


def case_kp(case, by_track=False):
    """what `wild.read_alphapose` returns for the case's items, without a file"""
    tracks = OrderedDict()
    for it in case['items']:
        if case['focus'] is not None and it['idx'] != case['focus']:
            continue
        tracks.setdefault(it['idx'] if by_track else None, []).append(np.array(it['keypoints']).reshape([-1, 3]))
    return OrderedDict((k, np.stack(v)) for k, v in tracks.items()) if by_track else np.stack(tracks[None])


PERSON_LENS = OrderedDict([(3, CLIP_LEN - 4), (7, 2 * CLIP_LEN), (1, CLIP_LEN + 1)])      # idx -> frames: shorter than a clip, a multiple, a tail of 1
PLANTS = ('first', 'last', 'invalid')


def persons():
    """three interleaved persons (PERSON_LENS), idx in order of first appearance 3, 7, 1; round-robin while a track has frames left"""
    tracks = OrderedDict((k, detections(n, 8100 + k)) for k, n in PERSON_LENS.items())
    for i, k in enumerate(tracks):
        tracks[k][:, :, 0] = (tracks[k][:, :, 0] + 180.0 * (i - 1)).astype(np.float32)
    order = [(k, f) for f in range(max(PERSON_LENS.values())) for k in tracks if f < PERSON_LENS[k]]
    return tracks, order


def input_cases():
    """name -> dict(items, vid_size, scale_range, focus): every case of the fixture, of the CPU checks and of the GPU parity test"""
    cases = OrderedDict()

    def add(name, kp, vid_size=None, scale_range=(1, 1), focus=None, item_list=None):
        cases[name] = dict(items=item_list if item_list is not None else items({0: kp}), vid_size=vid_size,
                           scale_range=list(scale_range) if scale_range else None, focus=focus)

    add('f1', detections(1, 8001))
    for name, k in (('valid3', 3), ('valid4', 4)):          # Halpe 12, 14, 16 (, 11) -> H36M 1, 2, 3 (, 4): exactly k valid joints in the track
        kp = detections(2, 8002)
        kp[:, :, 2] = 0.0
        kp[0, [12, 14, 16, 11][:k], 2] = np.float32(0.8)
        add(name, kp)
    kp = detections(3, 8003)                                # five valid joints at one point: scale == 0 in any precision
    kp[:, :, 2] = 0.0
    kp[1, [5, 6, 7, 8, 9], :] = np.array([812.25, 431.5, 0.75])
    add('coincident', kp)
    for F in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        for plant in PLANTS:
            kp = detections(F, 8010 + F)
            if plant == 'first':
                kp[0, 12, :2] = np.float32([50.123, 1070.77])
            elif plant == 'last':
                kp[F - 1, 10, :2] = np.float32([1890.61, 12.345])
            else:
                kp[F // 2, 9, :] = np.float32([5.5, 1079.9, 0.0])             # confidence 0: must not move the box
            add(f'chunk.{F}.{plant}', kp)
    kp = detections(5, 8020)                                # neck and hip undetected in two frames: H36M 0, 7, 8 invalid there
    kp[[1, 3], 18, 2] = kp[[1, 3], 19, 2] = 0.0
    kp[1, 19, :2] = np.float32([20.25, 30.75])              # ... and far outside: must not move the box
    add('neck_hip_0', kp)
    kp = detections(4, 8021)
    kp[:, ::3, 2] = np.float32(1.5)
    kp[:, 18, 2], kp[:, 19, 2] = np.float32(1.75), np.float32(0.5)        # joint 7: (1.75 + 0.5) / 2 = 1.125
    add('conf_gt1.crop', kp)
    add('conf_gt1.pixel', kp, vid_size=(1920, 1080), scale_range=None)
    add('pixel.1920x1080', detections(11, 8030), vid_size=(1920, 1080), scale_range=None)
    add('pixel.720x1280', detections(11, 8031, 720, 1280), vid_size=(720, 1280), scale_range=None)
    add('both.1920x1080', detections(11, 8032), vid_size=(1920, 1080))
    add('both.720x1280', detections(7, 8033, 720, 1280), vid_size=(720, 1280))
    tracks, order = persons()
    its = items(tracks, order)
    for k in tracks:
        add(f'persons.crop.focus{k}', None, focus=k, item_list=its)
        add(f'persons.pixel.focus{k}', None, vid_size=(1920, 1080), scale_range=None, focus=k, item_list=its)
    return cases


def persons_cases():
    """(items, [(name of the focus case, idx)]) for the by_track runs: 'crop' and 'pixel'"""
    tracks, order = persons()
    return items(tracks, order), list(tracks)


# ------------------------------------------------------------------------------------------------ output stage and the loop
def output_eq(pred, x, rootrel, gt_2d, corrupt=None, track_starts=None):
    """infer_wild.py:81-88 for one batch [N,T,17,3] float32 (a copy is returned; the reference writes in place)"""
    p = np.array(pred, dtype=np.float32, copy=True)
    if rootrel:
        p[:, :, 0, :] = 0                                   # :82
    elif corrupt == 'root_z_per_track':
        p[np.asarray(track_starts, dtype=bool), 0, 0, 2] = 0
    else:
        p[:, 0, 0, 2] = 0                                   # :84
    if gt_2d:
        xx = np.roll(x, 1, axis=0) if corrupt == 'gt2d_wrong_clip' else x
        p[..., :2] = xx[..., :2]                            # :87
    return p


def pixel_eq(results_all, vid_size):
    """infer_wild.py:93-96 on the stitched float32 result"""
    results_all = results_all * (min(vid_size) / 2.0)
    results_all[:, :, :2] = results_all[:, :, :2] + np.array(vid_size) / 2.0
    return results_all


def reference_loop(model, motion, clip_len, flip, rootrel, gt_2d, no_conf, vid_size=None, device='cpu'):
    """infer_wild.py:63-96 on `motion` = WildDetDataset.vid_all [F,17,3] float32: batch 1, two forwards and two flip_data copies per clip,
    a .cpu() per clip, np.hstack + np.concatenate; `vid_size`: opts.pixel"""
    results_all = []
    with torch.no_grad():
        for index in range(math.ceil(len(motion) / clip_len)):                                  # WildDetDataset.__getitem__, batch_size 1
            batch_input = torch.from_numpy(motion[index * clip_len:min((index + 1) * clip_len, len(motion))])[None].to(device)
            if no_conf:
                batch_input = batch_input[:, :, :, :2]
            if flip:
                batch_input_flip = flip_data(batch_input)
                predicted_3d_pos_1 = model(batch_input)
                predicted_3d_pos_flip = model(batch_input_flip)
                predicted_3d_pos_2 = flip_data(predicted_3d_pos_flip)
                predicted_3d_pos = (predicted_3d_pos_1 + predicted_3d_pos_2) / 2.0
            else:
                predicted_3d_pos = model(batch_input)
            if rootrel:
                predicted_3d_pos[:, :, 0, :] = 0
            else:
                predicted_3d_pos[:, 0, 0, 2] = 0
            if gt_2d:
                predicted_3d_pos[..., :2] = batch_input[..., :2]
            results_all.append(predicted_3d_pos.cpu().numpy())
    results_all = np.hstack(results_all)
    results_all = np.concatenate(results_all)
    if vid_size:
        results_all = pixel_eq(results_all, vid_size)
    return results_all


def output_cases(seed=8200):
    """seeded batches for mbx_wild_output: dict(pred [n,T,17,3], x [n,T,17,2|3], dst [n], starts [n], F, rootrel, gt_2d, vid_size)"""
    r = np.random.RandomState(seed)
    cases = OrderedDict()
    for name, n, T, xc, rootrel, gt_2d, vid in (('plain', 5, CLIP_LEN, 3, 0, 0, None), ('rootrel', 3, CLIP_LEN, 3, 1, 0, None),
                                               ('gt2d', 4, CLIP_LEN, 3, 0, 1, None), ('gt2d.noconf', 4, CLIP_LEN, 2, 1, 1, None),
                                               ('pixel.1920x1080', 5, CLIP_LEN, 3, 0, 0, (1920, 1080)), ('pixel.720x1280', 3, 4, 3, 1, 0, (720, 1280)),
                                               ('pixel.gt2d', 6, 1, 2, 0, 1, (1920, 1080)), ('one', 1, 1, 3, 0, 0, None), ('big', 70, CLIP_LEN, 3, 0, 1, (1920, 1080))):
        F = n * T + 7
        slots = r.permutation(n)                                # the clips land in shuffled places, with a gap of 7 rows that stay untouched
        dst =(slots * T + np.where(slots >= n // 2, 7, 0)).astype(np.int64)
        cases[name] = dict(pred=r.normal(0, 0.4, (n, T, 17, 3)).astype(np.float32), x=r.uniform(-1, 1, (n, T, 17, xc)).astype(np.float32),
                           dst=dst, starts=(dst == dst.min()), F=F, rootrel=bool(rootrel), gt_2d=bool(gt_2d), vid_size=vid)
    return cases


def output_ref(case, corrupt=None):
    """the stitched [F,17,3] float32 result of a case, NaN where no clip lands"""
    p = output_eq(case['pred'], case['x'], case['rootrel'], case['gt_2d'], corrupt, case['starts'])
    out = np.full((case['F'], 17, 3), np.nan, dtype=np.float32)
    T = p.shape[1]
    for i, d in enumerate(case['dst']):
        if corrupt == 'clip_dropped' and i == len(case['dst']) - 1:
            continue
        out[d:d + T] = p[i]
    if case['vid_size']:
        out = pixel_eq(out, case['vid_size'])
    return out


# ------------------------------------------------------------------------------------------------ a kernel provider in numpy (CPU tests)
class NumpyWildOps:
    """`wild_input` / `wild_output` of the kernel provider on CPU tensors, from the float64 restatements: same argument lists as HipOps.
    `corrupt`: one of CORRUPTIONS.  `calls` lists the entries used."""

    def __init__(self, corrupt=None):
        assert corrupt is None or corrupt in CORRUPTIONS
        self.corrupt, self.calls = corrupt, []

    def wild_input(self, kp, chunk_tab, seq_chunk_ptr, half_w, half_h, pix_scale, ratio, flags, y, box):
        assert kp.dtype == torch.float64 and y.dtype == torch.float32 and chunk_tab.dtype == torch.int32 and seq_chunk_ptr.dtype == torch.int32
        self.calls.append(('wild_input', tuple(kp.shape), int(flags), y.shape[-1]))
        tab, ptr, k = chunk_tab.numpy(), seq_chunk_ptr.numpy(), kp.numpy()
        assert tab[:, 2].sum() == len(k) and (tab[:, 2] >= 1).all() and (tab[:, 2] <= CHUNK).all()
        c = self.corrupt if self.corrupt in INPUT_CORRUPTIONS else None
        for s in range(len(ptr) - 1):
            rows = tab[ptr[s]:ptr[s + 1]]
            if not len(rows):
                if box is not None:
                    box[s] = 0.0
                continue
            assert (rows[:, 0] == s).all() and (rows[1:, 1] == rows[:-1, 1] + rows[:-1, 2]).all()
            f0, n = int(rows[0, 1]), int(rows[:, 2].sum())
            o, b = input_eq(k[f0:f0 + n], half_w, half_h, pix_scale, ratio, flags, corrupt=c)
            y[f0:f0 + n] = torch.from_numpy(o[..., :y.shape[-1]])
            if box is not None:
                box[s] = torch.from_numpy(b)

    def wild_output(self, pred, x, dst_frames, dst_max, flags, pix_scale, half_w, half_h, out):
        assert pred.dtype == torch.float32 and out.dtype == torch.float32 and dst_frames.dtype == torch.int32
        self.calls.append(('wild_output', tuple(pred.shape), int(flags)))
        c = self.corrupt if self.corrupt in OUTPUT_CORRUPTIONS else None
        dst = dst_frames.numpy()
        n, T = pred.shape[:2]
        assert len(dst) == n and (n == 0 or int(dst.max()) == int(dst_max)) and int(dst_max) + T <= out.shape[0]
        p = output_eq(pred.numpy(), None if x is None else x.numpy(), bool(flags & ROOTREL), bool(flags & GT_2D), c, dst == 0)
        if flags & OUT_PIXEL:                                   # infer_wild.py:95-96 with the constants as the kernel gets them
            p = p * np.float32(pix_scale)
            p[..., :2] = p[..., :2] + np.array([half_w, half_h])
        for i, d in enumerate(dst):
            if c == 'clip_dropped' and i == n - 1:
                continue
            out[int(d):int(d) + T] = torch.from_numpy(p[i])


class FixedNet:
    """Stands in for the backbone: an element-wise float32 function of the input (products, sums and a table over frame and joint), so
    that batch size and batch order cannot change a bit; `forward(x, return_rep='flip_tta')` is `flip_tta`'s contract in the reference's
    arithmetic (infer_wild.py:74-78)."""
    num_joints, maxlen = 17, 243

    def __init__(self, seed=8300, maxlen=243):
        r = np.random.RandomState(seed)
        self.w = [torch.from_numpy(r.uniform(-1, 1, 3).astype(np.float32)) for _ in range(3)]
        self.table = torch.from_numpy(r.normal(0, 0.3, (maxlen, 17, 3)).astype(np.float32))
        self.maxlen, self.calls, self.evals = maxlen, [], 0

    def eval(self):
        self.evals += 1
        return self

    def _f(self, x):
        assert x.dim() == 4 and x.shape[2] == 17 and x.shape[3] in (2, 3) and not torch.is_grad_enabled()
        out = x[..., 0:1] * self.w[0] + x[..., 1:2] * self.w[1]
        if x.shape[3] == 3:
            out = out + x[..., 2:3] * self.w[2]
        return out + self.table[:x.shape[1]]

    def __call__(self, x):
        self.calls.append(tuple(x.shape))
        return self._f(x)

    def forward(self, x, return_rep=False):
        if return_rep == 'flip_tta':
            self.calls.append(('tta',) + tuple(x.shape))
            return (self._f(x) + flip_data(self._f(flip_data(x)))) / 2.0
        return self(x)


# ------------------------------------------------------------------------------------------------ the gates
def differing(a, b):
    """elements whose BITS differ (NaN == NaN of the same bits; +0 != -0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return int((a.view(view) != b.view(view)).sum())


GUARD = 3      # rows of 17 x channels values kept NaN before and after an output


def run_input(ops, device, kp, seq_lens, vid_size, scale_range, channels=3, with_box=True):
    """`ops.wild_input` straight (no wrapper) into NaN-filled outputs with guard rows around them -> (y [F,17,channels] float32,
    box [S,4] float64, guards untouched) on the host"""
    from motionbert_amd import wild
    F = len(kp)
    tab, ptr = wild.chunk_table(seq_lens)
    hw, hh, ps = consts(vid_size)
    flags = (PIXEL if vid_size else 0) | (CROP if scale_range else 0)
    ybuf = torch.full((F + 2 * GUARD, 17, channels), math.nan, dtype=torch.float32, device=device)
    bbuf = torch.full((len(seq_lens) + 2, 4), math.nan, dtype=torch.float64, device=device)
    ops.wild_input(torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float64)).to(device), torch.from_numpy(tab).to(device), torch.from_numpy(ptr).to(device),
                   hw, hh, ps, float(scale_range[0]) if scale_range else 1.0, flags, ybuf[GUARD:GUARD + F], bbuf[1:-1] if with_box else None)
    yh, bh = ybuf.cpu(), bbuf.cpu()
    clean = bool(torch.isnan(yh[:GUARD]).all() and torch.isnan(yh[GUARD + F:]).all() and torch.isnan(bh[0]).all() and torch.isnan(bh[-1]).all())
    if not with_box:
        clean = clean and bool(torch.isnan(bh).all())
    return yh[GUARD:GUARD + F].numpy(), bh[1:-1].numpy(), clean


def input_check(ops, device, case, want_out, want_box):
    """dict(out = differing elements of the float32 output, box = of the float64 box, nan = NaN left in the output, clean = guards
    untouched, nc = differing elements of the two-channel form) for a fixture case"""
    kp = case_kp(case)
    y, box, clean = run_input(ops, device, kp, [len(kp)], case['vid_size'], case['scale_range'])
    y2, _, clean2 = run_input(ops, device, kp, [len(kp)], case['vid_size'], case['scale_range'], channels=2, with_box=False)
    return dict(out=differing(y, want_out), box=differing(box, want_box.reshape(1, 4)), nan=int(np.isnan(y).sum()), clean=clean and clean2,
                nc=differing(y2, np.ascontiguousarray(want_out[..., :2])))


def passes(res):
    return res['out'] == 0 and res['box'] == 0 and res['nan'] == 0 and res['nc'] == 0 and res['clean']


def run_output(ops, device, case):
    """`ops.wild_output` straight into a NaN-filled [F,17,3] with guard rows -> (out on the host, guards untouched, pred unchanged)"""
    F = case['F']
    buf = torch.full((F + 2 * GUARD, 17, 3), math.nan, dtype=torch.float32, device=device)
    pred = torch.from_numpy(case['pred']).to(device)
    hw, hh, ps = consts(case['vid_size'])
    flags = (ROOTREL if case['rootrel'] else 0) | (GT_2D if case['gt_2d'] else 0) | (OUT_PIXEL if case['vid_size'] else 0)
    ops.wild_output(pred, torch.from_numpy(case['x']).to(device), torch.from_numpy(case['dst'].astype(np.int32)).to(device), int(case['dst'].max()), flags,
                    ps, hw, hh, buf[GUARD:GUARD + F])
    bh = buf.cpu()
    clean = bool(torch.isnan(bh[:GUARD]).all() and torch.isnan(bh[GUARD + F:]).all())
    return bh[GUARD:GUARD + F].numpy(), clean, differing(pred.cpu().numpy(), case['pred']) == 0


def output_check(ops, device, case):
    out, clean, kept = run_output(ops, device, case)
    return dict(out=differing(out, output_ref(case)), clean=clean, pred_kept=kept)


def load_fixture():
    from tests.helpers import GOLDEN
    return np.load(os.path.join(GOLDEN, 'wild.npz'), allow_pickle=False)
