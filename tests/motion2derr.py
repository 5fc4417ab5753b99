"""Restatements, inputs and gates for the 2D pre-training front end (csrc/motion2d.hip: mbx_motion2d_input = lib/data/dataset_motion_2d.py:
116-147 + train.py:162-172 + lib/utils/utils_data.py:7-29,54-66).  Plain module, no fixtures: tests/test_gpu_motion2d.py applies it to the
kernel on the GPU, tests/test_motion2derr.py to seeded corruptions on the CPU, tools/mint_motion2d.py pins it to the reference's own data
sets at 1e-12 (tests/golden/motion2d.npz).

  item_eq        the data set's per-clip stage in torch, in a chosen dtype: crop_scale (actionerr.action_input_eq on x[:, None], crop only),
                 zeroing of the unseen joints, flip_data of the clips whose draw is below flip_prob
  front_eq       the no_grad block of train_epoch on that item: target (rootrel or not), confidence before augmentation, and
                 Augmenter2D.augment2D through oracle/augment_oracle.py with the counter-based draws evaluated in the same dtype
  all_eq         both: dict(data, gt, conf, x_aug) + zeroed samples + the magnitude of the floors
  posetrack_eq   posetrack2h36m
  motion_inputs / planted / PLANTED_PARAMS / posetrack_files / instav_arrays    seeded inputs (not stored in the fixture)
  gates / check  the gates
  TorchMotion2DOps   the kernel provider's entry on CPU tensors, for the host-logic tests

Gates, by the standing rule of tests/actionerr.py: the yardstick is the SAME equations evaluated in float32 by torch on the CPU against
float64, per sample and per output as a max-norm; the device gets 4 x that (a factor 2 for device log / cos / division rounding in other
places, a factor 2 for comparing maxima over different rounding patterns).  Floors, 8 fp32 ulps (actionerr.FLOOR) of the magnitude the
output went through: actionerr's `mag` of the crop for `data` and `conf`; twice that for `gt`, a difference of two such values, each with
its own rounding; for `x_aug` max(mag, 1), since the synthesised confidence a / (d + a) + b d + shift is of order 1 before its clip whatever
the coordinates are.  The discrete outcomes -- which samples are zeroed, params_out against the draws, which points the masks remove -- must
match exactly."""
import os

import numpy as np
import torch

from oracle import augment_oracle as AO
from tests import actionerr as AE

CROP, ZERO, FLIP, NOISE, MASK, ROOTREL = 1, 2, 4, 8, 16, 32
OUTPUTS = ('data', 'gt', 'conf', 'x_aug')
FLIP_PERM = [0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13]      # utils_data.py:60-61
STREAM_RATIO, STREAM_FLIP = 16, 17
SCALE_RANGE = (0.25, 1.0)

CORRUPTIONS = ('box_over_all', 'div_ratio', 'threshold_3', 'conf_unclipped', 'no_zeroing', 'flip_no_negate', 'flip_no_perm',
               'rootrel_xy_only', 'root_of_frame_0', 'conf_after_aug')
_CROP_CORRUPTIONS = ('box_over_all', 'div_ratio', 'threshold_3', 'conf_unclipped')


def f32(v):
    return float(np.float32(v))


class AugConfig:
    """the arguments of the augmentation as the kernel receives them: every scalar rounded to float32"""

    def __init__(self, z=None, mask_ratio=0.05, mask_T_ratio=0.1):
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment2d.npz')) if z is None else z
        self.noise = dict(mean=torch.from_numpy(z['noise_mean']).float(), std=torch.from_numpy(z['noise_std']).float(),
                          weight=torch.from_numpy(z['noise_weight']).float())
        self.d2c = dict(zip('abms', (f32(v) for v in z['d2c'])))
        self.mask_ratio, self.mask_T_ratio = f32(mask_ratio), f32(mask_T_ratio)
        self.uniform_range, self.noise_std = f32(0.06), f32(0.002)

    def augmenter(self):
        from motionbert_amd.augment import Augmenter2D
        return Augmenter2D(noise=self.noise, d2c=self.d2c, mask_ratio=self.mask_ratio, mask_T_ratio=self.mask_T_ratio)


# ------------------------------------------------------------------------------------------------ restatements
def draws_in(seed, B, T, J, dtype):
    """augment_oracle.draws with the normal numbers formed in `dtype` from the (exact, 24-bit) uniform ones"""
    u = lambda s, i: AO.uniform(seed, s, i).to(dtype)                                                       # noqa: E731
    nrm = lambda s, i: torch.sqrt(-2.0 * torch.log(u(s, i) + (1.0 / 33554432.0))) * torch.cos(6.28318530717958647692 * u(s + 1, i))   # noqa: E731
    ki = torch.arange(B * AO.K * J, dtype=torch.int64).reshape(B, AO.K, J)
    ti = torch.arange(T * J, dtype=torch.int64).reshape(T, J)
    ii = torch.arange(B * T * J, dtype=torch.int64).reshape(B, T, J)
    return dict(sel=u(0, ki)[..., None], gaussian=torch.stack([nrm(1, ki), nrm(3, ki)], -1), uniform=torch.stack([u(5, ki), u(6, ki)], -1),
                jitter=torch.stack([nrm(7, ti), nrm(9, ti)], -1), shift=nrm(11, ii), mask=u(13, ii)[..., None],
                mask_T=u(14, torch.arange(T, dtype=torch.int64)).reshape(1, T, 1, 1))


def item_eq(x, params, flags, flip_prob, dtype, corrupt=None, clip=True):
    """(data [N,T,J,3], zeroed [N], mag [N]) of x [N,T,J,3] and params [N,2] = (ratio, u_flip) in `dtype`"""
    assert corrupt is None or corrupt in CORRUPTIONS
    N = x.shape[0]
    p9 = torch.zeros(N, 9, dtype=params.dtype)           # float64 params (the reference's own draws) stay float64 in the float64 restatement
    p9[:, 8] = params[:, 0]
    y, zeroed, mag = AE.action_input_eq(x[:, None], p9, AE.CROP if flags & CROP else 0, dtype, corrupt if corrupt in _CROP_CORRUPTIONS else None, clip)
    data = y[:, 0]
    if flags & ZERO and corrupt != 'no_zeroing':
        data = torch.where((data[..., 2:] == 0), torch.zeros_like(data), data)
    if flags & FLIP:
        which = params[:, 1].float() < torch.tensor(flip_prob, dtype=torch.float32)
        f = data if corrupt == 'flip_no_perm' else data[:, :, FLIP_PERM]
        f = f.clone()
        if corrupt != 'flip_no_negate':
            f[..., 0] = -f[..., 0]
        data = torch.where(which.reshape(N, 1, 1, 1), f, data)
    return data, zeroed, mag


def front_eq(data, flags, seed, cfg, dtype, corrupt=None):
    """dict(gt, conf, x_aug) of the item `data` (train.py:162-172)"""
    B, T, J, _ = data.shape
    if flags & ROOTREL:
        if corrupt == 'rootrel_xy_only':
            gt = torch.cat([data[..., :2] - data[:, :, 0:1, :2], data[..., 2:]], -1)
        elif corrupt == 'root_of_frame_0':
            gt = data - data[:, 0:1, 0:1]
        else:
            gt = data - data[:, :, 0:1]
    else:
        gt = data.clone()
        gt[..., 2] = gt[..., 2] - gt[:, 0:1, 0:1, 2]
    x_aug = data
    if flags & (NOISE | MASK):
        r = draws_in(seed, B, T, J, dtype)
        if flags & NOISE:
            x_aug = AO.add_noise(x_aug, cfg.noise, cfg.d2c, r, uniform_range=cfg.uniform_range, noise_std=cfg.noise_std)
        if flags & MASK:
            x_aug = AO.add_mask(x_aug, r, cfg.mask_ratio, cfg.mask_T_ratio)
    conf = x_aug[..., 2:] if corrupt == 'conf_after_aug' else data[..., 2:]
    return dict(gt=gt, conf=conf, x_aug=x_aug)


def all_eq(x, params, flags, flip_prob, seed, cfg, dtype, corrupt=None):
    data, zeroed, mag = item_eq(x, params, flags, flip_prob, dtype, corrupt)
    out = front_eq(data, flags, seed, cfg, dtype, corrupt)
    out['data'] = data
    return out, zeroed, mag


def posetrack_eq(x, dtype=torch.float64):
    """posetrack2h36m (dataset_motion_2d.py:54-74) for x [...,T,17,C]"""
    x = x.to(dtype)
    src = {1: 12, 2: 14, 3: 16, 4: 11, 5: 13, 6: 15, 8: 1, 9: 0, 10: 2, 11: 5, 12: 7, 13: 9, 14: 6, 15: 8, 16: 10}
    y = torch.zeros_like(x)
    for j, c in src.items():
        y[..., j, :] = x[..., c, :]
    y[..., 0, :] = (x[..., 11, :] + x[..., 12, :]) * 0.5
    y[..., 7, :] = (y[..., 0, :] + y[..., 8, :]) * 0.5
    y[..., 0, 2] = torch.minimum(x[..., 11, 2], x[..., 12, 2])
    y[..., 7, 2] = torch.minimum(y[..., 0, 2], y[..., 8, 2])
    return y


def clipped_fraction(x, params):
    """per sample, the share of the x, y coordinates that the clip changes, on the float64 restatement alone"""
    y, _, _ = item_eq(x, params, CROP, 0.0, torch.float64, clip=False)
    return (y[..., :2].abs() > 1 + 1e-9).double().mean(dim=(1, 2, 3))


# ------------------------------------------------------------------------------------------------ gates
def gates(x, params, flags, flip_prob, seed, cfg):
    """(float64 outputs, per-sample gates {output: [N]}, all-zero samples [N])"""
    ref, zeroed, mag = all_eq(x, params, flags, flip_prob, seed, cfg, torch.float64)
    y32, _, _ = all_eq(x, params, flags, flip_prob, seed, cfg, torch.float32)
    floor = dict(data=mag, conf=mag, gt=2 * mag, x_aug=mag.clamp_min(1.0))
    g = {}
    for k in OUTPUTS:
        yard = (y32[k].double() - ref[k]).abs().reshape(len(x), -1).amax(1)
        g[k] = torch.maximum(AE.FACTOR * yard, AE.FLOOR * floor[k])
    return ref, g, zeroed | (ref['data'] == 0).reshape(len(x), -1).all(1)


def check(got, x, params, flags, flip_prob, seed, cfg):
    """dict(output -> worst share of its gate) + 'exact' (zeroed samples and masked points as float64 has them) for kernel (or corrupted)
    outputs `got` (a dict with any of OUTPUTS)"""
    ref, g, zero = gates(x, params, flags, flip_prob, seed, cfg)
    res, exact = {}, True
    for k in OUTPUTS:
        if k not in got:
            continue
        v = got[k].detach().cpu().double().reshape(ref[k].shape)
        err = (v - ref[k]).abs().reshape(len(x), -1).amax(1)
        res[k] = float(torch.nan_to_num(err / g[k], nan=float('inf')).max())
    if 'data' in got:
        exact = exact and bool(torch.equal((got['data'].detach().cpu() == 0).reshape(len(x), -1).all(1), zero))
    if 'x_aug' in got and flags & MASK:
        gone = lambda t: (t.detach().cpu() == 0).all(-1)                                                    # noqa: E731
        exact = exact and bool(torch.equal(gone(got['x_aug']), gone(ref['x_aug'])))
    res['exact'] = exact
    return res


def passes(res):
    return res['exact'] and all(v <= 1.0 for k, v in res.items() if k != 'exact')


def draw_params(N, seed, scale_range=SCALE_RANGE):
    """params [N,2] fp32 exactly as mbx_motion2d_input forms them from `seed` (the fused multiply-add restated in float64, as
    actionerr.draw_params does)"""
    idx = torch.arange(N, dtype=torch.int64)
    lo, hi = torch.tensor(scale_range[0], dtype=torch.float32), torch.tensor(scale_range[1], dtype=torch.float32)
    ratio = torch.minimum(((hi - lo).double() * AO.uniform(seed, STREAM_RATIO, idx).double() + lo.double()).float(), hi)
    return torch.stack([ratio, AO.uniform(seed, STREAM_FLIP, idx)], 1)


# ------------------------------------------------------------------------------------------------ inputs
def motion_inputs(N, T, J, seed, lost=0.04):
    """x [N,T,J,3] fp32: actionerr's clouds of joints around a drifting centre, confidences in [0.3, 1), `lost` of the joints undetected
    (confidence 0, parked near the corner (-1, -1))"""
    x = AE.motion_inputs(N, 1, T, J, seed)[:, 0].clone()
    g = torch.Generator().manual_seed(seed + 5)
    gone = torch.rand(N, T, J, generator=g) < lost
    k = int(gone.sum())
    x[gone] = torch.cat([-1.0 + 0.01 * torch.rand(k, 2, generator=g), torch.zeros(k, 1)], 1)
    return x.float().contiguous()


PLANTED = ('three_valid', 'coincident', 'root_unseen', 'ratio_quarter', 'conf_1p5')
PLANTED_PARAMS = torch.tensor([[1.0, 0.75], [1.0, 0.25], [0.7, 0.25], [0.25, 0.75], [1.0, 0.25]])      # (ratio, u_flip): flips at 0.5 where 0.25


def planted(seed=8300, T=9, J=17):
    """x [5,T,J,3]: the samples of PLANTED"""
    g = torch.Generator().manual_seed(seed)
    x = motion_inputs(len(PLANTED), T, J, seed + 1, lost=0.0)
    x[0, ..., :2] = 0.3 * (torch.rand(T, J, 2, generator=g) - 0.5)
    x[0, ..., 2] = 0.0
    x[0, 0, :3, :2] = torch.tensor([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5]])
    x[0, 0, :3, 2] = 0.9
    x[1, ..., 2] = 0.0                        # five valid joints of one frame at one point: scale == 0 exactly, in any precision
    x[1, T // 2, 3:8, :2] = torch.tensor([0.25, -0.125])
    x[1, T // 2, 3:8, 2] = 0.8
    x[2, 1, 0, 2] = 0.0                       # a frame's root, a left joint and a right joint unseen
    x[2, 2, 4, 2] = 0.0
    x[2, 3, 14, 2] = 0.0
    x[2, 4:6, 9, 2] = 0.0
    x[3, ..., :2] = 0.02 * torch.randn(T, J, 2, generator=g)      # a tight cloud and two far joints: ratio 0.25 clips the far ones and little else
    x[3, :, 13, :2] += torch.tensor([0.3, 0.3])
    x[3, :, 6, :2] -= torch.tensor([0.3, 0.3])
    x[4, :, ::3, 2] = 1.5
    x[4, :, 1::4, 2] = -1.5
    return x.contiguous()


def posetrack_files(seed=8400):
    """{file name: annotation dict} of three synthetic PoseTrack files: six tracks -- two ordinary ones, one of 25 frames (too short), one of
    low confidence (sum <= 306), one whose hips are hidden in a frame (root not visible), one of 40 frames (cut to 30) with a few joints
    undetected; coordinates in pixels, interleaved over the frames as the annotation files have them"""
    r = np.random.RandomState(seed)
    files, tid = {}, 0
    plan = {'000342_mpii_train.json': (('plain', 30), ('short', 25)), '001001_bonn_train.json': (('lowconf', 30), ('hips', 31)),
            '009999_mpii_train.json': (('long', 40), ('plain', 30))}
    for name, tracks in plan.items():
        per_track = []
        for kind, T0 in tracks:
            base = r.uniform(200, 900, (1, 1, 2)) + np.cumsum(r.normal(0, 3, (T0, 1, 2)), axis=0) + r.normal(0, 60, (1, 17, 2)) + r.normal(0, 2, (T0, 17, 2))
            conf = np.ones((T0, 17, 1))
            if kind == 'lowconf':
                conf[:, 5:] = 0.0
            if kind == 'hips':
                conf[7, 11] = 0.0
            if kind == 'long':
                conf[3, 9] = conf[12, 0] = conf[20, 15] = 0.0
            kp = np.concatenate([np.round(base, 2), conf], -1)
            kp[conf[..., 0] == 0] = 0.0
            per_track.append((tid, kp))
            tid += 1
        annots = []
        for t in range(max(len(kp) for _, kp in per_track)):
            for k, kp in per_track:
                if t < len(kp):
                    annots.append(dict(track_id=int(k), image_id=int(t), keypoints=[float(v) for v in kp[t].reshape(-1)]))
        files[name] = dict(annotations=annots, images=[dict(id=int(t)) for t in range(40)])
    return files


INSTAV_FRAMES = (100, 60, 110, 30)           # per video: one window of 81; a short video, resampled; two windows (stride 27); a short LAST
                                             # video, which split_clips drops


def instav_arrays(seed=8500):
    """(motion_all [300,17,3] float32, id_all [300]) of four synthetic videos; the first root confidence of video 2 is 0 (valid_idx drops it)"""
    r = np.random.RandomState(seed)
    motion, ids = [], []
    for v, F in enumerate(INSTAV_FRAMES):
        xy = r.uniform(-0.3, 0.3, (1, 1, 2)) + np.cumsum(r.normal(0, 0.004, (F, 1, 2)), axis=0) + r.normal(0, 0.12, (1, 17, 2)) + r.normal(0, 0.01, (F, 17, 2))
        conf = r.uniform(0.3, 1.0, (F, 17, 1))
        conf[r.uniform(size=(F, 17)) < 0.04] = 0.0
        conf[0, 0] = 0.0 if v == 2 else 0.9
        motion.append(np.concatenate([xy, conf], -1))
        ids += [v] * F
    return np.concatenate(motion).astype(np.float32), np.asarray(ids, dtype=np.int64)


def fixture_frames(T):
    return AE.fixture_frames(T)


# ------------------------------------------------------------------------------------------------ a kernel provider in torch (CPU tests)
class TorchMotion2DOps:
    """`motion2d_input` of the kernel provider on CPU tensors, from the restatements: same argument list as HipOps, float32 results.  `calls` lists (shape, flags, seed, params given, outputs asked)."""

    def __init__(self):
        self.calls = []

    def motion2d_input(self, x, data, gt, conf, x_aug, params_in, params_out, ratio_range, flip_prob, noise, uniform_range, jitter_std, d2c,
                       mask_ratio, mask_T_ratio, flags, seed):
        assert x.dtype == torch.float32 and x.is_contiguous()
        outs = dict(data=data, gt=gt, conf=conf, x_aug=x_aug)
        self.calls.append((tuple(x.shape), int(flags), int(seed), params_in is not None, tuple(k for k, v in outs.items() if v is not None)))
        p = params_in if params_in is not None else draw_params(x.shape[0], int(seed), ratio_range)
        if params_out is not None:
            params_out.copy_(p)
        cfg = AugConfig.__new__(AugConfig)
        cfg.noise = None if noise is None else dict(mean=noise[0], std=noise[1], weight=noise[2])
        cfg.d2c = dict(zip('abms', (f32(v) for v in d2c)))
        cfg.mask_ratio, cfg.mask_T_ratio, cfg.uniform_range, cfg.noise_std = f32(mask_ratio), f32(mask_T_ratio), f32(uniform_range), f32(jitter_std)
        # as the kernel: the item from the float64 restatement, rounded; target, confidence and augmentation in float32 from that item
        data32 = item_eq(x, p, flags, flip_prob, torch.float64)[0].float()
        ref = dict(front_eq(data32, flags, int(seed), cfg, torch.float32), data=data32)
        for k, v in outs.items():
            if v is not None:
                v.copy_(ref[k].reshape(v.shape))
