"""The input stage on the device: 2D augmentation for pre-training and flip test-time augmentation.

`Augmenter2D` keeps the reference's interface (`lib/data/augmentation.py:10-81`: built from the config namespace, called as
`args.aug.augment2D(batch_input, noise=..., mask=...)` in train.py:171-172) but runs noise synthesis, confidence synthesis
and both masks as ONE kernel on the batch already resident in HBM; the reference draws eight random tensors on the host,
copies them to the device and runs ~25 element-wise kernels.  Random numbers are counter-based (a 64-bit seed per call from
torch's CPU generator), so a call is reproducible from its seed.

`action_input` and `motion2d_input` are the per-clip `__getitem__` stages of the NTU and of the 2D pre-training data sets, one launch each;
`motion2d_input` can also write what `train_epoch`'s `no_grad` block derives from a 2D batch (target, confidence, augmented input).

`flip_tta(model, x)` is the evaluation pattern of train.py:67-72 / infer_wild.py:75-80 -- model(x), model(flip(x)), flip
back, average -- as ONE forward over 2B samples in which the flipped half is an index remap inside the embedding kernel and
the flip-back + average is one pass over the output: no deep copies of the input (`flip_data` deep-copies) or the output."""
from __future__ import annotations

import pickle
from contextlib import nullcontext as _nullcontext
from typing import Optional

import torch

#: lib/utils/utils_data.py:60-61 (H36M 17-joint layout): joint j of the flipped pose takes the values of joint FLIP_PERM[j]
LEFT, RIGHT = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
FLIP_PERM = list(range(17))
for _l, _r in zip(LEFT, RIGHT):
    FLIP_PERM[_l], FLIP_PERM[_r] = _r, _l


class Augmenter2D:
    """Drop-in for `lib.data.augmentation.Augmenter2D` (constructor takes the same config namespace: d2c_params_path,
    noise_path, mask_ratio, mask_T_ratio); `augment2D(motion_2d, mask=False, noise=False)` returns a NEW [N,T,J,3] tensor."""

    def __init__(self, args=None, *, noise=None, d2c=None, mask_ratio=None, mask_T_ratio=None):
        if args is not None:
            with open(args.d2c_params_path, 'rb') as f:
                d2c = pickle.load(f)
            noise = torch.load(args.noise_path, weights_only=False)
            mask_ratio, mask_T_ratio = args.mask_ratio, args.mask_T_ratio
        self.d2c_params, self.noise = d2c, noise
        self.mask_ratio = 0.0 if mask_ratio is None else float(mask_ratio)
        self.mask_T_ratio = 0.0 if mask_T_ratio is None else float(mask_T_ratio)
        self.num_Kframes, self.noise_std = 27, 0.002          # augmentation.py:19-20 (27 is fixed in the kernel)
        self._dev = {}
        self.last_seed: Optional[int] = None

    def _noise_on(self, device):
        if device not in self._dev:
            self._dev[device] = tuple(self.noise[k].float().contiguous().to(device) for k in ('mean', 'std', 'weight'))
        return self._dev[device]

    def augment2D(self, motion_2d: torch.Tensor, mask: bool = False, noise: bool = False, seed: Optional[int] = None):
        if not (mask or noise):
            return motion_2d
        if not motion_2d.is_cuda:
            raise RuntimeError('motionbert_amd.augment.Augmenter2D runs on the ROCm device (move the batch first)')
        from . import hip_ops
        x = motion_2d.contiguous().float()
        if x.shape[-1] not in (2, 3):
            raise ValueError(f'expected [N,T,J,2|3] keypoints, got {tuple(x.shape)}')
        if x.shape[-1] == 2 and not noise:      # add_mask keeps the channel count: pad with ones only to mask, then cut again
            x = torch.cat([x, torch.ones_like(x[..., :1])], -1)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.last_seed = seed
        y = torch.empty(x.shape[:3] + (3,), dtype=torch.float32, device=x.device)
        d = self.d2c_params or dict(a=0.0, b=0.0, m=0.0, s=0.0)
        ur = float(self.noise['uniform_range']) if (self.noise is not None and 'uniform_range' in self.noise) else 0.06   # :31-34
        with torch.cuda.device(x.device):
            hip_ops.get().augment2d(x, y, self._noise_on(x.device) if noise else None, ur, self.noise_std,
                                    (d['a'], d['b'], d['m'], d['s']), self.mask_ratio, self.mask_T_ratio,
                                    (1 if noise else 0) | (2 if mask else 0), seed)
        return y if (noise or motion_2d.shape[-1] == 3) else y[..., :2]


#: random_move's defaults (lib/data/dataset_action.py:76-80): rotation in degrees, scale, translation
MOVE_RANGES = ((-10.0, 10.0), (0.9, 1.1), (-0.1, 0.1))


def action_input(x: torch.Tensor, random_move: bool = True, scale_range=(1, 1), seed: Optional[int] = None, params: Optional[torch.Tensor] = None,
                 return_params: bool = False, ops=None, angle_range=MOVE_RANGES[0], move_scale_range=MOVE_RANGES[1],
                 transform_range=MOVE_RANGES[2]):
    """`NTURGBD.__getitem__` (lib/data/dataset_action.py:173-182) for a batch x [N,M,T,J,3] (x, y, confidence) in ONE launch of
    `mbx_action_input`: `random_move` (:76-112, every joint of every person rotated, scaled and shifted by a transform that is
    interpolated over the clip) followed by `crop_scale(scale_range)` (lib/utils/utils_data.py:7-29: the box of the joints with
    confidence != 0 to [-1, 1], everything clipped; `scale_range=None` skips it, as a config's `scale_range: None` does).  Returns a NEW tensor.

    Each sample uses nine draws, [A0, A1, S0, S1, Tx0, Tx1, Ty0, Ty1, ratio]: the rows of `params` [N,9] if given, otherwise counter-based
    random numbers from `seed` (default: 62 bits from torch's CPU generator).  `return_params=True`: `(y, params_used [N,9])`."""
    from . import hip_ops
    if x.dim() != 5 or x.shape[-1] != 3:
        raise ValueError(f'expected [N,M,T,J,3] keypoints with confidence, got {tuple(x.shape)}')
    ops = hip_ops.provider(ops, 'motionbert_amd.augment.action_input', x, params, move='the batch')
    xc = x.contiguous().float()
    N = xc.shape[0]
    if params is not None:
        if tuple(params.shape) != (N, 9):
            raise ValueError(f'params must be [{N}, 9], got {tuple(params.shape)}')
        params = params.detach().to(device=xc.device, dtype=torch.float32).contiguous()
    elif seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    crop = scale_range is not None and scale_range is not False
    ranges = (tuple(angle_range), tuple(move_scale_range), tuple(transform_range), tuple(scale_range) if crop else (1.0, 1.0))
    for lo, hi in ranges:
        if not lo <= hi:
            raise ValueError(f'range ({lo}, {hi}) has lo > hi')
    y = torch.empty_like(xc)
    used = torch.empty(N, 9, dtype=torch.float32, device=xc.device) if return_params else None
    if N:
        with (torch.cuda.device(xc.device) if xc.is_cuda else _nullcontext()):
            ops.action_input(xc, y, params, used, ranges, (1 if random_move else 0) | (2 if crop else 0), 0 if seed is None else int(seed))
    return (y, used) if return_params else y


#: flag bits of `mbx_motion2d_input` (include/mbx.h)
M2D_CROP, M2D_ZERO, M2D_FLIP, M2D_NOISE, M2D_MASK, M2D_ROOTREL = 1, 2, 4, 8, 16, 32
_M2D_OUTPUTS = ('data', 'gt', 'conf', 'x_aug')


def motion2d_input(x: torch.Tensor, *, scale_range=(0.25, 1), zero_unseen: bool = True, flip_prob: float = 0.5, aug: Optional[Augmenter2D] = None,
                   noise: bool = False, mask: bool = False, rootrel: bool = True, want=('data',), seed: Optional[int] = None,
                   params: Optional[torch.Tensor] = None, return_params: bool = False, ops=None):
    """`InstaVDataset2D.__getitem__` (lib/data/dataset_motion_2d.py:139-147) and the `no_grad` block of `train_epoch` for a 2D batch
    (train.py:162-172) for x [N,T,J,3] (x, y, confidence) in ONE launch of `mbx_motion2d_input`: `crop_scale(scale_range)` (`None` skips it),
    zeroing of the joints with confidence 0, `flip_data` of the clips whose draw is below `flip_prob`; then, from that item `data`, the
    target `gt` (`rootrel`: `data - data[:, :, 0:1]`, else the confidence channel minus `data[n,0,0,2]`), `conf` = `data[..., 2:]` and
    `x_aug` = `aug.augment2D(data, noise=noise, mask=mask)` with the same `seed` (bit for bit).  Returns a dict of the NEW tensors named in
    `want` ('data', 'gt', 'conf' [N,T,J,1], 'x_aug').

    Each sample uses two draws, (ratio, u_flip): the rows of `params` [N,2] if given, otherwise counter-based random numbers from `seed`
    (default: 62 bits from torch's CPU generator) on streams the augmentation does not use.  `return_params=True`: `(dict, params_used [N,2])`."""
    from . import hip_ops
    if x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f'expected [N,T,J,3] keypoints with confidence, got {tuple(x.shape)}')
    want = tuple(want)
    if not want or any(w not in _M2D_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f'want must name some of {_M2D_OUTPUTS} once each, got {want}')
    if (noise or mask) and aug is None:
        raise ValueError('noise / mask need an Augmenter2D (aug=)')
    if not 0.0 <= float(flip_prob) <= 1.0:
        raise ValueError(f'flip_prob = {flip_prob} is not in [0, 1]')
    if flip_prob > 0 and x.shape[2] != 17:
        raise ValueError(f'the flip uses the 17-joint left/right table of lib/utils/utils_data.py:60-61, J = {x.shape[2]} (pass flip_prob=0)')
    crop = scale_range is not None and scale_range is not False
    lo, hi = (float(scale_range[0]), float(scale_range[1])) if crop else (1.0, 1.0)
    if not lo <= hi:
        raise ValueError(f'range ({lo}, {hi}) has lo > hi')
    ops = hip_ops.provider(ops, 'motionbert_amd.augment.motion2d_input', x, params, move='the batch')
    xc = x.contiguous().float()
    N, T, J, _ = xc.shape
    if params is not None:
        if tuple(params.shape) != (N, 2):
            raise ValueError(f'params must be [{N}, 2], got {tuple(params.shape)}')
        params = params.detach().to(device=xc.device, dtype=torch.float32).contiguous()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    out = {w: torch.empty((N, T, J, 1 if w == 'conf' else 3), dtype=torch.float32, device=xc.device) for w in want}
    used = torch.empty(N, 2, dtype=torch.float32, device=xc.device) if return_params else None
    flags = ((M2D_CROP if crop else 0) | (M2D_ZERO if zero_unseen else 0) | (M2D_FLIP if flip_prob > 0 else 0) | (M2D_NOISE if noise else 0) |
             (M2D_MASK if mask else 0) | (M2D_ROOTREL if rootrel else 0))
    if N:
        d = (aug.d2c_params if aug is not None else None) or dict(a=0.0, b=0.0, m=0.0, s=0.0)
        ur = float(aug.noise['uniform_range']) if (aug is not None and aug.noise is not None and 'uniform_range' in aug.noise) else 0.06
        with (torch.cuda.device(xc.device) if xc.is_cuda else _nullcontext()):
            ops.motion2d_input(xc, out.get('data'), out.get('gt'), out.get('conf'), out.get('x_aug'), params, used, (lo, hi), float(flip_prob),
                               aug._noise_on(xc.device) if noise else None, ur, aug.noise_std if aug is not None else 0.002,
                               (d['a'], d['b'], d['m'], d['s']), aug.mask_ratio if aug is not None else 0.0,
                               aug.mask_T_ratio if aug is not None else 0.0, flags, int(seed))
        if aug is not None and 'x_aug' in want:
            aug.last_seed = int(seed)
    return (out, used) if return_params else out


def flip_tta(model, x: torch.Tensor, clip_lens=None, tables=None) -> torch.Tensor:
    """(model(x) + flip_back(model(flip(x)))) / 2 under no_grad, 17-joint H36M layout (train.py:67-72).
    With `clip_lens` it is the ragged form: x [F,17,dim_in] holds clips of those lengths one after another
    (`DSTformer.forward_ragged`, which also explains `tables`), and the result is [F,17,dim_out]."""
    if model.num_joints != 17:
        raise ValueError('flip_tta uses the 17-joint left/right table of lib/utils/utils_data.py:60-61')
    with torch.no_grad():
        if clip_lens is not None:
            return model.forward_ragged(x, clip_lens, return_rep='flip_tta', tables=tables)
        return model.forward(x, return_rep='flip_tta')
