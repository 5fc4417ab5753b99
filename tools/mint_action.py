#!/usr/bin/env python
"""Mint tests/golden/action.npz with the REFERENCE's own lib/data/dataset_action.py (ActionDataset, random_move), lib/utils/utils_data.py
(crop_scale, resample) and lib/utils/learning.py (accuracy), imported read-only at run time from the checkout oracle/make_golden.py names
(MOTIONBERT_REFERENCE).  lib/utils/tools.py imports `easydict`, which need not be installed: a stand-in module with a dict subclass is
registered first.  Everything in float64.

    python tools/mint_action.py             # write the fixture
    python tools/mint_action.py --check     # mint again and compare every array with the committed file, bit for bit

Inputs come from the seeded makers of tests/actionerr.py and are not stored, but for the annotation arrays:
    ann.{i}.keypoint / .keypoint_score / .meta (label, total_frames, height, width)   the synthetic annotation file of actionerr.annotations()
    ann.{split}.motions / .labels             the reference's `ActionDataset(pkl, split, n_frames=27).motions` / `.labels`, float32 as it keeps them
    in.{case}.params                          the nine draws per sample in the order random_move and crop_scale make them, numpy's own, rounded
                                              to float32 where they are drawn (np.random.uniform is wrapped for the call, so the reference
                                              computes with the values the kernel will be handed)
    in.{case}.out                             crop_scale(random_move(x)) per sample with x as float64, [N,M,F,J,3] on the frames
                                              actionerr.fixture_frames(T) (in.{case}.frames); the flag cases skip what their flags switch off
    xe.{N}.{C}.loss / .dlogits / .acc         nn.CrossEntropyLoss()(logits, labels), its autograd gradient (rows xe.{N}.{C}.rows) and
                                              accuracy(logits, labels, topk=(1, 5)) in percent"""
import importlib
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden                             # noqa: E402
from tests import actionerr as AE                          # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'action.npz')


def import_reference_action():
    """(lib.data.dataset_action, lib.utils.utils_data, lib.utils.learning) of the reference; this repository's own `lib` is put back after"""
    REF = make_golden.REF
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.')}
    had_easydict = sys.modules.get('easydict')
    try:
        if had_easydict is None:
            stand_in = types.ModuleType('easydict')
            stand_in.EasyDict = type('EasyDict', (dict,), {})
            sys.modules['easydict'] = stand_in
        for name in ('lib', 'lib.data', 'lib.utils', 'lib.model'):
            mod = types.ModuleType(name)
            mod.__path__ = [os.path.join(REF, *name.split('.'))]
            sys.modules[name] = mod
        return tuple(importlib.import_module(n) for n in ('lib.data.dataset_action', 'lib.utils.utils_data', 'lib.utils.learning'))
    finally:
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            sys.modules.pop(k)
        sys.modules.update(saved)
        if had_easydict is None:
            sys.modules.pop('easydict', None)


class Float32Draws:
    """np.random.uniform for the duration of a `with`: numpy's own draws, rounded to float32 and recorded"""

    def __enter__(self):
        self.real, self.drawn = np.random.uniform, []

        def uniform(*a, **k):
            v = np.asarray(self.real(*a, **k)).astype(np.float32).astype(np.float64)
            self.drawn.append(v.reshape(-1))
            return v
        np.random.uniform = uniform
        return self

    def __exit__(self, *exc):
        np.random.uniform = self.real


def mint():
    DA, UD, LE = import_reference_action()
    save = {}
    # ---- the annotation file through ActionDataset.__init__
    anns = AE.annotations()
    for i, a in enumerate(anns):
        save[f'ann.{i}.keypoint'], save[f'ann.{i}.keypoint_score'] = a['keypoint'], a['keypoint_score']
        save[f'ann.{i}.meta'] = np.asarray([a['label'], a['total_frames'], a['img_shape'][0], a['img_shape'][1]], dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        pkl = os.path.join(tmp, 'ntu_synthetic.pkl')
        with open(pkl, 'wb') as f:
            pickle.dump(AE.annotation_file(anns), f)
        for split in AE.ANN_SPLITS:
            ds = DA.ActionDataset(pkl, split, n_frames=AE.ANN_N_FRAMES)
            assert ds.motions.dtype == np.float32
            save[f'ann.{split}.motions'], save[f'ann.{split}.labels'] = ds.motions, np.asarray(ds.labels, dtype=np.int64)
            print(f'[annotations {split}] motions {ds.motions.shape} is_train {ds.is_train}')
    # ---- the input stage
    for name, (x, flags, crop_range) in AE.input_cases().items():
        N, M, T, J, _ = x.shape
        frames = AE.fixture_frames(T)
        np.random.seed(AE.input_seed((N, M, T)) + 17)
        outs, params = [], []
        for n in range(N):
            motion = x[n].double().numpy().copy()
            with Float32Draws() as d:
                drawn_move = flags & AE.MOVE
                if drawn_move:
                    motion = DA.random_move(motion)
                n_move = len(d.drawn)
                if flags & AE.CROP:
                    motion = UD.crop_scale(motion, scale_range=list(crop_range))
                move = np.concatenate(d.drawn[:n_move]) if drawn_move else np.asarray([0, 0, 1, 1, 0, 0, 0, 0], dtype=np.float64)
                ratio = d.drawn[n_move] if len(d.drawn) > n_move else np.asarray([1.0])       # crop_scale returns before its draw for < 4 valid joints
            assert move.shape == (8,) and ratio.shape == (1,)
            params.append(np.concatenate([move, ratio]))
            outs.append(np.asarray(motion, dtype=np.float64)[:, frames])
        save[name + '.params'], save[name + '.out'], save[name + '.frames'] = np.stack(params), np.stack(outs), frames.astype(np.int64)
        print(f'[input {name}] {tuple(x.shape)} flags {flags} kept frames {len(frames)}')
    # ---- cross-entropy and top-k
    crit = torch.nn.CrossEntropyLoss()
    for shape in AE.XENT_SHAPES:
        z, lab = AE.logit_inputs(*shape, AE.xent_seed(shape))
        zz = z.double().requires_grad_(True)
        loss = crit(zz, lab)
        loss.backward()
        top1, top5 = LE.accuracy(zz.detach(), lab, topk=(1, 5))
        rows = AE.fixture_rows(*shape)
        tag = 'xe.%d.%d' % shape
        save[tag + '.loss'] = np.asarray(float(loss.detach()), dtype=np.float64)
        save[tag + '.rows'], save[tag + '.dlogits'] = rows.astype(np.int64), zz.grad.numpy()[rows]
        save[tag + '.acc'] = np.asarray([float(top1), float(top5)], dtype=np.float64)
        print(f'[xent {shape}] loss {float(loss.detach()):.9f} top-1 {float(top1):.3f} % top-5 {float(top5):.3f} %')
    return save


def main():
    save = mint()
    if '--check' in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(save), (sorted(old.files), sorted(save))
        for k, v in save.items():
            assert old[k].dtype == np.asarray(v).dtype and old[k].tobytes() == np.asarray(v).tobytes(), k
        print('re-minted bit-identically:', OUT)
        return
    np.savez_compressed(OUT, **save)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
