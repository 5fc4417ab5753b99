#!/usr/bin/env python
"""Mint tests/golden/motion2d.npz with the REFERENCE's own lib/data/dataset_motion_2d.py (PoseTrackDataset2D, InstaVDataset2D), imported
read-only at run time from the checkout oracle/make_golden.py names (MOTIONBERT_REFERENCE).  The classes open fixed relative paths, so they
run inside a temporary directory that holds the synthetic annotation files of tests/motion2derr.py under those paths.

    python tools/mint_motion2d.py             # write the fixture
    python tools/mint_motion2d.py --check     # mint again and compare every array with the committed file, bit for bit

Inputs come from the seeded makers of tests/motion2derr.py (posetrack_files, instav_arrays) and are not stored.
    pt.motions_2d     PoseTrackDataset2D().motions_2d after np.random.seed(0), float64 as the class keeps it: six tracks in, the too-short, the
                      low-confidence and the root-hidden one filtered
    pt.items / pt.flips    what __getitem__ returns for every index, and whether it flipped (random.random is wrapped and recorded)
    iv.motions_2d     InstaVDataset2D().motions_2d after np.random.seed(0) (float32: motion_all holds float32 values)
    iv.params         per clip (ratio, u_flip): the ratio is numpy's own draw rounded to float32 where it is drawn (np.random.uniform is
                      wrapped for the call, so the reference computes with the value the kernel will be handed); u_flip is 0.25 where
                      random.random() > 0.5 made the reference flip and 0.75 where not
    iv.items          what __getitem__ returns for every index with those draws
Items are kept in float64: `torch.FloatTensor`, the last thing __getitem__ does to a clip (the first for PoseTrack), is replaced by a float64
conversion for the call, so that the restatement can be pinned at 1e-12."""
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import motion2derr as ME                         # noqa: E402
from tools.mint_action import Float32Draws                  # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'motion2d.npz')


def import_reference_motion2d():
    """lib.data.dataset_motion_2d of the reference, imported as mint_action.py imports its modules; this repository's own `lib` is put back after"""
    import importlib
    from oracle import make_golden
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.')}
    try:
        for name in ('lib', 'lib.data', 'lib.utils', 'lib.model'):
            mod = types.ModuleType(name)
            mod.__path__ = [os.path.join(make_golden.REF, *name.split('.'))]
            sys.modules[name] = mod
        return importlib.import_module('lib.data.dataset_motion_2d')
    finally:
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            sys.modules.pop(k)
        sys.modules.update(saved)


class RecordedFlips:
    """random.random for the duration of a `with`: python's own draws, recorded"""

    def __enter__(self):
        self.real, self.drawn = random.random, []

        def rnd():
            v = self.real()
            self.drawn.append(v)
            return v
        random.random = rnd
        return self

    def __exit__(self, *exc):
        random.random = self.real


class Float64Items:
    """`torch.FloatTensor` as the data set module sees it, for the duration of a `with`: a float64 conversion"""

    def __init__(self, module):
        self.module = module

    def __enter__(self):
        self.real = self.module.torch
        shim = types.SimpleNamespace(FloatTensor=lambda a: a.double() if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=np.float64)))
        self.module.torch = shim

    def __exit__(self, *exc):
        self.module.torch = self.real


def write_inputs(root):
    d = os.path.join(root, 'data/motion2d/posetrack18_annotations/train')
    os.makedirs(d)
    for name, content in ME.posetrack_files().items():
        with open(os.path.join(d, name), 'w') as f:
            json.dump(content, f)
    d = os.path.join(root, 'data/motion2d/InstaVariety')
    os.makedirs(d)
    motion_all, id_all = ME.instav_arrays()
    np.save(os.path.join(d, 'motion_all.npy'), motion_all.astype(np.float64))
    np.save(os.path.join(d, 'id_all.npy'), id_all)


def mint():
    DM = import_reference_motion2d()
    save = {}
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        write_inputs(tmp)
        os.chdir(tmp)
        try:
            np.random.seed(0)
            pt = DM.PoseTrackDataset2D()
            np.random.seed(0)
            iv = DM.InstaVDataset2D()
        finally:
            os.chdir(here)
    assert pt.motions_2d.dtype == np.float64
    save['pt.motions_2d'] = pt.motions_2d
    random.seed(8600)
    items, flips = [], []
    for i in range(len(pt)):
        with RecordedFlips() as r, Float64Items(DM):
            items.append(pt[i][0].numpy())
        flips.append(r.drawn[0] > 0.5)
    save['pt.items'], save['pt.flips'] = np.stack(items), np.asarray(flips)
    print(f'[posetrack] motions_2d {pt.motions_2d.shape} flips {flips}')
    m32 = iv.motions_2d.astype(np.float32)
    assert np.array_equal(m32.astype(np.float64), iv.motions_2d)
    save['iv.motions_2d'] = m32
    np.random.seed(8601)
    items, params = [], []
    for i in range(len(iv)):
        with Float32Draws() as d, RecordedFlips() as r, Float64Items(DM):
            items.append(iv[i][0].numpy())
        assert len(d.drawn) == 1 and len(r.drawn) == 1
        params.append([float(d.drawn[0][0]), 0.25 if r.drawn[0] > 0.5 else 0.75])
    save['iv.items'], save['iv.params'] = np.stack(items), np.asarray(params, dtype=np.float64)
    print(f'[instav] motions_2d {m32.shape} params {params}')
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
