#!/usr/bin/env python
"""Mint tests/golden/wild.npz with the REFERENCE's own lib/data/dataset_wild.py (read_input, WildDetDataset; through it halpe2h36m and
lib/utils/utils_data.crop_scale), imported read-only at run time from the checkout oracle/make_golden.py names (MOTIONBERT_REFERENCE).
dataset_wild.py imports `ipdb`, which need not be installed: an empty stand-in module is registered first.

    python tools/mint_wild.py             # write the fixture
    python tools/mint_wild.py --check     # mint again and compare every array with the committed file, bit for bit

The JSON files come from the seeded makers of tests/wilderr.py, are written into a temporary directory and are not stored.  Per case of
wilderr.input_cases():
    in.{case}.out      read_input(json, vid_size, scale_range, focus): float32 [F,17,3], the reference's own output
    in.{case}.clips    the first dimension of every item of WildDetDataset(json, clip_len=wilderr.CLIP_LEN, ...), in order
    in.{case}.box      float64 [4] = (xs, ys, scale, valid joints), (0, 0, 0, valid joints) where crop_scale returns zeros.  The reference
                       keeps these as locals of crop_scale and returns none of them: they are the restatement's
                       (wilderr.input_ref), recorded only after its float32 output was found equal to the reference's bit for bit
                       (asserted here, case by case).  In pixel-only mode: the box crop_scale would take of the pixel-normalised track.
infer_wild.py itself cannot be imported (it runs at import and needs imageio): its lines 81-96 are restated in tests/wilderr.py and are
not part of this fixture."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden                             # noqa: E402
from tests import wilderr as WE                            # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'wild.npz')


def import_reference_wild():
    """lib.data.dataset_wild of the reference; this repository's own `lib` is put back after"""
    REF = make_golden.REF
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.')}
    had_ipdb = sys.modules.get('ipdb')
    try:
        if had_ipdb is None:
            sys.modules['ipdb'] = types.ModuleType('ipdb')
        for name in ('lib', 'lib.data', 'lib.utils'):
            mod = types.ModuleType(name)
            mod.__path__ = [os.path.join(REF, *name.split('.'))]
            sys.modules[name] = mod
        return importlib.import_module('lib.data.dataset_wild')
    finally:
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            sys.modules.pop(k)
        sys.modules.update(saved)
        if had_ipdb is None:
            sys.modules.pop('ipdb', None)


def mint():
    DW = import_reference_wild()
    save = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in WE.input_cases().items():
            path = WE.write_json(os.path.join(tmp, name + '.json'), case['items'])
            out = DW.read_input(path, case['vid_size'], case['scale_range'], case['focus'])
            assert out.dtype == np.float32 and out.shape[1:] == (17, 3)
            ds = DW.WildDetDataset(path, clip_len=WE.CLIP_LEN, vid_size=case['vid_size'], scale_range=case['scale_range'], focus=case['focus'])
            clips = np.asarray([ds[i].shape[0] for i in range(len(ds))], dtype=np.int64)
            assert WE.differing(np.concatenate([ds[i] for i in range(len(ds))]), out) == 0
            mine, box = WE.input_ref(WE.case_kp(case), case['vid_size'], case['scale_range'])
            assert WE.differing(mine, out) == 0, f'{name}: the restatement differs from the reference in {WE.differing(mine, out)} elements'
            save[f'in.{name}.out'], save[f'in.{name}.clips'], save[f'in.{name}.box'] = out, clips, box.reshape(4)
            print(f'[{name}] {out.shape[0]} frames, clips {clips.tolist()}, box {box.reshape(4).tolist()}, all zero {not out.any()}')
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
