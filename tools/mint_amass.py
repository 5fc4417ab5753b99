#!/usr/bin/env python
"""Mint tests/golden/amass.npz with the REFERENCE's own tools/compress_amass.py and tools/convert_amass.py, run unmodified (runpy) and
read-only at run time from the checkout oracle/make_golden.py names (MOTIONBERT_REFERENCE).  The scripts open fixed relative paths, so they
run inside a temporary directory that holds the synthetic AMASS tree of tests/amasserr.py under those paths.

    python tools/mint_amass.py             # write the fixture
    python tools/mint_amass.py --check     # mint again and compare every array with the committed file, bit for bit

tools/preprocess_amass.py, the script between the two, needs `human_body_prior`, which is not a dependency of this project: its output
(`amass_joints_h36m_60.pkl`) is made here by its own loop (gender rule, slices of 2,916 frames, `torch.Tensor(...)` of every parameter) around
`plain_lbs_h` of tests/amasserr.py in float64 on the synthetic body models of `tests.amasserr.tree_models()`.  The body model is therefore
pinned by plain_lbs_h, exactly as SMPL was; what the fixture pins is everything the two runnable scripts do.
    fps_names / fps_rows   the rows of fps.csv: (len_ori, fps, len_new) per file compress_amass.py kept (it keeps the file with 150 pose
                           columns too; preprocess_amass.py could not evaluate it, and it takes no further part)
    strided_len            frames per sequence at 60 fps, of the sequences that reach convert_amass.py
    split_id               convert_amass.py's `split_clips(vid_list, 243, 81)` after np.random.seed(0)
    joints_cam             its `joints_cam_all` [frames,17,3] float32: the camera-frame joints, stacked"""
import os
import pickle
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import amasserr as AE                            # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'amass.npz')
MAX_LEN = 2916


class ReferenceModules:
    """for the duration of a `with`: the reference's `lib` mounted as tools/mint_motion2d.py mounts it, and an empty stand-in for `ipdb`
    (imported by the scripts, never used, not installed); this repository's own `lib` is put back after"""

    def __enter__(self):
        from oracle import make_golden
        self.ref = make_golden.REF
        self.saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.') or k == 'ipdb'}
        for name in ('lib', 'lib.data', 'lib.utils', 'lib.model'):
            mod = types.ModuleType(name)
            mod.__path__ = [os.path.join(self.ref, *name.split('.'))]
            sys.modules[name] = mod
        sys.modules['ipdb'] = types.ModuleType('ipdb')
        return self

    def __exit__(self, *exc):
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.') or k == 'ipdb']:
            sys.modules.pop(k)
        sys.modules.update(self.saved)

    def run(self, script):
        np.random.seed(0)
        path0 = list(sys.path)
        try:
            return runpy.run_path(os.path.join(self.ref, 'tools', script), run_name='__main__')
        finally:
            sys.path[:] = path0


def preprocess_stand_in(models):
    """preprocess_amass.py:26-63 with plain_lbs_h (float64) in the place of BodyModel: reads all_motions_fps60.pkl, writes
    amass_joints_h36m_60.pkl (a list of [17,T,3] arrays, one per slice); returns the strided lengths of the sequences it evaluated"""
    with open('data/AMASS/all_motions_fps60.pkl', 'rb') as f:
        motion_data = pickle.load(f)
    all_joints, lens = [], []
    for bdata in motion_data:
        if bdata['poses'].shape[1] != 156:
            continue
        gender = bdata['gender']
        if (str(gender) != 'female') and (str(gender) != 'male'):
            gender = 'female'
        m = AE.model_dict(models[str(gender)], AE.F64)
        n = len(bdata['trans'])
        lens.append(n)
        for sid in range(n // MAX_LEN + 1):
            a, b = sid * MAX_LEN, min((sid + 1) * MAX_LEN, n)
            t = {k: torch.Tensor(bdata[k][a:b]).double() for k in ('poses', 'trans')}
            betas = torch.Tensor(np.repeat(bdata['betas'][:16][np.newaxis], repeats=b - a, axis=0)).double()
            dmpls = torch.Tensor(bdata['dmpls'][a:b, :8]).double()
            kp = AE.plain_lbs_h(m, t['poses'], betas, dmpls, t['trans'])
            all_joints.append(np.ascontiguousarray(kp.numpy().transpose(1, 0, 2)))        # (17,T,3), as np.dot(J_reg, mesh) gives
    with open('data/AMASS/amass_joints_h36m_60.pkl', 'wb') as f:
        pickle.dump(all_joints, f)
    return lens


def mint():
    models = AE.tree_models()
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp, ReferenceModules() as ref:
        AE.write_tree(os.path.join(tmp, 'data/AMASS/amass_202203'))
        os.chdir(tmp)
        try:
            ref.run('compress_amass.py')
            with open('data/AMASS/fps.csv') as f:
                rows = [line.split(' , ') for line in f.read().splitlines()[1:]]
            lens = preprocess_stand_in(models)
            g = ref.run('convert_amass.py')
        finally:
            os.chdir(here)
    save = dict(fps_names=np.asarray([r[0] for r in rows]), fps_rows=np.asarray([[float(v) for v in r[1:]] for r in rows], dtype=np.float64),
                strided_len=np.asarray(lens, dtype=np.int64), split_id=np.stack([np.asarray(s, dtype=np.int64) for s in g['split_id']]),
                joints_cam=g['joints_cam_all'])
    assert save['joints_cam'].dtype == np.float32 and save['joints_cam'].shape == (sum(lens), 17, 3) and g['vid_len_list'] == lens
    print(f"[amass] fps rows {len(rows)}, frames {sum(lens)}, clips {save['split_id'].shape}")
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
