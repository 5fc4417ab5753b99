#!/usr/bin/env python
"""Mint tests/golden/mesh_gt.npz with the REFERENCE's own code (imported read-only at run time from the checkout oracle/make_golden.py names:
MOTIONBERT_REFERENCE, the way tools/mint_mesh.py imports it; lib/utils/tools.py imports `easydict`, which need not be installed: a stand-in
module is registered first).  lib/data/dataset_mesh.py itself needs `smplx` and cannot be imported; this tool calls the functions it calls.

    python tools/mint_mesh_gt.py             # write the fixture
    python tools/mint_mesh_gt.py --check     # mint again and compare every array with the committed file, bit for bit

Inputs come from the seeded makers of tests/meshgterr.py and are not stored.
  exact.{N}.{T}.{pattern}.x2d / .theta   MotionSMPL.__getitem__'s 2D input and `theta` for every clip of meshgterr.inputs(N, T, exact_seed): np.clip of
                                         the confidence, then flip_data / flip_thetas (lib/utils/utils_data.py, utils_mesh.py) where the
                                         pattern flips the clip, the pose joined with the shape; float32
  pack.{dataset}.{split}.motion2d / .pose / .shape   SMPLDataset.__init__ on the synthetic pickle of meshgterr.make_pickle: read_2d of
                                         DataReaderH36M / DataReaderMesh with the arguments of dataset_mesh.py:25-30, split_clips through
                                         get_split_id after np.random.seed(0); float32, as __getitem__'s `.float()` makes them"""
import importlib
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden                             # noqa: E402
from tests import meshgterr as GE                          # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'mesh_gt.npz')


def import_reference_mesh_data():
    """(utils_mesh, utils_data, datareader_h36m, datareader_mesh) of the reference, without shadowing by this repository's own lib/ shim"""
    REF = make_golden.REF
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.')}
    had_easydict = sys.modules.get('easydict')
    try:
        if had_easydict is None:
            stand_in = types.ModuleType('easydict')
            stand_in.EasyDict = type('EasyDict', (dict,), {})
            sys.modules['easydict'] = stand_in
        for name in ('lib', 'lib.data', 'lib.utils'):
            pkg = types.ModuleType(name)
            pkg.__path__ = [os.path.join(REF, *name.split('.'))]
            sys.modules[name] = pkg
        return tuple(importlib.import_module(n) for n in ('lib.utils.utils_mesh', 'lib.utils.utils_data', 'lib.data.datareader_h36m',
                                                          'lib.data.datareader_mesh'))
    finally:
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            sys.modules.pop(k)
        sys.modules.update(saved)
        if had_easydict is None:
            sys.modules.pop('easydict', None)


def ref_exact(UM, UD, pose, shape, m2d, flags):
    """dataset_mesh.py:66-77,91 per clip"""
    xs, ths = [], []
    for n in range(pose.shape[0]):
        motion_2d = m2d[n].copy()
        motion_2d[:, :, 2] = np.clip(motion_2d[:, :, 2], 0, 1)
        motion_smpl_pose = pose[n].reshape(-1, 24, 3)
        if flags[n]:
            motion_2d = UD.flip_data(motion_2d)
            motion_smpl_pose = UM.flip_thetas(motion_smpl_pose)
        xs.append(motion_2d)
        ths.append(np.concatenate((motion_smpl_pose.reshape(-1, 72), shape[n].reshape(-1, 10)), -1))
    return np.stack(xs).astype(np.float32), np.stack(ths).astype(np.float32)


def ref_pack(RH, RM, dataset, clip_len, data_stride, root):
    """SMPLDataset.__init__ (dataset_mesh.py:21-45) on the pickle `<root>/<dataset>.pkl`"""
    np.random.seed(0)
    if dataset == 'h36m':
        reader = RH.DataReaderH36M(n_frames=clip_len, sample_stride=1, data_stride_train=data_stride, data_stride_test=clip_len, dt_root=root,
                                   dt_file='h36m.pkl')
    elif dataset == 'coco':
        reader = RM.DataReaderMesh(n_frames=1, sample_stride=1, data_stride_train=1, data_stride_test=1, dt_root=root, dt_file='coco.pkl',
                                   res=[640, 640])
    else:
        reader = RM.DataReaderMesh(n_frames=clip_len, sample_stride=1, data_stride_train=data_stride, data_stride_test=clip_len, dt_root=root,
                                   dt_file='pw3d.pkl', res=[1920, 1920])
    ids = dict(zip(('train', 'test'), reader.get_split_id()))
    data = dict(zip(('train', 'test'), reader.read_2d()))
    out = {}
    for split in ('train', 'test'):
        dt = reader.dt_dataset[split]
        out[split] = (data[split][ids[split]], dt['smpl_pose'][ids[split]], dt['smpl_shape'][ids[split]])
    return out


def mint():
    UM, UD, RH, RM = import_reference_mesh_data()
    save = {}
    for N, T, pattern in GE.EXACT_CASES:
        pose, shape, m2d = [a.numpy() for a in GE.inputs(N, T, GE.exact_seed(N, T))]
        flags = GE.flip_pattern(N, pattern).numpy()
        x, th = ref_exact(UM, UD, pose, shape, m2d, flags)
        mine = GE.exact_targets(pose, shape, m2d, flags)
        assert x.tobytes() == mine[0].tobytes() and th.tobytes() == mine[1].tobytes(), (N, T, pattern)
        save[f'exact.{N}.{T}.{pattern}.x2d'], save[f'exact.{N}.{T}.{pattern}.theta'] = x, th
        print(f'[exact {N} x {T} {pattern}] x2d {x.shape} theta {th.shape}')
    with tempfile.TemporaryDirectory() as root:
        for dataset, clip_len, data_stride in GE.PACK_CASES:
            with open(os.path.join(root, dataset + '.pkl'), 'wb') as f:
                pickle.dump(GE.make_pickle(dataset, GE.PACK_SEED[dataset]), f)
            for split, (m, p, s) in ref_pack(RH, RM, dataset, clip_len, data_stride, root).items():
                for name, a in (('motion2d', m), ('pose', p), ('shape', s)):
                    save[f'pack.{dataset}.{split}.{name}'] = np.ascontiguousarray(a).astype(np.float32)
                print(f'[pack {dataset} {split}] motion_2d {m.shape} {m.dtype} pose {p.shape} shape {s.shape}')
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
