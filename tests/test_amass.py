"""motionbert_amd/amass.py on the CPU, through tests/amasserr.MockOps: model validation, read_amass, the slice table, pack_amass end to end,
and the committed fixture tests/golden/amass.npz (the reference's own compress_amass.py and convert_amass.py: tools/mint_amass.py)."""
import json
import os

import numpy as np
import pytest
import torch

from motionbert_amd import amass as AM
from motionbert_amd.data import PackedMotion3D, _split_clips
from tests import amasserr as AE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'amass.npz')
PACK = dict(n_frames=9, data_stride=3, max_len=12)


def arrays(V=5, seed=1):
    m = AM.SMPLHModel.synthetic(V, seed)
    return dict(v_template=m.v_template, shapedirs=m.shapedirs, dmpldirs=m.dmpldirs, posedirs=m.posedirs, J_regressor=m.J_regressor,
                parents=m.parents, weights=m.weights, J_regressor_h36m=m.J_regressor_h36m)


@pytest.fixture(scope='module')
def models():
    return AE.tree_models()


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('amass_tree')
    AE.write_tree(str(root))
    return str(root)


# ------------------------------------------------------------------------------------------------ the model
def test_model_validation_errors():
    a = arrays()
    AM.SMPLHModel.from_arrays(**a)
    bad = dict(a, parents=(-1, 0, 5) + tuple(a['parents'][3:]))
    with pytest.raises(ValueError, match='forward-ordered'):
        AM.SMPLHModel.from_arrays(**bad)
    with pytest.raises(ValueError, match='52 entries'):
        AM.SMPLHModel.from_arrays(**dict(a, parents=a['parents'][:24]))
    with pytest.raises(ValueError, match='posedirs'):
        AM.SMPLHModel.from_arrays(**dict(a, posedirs=a['posedirs'][:, :, :207]))
    with pytest.raises(ValueError, match='shapedirs'):
        AM.SMPLHModel.from_arrays(**dict(a, shapedirs=a['shapedirs'][:, :, :10]))
    with pytest.raises(ValueError, match='dmpldirs'):
        AM.SMPLHModel.from_arrays(**dict(a, dmpldirs=a['dmpldirs'][:, :, :4]))
    with pytest.raises(ValueError, match='weights'):
        AM.SMPLHModel.from_arrays(**dict(a, weights=a['weights'][:, :24]))
    with pytest.raises(ValueError, match='J_regressor_h36m'):
        AM.SMPLHModel.from_arrays(**dict(a, J_regressor_h36m=torch.zeros(33, 5)))
    nan = a['v_template'].clone()
    nan[0, 0] = float('nan')
    with pytest.raises(ValueError, match='non-finite'):
        AM.SMPLHModel.from_arrays(**dict(a, v_template=nan))
    with pytest.raises(TypeError):
        AM.amass_joints(a, torch.zeros(1, 156), torch.zeros(16), ops=AE.MockOps())
    m = AM.SMPLHModel.from_arrays(**a)
    for kw, match in ((dict(poses=torch.zeros(2, 72), betas=torch.zeros(16)), 'poses'), (dict(poses=torch.zeros(2, 156), betas=torch.zeros(3, 16)), 'betas'),
                      (dict(poses=torch.zeros(2, 156), betas=torch.zeros(16), dmpls=torch.zeros(2, 4)), 'dmpls'),
                      (dict(poses=torch.zeros(2, 156), betas=torch.zeros(16), trans=torch.zeros(3, 3)), 'trans')):
        with pytest.raises(ValueError, match=match):
            AM.amass_joints(m, ops=AE.MockOps(), **kw)
    assert tuple(AM.amass_joints(m, torch.zeros(0, 156), torch.zeros(16), ops=AE.MockOps()).shape) == (0, 17, 3)


def test_model_files_round_trip(tmp_path):
    a = arrays(V=7, seed=3)
    kin = np.stack([np.asarray((2 ** 32 - 1,) + tuple(a['parents'][1:]), np.int64), np.arange(52)])
    big_sd = torch.cat([a['shapedirs'], torch.ones(7, 3, 4)], dim=2)             # the files hold more components than BodyModel uses
    np.savez(tmp_path / 'smplh.npz', v_template=a['v_template'].numpy(), shapedirs=big_sd.numpy(), posedirs=a['posedirs'].numpy(),
             J_regressor=a['J_regressor'].numpy(), weights=a['weights'].numpy(), kintree_table=kin)
    np.savez(tmp_path / 'dmpl.npz', eigvec=torch.cat([a['dmpldirs'], torch.ones(7, 3, 2)], dim=2).numpy())
    np.save(tmp_path / 'jreg.npy', a['J_regressor_h36m'].numpy())
    m = AM.SMPLHModel.from_npz(tmp_path / 'smplh.npz', tmp_path / 'dmpl.npz', tmp_path / 'jreg.npy')
    ref = AM.SMPLHModel.from_arrays(**a)
    assert m.parents == ref.parents == AM.SMPLH_PARENTS
    for k in ('Jt', 'Jd', 'pairs', 'P', 's', 'qs'):
        assert torch.equal(getattr(m, k), getattr(ref, k)), k
    np.savez(tmp_path / 'short.npz', v_template=a['v_template'].numpy())
    with pytest.raises(ValueError, match='missing arrays'):
        AM.SMPLHModel.from_npz(tmp_path / 'short.npz', tmp_path / 'dmpl.npz', tmp_path / 'jreg.npy')


def test_fold_keeps_the_live_pairs_sorted():
    m = AM.SMPLHModel.synthetic(40, 5, regressor_support=2)
    pairs = m.pairs.numpy()
    assert 1 <= m.Np <= 17 * 8 and m.P.shape == (m.Np, 3, 484) and m.pairs.dtype == torch.int32
    order = pairs[:, 0].astype(np.int64) * 52 + pairs[:, 1]
    assert (np.diff(order) > 0).all()
    live = (m.J_regressor_h36m.numpy() != 0).astype(np.float64) @ (m.weights.numpy() != 0).astype(np.float64) > 0
    assert np.array_equal(np.argwhere(live), pairs)
    assert AM.SMPLHModel.synthetic(9, 6, dense_weights=True).Np == 17 * 52


# ------------------------------------------------------------------------------------------------ compress_amass.py
def test_read_amass_strides_and_skipped_files(tree):
    seqs, skipped = AM.read_amass(tree)
    names = ['_'.join(rel.split('/')) for rel in sorted(AE.STRIDES)]
    assert [s['name'] for s in seqs] == names                               # sorted path order
    by_rel = {rel: spec for rel, *spec in AE.TREE}
    for s, rel in zip(seqs, sorted(AE.STRIDES)):
        fps, n, gender, _keep, _cols = by_rel[rel]
        stride = AE.STRIDES[rel]
        assert stride == round(fps / 60)
        raw = np.load(os.path.join(tree, *rel.split('/')))
        assert s['len_ori'] == n and s['fps'] == fps
        for k in ('poses', 'dmpls', 'trans'):
            assert np.array_equal(s[k], raw[k][::stride]), (rel, k)
        assert len(s['poses']) == len(range(0, n, stride))
    assert sorted(os.path.relpath(p, tree).replace(os.sep, '/') for p, _why in skipped) == sorted(AE.SKIPPED)
    why = {os.path.relpath(p, tree).replace(os.sep, '/'): w for p, w in skipped}
    assert 'dmpls' in why['CMU/01/no_dmpls_poses.npz'] and 'stride' in why['CMU/01/slow_poses.npz'] and '150' in why['CMU/01/smplx_poses.npz']


def test_slice_table():
    assert AM.slice_table(0, 12) == [(0, 0)]
    assert AM.slice_table(5, 12) == [(0, 5)]
    assert AM.slice_table(12, 12) == [(0, 12), (12, 12)]                    # a multiple of max_len: an empty last slice, as in the reference
    assert AM.slice_table(36, 12) == [(0, 12), (12, 24), (24, 36), (36, 36)]
    assert AM.slice_table(37, 12) == [(0, 12), (12, 24), (24, 36), (36, 37)]
    assert AM.slice_table(5834, 2916) == [(0, 2916), (2916, 5832), (5832, 5834)]


def test_gender_rules():
    assert AM.pick_gender(np.array('male')) == 'male' and AM.pick_gender(np.array('female')) == 'female'
    assert AM.pick_gender(np.array('neutral')) == 'female'
    assert AM.pick_gender(np.array(b'male')) == 'female'                    # str(b'male') = "b'male'": the reference's literal rule
    assert AM.pick_gender(np.array(b'male'), 'decode') == 'male'
    with pytest.raises(ValueError):
        AM.pick_gender('male', 'guess')


# ------------------------------------------------------------------------------------------------ the three scripts end to end
def expected_pack(tree, models, rule, seed=0):
    """pack_amass, step by step from the restatements: float32 model joints per sequence, slices as videos, the split, the gather"""
    seqs, _ = AM.read_amass(tree)
    joints, vid_list, nvid = [], [], 0
    for s in seqs:
        g = AM.pick_gender(s['gender'], rule)
        inp = dict(poses=torch.from_numpy(s['poses']).float(), betas=torch.from_numpy(s['betas'][:16]).float(),
                   dmpls=torch.from_numpy(s['dmpls'][:, :8]).float(), trans=torch.from_numpy(s['trans']).float())
        joints.append(AE.eq(models[g], inp, AE.F32, camera=True).numpy())
        for a, b in AM.slice_table(len(s['poses']), PACK['max_len']):
            if b > a:
                vid_list += [nvid] * (b - a)
                nvid += 1
    split = _split_clips(vid_list, PACK['n_frames'], PACK['data_stride'], np.random.RandomState(seed))
    return np.concatenate(joints)[np.stack(split)], nvid, len(vid_list)


@pytest.mark.parametrize('rule', ['reference', 'decode'])
def test_pack_amass_end_to_end(tree, models, tmp_path, rule):
    prefix = str(tmp_path / f'amass_{rule}')
    ops = AE.MockOps()
    meta = AM.pack_amass(tree, models, prefix, ops=ops, gender_rule=rule, chunk=4, **PACK)
    want, nvid, frames = expected_pack(tree, models, rule)
    assert ops.calls['amass_joints'] == 5                                    # one launch per sequence
    lab = np.load(prefix + '.label.npy')
    assert lab.dtype == np.float32 and lab.shape == want.shape == (meta['n'], 9, 17, 3) and np.array_equal(lab, want)
    assert json.load(open(prefix + '.json')) == meta and meta['has_input'] is False and meta['frames'] == frames and len(meta['videos']) == nvid
    # 25 + 16 + 21 + 12 + 36 frames; the 36-frame sequence is three full slices and an empty fourth, which adds no video
    assert frames == 110 and nvid == 3 + 2 + 2 + 1 + 3
    assert len(meta['skipped']) == 3
    ds = PackedMotion3D(prefix, device='cpu', synthetic=True, flip=False)
    assert len(ds) == meta['n']
    x, y = next(iter(ds.batches(4, shuffle=False)))
    assert tuple(x.shape) == (4, 9, 17, 3) and torch.equal(y, torch.from_numpy(want[:4])) and torch.equal(x[..., :2], y[..., :2]) and (x[..., 2] == 1).all()


def test_gender_rule_changes_the_bytes_typed_sequence_only(tree, models, tmp_path):
    a, b = str(tmp_path / 'ref'), str(tmp_path / 'dec')
    AM.pack_amass(tree, models, a, ops=AE.MockOps(), gender_rule='reference', **PACK)
    AM.pack_amass(tree, models, b, ops=AE.MockOps(), gender_rule='decode', **PACK)
    la, lb = np.load(a + '.label.npy'), np.load(b + '.label.npy')
    assert la.shape == lb.shape and not np.array_equal(la, lb)
    seqs, _ = AM.read_amass(tree)
    assert [AM.pick_gender(s['gender'], 'reference') for s in seqs] == ['female', 'male', 'female', 'female', 'female']
    assert [AM.pick_gender(s['gender'], 'decode') for s in seqs] == ['female', 'male', 'male', 'female', 'female']


def test_another_scale_is_applied_outside_the_launch(tree, models, tmp_path):
    a, b = str(tmp_path / 's298'), str(tmp_path / 's5')
    AM.pack_amass(tree, models, a, ops=AE.MockOps(), **PACK)
    AM.pack_amass(tree, models, b, ops=AE.MockOps(), scale=0.5, **PACK)
    la, lb = np.load(a + '.label.npy'), np.load(b + '.label.npy')
    np.testing.assert_allclose(lb * np.float32(0.298), la * np.float32(0.5), rtol=3e-7, atol=0)


# ------------------------------------------------------------------------------------------------ the reference's own scripts
def test_golden_fixture_of_the_reference_scripts(tmp_path):
    """tests/golden/amass.npz holds what the reference's compress_amass.py and convert_amass.py made of the tree of tests/amasserr.py
    (tools/mint_amass.py: its joints file came from plain_lbs_h in float64, since preprocess_amass.py needs human_body_prior)."""
    g = np.load(GOLDEN)
    root = str(tmp_path / 'tree')
    AE.write_tree(root)
    seqs, skipped = AM.read_amass(root)
    # fps.csv: (len_ori, fps, len_new) per file compress_amass.py kept, in its order; it keeps the file with 150 pose columns too, which
    # preprocess_amass.py could not evaluate: that one is in our skipped list
    rows = {str(n): tuple(r) for n, r in zip(g['fps_names'], g['fps_rows'])}
    ours = [n for n in (str(n) for n in g['fps_names']) if any(n.endswith(s['name']) for s in seqs)]
    assert len(ours) == len(seqs) and len(rows) == len(seqs) + 1
    for name, s in zip(ours, seqs):
        assert name.endswith(s['name']) and rows[name] == (s['len_ori'], s['fps'], len(s['poses']))
    extra = [n for n in rows if n not in ours]
    assert extra[0].endswith('smplx_poses.npz') and any(p.endswith('smplx_poses.npz') for p, _why in skipped)
    assert np.array_equal(g['strided_len'], [len(s['poses']) for s in seqs])
    # convert_amass.py with max_len = 2916 on these short sequences: one video per sequence; its split and camera step
    models = AE.tree_models()
    prefix = str(tmp_path / 'gold')
    meta = AM.pack_amass(root, models, prefix, ops=AE.MockOps())
    lab = np.load(prefix + '.label.npy')
    split = np.stack(_split_clips(sum(([i] * len(s['poses']) for i, s in enumerate(seqs)), []), 243, 81, np.random.RandomState(0)))
    assert np.array_equal(split, g['split_id'])
    assert lab.shape == (len(g['split_id']), 243, 17, 3) and meta['n'] == len(g['split_id'])
    want = g['joints_cam'][g['split_id']]                                    # float32 roundings of the float64 definition
    # the standing gate per sequence (the worst one), plus the two fp32 roundings of the stored reference (astype and the 0.298 product)
    gate = 0.0
    for s in seqs:
        inp = dict(poses=torch.from_numpy(s['poses']).float(), betas=torch.from_numpy(s['betas'][:16]).float(),
                   dmpls=torch.from_numpy(s['dmpls'][:, :8]).float(), trans=torch.from_numpy(s['trans']).float())
        gate = max(gate, AE.gates(models[AM.pick_gender(s['gender'])], inp, camera=True)[1])
    assert AE.stat(lab, want.astype(np.float64)) <= gate + 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the C entry point
def test_argument_errors_return_a_code():
    """validation happens before any launch, so this is safe without a GPU"""
    import ctypes as C
    import re
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 180
    with open(os.path.join(ROOT, 'include', 'mbx.h')) as f:
        assert int(re.search(r'#define MBX_AMASS_TILE (\d+)', f.read()).group(1)) == 16
    parents = (C.c_int * 52)(*AM.SMPLH_PARENTS)
    buf = C.create_string_buffer(64)                      # a non-null stand-in: no argument below passes validation
    p = C.cast(buf, C.c_void_p).value

    def call(F=4, K=17, Np=10, flags=0, Jt=p, parents=parents, P=p):
        return lib.mbx_amass_joints(p, p, 0, None, None, Jt, p, parents, p, P, p, p, Np, K, flags, p, F, None)
    for kw, word in ((dict(F=-1), b'frame count'), (dict(K=33), b'K=33'), (dict(K=0), b'K=0'), (dict(Np=17 * 52 + 1), b'Np=885'), (dict(Np=-1), b'Np=-1'),
                     (dict(flags=4), b'flag'), (dict(Jt=None), b'null model array'), (dict(P=None), b'null model array'),
                     (dict(parents=None), b'null model array')):
        assert call(**kw) != 0 and word in lib.mbx_last_error(), (kw, lib.mbx_last_error())
    bad = (C.c_int * 52)(*((-1, 0, 5) + AM.SMPLH_PARENTS[3:]))
    assert call(parents=bad) != 0 and b'forward-ordered' in lib.mbx_last_error()
    assert call(F=0) == 0                                 # a no-op
