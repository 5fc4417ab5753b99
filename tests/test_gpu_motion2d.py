"""mbx_motion2d_input on a real MI355X (csrc/motion2d.hip): (A) against the float64 restatement of tests/motion2derr.py and the reference's
own items (tests/golden/motion2d.npz), per sample within the gate; (B) bit equality with the composition of the entry points that existed
before it; (C) the draws; (D) one pre-training step through the one-launch front end against PretrainStep.__call__ on the composed batch.
The measured shares go to motion2d_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import os
import re
import time

import numpy as np
import pytest
import torch

from tests import motion2derr as ME
from tests.helpers import GOLDEN, build_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
ALL = ME.CROP | ME.ZERO | ME.FLIP | ME.NOISE | ME.MASK | ME.ROOTREL
WANT = ME.OUTPUTS
LITE = dict(dim_in=3, dim_out=3, dim_feat=256, dim_rep=512, depth=1, num_heads=8, mlp_ratio=4, num_joints=17, maxlen=243)


def _resident():
    with open(os.path.join(ROOT, 'include', 'mbx.h')) as f:
        return int(re.search(r'#define MBX_MOTION2D_RESIDENT (\d+)', f.read()).group(1))


T_RES = _resident() // 17          # the largest T that stays resident at J = 17
# (N, T, J): PoseTrack's shape, InstaVariety's, one frame, the largest J (no flip: the left / right table has 17 joints), and the two sides
# of the resident bound: the largest T J that stays in LDS and the next T above it (the path that reads the sample twice)
SHAPES = ((3, 30, 17), (2, 81, 17), (2, 1, 17), (2, 5, 32), (2, T_RES, 17), (2, T_RES + 1, 17))


def _inputs(shape, seed):
    """x and params: the ratios the kernel would draw from `seed`, and every other clip flipped (the first one is)"""
    N, T, J = shape
    p = ME.draw_params(N, seed)
    p[:, 1] = torch.where(torch.arange(N) % 2 == 0, 0.25, 0.75)
    return ME.motion_inputs(N, T, J, seed), p


def _seed(shape):
    return 8100 + sum(int(v) * w for v, w in zip(shape, (1, 17, 289))) % 9973


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = os.environ.get('MBX_REPORT_DIR') or os.path.join(ROOT, 'reports')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'motion2d_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, resident_joints=_resident(), cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'motion2d_parity.txt'), 'w') as f:
        f.write('mbx_motion2d_input against float64: worst error / gate per case and output (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:28s} ' + ' '.join(f'{o}={v:.4f}' if isinstance(v, float) else f'{o}={v}' for o, v in sorted(REPORT[k].items())) + '\n')


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'motion2d.npz'))


@pytest.fixture(scope='module')
def cfg():
    return ME.AugConfig(np.load(os.path.join(GOLDEN, 'augment2d.npz')))


def _run(x, cfg, flags, seed, params=None, want=WANT, flip_prob=0.5, scale_range=ME.SCALE_RANGE, return_params=False):
    from motionbert_amd.augment import motion2d_input
    noise, mask = bool(flags & ME.NOISE), bool(flags & ME.MASK)
    return motion2d_input(x.to(DEV), scale_range=scale_range if flags & ME.CROP else None, zero_unseen=bool(flags & ME.ZERO),
                          flip_prob=flip_prob if flags & ME.FLIP else 0.0, aug=cfg.augmenter() if (noise or mask) else None, noise=noise, mask=mask,
                          rootrel=bool(flags & ME.ROOTREL), want=want, seed=seed, params=None if params is None else params.to(DEV),
                          return_params=return_params)


def _flags(J, flags=ALL):
    """(the flip's table and the fixture's noise statistics have 17 joints)"""
    return flags if J == 17 else flags & ~(ME.FLIP | ME.NOISE)


def _compose(x, params, cfg, flags, seed, flip_prob=0.5):
    """the same result on the entry points that existed before the kernel: a crop-only action_input on x[:, None], where, flip_batch, the
    root subtraction, Augmenter2D.augment2D"""
    from motionbert_amd.augment import action_input
    from motionbert_amd.data import flip_batch
    x, params = x.to(DEV), params.to(DEV)
    d = x
    if flags & ME.CROP:
        p9 = torch.zeros(len(x), 9, device=DEV)
        p9[:, 8] = params[:, 0]
        d = action_input(x[:, None], random_move=False, scale_range=ME.SCALE_RANGE, params=p9)[:, 0]
    if flags & ME.ZERO:
        d = torch.where(d[..., 2:] == 0, torch.zeros_like(d), d)
    if flags & ME.FLIP:
        d = flip_batch(d, params[:, 1] < flip_prob)
    if flags & ME.ROOTREL:
        gt = d - d[:, :, 0:1, :]
    else:
        gt = d.clone()
        gt[..., 2] = gt[..., 2] - gt[:, 0:1, 0:1, 2]
    x_aug = cfg.augmenter().augment2D(d, noise=bool(flags & ME.NOISE), mask=bool(flags & ME.MASK), seed=seed)
    return dict(data=d, gt=gt, conf=d[..., 2:], x_aug=x_aug)


# ------------------------------------------------------------------------------------------------ A: float64 and the fixture
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_a_within_the_gate_of_float64(shape, cfg):
    N, T, J = shape
    seed = _seed(shape)
    x, p = _inputs(shape, seed)
    for flags in (_flags(J), _flags(J, ALL & ~ME.ROOTREL)):
        got, used = _run(x, cfg, flags, seed, params=p, return_params=True)
        res = ME.check(got, x, p, flags, 0.5, seed, cfg)
        REPORT['A.%dx%dx%d.flags%d' % (N, T, J, flags)] = res
        print(shape, flags, res)
        assert torch.equal(used.cpu(), p)
        assert ME.passes(res), (shape, flags, res)


def test_a_planted_batch(cfg):
    x, p = ME.planted(), ME.PLANTED_PARAMS
    got = _run(x, cfg, ALL, 8701, params=p)
    res = ME.check(got, x, p, ALL, 0.5, 8701, cfg)
    REPORT['A.planted'] = res
    print(res)
    assert ME.passes(res), res
    assert all(bool((got[k][:2] == 0).all()) for k in ('data', 'gt', 'conf'))                        # three valid joints; coincident joints
    assert bool((got['data'][2:] != 0).any()) and float(got['conf'].abs().max()) == 1.0              # confidences of +-1.5 clipped
    assert bool((got['data'][2, 1, 0] == 0).all())                                                   # the unseen root of sample 2 (not flipped: joint 0)


def test_a_reference_items(fixture, cfg):
    x, p = torch.from_numpy(fixture['iv.motions_2d']), torch.from_numpy(fixture['iv.params']).float()
    flags = ME.CROP | ME.ZERO | ME.FLIP
    got = _run(x, cfg, flags, 1, params=p, want=('data',))['data'].cpu()
    _, g, _ = ME.gates(x, p, flags, 0.5, 1, cfg)
    err = (got.double() - torch.from_numpy(fixture['iv.items'])).abs().reshape(len(x), -1).amax(1)
    REPORT['A.instav_items'] = dict(data=float((err / g['data']).max()))
    print(REPORT['A.instav_items'])
    assert bool((err <= g['data']).all()), (err, g['data'])
    m = torch.from_numpy(fixture['pt.motions_2d'].astype(np.float32))
    p = torch.stack([torch.ones(len(m)), torch.where(torch.from_numpy(fixture['pt.flips']), 0.25, 0.75)], 1)
    got = _run(m, cfg, ME.FLIP, 1, params=p, want=('data',))['data'].cpu()
    assert torch.equal(got, torch.from_numpy(fixture['pt.items']).float())                           # PoseTrack's item: the flip alone, exact


# ------------------------------------------------------------------------------------------------ B: the composition of what existed
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_b_bit_equal_to_the_composition(shape, cfg):
    N, T, J = shape
    seed = _seed(shape) + 1
    x, p = _inputs(shape, seed)
    for aug_bits in (0, ME.NOISE, ME.MASK, ME.NOISE | ME.MASK):
        for rootrel in (ME.ROOTREL, 0):
            flags = _flags(J, ME.CROP | ME.ZERO | ME.FLIP | aug_bits | rootrel)
            got, ref = _run(x, cfg, flags, seed, params=p), _compose(x, p, cfg, flags, seed)
            for k in WANT:
                assert torch.equal(got[k], ref[k]), (shape, flags, k, float((got[k] - ref[k]).abs().max()))


def test_b_planted_batch_bit_equal(cfg):
    x, p = ME.planted(), ME.PLANTED_PARAMS
    got, ref = _run(x, cfg, ALL, 77, params=p), _compose(x, p, cfg, ALL, 77)
    for k in WANT:
        assert torch.equal(got[k], ref[k]), k


# ------------------------------------------------------------------------------------------------ C: the draws
def test_c_draws(cfg):
    x = ME.motion_inputs(6, 30, 17, 8801)
    got, used = _run(x, cfg, ALL, 4242, return_params=True)
    want = ME.draw_params(6, 4242)
    assert torch.equal(used.cpu(), want)                                                             # the hash on streams 16 / 17
    assert float(used[:, 0].min()) >= 0.25 and float(used[:, 0].max()) <= 1.0 and 0 <= float(used[:, 1].min()) and float(used[:, 1].max()) < 1
    again, used2 = _run(x, cfg, ALL, 4242, return_params=True)
    assert torch.equal(used, used2) and all(torch.equal(got[k], again[k]) for k in WANT)
    # params_in = params_out: the same memory on both sides
    from motionbert_amd import hip_ops
    from motionbert_amd.augment import M2D_CROP, M2D_ZERO, M2D_FLIP, M2D_ROOTREL
    xd, inout, data = x.to(DEV), used.clone(), torch.empty_like(x, device=DEV)
    hip_ops.get().motion2d_input(xd, data, None, None, None, inout, inout, ME.SCALE_RANGE, 0.5, None, 0.06, 0.002, (0, 0, 0, 0), 0.0, 0.0,
                                 M2D_CROP | M2D_ZERO | M2D_FLIP | M2D_ROOTREL, 4242)
    assert torch.equal(inout, used) and torch.equal(data, got['data'])
    _, other = _run(x, cfg, ALL, 4243, return_params=True)
    assert not torch.equal(other, used)
    flipped = used[:, 1] < 0.5
    assert bool(flipped.any()) and not bool(flipped.all())
    never, always = _run(x, cfg, ALL, 4242, flip_prob=0.0, want=('data',))['data'], _run(x, cfg, ALL, 4242, flip_prob=1.0, want=('data',))['data']
    from motionbert_amd.data import flip_batch
    everyone = torch.ones(6, dtype=torch.bool, device=DEV)
    assert torch.equal(flip_batch(never, everyone), always) and torch.equal(flip_batch(never, flipped), got['data'])
    assert not torch.equal(never, always)
    for k in WANT:                                                                                   # each output alone: the bits it has among all four
        assert torch.equal(_run(x, cfg, ALL, 4242, want=(k,))[k], got[k]), k


def test_c_aliasing_is_refused(cfg):
    from motionbert_amd import hip_ops
    x = ME.motion_inputs(2, 5, 17, 3).to(DEV)
    with pytest.raises(RuntimeError, match='overlaps'):
        hip_ops.get().motion2d_input(x, x, None, None, None, None, None, ME.SCALE_RANGE, 0.5, None, 0.06, 0.002, (0, 0, 0, 0), 0.0, 0.0, 7, 0)


# ------------------------------------------------------------------------------------------------ D: end to end
def test_d_front_end_step_equals_call_on_the_composed_batch(fixture, cfg, tmp_path):
    from motionbert_amd.data import PackedAction, PackedMotion2D
    from motionbert_amd.train import FlatAdamW, PretrainStep
    sets = {}
    for kind, key in (('posetrack', 'pt.motions_2d'), ('instav', 'iv.motions_2d')):
        clips = fixture[key].astype(np.float32)
        np.save(str(tmp_path / (kind + '.motion2d.npy')), clips)
        with open(tmp_path / (kind + '.json'), 'w') as f:
            json.dump(dict(n=len(clips), kind=kind), f)
        sets[kind] = (PackedMotion2D(str(tmp_path / kind), device=DEV, kind=kind), torch.from_numpy(clips))
    nets, steps = [], []
    for _ in range(2):
        m = build_model(LITE, seed=4).to(DEV)
        nets.append(m)
        steps.append(PretrainStep(m, FlatAdamW(m, lr=5e-4, weight_decay=0.01), aug=cfg.augmenter(), rootrel=True, mask=True, noise=True))
    for kind, has_gt in (('posetrack', True), ('instav', False)):
        ds, clips = sets[kind]
        (x_aug, gt, conf), = list(ds.batches(8, shuffle=False, epoch=2, seed=5, front=steps[0], has_gt=has_gt))
        la = steps[0].step_prepared(x_aug, gt, conf, has_3d=False)
        s = PackedAction.batch_seed(5, 2, 0, 0)
        flags = (ME.CROP | ME.ZERO | ME.FLIP) if kind == 'instav' else ME.FLIP
        batch = _compose(clips, ME.draw_params(len(clips), s), cfg, flags, s)['data']
        lb = steps[1](batch, batch, has_3d=False, has_gt=has_gt, seed=s)
        assert torch.equal(la, lb) and float(la[3]) > 0, (kind, la, lb)
    for (n, p), q in zip(nets[0].named_parameters(), nets[1].parameters()):
        assert torch.equal(p, q), n
