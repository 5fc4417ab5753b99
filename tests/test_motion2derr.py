"""tests/motion2derr.py on the CPU: the float64 restatement against the reference's own data sets (tests/golden/motion2d.npz, minted by
tools/mint_motion2d.py), every seeded corruption against the gates, the float32 restatement inside them, and the planted inputs."""
import os

import numpy as np
import pytest
import torch

from tests import motion2derr as ME
from tests.helpers import GOLDEN

ALL = ME.CROP | ME.ZERO | ME.FLIP | ME.NOISE | ME.MASK | ME.ROOTREL


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'motion2d.npz'))


@pytest.fixture(scope='module')
def cfg():
    return ME.AugConfig(np.load(os.path.join(GOLDEN, 'augment2d.npz')))


@pytest.fixture(scope='module')
def cases():
    """[(x, params, seed)]: the planted batch with its planted draws, and a PoseTrack-shaped batch with the kernel's own draws"""
    return [(ME.planted(), ME.PLANTED_PARAMS.clone(), 8701), (ME.motion_inputs(3, 30, 17, 8702), ME.draw_params(3, 8702), 8702)]


def test_instav_item_restatement_equals_the_reference(fixture):
    x, p = torch.from_numpy(fixture['iv.motions_2d']), torch.from_numpy(fixture['iv.params'])
    assert x.shape[1:] == (81, 17, 3) and len(x) >= 3 and set(p[:, 1].tolist()) == {0.25, 0.75}            # flipped and unflipped clips
    data, zeroed, _ = ME.item_eq(x, p, ME.CROP | ME.ZERO | ME.FLIP, 0.5, torch.float64)
    assert not bool(zeroed.any())
    assert float((data - torch.from_numpy(fixture['iv.items'])).abs().max()) < 1e-12
    assert bool((x[..., 2] == 0).any()) and bool(((data[..., 2] == 0) & (data[..., :2] == 0).all(-1)).any())     # unseen joints occur


def test_posetrack_item_and_init_restatements_equal_the_reference(fixture):
    m = torch.from_numpy(fixture['pt.motions_2d'])
    flips = torch.from_numpy(fixture['pt.flips'])
    assert m.shape == (3, 30, 17, 3) and bool(flips.any()) and not bool(flips.all())
    p = torch.stack([torch.ones(3, dtype=torch.float64), torch.where(flips, 0.25, 0.75).double()], 1)
    data, _, _ = ME.item_eq(m, p, ME.FLIP, 0.5, torch.float64)
    assert torch.equal(data, torch.from_numpy(fixture['pt.items']))
    # __init__: tracks in file order, filters, crop_scale with numpy's draws in motion order, posetrack2h36m, zeroing, root filter
    rng, kept = np.random.RandomState(0), []
    for name, content in sorted(ME.posetrack_files().items()):
        tracks = {}
        for a in content['annotations']:
            tracks.setdefault(a['track_id'], []).append(np.asarray(a['keypoints']).reshape(17, 3))
        for track in tracks.values():
            if len(track) < 30 or np.sum(np.asarray(track[:30])[:, :, 2]) <= 306:
                continue
            x = torch.from_numpy(np.asarray(track[:30]))[None]
            ratio = rng.uniform(0.25, 1, size=1)[0]
            y, _, _ = ME.item_eq(x, torch.tensor([[ratio, 1.0]], dtype=torch.float64), ME.CROP, 0.0, torch.float64)
            y = ME.posetrack_eq(y)
            y = torch.where(y[..., 2:] == 0, torch.zeros_like(y), y)
            if float(y[0, :, 0, 2].sum()) >= 30:
                kept.append(y[0])
    assert len(kept) == 3 and float((torch.stack(kept) - m).abs().max()) < 1e-12


@pytest.mark.parametrize('corrupt', ME.CORRUPTIONS)
def test_every_corruption_fails_a_gate(corrupt, cases, cfg):
    failed = False
    for x, p, seed in cases:
        got, _, _ = ME.all_eq(x, p, ALL, 0.5, seed, cfg, torch.float64, corrupt=corrupt)
        failed = failed or not ME.passes(ME.check(got, x, p, ALL, 0.5, seed, cfg))
    assert failed, corrupt


@pytest.mark.parametrize('flags', [ALL, ALL & ~ME.ROOTREL, ME.FLIP, ME.CROP | ME.ZERO | ME.MASK])
def test_float32_restatement_and_float64_pass(flags, cases, cfg):
    for x, p, seed in cases:
        for dtype in (torch.float32, torch.float64):
            got, _, _ = ME.all_eq(x, p, flags, 0.5, seed, cfg, dtype)
            res = ME.check(got, x, p, flags, 0.5, seed, cfg)
            assert ME.passes(res), (flags, dtype, res)


def test_planted_batch_holds_what_it_says(cfg):
    x, p = ME.planted(), ME.PLANTED_PARAMS
    _, zeroed, _ = ME.item_eq(x, p, ME.CROP | ME.ZERO | ME.FLIP, 0.5, torch.float64)
    assert zeroed.tolist() == [True, True, False, False, False]
    assert int((x[0, ..., 2] != 0).sum()) == 3 and int((x[1, ..., 2] != 0).sum()) >= 4
    assert float(x[2, 1, 0, 2]) == 0 and float(x[4, ..., 2].max()) > 1 and float(x[4, ..., 2].min()) < -1
    share = ME.clipped_fraction(x, p)
    assert 0 < float(share[3]) < 0.5 and float(p[3, 0]) == 0.25, share


def test_draws_are_the_hash_on_streams_16_and_17():
    p = ME.draw_params(64, 12345)
    assert float(p[:, 0].min()) >= 0.25 and float(p[:, 0].max()) <= 1.0 and 0 <= float(p[:, 1].min()) and float(p[:, 1].max()) < 1
    assert not torch.equal(p, ME.draw_params(64, 12346)) and torch.equal(p, ME.draw_params(64, 12345))
