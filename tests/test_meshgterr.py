"""tests/meshgterr.py checked on the CPU: its restatements against the reference-minted fixture (tests/golden/mesh_gt.npz), the torch mock
provider through `mesh_targets` against every gate, and the seeded corruptions, each of which must fail at least one gate."""
import os

import numpy as np
import pytest
import torch

from motionbert_amd.smpl import SMPLLayer, SMPLModel
from tests import meshgterr as GE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh_gt.npz')
V = 65
MODEL = SMPLModel.synthetic(V, 3100)


@pytest.fixture(scope='module')
def fx():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def layer():
    return SMPLLayer(MODEL)


@pytest.fixture(scope='module')
def case():
    """one seeded batch (3 clips of 2 frames, alternating flips: clips 0 and 2) with its exact targets, float64 reference and gates"""
    N, T = 3, 2
    pose, shape, m2d = GE.inputs(N, T, GE.exact_seed(N, T))
    flags = GE.flip_pattern(N, 'alternating')
    x2d, theta = GE.exact_targets(pose.numpy(), shape.numpy(), m2d.numpy(), flags.numpy())
    ref64, gate = GE.gates(MODEL, theta)
    return dict(pose=pose, shape=shape, m2d=m2d, flags=flags, x2d=x2d, theta=theta, ref64=ref64, gate=gate)


@pytest.mark.parametrize('N,T,pattern', GE.EXACT_CASES)
def test_restated_flips_equal_the_reference_bit_for_bit(fx, N, T, pattern):
    pose, shape, m2d = [a.numpy() for a in GE.inputs(N, T, GE.exact_seed(N, T))]
    x2d, theta = GE.exact_targets(pose, shape, m2d, GE.flip_pattern(N, pattern).numpy())
    assert x2d.tobytes() == fx[f'exact.{N}.{T}.{pattern}.x2d'].tobytes()
    assert theta.tobytes() == fx[f'exact.{N}.{T}.{pattern}.theta'].tobytes()
    assert (x2d[..., 2] >= 0).all() and (x2d[..., 2] <= 1).all() and (m2d[..., 2] < 0).any() and (m2d[..., 2] > 1).any()
    if pattern == 'all':               # the planted zero component (joint 19, component 1) lands in joint 18 with its sign bit set
        assert theta[0, 0, 18 * 3 + 1] == 0.0 and np.signbit(theta[0, 0, 18 * 3 + 1])


def test_planted_rows_are_there():
    pose, shape, m2d = GE.inputs(3, 2, 1)
    p = pose.reshape(6, 24, 3)
    assert bool((p[:, 22:] == 0).all()) and bool((p[5] == 0).all())
    assert bool(((p[:5, 20].double().norm(dim=1) - GE.TINY).abs() < 1e-15).all())
    assert bool(((np.pi - p[:5, 21].double().norm(dim=1)).abs() <= GE.NEAR_PI + 1e-6).all())
    assert float(m2d[..., 2].min()) < 0 and float(m2d[..., 2].max()) > 1


def test_mock_provider_passes_every_gate(layer, case):
    got = GE.run_mock(layer, case['pose'], case['shape'], case['m2d'], case['flags'])
    report = {}
    assert GE.check(got, case['x2d'], case['theta'], case['flags'], case['ref64'], case['gate'], report) == []
    assert set(report) == {'kp_3d', 'verts'} and max(report.values()) <= 1.0
    assert bool((got['kp_3d'][:, :, 0] == 0).all())
    # the all-zero frame (the last one) is the rest pose: every rotation the identity, finite outputs
    assert bool(torch.isfinite(got['verts']).all()) and bool(torch.isfinite(got['kp_3d']).all())


@pytest.mark.parametrize('corrupt', GE.CORRUPTIONS)
def test_every_corruption_fails_a_gate(layer, case, corrupt):
    got = GE.run_mock(layer, case['pose'], case['shape'], case['m2d'], case['flags'], gt_corrupt=corrupt)
    failed = GE.check(got, case['x2d'], case['theta'], case['flags'], case['ref64'], case['gate'])
    print(corrupt, failed)
    assert failed, f'{corrupt} passes every gate'
    expect = {'pairs_without_sign': 'theta', 'sign_on_component_0': 'theta', 'root_before_scale': 'verts', 'root_from_joint_1': 'kp_3d',
              'verts_uncentred': 'verts', 'conf_unclipped': 'x2d', 'x_not_negated': 'x2d', 'flag_by_frame': 'theta',
              'rodrigues_without_eps': 'verts'}[corrupt]
    assert expect in failed


def test_drawn_flags_follow_the_seed():
    a, b = GE.drawn_flags(11, 4096, 0.5), GE.drawn_flags(12, 4096, 0.5)
    assert torch.equal(a, GE.drawn_flags(11, 4096, 0.5)) and not torch.equal(a, b)
    assert abs(int(a.sum()) - 2048) <= 160            # five standard deviations of the binomial
    assert int(GE.drawn_flags(11, 64, 0.0).sum()) == 0 and int(GE.drawn_flags(11, 64, 1.0).sum()) == 64


def test_gate_is_four_times_the_float32_plain_path_and_never_below_the_floor(case):
    k64, v64 = GE.body_targets(MODEL, case['theta'], torch.float64)
    k32, v32 = GE.body_targets(MODEL, case['theta'], torch.float32)
    assert case['gate']['verts'] == max(4 * GE.SE.stat(v32, v64), GE.SE.FLOOR) and case['gate']['kp_3d'] == max(4 * GE.SE.stat(k32, k64), GE.SE.FLOOR)
    assert bool((k64[:, :, 0] == 0).all())
