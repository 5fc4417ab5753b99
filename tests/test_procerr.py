"""tests/procerr.py on the CPU: the model of pe_rotation (csrc/pose_solve.h) passes the gate on every family, pose form and mesh form; every
seeded corruption of procerr.CORRUPTIONS fails on the families named for it (procerr.CAUGHT_BY) -- `no_rank_one_guard`, the routine
before its guard, by NaN on the axis-aligned lines and on J = 2, and by value on the oblique line; the families keep the conditions they
owe; the model's R is a proper rotation everywhere and agrees with the eigh model of tests/mesherr.py where both are conditioned."""
import numpy as np
import pytest

from tests import mesherr as ME
from tests import procerr as P

NAMES = list(P.families())


@pytest.fixture(scope='module')
def cases():
    return P.cases()


def _H(c):
    X0, Y0 = P._centred(c.pred, c.gt)
    return np.matmul(X0.transpose(0, 2, 1), Y0) / (np.sqrt((X0 ** 2).sum((1, 2))) * np.sqrt((Y0 ** 2).sum((1, 2))))[:, None, None]


def test_the_families_keep_their_conditions(cases):
    """asserted where the families are built (procerr.cases); here: the list is the issue's, every frame has a gate, and the stated ranges"""
    want = ['conditioned', 'planar.gt', 'planar.pred', 'planar.both', 'planar.both.mirrored', 'mirrored', 'mirrored.thin', 'equal.cube',
            'equal.identity', 'similarity', 'units.metres', 'units.far', 'collapsed', 'J2.random', 'J2.axis', 'J3', 'J4', 'J64.planar',
            'line.pred.axis', 'line.pred.oblique', 'line.gt.axis', 'line.gt.oblique', 'line.both']
    want += [f'needle.{side}.{eps}' for eps in ('1e-2', '1e-4', '1e-6', '1e-8') for side in ('gt', 'pred')]
    assert list(cases) == want
    for name, c in cases.items():
        cond = c.s[:, 1] / c.s[:, 0]
        assert c.pred.shape[0] == 203 and np.isfinite(c.e2_ref).all() and bool((c.allowed > 0).all()), name
        assert np.array_equal(c.pred, c.pred.astype(np.float64).astype(np.float32)), name
        if name.split('.')[0] not in ('line', 'needle', 'J2'):
            assert cond.min() >= P.WELL, name
        if name in ('line.pred.axis', 'line.gt.axis', 'J2.axis'):
            assert bool((c.s[:, 1] == 0.0).all()), name
        if name.startswith(('line.', 'J2.')):
            assert cond.max() < P.RANK_ONE, name          # rank one: all of these frames take the guard
        if name.startswith('needle.'):
            assert cond.min() < P.WELL, name
    assert {c.pred.shape[1] for c in cases.values()} == {2, 3, 4, 8, 17, 64}
    # the needles reach from the conditioned region down to the guard's threshold and below it
    lo = min(float((cases[n].s[:, 1] / cases[n].s[:, 0]).min()) for n in NAMES if n.startswith('needle.'))
    assert lo < P.RANK_ONE


@pytest.mark.parametrize('name', NAMES)
def test_the_model_passes_the_gate(cases, name):
    c = cases[name]
    r = P.ratios(P.p_mpjpe_model(c.pred, c.gt), c.e2_ref, c.allowed)
    print(f'{name}: pose form, worst |d| / allowed {r.max():.3g} at frame {int(r.argmax())}')
    assert r.max() <= 1.0
    if c.pred.shape[1] == 17:
        for what, idx in (('17 joints', list(range(17))), ('14 joints', list(ME.H36M_17_TO_14))):
            p, g = c.pred[:, idx], c.gt[:, idx]
            ref = P.reference_mesh(p, g)
            r = P.ratios(P.rigid_align_model(p, g), ref, P.gate(p, g, ref))
            print(f'{name}: mesh form, {what}, worst |d| / allowed {r.max():.3g} at frame {int(r.argmax())}')
            assert r.max() <= 1.0


@pytest.mark.parametrize('corrupt', P.CORRUPTIONS)
def test_every_corruption_fails_on_its_families(cases, corrupt):
    for name, how in P.CAUGHT_BY[corrupt]:
        c = cases[name]
        r = P.ratios(P.p_mpjpe_model(c.pred, c.gt, corrupt), c.e2_ref, c.allowed)
        finite = np.isfinite(r)
        print(f'{corrupt} on {name}: {int((~finite).sum())} frames not finite, {int((finite & (r > 1.0)).sum())} finite frames outside the gate, '
              f'worst finite ratio {r[finite].max() if finite.any() else float("nan"):.3g}')
        if how == 'nan':
            assert not finite.all(), (corrupt, name)
        else:
            assert bool((finite & (r > 10.0)).any()), (corrupt, name)


def test_the_code_before_the_guard_is_nan_on_every_axis_aligned_frame(cases):
    for name in ('line.pred.axis', 'line.gt.axis', 'J2.axis'):
        c = cases[name]
        assert np.isnan(P.p_mpjpe_model(c.pred, c.gt, 'no_rank_one_guard')).all(), name
        assert np.isfinite(P.p_mpjpe_model(c.pred, c.gt)).all(), name


def test_every_corruption_of_the_list_is_exercised():
    assert sorted(P.CAUGHT_BY) == sorted(P.CORRUPTIONS)
    names = set(NAMES)
    assert all(n in names and how in ('nan', 'value') for v in P.CAUGHT_BY.values() for n, how in v)
    assert {('line.pred.axis', 'nan'), ('line.gt.axis', 'nan'), ('J2.axis', 'nan'), ('line.gt.oblique', 'value')} <= set(P.CAUGHT_BY['no_rank_one_guard'])


@pytest.mark.parametrize('name', NAMES)
def test_the_rotation_is_proper(cases, name):
    H = _H(cases[name])
    for scale in (1.0, 3.7e-3):                   # H as mbx_pose_errors normalises it, and on another scale as mbx_mesh_errors may
        ssum, R = P.rotation_model(H * scale)
        orth = float(np.abs(np.matmul(R, R.transpose(0, 2, 1)) - np.eye(3)).max())
        det = float(np.abs(np.linalg.det(R) - 1.0).max())
        print(f'{name} x {scale}: |R R^T - I| {orth:.2e}, |det R - 1| {det:.2e}')
        assert np.isfinite(ssum).all() and orth <= 1e-14 and det <= 1e-14


def test_the_model_agrees_with_the_eigh_model_where_both_are_conditioned(cases):
    c = cases['conditioned']
    got = P.rigid_align_model(c.pred, c.gt)
    want = np.array([ME._align_model(a, b) for a, b in zip(c.pred.astype(np.float64), c.gt.astype(np.float64))])
    rel = float(np.max(np.abs(got - want) / want))
    print(f'Jacobi model against eigh model: {rel:.3e}')
    assert rel <= 1e-13


def test_the_guard_is_shared_and_passes_nan_through(cases):
    """mesherr._align_model takes its u1 from procerr.rank_one_guard: finite on a rank-one frame, and NaN in gives NaN out"""
    c = cases['line.pred.axis']
    a, b = c.pred[0].astype(np.float64), c.gt[0].astype(np.float64)
    ref = float(np.sqrt(((ME.rigid_align64(a, b) - b) ** 2).sum(-1)).mean())
    assert abs(ME._align_model(a, b) - ref) <= P.gate(c.pred[:1], c.gt[:1], np.array([ref]))[0]
    H = _H(c)[:2].copy()
    H[1, 0, 0] = np.nan
    ssum, R = P.rotation_model(H)
    assert np.isfinite(ssum[0]) and np.isfinite(R[0]).all() and np.isnan(ssum[1]) and np.isnan(R[1]).all()
