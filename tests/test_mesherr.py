"""tests/mesherr.py on the CPU: the restatements are the reference (tests/golden/mesh.npz, minted by tools/mint_mesh.py from the
reference's own code, pins them at 1e-12), the gates accept a float32 model of each fp32 kernel and the fp64 kernel's own algebra, and
reject every seeded corruption of mesherr.CORRUPTIONS by at least 10 x the gate."""
import math

import numpy as np
import pytest
import torch

from tests import mesherr as ME
from tests.helpers import load_golden

PIN = 1e-12
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def fx():
    return load_golden('mesh')[0]


@pytest.mark.parametrize('M', ME.ROT_M)
def test_rotation_chain_restatement_is_the_reference(fx, M):
    x6, drot, daa = ME.rot_inputs(M, ME.rot_seed(M))
    rows = fx[f'rot.{M}.rows']
    for name, got in zip(('rotmat', 'aa', 'dx6'), ME.rot_chain_grad(x6, drot, daa, F64)):
        assert ME.stat(got[rows], fx[f'rot.{M}.{name}']) <= PIN, name
    if M >= 72:
        counts = torch.bincount(ME.rot_cases(ME.rot_chain(x6.double())[0].transpose(1, 2)), minlength=4)
        assert int(counts.min()) >= 1


@pytest.mark.parametrize('F', ME.LOSS_F)
@pytest.mark.parametrize('t', (0, 1))
def test_parameter_loss_restatement_is_the_reference(fx, F, t):
    pred, gt = ME.theta_inputs(F, ME.loss_seed(F))
    ls, d = ME.param_loss_grad(pred, gt, t, ME.LAMBDAS3, F64)
    ref = fx[f'loss.{F}.t{t}.losses']
    assert float(np.max(np.abs(ls.numpy() - ref) / np.abs(ref))) <= PIN
    assert ME.stat(d[fx[f'loss.{F}.rows']], fx[f'loss.{F}.t{t}.dtheta']) <= PIN


@pytest.mark.parametrize('case', [c for c in ME.ERR_CASES if c[1] == 6890])
def test_error_restatement_is_the_reference(fx, case):
    vp, vg, kp, kg = [a.numpy() for a in ME.err_inputs(*case, ME.err_seed(case))]
    err = ME.mesh_errors64(vp, vg, kp, kg)
    assert ME.err_ratio(err, fx['err.%d.%d.rows' % case]) <= PIN / ME.GATE64
    agg = ME.aggregate(err)
    assert ME.err_ratio([agg[k] for k in ME.ERR_ROWS], fx['err.%d.%d.dict' % case]) <= PIN / ME.GATE64
    if case in ME.PLANTED:
        same, mirror, flat = ME.PLANTED[case]
        assert np.all(err[:3, same] == 0) and np.all(err[3:, same] < 1e-10)
        assert np.isnan(err[3:, flat]).all() and np.isfinite(err[:3, flat]).all()
        assert int(np.isnan(err).sum()) == 2


def test_l1_inputs_stay_off_the_kink():
    pred, gt = ME.theta_inputs(33, ME.loss_seed(33))
    d = (ME.rodrigues(pred[:, :72].reshape(-1, 3).double()) - ME.rodrigues(gt[:, :72].reshape(-1, 3).double())).abs()
    assert bool(((d == 0) | (d >= ME.KINK)).all())
    assert bool((d.reshape(33, -1)[1] == 0).all()), 'row 1 of the target is the prediction'
    zero = (pred[:, :72].reshape(-1, 3) == 0).all(1) | (gt[:, :72].reshape(-1, 3) == 0).all(1)
    assert int(zero.sum()) >= 33, 'exactly-zero joints on either side'


# ------------------------------------------------------------------------------------------------ gates against corruptions
@pytest.mark.parametrize('M', (72, 264))
def test_rotation_gates_accept_the_fp32_model_and_reject_corruptions(fx, M):
    x6, drot, daa = ME.rot_inputs(M, ME.rot_seed(M))
    ref = ME.rot_chain_grad(x6, drot, daa, F64)
    names = ('rotmat', 'aa', 'dx6')
    gates = [ME.gate32(fx[f'rot.{M}.{n}.ref32']) for n in names]
    for n, got, r, g in zip(names, ME.rot_chain_grad(x6, drot, daa, F32), ref, gates):
        s = ME.stat(got, r)
        print(f'rot M={M} {n}: fp32 model {s:.3g} gate {g:.3g}')
        assert s <= g, n
    for c in ME.ROT_CORRUPTIONS:
        worst = max(ME.stat(got, r) / g for got, r, g in zip(ME.rot_chain_grad(x6, drot, daa, F32, corrupt=c), ref, gates))
        print(f'rot M={M} {c}: worst stat / gate {worst:.3g}')
        assert worst >= 10, c


@pytest.mark.parametrize('F', (3, 33))
def test_loss_gates_accept_the_fp32_model_and_reject_corruptions(fx, F):
    pred, gt = ME.theta_inputs(F, ME.loss_seed(F))

    def ratios(t, dtype, corrupt=None):
        rl, rd = ME.param_loss_grad(pred, gt, t, ME.LAMBDAS3, F64)
        ls, d = ME.param_loss_grad(pred, gt, t, ME.LAMBDAS3, dtype, corrupt)
        gl = [ME.gate32(v) for v in fx[f'loss.{F}.t{t}.losses.ref32']]
        out = [(abs(float(a) - float(b)) / abs(float(b))) / g if math.isfinite(float(a)) else math.inf for a, b, g in zip(ls, rl, gl)]
        return out + [ME.stat(d, rd) / ME.gate32(fx[f'loss.{F}.t{t}.dtheta.ref32'])]
    for t in (0, 1):
        r = ratios(t, F32)
        print(f'loss F={F} type {t}: fp32 model / gate {r}')
        assert max(r) <= 1.0
    for c in ME.LOSS_CORRUPTIONS:
        worst = max(ratios(1, F32, c))
        print(f'loss F={F} {c}: worst / gate {worst:.3g}')
        assert worst >= 10, c


@pytest.mark.parametrize('case', ((3, 7), (37, 6890)))
def test_error_gate_accepts_the_kernel_algebra_and_rejects_corruptions(case):
    vp, vg, kp, kg = [a.numpy() for a in ME.err_inputs(*case, ME.err_seed(case))]
    ref = ME.mesh_errors64(vp, vg, kp, kg)
    r = ME.err_ratio(ME.mesh_errors_model(vp, vg, kp, kg), ref)
    print(f'errors {case}: eigen-decomposition model / gate {r:.3g}')
    assert r <= 1.0
    for c in ME.ERR_CORRUPTIONS:
        worst = ME.err_ratio(ME.mesh_errors_model(vp, vg, kp, kg, c), ref)
        print(f'errors {case} {c}: worst / gate {worst:.3g}')
        assert worst >= 10, c


def test_every_corruption_of_the_list_is_exercised():
    assert sorted(ME.CORRUPTIONS) == sorted(ME.ROT_CORRUPTIONS + ME.LOSS_CORRUPTIONS + ME.ERR_CORRUPTIONS)
