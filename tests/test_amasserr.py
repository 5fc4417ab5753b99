"""tests/amasserr.py against itself, on the CPU: the folding identity in float64, analytic cases, the float32 model inside the gate, and
seeded corruptions that each fail it."""
import numpy as np
import pytest
import torch

from motionbert_amd import amass as AM
from tests import amasserr as AE

F64, F32 = AE.F64, AE.F32

#: (V, dense weights, regressor support, trans scale in metres): the six configurations the gate was sized on
CONFIGS = ((1, False, None, 0.0), (65, False, None, 1.0), (65, True, None, 3.0), (130, False, 3, 1.0), (300, False, None, 3.0),
           (300, True, 5, 0.0))


@pytest.fixture(scope='module')
def model65():
    return AM.SMPLHModel.synthetic(65, 8710)


@pytest.mark.parametrize('V,dense,support,tscale', CONFIGS)
def test_folding_is_an_identity_in_float64(V, dense, support, tscale):
    model = AM.SMPLHModel.synthetic(V, 8700 + V, dense_weights=dense, regressor_support=support)
    inp = AE.inputs(5, 8701 + V, max_angle=3.1, per_frame_betas=dense, trans_scale=tscale)
    ref = AE.plain(model, inp, F64)
    got = AE.eq(model, inp, F64, exact_fold=True)
    assert AE.stat(got, ref) <= 1e-12
    assert AE.stat(AE.eq(model, inp, F64, camera=True, exact_fold=True), AE.plain(model, inp, F64, camera=True)) <= 1e-12
    # the model's own fold (motionbert_amd/amass.py) is this one, rounded to fp32
    m = AE.model_dict(model, F64, exact_fold=True)
    for k in ('Jt', 'Jd', 'P', 's', 'qs'):
        assert AE.stat(getattr(model, k), m[k]) <= 2.0 ** -24, k
    if dense:
        assert model.Np == 17 * 52


@pytest.mark.parametrize('V,dense,support,tscale', CONFIGS)
def test_float32_model_is_inside_the_gate(V, dense, support, tscale):
    model = AM.SMPLHModel.synthetic(V, 8700 + V, dense_weights=dense, regressor_support=support)
    for camera in (False, True):
        inp = AE.inputs(7, 8702 + V, max_angle=3.1, trans_scale=tscale)
        ref, gate = AE.gates(model, inp, camera)
        assert AE.stat(AE.eq(model, inp, F32, camera), ref) <= gate


def test_zero_pose_is_the_regressed_shaped_template(model65):
    inp = AE.inputs(4, 8720)
    inp['poses'] = torch.zeros_like(inp['poses'])
    m = AE.model_dict(model65, F64, exact_fold=True)
    c = torch.cat([inp['betas'][None].expand(4, -1), inp['dmpls']], 1).double()
    v_shaped = m['v_template'][None] + torch.einsum('vck,fk->fvc', torch.cat([m['shapedirs'], m['dmpldirs']], 2), c)
    wsum = m['weights'].sum(1)                          # 1 up to the fp32 rounding of the stored weights
    want = torch.einsum('jv,fvc->fjc', m['J_regressor_h36m'] * wsum[None], v_shaped) + m['qs'][None, :, None] * inp['trans'].double()[:, None, :]
    assert AE.stat(AE.eq(model65, inp, F64, exact_fold=True), want) <= 1e-12
    assert AE.stat(AE.plain(model65, inp, F64), want) <= 1e-12


def test_root_rotation_rotates_about_the_root_joint(model65):
    inp = AE.inputs(3, 8721, max_angle=1.0)
    rest = dict(inp, trans=None)
    turned = dict(inp, poses=inp['poses'].clone())
    turned['poses'][:, :3] = torch.tensor([[0.3, -1.1, 0.7], [2.0, 0.1, 0.0], [0.0, 0.0, 3.0]])
    m = AE.model_dict(model65, F64, exact_fold=True)
    c = torch.cat([inp['betas'][None].expand(3, -1), inp['dmpls']], 1).double()
    J0 = m['Jt'][0][None] + torch.einsum('ck,fk->fc', m['Jd'][0], c)
    R_old, R_new = AE.rodrigues_plain(inp['poses'][:, :3].double()), AE.rodrigues_plain(turned['poses'][:, :3].double())
    qs, t = m['qs'][None, :, None], inp['trans'].double()[:, None, :]
    sw = (m['J_regressor_h36m'] @ m['weights'].sum(1))[None, :, None]      # sum_v Q[j,v] sum_k w[v,k]: qs up to the rounding of the weights
    # kp - qs trans = sw J0 + R_root (...): swapping the root rotation maps the part about J0 by R_new R_old^-1 (smplx's Rodrigues
    # form, angle = |r + 1e-8| with the axis r / angle, is orthogonal only to 1e-8: the inverse, not the transpose)
    about = AE.eq(model65, rest, F64, exact_fold=True) - sw * J0[:, None, :]
    want = torch.einsum('fcd,fjd->fjc', R_new @ torch.linalg.inv(R_old), about) + sw * J0[:, None, :] + qs * t
    assert AE.stat(AE.eq(model65, turned, F64, exact_fold=True), want) <= 1e-12


@pytest.mark.parametrize('corrupt', AE.CORRUPTIONS)
def test_corruptions_fail_the_gate(model65, corrupt):
    assert len(AE.CORRUPTIONS) >= 10
    camera = corrupt.startswith('camera')
    inp = AE.inputs(6, 8730, max_angle=2.0, trans_scale=1.0)
    ref, gate = AE.gates(model65, inp, camera)
    assert AE.stat(AE.eq(model65, inp, F32, camera), ref) <= gate
    assert AE.stat(AE.eq(model65, inp, F32, camera, corrupt=corrupt), ref) > 10 * gate


def test_mock_provider_runs_the_float32_model(model65):
    inp = AE.inputs(5, 8731)
    got = AM.amass_joints(model65, inp['poses'].numpy().astype(np.float64), inp['betas'], inp['dmpls'], inp['trans'], camera=True, ops=AE.MockOps())
    assert got.dtype == F32 and tuple(got.shape) == (5, 17, 3)
    assert torch.equal(got, AE.eq(model65, inp, F32, camera=True))
    un = AM.amass_joints(model65, inp['poses'], inp['betas'], inp['dmpls'], inp['trans'], ops=AE.MockOps())
    cam = (un.numpy()[..., [0, 2, 1]] * np.array([1, -1, 1], np.float32)) * np.float32(0.298)
    assert np.array_equal(cam, got.numpy())
