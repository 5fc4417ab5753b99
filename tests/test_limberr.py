"""The checker of tests/test_gpu_limb_loss.py checked on the CPU (tests/limberr.py): the float64 restatement of the seven 3D losses
reproduces the fixture minted with the reference's own loss.py, the fp32 rounding model passes the gates and the bounds, seeded corruptions
of the model fail them, and the input generator keeps its promises for every seed and shape the GPU test uses.  Also what of the new
entry can be exercised without a GPU: mbx_pose_loss_full refuses bad arguments before any launch, PretrainStepFull constructs."""
import numpy as np
import pytest
import torch

from tests import limberr as LM
from tests import steperr as SE

TAGS = (('a', 3, 7), ('t1', 2, 1), ('t2', 2, 2), ('b', 2, 243))


@pytest.fixture(scope='module')
def golden():
    return np.load('tests/golden/pose_loss_full.npz')


def _close(got, want, what):
    scale = float(np.abs(want).max())
    assert float(np.abs(got - want).max()) <= 1e-12 * scale, (what, float(np.abs(got - want).max()), scale)


@pytest.mark.parametrize('tag,B,T', TAGS)
def test_restatement_reproduces_the_reference_fixture(golden, tag, B, T):
    z = golden
    lam = tuple(z['lambdas'])
    assert len(lam) == 6 and all(v != 0 for v in lam)
    pred, gt = torch.from_numpy(z[f'{tag}.pred']), torch.from_numpy(z[f'{tag}.gt'])
    assert pred.dtype == torch.float64 and tuple(pred.shape) == (B, T, 17, 3) and float(gt[:, :, 0].abs().max()) == 0.0
    assert torch.equal(pred.float().double(), pred) and torch.equal(gt.float().double(), gt), 'the fixture inputs are exact in fp32'
    losses, dpred = LM.full_ref64(pred, gt, lam, 1.0)
    for i, nm in enumerate(LM.NAMES):
        want = float(z[f'{tag}.losses'][i])
        assert abs(float(losses[i]) - want) <= 1e-12 * abs(want), (tag, nm, float(losses[i]), want)
    if T == 1:
        assert all(float(z[f'{tag}.losses'][i]) == 0.0 for i in (2, 3, 6))
    _close(dpred.numpy(), z[f'{tag}.dpred'], f'{tag}.dpred')
    frames = z[f'{tag}.dterm_frames'] if f'{tag}.dterm_frames' in z.files else np.arange(B * T)
    for i in range(7):
        p = pred.clone().requires_grad_(True)
        v = LM.terms64(p, gt)[i]
        v.backward()
        want = z[f'{tag}.dterms'][i].reshape(len(frames), 17, 3)
        if float(np.abs(want).max()) == 0.0:
            assert float(p.grad.abs().max()) == 0.0, (tag, LM.NAMES[i])
        else:
            _close(p.grad.reshape(B * T, 17, 3).numpy()[frames], want, f'{tag}.dterms[{LM.NAMES[i]}]')
    assert float(LM.ambiguous_frames(pred.float(), gt.float()).double().mean()) <= LM.MAX_AMBIGUOUS


@pytest.mark.parametrize('B,T', LM.GPU_SHAPES)
def test_input_generator_keeps_its_conditions_for_every_gpu_case(B, T):
    pred, gt = LM.limb_inputs(B, T, LM.SEEDS[(B, T)], 'cpu')
    assert pred.dtype == torch.float32 and bool(LM.conditioned(pred, gt).all())
    for x in (pred.double(), gt.double()):
        ln = LM.limb_lens(x)
        assert float(ln.min()) > LM.MIN_LIMB * float(ln.mean())
        assert float(torch.cos(LM.angles(x)).abs().max()) <= LM.MAX_COS + 1e-12
    amb = LM.ambiguous_frames(pred, gt)
    assert float(amb.double().mean()) <= LM.MAX_AMBIGUOUS, f'{int(amb.sum())} of {B * T} frames are sign-ambiguous'
    again, _ = LM.limb_inputs(B, T, LM.SEEDS[(B, T)], 'cpu')
    assert torch.equal(again, pred)


@pytest.mark.parametrize('B,T', LM.GPU_SHAPES[:-1])
@pytest.mark.parametrize('lam', (LM.LAMBDAS, LM.LAMBDAS_BASE))
def test_fp32_model_passes_the_gates_and_the_bounds_hold_and_are_small(B, T, lam):
    pred, gt = LM.limb_inputs(B, T, LM.SEEDS[(B, T)], 'cpu')
    ref_l, ref_g = LM.full_ref64(pred, gt, lam, 128.0)
    ml, mg = LM.full_model(pred, gt, lam, 128.0)
    bound = LM.full_loss_bounds(pred, gt, lam)
    for i, nm in enumerate(LM.NAMES):
        d = abs(float(ml[i].double() - ref_l[i]))
        assert d <= float(bound[i]), (nm, d, float(bound[i]))
        assert float(bound[i]) <= 1e-4 * abs(float(ref_l[i])), (nm, float(bound[i]), float(ref_l[i]))       # a bound, not an excuse
    if T == 1:
        assert all(float(ml[i]) == 0.0 and float(bound[i]) == 0.0 for i in (2, 3, 6))
    keep = ~LM.ambiguous_frames(pred, gt)
    f, p = LM.gate_frames(mg, ref_g, mg, B, T, keep)
    assert f[2] and f[1]['worst'] < 1e-5, f[3]
    assert p is not None and p[2], p
    # the base three terms are steperr's: with the new lambdas 0 the model's gradient IS pose_model's
    if lam == LM.LAMBDAS_BASE:
        assert torch.equal(mg, SE.pose_model(pred, gt, lam[0], lam[1], 128.0))


@pytest.mark.parametrize('corrupt', ('limb_table', 'var_T', 'leak', 'clamp_mask'))
def test_seeded_corruptions_fail(corrupt):
    B, T = (3, 7) if corrupt != 'clamp_mask' else (2, 1)
    lam = LM.LAMBDAS
    pred, gt = LM.limb_inputs(B, T, 31, 'cpu')
    if corrupt == 'clamp_mask':
        pred, gt = LM.plant_collinear(pred, gt, 0, 0, tilt=2.0 ** -13)
    ref_l, ref_g = LM.full_ref64(pred, gt, lam, 1.0)
    ml, mg = LM.full_model(pred, gt, lam, 1.0)
    cl, cg = LM.full_model(pred, gt, lam, 1.0, corrupt=corrupt)
    keep = ~LM.ambiguous_frames(pred, gt)
    if corrupt == 'clamp_mask':
        # the planted frame is ill-conditioned by construction: compared place by place, as the GPU test does
        assert bool(torch.isfinite(mg).all()) and float(mg[0, 0, 0].abs().max()) == 0.0 and float(ref_g[0, 0, 0].abs().max()) == 0.0
        assert float(cg[0, 0, 0].abs().max()) > 0.0
        err = lambda g: float((g[0, 0].double() - ref_g[0, 0]).norm() / ref_g[0, 0].norm())
        assert err(mg) < 2e-5 and err(cg) > 1e-2, (err(mg), err(cg))
        return
    f, p = LM.gate_frames(cg, ref_g, mg, B, T, keep)
    good, _ = LM.gate_frames(mg, ref_g, mg, B, T, keep)
    assert good[2] and not f[2], (corrupt, f[3])
    if corrupt == 'leak':
        assert not p[2], 'the clip-boundary pairs must see a term that crosses the boundary'
    if corrupt == 'var_T':
        bound = LM.full_loss_bounds(pred, gt, lam)
        assert abs(float(cl[3].double() - ref_l[3])) > float(bound[3]) and abs(float(cl[7].double() - ref_l[7])) > float(bound[7])


@pytest.fixture(scope='module')
def lib():
    import os
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_pose_loss_full_refuses_bad_arguments_before_any_launch(lib):
    # argument validation happens before any launch, so this is safe without a GPU (fake non-null addresses are never dereferenced)
    f6 = (0.5, 20.0, 0.25, 0.5, 0.125, 2.0)
    ok = 4096
    assert lib.mbx_pose_loss_full_ws(2, 243) >= (2 * 243 * 60 + 2 * 16) * 4
    for J in (16, 18):
        rc = lib.mbx_pose_loss_full(ok, ok, *f6, ok, ok, 1.0, 2, 3, J, ok, None)
        assert rc != 0 and b'17' in lib.mbx_last_error(), (J, lib.mbx_last_error())
    for args in ((None, ok, ok, ok), (ok, None, ok, ok), (ok, ok, None, ok), (ok, ok, ok, None)):
        pred, gt, losses, ws = args
        rc = lib.mbx_pose_loss_full(pred, gt, *f6, losses, ok, 1.0, 2, 3, 17, ws, None)
        assert rc != 0 and b'null' in lib.mbx_last_error(), (args, lib.mbx_last_error())
    rc = lib.mbx_pose_loss_full(ok, ok, *f6, ok, None, 1.0, 0, 3, 17, ok, None)
    assert rc != 0 and b'shape' in lib.mbx_last_error()


def test_pretrain_step_full_accepts_the_limb_and_angle_lambdas():
    from motionbert_amd.train import PretrainStep, PretrainStepFull
    net, opt = torch.nn.Linear(1, 1), None
    step = PretrainStepFull(net, opt, aug=None, mask=False, noise=False, lambda_lv=0.1)
    assert isinstance(step, PretrainStep) and step.lambdas4 == (0.1, 0.0, 0.0, 0.0) and (step.ls, step.lv) == (0.5, 20.0)
    with pytest.raises(NotImplementedError, match='PretrainStepFull'):
        PretrainStep(net, opt, aug=None, mask=False, noise=False, lambda_lv=0.1)
    with pytest.raises(ValueError):
        PretrainStepFull(net, opt, aug=None, lambda_lv=0.1)      # mask / noise still need an augmenter
