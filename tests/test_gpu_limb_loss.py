"""mbx_pose_loss_full on a real MI355X: the seven 3D losses of the reference's training step, their total and its gradient against float64
(tests/limberr.py: reference, rounding model, bounds, inputs; its own checks on the CPU: tests/test_limberr.py), bit-compatibility with
mbx_pose_loss, planted degenerate frames, and the eight-loss training step end to end, eager and captured.

Gates, neither a number read off the kernel: the eight scalars within limberr.full_loss_bounds of float64; dpred per frame and per
clip-boundary pair within 2 x the rounding model's worst unit (steperr.gate_units with its floor), over the frames that are not
sign-ambiguous (limberr.ambiguous_frames; at most 0.1 % of the frames)."""
import numpy as np
import pytest
import torch

from tests import limberr as LM
from tests.helpers import build_model, make_input
from tests.test_gpu_local_parity import nan
from tests.test_gpu_train import LITE, _aug_from_fixture, _ref_loss_2d

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = torch.float32


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def bits(t):
    return t.view(torch.int32)


def _check(tag, ops, pred, gt, lam, gs, ref_l, ref_g1, bound, keep):
    """one launch with NaN-filled outputs against the float64 reference (ref_g1: the gradient at grad_scale 1); returns (losses, dpred)"""
    B, T = pred.shape[:2]
    losses, dpred = nan(8, dtype=F32), nan(B, T, 17, 3, dtype=F32)
    ops.pose_loss_full(pred, gt, lam, losses, dpred, gs)
    torch.cuda.synchronize()
    for i, nm in enumerate(LM.NAMES):
        d = abs(float(losses[i].double() - ref_l[i]))
        print(f'{tag} {nm}: kernel {float(losses[i]):.9g} float64 {float(ref_l[i]):.9g} |d| {d:.3e} bound {float(bound[i]):.3e}')
        assert np.isfinite(float(losses[i])) and d <= float(bound[i]), f'{tag} {nm}: |{float(losses[i])} - {float(ref_l[i])}| = {d:.3e} > {float(bound[i]):.3e}'
    if T == 1:
        assert all(float(losses[i]) == 0.0 for i in (2, 3, 6)), f'{tag}: the T <= 1 terms must be exactly 0, got {losses.tolist()}'
    _, model = LM.full_model(pred, gt, lam, gs)
    f, p = LM.gate_frames(dpred, ref_g1 * gs, model, B, T, keep)
    print(f'{tag} dpred per frame: {f[3]}')
    assert f[2], f'{tag} dpred per frame: {f[3]}'
    assert p is not None
    print(f'{tag} dpred per clip-boundary pair: {p[3]}')
    assert p[2], f'{tag} dpred per clip-boundary pair: {p[3]}'
    only = nan(8, dtype=F32)
    ops.pose_loss_full(pred, gt, lam, only, None, gs)          # dpred = NULL: the same scalars, nothing else written
    torch.cuda.synchronize()
    assert torch.equal(bits(only), bits(losses)), f'{tag}: the scalars differ without dpred'
    return losses, dpred


@pytest.mark.parametrize('B,T', LM.GPU_SHAPES)
def test_pose_loss_full(ops, B, T):
    pred, gt = LM.limb_inputs(B, T, LM.SEEDS[(B, T)], DEV)
    amb = LM.ambiguous_frames(pred, gt)
    print(f'B{B}T{T}: {int(amb.sum())} of {B * T} frames sign-ambiguous')
    assert float(amb.double().mean()) <= LM.MAX_AMBIGUOUS
    keep = ~amb
    for kind, lam in (('base', LM.LAMBDAS_BASE), ('all', LM.LAMBDAS)):
        ref_l, ref_g1 = LM.full_ref64(pred, gt, lam, 1.0)
        bound = LM.full_loss_bounds(pred, gt, lam)
        for gs in (1.0, 128.0):
            losses, dpred = _check(f'{kind}.gs{gs:g}.B{B}T{T}', ops, pred, gt, lam, gs, ref_l, ref_g1, bound, keep)
            if kind == 'base':
                # the four new lambdas at zero: total and gradient are mbx_pose_loss's, bit for bit
                l4, d4 = nan(4, dtype=F32), nan(B, T, 17, 3, dtype=F32)
                ops.pose_loss(pred, gt, lam[0], lam[1], l4, d4, gs)
                torch.cuda.synchronize()
                assert torch.equal(bits(losses[[0, 1, 2, 7]]), bits(l4)), (losses.tolist(), l4.tolist())
                assert torch.equal(bits(dpred), bits(d4))
    if (B, T) == LM.GPU_SHAPES[-1]:
        runs = []
        for _ in range(3):
            losses, dpred = nan(8, dtype=F32), nan(B, T, 17, 3, dtype=F32)
            ops.pose_loss_full(pred, gt, LM.LAMBDAS, losses, dpred, 1.0)
            torch.cuda.synchronize()
            runs.append((losses, dpred))
        for l, d in runs[1:]:
            assert torch.equal(bits(l), bits(runs[0][0])) and torch.equal(bits(d), bits(runs[0][1])), 'three launches must be bit-identical'


@pytest.mark.parametrize('tag', ('a', 't1', 't2', 'b'))
def test_pose_loss_full_matches_the_reference_fixture(ops, tag):
    z = np.load('tests/golden/pose_loss_full.npz')
    lam = tuple(float(v) for v in z['lambdas'])
    pred, gt = torch.from_numpy(z[f'{tag}.pred']).float().to(DEV), torch.from_numpy(z[f'{tag}.gt']).float().to(DEV)
    amb = LM.ambiguous_frames(pred, gt)
    assert float(amb.double().mean()) <= LM.MAX_AMBIGUOUS
    ref_l, ref_g = torch.from_numpy(z[f'{tag}.losses']).to(DEV), torch.from_numpy(z[f'{tag}.dpred']).to(DEV)
    _check(f'fixture.{tag}', ops, pred, gt, lam, 1.0, ref_l, ref_g, LM.full_loss_bounds(pred, gt, lam), ~amb)


def _launch(ops, pred, gt, lam):
    B, T = pred.shape[:2]
    losses, dpred = nan(8, dtype=F32), nan(B, T, 17, 3, dtype=F32)
    ops.pose_loss_full(pred, gt, lam, losses, dpred, 1.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(dpred).all()), (losses.tolist(), int((~torch.isfinite(dpred)).sum()))
    return losses, dpred


def _frame_err(got, ref64):
    return float(((got.double() - ref64).reshape(-1, 51).norm(dim=-1) / ref64.reshape(-1, 51).norm(dim=-1).clamp_min(1e-300)).max())


def test_planted_collinear_limbs_contribute_no_gradient(ops):
    """Two exactly parallel limbs (limberr.plant_collinear): the cosine is clamped, that angle passes no gradient, and joint 0 of the planted
    frame -- which nothing else moves -- gets exactly 0.  The other joints compared with float64 place by place: the planted angle differs
    between the precisions (acos of 1 - 2^-23 and of 1 - 1e-7) but only its sign enters the gradient."""
    pred, gt = LM.limb_inputs(2, 1, 41, DEV)
    pred, gt = LM.plant_collinear(pred, gt, 0, 0)
    _, ref_g = LM.full_ref64(pred, gt, LM.LAMBDAS, 1.0)
    losses, dpred = _launch(ops, pred, gt, LM.LAMBDAS)
    assert float(ref_g[0, 0, 0].abs().max()) == 0.0 and float(dpred[0, 0, 0].abs().max()) == 0.0, dpred[0, 0, 0].tolist()
    assert _frame_err(dpred, ref_g) < 2e-5, _frame_err(dpred, ref_g)


def test_planted_pred_equal_gt_has_every_sign_zero(ops):
    """pred = gt: every sign() is 0 and the three base terms vanish; without the limb variance (which does not look at gt) the gradient is
    exactly 0, and with it the gradient is the variance term's alone."""
    _, gt = LM.limb_inputs(3, 7, 42, DEV)
    lam = (0.5, 20.0, 0.0, 0.5, 0.125, 2.0)
    losses, dpred = _launch(ops, gt.clone(), gt, lam)
    assert float(dpred.abs().max()) == 0.0 and all(float(losses[i]) == 0.0 for i in (0, 1, 2, 4, 5, 6, 7)), losses.tolist()
    assert float(losses[3]) > 0.0
    losses, dpred = _launch(ops, gt.clone(), gt, LM.LAMBDAS)
    _, ref_g = LM.full_ref64(gt.clone(), gt, LM.LAMBDAS, 1.0)
    assert _frame_err(dpred, ref_g) < 2e-5, _frame_err(dpred, ref_g)


def test_planted_zero_length_limb_stays_finite(ops):
    """joint 3 = joint 2 in one frame of pred: the limb's length is 0, d len / d v is 0 as torch.norm's backward gives, the cosine of its angle
    is 0 and its gradient passes through the norm's clamp at 1e-8 (large but finite), as autograd gives."""
    pred, gt = LM.limb_inputs(2, 3, 43, DEV)
    pred[1, 1, 3] = pred[1, 1, 2]
    _, ref_g = LM.full_ref64(pred, gt, LM.LAMBDAS, 1.0)
    assert bool(torch.isfinite(ref_g).all())
    losses, dpred = _launch(ops, pred, gt, LM.LAMBDAS)
    assert _frame_err(dpred, ref_g) < 2e-5, _frame_err(dpred, ref_g)


def test_pose_loss_full_autograd_and_refusals(ops):
    from motionbert_amd.train import pose_loss, pose_loss_full
    pred, gt = LM.limb_inputs(2, 9, 44, DEV)
    p = pred.clone().requires_grad_(True)
    total, losses = pose_loss_full(p, gt, *LM.LAMBDAS)
    (total * 2.5).backward()
    _, ref_g = LM.full_ref64(pred, gt, LM.LAMBDAS, 2.5)
    assert losses.shape == (8,) and float(total) == float(losses[7]) and _frame_err(p.grad, ref_g) < 2e-5
    q = pred.clone().requires_grad_(True)
    t4, l4 = pose_loss(q, gt)
    t8, l8 = pose_loss_full(pred.clone().requires_grad_(True), gt)      # the new lambdas default to 0: the reference's log
    assert torch.equal(l8[[0, 1, 2, 7]], l4) and float(l8[3]) > 0 and float(l8[5]) > 0
    with pytest.raises(RuntimeError, match='17'):
        pose_loss_full(torch.zeros(1, 2, 16, 3, device=DEV), torch.zeros(1, 2, 16, 3, device=DEV))


LAM_E2E = dict(lambda_scale=0.5, lambda_velocity=20.0, lambda_lv=0.25, lambda_lg=0.5, lambda_a=0.125, lambda_av=2.0)


def test_pretrain_step_full_matches_the_restated_reference_loop():
    """tests/test_gpu_train.py::test_pretrain_step_matches_the_restated_reference_loop with all seven terms weighted (train.py:177-199): a
    2D batch and a 3D batch through PretrainStepFull on model `a` and through the reference's statements restated with torch ops on model
    `b`; that test's tolerances (they bound the same backbone and optimizer, the loss adds only fp32 scalars)."""
    from motionbert_amd.train import FlatAdamW, PretrainStepFull
    a = build_model(LITE, seed=6).to(DEV)
    b = build_model(LITE, seed=6).to(DEV)
    for m in (a, b):
        m.precision = 'fp32'
    oa, ob = FlatAdamW(a, lr=5e-4, weight_decay=0.01), FlatAdamW(b, lr=5e-4, weight_decay=0.01)
    aug = _aug_from_fixture()
    step = PretrainStepFull(a, oa, aug=aug, rootrel=True, mask=True, noise=True, **LAM_E2E)
    g = torch.Generator().manual_seed(9)
    batches = [(make_input(3, 30, 17, 71).to(DEV), None, False, True),
               (make_input(2, 27, 17, 73).to(DEV), (torch.randn(2, 27, 17, 3, generator=g) * 0.3).to(DEV), True, True)]
    w7 = LM.weights7(tuple(LAM_E2E.values()))
    for k, (x, gt, has_3d, has_gt) in enumerate(batches):
        gt = x if gt is None else gt
        x0 = x.clone()
        la = step(x, gt, has_3d=has_3d, has_gt=has_gt, seed=1000 + k)
        assert torch.equal(x, x0) and la.shape == (8,)
        conf = x[..., 2:].clone()
        tgt = gt - gt[:, :, 0:1, :]
        xin = aug.augment2D(x, noise=has_gt, mask=True, seed=1000 + k)
        pred = b(xin)
        ob.zero_grad(set_to_none=True)
        if has_3d:
            t = LM.terms64(pred, tgt)
            total = sum(w * v for w, v in zip(w7, t))
            lb = torch.stack([v.detach() for v in t] + [total.detach()])
        else:
            total = _ref_loss_2d(pred, tgt, conf)
            lb = torch.stack([total.detach() * 0] * 7 + [total.detach()])
        total.backward()
        ob.step()
        print(k, la.tolist(), lb.tolist())
        assert torch.allclose(la, lb.float(), rtol=2e-5, atol=1e-7), (k, la, lb)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert float((p - q).abs().max()) <= 2 * 5e-4 * 3, n
        if p.ndim >= 2 and not n.startswith('ts_attn'):
            assert float((p - q).norm() / q.norm()) < 1e-4, (n, float((p - q).norm() / q.norm()))


def test_graphed_train_step_full_matches_eager_steps():
    """the eight-loss step replayed from one hipGraph == the same steps issued eagerly: same losses, same parameters"""
    from motionbert_amd.train import FlatAdamW, GraphedTrainStepFull, pose_loss_full
    a = build_model(LITE, seed=1).to(DEV)
    b = build_model(LITE, seed=1).to(DEV)
    oa, ob = FlatAdamW(a, lr=2e-4, weight_decay=0.01), FlatAdamW(b, lr=2e-4, weight_decay=0.01)
    batches = [(make_input(2, 27, 17, 10 + i).to(DEV), (torch.randn(2, 27, 17, 3, generator=torch.Generator().manual_seed(20 + i)) * 0.3).to(DEV))
               for i in range(3)]
    step = GraphedTrainStepFull(a, oa, *batches[0], **LAM_E2E)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters())), 'capture must not change the training state'
    for i, (x, gt) in enumerate(batches):
        la = step(x, gt)
        ob.zero_grad(set_to_none=True)
        total, lb = pose_loss_full(b(x), gt, **LAM_E2E)
        total.backward()
        ob.step()
        assert la.shape == (8,) and torch.allclose(la, lb, rtol=1e-6, atol=0), (i, la, lb)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters())), 'graph replay and eager steps must be bit-identical'
    assert float(oa.state_t[0]) == 3.0
