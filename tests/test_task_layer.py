"""The pieces the task families share (CPU only, no kernel): `hip_ops.provider`, the fused-loss autograd function of `train.py`, and the
pre-training steps that exist once."""
import pytest
import torch

from motionbert_amd import hip_ops, train


# ------------------------------------------------------------------------------------------------------------------ (a) provider
def test_provider_returns_an_injected_object_for_host_tensors():
    marker = object()
    assert hip_ops.provider(marker, 'motionbert_amd.x.f', torch.zeros(2), None) is marker
    assert hip_ops.evaluator_provider(marker, None, 'motionbert_amd.x.E') == (marker, torch.device('cpu'))


def test_provider_raises_with_the_callers_name_and_does_not_load_the_library(monkeypatch):
    monkeypatch.setattr(hip_ops, '_OPS', None)
    with pytest.raises(RuntimeError) as e:
        hip_ops.provider(None, 'motionbert_amd.mesh.MeshLoss', None, torch.zeros(2))
    assert str(e.value) == 'motionbert_amd.mesh.MeshLoss runs on the ROCm device (move the tensors first); there is no CPU path'
    with pytest.raises(RuntimeError) as e:
        hip_ops.provider(None, 'motionbert_amd.smpl.SMPLLayer', torch.zeros(2), move='the module and the tensors')
    assert str(e.value) == 'motionbert_amd.smpl.SMPLLayer runs on the ROCm device (move the module and the tensors first); there is no CPU path'
    with pytest.raises(RuntimeError) as e:
        hip_ops.evaluator_provider(None, 'cpu', 'motionbert_amd.oneshot.OneShotEvaluator')
    assert str(e.value) == 'motionbert_amd.oneshot.OneShotEvaluator runs on the ROCm device; there is no CPU path'
    with pytest.raises(RuntimeError) as e:
        hip_ops.model_device(torch.nn.Linear(2, 2), 'motionbert_amd.evaluate.evaluate')
    assert str(e.value) == 'motionbert_amd.evaluate.evaluate runs on the ROCm device (move the model first); there is no CPU path'
    assert hip_ops.peek() is None


@pytest.mark.parametrize('name, n_args', [('pose_loss', 2), ('pose_loss_full', 2), ('loss_2d_weighted', 3)])
def test_train_losses_raise_for_host_tensors(monkeypatch, name, n_args):
    monkeypatch.setattr(hip_ops, '_OPS', None)
    args = [torch.zeros(2, 3, 17, 3, requires_grad=(i == 0)) for i in range(n_args)]
    with pytest.raises(RuntimeError) as e:
        getattr(train, name)(*args)
    assert str(e.value) == f'motionbert_amd.train.{name} runs on the ROCm device (move the tensors first); there is no CPU path'
    assert hip_ops.peek() is None


# ------------------------------------------------------------------------------------------------------------------ (b) fused loss
def _stand_in(seen):
    """a plain-torch `launch`: values[k] = (k + 1) * sum(x^2), dx = d values[-1] / dx"""
    def launch(x, values, dx):
        assert x.is_contiguous() and x.dtype == torch.float32
        seen.append(dx)
        s = (x * x).sum()
        for k in range(values.numel()):
            values[k] = (k + 1) * s
        if dx is not None:
            assert dx.shape == x.shape and dx.dtype == torch.float32
            dx.copy_(2 * values.numel() * x)
    return launch


@pytest.mark.parametrize('shape, n', [((2, 3, 17, 3), 4), ((2, 3), 1)])
def test_fused_loss_gradient_is_the_stored_dx_times_the_cotangent(shape, n):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g).requires_grad_(True)
    seen = []
    total, values = train._FusedLossFn.apply(_stand_in(seen), n, n - 1, x)
    assert total.dim() == 0 and values.shape == (n,)
    assert total.requires_grad and not values.requires_grad
    assert torch.equal(total.detach(), values[n - 1]) and torch.equal(values, torch.arange(1, n + 1) * (x.detach() ** 2).sum())
    (total * 1.5).backward()
    assert len(seen) == 1 and seen[0] is not None
    assert torch.equal(x.grad, 2 * n * x.detach() * 1.5)
    assert torch.equal(seen[0], 2 * n * x.detach()), 'backward scales a copy, not the stored gradient'


@pytest.mark.parametrize('shape, n', [((2, 3, 17, 3), 4), ((2, 3), 1)])
def test_fused_loss_allocates_no_dx_without_a_gradient(shape, n):
    seen = []
    total, values = train._FusedLossFn.apply(_stand_in(seen), n, n - 1, torch.ones(*shape))
    assert seen == [None]
    assert not total.requires_grad and not values.requires_grad
    assert float(total) == n * float(torch.ones(*shape).sum())


def test_public_wrappers_keep_their_return_forms():
    class Ops:
        def pose_loss(self, pred, gt, ls, lv, losses, dpred):
            losses.copy_(torch.arange(4.0))
            dpred.fill_(1.0)

        def pose_loss_full(self, pred, gt, lambdas6, losses, dpred):
            assert len(lambdas6) == 6
            losses.copy_(torch.arange(8.0))
            dpred.fill_(2.0)

        def loss_2d_weighted(self, pred, target, conf, loss, dpred):
            loss.fill_(5.0)
            dpred.fill_(3.0)

    pred, gt = torch.zeros(2, 3, 17, 3, requires_grad=True), torch.zeros(2, 3, 17, 3)
    for fn, n, d in ((train.pose_loss, 4, 1.0), (train.pose_loss_full, 8, 2.0)):
        total, losses = fn(pred, gt, ops=Ops())
        assert float(total.detach()) == n - 1 and losses.shape == (n,) and not losses.requires_grad
        assert total.untyped_storage().data_ptr() != losses.untyped_storage().data_ptr()      # a clone of losses[n - 1]
        pred.grad = None
        (2 * total).backward()
        assert torch.equal(pred.grad, torch.full_like(pred, 2 * d))
    loss = train.loss_2d_weighted(pred, gt, gt[..., 2:], ops=Ops())
    assert loss.dim() == 0 and float(loss.detach()) == 5.0
    pred.grad = None
    loss.backward()
    assert torch.equal(pred.grad, torch.full_like(pred, 3.0))


# ------------------------------------------------------------------------------------------------------------------ (c) one body each
def test_the_full_steps_override_only_the_loss():
    assert issubclass(train.PretrainStepFull, train.PretrainStep)
    assert '__call__' not in vars(train.PretrainStepFull)
    assert train.PretrainStep.log_width == 4 and train.PretrainStepFull.log_width == 8
    assert issubclass(train.GraphedTrainStepFull, train.GraphedTrainStep)
    assert '_one' not in vars(train.GraphedTrainStepFull) and '__call__' not in vars(train.GraphedTrainStepFull)
    with pytest.raises(NotImplementedError, match='PretrainStepFull computes all seven'):
        train.PretrainStep(None, None, mask=False, noise=False, lambda_a=0.1)
    assert train.PretrainStepFull(None, None, mask=False, noise=False, lambda_a=0.1).lambdas4 == (0.0, 0.0, 0.1, 0.0)


def test_the_two_group_steps_share_one_base():
    from motionbert_amd import mesh, oneshot
    for cls in (train.ActionStep, oneshot.OneShotStep, mesh.MeshStep):
        assert issubclass(cls, train.TwoGroupStep)
        assert not {'decay', 'zero_grad', 'step'} & set(vars(cls))
