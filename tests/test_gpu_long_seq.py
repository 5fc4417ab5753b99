"""DSTformer with maxlen > 256 through the public API on a real MI355X.  Temporal attention over more than 256 frames runs the
streamed kernels (csrc/attention_stream.hip); every layer above them is length-agnostic.  References: the numpy fp64 oracle
(forward and hand-written backward) and, for dropout, where the oracle has no counterpart, the torch restatement of the kernel set
(MockOps) drawing the same counter-based masks.  Gates are those of tests/test_gpu_model.py."""
import numpy as np
import pytest
import torch

from motionbert_amd import model as M
from tests.helpers import build_model, make_input, oracle_cfg, rel_l2, trained_like
from tests.test_gpu_model import TOL_FP32, _mock_reference, _oracle_reference, grad_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SMALL = dict(dim_in=3, dim_out=3, dim_feat=64, dim_rep=128, depth=1, num_heads=2, mlp_ratio=2, num_joints=5, maxlen=600)
LITE1 = dict(dim_in=3, dim_out=3, dim_feat=256, dim_rep=512, depth=1, num_heads=8, mlp_ratio=4, num_joints=17, maxlen=512)
FULL1 = dict(dim_in=3, dim_out=3, dim_feat=512, dim_rep=512, depth=1, num_heads=8, mlp_ratio=2, num_joints=17, maxlen=300)
CFGS = dict(small=SMALL, lite=LITE1, full=FULL1)


def _fwd_bwd(model, x, cot):
    model.zero_grad(set_to_none=True)
    xd = x.requires_grad_(True)
    out = model(xd)
    (out * cot).sum().backward()
    return out.detach(), xd.grad, {n: p.grad.cpu().numpy() for n, p in model.named_parameters()}


@pytest.mark.parametrize('name,B,T', [('small', 1, 257), ('small', 2, 300), ('small', 1, 511), ('lite', 1, 512), ('full', 1, 300)])
def test_long_sequence_vs_numpy_oracle(name, B, T):
    cfg = CFGS[name]
    model = build_model(cfg, seed=31)
    trained_like(model, 32)
    J = cfg['num_joints']
    x = make_input(B, T, J, 33 + T)
    cot = torch.randn(B, T, J, 3, generator=torch.Generator().manual_seed(34 + T))
    ref, G, dx = _oracle_reference(cfg, model, x, cot)
    model = model.to(DEV)
    for precision in ('fp32', 'bf16x3'):
        model.precision = precision
        out, gx, grads = _fwd_bwd(model, x.to(DEV), cot.to(DEV))
        e_out, e_dx = rel_l2(out.cpu().numpy(), ref), rel_l2(gx.cpu().numpy(), dx)
        e_all, e_worst, worst = grad_errors(grads, G)
        assert max(e_out, e_dx, e_all) < TOL_FP32, (precision, e_out, e_dx, e_all)
        assert e_worst < (TOL_FP32 if precision == 'fp32' else 3e-3), (precision, worst, e_worst)


class _CountingOps:
    """The kernel provider, with a record of the sequence lengths that attn_bwd_stats ran at."""

    def __init__(self, ops):
        self._ops, self.stats_T = ops, []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def attn_bwd_stats(self, *a, **k):
        self.stats_T.append(a[9])            # (qkv, o, do, lse, dqkv, bias_f, rsum, part, B, T, ...)
        return self._ops.attn_bwd_stats(*a, **k)


@pytest.mark.parametrize('name', ['lite', 'full', 'small'])
def test_bf16_training_default_schedule(name):
    """bf16 training as it ships (LayerNorm folding, row-owner kernels, two gradient streams) at T = 300 against the fp32 MockOps
    run of the same weights, with the bounds of test_shape_sweep_fwd_bwd.  At Lite and full widths the row-owner LayerNorm-backward
    tail takes every folded pair; at dim_feat 64 (no row-owner kernels) every folded pair runs the row-dot form of the attention
    backward (mbx_attn_bwd_stats), which must then have run at this length."""
    from motionbert_amd import hip_ops
    cfg = dict(CFGS[name], depth=2, maxlen=300)
    model = build_model(cfg, seed=41)
    trained_like(model, 42)
    model = model.to(DEV)
    B, T, J = 2, 300, cfg['num_joints']
    x = make_input(B, T, J, 43).to(DEV)
    cot = torch.randn(B, T, J, 3, generator=torch.Generator().manual_seed(44)).to(DEV)
    ref, gref = _mock_reference(model, x, cot)
    spy = _CountingOps(hip_ops.get())
    model.precision = 'bf16'
    out = M.run(spy, model, x)
    (out * cot).sum().backward()
    grads = {n: p.grad.cpu().numpy() for n, p in model.named_parameters()}
    e_out = rel_l2(out.detach().cpu().numpy(), ref.cpu().numpy())
    e_all, e_worst, worst = grad_errors(grads, {n: g.cpu().numpy() for n, g in gref.items()})
    assert e_out < 5e-2 and e_all < 0.12, (e_out, e_all, worst, e_worst)
    assert all(t == T for t in spy.stats_T), spy.stats_T
    if name == 'small':
        assert len(spy.stats_T) >= 2 * cfg['depth'], spy.stats_T      # the attention sub-layer of both Blocks of every level


def test_no_grad_bf16_full_widths():
    """The no-grad bf16 path (fused row-owner / MLP kernels) at T = 300 against the oracle's forward."""
    from oracle import dstformer_oracle as O
    model = build_model(FULL1, seed=51)
    trained_like(model, 52)
    x = make_input(1, 300, 17, 53)
    P = {k: v.detach().numpy().astype(np.float64) for k, v in model.state_dict().items()}
    ref = O.forward(P, x.numpy(), oracle_cfg(FULL1))
    model = model.to(DEV).eval()
    model.precision = 'bf16'
    with torch.no_grad():
        out = model(x.to(DEV))
    assert rel_l2(out.cpu().numpy(), ref) < 5e-2


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_dropout_training_long(precision):
    """attn_drop_rate, drop_rate and drop_path_rate > 0 at T = 300 (depth 2: the second level's drop-path rate is > 0) against
    M.run(MockOps()) at the same seed, which draws the same counter-based masks."""
    cfg = dict(LITE1, depth=2, maxlen=300, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2)
    model = build_model(cfg, seed=61)
    trained_like(model, 62)
    model = model.to(DEV).train()
    model._drop_seed = 0x5EED1234
    x = make_input(1, 300, 17, 63).to(DEV)
    cot = torch.randn(1, 300, 17, 3, generator=torch.Generator().manual_seed(64)).to(DEV)
    ref, gref = _mock_reference(model, x, cot)
    model.precision = precision
    out, _, grads = _fwd_bwd(model, x, cot)
    e_out = rel_l2(out.cpu().numpy(), ref.cpu().numpy())
    e_all, e_worst, worst = grad_errors(grads, {n: g.cpu().numpy() for n, g in gref.items()})
    assert e_out < TOL_FP32 and e_all < TOL_FP32, (precision, e_out, e_all, worst, e_worst)
