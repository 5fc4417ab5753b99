"""The one-shot kernels on a real MI355X (csrc/oneshot.hip): mbx_supcon_loss and mbx_nn_cosine against float64 (tests/supconerr.py:
restatements, bounds, inputs; its own checks on the CPU: tests/test_supconerr.py), the embedding head, OneShotStep and OneShotEvaluator.

Gates, none of them a number read off a kernel: the loss within supconerr.supcon_bounds' loss bound of float64, every anchor row of dfeat
within its row bound (max-norm); a predicted exemplar equal to float64's wherever the float64 top-two margin exceeds twice
supconerr.nn_sim_bound, and for every row within that bound of the float64 maximum.  The worst ratios go to oneshot_parity.json / .txt in
the directory MBX_REPORT_DIR names (default reports/)."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from tests import supconerr as SC
from tests.helpers import GOLDEN, build_model, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, I32 = torch.float32, torch.int32
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'oneshot_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'oneshot_parity.txt'), 'w') as f:
        f.write('one-shot kernels against float64: worst error / derived bound per case (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:56s} ' + '  '.join(f'{n} {v:.4g}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def nan(*shape, dtype=F32):
    return torch.full(shape, math.nan, dtype=dtype, device=DEV)


def bits(t):
    return t.view(torch.int32)


def launch(ops, feat, lab, taus, normalize, gs=1.0, grad=True):
    loss = nan(1)
    d = nan(*feat.shape) if grad else None
    ops.supcon_loss(feat, lab.to(I32), taus[0], taus[1], normalize, loss, d, gs)
    torch.cuda.synchronize()
    return loss, d


def check(tag, ops, feat, lab, taus, normalize, gs=1.0):
    """one launch with NaN-filled outputs against float64, printed before it is asserted; returns (loss, dfeat)"""
    rl, rd = SC.supcon_ref64(feat, lab, *taus, normalize, gs)
    bl, br = SC.supcon_bounds(feat, lab, *taus, normalize, gs)
    loss, d = launch(ops, feat, lab, taus, normalize, gs)
    rloss, rrow, ok = SC.supcon_gate(loss[0], d, rl, rd, bl, br)
    print(f'{tag}: loss kernel {float(loss):.9g} float64 {float(rl):.9g} bound {float(bl):.3e} ratio {rloss:.4f}; worst row ratio {rrow:.4f}')
    REPORT[tag] = dict(loss_ratio=rloss, row_ratio=rrow)
    assert ok, f'{tag}: loss ratio {rloss:.4g}, worst row ratio {rrow:.4g} (kernel loss {float(loss)}, float64 {float(rl)})'
    return loss, d


# ------------------------------------------------------------------------------------------------ mbx_supcon_loss
@pytest.mark.parametrize('shape', SC.GPU_SHAPES)
def test_supcon_loss_against_float64(ops, shape):
    feat, lab = SC.supcon_inputs(*shape, SC.case_seed(shape), DEV)
    for taus in SC.TAUS:
        for normalize in (False, True):
            tag = 'supcon.%d.%d.%d.tau%g.n%d' % (shape + (taus[0], normalize))
            loss, d = check(tag, ops, feat, lab, taus, normalize)
            only, _ = launch(ops, feat, lab, taus, normalize, grad=False)            # dfeat = NULL: the same loss bits
            assert torch.equal(bits(only), bits(loss)), f'{tag}: the loss differs without dfeat'
            again, d2 = launch(ops, feat, lab, taus, normalize)
            assert torch.equal(bits(again), bits(loss)) and torch.equal(bits(d2), bits(d)), f'{tag}: two calls must be bit-identical'
    check('supcon.%d.%d.%d.gs' % shape, ops, feat, lab, SC.TAUS[0], True, gs=-3.0)
    check('supcon.%d.%d.%d.gs.plain' % shape, ops, feat, lab, SC.TAUS[0], False, gs=128.0)


@pytest.mark.parametrize('shape', SC.GPU_SHAPES)
def test_supcon_loss_matches_the_reference_fixture(ops, shape):
    """the kernel against the reference's own loss_supcon.py (tests/golden/supcon.npz), within the same bounds"""
    z = np.load(os.path.join(GOLDEN, 'supcon.npz'))
    bsz, nv, D = shape
    tag = 'sc.%d.%d.%d' % shape
    feat, lab = SC.supcon_inputs(*shape, SC.case_seed(shape), DEV)
    rows = SC.fixture_rows(bsz * nv, D).to(DEV)
    for n in (0, 1):
        bl, br = SC.supcon_bounds(feat, lab, *SC.FIXTURE_TAUS, bool(n))
        loss, d = launch(ops, feat, lab, SC.FIXTURE_TAUS, bool(n))
        dl = abs(float(loss) - float(z[f'{tag}.n{n}.loss']))
        print(f'{tag}.n{n}: loss {float(loss):.9g} fixture {float(z[f"{tag}.n{n}.loss"]):.9g} |d| {dl:.3e} bound {float(bl):.3e}')
        assert dl <= float(bl)
        err = (d.reshape(bsz * nv, D)[rows].double() - torch.from_numpy(z[f'{tag}.n{n}.dfeat']).to(DEV)).abs().max(1).values
        assert bool((err <= br[rows]).all()), (n, float((err / br[rows]).max()))


@pytest.mark.parametrize('shape', ((3, 2, 5), (17, 2, 129), (32, 1, 2048)))
def test_supcon_loss_normalizes_rows_of_any_norm(ops, shape):
    """rows whose norms span 1e-3 .. 1e3: the loss is the unit rows', the gradient comes back per row at its own scale"""
    feat, lab = SC.supcon_inputs(*shape, SC.case_seed(shape) + 1, DEV, spread=(1e-3, 1e3))
    norms = feat.reshape(-1, shape[2]).norm(dim=-1)
    assert float(norms.max() / norms.min()) > 1e5
    loss, _ = check('supcon.%d.%d.%d.spread' % shape, ops, feat, lab, SC.TAUS[0], True)
    unit, _ = SC.supcon_inputs(*shape, SC.case_seed(shape) + 1, DEV)
    assert abs(float(loss) - float(SC.supcon_ref64(unit, lab, *SC.TAUS[0], True)[0])) <= 2 * float(SC.supcon_bounds(unit, lab, *SC.TAUS[0], True)[0])


def test_supcon_loss_with_an_all_zero_row(ops):
    feat, lab = SC.supcon_inputs(17, 2, 129, 31, DEV)
    feat[5, 1] = 0
    for normalize in (False, True):
        loss, d = check(f'supcon.zero_row.n{int(normalize)}', ops, feat, lab, SC.TAUS[0], normalize)
        assert bool(torch.isfinite(d).all())
    assert float(d[5, 1].abs().max()) > 1e8, 'under the clamp of F.normalize the row gets g / 1e-12'


def test_supcon_loss_is_nan_when_an_anchor_has_no_positive(ops):
    feat, _ = SC.supcon_inputs(32, 1, 2048, 32, DEV)
    lab = torch.arange(32, device=DEV) // 2
    lab[31] = 99                                             # rows 30 and 31 are alone now
    for normalize in (False, True):
        loss, d = launch(ops, feat, lab, SC.TAUS[0], normalize)
        assert math.isnan(float(loss)) and bool(torch.isnan(d).all()), (float(loss), int(torch.isnan(d).sum()), d.numel())
        rl, rd = SC.supcon_ref64(feat, lab, *SC.TAUS[0], normalize)
        assert math.isnan(float(rl)) and bool(torch.isnan(rd).all())
    from motionbert_amd.oneshot import supcon_loss
    assert math.isnan(float(supcon_loss(feat)))              # SimCLR labels with one view


def test_supcon_loss_autograd_and_refusals(ops):
    from motionbert_amd.oneshot import supcon_loss
    feat, lab = SC.supcon_inputs(17, 2, 129, 33, DEV)
    a = feat.clone().requires_grad_(True)
    loss = supcon_loss(a, lab, temperature=0.1, normalize=True)
    (loss * 2.5).backward()
    rl, rd = SC.supcon_ref64(feat, lab, 0.1, 0.07, True, 2.5)
    bl, br = SC.supcon_bounds(feat, lab, 0.1, 0.07, True, 2.5)
    rloss, rrow, _ = SC.supcon_gate(loss.detach(), a.grad, rl, rd, bl, br)
    assert loss.is_cuda and rloss <= 1.0 and rrow <= 1.0 + 1e-6, (rloss, rrow)      # d * dloss: one more rounding than grad_scale inside
    with pytest.raises(RuntimeError, match='anchors'):
        ops.supcon_loss(torch.zeros(65, 2, 8, device=DEV), torch.zeros(65, dtype=I32, device=DEV), 0.1, 0.07, False, nan(1), None)
    with pytest.raises(RuntimeError, match='no CPU path'):
        supcon_loss(feat.cpu(), lab.cpu())


# ------------------------------------------------------------------------------------------------ mbx_nn_cosine
def run_nn(ops, a, al, t, tl, hits=None):
    N = t.shape[0]
    pred = torch.full((N,), -7, dtype=I32, device=DEV)
    best = nan(N)
    hits = torch.zeros(1, dtype=torch.int64, device=DEV) if hits is None else hits
    ops.nn_cosine(a, al, t, tl, pred, best, hits)
    torch.cuda.synchronize()
    return pred, best, hits


@pytest.mark.parametrize('shape', SC.NN_SHAPES)
def test_nn_cosine_against_float64(ops, shape):
    M, N, D = shape
    a, al, t, tl = SC.nn_inputs(M, N, D, SC.case_seed(shape), SC.NN_NOISE[shape], DEV)
    idx, sims, pred64, acc = SC.nn_ref64(a, al, t, tl)
    bound = SC.nn_sim_bound(a, t)
    margin, unit = SC.nn_margin(sims, bound)
    under = float((~unit).double().mean())
    print(f'nn {shape}: float64 accuracy {acc:.4f}, largest bound {float(bound.max()):.3e}, rows under the margin {under:.4f}')
    lo, hi = SC.NN_ACCURACY[shape]
    assert lo <= acc <= hi, acc                              # conditions on the inputs: the reference alone
    assert under <= SC.MAX_UNDER_MARGIN
    pred, best, hits = run_nn(ops, a, al, t, tl)
    chosen = ((pred.long() - 100) // 3)
    assert bool(((pred.long() - 100) % 3 == 0).all()) and int(chosen.min()) >= 0 and int(chosen.max()) < M, 'a label of the exemplar table'
    assert torch.equal(pred[unit], pred64[unit]), f'{int((pred[unit] != pred64[unit]).sum())} rows with a clear float64 margin differ'
    cols = torch.arange(N, device=DEV)
    s_chosen, b_chosen = sims[chosen, cols], bound[chosen, cols]
    short = (sims.max(0).values - s_chosen) / bound.max(0).values.clamp_min(1e-300)
    sim_err = (best.double() - s_chosen).abs() / b_chosen.clamp_min(1e-300)
    print(f'nn {shape}: worst (float64 max - float64 sim of the chosen) / bound {float(short.max()):.4f}, worst |best_sim - float64| / bound {float(sim_err.max()):.4f}')
    REPORT['nn.%d.%d.%d' % shape] = dict(chosen_short=float(short.max()), best_sim_ratio=float(sim_err.max()), under_margin=under, accuracy64=acc)
    # Two bounds, not one, and not a loosened gate: the kernel chose c because its fp32 sim(c) >= its fp32 sim(m), m the float64 argmax; the
    # fp32 sim(c) is at most one bound above the float64 sim(c) and the fp32 sim(m) at most one bound below the float64 sim(m), so
    # float64 sim(m) - float64 sim(c) <= bound(c) + bound(m) <= 2 x the column's largest bound is all a correct kernel guarantees.
    assert float(short.max()) <= 2.0, 'the chosen exemplar is within the bounds of the float64 maximum'
    assert float(sim_err.max()) <= 1.0
    n_hit = int((pred == tl).sum())
    assert int(hits) == n_hit
    p2, b2, hits = run_nn(ops, a, al, t, tl, hits)           # the counter accumulates; the same bits again
    assert int(hits) == 2 * n_hit and torch.equal(p2, pred) and torch.equal(bits(b2), bits(best))
    none = torch.full((N,), -7, dtype=I32, device=DEV)
    ops.nn_cosine(a, al, t, None, none, None, None)          # no labels, no best_sim, no counter
    torch.cuda.synchronize()
    assert torch.equal(none, pred)


def test_nn_cosine_planted_ties_zero_rows_and_nan(ops):
    a, al, t, tl = SC.nn_inputs(40, 70, 129, 51, 1.0, DEV)
    a[37] = a[3]                                             # bit-identical duplicates, in two different exemplar tiles: the lower index wins
    a[12] = a[5]
    t[0], t[1], t[2] = a[3], a[5], a[37]
    t[9] = 0                                                 # a zero test row: every similarity is 0, index 0
    a[20] = 0                                                # a zero exemplar: similarity 0, never NaN
    pred, best, _ = run_nn(ops, a, al, t, tl)
    idx, sims, pred64, _ = SC.nn_ref64(a, al, t, tl)
    assert pred[:3].tolist() == [int(al[3]), int(al[5]), int(al[3])] and pred[9] == al[0] and float(best[9]) == 0.0
    assert torch.equal(pred[:10], pred64[:10]) and bool(torch.isfinite(best).all())
    assert abs(float(best[0]) - 1.0) < 1e-5
    # NaN counts as maximal, the first NaN wins (torch.argmax); a NaN test row makes every similarity NaN: index 0
    a[35, 7] = math.nan
    a[33, 0] = math.nan
    t[11, 5] = math.nan
    pred, best, _ = run_nn(ops, a, al, t, tl)
    idx, _, pred64, _ = SC.nn_ref64(a, al, t, tl)
    assert bool((idx == 33).sum() == 69) and int(idx[11]) == 0
    assert torch.equal(pred, pred64) and bool(torch.isnan(best).all())
    # N = 0 is a no-op
    ops.nn_cosine(a, al, t[:0], tl[:0], torch.empty(0, dtype=I32, device=DEV), None, torch.zeros(1, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------ head, step, evaluator
CFG = dict(dim_in=3, dim_out=3, dim_feat=128, dim_rep=128, depth=2, num_heads=4, mlp_ratio=4, num_joints=17, maxlen=243)
HIDDEN = 256


def embed_net(seed=91):
    from motionbert_amd.action import ActionNet
    torch.manual_seed(seed)
    net = ActionNet(backbone=build_model(CFG), dim_rep=128, dropout_ratio=0., version='embed', hidden_dim=HIDDEN, num_joints=17).to(DEV)
    net.backbone.precision = 'fp32'
    return net


def clips(n, seed):
    return torch.stack([make_input(2, 27, 17, seed + i) for i in range(n)]).to(DEV)           # [n, M=2, T, 17, 3]


def test_embed_head_keys_and_unit_rows():
    net = embed_net().eval()
    keys = list(net.state_dict())
    assert all(k.startswith('backbone.') or k.startswith('head.fc1.') for k in keys)
    assert sorted(k for k in keys if k.startswith('head.')) == ['head.fc1.bias', 'head.fc1.weight']
    with torch.no_grad():
        out = net(clips(3, 60))
    assert out.shape == (3, HIDDEN) and float((out.norm(dim=-1) - 1).abs().max()) < 1e-5


def test_oneshot_step_matches_the_restated_reference_step():
    from motionbert_amd.oneshot import OneShotStep
    a, b = embed_net().train(), embed_net().train()
    step = OneShotStep(a, temperature=0.1, lr_backbone=1e-4, lr_head=1e-3, weight_decay=0.01)
    x = clips(8, 80)
    labels = torch.tensor([0, 1, 2, 3, 3, 2, 1, 0], device=DEV)
    lr0 = (step.opt_backbone.lr, step.opt_head.lr)
    # the restated step on the identical copy: the embedding before the step, float64 loss and gradient of fc1's output
    pooled = b.head.pooled(b.backbone, x).detach()              # with the graph on, as the step runs it: the same kernels, the same bits
    z = b.head.fc1(pooled).detach()
    with torch.no_grad():
        out = b.eval()(x)
    assert float((out - torch.nn.functional.normalize(z, dim=-1)).abs().max()) < 1e-4
    zf = z.reshape(8, 1, HIDDEN)
    rl, rd = SC.supcon_ref64(zf, labels, 0.1, 0.07, True)
    bl, br = SC.supcon_bounds(zf, labels, 0.1, 0.07, True)
    la = step(x, labels)
    assert la.is_cuda and la.shape == () and not la.requires_grad
    print(f'step loss {float(la):.9g} float64 {float(rl):.9g} bound {float(bl):.3e}')
    assert abs(float(la) - float(rl)) <= float(bl)
    # fc1.weight.grad = dz^T pooled: every element within the row gate carried through the product (8 terms, fp32: 10 roundings)
    dz, p64 = rd.reshape(8, HIDDEN), pooled.double()
    want = dz.T @ p64
    bw = br[None, :] @ p64.abs() + 10 * SC.U * (dz.abs().T @ p64.abs())
    got = a.head.fc1.weight.grad.double()
    ratio = float(((got - want).abs() / bw.clamp_min(1e-300)).max())
    print(f'fc1.weight.grad worst error / bound {ratio:.4f}')
    REPORT['step.fc1_weight_grad'] = dict(ratio=ratio, loss_ratio=abs(float(la) - float(rl)) / float(bl))
    assert ratio <= 1.0
    assert a.backbone.head.weight.grad is None, 'the backbone head is unused on the representation path'
    first = float(la)
    for _ in range(5):
        last = float(step(x, labels))
    assert math.isfinite(last) and last < first, (first, last)
    step.decay(0.5)
    assert (step.opt_backbone.lr, step.opt_head.lr) == (lr0[0] * 0.5, lr0[1] * 0.5)


class Recorder:
    """the model, with the embeddings it returned kept: a batch of one clip may run other kernels than a batch of nine, so the float64
    reference is taken of the very rows the evaluator saw"""

    def __init__(self, net):
        self.net, self.outs = net, []

    def eval(self):
        self.net.eval()
        return self

    def parameters(self):
        return self.net.parameters()

    def __call__(self, x):
        out = self.net(x)
        self.outs.append(out.clone())
        return out


def test_oneshot_evaluator_over_three_batches():
    from motionbert_amd.oneshot import OneShotEvaluator, validate
    rec = Recorder(embed_net(seed=92).train())
    xa, xt = clips(4, 100), clips(9, 200)
    la, lt = torch.tensor([5, 6, 7, 8]), torch.tensor([5, 6, 7, 8, 5, 6, 7, 8, 5])
    ev = OneShotEvaluator()
    ev.set_anchors(rec, [(xa[:3], la[:3]), (xa[3:], la[3:])])
    assert not rec.net.training and ev.anchors.shape == (4, HIDDEN)
    preds = torch.cat([ev.update(rec, xt[lo:hi], lt[lo:hi]) for lo, hi in ((0, 4), (4, 5), (5, 9))])
    fa, ft = torch.cat(rec.outs[:2]), torch.cat(rec.outs[2:])
    idx, sims, pred64, acc = SC.nn_ref64(fa, la.to(DEV).to(I32), ft, lt.to(DEV).to(I32))
    margin, unit = SC.nn_margin(sims, SC.nn_sim_bound(fa, ft))
    print(f'evaluator: float64 accuracy {acc:.4f}, {int(unit.sum())} of 9 rows with a clear margin')
    assert torch.equal(preds[unit], pred64[unit])
    got = ev.finish()
    assert got == float((preds.long() == lt.to(DEV)).double().mean()) and ev.count == 9
    if bool(unit.all()):
        assert got == acc
    rec.outs = []
    out = validate([(xa, la)], [(xt[:5], lt[:5]), (xt[5:], lt[5:])], rec)
    fa, ft = rec.outs[0], torch.cat(rec.outs[1:])
    _, sims, _, acc = SC.nn_ref64(fa, la.to(DEV).to(I32), ft, lt.to(DEV).to(I32))
    _, unit = SC.nn_margin(sims, SC.nn_sim_bound(fa, ft))
    assert isinstance(out, torch.Tensor) and out.shape == () and 0.0 <= float(out) <= 1.0
    if bool(unit.all()):
        assert float(out) == pytest.approx(acc)
