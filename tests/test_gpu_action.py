"""The action-recognition kernels on a real MI355X (csrc/action.hip): mbx_action_input and mbx_xent_topk against float64 (tests/actionerr.py:
restatements, gates, inputs; its own checks on the CPU: tests/test_actionerr.py), the functional entries, PackedAction and ActionStep(fused_loss=True).

Gates, none of them a number read off a kernel: per sample (input stage) and per row (loss, gradient) at most 4 x the error of the same
equations in float32 on the CPU, with the floors actionerr derives; zeroed samples, hit counts and reported draws exactly.  The worst
shares go to action_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import math
import os
import pickle
import time

import numpy as np
import pytest
import torch

from tests import actionerr as AE
from tests.helpers import GOLDEN, build_model, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, I32, F64 = torch.float32, torch.int32, torch.float64
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'action_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'action_parity.txt'), 'w') as f:
        f.write('action-recognition kernels against float64: worst error / gate per case (<= 1 passes)\n')
        for k in sorted(REPORT):
            f.write(f'{k:40s} ' + '  '.join(f'{n} {v:.4g}' for n, v in sorted(REPORT[k].items())) + '\n')
        worst = max((v for c in REPORT.values() for v in c.values()), default=0.0)
        f.write(f'worst share of a gate {worst:.4g}\nmodule wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'action.npz'))


@pytest.fixture(scope='module')
def cases():
    return AE.input_cases()


def nan(*shape, dtype=F32):
    return torch.full(shape, math.nan, dtype=dtype, device=DEV)


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ mbx_action_input
def run_input(ops, x, flags, crop, params=None, seed=0):
    """one launch into NaN-filled outputs; returns (y, params_out) on the device"""
    y, pout = nan(*x.shape), nan(x.shape[0], 9)
    ops.action_input(x, y, params, pout, AE.RANGES + (crop,), flags, seed)
    torch.cuda.synchronize()
    return y, pout


CASE_NAMES = ['in.%d.%d.%d' % s for s in AE.INPUT_SHAPES] + ['in.planted', 'in.clip', 'in.flags0', 'in.flags1', 'in.flags2']


@pytest.mark.parametrize('name', CASE_NAMES)
def test_action_input_against_float64_and_the_reference(ops, fixture, cases, name):
    """the reference's own draws as params_in: every sample within its gate of float64, zeroed samples and reported draws exactly; the
    kept frames within the same gate of the reference's own output"""
    xh, flags, crop = cases[name]
    ph = AE.case_params(fixture, name)
    x, p = xh.to(DEV), ph.to(DEV)
    y, pout = run_input(ops, x, flags, crop, params=p)
    assert torch.equal(bits(pout), bits(p)), f'{name}: params_out must be params_in'
    ref, gate, zero = AE.input_gates(xh, ph, flags)
    share, same, per = AE.input_gate(y, xh, ph, flags)
    frames = torch.from_numpy(fixture[name + '.frames'])
    err_fix = (y.cpu().double()[:, :, frames] - torch.from_numpy(fixture[name + '.out'])).abs().amax(dim=(1, 2, 3, 4))
    share_fix = float((err_fix / gate).max())
    print(f'{name}: worst share of a sample gate {share:.4f} (against the reference file {share_fix:.4f}); zeroed {zero.tolist()}; per sample {[round(float(v), 4) for v in per]}')
    REPORT[name] = dict(share=share, share_reference=share_fix)
    assert same, f'{name}: zeroed samples differ from float64 ({zero.tolist()})'
    assert share <= 1 and share_fix <= 1, (name, share, share_fix)
    if name == 'in.planted':
        assert zero.tolist() == [True, True, False, True, False, False, False]
        assert float(y[5, ..., 2].max()) == 1.0 and float(y[5, ..., 2].min()) == -1.0
    if not flags & AE.CROP:
        assert torch.equal(bits(y[..., 2]), bits(x[..., 2])), 'without the crop the confidence is written as it is'
    if flags == 0:
        assert torch.equal(bits(y), bits(x))


@pytest.mark.parametrize('name', CASE_NAMES)
def test_action_input_seeded_draws(ops, cases, name):
    """draws from a seed: the hash of csrc/aug_rng.h restated on the host bit for bit, inside the ranges, reproduced by a second call, and
    the output equal to a params_in = params_out call bit for bit -- and within the gates of float64 with those draws"""
    xh, flags, crop = cases[name]
    x = xh.to(DEV)
    seed = 0x1234_5678_9ABC_DEF0 ^ (AE.input_seed(xh.shape[:3]) * 1000003)
    y, pout = run_input(ops, x, flags, crop, seed=seed)
    want = AE.draw_params(x.shape[0], seed, crop)
    assert torch.equal(bits(pout.cpu()), bits(want)), f'{name}: draws differ from the host restatement of the hash'
    for k in range(9):
        lo, hi = AE.RANGES[k // 2] if k < 4 else AE.RANGES[2] if k < 8 else crop
        assert float(pout[:, k].min()) >= np.float32(lo) and float(pout[:, k].max()) <= np.float32(hi), (name, k)
    y2, pout2 = run_input(ops, x, flags, crop, seed=seed)
    assert torch.equal(bits(pout2), bits(pout)) and torch.equal(bits(y2), bits(y)), f'{name}: a second call must reproduce the first'
    y3, _ = run_input(ops, x, flags, crop, params=pout)
    assert torch.equal(bits(y3), bits(y)), f'{name}: params_in = params_out must give the same bits'
    y4, pout4 = run_input(ops, x, flags, crop, seed=seed + 1)
    if flags & AE.MOVE:
        assert not torch.equal(pout4, pout) and not torch.equal(y4, y), 'another seed, other draws'
    share, same, _ = AE.input_gate(y, xh, pout.cpu(), flags)
    print(f'{name} (seeded): worst share of a sample gate {share:.4f}')
    REPORT[name + '.seeded'] = dict(share=share)
    assert same and share <= 1, (name, share)


def test_action_input_functional_entry_and_errors(ops):
    from motionbert_amd import augment
    xh = AE.motion_inputs(3, 2, 27, 17, 7900)
    x = xh.to(DEV)
    y, used = augment.action_input(x, seed=77, return_params=True)
    assert y.shape == x.shape and y.data_ptr() != x.data_ptr() and torch.equal(bits(used.cpu()), bits(AE.draw_params(3, 77)))
    share, same, _ = AE.input_gate(y, xh, used.cpu(), 3)
    assert same and share <= 1
    assert torch.equal(bits(augment.action_input(x, params=used)), bits(y))
    assert torch.equal(bits(augment.action_input(x, random_move=False, scale_range=None)), bits(x))
    val = augment.action_input(x, random_move=False)                      # the validation loader: crop only
    share, same, _ = AE.input_gate(val, xh, used.cpu(), AE.CROP)
    assert same and share <= 1
    assert float(augment.action_input(x, seed=1).sub(augment.action_input(x, seed=2)).abs().max()) > 0
    with pytest.raises(RuntimeError, match='ROCm device'):
        augment.action_input(xh)
    with pytest.raises(ValueError, match='lo > hi'):
        augment.action_input(x, scale_range=(1.2, 0.8))
    with pytest.raises(RuntimeError, match='lo > hi'):
        ops.action_input(x, torch.empty_like(x), None, None, ((10.0, -10.0),) + AE.RANGES[1:] + (AE.CROP_DEFAULT,), 3, 0)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.action_input(x[:, :, ::2], torch.empty_like(x), None, None, AE.RANGES + (AE.CROP_DEFAULT,), 3, 0)


def test_packed_action_stream_on_the_device(fixture, tmp_path):
    from motionbert_amd import augment, data
    anns = AE.annotations()
    pkl = str(tmp_path / 'ntu.pkl')
    with open(pkl, 'wb') as f:
        pickle.dump(AE.annotation_file(anns), f)
    prefix = str(tmp_path / 'train')
    data.pack_action(pkl, 'xsub_train', AE.ANN_N_FRAMES, prefix)
    ds = data.PackedAction(prefix, device=DEV)
    got = list(ds.batches(3, shuffle=True, epoch=2, seed=5))
    assert [tuple(b.shape) for b, _ in got] == [(3, 2, 27, 17, 3), (1, 2, 27, 17, 3)] and all(b.is_cuda and l.is_cuda and l.dtype == torch.int64 for b, l in got)
    idx = data.shard_indices(4, True, 2, 5, 0, 1)
    motions = torch.from_numpy(fixture['ann.xsub_train.motions'])
    for k, (b, l) in enumerate(got):
        rows = np.sort(idx[3 * k:3 * k + 3])
        want = augment.action_input(motions[rows].to(DEV), seed=ds.batch_seed(5, 2, 0, k))
        assert torch.equal(bits(b), bits(want)) and l.tolist() == fixture['ann.xsub_train.labels'][rows].tolist()
    again = list(ds.batches(3, shuffle=True, epoch=2, seed=5))
    assert all(torch.equal(bits(a), bits(b)) for (a, _), (b, _) in zip(got, again))


# ------------------------------------------------------------------------------------------------ mbx_xent_topk
def run_xent(ops, z, lab, gs=1.0, grad=True, acc=None):
    values = nan(3)
    d = nan(*z.shape) if grad else None
    ops.xent_topk(z, lab.to(I32), values, d, acc, gs)
    torch.cuda.synchronize()
    return values, d


def check_xent(tag, ops, zh, labh, gs=1.0):
    z, lab = zh.to(DEV), labh.to(DEV)
    values, d = run_xent(ops, z, lab, gs)
    got = AE.xent_check(values, d, zh, labh, gs)
    # every row's loss on its own: a one-row call returns it as the mean
    r64, g_row, _, _ = AE.xent_gates(zh, labh, gs)
    rows = nan(len(zh), 3)
    for i in range(len(zh)):
        ops.xent_topk(z[i:i + 1], lab[i:i + 1].to(I32), rows[i], None, None, gs)
    torch.cuda.synchronize()
    rl = rows[:, 0].cpu().double()
    same_nan = AE.same_nan(rl, r64['row_loss'])
    row_share = float(torch.nan_to_num(torch.where(torch.isnan(r64['row_loss']), torch.zeros_like(rl), (rl - r64['row_loss']).abs()) / g_row,
                                       nan=float('inf')).max())
    print(f'{tag}: loss {float(values[0]):.9g} float64 {float(r64["loss"]):.9g} share {got["loss"]:.4f}; worst row-loss share {row_share:.4f}; '
          f'worst gradient-row share {got["grad"]:.4f}; hits {int(values[1])} / {int(values[2])} float64 {r64["hit1"]} / {r64["hit5"]}')
    REPORT[tag] = dict(loss=got['loss'], row_loss=row_share, grad=got['grad'])
    assert got['exact'] and same_nan, f'{tag}: hit counts or NaN pattern differ from float64'
    assert got['loss'] <= 1 and row_share <= 1 and got['grad'] <= 1, (tag, got, row_share)
    return z, lab, values, d


@pytest.mark.parametrize('shape', AE.XENT_SHAPES)
def test_xent_topk_against_float64_and_the_reference(ops, fixture, shape):
    zh, labh = AE.logit_inputs(*shape, AE.xent_seed(shape))
    tag = 'xe.%d.%d' % shape
    z, lab, values, d = check_xent(tag, ops, zh, labh)
    only, _ = run_xent(ops, z, lab, grad=False)                              # dlogits = NULL: the same values
    assert torch.equal(bits(only), bits(values)), f'{tag}: the values differ without dlogits'
    again, d2 = run_xent(ops, z, lab)
    assert torch.equal(bits(again), bits(values)) and torch.equal(bits(d2), bits(d)), f'{tag}: two calls must be bit-identical'
    # the reference's own CrossEntropyLoss, gradient and accuracy (tests/golden/action.npz), within the same gates
    _, _, g_mean, g_d = AE.xent_gates(zh, labh)
    assert abs(float(values[0]) - float(fixture[tag + '.loss'])) <= g_mean
    rows = torch.from_numpy(fixture[tag + '.rows'])
    err = (d.cpu().double()[rows] - torch.from_numpy(fixture[tag + '.dlogits'])).abs().amax(dim=1)
    assert bool((err <= g_d[rows]).all()), float((err / g_d[rows]).max())
    assert [round(float(a) * shape[0] / 100) for a in fixture[tag + '.acc']] == [int(values[1]), int(values[2])]
    check_xent(tag + '.gs', ops, zh, labh, gs=-3.0)
    # acc: two calls add up
    acc = torch.zeros(4, dtype=F64, device=DEV)
    zh2, labh2 = AE.logit_inputs(*shape, AE.xent_seed(shape) + 1)
    v1, _ = run_xent(ops, z, lab, grad=False, acc=acc)
    v2, _ = run_xent(ops, zh2.to(DEV), labh2.to(DEV), acc=acc)
    a = acc.cpu()
    n = shape[0]
    assert a[1:].tolist() == [float(v1[1] + v2[1]), float(v1[2] + v2[2]), 2.0 * n]
    assert abs(float(a[0]) / n - (float(v1[0]) + float(v2[0]))) <= 2 * AE.EPS32 * abs(float(a[0]) / n), 'acc[0] is the sum of the two calls\' row losses'


def test_xent_topk_planted_rows_and_labels_out_of_range(ops):
    """scores at +-80 and 1e4, the target exactly 5th and 6th, exact ties, and labels outside [0, C): NaN in their rows and the mean, no hit,
    nothing read out of bounds"""
    zh, labh = AE.planted_logits()
    _, _, values, d = check_xent('xe.planted', ops, zh, labh)
    assert bool(torch.isfinite(d).all()) and 0 < int(values[1]) < int(values[2]) < len(zh)
    zb, lb = AE.bad_label_logits()
    _, _, values, d = check_xent('xe.bad_label', ops, zb, lb)
    assert math.isnan(float(values[0])) and torch.isnan(d).all(1).tolist() == [True, False, True, False]
    acc = torch.zeros(4, dtype=F64, device=DEV)
    run_xent(ops, zb.to(DEV), lb.to(DEV), grad=False, acc=acc)
    assert math.isnan(float(acc[0])) and acc[1:].tolist() == [float(values[1]), float(values[2]), 4.0]
    with pytest.raises(RuntimeError, match='bad shape'):
        ops.xent_topk(torch.zeros(2, 4097, device=DEV), torch.zeros(2, dtype=I32, device=DEV), nan(3), None, None)


def test_cross_entropy_topk_is_differentiable(ops):
    from motionbert_amd.action import cross_entropy_topk
    zh, labh = AE.logit_inputs(32, 60, 7950)
    z = zh.to(DEV).requires_grad_(True)
    acc = torch.zeros(4, dtype=F64, device=DEV)
    loss, values = cross_entropy_topk(z, labh.to(DEV), acc=acc)
    (loss * 2.5).backward()
    got = AE.xent_check(values, z.grad, zh, labh, 2.5)
    assert loss.dim() == 0 and not values.requires_grad and got['exact'] and got['loss'] <= 1 and got['grad'] <= 1, got
    assert float(acc[3]) == 32.0
    with pytest.raises(RuntimeError, match='ROCm device'):
        cross_entropy_topk(zh, labh)


# ------------------------------------------------------------------------------------------------ the step and the evaluation
def _action_net():
    from motionbert_amd.action import ActionNet
    from tests.test_gpu_train import LITE
    cfg = dict(LITE, depth=2, dim_feat=128, dim_rep=128, num_heads=4)
    torch.manual_seed(91)
    net = ActionNet(backbone=build_model(cfg), dim_rep=128, num_classes=60, dropout_ratio=0., version='class', hidden_dim=2048, num_joints=17).to(DEV)
    net.backbone.precision = 'fp32'
    return net.train()


def test_action_step_fused_loss_against_the_torch_loss():
    """one ActionStep(fused_loss=True) against fused_loss=False on identical copies of the tiny model of tests/test_gpu_train.py's action
    test, dropout 0: the losses within the loss gate of the scores' float64 loss, the parameters after the step as that test compares them
    (an AdamW step moves an element by at most lr, so two runs differ by at most 2 lr; matrices within 1e-4 in norm), the meters against
    a float64 count"""
    from motionbert_amd.train import ActionStep
    a, b = _action_net(), _action_net()
    fused, plain = ActionStep(a, fused_loss=True), ActionStep(b)
    x = torch.stack([make_input(2, 27, 17, 80 + i) for i in range(4)]).to(DEV)
    labels = torch.tensor([3, 7, 59, 0], device=DEV)
    la, oa = fused(x, labels)
    lb, ob = plain(x, labels)
    r64, _, g_mean, _ = AE.xent_gates(oa.float().cpu(), labels.cpu())
    print(f'step: fused loss {float(la):.9g} torch loss {float(lb):.9g} float64 of the scores {float(r64["loss"]):.9g} gate {g_mean:.3e}; '
          f'scores bit-equal {torch.equal(oa, ob)}')
    REPORT['step'] = dict(loss_vs_torch=abs(float(la) - float(lb)) / g_mean, loss_vs_float64=abs(float(la) - float(r64['loss'])) / g_mean)
    assert abs(float(la) - float(r64['loss'])) <= g_mean and abs(float(la) - float(lb)) <= g_mean
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        lr = 1e-3 if n.startswith('head.') else 1e-4
        assert float((p.detach() - q.detach()).abs().max()) <= 2 * lr, n
        if p.ndim >= 2 and 'ts_attn' not in n:
            assert float((p.detach() - q.detach()).norm() / q.detach().norm()) < 1e-4, n
    loss_avg, top1, top5 = fused.meters()
    assert abs(loss_avg - float(r64['loss'])) <= g_mean and (top1, top5) == (100.0 * r64['hit1'] / 4, 100.0 * r64['hit5'] / 4)
    fused(x, labels)
    assert float(fused.meter[3]) == 8.0
    fused.reset_meters()
    assert float(fused.meter.abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match='fused_loss=True'):
        plain.meters()


def test_action_validate_on_the_device():
    from motionbert_amd.action import ActionEvaluator, validate
    net = _action_net()
    loader = [(torch.stack([make_input(2, 27, 17, 60 + 4 * k + i) for i in range(n)]), torch.tensor([(7 * (4 * k + i)) % 60 for i in range(n)]))
              for k, n in enumerate((4, 3))]
    loss, top1, top5 = validate(loader, net, torch.nn.CrossEntropyLoss())
    assert not net.training and all(isinstance(v, float) for v in (loss, top1, top5))
    with torch.no_grad():
        scores = torch.cat([net(b.to(DEV)) for b, _ in loader]).float().cpu()
    labels = torch.cat([l for _, l in loader])
    r64, _, g_mean, _ = AE.xent_gates(scores, labels)
    assert abs(loss - float(r64['loss'])) <= g_mean and (top1, top5) == (100.0 * r64['hit1'] / 7, 100.0 * r64['hit5'] / 7)
    ev = ActionEvaluator()
    out = ev.update(net, *loader[0])
    assert out.shape == (4, 60) and ev.finish()[0] > 0
