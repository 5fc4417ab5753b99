"""Generate the golden fixtures under tests/golden/ from the REAL reference model.

TEST INFRASTRUCTURE ONLY.  Run in the build container, where the reference
checkout is mounted read-only at /root/reference:

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden.py

The reference (pure PyTorch) is imported, never copied; it cannot travel to the
GPU box, so its inputs/outputs/gradients are committed as small .npz fixtures:

  tiny_default.npz / tiny_trained.npz
      a small DSTformer (C=64, 2 heads of 32, depth 2, T=9) with every weight,
      the input, the output, the representation, a random cotangent and the
      reference autograd gradient of every parameter and of the input (fp64).
  seed0_lite.npz / seed0_full.npz
      MotionBERT-Lite / full model exactly as `load_backbone` builds them
      (lib/utils/learning.py:83-85) after torch.manual_seed(0): per-parameter
      (sum, |sum|) of the initial weights, a [1,27,17,3] input, the fp64 output
      and per-parameter (l2, sum) of the gradients.  The weights themselves are
      re-created on the test machine from the same seed (weights drawn with
      tests.helpers.portable_erfinv, here and in the tests: the same on every host).

  full_1x243.npz / lite_2x81.npz
      the BASELINE.json shapes: the full model on [1,243,17,3] ("trained-like"
      weights: seed 0 + helpers.trained_like(5)) and MotionBERT-Lite on
      [2,81,17,3] (configs[0], seed-0 init).  fp64 output and input gradient,
      (l2, sum) of every parameter gradient, the FULL gradient of every tensor
      with <= 16384 elements and a fixed 4096-element sample of every larger one,
      plus the error of the reference ITSELF under torch.autocast(bfloat16)
      against its fp64 run (output, input gradient, global gradient, per tensor): the yardstick
      the bf16 mode of the HIP path is gated against.
      Their seed-0 weights were drawn with torch's own erfinv on MKL's AVX-512 branch.
  lite_2x81_init.npz
      where those weights of lite_2x81 differ from the tests.helpers.portable_erfinv
      draw (one or two ulps: position gaps + bit-pattern steps), so that
      tests.helpers.minted_weights rebuilds them bit for bit on any host.  Written
      on a host whose MKL takes the AVX-512 branch (checked against the fixture).

While generating, the numpy oracle is checked against the reference (fp64
forward and every gradient); the script aborts if they disagree.
"""
from __future__ import annotations

import os
import sys
from functools import partial

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('MOTIONBERT_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn as nn

from oracle import dstformer_oracle as O
from tests.helpers import portable_erfinv


def import_reference(REF=None):
    """Import the reference class without shadowing by this repo's own lib/ shim."""
    import importlib.util
    REF = REF or globals()['REF']
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.')}
    sys.path.insert(0, REF)
    try:
        spec = importlib.util.spec_from_file_location('ref_lib_model_drop', os.path.join(REF, 'lib/model/drop.py'))
        drop = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drop)
        # DSTformer.py does `from lib.model.drop import DropPath`
        import types
        lib = types.ModuleType('lib'); lib.__path__ = [os.path.join(REF, 'lib')]
        libm = types.ModuleType('lib.model'); libm.__path__ = [os.path.join(REF, 'lib/model')]
        sys.modules.update({'lib': lib, 'lib.model': libm, 'lib.model.drop': drop})
        spec = importlib.util.spec_from_file_location('lib.model.DSTformer', os.path.join(REF, 'lib/model/DSTformer.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.DSTformer
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            sys.modules.pop(k)
        sys.modules.update(saved)


def make_input(B, T, J, seed):
    """Synthetic 2D keypoints: x,y ~ U(-1,1), confidence ~ U(0,1)."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(B, T, J, 2, generator=g) * 2 - 1
    conf = torch.rand(B, T, J, 1, generator=g)
    return torch.cat([xy, conf], -1)


def trained_like(model, seed):
    """Perturb default init so softmaxes are not flat and the fusion is data dependent."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.startswith('ts_attn'):
                p.add_(torch.randn(p.shape, generator=g) * (0.05 if p.ndim == 2 else 0.2))
            elif p.ndim >= 2 and 'embed' not in n:
                p.mul_(3.0)
            elif 'norm' in n and n.endswith('weight'):
                p.add_(torch.randn(p.shape, generator=g) * 0.2)
            elif n.endswith('bias'):
                p.add_(torch.randn(p.shape, generator=g) * 0.1)


def run_reference(model, x, cot, return_rep=False):
    m = model.double()
    xd = x.double().requires_grad_(True)
    out = m(xd, return_rep=return_rep)
    rep = m.get_representation(xd).detach()
    (out * cot.double()).sum().backward()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy() for n, p in m.named_parameters()}
    return out.detach().numpy(), rep.numpy(), grads, xd.grad.numpy().copy()


def check_oracle(cfg, sd, x, cot, out_ref, grads_ref, dx_ref, tag):
    out, cache = O.forward(sd, x, cfg, want_cache=True)
    e = O.rel_l2(out, out_ref)
    G, dx = O.backward(sd, cache, cot, cfg)
    worst = max(O.rel_l2(G[k], grads_ref[k]) if np.linalg.norm(grads_ref[k]) > 0 else float(np.abs(G[k]).max()) for k in grads_ref)
    edx = O.rel_l2(dx, dx_ref)
    print(f'[{tag}] oracle vs reference(fp64): out {e:.2e}  worst-grad {worst:.2e}  dx {edx:.2e}')
    assert e < 1e-10 and worst < 1e-8 and edx < 1e-9, 'oracle disagrees with the reference'
    assert set(G) == set(grads_ref), (set(G) ^ set(grads_ref))


def tiny(DST, variant):
    kw = dict(dim_in=3, dim_out=3, dim_feat=64, dim_rep=64, depth=2, num_heads=2, mlp_ratio=2,
              num_joints=17, maxlen=16)
    torch.manual_seed(1234)
    model = DST(norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    if variant == 'trained':
        trained_like(model, 99)
    B, T = 2, 9
    x = make_input(B, T, 17, 7)
    cot = torch.randn(B, T, 17, 3, generator=torch.Generator().manual_seed(8))
    sd32 = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    out, rep, grads, dx = run_reference(model, x, cot)
    cfg = O.OracleConfig(eps=1e-6, **kw)
    check_oracle(cfg, sd32, x.numpy(), cot.numpy(), out, grads, dx, f'tiny_{variant}')
    # representation-path gradients (ActionNet path, model_action.py:68): head gets no gradient
    cot_rep = torch.randn(B, T, 17, 64, generator=torch.Generator().manual_seed(9))
    model.zero_grad()
    out_r, _, grads_r, dx_r = run_reference(model, x, cot_rep, return_rep=True)
    o2, cache = O.forward(sd32, x.numpy(), cfg, return_rep=True, want_cache=True)
    G2, dx2 = O.backward(sd32, cache, cot_rep.numpy(), cfg, return_rep=True)
    assert O.rel_l2(o2, out_r) < 1e-10 and O.rel_l2(dx2, dx_r) < 1e-9
    assert max(O.rel_l2(G2[k], grads_r[k]) for k in grads_r if np.linalg.norm(grads_r[k]) > 0) < 1e-8
    save = dict(x=x.numpy(), cot=cot.numpy(), out=out, rep=rep, dx=dx,
                cot_rep=cot_rep.numpy(), dx_rep=dx_r)
    save.update({f'cfg.{k}': np.asarray(v) for k, v in kw.items()})
    save.update({f'w.{k}': v for k, v in sd32.items()})
    save.update({f'g.{k}': v.astype(np.float32) for k, v in grads.items()})
    save.update({f'grep.{k}': v.astype(np.float32) for k, v in grads_r.items()})
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', f'tiny_{variant}.npz'), **save)


def seeded(DST, name, dim_feat, mlp_ratio):
    kw = dict(dim_in=3, dim_out=3, dim_feat=dim_feat, dim_rep=512, depth=5, num_heads=8, mlp_ratio=mlp_ratio,
              num_joints=17, maxlen=243)
    torch.manual_seed(0)  # train.py:37,41-44 default seed
    with portable_erfinv():
        model = DST(norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    sd32 = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    nparam = sum(v.size for v in sd32.values())
    B, T = 1, 27
    x = make_input(B, T, 17, 11)
    cot = torch.randn(B, T, 17, 3, generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        out32 = model(x).numpy().copy()
    out, rep, grads, dx = run_reference(model, x, cot)
    cfg = O.OracleConfig(eps=1e-6, **kw)
    check_oracle(cfg, sd32, x.numpy(), cot.numpy(), out, grads, dx, name)
    names = list(sd32.keys())
    save = dict(x=x.numpy(), cot=cot.numpy(), out=out, out_fp32=out32, dx=dx, nparam=np.asarray(nparam),
                names=np.asarray(names),
                w_stats=np.asarray([[sd32[k].astype(np.float64).sum(), np.abs(sd32[k].astype(np.float64)).sum()] for k in names]),
                g_stats=np.asarray([[np.linalg.norm(grads[k]), grads[k].sum()] for k in names]),
                rep_stats=np.asarray([np.linalg.norm(rep), rep.sum()]))
    save.update({f'cfg.{k}': np.asarray(v) for k, v in kw.items()})
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', f'seed0_{name}.npz'), **save)
    print(f'[{name}] params {nparam:,}; fp32-vs-fp64 output rel-l2 {O.rel_l2(out32, out):.2e}')


def init_fixup(name, kw):
    """tests/golden/<name>_init.npz: where the seed-0 weights the committed <name>.npz was minted with (torch's erfinv on this host)
    differ from the portable draw: `names` (the tensors that differ) and `count` (how many elements of each), then for every such
    element in that order `gap_lo` / `gap_hi` (the low / high byte of the gap to the previous differing flat position of the
    same tensor, the first from -1) and `step` (int8: minted minus portable float32 bit pattern; one or two ulps, never across zero)."""
    from tests.helpers import build_model
    with np.load(os.path.join(ROOT, 'tests/golden', f'{name}.npz')) as z:
        names, w_stats = [str(n) for n in z['names']], z['w_stats']
    minted = build_model(kw, seed=0).state_dict()
    got = np.asarray([[minted[k].double().sum().item(), minted[k].double().abs().sum().item()] for k in names])
    assert np.allclose(got, w_stats, rtol=1e-12, atol=1e-12), f'this host does not draw the weights {name}.npz was minted with'
    with portable_erfinv():
        portable = build_model(kw, seed=0).state_dict()
    diff_names, count, gaps, steps = [], [], [], []
    for k in names:
        m, p = minted[k].reshape(-1).numpy(), portable[k].reshape(-1).numpy()
        pos = np.flatnonzero(m != p)
        if pos.size == 0:
            continue
        step = m[pos].view(np.int32).astype(np.int64) - p[pos].view(np.int32)
        assert np.abs(step).max() <= 2 and np.array_equal(np.sign(m[pos]), np.sign(p[pos]))
        gap = np.diff(pos, prepend=-1)
        assert gap.max() < 65536
        diff_names.append(k), count.append(pos.size), gaps.append(gap), steps.append(step)
    gap, step = np.concatenate(gaps), np.concatenate(steps)
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', f'{name}_init.npz'), names=np.asarray(diff_names), count=np.asarray(count),
                        gap_lo=(gap & 255).astype(np.uint8), gap_hi=(gap >> 8).astype(np.uint8), step=step.astype(np.int8))
    print(f'[{name}_init] {gap.size:,} weights one or two ulps off the portable draw')


SAMPLE_FULL_BELOW = 16384
SAMPLE_N = 4096


def sample_index(numel):
    """Fixed pseudo-random sample of a flattened tensor with `numel` elements (stored in the fixture)."""
    return np.sort(np.random.default_rng(numel).choice(numel, SAMPLE_N, replace=False)).astype(np.int64)


def grad_error_table(got, ref, names):
    """global rel-L2 and per-tensor ||got-ref|| / max(||ref||, 1% of the global norm) -- the measure of tests/test_gpu_model.py."""
    g = np.sqrt(sum(float(np.sum(ref[n].astype(np.float64) ** 2)) for n in names))
    d = np.sqrt(sum(float(np.sum((got[n].astype(np.float64) - ref[n]) ** 2)) for n in names))
    per = np.asarray([np.linalg.norm(got[n].astype(np.float64) - ref[n]) / max(np.linalg.norm(ref[n]), 0.01 * g) for n in names])
    return d / g, per


def baseline_shape(DST, name, kw, B, T, trained_seed):
    """Reference-minted fixture at a BASELINE.json shape, with real gradients."""
    torch.manual_seed(0)
    model = DST(norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    if trained_seed is not None:
        trained_like(model, trained_seed)
    sd32 = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    names = list(sd32.keys())
    x = make_input(B, T, 17, 31)
    cot = torch.randn(B, T, 17, 3, generator=torch.Generator().manual_seed(32))
    # the reference under autocast(bf16), fp32 weights: what "bf16" means for the reference itself
    import copy
    m16 = copy.deepcopy(model)
    x16 = x.clone().requires_grad_(True)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o16 = m16(x16)
    (o16.float() * cot).sum().backward()
    g16 = {n: p.grad.detach().numpy().copy() for n, p in m16.named_parameters()}
    dx16 = x16.grad.detach().numpy().copy()
    # fp32 reference (its own round-off against fp64 is the floor of the 1e-3 gate)
    m32 = copy.deepcopy(model)
    o32 = m32(x)
    (o32 * cot).sum().backward()
    g32 = {n: p.grad.detach().numpy().copy() for n, p in m32.named_parameters()}
    out, rep, grads, dx = run_reference(model, x, cot)
    cfg = O.OracleConfig(eps=1e-6, **kw)
    check_oracle(cfg, sd32, x.numpy(), cot.numpy(), out, grads, dx, name)
    ac_global, ac_per = grad_error_table(g16, grads, names)
    f32_global, f32_per = grad_error_table(g32, grads, names)
    ac_out = O.rel_l2(o16.detach().float().numpy(), out)
    ac_dx = O.rel_l2(dx16, dx)      # (round 6) the yardstick of the bf16 INPUT gradient, which had no gate of its own
    print(f'[{name}] reference under autocast(bf16) vs fp64: out {ac_out:.2e}  dx {ac_dx:.2e}  grad global {ac_global:.2e}  worst tensor '
          f'{ac_per.max():.2e} ({names[int(ac_per.argmax())]});  fp32 vs fp64: out {O.rel_l2(o32.detach().numpy(), out):.2e} '
          f'grad global {f32_global:.2e} worst {f32_per.max():.2e}')
    save = dict(x=x.numpy(), cot=cot.numpy(), out=out, dx=dx.astype(np.float32), names=np.asarray(names),
                trained_seed=np.asarray(-1 if trained_seed is None else trained_seed),
                w_stats=np.asarray([[sd32[k].astype(np.float64).sum(), np.abs(sd32[k].astype(np.float64)).sum()] for k in names]),
                g_stats=np.asarray([[np.linalg.norm(grads[k]), grads[k].sum()] for k in names]),
                autocast_out=np.asarray(ac_out), autocast_dx=np.asarray(ac_dx), autocast_grad_global=np.asarray(ac_global), autocast_grad_per=ac_per,
                fp32_out=np.asarray(O.rel_l2(o32.detach().numpy(), out)), fp32_grad_global=np.asarray(f32_global), fp32_grad_per=f32_per)
    # The autocast yardsticks are ONE realisation of the reference's bf16 rounding noise and differ from run to run with the thread
    # count and the torch build (full_1x243, global gradient: 0.217 when the fixture was first minted in round 1, 0.107 in round 6;
    # everything fp64 in the fixture re-derives bit for bit).  The bf16 gates of tests/test_gpu_model.py are multiples of these
    # numbers and are frozen, so a yardstick that is already in the committed fixture is KEPT; a re-run only adds what is missing
    # (round 6: autocast_dx).  MBX_REFRESH_YARDSTICK=1 overwrites them.
    old_path = os.path.join(ROOT, 'tests/golden', f'{name}.npz')
    if os.path.exists(old_path) and os.environ.get('MBX_REFRESH_YARDSTICK', '0') != '1':
        with np.load(old_path) as old:
            for k in ('autocast_out', 'autocast_dx', 'autocast_grad_global', 'autocast_grad_per'):
                if k in old.files:
                    if not np.array_equal(old[k], save[k]):
                        print(f'[{name}] keeping the committed {k} = {float(np.max(old[k])):.4g} (this run: {float(np.max(save[k])):.4g})')
                    save[k] = old[k]
    for k in names:
        g = grads[k].reshape(-1)
        if g.size <= SAMPLE_FULL_BELOW:
            save['g.' + k] = g.astype(np.float32)
        else:
            if f'idx.{g.size}' not in save:
                save[f'idx.{g.size}'] = sample_index(g.size)
            save['gs.' + k] = g[save[f'idx.{g.size}']].astype(np.float32)
    save.update({f'cfg.{k}': np.asarray(v) for k, v in kw.items()})
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', f'{name}.npz'), **save)


def import_reference_loss(REF=None):
    """lib/model/loss.py of the reference (torch + numpy only), imported read-only."""
    import importlib.util
    REF = REF or globals()['REF']
    spec = importlib.util.spec_from_file_location('ref_lib_model_loss', os.path.join(REF, 'lib/model/loss.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pose_loss_fixture():
    """the reference's own loss_mpjpe / n_mpjpe / loss_velocity (loss.py:56-62,81-91,133-142), combined as
    train.py:176-189 does with the lambdas of MB_train_h36m.yaml (lambda_scale 0.5, lambda_3d_velocity 20), and the autograd
    gradient of the total with respect to the prediction, in fp64."""
    L = import_reference_loss()
    save = {}
    for tag, (B, T) in (('a', (3, 7)), ('t1', (2, 1)), ('b', (2, 243))):
        g = torch.Generator().manual_seed(100 + T)
        pred = (torch.randn(B, T, 17, 3, generator=g) * 0.4).double().requires_grad_(True)
        gt = (torch.randn(B, T, 17, 3, generator=g) * 0.3).double()
        gt = gt - gt[:, :, 0:1]
        l1, l2, l3 = L.loss_mpjpe(pred, gt), L.n_mpjpe(pred, gt), L.loss_velocity(pred, gt)
        tot = l1 + 0.5 * l2 + 20.0 * l3
        tot.backward()
        save.update({f'{tag}.pred': pred.detach().numpy().astype(np.float32), f'{tag}.gt': gt.numpy().astype(np.float32),
                     f'{tag}.losses': np.asarray([l1.item(), l2.item(), float(l3), tot.item()]), f'{tag}.dpred': pred.grad.numpy()})
        print(f'[pose_loss {tag}] mpjpe {l1.item():.6f} n_mpjpe {l2.item():.6f} velocity {float(l3):.6f} total {tot.item():.6f}')
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', 'pose_loss.npz'), **save)


def loss_2d_fixture():
    """VERDICT r2 item 7 / SURVEY 8d config 4: the reference's own loss_2d_weighted (loss.py:72-77) as the 2D branch of
    train_epoch uses it (train.py:163-166,200-203): the target IS the 2D batch (x, y, confidence), made root-relative, the
    confidence is the input's third channel; fp64 loss and autograd gradient with respect to the 3D prediction.  Case 'z'
    contains joints with zero confidence and joints where prediction == target (|.| = 0 -> zero gradient)."""
    L = import_reference_loss()
    save = {}
    for tag, (B, T) in (('a', (3, 30)), ('b', (2, 81)), ('z', (2, 5))):
        g = torch.Generator().manual_seed(300 + T)
        xy = torch.rand(B, T, 17, 2, generator=g) * 2 - 1
        conf = torch.rand(B, T, 17, 1, generator=g)
        if tag == 'z':
            conf[0, :, 3] = 0.0
        batch = torch.cat([xy, conf], -1).double()                      # motion_2d, returned as (input, target) by the 2D datasets
        target = batch - batch[:, :, 0:1, :]                            # rootrel (train.py:165-166)
        pred = (torch.randn(B, T, 17, 3, generator=g) * 0.4).double()
        if tag == 'z':
            pred[1, 2, 5, :2] = target[1, 2, 5, :2]
        pred.requires_grad_(True)
        loss = L.loss_2d_weighted(pred, target, batch[..., 2:])
        loss.backward()
        save.update({f'{tag}.batch': batch.numpy().astype(np.float32), f'{tag}.pred': pred.detach().numpy().astype(np.float32),
                     f'{tag}.loss': np.asarray(loss.item()), f'{tag}.dpred': pred.grad.numpy()})
        print(f'[loss_2d {tag}] {loss.item():.6f}')
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', 'loss_2d.npz'), **save)


def actionnet_fixture(DST):
    """the reference's own ActionNet (lib/model/model_action.py) on a small reference backbone, evaluation
    mode (BatchNorm on perturbed running statistics) and training mode (batch statistics, dropout 0): class scores, the
    cross-entropy loss and the autograd gradients of the head and of the backbone, fp64.  The weights are re-created on the
    test machine from the seeds; fc1 is 1088 x 2048, so only sampled gradients are stored."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('ref_lib_model_action', os.path.join(REF, 'lib/model/model_action.py'))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    kw = dict(dim_in=3, dim_out=3, dim_feat=64, dim_rep=64, depth=2, num_heads=2, mlp_ratio=2, num_joints=17, maxlen=16)
    torch.manual_seed(77)
    backbone = DST(norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    trained_like(backbone, 78)
    net = A.ActionNet(backbone=backbone, dim_rep=64, num_classes=7, dropout_ratio=0., version='class', hidden_dim=2048, num_joints=17)
    g = torch.Generator().manual_seed(79)
    with torch.no_grad():
        net.head.bn.running_mean.copy_(torch.randn(2048, generator=g) * 0.05)
        net.head.bn.running_var.copy_(torch.rand(2048, generator=g) * 0.5 + 0.75)
    N, Mp, T = 3, 2, 9
    x = make_input(N * Mp, T, 17, 80).reshape(N, Mp, T, 17, 3)
    labels = torch.tensor([2, 6, 0])
    net = net.double()
    bn_mean0, bn_var0 = net.head.bn.running_mean.numpy().copy(), net.head.bn.running_var.numpy().copy()   # before the train-mode pass
    net.eval()
    with torch.no_grad():
        logits_eval = net(x.double()).numpy().copy()
    net.train()
    logits = net(x.double())
    loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    names = [n for n, _ in net.named_parameters()]
    grads = {n: p.grad.numpy().copy() for n, p in net.named_parameters() if p.grad is not None}
    save = dict(x=x.numpy(), labels=labels.numpy(), logits_eval=logits_eval, logits_train=logits.detach().numpy(), loss=np.asarray(loss.item()),
                names=np.asarray(names), has_grad=np.asarray([n in grads for n in names]),
                g_l2=np.asarray([np.linalg.norm(grads[n]) if n in grads else 0.0 for n in names]),
                bn_mean=bn_mean0, bn_var=bn_var0)
    for n, v in grads.items():
        v = v.reshape(-1)
        if v.size <= SAMPLE_FULL_BELOW:
            save['g.' + n] = v.astype(np.float32)
        else:
            if f'idx.{v.size}' not in save:
                save[f'idx.{v.size}'] = sample_index(v.size)
            save['gs.' + n] = v[save[f'idx.{v.size}']].astype(np.float32)
    # weights are NOT stored: the test re-creates backbone and head from the same seeds (same module construction order ->
    # same RNG consumption); (sum, |sum|) per tensor guards against a silent mismatch
    save['w_stats'] = np.asarray([[p.detach().sum().item(), p.detach().abs().sum().item()] for _, p in net.named_parameters()])
    save.update({f'cfg.{k}': np.asarray(v) for k, v in kw.items()})
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', 'actionnet.npz'), **save)
    print(f'[actionnet] loss {loss.item():.6f}, head.backbone-head gradient present: {"backbone.head.weight" in grads}')


def dropout_fixture(DST):
    """the REAL reference in training mode with drop_rate 0.1, attn_drop_rate 0.1, drop_path_rate 0.2, its
    nn.Dropout / DropPath modules patched to draw the counter-based masks of motionbert_amd.dropmask (same seeds per site
    as the engine) instead of torch's RNG -- so WHERE each mask is applied, on WHICH tensor layout and with WHICH scaling
    is the reference's own code.  Weights and input of tiny_trained.npz; output and every gradient in fp64."""
    from motionbert_amd.dropmask import keep, mask_like, site_seed
    z = np.load(os.path.join(ROOT, 'tests/golden/tiny_trained.npz'))
    kw = {k[4:]: z[k].item() for k in z.files if k.startswith('cfg.')}
    model = DST(norm_layer=partial(nn.LayerNorm, eps=1e-6), drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2, **kw)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w.')}, strict=True)
    model = model.double().train()
    BASE = 4242
    SUB = {'blocks_st': {'attn_s': 0, 'mlp_s': 1, 'attn_t': 2, 'mlp_t': 3}, 'blocks_ts': {'attn_t': 0, 'mlp_t': 1, 'attn_s': 2, 'mlp_s': 3}}
    calls = {}

    def patch(name, mod):
        parts = name.split('.')
        def fwd(x, name=name, mod=mod):
            c = calls.get(name, 0)
            calls[name] = c + 1
            if name == 'pos_drop':
                p, seed = mod.p, site_seed(BASE, -1, 0, 0, 1)
                return x * mask_like(x.detach().contiguous(), p, seed)
            stream, level = (0 if parts[0] == 'blocks_st' else 1), int(parts[1])
            if parts[-1] == 'drop_path':                       # called once per sub-layer, in order
                p = mod.drop_prob
                if not p:
                    return x
                idx = torch.arange(x.shape[0], dtype=torch.int64)
                m = keep(idx, p, site_seed(BASE, level, stream, c % 4, 3)).to(x.dtype) / (1.0 - p)
                return x * m.reshape(-1, *([1] * (x.ndim - 1)))
            sub = SUB[parts[0]][parts[2]]
            if parts[-1] == 'attn_drop':
                kind = 0
            elif parts[-1] == 'proj_drop':
                kind = 1
            else:                                             # MLP.drop: after the activation, then after fc2
                kind = 2 if c % 2 == 0 else 1
            assert x.is_contiguous()
            return x * mask_like(x.detach(), mod.p, site_seed(BASE, level, stream, sub, kind))
        mod.forward = fwd
    n_patched = 0
    for name, mod in model.named_modules():
        if isinstance(mod, nn.Dropout) or type(mod).__name__ == 'DropPath':
            patch(name, mod)
            n_patched += 1
    x = torch.from_numpy(z['x']).double().requires_grad_(True)
    cot = torch.from_numpy(z['cot']).double()
    out = model(x)
    (out * cot).sum().backward()
    save = dict(out=out.detach().numpy(), dx=x.grad.numpy(), base_seed=np.asarray(BASE),
                rates=np.asarray([0.1, 0.1, 0.2]))
    save.update({'g.' + n: p.grad.numpy().astype(np.float32) for n, p in model.named_parameters()})
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', 'tiny_dropout.npz'), **save)
    ref_nodrop = z['out']
    print(f'[dropout] {n_patched} modules patched, {sum(calls.values())} mask draws; output moved by '
          f'{O.rel_l2(out.detach().numpy(), ref_nodrop):.3f} relative to the no-dropout output')


def augment_fixture():
    """the REAL Augmenter2D (lib/data/augmentation.py) with params/synthetic_noise.pth and
    params/d2c_params.pkl, its torch.rand / torch.randn calls patched to hand out the counter-based draws of
    oracle/augment_oracle.draws(seed): noise, mask and noise + mask outputs.  Also pins the oracle restatement."""
    import importlib.util, pickle, types
    from types import SimpleNamespace
    from oracle import augment_oracle as AO
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.')}
    try:
        tools = types.ModuleType('lib.utils.tools')
        tools.read_pkl = lambda path: pickle.load(open(path, 'rb'))
        lib = types.ModuleType('lib'); lib.__path__ = [os.path.join(REF, 'lib')]
        libu = types.ModuleType('lib.utils'); libu.__path__ = [os.path.join(REF, 'lib/utils')]
        sys.modules.update({'lib': lib, 'lib.utils': libu, 'lib.utils.tools': tools})
        spec = importlib.util.spec_from_file_location('lib.utils.utils_data', os.path.join(REF, 'lib/utils/utils_data.py'))
        ud = importlib.util.module_from_spec(spec); sys.modules['lib.utils.utils_data'] = ud; spec.loader.exec_module(ud)
        spec = importlib.util.spec_from_file_location('ref_augmentation', os.path.join(REF, 'lib/data/augmentation.py'))
        aug = importlib.util.module_from_spec(spec); spec.loader.exec_module(aug)
    finally:
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            sys.modules.pop(k)
        sys.modules.update(saved)
    args = SimpleNamespace(d2c_params_path=os.path.join(REF, 'params/d2c_params.pkl'), noise_path=os.path.join(REF, 'params/synthetic_noise.pth'),
                           mask_ratio=0.05, mask_T_ratio=0.1)
    A = aug.Augmenter2D(args)
    B, T, J, seed = 3, 50, 17, 0x1234567890
    x = make_input(B, T, J, 60)
    r = AO.draws(seed, B, T, J)
    real_rand, real_randn = torch.rand, torch.randn

    def run(mask, noise):
        q_rand = ([r['sel'], r['uniform']] if noise else []) + ([r['mask'], r['mask_T']] if mask else [])
        q_randn = [r['gaussian'], r['jitter'], r['shift']] if noise else []
        def fake(q):
            def f(*shape, **kw):
                t = q.pop(0)
                want = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
                assert tuple(t.shape) == want, (tuple(t.shape), want)
                return t.clone()
            return f
        torch.rand, torch.randn = fake(q_rand), fake(q_randn)
        try:
            out = A.augment2D(x.clone(), mask=mask, noise=noise)
        finally:
            torch.rand, torch.randn = real_rand, real_randn
        assert not q_rand and not q_randn
        return out
    outs = dict(noise=run(False, True), mask=run(True, False), both=run(True, True))
    noise = {k: v.float() for k, v in A.noise.items()}
    d2c = {k: float(v) for k, v in A.d2c_params.items()}
    for k, (m_, n_) in dict(noise=(False, True), mask=(True, False), both=(True, True)).items():
        mine = AO.augment2D(x.clone(), r, noise, d2c, 0.05, 0.1, use_mask=m_, use_noise=n_)
        err = float((mine - outs[k]).abs().max())
        print(f'[augment2d {k}] oracle vs reference max abs diff {err:.2e}')
        assert err < 1e-6
    flipped = ud.flip_data(x)
    assert torch.equal(AO.flip_data(x), flipped)
    # crop_scale_3d (utils_data.py:31-52) with the ratio forced: pins oracle.augment_oracle.crop_scale_3d
    clip = (np.random.default_rng(5).standard_normal((30, 17, 3)) * 0.4).astype(np.float64)
    real_uniform = np.random.uniform
    np.random.uniform = lambda low, high, size: np.asarray([0.8123])
    try:
        cs_ref = ud.crop_scale_3d(clip, [0.5, 1.0])
    finally:
        np.random.uniform = real_uniform
    assert np.abs(AO.crop_scale_3d(clip, 0.8123) - cs_ref).max() < 1e-12
    np.savez_compressed(os.path.join(ROOT, 'tests/golden', 'augment2d.npz'), x=x.numpy(), seed=np.asarray(seed), flipped=flipped.numpy(), cs_clip=clip, cs_ratio=np.asarray(0.8123), cs_out=cs_ref,
                        noise_mean=noise['mean'].numpy(), noise_std=noise['std'].numpy(), noise_weight=noise['weight'].numpy(),
                        d2c=np.asarray([d2c['a'], d2c['b'], d2c['m'], d2c['s']]), **{'out.' + k: v.numpy() for k, v in outs.items()})


FULL_KW = dict(dim_in=3, dim_out=3, dim_feat=512, dim_rep=512, depth=5, num_heads=8, mlp_ratio=2, num_joints=17, maxlen=243)
LITE_KW = dict(dim_in=3, dim_out=3, dim_feat=256, dim_rep=512, depth=5, num_heads=8, mlp_ratio=4, num_joints=17, maxlen=243)


def main():
    assert os.path.isdir(REF), f'reference checkout not found at {REF}'
    DST = import_reference()
    os.makedirs(os.path.join(ROOT, 'tests/golden'), exist_ok=True)
    only = sys.argv[1:]
    if only:      # e.g. `python oracle/make_golden.py lite_2x81 full_1x243` regenerates just those
        for name in only:
            {'pose_loss': pose_loss_fixture, 'loss_2d': loss_2d_fixture, 'actionnet': lambda: actionnet_fixture(DST), 'dropout': lambda: dropout_fixture(DST), 'augment': augment_fixture,
             'seed0_lite': lambda: seeded(DST, 'lite', 256, 4), 'seed0_full': lambda: seeded(DST, 'full', 512, 2),
             'lite_2x81': lambda: baseline_shape(DST, 'lite_2x81', LITE_KW, 2, 81, None),
             'lite_2x81_init': lambda: init_fixup('lite_2x81', LITE_KW),
             'full_1x243': lambda: baseline_shape(DST, 'full_1x243', FULL_KW, 1, 243, 5)}[name]()
        return
    tiny(DST, 'default')
    tiny(DST, 'trained')
    seeded(DST, 'lite', 256, 4)
    seeded(DST, 'full', 512, 2)
    baseline_shape(DST, 'lite_2x81', LITE_KW, 2, 81, None)
    baseline_shape(DST, 'full_1x243', FULL_KW, 1, 243, 5)
    init_fixup('lite_2x81', LITE_KW)
    pose_loss_fixture()
    loss_2d_fixture()
    actionnet_fixture(DST)
    dropout_fixture(DST)
    augment_fixture()
    print('golden fixtures written')


if __name__ == '__main__':
    main()
