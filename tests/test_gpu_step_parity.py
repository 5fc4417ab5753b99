"""Float64 parity of every kernel of csrc/train_step.hip at the training step's sizes and at their edges, on a real MI355X: pose loss,
2D loss, AdamW (kernel level), dropout / residual_drop / grad_drop, and the ActionNet pooling pair.  The treatment of
tests/test_gpu_local_parity.py: float64 references from the same fp32 / bf16 bits (on the device, in slabs where the tensors are
large), NaN-filled outputs (a NaN sentinel around ranges updated in place), the training-size case of each kernel launched three times
and bit-identical, and two kinds of gate, neither a number read off a kernel:

  (A) an elementwise worst-case bound derived at its definition (tests/steperr.py) or at its use, every element, no margin;
  (B) the worst unit of kernel-vs-float64 within 2 x the worst unit of the rounding model (the kernel's formula in torch fp32, in its
      operation order: steperr.*_model) against float64 on the same inputs; the floor exempts at most 0.1 % of the units.

The checker's own tests (seeded corruptions on the CPU): tests/test_steperr.py.  Everything measured goes to step_parity.json / .txt in
MBX_REPORT_DIR (default reports/), with the module's wall time beside the one test_gpu_local_parity.py recorded."""
import json
import math
import os
import time

import pytest
import torch

from tests import localerr as LE
from tests import steperr as SE
from tests import test_gpu_local_parity as LP
from tests.test_gpu_local_parity import nan, rnd

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
F32 = torch.float32
U = LE.U32
ROWS_STEP = 64 * 243 * 17
PRE = 'step.'
SEEDS = (7, 2 ** 40 + 12345, 987654321012345)      # below and above 2^32


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    rep = {k[len(PRE):]: v for k, v in LP.REPORT.items() if k.startswith(PRE)}
    rep['_wall_seconds'] = time.time() - t0
    other = os.path.join(out, 'local_parity.json')
    if os.path.exists(other):
        with open(other) as f:
            rep['_local_parity_wall_seconds'] = json.load(f).get('_wall_seconds')
    with open(os.path.join(out, 'step_parity.json'), 'w') as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'step_parity.txt'), 'w') as f:
        f.write(f'{"output":76s} {"gate":>10s} {"value":>10s} {"against":>10s} {"ratio":>7s}  worst unit ((b, t) | (row, col) | (element, 0))\n')
        for k in sorted(rep):
            v = rep[k]
            if isinstance(v, dict) and 'ratio' in v:
                f.write(f'{k:76s} {v["gate"]:>10s} {v["value"]:10.3e} {v["against"]:10.3e} {v["ratio"]:7.3f}  ({v["row"]}, {v["col"]})\n')
        for k in sorted(rep):
            if k.endswith('.three_launches_identical'):
                f.write(f'{k:76s} {"identical" if rep[k] else "DIFFER"}\n')
        f.write(f'wall time of the module: {rep["_wall_seconds"]:.1f} s\n')
        lp = rep.get('_local_parity_wall_seconds')
        f.write(f'wall time of test_gpu_local_parity.py (its own report in this directory): {f"{lp:.1f} s" if lp else "not recorded here"}\n')


def note(name, *a, **k):
    LP.note(PRE + name, *a, **k)


def thrice(name, launch, outs):
    LP.thrice(PRE + name, launch, outs)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def gate_a(name, got, x64, bound64, where=None):
    """every element within its bound; `where` maps the flat index of the worst element to what the report names"""
    b = LE.bound_check(got.reshape(-1, 1), x64.reshape(-1, 1), bound64.reshape(-1, 1))
    r, c = where(b['row']) if where else (b['row'], 0)
    note(name, 'bound', b['ratio'], 1.0, r, c, dict(violations=b['violations']))
    assert b['violations'] == 0, f'{name}: {b["violations"]} elements outside the bound, the worst at {b["ratio"]:.3f} x, element {b["row"]} -> {(r, c)}'


def gate_b(name, got, ref64, model, cols, where=None, floor_frac=LE.FLOOR_FRAC):
    torch.cuda.synchronize()
    g, m, ok, msg = SE.gate_units(got, ref64, model, cols, floor_frac)
    r, c = where(g['row']) if where else (g['row'], 0)
    note(name, '2 x model', g['worst'], m['worst'], r, c, dict(exempt=m['exempt'], model_mean=m['mean'], n_units=g['n_units']))
    assert ok, f'{name}: {msg} -> {(r, c)}'


# ---------------------------------------------------------------------------------------------- 1. pose loss and 2D loss
POSE_SHAPES = [(64, 243, 17), (1, 1, 17), (3, 1, 17), (5, 7, 17), (7, 243, 17), (2, 50, 1), (2, 50, 63), (2, 50, 64)]
LOSS_NAMES = ('mpjpe', 'n_mpjpe', 'velocity', 'total')


def _pose_gates(tag, B, T, J, pred, gt, ls, lv, gs, losses, dpred, skip_frames=None):
    ref_l, ref_g = SE.pose_ref64(pred, gt, ls, lv, gs)
    model = SE.pose_model(pred, gt, ls, lv, gs)
    got = dpred
    F = B * T
    frames = torch.arange(F, device=pred.device)
    if skip_frames is not None:
        # frames whose reference is NaN are compared place by place by the caller.  They are no units of the per-frame gate (a zeroed frame
        # would sit on the floor and count as exempt); no clip boundary may be among them, and they are zeroed for that gate's reshape only
        assert not bool(skip_frames.reshape(B, T)[:, [0, T - 1]].any())
        frames = frames[~skip_frames]
        got, ref_g, model = got.clone(), ref_g.clone(), model.clone()
        for t_ in (got, ref_g, model):
            t_.reshape(F, -1)[skip_frames] = 0
    else:
        bound = SE.pose_loss_bounds(pred, gt, ls, lv)
        for i, nm in enumerate(LOSS_NAMES):
            d = abs(float(losses[i].double() - ref_l[i]))
            note(f'pose_loss.{nm}.{tag}', 'bound', d, float(bound[i]), 0, 0, dict(value64=float(ref_l[i])))
            assert math.isfinite(float(losses[i])) and d <= float(bound[i]), f'pose_loss.{nm}.{tag}: |{float(losses[i])} - {float(ref_l[i])}| = {d:.3e} > {float(bound[i]):.3e}'
    gate_b(f'pose_loss.dpred.frame.{tag}', got.reshape(F, -1)[frames], ref_g.reshape(F, -1)[frames], model.reshape(F, -1)[frames], J * 3,
           where=lambda u: divmod(int(frames[u]), T))
    gate_b(f'pose_loss.dpred.clip_boundary.{tag}', SE.boundary_pairs(got, B, T), SE.boundary_pairs(ref_g, B, T), SE.boundary_pairs(model, B, T),
           2 * J * 3, where=lambda u: (u, T - 1))


@pytest.mark.parametrize('B,T,J', POSE_SHAPES)
def test_pose_loss(ops, B, T, J):
    pred, gt = SE.pose_inputs(B, T, J, seed=1000 * B + T + J, device=DEV)
    for ls, lv, gs, kind in ((0.5, 20.0, 1.0, 'default'), (0.25, 3.0, 2.5, 'lambdas_gscale')):      # all exact in fp32
        tag = f'{kind}.B{B}T{T}J{J}'
        losses, dpred = nan(4, dtype=F32), nan(B, T, J, 3, dtype=F32)
        ops.pose_loss(pred, gt, ls, lv, losses, dpred, gs)
        torch.cuda.synchronize()
        _pose_gates(tag, B, T, J, pred, gt, ls, lv, gs, losses, dpred)
        only = nan(4, dtype=F32)
        ops.pose_loss(pred, gt, ls, lv, only, None, gs)      # dpred = NULL: the same scalars, nothing else written
        torch.cuda.synchronize()
        assert torch.equal(bits(only), bits(losses)), f'pose_loss.{tag}: the scalars differ without dpred'
    if (B, T, J) == POSE_SHAPES[0]:
        thrice(f'pose_loss.B{B}T{T}J{J}', lambda: ops.pose_loss(pred, gt, 0.5, 20.0, losses, dpred, 1.0), [losses, dpred])


def test_pose_loss_refuses_more_than_64_joints(ops):
    z = torch.zeros(1, 2, 65, 3, device=DEV)
    with pytest.raises(RuntimeError):
        ops.pose_loss(z, z, 0.5, 20.0, nan(4, dtype=F32), nan(1, 2, 65, 3, dtype=F32))
    with pytest.raises(RuntimeError):
        ops.loss_2d_weighted(z, z, z[..., 2], nan(1, dtype=F32), nan(1, 2, 65, 3, dtype=F32))


def test_pose_loss_frame_with_pred_all_zero(ops):
    """sum p.p = 0 in one frame: the reference's scale is 0 / 0.  The float64 reference is the specification: NaN in the same places."""
    B, T, J = 2, 9, 17
    pred, gt = SE.pose_inputs(B, T, J, seed=77, device=DEV, plant=False)
    pred[1, 4] = 0
    losses, dpred = nan(4, dtype=F32), nan(B, T, J, 3, dtype=F32)
    ops.pose_loss(pred, gt, 0.5, 20.0, losses, dpred)
    torch.cuda.synchronize()
    ref_l, ref_g = SE.pose_ref64(pred, gt, 0.5, 20.0, 1.0)
    REP = dict(kernel_nan_losses=torch.isnan(losses).tolist(), ref_nan_losses=torch.isnan(ref_l).tolist(),
               kernel_nan_elements=int(torch.isnan(dpred).sum()), ref_nan_elements=int(torch.isnan(ref_g).sum()))
    LP.REPORT[PRE + 'pose_loss.zero_frame'] = REP
    assert torch.equal(torch.isnan(losses), torch.isnan(ref_l)), REP
    assert torch.equal(torch.isnan(dpred), torch.isnan(ref_g)), REP
    assert bool(torch.isfinite(dpred[~torch.isnan(ref_g)]).all()) and bool(torch.isfinite(losses[~torch.isnan(ref_l)]).all())
    nan_frames = torch.isnan(ref_g).reshape(B * T, -1).any(-1)
    _pose_gates('zero_frame', B, T, J, pred, gt, 0.5, 20.0, 1.0, losses, dpred, skip_frames=nan_frames)


@pytest.mark.parametrize('B,T,J', POSE_SHAPES)
def test_loss_2d(ops, B, T, J):
    pred, batch = SE.loss2d_inputs(B, T, J, seed=2000 * B + T + J, device=DEV)
    F = B * T
    views = {'strided': (batch, batch[..., 2]), 'contiguous': (batch[..., :2].contiguous(), batch[..., 2].contiguous())}
    assert views['strided'][1].stride(2) == 3 and views['contiguous'][1].stride(2) == 1
    got = {}
    for kind, (target, conf) in views.items():
        for gs in (1.0, 1.5):
            tag = f'{kind}.g{gs}.B{B}T{T}J{J}'
            loss, dpred = nan(1, dtype=F32), nan(B, T, J, 3, dtype=F32)
            ops.loss_2d_weighted(pred, target, conf, loss, dpred, gs)
            torch.cuda.synchronize()
            ref_l, ref_g = SE.loss2d_ref64(pred, target, conf, gs)
            bound = float(SE.loss2d_bound(pred, target, conf))
            d = abs(float(loss[0].double() - ref_l))
            note(f'loss_2d.loss.{tag}', 'bound', d, bound, 0, 0, dict(value64=float(ref_l)))
            assert math.isfinite(float(loss[0])) and d <= bound, f'loss_2d.loss.{tag}: {d:.3e} > {bound:.3e}'
            assert float(dpred[..., 2].abs().max()) == 0.0, f'loss_2d.{tag}: the z gradient is not exactly 0'
            assert float(dpred[..., :2][conf == 0].abs().max() if bool((conf == 0).any()) else 0.0) == 0.0, 'zero confidence: the gradient is exactly 0'
            model = SE.loss2d_model(pred, target, conf, gs)
            gate_b(f'loss_2d.dpred.frame.{tag}', dpred.reshape(F, -1), ref_g.reshape(F, -1), model.reshape(F, -1), J * 3, where=lambda u: (u // T, u % T))
            only = nan(1, dtype=F32)
            ops.loss_2d_weighted(pred, target, conf, only, None, gs)
            torch.cuda.synchronize()
            assert torch.equal(bits(only), bits(loss))
            got[(kind, gs)] = (loss.clone(), dpred.clone())
    for gs in (1.0, 1.5):       # the stride is addressing only
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got[('strided', gs)], got[('contiguous', gs)]))
    if (B, T, J) == POSE_SHAPES[0]:
        thrice(f'loss_2d.B{B}T{T}J{J}', lambda: ops.loss_2d_weighted(pred, batch, batch[..., 2], loss, dpred, 1.0), [loss, dpred])


# ---------------------------------------------------------------------------------------------- 2. AdamW at kernel level
HYP = dict(lr=SE.f32(1e-3), b1=SE.f32(0.9), b2=SE.f32(0.999), eps=SE.f32(1e-8), wd=SE.f32(0.01))      # what the C ABI receives
HYP_PY = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)
PAD = 16
# (value written to state[0] before the call or None, tick, the step count the update must use)
SCHEDULE = [(None, True, 1), (None, True, 2), (None, True, 3), (999.0, True, 1000), (99999.0, True, 100000), (None, False, 100000)]


def _full_param_count():
    from tests.helpers import build_model
    from tests.test_gpu_model import FULL
    return sum(p.numel() for p in build_model(FULL, seed=0).parameters())


def _adamw_buffers(n, off, seed):
    """four parallel buffers, NaN outside the range [PAD + off, PAD + off + n): the slices share their offset in a 16-byte line"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    full = lambda: torch.full((n + 2 * PAD + 4,), float('nan'), device=DEV, dtype=F32)
    sl = slice(PAD + off, PAD + off + n)
    P, G, M, V = full(), full(), full(), full()
    assert P.data_ptr() % 16 == 0
    P[sl] = torch.randn(n, device=DEV, generator=gen) * 0.05
    mag = 10.0 ** (torch.rand(n, device=DEV, generator=gen) * 10.0 - 8.0)      # 1e-8 .. 1e2
    g = mag * torch.where(torch.rand(n, device=DEV, generator=gen) < 0.5, -1.0, 1.0)
    zero = torch.arange(n, device=DEV) % 1024 == 3      # exactly 0 with m = v = 0: the update is exactly the decay
    g[zero] = 0
    G[sl] = g
    M[sl] = 0
    V[sl] = 0
    return (P, G, M, V), sl, zero


def _adamw_run(ops, n, off, seed, collect):
    (P, G, M, V), sl, zero = _adamw_buffers(n, off, seed)
    p, g, m, v = P[sl], G[sl], M[sl], V[sl]
    g0 = g.clone()
    state = torch.tensor([0.0, HYP['lr']], device=DEV, dtype=F32)
    outside = [bits(t).clone() for t in (P, G, M, V)]
    idx = torch.arange(n, device=DEV)
    decay32 = 1.0 - torch.tensor(HYP['lr'], dtype=F32, device=DEV) * torch.tensor(HYP['wd'], dtype=F32, device=DEV)
    for k, (preset, tick, t) in enumerate(SCHEDULE):
        if preset is not None:
            state[0] = preset
        before = float(state[0])
        g.copy_(g0 * torch.where((idx * (k + 1)) % 3 == 0, -1.0, 1.0))      # the sign pattern changes from step to step, zeros stay
        old = [x.clone() for x in (p, m, v)]
        ops.adamw_step(p, g, m, v, state, HYP['b1'], HYP['b2'], HYP['eps'], HYP['wd'], tick=tick)
        torch.cuda.synchronize()
        assert float(state[0]) == (before + 1.0 if tick else before) == float(t), (float(state[0]), before, tick, t)
        assert float(state[1]) == HYP['lr']
        if n == 0:
            continue
        ref = SE.adamw_ref64(old[0], g, old[1], old[2], t, **HYP)
        mod = SE.adamw_model(old[0], g, old[1], old[2], t, **HYP)
        bm, bv = SE.adamw_moment_bounds(g, ref[1], ref[2], HYP['b1'], HYP['b2'])
        gate_a(f'adamw.m.bound.n{n}.off{off}.t{t}{"" if tick else ".notick"}', m, ref[1], bm)
        gate_a(f'adamw.v.bound.n{n}.off{off}.t{t}{"" if tick else ".notick"}', v, ref[2], bv)
        if bool(zero.any()):
            assert torch.equal(bits(p[zero]), bits(old[0][zero] * decay32)), f'adamw n{n} off{off} t{t}: g = m = v = 0 must give exactly the decay'
            assert float(m[zero].abs().max()) == 0.0 and float(v[zero].abs().max()) == 0.0
        nz = ~zero
        o64 = old[0].double()
        collect.setdefault(k, []).append(dict(n=n, off=off, t=t, upd=(p.double() - o64)[nz], upd_ref=(ref[0] - o64)[nz], upd_mod=(mod[0].double() - o64)[nz],
                                              m=m[nz].clone(), m_ref=ref[1][nz], m_mod=mod[1][nz], v=v[nz].clone(), v_ref=ref[2][nz], v_mod=mod[2][nz],
                                              index=idx[nz]))
    for t_, was in zip((P, G, M, V), outside):      # everything outside the range (>= 16 floats on each side), and g itself, bit-identical
        now = bits(t_)
        assert torch.equal(now[:PAD + off], was[:PAD + off]) and torch.equal(now[PAD + off + n:], was[PAD + off + n:]), f'adamw n{n} off{off}: memory outside the range changed'
    return (P, G, M, V), sl, state


def _adamw_gate_b(name, runs):
    """gate B per element over the pooled runs of one step.  m and v span ten orders of magnitude with g, and the update of an element whose
    |g| is near eps = 1e-8 is a fraction of the others' (sqrt(v) no longer dominates the denominator): with the floor of unit_errors more than
    0.1 % of such elements would be exempt.  So all three are judged purely relative (floor 0: nothing exempt)."""
    cat = lambda key: torch.cat([r[key].double() for r in runs])
    sizes = torch.tensor([r['index'].numel() for r in runs]).cumsum(0)

    def where(u):
        i = int((sizes <= u).sum())
        r = runs[i]
        return (f'n{r["n"]}.off{r["off"]}', int(r['index'][u - (int(sizes[i - 1]) if i else 0)]))
    t = runs[0]['t']
    gate_b(f'{name}.update.t{t}', cat('upd')[:, None], cat('upd_ref')[:, None], cat('upd_mod')[:, None], 1, where=where, floor_frac=0.0)
    gate_b(f'{name}.m.t{t}', cat('m')[:, None], cat('m_ref')[:, None], cat('m_mod')[:, None], 1, where=where, floor_frac=0.0)
    gate_b(f'{name}.v.t{t}', cat('v')[:, None], cat('v_ref')[:, None], cat('v_mod')[:, None], 1, where=where, floor_frac=0.0)


def test_adamw_small_ranges(ops):
    """n = 0 .. 8 at the four offsets: head and tail scalars only, or one 16-byte group.  Gate A holds per element of every run; gate B compares
    two WORST units, which needs a population: a single element's rounding error of the model can be 0 by chance.  So the runs of all these
    sizes and offsets are pooled per step (30 .. 120 elements); each larger size below is pooled over its four offsets."""
    collect = {}
    for n in (0, 1, 2, 3, 4, 5, 7, 8):
        for off in range(4):
            _adamw_run(ops, n, off, seed=100 * n + off, collect=collect)
    for k in sorted(collect):
        _adamw_gate_b(f'adamw.n0to8{"" if SCHEDULE[k][1] else ".notick"}', collect[k])


@pytest.mark.parametrize('n', [1023, 1024, 4 * 256 * 4096 + 5, 'full'])
def test_adamw_ranges(ops, n):
    """1023 / 1024: around one block; 4 * 256 * 4096 + 5: one float4 per thread of the capped grid and a tail; the full model's parameter
    count: the grid-stride loop beyond 256 * 16 * 256 float4s"""
    big = n == 'full'
    n = _full_param_count() if big else n
    if big:
        assert n // 4 > 256 * 16 * 256, n
    collect = {}
    for off in range(4):
        if big:
            collect = {}
        bufs, sl, state = _adamw_run(ops, n, off, seed=n % 9973 + off, collect=collect)
        if big:
            for k in sorted(collect):
                _adamw_gate_b(f'adamw.n{n}.off{off}{"" if SCHEDULE[k][1] else ".notick"}', collect[k])
    if not big:
        for k in sorted(collect):
            _adamw_gate_b(f'adamw.n{n}{"" if SCHEDULE[k][1] else ".notick"}', collect[k])
    else:
        P, G, M, V = bufs
        p, g, m, v = P[sl], G[sl], M[sl], V[sl]
        saved = [x.clone() for x in (p, m, v, state)]

        def launch():
            for x, s in zip((p, m, v, state), saved):      # (thrice has just NaN-filled p, m, v)
                x.copy_(s)
            ops.adamw_step(p, g, m, v, state, HYP['b1'], HYP['b2'], HYP['eps'], HYP['wd'])
        thrice(f'adamw.n{n}.off3', launch, [p, m, v])


def test_adamw_refuses_mismatched_offsets(ops):
    a, b = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    state = torch.tensor([0.0, 1e-3], device=DEV)
    with pytest.raises(RuntimeError):
        ops.adamw_step(a[1:9], b[0:8], a[17:25], a[33:41], state, 0.9, 0.999, 1e-8, 0.01)
    with pytest.raises(RuntimeError):
        ops.adamw_step(a[0:8], b[0:8], a[16:24], a[33:41], state, 0.9, 0.999, 1e-8, 0.01)
    torch.cuda.synchronize()
    assert float(state[0]) == 0.0 and float(a.abs().max()) == 0.0


def test_adamw_against_torch_adamw_in_float64(ops):
    """What the fp32 C ABI and the fp32 bias corrections cost against torch.optim.AdamW in float64 with Python-double hyper-parameters, on the
    same gradients, step by step (each side on its own trajectory from the same start).  Derived elementwise, to first order:

      bias corrections   update ~ sqrt(bc2) / bc1, bc = 1 - b^t: d bc / bc = |b_f32 - b| t b^(t-1) / (1 - b^t) =: T(b, t)  ->  T(b1, t) + T(b2, t) / 2.
                         powf to 2 ulp of b^t: 4 U b^t / (1 - b^t), likewise (half for b2); the two subtractions 1 - b^t, rsqrt (2 ulp, halved by nothing: 4 U), the division lr / bc1: 6 U in all
      moments            m = (1 - b1) sum_k b1^(s-k) g_k after s accumulations: each weight moves by |d b1| (1 / (1 - b1) + (s - 1) / b1) relative,
                         so |dm| <= that x Am, Am = the same recurrence on |g| (signs change between steps); v likewise with Av = v (all >= 0),
                         entering the update with 1/2.  fp32: m rounds 2 U Am per accumulation, v 3 U v.
      lr, eps, wd        relative roundings r_lr, r_eps, r_wd <= U of the C floats: |u| r_lr, |u| eps r_eps / den (<= |u| r_eps), |p| lr wd (r_lr + r_wd)
      the kernel's own   p decay and the final subtraction: 2 U |p|; step m, sqrt, . rs2, + eps, the division: 5 U |u|; decay = 1 - lr wd: U |p| lr wd ... U |p|
    The measured relative L2 of the update's deviation and the derived one go to the report (DESIGN.md names both)."""
    n = 4 * 256 * 4096 + 5
    (P, G, M, V), sl, zero = _adamw_buffers(n, 0, seed=5)
    p, g, m, v = P[sl], G[sl], M[sl], V[sl]
    g0 = g.clone()
    idx = torch.arange(n, device=DEV)
    state = torch.tensor([0.0, HYP['lr']], device=DEV, dtype=F32)
    w = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.AdamW([w], lr=HYP_PY['lr'], betas=(HYP_PY['b1'], HYP_PY['b2']), eps=HYP_PY['eps'], weight_decay=HYP_PY['wd'])
    rel = {k: abs(HYP[k] - HYP_PY[k]) / HYP_PY[k] for k in HYP}
    db1, db2 = abs(HYP['b1'] - HYP_PY['b1']), abs(HYP['b2'] - HYP_PY['b2'])
    b1, b2, lr, eps, wd = (HYP_PY[k] for k in ('b1', 'b2', 'lr', 'eps', 'wd'))
    T = lambda b, d, t: d * t * b ** (t - 1) / (1.0 - b ** t)
    Am = torch.zeros(n, device=DEV, dtype=torch.float64)
    dm_round = torch.zeros_like(Am)      # accumulated fp32 rounding of m, absolute
    v_round = 0.0                        # ... of v, relative
    for s, (preset, tick, t) in enumerate(SCHEDULE[:5], start=1):
        if preset is not None:
            state[0] = preset
            opt.state[w]['step'] = torch.tensor(preset, dtype=opt.state[w]['step'].dtype, device=opt.state[w]['step'].device)
        g.copy_(g0 * torch.where((idx * s) % 3 == 0, -1.0, 1.0))
        p_old, w_old = p.double(), w.detach().clone()
        ops.adamw_step(p, g, m, v, state, HYP['b1'], HYP['b2'], HYP['eps'], HYP['wd'])
        w.grad = g.double()
        opt.step()
        torch.cuda.synchronize()
        upd_k, upd_t = p.double() - p_old, w.detach() - w_old
        st = opt.state[w]
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        Am = b1 * Am + (1.0 - b1) * g.double().abs()
        dm_round = b1 * dm_round + 2 * U * Am
        v_round = v_round + 3 * U
        den = st['exp_avg_sq'].sqrt() / math.sqrt(bc2) + eps
        u = (lr / bc1) * st['exp_avg'].abs() / den                       # the Adam part of torch's update
        moment = (lr / bc1) * (db1 * (1.0 / (1.0 - b1) + (s - 1) / b1) * Am + dm_round) / den + u * 0.5 * (db2 * (1.0 / (1.0 - b2) + (s - 1) / b2) + v_round)
        bias = u * (T(b1, db1, t) + 0.5 * T(b2, db2, t) + 4 * U * b1 ** t / bc1 + 2 * U * b2 ** t / bc2 + 6 * U)
        hyper = u * (rel['lr'] + rel['eps']) + w_old.abs() * lr * wd * (rel['lr'] + rel['wd'])
        own = 3 * U * w_old.abs() + 5 * U * u
        # the two trajectories' parameters differ by the deviations of the earlier steps: decay acts on that difference too (lr wd of it)
        E = bias + moment + hyper + own + (p_old - w_old).abs() * lr * wd
        dev = upd_k - upd_t
        measured = float(dev.norm() / upd_t.norm())
        derived = float(E.norm() / upd_t.norm())
        note(f'adamw.vs_torch_float64.update_rel_l2.t{t}', 'bound', measured, derived, 0, 0,
             dict(bias_correction_term=T(b1, db1, t) + 0.5 * T(b2, db2, t), d_bc2_over_bc2=T(b2, db2, t)))
        assert measured <= derived, f't = {t}: the update deviates from torch.optim.AdamW (float64) by {measured:.3e} relative L2, derived {derived:.3e}'
        gate_a(f'adamw.vs_torch_float64.update_elementwise.t{t}', upd_k, upd_t, E)


# ---------------------------------------------------------------------------------------------- 3. dropout kernels
def _away_from_zero(*shape, seed, dtype=F32):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(*shape, device=DEV, generator=gen)
    return (torch.where(x < 0, -1.0, 1.0) * (0.5 + x.abs())).to(dtype)


ELEMS = 1 << 24      # elements of a float64 slab


@pytest.mark.parametrize('dtype', [F32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('n,inplace', [(ROWS_STEP * 1024, False), (4, False), (1000 * 384 + 4, False), (1000 * 384 + 4, True)])
def test_dropout(ops, n, inplace, dtype):
    x0 = _away_from_zero(n, seed=n % 1000, dtype=dtype)
    for (p, seed) in ((0.1, SEEDS[0]), (0.5, SEEDS[1]), (0.05, SEEDS[2]), (0.0, SEEDS[1])):
        tag = f'{"bf16" if dtype == BF else "fp32"}.n{n}{".inplace" if inplace else ""}.p{p}'
        x = x0.clone()
        y = x if inplace else nan(n, dtype=dtype)
        ops.dropout(x, y, p, seed)
        torch.cuda.synchronize()
        if not inplace:
            assert torch.equal(bits(x), bits(x0))
        sc = SE.scale32(p)
        kept, worst, bad = 0, dict(ratio=-1.0), 0
        for i0 in range(0, n, ELEMS):
            i1 = min(n, i0 + ELEMS)
            want = SE.keep_range(i0, i1, p, seed, DEV)
            nbad, first = SE.mask_mismatch(y[i0:i1] != 0, want)
            assert nbad == 0, f'dropout.{tag}: {nbad} keep decisions differ from dropmask.keep, the first at element {i0 + first}'
            kept += int(want.sum())
            # a kept value is x * sc with sc = 1.0f / (1.0f - p) the kernel's fp32 scalar (two correctly rounded operations, restated by
            # steperr.scale32): ONE fp32 rounding of the product, + the bf16 store rounding of the rounded product
            ref = x0[i0:i1].double() * sc * want
            bound = (U * ref.abs()) if dtype == F32 else (LE.R_BF16 * ref.abs() + (1 + LE.R_BF16) * U * ref.abs())
            b = LE.bound_check(y[i0:i1].reshape(-1, 1), ref.reshape(-1, 1), bound.reshape(-1, 1))
            bad += b['violations']
            if b['ratio'] > worst['ratio']:
                worst = dict(b, row=b['row'] + i0)
        note(f'dropout.{tag}', 'bound', worst['ratio'], 1.0, worst['row'], 0, dict(violations=bad, kept_fraction=kept / n))
        assert bad == 0, f'dropout.{tag}: {bad} kept values outside one rounding, element {worst["row"]}'
        if p == 0.0 and dtype == F32:
            assert torch.equal(bits(y), bits(x0)), 'p = 0 is the identity'
        if n == ROWS_STEP * 1024 and p > 0:
            assert SE.kept_fraction_ok(kept, n, SE.f32(p)), f'dropout.{tag}: kept fraction {kept / n} outside 4 sigma of {1 - p}: not a usable input'
    if n == ROWS_STEP * 1024:
        y = nan(n, dtype=dtype)
        thrice(f'dropout.{"bf16" if dtype == BF else "fp32"}.n{n}', lambda: ops.dropout(x0, y, 0.1, SEEDS[1]), [y])
    with pytest.raises(RuntimeError):
        ops.dropout(x0[:6] if n > 4 else torch.ones(6, device=DEV, dtype=dtype), nan(6, dtype=dtype), 0.1, 1)


PP = [(0.1, 0.0), (0.0, 0.2), (0.1, 0.2), (0.0, 0.0), (0.5, 0.5)]


@pytest.mark.parametrize('rows,C,rps', [(ROWS_STEP, 512, 17), (ROWS_STEP, 256, 17), (33 * 17 + 5, 512, 17), (33 * 17 + 5, 256, 1)])
def test_residual_and_grad_drop(ops, rows, C, rps):
    x = rnd(rows, C, seed=3) if rows < 10000 else torch.randn(rows, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    branch = _away_from_zero(rows, C, seed=4)
    y0 = x + branch            # what the fused epilogue leaves: y0 - x is at least 0.5 - rounding in magnitude, so y != x marks a kept element
    step = max(1, ELEMS // C)
    for ci, (p, pp) in enumerate(PP):
        seed, seed_path = SEEDS[ci % 3], SEEDS[(ci + 1) % 3]
        tag = f'rows{rows}.C{C}.rps{rps}.p{p}.pp{pp}'
        y = y0.clone()
        ops.residual_drop(y, x, rps, p, seed, pp, seed_path)
        d32, d16 = nan(rows, C, dtype=F32), nan(rows, C)
        ops.grad_drop(branch, d32, rps, p, seed, pp, seed_path)
        ops.grad_drop(branch, d16, rps, p, seed, pp, seed_path)
        torch.cuda.synchronize()
        mult = SE.branch_mult32(p, pp)
        worst = {k: dict(ratio=-1.0) for k in ('residual', 'grad32', 'grad16')}
        viol = dict.fromkeys(worst, 0)
        kept_e = n_e = kept_f = 0
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            want = SE.branch_keep(r0, r1, C, rps, p, seed, pp, seed_path, DEV)
            fwd, b32, b16 = y[r0:r1] != x[r0:r1], d32[r0:r1] != 0, d16[r0:r1] != 0
            for nm, k in (('residual_drop', fwd), ('grad_drop fp32', b32), ('grad_drop bf16', b16)):
                nbad, first = SE.mask_mismatch(k, want)
                assert nbad == 0, f'{nm}.{tag}: {nbad} keep decisions differ from dropmask.keep (element mask on row * C + col, DropPath on row // {rps}), the first at row {r0 + first // C}, col {first % C}'
            assert torch.equal(fwd, b32) and torch.equal(fwd, b16), f'{tag}: forward and backward zero patterns differ'
            xd, dd = x[r0:r1].double(), y0[r0:r1].double() - x[r0:r1].double()
            # residual_drop: d = fl(y - x) rounds once (U |y - x|) and is multiplied by m; fma(d, m, x) rounds once (U |result|); a dropped
            # element is fma(d, 0, x) = x exactly.  p = p_path = 0: untouched.
            ref = xd + dd * mult * want
            bound = (U * dd.abs() * mult * want + U * ref.abs()) * (1 + U)
            if p == 0.0 and pp == 0.0:
                ref, bound = y0[r0:r1].double(), torch.zeros_like(ref)
            # grad_drop: dy * m with m the kernel's fp32 product of the two scales (steperr.branch_mult32): ONE rounding, + the bf16 store
            gref = branch[r0:r1].double() * mult * want
            for nm, got, rf, bd in (('residual', y[r0:r1], ref, bound), ('grad32', d32[r0:r1], gref, U * gref.abs()),
                                    ('grad16', d16[r0:r1], gref, LE.R_BF16 * gref.abs() + (1 + LE.R_BF16) * U * gref.abs())):
                b = LE.bound_check(got, rf, bd) if float(bd.max()) > 0 else dict(ratio=0.0 if torch.equal(got.double(), rf) else float('inf'), row=0, col=0,
                                                                                   violations=int((got.double() != rf).sum()))
                viol[nm] += b['violations']
                if b['ratio'] > worst[nm]['ratio']:
                    worst[nm] = dict(b, row=b['row'] + r0)
            if pp > 0:
                rows_kept = want.any(-1) if p < 1 else None
                n_e += int(rows_kept.sum()) * C
            else:
                n_e += (r1 - r0) * C
            kept_e += int(want.sum())
        for nm in worst:
            note(f'{nm}_drop.{tag}', 'bound', worst[nm]['ratio'], 1.0, worst[nm]['row'], worst[nm]['col'], dict(violations=viol[nm]))
            assert viol[nm] == 0, f'{nm}.{tag}: {viol[nm]} kept values outside their bound, the worst at row {worst[nm]["row"]}, col {worst[nm]["col"]}'
        if p == 0.0 and pp == 0.0:
            assert torch.equal(bits(y), bits(y0)) and torch.equal(bits(d32), bits(branch))
        if rows == ROWS_STEP:
            # conditions on the inputs: the element mask among the rows DropPath keeps, and DropPath over the frames, within 4 sigma
            if p > 0:
                assert SE.kept_fraction_ok(kept_e, n_e, SE.f32(p)), (tag, kept_e / n_e)
            if pp > 0:
                frames = -(-rows // rps)
                kf = int(SE.keep_range(0, frames, pp, seed_path, DEV).sum())
                assert SE.kept_fraction_ok(kf, frames, SE.f32(pp)), (tag, kf / frames)
    if rows == ROWS_STEP and C == 512:
        y = y0.clone()

        def launch():
            y.copy_(y0)
            ops.residual_drop(y, x, rps, 0.1, SEEDS[1], 0.2, SEEDS[0])
            ops.grad_drop(branch, d32, rps, 0.1, SEEDS[1], 0.2, SEEDS[0])
            ops.grad_drop(branch, d16, rps, 0.1, SEEDS[1], 0.2, SEEDS[0])
        thrice(f'branch_drop.rows{rows}.C{C}', launch, [y, d32, d16])


def test_drop_kernels_refuse_bad_arguments(ops):
    y, x = torch.ones(8, 6, device=DEV), torch.ones(8, 6, device=DEV)
    with pytest.raises(RuntimeError):
        ops.residual_drop(y, x, 17, 0.1, 1, 0.1, 2)      # C % 4 != 0
    with pytest.raises(RuntimeError):
        ops.grad_drop(y, torch.ones(8, 6, device=DEV), 17, 0.1, 1, 0.1, 2)
    with pytest.raises(RuntimeError):
        ops.residual_drop(torch.ones(8, 8, device=DEV), torch.ones(8, 8, device=DEV), 0, 0.1, 1, 0.1, 2)      # rows_per_sample 0


# ---------------------------------------------------------------------------------------------- 4. pool kernels
@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
@pytest.mark.parametrize('N,Mp,T,J,R', [(32, 2, 243, 17, 512), (1, 1, 1, 17, 512), (3, 2, 27, 5, 64), (2, 1, 5, 3, 516)])
def test_pool_kernels(ops, N, Mp, T, J, R, p):
    seed = SEEDS[1]
    ntok, K = N * Mp * T * J, Mp * T
    gen = torch.Generator(device=DEV).manual_seed(N + R)
    rep = torch.tanh(torch.randn(ntok, R, device=DEV, generator=gen))      # the backbone's tanh output
    dpool = torch.randn(N, J, R, device=DEV, generator=gen)
    pooled = nan(N, J, R, dtype=F32)
    d32, d16 = nan(ntok, R, dtype=F32), nan(ntok, R)
    ops.pool_rep_fwd(rep, pooled, N, Mp, T, J, p, seed)
    ops.tanh_pool_bwd(dpool, rep, d32, N, Mp, T, J, p, seed)
    ops.tanh_pool_bwd(dpool, rep, d16, N, Mp, T, J, p, seed)
    ones, zeros, back = torch.ones(N, J, R, device=DEV), torch.zeros(ntok, R, device=DEV), nan(ntok, R, dtype=F32)
    fwd1 = nan(N, J, R, dtype=F32)
    ops.pool_rep_fwd(torch.ones(ntok, R, device=DEV), fwd1, N, Mp, T, J, p, seed)
    ops.tanh_pool_bwd(ones, zeros, back, N, Mp, T, J, p, seed)
    torch.cuda.synchronize()
    tag = f'N{N}Mp{Mp}T{T}J{J}R{R}.p{p}'
    p32 = SE.f32(p)
    s64 = (1.0 / (1.0 - p32) if p > 0 else 1.0) / K      # the exact scalar; the kernels' fp32 one carries three roundings (1 - p, 1 / ., / (Mp T))
    per = Mp * T * J * R                                  # elements of one n
    nstep = max(1, ELEMS // per)
    for n0 in range(0, N, nstep):
        n1 = min(N, n0 + nstep)
        keep = SE.keep_range(n0 * per, n1 * per, p, seed, DEV).reshape(n1 - n0, K, J, R).double()
        r5 = rep[n0 * K * J:n1 * K * J].double().reshape(n1 - n0, K, J, R)
        # forward: a serial chain of K = Mp T fma, each partial sum bounded by amp = sum |kept rep|: K U amp; the product with s: U; s itself 3 U
        x, amp = (r5 * keep).sum(1) * s64, (r5.abs() * keep).sum(1) * s64
        gate_a(f'pool_rep_fwd.{tag}.n{n0}', pooled[n0:n1], x, (4 * U * x.abs() + K * U * amp) * (1 + U), where=lambda i: (n0 * J + i // R, i % R))
        # the forward on ones = (kept count) s; the backward with rep = 0, dpooled = 1 writes keep s per element: summed over (m, t) in float64
        # it must be the forward within the forward's bound -- the same mask in both passes
        cnt = keep.sum(1) * s64
        gate_a(f'pool_rep_fwd.ones.{tag}.n{n0}', fwd1[n0:n1], cnt, (4 * U * cnt + K * U * cnt) * (1 + U))
        bsum = back[n0 * K * J:n1 * K * J].double().reshape(n1 - n0, K, J, R).sum(1)
        gate_a(f'pool.same_mask.{tag}.n{n0}', bsum, fwd1[n0:n1].double(), (4 * U * cnt + K * U * cnt) * (1 + U) + 4 * U * cnt)
        assert torch.equal(back[n0 * K * J:n1 * K * J].reshape(n1 - n0, K, J, R) != 0, keep != 0), f'tanh_pool_bwd.{tag}: the mask differs from dropmask.keep'
        # backward: d km (1 - r r): d km rounds once, r r once, 1 - r r once (absolute U each on values <= 1: 2 U |d km| in all), the last
        # product once; s itself 3 U  ->  5 U |x| + 2 U |d s keep|; + the bf16 store
        dd = dpool[n0:n1].double()[:, None] * s64 * keep
        xb = dd * (1.0 - r5 * r5)
        bb = (5 * U * xb.abs() + 2 * U * dd.abs()) * (1 + U)
        sl = slice(n0 * K * J, n1 * K * J)
        gate_a(f'tanh_pool_bwd.fp32.{tag}.n{n0}', d32[sl], xb.reshape(-1, R), bb.reshape(-1, R), where=lambda i: (n0 * K * J + i // R, i % R))
        gate_a(f'tanh_pool_bwd.bf16.{tag}.n{n0}', d16[sl], xb.reshape(-1, R), (LE.R_BF16 * xb.abs() + (1 + LE.R_BF16) * bb).reshape(-1, R),
               where=lambda i: (n0 * K * J + i // R, i % R))
    if N == 32 and p == 0.1:
        thrice(f'pool.{tag}', lambda: (ops.pool_rep_fwd(rep, pooled, N, Mp, T, J, p, seed), ops.tanh_pool_bwd(dpool, rep, d32, N, Mp, T, J, p, seed),
                                       ops.tanh_pool_bwd(dpool, rep, d16, N, Mp, T, J, p, seed)), [pooled, d32, d16])


def test_pool_kernels_refuse_a_width_that_is_no_multiple_of_4(ops):
    rep = torch.zeros(2 * 3, 6, device=DEV)
    with pytest.raises(RuntimeError):
        ops.pool_rep_fwd(rep, nan(1, 3, 6, dtype=F32), 1, 1, 2, 3, 0.0, 0)
    with pytest.raises(RuntimeError):
        ops.tanh_pool_bwd(torch.zeros(1, 3, 6, device=DEV), rep, nan(6, 6, dtype=F32), 1, 1, 2, 3, 0.0, 0)
