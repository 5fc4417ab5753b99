"""Float64 parity of the weight-fold, unfold and operand-split kernels of csrc/elementwise.hip on a real MI355X: mbx_prep_weights (float,
bf16, lo plane), mbx_fold_norm_weights, mbx_lnbwd_rowc, mbx_unfold_norm_grads, mbx_split_bf16, mbx_gelu_fwd -- the kernels the bf16
training step runs once per step or once per sub-layer.  tests/folderr.py holds the references, the restatements and the bounds:

  bits    prep_weights' dst_n / dst_t, W' and W'^T of the fold, rowc, the split planes: equal to the restatement bit for bit; bias_f, rsum
          and the unfolded dw too, with the one documented exception of rowerr.fma32 (folderr.tie_gate), which is 0 for these seeds
  bound   bias_f, rsum, dgamma, dbeta: every element within gam(L) sum |terms| of the float64 value, L counted from the kernel, no margin
  4 x model   gelu_fwd: every 4-element vector within 4 x the worst float64 error of torch's fp32 erf form over the vectors of its
          |u| bin, floored at one unit roundoff of the bin's largest |gelu|
  every output is NaN-filled with a 64-element guard band behind it: the payload comes back finite, the band untouched; every entry is
  launched three times into freshly filled outputs and must give the same bits

The checker's own tests (seeded corruptions on the CPU): tests/test_folderr.py.  Everything measured goes to fold_parity_gates.json and
fold_parity.txt in MBX_REPORT_DIR (default reports/), as tests/test_gpu_row_parity.py does."""
import json
import os

import pytest
import torch

from tests import folderr as FE
from tests import rowerr as RE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
REPORT = {}


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    yield
    out = os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'fold_parity_gates.json'), 'w') as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'fold_parity.txt'), 'w') as f:
        f.write('worst value of every gated quantity of tests/test_gpu_fold_parity.py as a share of its gate (bits: elements that differ)\n')
        f.write(f'{"output":64s} {"gate":>10s} {"value":>10s} {"against":>10s} {"share":>8s}  worst unit (row, col)\n')
        for k in sorted(REPORT):
            v = REPORT[k]
            if isinstance(v, dict) and 'ratio' in v:
                f.write(f'{k:64s} {v["gate"]:>10s} {v["value"]:10.3e} {v["against"]:10.3e} {v["ratio"]:8.3f}  ({v["row"]}, {v["col"]})'
                        f'{"  " + v["more"] if v.get("more") else ""}\n')
        ties = {k: v for k, v in REPORT.items() if k.endswith('.tie_exemptions')}
        f.write(f'tie exemptions (elements that differ from the fma32 restatement; cap {FE.TIE_CAP:.0e} of the elements, and none where the '
                f'restatement has no float64 midpoint): {sum(v["differ"] for v in ties.values())} over {len(ties)} outputs, '
                f'{sum(v["ties"] for v in ties.values())} midpoints in their restatements\n')
        for k in sorted(REPORT):
            if k.endswith('.bins'):
                f.write(f'{k}: |u| bin from, units, kernel worst, model worst, floor, kernel / model\n')
                for b, (n, g, m, fl, r) in sorted(REPORT[k].items(), key=lambda t: int(t[0])):
                    f.write(f'   {int(b) * FE.GELU_BIN:5.1f} {n:8d} {g:10.3e} {m:10.3e} {fl:10.3e} {r:8.3f}\n')
        f.write('launches: ' + ', '.join(f'{k[:-len(".three_launches_identical")]}' for k in sorted(REPORT) if k.endswith('.three_launches_identical'))
                + ': three launches bit-identical, guard bands intact\n')


def note(name, gate, value, against, row, col, more=None):
    REPORT[name] = dict(gate=gate, value=value, against=against, ratio=value / max(against, 1e-300) if against else value, row=row, col=col, more=more)


def exact(name, got, want, ties=None):
    """bit-equality with the restatement; ties (a count): the fma32 exception of folderr.tie_gate applies"""
    ok, n, first = FE.tie_gate(got, want, ties or 0)
    cols = got.shape[-1] if got.dim() > 1 else 1
    print(f'{name}: {n} of {got.numel()} elements differ in their bits' + (f', the first at {divmod(first, cols)}' if n else ''))
    note(name, 'bits', float(n), 0.0, max(first, 0) // cols, max(first, 0) % cols)
    if ties is not None:
        REPORT[name + '.tie_exemptions'] = dict(differ=n, ties=ties, elements=got.numel())
    assert ok, f'{name}: {n} of {got.numel()} elements differ in their bits, the first at {divmod(first, cols)} ({ties or 0} midpoints in the restatement)'


def bounded(name, got, ref64, bound64):
    b = FE.bound_gate(got, ref64, bound64)
    cols = got.shape[-1] if got.dim() > 1 else 1
    k = b['row'] * cols + b['col']
    err, bd = float((got.double().reshape(-1)[k] - ref64.reshape(-1)[k]).abs()), float(bound64.reshape(-1)[k])
    print(f'{name}: bound ratio {b["ratio"]:.3f} (|err| {err:.3e}, bound {bd:.3e}) at element {k}, {b["violations"]} outside')
    note(name, 'bound', err, bd, b['row'], b['col'])
    assert b['violations'] == 0, f'{name}: {b["violations"]} elements outside the bound, the worst {b["ratio"]:.3f} x at element {k}'


class Outs:
    """NaN-filled outputs with a guard band; check() after the launches: payload finite, band untouched"""

    def __init__(self, tag):
        self.tag, self.items = tag, []

    def new(self, name, shape, dtype=F32):
        p, buf = RE.guarded(tuple(shape), dtype, DEV)
        self.items.append((name, p, buf))
        return p

    def refill(self):
        for _, p, _ in self.items:
            p.fill_(float('nan'))

    def check(self):
        for name, p, buf in self.items:
            assert bool(torch.isfinite(p.float()).all()), f'{self.tag}.{name}: {int((~torch.isfinite(p.float())).sum())} elements of the payload not written'
            assert RE.guard_intact(buf), f'{self.tag}.{name}: the guard band behind the output was written'


def thrice(outs, launch, reset=None):
    """three launches into freshly NaN-filled outputs, bit-identical; the outputs keep the third launch's result"""
    res = []
    for _ in range(3):
        outs.refill()
        if reset is not None:
            reset()
        launch()
        torch.cuda.synchronize()
        res.append([p.clone() for _, p, _ in outs.items])
    same = all(RE.same_bits(a, b) for r in res[1:] for a, b in zip(res[0], r))
    REPORT[outs.tag + '.three_launches_identical'] = bool(same)
    assert same, f'{outs.tag}: three launches differ'
    outs.check()


def ptr(t):
    return 0 if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- prep_weights
@pytest.mark.parametrize('need_t', [True, False])
@pytest.mark.parametrize('kind', sorted(FE.PREP_KINDS))
@pytest.mark.parametrize('shapes', [FE.DESC_SET, FE.DESC_SINGLE], ids=['set', 'single'])
def test_prep_weights(ops, shapes, kind, need_t):
    code, dt = FE.PREP_KINDS[kind]
    ws = FE.prep_inputs(shapes, seed=102, device=DEV)
    tag = f'prep_weights.{kind}.{"set" if len(shapes) > 1 else "single"}.{"nt" if need_t else "n"}'
    outs = Outs(tag)
    dn = [outs.new(f'dst_n{i}', w.shape, dt) for i, w in enumerate(ws)]
    dtr = [outs.new(f'dst_t{i}', w.t().shape, dt) if need_t else None for i, w in enumerate(ws)]
    desc = torch.tensor([[w.data_ptr(), ptr(a), ptr(b), *w.shape] for w, a, b in zip(ws, dn, dtr)], dtype=torch.int64).to(DEV)
    max_n, max_k = max(s[0] for s in shapes), max(s[1] for s in shapes)
    thrice(outs, lambda: ops._ck(ops.lib.mbx_prep_weights(desc.data_ptr(), len(ws), max_n, max_k, code, ops._stream())))
    for i, w in enumerate(ws):
        wn, wt = FE.prep_model(w, kind, need_t)
        exact(f'{tag}.{w.shape[0]}x{w.shape[1]}.dst_n', dn[i], wn)
        if need_t:
            exact(f'{tag}.{w.shape[0]}x{w.shape[1]}.dst_t', dtr[i], wt)


# ---------------------------------------------------------------------------------------------- fold_norm_weights
@pytest.mark.parametrize('need_t', [True, False])
@pytest.mark.parametrize('shapes,bias_on,seed', [(FE.DESC_SET, FE.DESC_BIAS, 101), (FE.DESC_SINGLE, (True,), 103)], ids=['set', 'single'])
def test_fold_norm_weights(ops, shapes, bias_on, seed, need_t):
    ds = FE.fold_inputs(shapes, bias_on, seed=seed, device=DEV)
    tag = f'fold_norm_weights.{"set" if len(shapes) > 1 else "single"}.{"nt" if need_t else "n"}'
    outs = Outs(tag)
    o = [dict(wn=outs.new(f'wn{i}', (N, K), BF), wt=outs.new(f'wt{i}', (K, N), BF) if need_t else None, bias_f=outs.new(f'bias_f{i}', (N,)),
              rsum=outs.new(f'rsum{i}', (N,))) for i, (N, K) in enumerate(shapes)]
    desc = torch.tensor([[d['w'].data_ptr(), ptr(d['b']), d['gamma'].data_ptr(), d['beta'].data_ptr(), ptr(q['wn']), ptr(q['wt']), ptr(q['bias_f']),
                          ptr(q['rsum']), *d['w'].shape] for d, q in zip(ds, o)], dtype=torch.int64).to(DEV)
    max_n, max_k = max(s[0] for s in shapes), max(s[1] for s in shapes)
    thrice(outs, lambda: ops._ck(ops.lib.mbx_fold_norm_weights(desc.data_ptr(), len(ds), max_n, max_k, ops._stream())))
    for d, q, (N, K) in zip(ds, o, shapes):
        t = f'{tag}.{N}x{K}'
        wn, wt = FE.fold_w_model(d, need_t)
        exact(t + '.wn', q['wn'], wn)
        if need_t:
            exact(t + '.wt', q['wt'], wt)
        bf64, rs64 = FE.fold_rows_ref64(d)
        bb, br = FE.fold_rows_bounds(d)
        bounded(t + '.bias_f', q['bias_f'], bf64, bb)
        bounded(t + '.rsum', q['rsum'], rs64, br)
        m_bias, m_rsum, ties = FE.fold_rows_model(d)
        exact(t + '.bias_f.order', q['bias_f'], m_bias, ties=ties)
        exact(t + '.rsum.order', q['rsum'], m_rsum, ties=0)          # plain additions: nothing to round twice


# ---------------------------------------------------------------------------------------------- lnbwd_rowc
@pytest.mark.parametrize('nb,M,C', FE.ROWC_CASES)
def test_lnbwd_rowc(ops, nb, M, C):
    part, rstd = FE.rowc_inputs(nb, M, seed=104 + nb, device=DEV)
    outs = Outs(f'lnbwd_rowc.nb{nb}.M{M}.C{C}')
    rowc = outs.new('rowc', (M, 4))
    thrice(outs, lambda: ops.lnbwd_rowc(part, rstd, rowc, C))
    exact(outs.tag, rowc, FE.rowc_model(part, rstd, C))
    bounded(outs.tag + '.vs_float64', rowc, FE.rowc_ref64(part, rstd, C), FE.rowc_sanity_bound(part, rstd, C) + 1e-300)


# ---------------------------------------------------------------------------------------------- unfold_norm_grads
@pytest.mark.parametrize('N,K,vec', [s + (v,) for s, v in zip(FE.UNFOLD_SHAPES, FE.UNFOLD_VEC)])
def test_unfold_norm_grads(ops, N, K, vec):
    assert FE.unfold_vec(K) == vec, 'the case is meant for the other colsum kernel'
    dwp, db, w, gamma, beta = FE.unfold_inputs(N, K, seed=105, device=DEV)
    keep = dwp.clone()                      # dgamma is formed from dw' as it was BEFORE the in-place update
    outs = Outs(f'unfold_norm_grads.{N}x{K}.{"colsum4" if vec else "colsum"}')
    dw, dg, dbt = outs.new('dw', (N, K)), outs.new('dgamma', (K,)), outs.new('dbeta', (K,))
    thrice(outs, lambda: ops.unfold_norm_grads(dw, db, w, gamma, beta, dg, dbt), reset=lambda: dw.copy_(keep))
    assert RE.same_bits(dwp, keep)
    m_dw, m_dg, m_db, ties_dw, ties_chain = FE.unfold_model(keep, db, w, gamma, beta)
    exact(outs.tag + '.dw', dw, m_dw, ties=ties_dw)
    _, dg64, db64 = FE.unfold_ref64(keep, db, w, gamma, beta)
    bg, bb = FE.unfold_bounds(keep, db, w)
    bounded(outs.tag + '.dgamma', dg, dg64, bg)
    bounded(outs.tag + '.dbeta', dbt, db64, bb)
    for n, got, m in (('dgamma', dg, m_dg), ('dbeta', dbt, m_db)):      # reported, not gated: the issue bounds these two
        REPORT[f'{outs.tag}.{n}.differs_from_ordered_model'] = dict(elements=FE.diff_count(got, m)[0], of=K, midpoints=ties_chain)


# ---------------------------------------------------------------------------------------------- split_bf16, gelu_fwd
@pytest.mark.parametrize('n', FE.FLAT_N)
def test_split_bf16(ops, n):
    x = FE.split_inputs(n, seed=106, device=DEV)
    outs = Outs(f'split_bf16.{n}')
    hi, lo = outs.new('hi', (n,), BF), outs.new('lo', (n,), BF)
    thrice(outs, lambda: ops._ck(ops.lib.mbx_split_bf16(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), n, ops._stream())))
    m_hi, m_lo = FE.split_model(x)
    exact(outs.tag + '.hi', hi, m_hi)
    exact(outs.tag + '.lo', lo, m_lo)
    assert n <= FE.first_pass(n) or n - FE.first_pass(n) == 8


@pytest.mark.parametrize('dtype', [F32, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('n', FE.FLAT_N)
def test_gelu_fwd(ops, n, dtype):
    u = FE.gelu_inputs(n, dtype, seed=107, device=DEV)
    outs = Outs(f'gelu_fwd.{"f32" if dtype == F32 else "bf16"}.{n}')
    g = outs.new('g', (n,), dtype)
    thrice(outs, lambda: ops.gelu_fwd(u, g))
    r = FE.gelu_gate(g, FE.gelu_ref64(u), FE.gelu_model(u), u)
    bins = r.pop('bins')
    tail = {b: v for b, v in bins.items() if b * FE.GELU_BIN >= 5.0}
    print(f'{outs.tag}: {r}; kernel / model per bin {[(b * FE.GELU_BIN, round(v[4], 3)) for b, v in sorted(bins.items())]}')
    note(outs.tag, '4 x model', r['ratio'], 1.0, r['unit'], r['bin'] * FE.GELU_BIN,
         more=f'worst kernel / model of a bin {max(v[4] for v in bins.values()):.3f}, in |u| >= 5 {max([v[4] for v in tail.values()] or [0.0]):.3f}')
    REPORT[outs.tag + '.bins'] = {str(b): v for b, v in bins.items()}
    assert r['n_over'] == 0, f'{outs.tag}: {r["n_over"]} vectors outside the gate, the worst {r["ratio"]:.3f} x at vector {r["unit"]} (|u| bin {r["bin"] * FE.GELU_BIN})'
