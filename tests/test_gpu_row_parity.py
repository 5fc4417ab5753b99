"""Float64 parity of the kernels of csrc/elementwise.hip between the GEMMs and the loss, on a real MI355X, at the smallest shapes that reach
every path of their launchers: embedding forward / backward, LayerNorm forward / backward (and their operand-plane forms), adaptive
fusion (plain, with its fused LayerNorms, backward, backward from a bf16 pair), regression head, tanh backward, average.  The treatment
of tests/test_gpu_step_parity.py, with tests/rowerr.py holding the references, the rounding models and the derived bounds:

  (A) every element within a worst-case bound derived from the operation count; for the reduced outputs (dgamma, dbeta, the embedding,
      fusion and head parameter gradients) the bound follows the kernel's summation structure
  (B) row outputs of the normalising and fusion kernels: the worst row within 2 x the worst row of the rounding model, both against
      float64, every row within per_unit_excess, and no row of the model on the floor
  bits  where a value is a copy: bf16 copies, operand planes, the *_pair entries, fuse_ln_fwd's fused row, average, constant rows
  every output is allocated NaN-filled with a 64-element guard band: the payload must come back finite, the band untouched

The checker's own tests (seeded corruptions on the CPU): tests/test_rowerr.py.  Everything measured goes to row_parity.json / .txt in
MBX_REPORT_DIR (default reports/), with the module's wall time."""
import json
import os
import time

import pytest
import torch

from tests import localerr as LE
from tests import rowerr as RE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
EPS = RE.f32(1e-6)
REPORT = {}
TN = {F32: 'f32', BF: 'bf16'}
RT = {F32: LE.R_F32, BF: LE.R_BF16}


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
    rep = dict(REPORT)
    rep['_wall_seconds'] = time.time() - t0
    other = os.path.join(out, 'step_parity.json')
    if os.path.exists(other):
        with open(other) as f:
            rep['_step_parity_wall_seconds'] = json.load(f).get('_wall_seconds')
    with open(os.path.join(out, 'row_parity.json'), 'w') as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'row_parity.txt'), 'w') as f:
        f.write(f'{"output":84s} {"gate":>10s} {"value":>10s} {"against":>10s} {"ratio":>9s}  worst unit (row, col)\n')
        for k in sorted(rep):
            v = rep[k]
            if isinstance(v, dict) and 'ratio' in v:
                f.write(f'{k:84s} {v["gate"]:>10s} {v["value"]:10.3e} {v["against"]:10.3e} {v["ratio"]:9.3f}  ({v["row"]}, {v["col"]})\n')
        worst = {}
        for k, v in rep.items():
            if isinstance(v, dict) and 'ratio' in v and v['gate'] != 'bits':
                fam = k.split('.')[0] + ' / ' + v['gate']
                if v['ratio'] > worst.get(fam, ('', -1.0))[1]:
                    worst[fam] = (k, v['ratio'])
        f.write('worst ratio per kernel family and gate:\n')
        for fam in sorted(worst):
            f.write(f'  {fam:32s} {worst[fam][1]:9.3f}  {worst[fam][0]}\n')
        f.write(f'wall time of the module: {rep["_wall_seconds"]:.1f} s\n')
        sp = rep.get('_step_parity_wall_seconds')
        f.write(f'wall time of test_gpu_step_parity.py (its own report in this directory): {f"{sp:.1f} s" if sp else "not recorded here"}\n')


def note(name, gate, value, against, row, col, extra=None):
    REPORT[name] = dict(gate=gate, value=value, against=against, ratio=value / max(against, 1e-300), row=row, col=col, **(extra or {}))


def gate_a(name, got, x64, bound64):
    """every element within its bound; the worst element's (row, column) in the output's own 2-D shape"""
    cols = got.shape[-1] if got.dim() > 1 else 1
    b = LE.bound_check(got.reshape(-1, 1), x64.reshape(-1, 1), bound64.expand(x64.shape).reshape(-1, 1))
    d = float((got.double().reshape(-1)[b['row']] - x64.reshape(-1)[b['row']]).abs())
    print(f'{name}: bound ratio {b["ratio"]:.3f} (|err| {d:.3e}) at element {divmod(b["row"], cols)}')
    note(name, 'bound', d, d / max(b['ratio'], 1e-300) if b['ratio'] > 0 else float(bound64.max()), b['row'] // cols, b['row'] % cols,
         dict(violations=b['violations']))
    assert b['violations'] == 0, f'{name}: {b["violations"]} elements outside the bound, the worst at {b["ratio"]:.3f} x, element {divmod(b["row"], cols)}'


def gate_b(name, got, ref64, model):
    g, m, px, ok, msg = RE.gate_rows(got, ref64, model)
    print(f'{name}: {msg}')
    note(name, '2 x model', g['worst'], m['worst'], g['row'], 0, dict(exempt=m['exempt'], model_mean=m['mean'], n_units=g['n_units']))
    note(name + '.per_unit', 'per-unit', px['excess'], 1.0, px['row'], 0, dict(n_over=px['n_over']))
    assert m['exempt'] == 0, f'{name}: {m["exempt"]:.2%} of the model\'s rows on the floor (badly chosen input)'
    assert ok, f'{name}: {msg}'


def exact(name, got, want):
    same = RE.same_bits(got, want)
    bad = 0 if same else int((RE.bits(got) != RE.bits(want)).sum()) if got.shape == want.shape and got.dtype == want.dtype else -1
    first = int(torch.nonzero((RE.bits(got) != RE.bits(want)).reshape(-1))[0]) if bad > 0 else 0
    cols = got.shape[-1] if got.dim() > 1 else 1
    note(name, 'bits', float(bad), 0.0, first // cols, first % cols)
    assert same, f'{name}: {bad} elements differ in their bits, the first at {divmod(first, cols)}'


class Outs:
    """NaN-filled outputs with a guard band; check() after the launch: payload finite, band untouched"""

    def __init__(self, tag):
        self.tag, self.items = tag, []

    def new(self, name, shape, dtype=F32):
        p, buf = RE.guarded(tuple(shape), dtype, DEV)
        self.items.append((name, p, buf))
        return p

    def check(self):
        for name, p, buf in self.items:
            assert bool(torch.isfinite(p.float()).all()), f'{self.tag}.{name}: {int((~torch.isfinite(p.float())).sum())} elements of the payload not written'
            assert RE.guard_intact(buf), f'{self.tag}.{name}: the guard band behind the output was written'
        REPORT[self.tag + '.sentinels'] = f'{len(self.items)} outputs finite, guard bands intact'
        self.items = []


def rnd(*shape, seed=0, dtype=F32, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


# ---------------------------------------------------------------------------------------------- 1. LayerNorm
LN_M = [1, 3, 4, 5, 306, 4095, 4097, 8191, 8193, 12291]
LN_C = [64, 252, 256, 260, 512, 516, 1024, 2048]
LN_SHAPES = sorted({(M, C) for M in LN_M for C in (64, 260)} | {(8193, C) for C in LN_C})


def _ln_case(ops, tag, x, g, b, dtypes=(F32, BF)):
    M, C = x.shape
    ref, mu64, rs64 = RE.ln_fwd_ref64(x, g, b, EPS)
    bm, br = RE.ln_stat_bounds(x, EPS)
    for dt in dtypes:
        o = Outs(f'ln_fwd.{tag}.{TN[dt]}')
        y, mean, rstd = o.new('y', (M, C), dt), o.new('mean', (M,)), o.new('rstd', (M,))
        ops.layernorm_fwd(x, g, b, EPS, y, mean, rstd)
        o.check()
        model = RE.ln_fwd_model(x, g, b, EPS, dt)
        gate_b(f'ln_fwd.y.{tag}.{TN[dt]}', y, ref, model[0])
        gate_a(f'ln_fwd.mean.{tag}.{TN[dt]}', mean, mu64, bm)
        gate_a(f'ln_fwd.rstd.{tag}.{TN[dt]}', rstd, rs64, br)
    return RE.ln_fwd_model(x, g, b, EPS, F32)


@pytest.mark.parametrize('M,C', LN_SHAPES)
def test_layernorm(ops, M, C):
    x, g, b = RE.ln_inputs(M, C, seed=M + C, device=DEV)
    tag = f'M{M}.C{C}'
    _, mean, rstd = _ln_case(ops, tag, x, g, b)
    dres, extra = rnd(M, C, seed=5), rnd(M, C, seed=6)
    for dt in (F32, BF):
        dy = rnd(M, C, seed=4, dtype=dt)
        bg, bb = RE.ln_bwd_param_bounds(dy, x, mean, rstd)
        for kind, (dr, ex) in (('res', (dres, extra)), ('bare', (None, None))):
            t = f'{kind}.{tag}.{TN[dt]}'
            o = Outs(f'ln_bwd.{t}')
            dx, dx_t, dg, db = o.new('dx', (M, C)), o.new('dx_t', (M, C), dt), o.new('dgamma', (C,)), o.new('dbeta', (C,))
            ops.layernorm_bwd(dy, x, mean, rstd, g, dr, ex, dx, dx_t, dg, db)
            o.check()
            r64 = RE.ln_bwd_ref64(dy, x, mean, rstd, g, dr, ex)
            model = RE.ln_bwd_model(dy, x, mean, rstd, g, dr, ex)
            gate_b(f'ln_bwd.dx.{t}', dx, r64[0], model[0])
            exact(f'ln_bwd.dx_t.{t}', dx_t, RE.bf16_store(dx) if dt == BF else dx)
            gate_a(f'ln_bwd.dgamma.{t}', dg, r64[1], bg)
            gate_a(f'ln_bwd.dbeta.{t}', db, r64[2], bb)


@pytest.mark.parametrize('C', [260, 512])
def test_layernorm_plain_and_planes(ops, C):
    """gamma = beta = None (plain normalisation), and the hi / lo operand planes of both directions against the fp32-mode launch"""
    M = 8193
    x, g, b = RE.ln_inputs(M, C, seed=C, device=DEV)
    _ln_case(ops, f'plain.M{M}.C{C}', x, None, None)
    for kind, (gg, bb_) in (('affine', (g, b)), ('plain', (None, None))):
        o = Outs(f'ln_fwd_planes.{kind}.C{C}')
        y, mean, rstd = o.new('y', (M, C)), o.new('mean', (M,)), o.new('rstd', (M,))
        hi, lo, mean2, rstd2 = o.new('hi', (M, C), BF), o.new('lo', (M, C), BF), o.new('mean2', (M,)), o.new('rstd2', (M,))
        ops.layernorm_fwd(x, gg, bb_, EPS, y, mean, rstd)
        ops.layernorm_fwd(x, gg, bb_, EPS, (hi, lo), mean2, rstd2)
        o.check()
        wh, wl = RE.split_planes(y)
        exact(f'ln_fwd_planes.hi.{kind}.C{C}', hi, wh)
        exact(f'ln_fwd_planes.lo.{kind}.C{C}', lo, wl)
        exact(f'ln_fwd_planes.mean.{kind}.C{C}', mean2, mean)
        exact(f'ln_fwd_planes.rstd.{kind}.C{C}', rstd2, rstd)
    dy, dres = rnd(M, C, seed=7), rnd(M, C, seed=8)
    for kind, dr in (('res', dres), ('bare', None)):
        o = Outs(f'ln_bwd_planes.{kind}.C{C}')
        a = [o.new('dx', (M, C)), o.new('dx_t', (M, C)), o.new('dg', (C,)), o.new('db', (C,))]
        p = [o.new('dx2', (M, C)), (o.new('hi', (M, C), BF), o.new('lo', (M, C), BF)), o.new('dg2', (C,)), o.new('db2', (C,))]
        ops.layernorm_bwd(dy, x, mean, rstd, g, dr, None, *a)
        ops.layernorm_bwd(dy, x, mean, rstd, g, dr, None, *p)
        o.check()
        wh, wl = RE.split_planes(a[0])
        exact(f'ln_bwd_planes.hi.{kind}.C{C}', p[1][0], wh)
        exact(f'ln_bwd_planes.lo.{kind}.C{C}', p[1][1], wl)
        for n, u, v in (('dx', p[0], a[0]), ('dgamma', p[2], a[2]), ('dbeta', p[3], a[3])):
            exact(f'ln_bwd_planes.{n}.{kind}.C{C}', u, v)


@pytest.mark.parametrize('offset', [0.0, 40.0, -300.0])
def test_layernorm_rows_with_a_common_offset(ops, offset):
    for C in (64, 516):
        x, g, b = RE.ln_inputs(8193, C, seed=17, device=DEV, offset=offset)
        _ln_case(ops, f'offset{offset:g}.M8193.C{C}', x, g, b)


@pytest.mark.parametrize('C', [64, 256, 512])
def test_layernorm_constant_row_is_exact(ops, C):
    """every element 0.375: the row sum is exact at these widths, so mean = 0.375, v = 0, y = beta and rstd = fl(1 / fl(sqrt(fl(eps)))), in bits"""
    M = 5
    _, g, b = RE.ln_inputs(M, C, seed=3, device=DEV)
    x = torch.full((M, C), 0.375, device=DEV)
    o = Outs(f'ln_fwd.constant.C{C}')
    y, mean, rstd = o.new('y', (M, C)), o.new('mean', (M,)), o.new('rstd', (M,))
    ops.layernorm_fwd(x, g, b, EPS, y, mean, rstd)
    o.check()
    exact(f'ln_fwd.constant.mean.C{C}', mean, torch.full((M,), 0.375, device=DEV))
    exact(f'ln_fwd.constant.y.C{C}', y, b.expand(M, C).contiguous())
    exact(f'ln_fwd.constant.rstd.C{C}', rstd, (1.0 / torch.sqrt(torch.full((M,), EPS, dtype=F32, device=DEV))))


# ---------------------------------------------------------------------------------------------- 2. embedding
EMBF = [(512, 5, 243, 17, 3), (256, 8, 243, 17, 3), (64, 32, 243, 17, 3), (1024, 2, 243, 17, 3), (64, 600, 1, 16, 3), (64, 3, 7, 5, 3),
        (192, 3, 7, 17, 3), (512, 5, 243, 17, 2), (512, 5, 243, 17, 4)]


@pytest.mark.parametrize('C,B,T,J,Din', EMBF)
def test_embed_fwd(ops, C, B, T, J, Din):
    x, w, b, pos, temp = RE.embed_inputs(B, T, J, Din, C, seed=C + B + Din, device=DEV)
    tag = f'C{C}.B{B}.T{T}.J{J}.Din{Din}'
    M = B * T * J
    o = Outs(f'embed_fwd.{tag}')
    h = o.new('h', (M, C))
    ops.embed_fwd(x, w, b, pos, temp, h, B, T, J)
    o.check()
    ref, bound = RE.embed_fwd_ref64(x, w, b, pos, temp, B, T, J), RE.embed_fwd_bound(x, w, b, pos, temp, B, T, J)
    gate_a(f'embed_fwd.h.{tag}', h, ref, bound)
    for n, hh, rr, bb_ in zip(('first_row_of_clip', 'last_row_of_clip'), RE.clip_edges(h, B, T, J), RE.clip_edges(ref, B, T, J), RE.clip_edges(bound, B, T, J)):
        gate_a(f'embed_fwd.h.{n}.{tag}', hh.contiguous(), rr.contiguous(), bb_.contiguous())


EMBB = [(512, 17, 3, 17), (512, 1, 3, 17), (64, 129, 3, 17), (1024, 9, 2, 17), (2048, 2, 2, 5), (12, 3, 2, 17), (256, 2, 243, 17), (64, 2, 1, 17)]


@pytest.mark.parametrize('C,B,T,J', EMBB)
def test_embed_bwd(ops, C, B, T, J):
    Din, M, maxlen = 3, B * T * J, T + 3
    x, w, _, _, _ = RE.embed_inputs(B, T, J, Din, C, seed=C + B, device=DEV)
    tag = f'C{C}.B{B}.T{T}.J{J}'
    dh_a, dh_b = rnd(M, C, seed=7, dtype=BF), rnd(M, C, seed=8, dtype=BF, scale=0.3)
    shapes = dict(dw=(C, Din), db=(C,), dpos=(1, J, C), dtemp=(1, maxlen, 1, C))

    def launch(kind, fn, with_dx):
        o = Outs(f'embed_bwd.{kind}.{tag}')
        outs = {k: o.new(k, s) for k, s in shapes.items()}
        outs['dx'] = o.new('dx', (M, Din)) if with_dx else None
        fn(outs)
        o.check()
        assert float(outs['dtemp'][0, T:].abs().max()) == 0.0, f'embed_bwd.{kind}.{tag}: dtemp rows >= T are not the zeros the wrapper wrote'
        return outs

    for dhk, dh in (('f32', rnd(M, C, seed=6)), ('pairsum', dh_a.float() + dh_b.float())):
        got = launch(dhk, lambda o: ops.embed_bwd(dh, x, w, o['dw'], o['db'], o['dpos'], o['dtemp'], o['dx'], B, T, J), True)
        ref, bnd = RE.embed_bwd_ref64(dh, x, w, B, T, J), RE.embed_bwd_bounds(dh, x, w, B, T, J)
        for k in ('dw', 'db', 'dpos', 'dx'):
            gate_a(f'embed_bwd.{k}.{dhk}.{tag}', got[k].reshape(ref[k].shape), ref[k], bnd[k])
        gate_a(f'embed_bwd.dtemp.{dhk}.{tag}', got['dtemp'][0, :T, 0], ref['dtemp'], bnd['dtemp'])
        nodx = launch(dhk + '.nodx', lambda o: ops.embed_bwd(dh, x, w, o['dw'], o['db'], o['dpos'], o['dtemp'], None, B, T, J), False)
        for k in shapes:
            exact(f'embed_bwd.{k}.{dhk}.nodx.{tag}', nodx[k], got[k])
    for with_dx in (True, False):
        pair = launch('pair' + ('' if with_dx else '.nodx'),
                      lambda o: ops.embed_bwd_pair(dh_a, dh_b, x, w, o['dw'], o['db'], o['dpos'], o['dtemp'], o['dx'], B, T, J), with_dx)
        for k in list(shapes) + (['dx'] if with_dx else []):
            exact(f'embed_bwd_pair.{k}{"" if with_dx else ".nodx"}.{tag}', pair[k], got[k])


# ---------------------------------------------------------------------------------------------- 3. adaptive fusion
FUSE_SHAPES = [(1, 64), (5, 64), (8191, 64), (8193, 64), (16389, 64), (8193, 260), (8193, 512), (8193, 1024)]


def _fuse_fwd_gates(ops, tag, x_st, x_ts, w, b):
    M, C = x_st.shape
    o = Outs(f'fuse_fwd.{tag}')
    out, alpha = o.new('out', (M, C)), o.new('alpha', (M, 2))
    ops.fuse_fwd(x_st, x_ts, w, b, out, alpha)
    o.check()
    out64, a64, l64, amp = RE.fuse_fwd_ref64(x_st, x_ts, w, b)
    m_out, m_alpha = RE.fuse_fwd_model(x_st, x_ts, w, b)
    ab = RE.fuse_alpha_bound(amp, C, m_alpha, a64)
    cols = alpha.shape[-1]
    chk = LE.bound_check(alpha.reshape(-1, 1), a64.reshape(-1, 1), ab.expand(M, 2).reshape(-1, 1))
    REPORT[f'fuse_fwd.alpha.{tag}.worst_row'] = dict(row=chk['row'] // cols, gap=float(l64[chk['row'] // cols, 0] - l64[chk['row'] // cols, 1]), bound_ratio=chk['ratio'])
    gate_a(f'fuse_fwd.alpha.{tag}', alpha, a64, ab.expand(M, 2))
    gate_b(f'fuse_fwd.out.{tag}', out, out64, m_out)
    return out, alpha, l64


@pytest.mark.parametrize('M,C', FUSE_SHAPES)
def test_fuse_fwd_and_fuse_ln_fwd(ops, M, C):
    x_st, x_ts, w, b = RE.fuse_inputs(M, C, seed=M + C, device=DEV)
    tag = f'M{M}.C{C}'
    out, alpha, _ = _fuse_fwd_gates(ops, tag, x_st, x_ts, w, b)
    _, g1, b1 = RE.ln_inputs(1, C, seed=21, device=DEV)
    _, g2, b2 = RE.ln_inputs(1, C, seed=22, device=DEV)
    bm, br = RE.ln_stat_bounds(out, EPS)
    _, mu64, rs64 = RE.ln_fwd_ref64(out, None, None, EPS)
    for dt in (F32, BF):
        for kind, (p1, p2) in (('two', ((g1, b1), (g2, b2))), ('one', ((g1, b1), None)), ('plain', ((None, None), None))):
            t = f'{kind}.{tag}.{TN[dt]}'
            o = Outs(f'fuse_ln_fwd.{t}')
            out2, alpha2, xn1 = o.new('out', (M, C)), o.new('alpha', (M, 2)), o.new('xn1', (M, C), dt)
            xn2 = o.new('xn2', (M, C), dt) if p2 else None
            mean, rstd = o.new('mean', (M,)), o.new('rstd', (M,))
            ops.fuse_ln_fwd(x_st, x_ts, w, b, out2, alpha2, p1[0], p1[1], xn1, p2[0] if p2 else None, p2[1] if p2 else None, xn2, EPS, mean, rstd)
            o.check()
            exact(f'fuse_ln_fwd.out.{t}', out2, out)
            exact(f'fuse_ln_fwd.alpha.{t}', alpha2, alpha)
            # the LayerNorm part is judged on the fused row the same launch stored (gated above): it is the row the kernel holds in registers
            gate_a(f'fuse_ln_fwd.mean.{t}', mean, mu64, bm)
            gate_a(f'fuse_ln_fwd.rstd.{t}', rstd, rs64, br)
            for n, xn, pp in (('xn1', xn1, p1), ('xn2', xn2, p2)):
                if xn is not None:
                    gate_b(f'fuse_ln_fwd.{n}.{t}', xn, RE.ln_fwd_ref64(out, pp[0], pp[1], EPS)[0], RE.ln_fwd_model(out, pp[0], pp[1], EPS, dt)[0])


def test_fuse_fwd_logit_gaps(ops):
    """rows whose l0 - l1 is 0, +-10, +-40, +-90: finite outputs, alpha within its bound, the fused row within gate B"""
    M, C = 8193, 64
    x_st, x_ts, w, b = RE.fuse_inputs(M, C, seed=31, device='cpu')
    rows, gaps = [3, 100, 101, 4097, 4098, 8190, 8192], [0.0, 10.0, -10.0, 40.0, -40.0, 90.0, -90.0]
    x_st = RE.fuse_plant_logit_gaps(x_st, x_ts, w, b, rows, gaps)
    x_st, x_ts, w, b = (t.to(DEV) for t in (x_st, x_ts, w, b))
    out, alpha, l64 = _fuse_fwd_gates(ops, 'gaps.M8193.C64', x_st, x_ts, w, b)
    got = (l64[rows, 0] - l64[rows, 1]).tolist()
    REPORT['fuse_fwd.gaps.planted'] = dict(rows=rows, gaps=got, alpha0=alpha[rows, 0].tolist())
    assert all(abs(a - g_) < 1e-3 for a, g_ in zip(got, gaps)), got


@pytest.mark.parametrize('M,C', FUSE_SHAPES)
def test_fuse_bwd(ops, M, C):
    x_st, x_ts, w, b = RE.fuse_inputs(M, C, seed=M + C, device=DEV)
    tag = f'M{M}.C{C}'
    _, alpha = RE.fuse_fwd_model(x_st, x_ts, w, b)
    dh_a, dh_b = rnd(M, C, seed=7, dtype=BF), rnd(M, C, seed=8, dtype=BF, scale=0.3)
    for dhk, dh in (('f32', rnd(M, C, seed=5)), ('pairsum', dh_a.float() + dh_b.float())):
        r64 = RE.fuse_bwd_ref64(dh, x_st, x_ts, alpha, w)
        bw, bb = RE.fuse_bwd_param_bounds(dh, x_st, x_ts, alpha, w)
        model = None
        for dt in (F32, BF):
            t = f'{dhk}.{tag}.{TN[dt]}'
            o = Outs(f'fuse_bwd.{t}')
            d_st, d_ts, st_t, ts_t = o.new('d_st', (M, C)), o.new('d_ts', (M, C)), o.new('d_st_t', (M, C), dt), o.new('d_ts_t', (M, C), dt)
            dw, db = o.new('dw', (2, 2 * C)), o.new('db', (2,))
            ops.fuse_bwd(dh, x_st, x_ts, alpha, w, d_st, d_ts, st_t, ts_t, dw, db)
            o.check()
            if model is None:       # the rounding model of the kernel that runs: which form of `dot` the compiler chose (rowerr.fuse_bwd_dot_form)
                form, model, agree = RE.fuse_bwd_dot_form(d_st, dh, x_st, x_ts, alpha, w)
                REPORT[f'fuse_bwd.dot_form.{dhk}.{tag}'] = dict(fma=bool(form), identical_elements_plain=agree[False], identical_elements_fma=agree[True], elements=M * C)
            gate_b(f'fuse_bwd.d_st.{t}', d_st, r64[0], model[0])
            gate_b(f'fuse_bwd.d_ts.{t}', d_ts, r64[1], model[1])
            exact(f'fuse_bwd.d_st_t.{t}', st_t, RE.bf16_store(d_st) if dt == BF else d_st)
            exact(f'fuse_bwd.d_ts_t.{t}', ts_t, RE.bf16_store(d_ts) if dt == BF else d_ts)
            gate_a(f'fuse_bwd.dw.{t}', dw, r64[2], bw)
            gate_a(f'fuse_bwd.db.{t}', db, r64[3], bb)
            # d_st = d_ts = None: only the T-typed copies, the same bits
            o = Outs(f'fuse_bwd.nofp32.{t}')
            st2, ts2, dw2, db2 = o.new('d_st_t', (M, C), dt), o.new('d_ts_t', (M, C), dt), o.new('dw', (2, 2 * C)), o.new('db', (2,))
            ops.fuse_bwd(dh, x_st, x_ts, alpha, w, None, None, st2, ts2, dw2, db2)
            o.check()
            for n, u, v in (('d_st_t', st2, st_t), ('d_ts_t', ts2, ts_t), ('dw', dw2, dw), ('db', db2, db)):
                exact(f'fuse_bwd.nofp32.{n}.{t}', u, v)
            if dhk == 'pairsum' and dt == BF:
                o = Outs(f'fuse_bwd_pair.{tag}')
                st3, ts3, dw3, db3 = o.new('d_st_t', (M, C), BF), o.new('d_ts_t', (M, C), BF), o.new('dw', (2, 2 * C)), o.new('db', (2,))
                ops.fuse_bwd_pair(dh_a, dh_b, x_st, x_ts, alpha, w, st3, ts3, dw3, db3)
                o.check()
                for n, u, v in (('d_st_t', st3, st_t), ('d_ts_t', ts3, ts_t), ('dw', dw3, dw), ('db', db3, db)):
                    exact(f'fuse_bwd_pair.{n}.{tag}', u, v)


# ---------------------------------------------------------------------------------------------- 4. head, tanh backward, average
@pytest.mark.parametrize('M,R,D', [(1, 64, 3), (4097, 512, 3), (8193, 260, 5), (4097, 64, 8), (5, 512, 1), (4097, 512, 4)])
def test_head(ops, M, R, D):
    rep, w, b, dout = RE.head_inputs(M, R, D, seed=M + R + D, device=DEV)
    tag = f'M{M}.R{R}.D{D}'
    o = Outs(f'head_fwd.{tag}')
    out = o.new('out', (M, D))
    ops.head_fwd(rep, w, b, out)
    o.check()
    gate_a(f'head_fwd.out.{tag}', out, RE.head_fwd_ref64(rep, w, b), RE.head_fwd_bound(rep, w, b))
    dpre64, dw64, db64 = RE.head_bwd_ref64(dout, rep, w)
    bw, bb = RE.head_bwd_param_bounds(dout, rep, M, R, D)
    drep = rnd(M, R, seed=9)
    for dt in (F32, BF):
        o = Outs(f'head_bwd.{tag}.{TN[dt]}')
        dpre, dw, db, tb = o.new('dpre', (M, R), dt), o.new('dw', (D, R)), o.new('db', (D,)), o.new('tanh_bwd', (M, R), dt)
        ops.head_bwd(dout, rep, w, dpre, dw, db)
        ops.tanh_bwd(drep, rep, tb)
        o.check()
        gate_a(f'head_bwd.dpre.{tag}.{TN[dt]}', dpre, dpre64, RE.head_dpre_bound(dout, rep, w, RT[dt]))
        gate_a(f'head_bwd.dw.{tag}.{TN[dt]}', dw, dw64, bw)
        gate_a(f'head_bwd.db.{tag}.{TN[dt]}', db, db64, bb)
        gate_a(f'tanh_bwd.{tag}.{TN[dt]}', tb, RE.tanh_bwd_ref64(drep, rep), RE.tanh_bwd_bound(drep, rep, RT[dt]))


@pytest.mark.parametrize('n', [4, 1028, 16777216 + 1200])
def test_average_and_tanh_bwd_flat(ops, n):
    """n = 16,777,216 + 1200 is the one size at which the grid-stride loops of these kernels iterate"""
    gen = torch.Generator(device=DEV).manual_seed(n)      # on the device: three 16.7M-element tensors from the host cost more than the kernels
    u, v = torch.randn(n, device=DEV, generator=gen), torch.randn(n, device=DEV, generator=gen)
    rep = torch.tanh(torch.randn(n, device=DEV, generator=gen) * 1.5)
    rep[0], rep[n - 1], rep[n // 2] = 1.0, -1.0, 0.0
    tag = f'n{n}'
    o = Outs(f'average.{tag}')
    avg = o.new('out', (n,))
    ops.average(u, v, avg)
    o.check()
    exact(f'average.out.{tag}', avg, (u + v) * 0.5)
    gate_a(f'average.out.bound.{tag}', avg, (u.double() + v.double()) * 0.5, RE.average_bound(u, v))
    for dt in (F32, BF):
        o = Outs(f'average_bwd.{tag}.{TN[dt]}')
        d_st, d_ts, st_t, ts_t, tb = o.new('d_st', (n,)), o.new('d_ts', (n,)), o.new('d_st_t', (n,), dt), o.new('d_ts_t', (n,), dt), o.new('tanh_bwd', (n,), dt)
        ops.average_bwd(u, d_st, d_ts, st_t, ts_t)
        ops.tanh_bwd(u, rep, tb)
        o.check()
        gate_a(f'average_bwd.d_st.{tag}.{TN[dt]}', d_st, u.double() * 0.5, RE.average_bwd_bound(u))
        exact(f'average_bwd.d_ts.{tag}.{TN[dt]}', d_ts, d_st)
        exact(f'average_bwd.d_st_t.{tag}.{TN[dt]}', st_t, RE.bf16_store(d_st) if dt == BF else d_st)
        exact(f'average_bwd.d_ts_t.{tag}.{TN[dt]}', ts_t, st_t)
        gate_a(f'tanh_bwd.flat.{tag}.{TN[dt]}', tb, RE.tanh_bwd_ref64(u, rep), RE.tanh_bwd_bound(u, rep, RT[dt]))
