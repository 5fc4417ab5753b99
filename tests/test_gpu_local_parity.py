"""Per-row and per-tile parity gates for the pipelined bf16 kernels on a real MI355X (the metrics and their derivations: tests/localerr.py;
the checker's own tests: tests/test_localerr.py).

The per-kernel tests judge an output by one relative L2 norm over the whole tensor; a pipeline defect (a wait one too weak, a fragment
requested a stage late) corrupts a fragment, a row or one wave's tile and does not move that norm.  Here every family is judged at the
smallest units its work is divided into, against a float64 reference computed from the same operand bits, at its edge shapes and at the
training step's M = 64 * 243 * 17 = 264,384 rows:

  * outputs with ONE final rounding: the worst-case elementwise bound of localerr.elementwise_bound, every element, no margin (the
    comment at each use derives it for that epilogue); worst row and worst 32 x 32 tile are reported;
  * outputs rounded INSIDE the kernel (attention: P and dS; the fused MLP: the hidden): worst row, worst (row, head) and worst 32-row
    wave block of the kernel against the exact float64 result may not exceed 2 x the same worst unit of the rounding-model reference
    against the exact result on the same inputs -- never a number read off the kernel;
  * each family's training-step case is launched three times into freshly sentinel-filled outputs: bit-identical;
  * the floor of unit_errors may exempt at most 0.1 % of the units of any tensor.

Outputs are pre-filled with NaN; operands carry a per-row scale and offset so that neighbouring rows differ in magnitude.  Everything
measured goes to local_parity.json and a table, local_parity.txt, in the directory MBX_REPORT_DIR names (default: reports/ in the repository root,
git-ignored); none of it feeds back into a gate."""
import json
import os
import time

import pytest
import torch

from motionbert_amd.engine import EPI_DGELU, EPI_GELU, EPI_RESID, EPI_STORE, EPI_TANH, MODE_SPATIAL, MODE_TEMPORAL
from tests import localerr as LE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
REPORT = {}
M_STEP = 64 * 243 * 17          # rows of the benchmark's training step
U = LE.U32


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()      # the module's own wall time (fixture setup to teardown), whatever ran before it
    yield
    out = os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')
    os.makedirs(out, exist_ok=True)
    REPORT['_wall_seconds'] = time.time() - t0
    with open(os.path.join(out, 'local_parity.json'), 'w') as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'local_parity.txt'), 'w') as f:
        f.write(f'{"output":72s} {"gate":>10s} {"value":>10s} {"against":>10s} {"ratio":>7s}  worst unit (row, col)\n')
        for k in sorted(REPORT):
            v = REPORT[k]
            if isinstance(v, dict) and 'ratio' in v:
                f.write(f'{k:72s} {v["gate"]:>10s} {v["value"]:10.3e} {v["against"]:10.3e} {v["ratio"]:7.3f}  ({v["row"]}, {v["col"]})\n')
        for k in sorted(REPORT):
            if k.endswith('.three_launches_identical'):
                f.write(f'{k:72s} {"identical" if REPORT[k] else "DIFFER"}\n')
        f.write(f'wall time of the module: {REPORT["_wall_seconds"]:.1f} s\n')


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0, device=DEV):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(device).to(dtype)


def rows_scaled(M, K, seed, offset=0.3, device=DEV):
    """fp32 rows with a scale and an offset of their own (as test_rows_lnbwd_t builds them): neighbouring rows differ in magnitude"""
    return rnd(M, K, seed=seed, device=device) * (0.5 + rnd(M, 1, seed=seed + 101, device=device).abs()) + offset * rnd(M, 1, seed=seed + 102, device=device)


def gemm_operands(M, N, K, seed, device=DEV):
    return rows_scaled(M, K, seed, device=device).to(BF), rnd(N, K, seed=seed + 1, dtype=BF, scale=0.05, device=device), rnd(N, seed=seed + 2, scale=0.5, device=device)


def nan(*shape, dtype=BF):
    return torch.full(shape, float('nan'), device=DEV, dtype=dtype)


def note(name, gate, value, against, row, col, extra=None):
    REPORT[name] = dict(gate=gate, value=value, against=against, ratio=value / max(against, 1e-300), row=row, col=col, **(extra or {}))


def gate_once(name, got, ref_fn, geometry, units=(('row', None), ('tile', (32, 32)))):
    """One final rounding.  ref_fn(r0, r1) -> (x64, bound64) for rows r0:r1 (float64 products are made a slab of rows at a time).  Every
    element within its bound; the worst row and the worst 32 x 32 tile are recorded with their place in the kernel's geometry."""
    torch.cuda.synchronize()
    M, N = got.shape
    worst = dict(ratio=-1.0)
    viol, exempt = 0, 0.0
    wu = {u: dict(worst=-1.0) for u, _ in units}
    for r0, r1 in LE.slabs(M):
        x, bound = ref_fn(r0, r1)
        b = LE.bound_check(got[r0:r1], x, bound)
        viol += b['violations']
        if b['ratio'] > worst['ratio']:
            worst = dict(b, row=b['row'] + r0)
        for u, shp in units:
            e = LE.unit_errors(got[r0:r1], x, *(shp or (1, N)))
            exempt = max(exempt, e['exempt'])
            if e['worst'] > wu[u]['worst']:
                wu[u] = dict(e, row=e['row'] + r0)
        del x, bound
    note(name + '.elementwise', 'bound', worst['ratio'], 1.0, worst['row'], worst['col'], dict(violations=viol))
    for u, _ in units:
        note(f'{name}.{u}', 'reported', wu[u]['worst'], wu[u]['worst'], wu[u]['row'], wu[u]['col'], dict(where=str(LE.locate(wu[u]['row'], wu[u]['col'], geometry))))
    assert viol == 0, f'{name}: {viol} elements outside the elementwise bound; {LE.where(worst, geometry)}'
    assert exempt <= LE.MAX_EXEMPT, f'{name}: {exempt:.2%} of the units sit on the floor'


def gate_model(name, got, exact, model, geometry, units, seq_row=None):
    """Rounded inside the kernel: per unit, worst(kernel vs exact) <= 2 x worst(model vs exact); units = {name: (rows, cols)}"""
    torch.cuda.synchronize()
    for u, shp in units.items():
        g, m = LE.unit_errors(got, exact, *shp, full=True), LE.unit_errors(model, exact, *shp, full=True)
        x = LE.per_unit_excess(g, m, *shp)
        note(f'{name}.{u}', '2 x model', g['worst'], m['worst'], g['row'], g['col'], dict(exempt=m['exempt'], model_mean=m['mean']))
        note(f'{name}.{u}.per_unit', 'per unit', x['excess'], 1.0, x['row'], x['col'], dict(units_over=x['n_over']))
        assert m['exempt'] <= LE.MAX_EXEMPT, f'{name}.{u}: {m["exempt"]:.2%} of the units sit on the floor'
        assert g['worst'] <= 2.0 * m['worst'], (f'{name}.{u}: kernel {g["worst"]:.3e} > 2 x model {m["worst"]:.3e}; '
                                                f'{LE.where(g, geometry, seq_row)}')
        assert x['excess'] <= 1.0, (f'{name}.{u}: {x["n_over"]} units above 2 x their own model error + 2 x the model mean, the worst at '
                                    f'{x["excess"]:.2f} x: {LE.where(dict(x, worst=x["excess"]), geometry, seq_row)}')


def thrice(name, launch, outs):
    """three launches into freshly sentinel-filled outputs, bit-identical (three, fixed; tools/rows_soak.py is the tool for long soaks)"""
    res = []
    for _ in range(3):
        for o in outs:
            o.fill_(float('nan'))
        launch()
        torch.cuda.synchronize()
        res.append([o.clone() for o in outs])
    same = all(torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))
               for r in res[1:] for a, b in zip(res[0], r))
    REPORT[name + '.three_launches_identical'] = bool(same)
    assert same, f'{name}: three launches differ'


def prod(a, w, bias, r0, r1):
    """float64 product of rows r0:r1 from the bf16 operand bits and its amplitude |a| . |w|^T"""
    ad, wd = a[r0:r1].double(), w.double()
    x = ad @ wd.t()
    if bias is not None:
        x = x + bias.double()
    return x, ad.abs() @ wd.abs().t()


# ---------------------------------------------------------------------------------------------- tile GEMM 256 x 256 (gemm_nt_pp256_kernel)
STEP_NK = [(1536, 512), (1024, 512), (768, 256), (1024, 256)]      # qkv, fc1 / fc2-dX (the same pair) at dim_feat 512 and 256
EDGE_M = [255, 256, 257]


@pytest.mark.parametrize('M,N,K', [(M_STEP, n, k) for n, k in STEP_NK] + [(m, 256, 64) for m in EDGE_M] + [(257, 1536, 512)])
def test_tile256_store(ops, M, N, K):
    a, w, bias = gemm_operands(M, N, K, seed=N + K)
    out = nan(M, N)
    ops.gemm_nt(a, w, bias, EPI_STORE, out_t=out)

    def ref(r0, r1):
        # STORE: x = acc + bias: K exact products accumulated in fp32, one more fp32 add, Lipschitz constant 1, one bf16 rounding
        x, amp = prod(a, w, bias, r0, r1)
        return x, LE.elementwise_bound(x, amp, K, LE.R_BF16, lip=1.0, ops=1, mag64=amp + bias.double().abs())
    gate_once(f'tile256.store.{M}x{N}x{K}', out, ref, 'pp256')
    if M == M_STEP and (N, K) == (1536, 512):
        thrice(f'tile256.store.{M}x{N}x{K}', lambda: ops.gemm_nt(a, w, bias, EPI_STORE, out_t=out), [out])


@pytest.mark.parametrize('M,N,K', [(M_STEP, 1024, 512), (M_STEP, 1024, 256)] + [(m, 256, 64) for m in EDGE_M])
def test_tile256_gelu_forms(ops, M, N, K):
    a, w, bias = gemm_operands(M, N, K, seed=N + K + 1)
    u_t, g_t, d_t, g2_t = nan(M, N), nan(M, N), nan(M, N), nan(M, N)
    ops.gemm_nt(a, w, bias, EPI_GELU, out_t=u_t, out2_t=g_t)
    ops.gemm_nt_gelu_d(a, w, bias, d_t, g2_t)
    tag = f'{M}x{N}x{K}'

    def base(r0, r1):
        x, amp = prod(a, w, bias, r0, r1)
        return x, amp, amp + bias.double().abs()

    def ref_u(r0, r1):      # the pre-activation: STORE
        x, amp, mag = base(r0, r1)
        return x, LE.elementwise_bound(x, amp, K, LE.R_BF16, ops=1, mag64=mag)

    def ref_g(r0, r1):
        # GELU: Lipschitz constant sup |gelu'| = 1.129; the fast erf forms of gelu_fast.h are off by |u| / 2 x 3e-7 + 7e-7 absolute (as
        # stated there); three further fp32 operations on values bounded by mag (the bias add and the two of u (1 + erf) / 2)
        x, amp, mag = base(r0, r1)
        return LE.gelu64(x), LE.elementwise_bound(LE.gelu64(x), amp, K, LE.R_BF16, lip=LE.GELU_LIP, ops=3, eabs=LE.gelu_eabs(x), mag64=mag)

    def ref_d(r0, r1):
        # GELU' of the accumulator: Lipschitz constant sup |gelu''| = 2 phi(0) = 0.798 < 1; its own evaluation error gelu_grad_eabs
        x, amp, mag = base(r0, r1)
        return LE.gelu_grad64(x), LE.elementwise_bound(LE.gelu_grad64(x), amp, K, LE.R_BF16, lip=1.0, ops=1, eabs=LE.gelu_grad_eabs(x), mag64=mag)
    gate_once(f'tile256.gelu.u.{tag}', u_t, ref_u, 'pp256')
    gate_once(f'tile256.gelu.g.{tag}', g_t, ref_g, 'pp256')
    gate_once(f'tile256.gelu_d.g.{tag}', g2_t, ref_g, 'pp256')
    gate_once(f'tile256.gelu_d.d.{tag}', d_t, ref_d, 'pp256')
    if M == M_STEP and K == 512:
        thrice(f'tile256.gelu_d.{tag}', lambda: ops.gemm_nt_gelu_d(a, w, bias, d_t, g2_t), [d_t, g2_t])


@pytest.mark.parametrize('M,N,K', [(M_STEP, 1024, 512), (M_STEP, 1024, 256)] + [(m, 256, 64) for m in EDGE_M])
def test_tile256_backward_epilogues(ops, M, N, K):
    """fc2's dX with the GELU' epilogues: gemm_nt_mul (the saved derivative), EPI_DGELU and its row-dot form, and TANH (fp32 output)"""
    a, w, _ = gemm_operands(M, N, K, seed=N + K + 2)
    aux = rnd(M, N, seed=5, dtype=BF, scale=1.5)
    tag = f'{M}x{N}x{K}'
    mul, dg, dgs, th = nan(M, N), nan(M, N), nan(M, N), nan(M, N, dtype=torch.float32)
    bias_f, rsum = rnd(N, seed=6, scale=0.3), rnd(N, seed=7)
    part = nan(N // 64, M, 2, dtype=torch.float32)
    ops.gemm_nt_mul(a, w, aux, mul)
    ops.gemm_nt(a, w, None, EPI_DGELU, out_t=dg, aux_t=aux)
    ops.gemm_nt_dgelu_stats(a, w, dgs, aux, bias_f, rsum, part)
    ops.gemm_nt(a, w, None, EPI_TANH, out_f=th)

    def ref_mul(r0, r1):      # out = acc * aux: the multiplier is an exact bf16 value, Lipschitz constant |aux|, one fp32 multiply
        x, amp = prod(a, w, None, r0, r1)
        m = aux[r0:r1].double()
        return x * m, LE.elementwise_bound(x * m, amp * m.abs(), K, LE.R_BF16, ops=1)

    def ref_dg(r0, r1):
        # out = acc * gelu'(aux): Lipschitz constant |gelu'(aux)| <= 1.13 in the accumulator; gelu' itself is evaluated in fp32 with the
        # absolute error gelu_grad_eabs, which the accumulator multiplies; one fp32 multiply
        x, amp = prod(a, w, None, r0, r1)
        ud = aux[r0:r1].double()
        g = LE.gelu_grad64(ud)
        return x * g, LE.elementwise_bound(x * g, amp * g.abs(), K, LE.R_BF16, ops=1, eabs=x.abs() * LE.gelu_grad_eabs(ud), mag64=amp * LE.GELU_LIP)

    def ref_tanh(r0, r1):     # tanh: Lipschitz constant 1; tanhf is a 2-ulp function: 2 x 2^-23 of the value; fp32 output
        x, amp = prod(a, w, None, r0, r1)
        t = torch.tanh(x)
        return t, LE.elementwise_bound(t, amp, K, LE.R_F32, ops=0, eabs=2 * 2.0 ** -23 * t.abs())
    gate_once(f'tile256.mul.{tag}', mul, ref_mul, 'pp256')
    gate_once(f'tile256.dgelu.{tag}', dg, ref_dg, 'pp256')
    gate_once(f'tile256.dgelu_stats.du.{tag}', dgs, ref_dg, 'pp256')
    gate_once(f'tile256.tanh.{tag}', th, ref_tanh, 'pp256')
    # part: per row and 64-column block, fp32 dots of the kernel's OWN rounded output with bf16(rsum) and (aux - bf16(bias_f)): 64 products and
    # 64 additions in fp32 (packed-bf16 dots accumulate in fp32), each bounded by the dot's amplitude: |got - dot| <= 2 * 64 * 2^-24 * amplitude
    torch.cuda.synchronize()
    worst = dict(ratio=-1.0)
    for r0, r1 in LE.slabs(M):
        d = dgs[r0:r1].double()
        rb, bb = LE.bf16_round(rsum.double()), LE.bf16_round(bias_f.double())
        y = aux[r0:r1].double() - bb
        f = lambda t: t.reshape(r1 - r0, N // 64, 64).sum(-1)
        own = torch.stack([f(d * rb), f(d * y)], -1)
        amp = torch.stack([f(d.abs() * rb.abs()), f(d.abs() * y.abs())], -1)
        b = LE.row_abs_rel_check(part[:, r0:r1].transpose(0, 1).reshape(r1 - r0, -1), own.reshape(r1 - r0, -1), (2 * 64 * U * amp).reshape(r1 - r0, -1), U)
        if b['ratio'] > worst['ratio']:
            worst = dict(b, row=b['row'] + r0)
    note(f'tile256.dgelu_stats.part.{tag}', 'bound', worst['ratio'], 1.0, worst['row'], worst['col'])
    assert worst['ratio'] <= 1.0, f'tile256.dgelu_stats.part.{tag}: {LE.where(worst, "pp256")}'
    if M == M_STEP and K == 512:
        thrice(f'tile256.dgelu_stats.{tag}', lambda: ops.gemm_nt_dgelu_stats(a, w, dgs, aux, bias_f, rsum, part), [dgs, part])


@pytest.mark.parametrize('M,N,K', [(M_STEP, 1024, 512), (M_STEP, 768, 256)] + [(m, 256, 64) for m in EDGE_M])
def test_tile256_x3(ops, M, N, K):
    """bf16x3 (three bf16 MFMA passes over hi / lo planes, fp32 outputs): every epilogue mbx_gemm_nt_x3 has"""
    a32, w32, bias = rows_scaled(M, K, seed=N), rnd(N, K, seed=N + 1, scale=0.05), rnd(N, seed=N + 2, scale=0.5)
    (ah, al), (wh, wl) = ops.split(a32), ops.split(w32)
    out, g = nan(M, N, dtype=torch.float32), nan(M, N, dtype=torch.float32)
    ops.gemm_nt((ah, al), (wh, wl), bias, EPI_STORE, out_t=out)
    ops.gemm_nt((ah, al), (wh, wl), bias, EPI_GELU, out_t=None, out2_t=g)

    def base(r0, r1):
        # the three products that are taken (hi.hi + hi.lo + lo.hi: 3 K exact bf16 products in fp32) from the operand planes' own bits
        H, L, WH, WL = ah[r0:r1].double(), al[r0:r1].double(), wh.double(), wl.double()
        x = H @ WH.t() + H @ WL.t() + L @ WH.t() + bias.double()
        amp = H.abs() @ WH.abs().t() + H.abs() @ WL.abs().t() + L.abs() @ WH.abs().t()
        return x, amp

    def ref(r0, r1):
        x, amp = base(r0, r1)
        return x, LE.elementwise_bound(x, amp, 3 * K, LE.R_F32, ops=3, mag64=amp + bias.double().abs())

    def ref_g(r0, r1):      # as the bf16 GELU bound, fp32 output
        x, amp = base(r0, r1)
        return LE.gelu64(x), LE.elementwise_bound(LE.gelu64(x), amp, 3 * K, LE.R_F32, lip=LE.GELU_LIP, ops=5, eabs=LE.gelu_eabs(x), mag64=amp + bias.double().abs())
    gate_once(f'tile256.x3.store.{M}x{N}x{K}', out, ref, 'pp256')
    gate_once(f'tile256.x3.gelu.{M}x{N}x{K}', g, ref_g, 'pp256')
    # the other X3 epilogues of mbx_gemm_nt_x3: RESID, TANH, DGELU (fp32 aux).  gemm_nt_gelu_d, gemm_nt_mul and gemm_nt_dgelu_stats have no X3
    # form: they are bf16 entries (hip_ops.can_gelu_d / can_fold require bf16).
    resid, aux = rows_scaled(M, N, seed=9, offset=3.0), rnd(M, N, seed=5, scale=1.5)
    y, th, dg = (nan(M, N, dtype=torch.float32) for _ in range(3))
    ops.gemm_nt((ah, al), (wh, wl), bias, EPI_RESID, out_f=y, resid=resid)
    ops.gemm_nt((ah, al), (wh, wl), None, EPI_TANH, out_f=th)
    ops.gemm_nt((ah, al), (wh, wl), None, EPI_DGELU, out_t=dg, aux_t=aux)

    def ref_y(r0, r1):      # as the bf16 residual epilogue: two fp32 additions after the three passes' accumulation
        x, amp = base(r0, r1)
        rd = resid[r0:r1].double()
        return x + rd, LE.elementwise_bound(x + rd, amp, 3 * K, LE.R_F32, ops=2, mag64=amp + bias.double().abs() + rd.abs())

    def ref_th(r0, r1):     # as the bf16 TANH bound (tanhf: 2 ulp)
        x, amp = base(r0, r1)
        t = torch.tanh(x - bias.double())
        return t, LE.elementwise_bound(t, amp, 3 * K, LE.R_F32, ops=0, eabs=2 * 2.0 ** -23 * t.abs())

    def ref_dg(r0, r1):     # as the bf16 GELU' bound, with the fp32 pre-activation
        x, amp = base(r0, r1)
        x = x - bias.double()
        ud = aux[r0:r1].double()
        gg = LE.gelu_grad64(ud)
        return x * gg, LE.elementwise_bound(x * gg, amp * gg.abs(), 3 * K, LE.R_F32, ops=1, eabs=x.abs() * LE.gelu_grad_eabs(ud), mag64=amp * LE.GELU_LIP)
    gate_once(f'tile256.x3.resid.{M}x{N}x{K}', y, ref_y, 'pp256')
    gate_once(f'tile256.x3.tanh.{M}x{N}x{K}', th, ref_th, 'pp256')
    gate_once(f'tile256.x3.dgelu.{M}x{N}x{K}', dg, ref_dg, 'pp256')
    if M == M_STEP:
        thrice(f'tile256.x3.store.{M}x{N}x{K}', lambda: ops.gemm_nt((ah, al), (wh, wl), bias, EPI_STORE, out_t=out), [out])


# ---------------------------------------------------------------------------------------------- tile GEMM 256 x 128 (gemm_nt_pipe_kernel)
@pytest.mark.parametrize('M,N,K', [(M_STEP, 512, 512), (M_STEP, 512, 1024), (M_STEP, 512, 1536), (M_STEP, 256, 1024)] + [(m, 512, 512) for m in EDGE_M])
def test_tile128_resid_and_lnbwd(ops, M, N, K):
    a, w, bias = gemm_operands(M, N, K, seed=N + K + 3)
    resid = rows_scaled(M, N, seed=9, offset=3.0)
    tag = f'{M}x{N}x{K}'
    y = nan(M, N, dtype=torch.float32)
    ops.gemm_nt(a, w, bias, EPI_RESID, resid=resid, out_f=y)

    def ref_y(r0, r1):      # y = resid + acc + bias: two fp32 additions after the accumulation, fp32 output
        x, amp = prod(a, w, bias, r0, r1)
        rd = resid[r0:r1].double()
        return x + rd, LE.elementwise_bound(x + rd, amp, K, LE.R_F32, ops=2, mag64=amp + bias.double().abs() + rd.abs())
    gate_once(f'tile128.resid.{tag}', y, ref_y, 'pipe')
    xhat, rowc = rnd(M, N, seed=10, dtype=BF), rnd(M, 4, seed=11)
    dres32, dres16 = rows_scaled(M, N, seed=12), rows_scaled(M, N, seed=13).to(BF)
    dx, dx_t, dx2, dx2_t = nan(M, N, dtype=torch.float32), nan(M, N), nan(M, N, dtype=torch.float32), nan(M, N)
    ops.gemm_nt_lnbwd(a, w, xhat, rowc, dres32, None, dx, dx_t)
    ops.gemm_nt_lnbwd(a, w, xhat, rowc, dres16, None, dx2, dx2_t)

    def ref_ln(dres, r):
        def f(r0, r1):
            # dx = dres + rowc.x acc - rowc.y - xhat rowc.z: Lipschitz constant |rowc.x| in the accumulator, five fp32 operations on values
            # bounded by mag = |rowc.x| amp + |rowc.y| + |xhat rowc.z| + |dres|
            x, amp = prod(a, w, None, r0, r1)
            c, xh, dr = rowc[r0:r1].double(), xhat[r0:r1].double(), dres[r0:r1].double()
            v = dr + c[:, 0:1] * x - c[:, 1:2] - xh * c[:, 2:3]
            mag = c[:, 0:1].abs() * amp + c[:, 1:2].abs() + (xh * c[:, 2:3]).abs() + dr.abs()
            return v, r * v.abs() + (1 + r) * (K * U * c[:, 0:1].abs() * amp + 5 * U * mag)
        return f
    gate_once(f'tile128.lnbwd.dx.{tag}', dx, ref_ln(dres32, LE.R_F32), 'pipe')
    gate_once(f'tile128.lnbwd.dx_t.{tag}', dx_t, ref_ln(dres32, LE.R_BF16), 'pipe')
    gate_once(f'tile128.lnbwd_t.dx.{tag}', dx2, ref_ln(dres16, LE.R_F32), 'pipe')
    gate_once(f'tile128.lnbwd_t.dx_t.{tag}', dx2_t, ref_ln(dres16, LE.R_BF16), 'pipe')
    if M == M_STEP and K == 1024 and N == 512:
        thrice(f'tile128.lnbwd_t.{tag}', lambda: ops.gemm_nt_lnbwd(a, w, xhat, rowc, dres16, None, dx2, dx2_t), [dx2, dx2_t])


# ---------------------------------------------------------------------------------------------- weight gradient (gemm_tn_pipe256 / gemm_tn_pipe)
@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('M,N,K', [(M_STEP, 1536, 512), (M_STEP, 512, 1024), (M_STEP, 768, 256), (M_STEP + 37, 512, 512), (4131 + 5, 128, 512),
                                   (4131 + 5, 512, 128), (257, 256, 256),
                                   # branches of the launch plan (TnPlan, csrc/mbx_common.h) that the shapes above do not reach: one chunk and one split
                                   # (bf16: the kernel writes dw and db itself, no column sum); five tiles through the round-6 search; ntk = 8 with
                                   # one bias slot; the small tile with its split count clamped to 1
                                   (17, 256, 256), (4131, 1280, 256), (4131, 512, 2048), (33, 128, 512)])
def test_weight_gradient(ops, M, N, K, x3):
    dy32, a32 = rows_scaled(M, N, seed=N + 4), rows_scaled(M, K, seed=K + 5)
    dw, db = nan(N, K, dtype=torch.float32), nan(N, dtype=torch.float32)
    if x3:
        dyp, ap = ops.split(dy32), ops.split(a32)
        ops.gemm_tn(dyp, ap, dw, db)
        terms = [(dyp[0], ap[0]), (dyp[0], ap[1]), (dyp[1], ap[0])]
        col = [dyp[0], dyp[1]]
    else:
        dy, a = dy32.to(BF), a32.to(BF)
        ops.gemm_tn(dy, a, dw, db)
        terms, col = [(dy, a)], [dy]
    torch.cuda.synchronize()
    x = torch.zeros(N, K, device=DEV, dtype=torch.float64)
    amp = torch.zeros_like(x)
    for r0, r1 in LE.slabs(M):
        for p, q in terms:
            x += p[r0:r1].double().t() @ q[r0:r1].double()
            amp += p[r0:r1].double().abs().t() @ q[r0:r1].double().abs()
    # dW: the contraction runs over the M tokens, divided over `splits` workgroups per output tile whose fp32 partial tiles a column-sum pass
    # adds (tn_finalize): localerr.split_sum_bound.  The split count is localerr.tn_splits (the rule of tnp_splits restated);
    # the library's workspace holds splits x (N K + 4 N) floats + 256 bytes (X3: exactly; bf16: at least -- it is the larger of two kernels')
    splits = LE.tn_splits(M, N, K, x3)
    ws_bytes = int((ops.lib.mbx_gemm_tn_x3_workspace if x3 else ops.lib.mbx_gemm_tn_ws)(M, N, K))
    need = splits * (N * K + 4 * N) * 4 + 256
    assert ws_bytes == need if x3 else ws_bytes >= need, (ws_bytes, need, splits)
    tag = f'{"x3" if x3 else "bf16"}.{M}x{N}x{K}'
    geo = 'tn256' if N >= 256 and K >= 256 else 'tn'
    gate_once(f'gemm_tn.dw.{tag}', dw, lambda r0, r1: (x[r0:r1], LE.split_sum_bound(x[r0:r1], amp[r0:r1], len(terms) * M, splits)), geo)
    REPORT[f'gemm_tn.dw.{tag}.elementwise']['splits'] = splits
    # db: column sums of dy (both planes for X3): the same split structure, up to four partial slots per split (TnPlan::slots)
    s = sum(c.double().sum(0) for c in col)
    sa = sum(c.double().abs().sum(0) for c in col)
    b = LE.row_abs_rel_check(db, s, (-(-len(col) * M // splits) + 64 + 4 * splits) * U * sa, LE.R_F32)
    note(f'gemm_tn.db.{tag}', 'bound', b['ratio'], 1.0, b['row'], 0)
    assert b['ratio'] <= 1.0, f'gemm_tn.db.{tag}: column {b["row"]} at {b["ratio"]:.2f} x its bound'
    # without db the plan is the same and the bias sums are simply not taken: dw must not move by a bit
    dw_nob = nan(N, K, dtype=torch.float32)
    ops.gemm_tn(*((dyp, ap) if x3 else (dy, a)), dw_nob, None)
    torch.cuda.synchronize()
    assert torch.equal(dw_nob.view(torch.int32), dw.view(torch.int32)), f'gemm_tn.dw.{tag}: dw differs between the launches with and without db'
    if M == M_STEP and N == 1536 and not x3:
        thrice(f'gemm_tn.{tag}', lambda: ops.gemm_tn(dy, a, dw, db), [dw, db])


# ---------------------------------------------------------------------------------------------- K-resident row owners (gemm_rows.hip)
@pytest.mark.parametrize('M,N,K', [(M_STEP, 1536, 512), (M_STEP, 768, 256), (127, 1536, 512), (128, 1536, 512), (129, 1536, 512), (129, 768, 256)])
def test_rows_nk(ops, M, N, K):
    a, w, bias = gemm_operands(M, N, K, seed=N + K + 6)
    packed = ops.rows_pack_nk(w)
    rsum = w.float().sum(1)
    mean, rstd = rnd(M, seed=5, scale=0.2), rnd(M, seed=6).abs() + 0.5
    out, out_ln, out_x = nan(M, N), nan(M, N), nan(M, N)
    ops.rows_gemm_nk(a, packed, bias, out)
    ops.rows_gemm_nk(a, packed, bias, out_ln, rsum, mean, rstd)
    eps = 1e-6
    x32 = rows_scaled(M, K, seed=7, offset=0.7)
    ops.rows_gemm_nk_ln(x32, packed, bias, rsum, eps, out_x)
    tag = f'{M}x{N}x{K}'

    def ref(r0, r1):      # as the tile kernel's STORE
        x, amp = prod(a, w, bias, r0, r1)
        return x, LE.elementwise_bound(x, amp, K, LE.R_BF16, ops=1, mag64=amp + bias.double().abs())

    def ref_ln(r0, r1):
        # out = rstd (acc - mean rsum) + bias with fp32 row constants given: Lipschitz constant rstd; four fp32 operations on values bounded by
        # mag = rstd (amp + |mean rsum|) + |bias|
        x, amp = prod(a, w, None, r0, r1)
        mu, rs = mean[r0:r1].double()[:, None], rstd[r0:r1].double()[:, None]
        v = rs * (x - mu * rsum.double()) + bias.double()
        mag = rs * (amp + (mu * rsum.double()).abs()) + bias.double().abs()
        return v, LE.R_BF16 * v.abs() + (1 + LE.R_BF16) * (K * U * rs * amp + 4 * U * mag)

    op = (x32 - x32[:, :1]).to(BF)      # the operand the kernel makes: the fp32 row shifted by its first element, rounded to bf16 (gemm_rows.hip:140)

    def ref_x(r0, r1):
        # the same epilogue with the row constants taken in the kernel from the K fp32 values of the shifted row s = x - x[0]: a K-term fp32 sum
        # for the mean (|d mu| <= (K + 1) 2^-24 mean|s|) and for the variance (relative (2 K + 8) 2^-24, two-pass, plus twice the mean's part
        # |d mu| mean|s - mu| / var), rsqrt to 2 ulp: |d rstd| / rstd <= half of the variance's relative error + 2^-22
        x, amp = prod(op, w, None, r0, r1)
        s = x32[r0:r1].double() - x32[r0:r1, :1].double()
        mu = s.mean(-1, keepdim=True)
        var = ((s - mu) ** 2).mean(-1, keepdim=True)
        rs = torch.rsqrt(var + eps)
        dmu = (K + 1) * U * s.abs().mean(-1, keepdim=True) + U * x32[r0:r1].double().abs().amax(-1, keepdim=True)      # + the shift's own rounding
        drs = rs * (0.5 * ((2 * K + 8) * U + 2 * dmu * (s - mu).abs().mean(-1, keepdim=True) / (var + eps)) + 2.0 ** -22)
        rsd = rsum.double()
        v = rs * (x - mu * rsd) + bias.double()
        mag = rs * (amp + (mu * rsd).abs()) + bias.double().abs()
        return v, LE.R_BF16 * v.abs() + (1 + LE.R_BF16) * (K * U * rs * amp + 4 * U * mag + rs * dmu * rsd.abs() + drs * (x - mu * rsd).abs())
    gate_once(f'rows_nk.store.{tag}', out, ref, 'rows_nk')
    gate_once(f'rows_nk.raw_ln.{tag}', out_ln, ref_ln, 'rows_nk')
    gate_once(f'rows_nk.from_rows.{tag}', out_x, ref_x, 'rows_nk')
    if M == M_STEP and K == 512:
        thrice(f'rows_nk.from_rows.{tag}', lambda: ops.rows_gemm_nk_ln(x32, packed, bias, rsum, eps, out_x), [out_x])


# ---------------------------------------------------------------------------------------------- N-resident row owners (gemm_rows_n.hip)
@pytest.mark.parametrize('M,K,N', [(M_STEP, 1024, 512), (M_STEP, 1024, 256), (129, 1536, 512)])
def test_rows_n(ops, M, K, N):
    """rows_resid_ln (y, mean, rstd, xhat) and rows_lnbwd_t at the shapes tests/test_gpu_rows.py already runs: the elementwise bound and the
    tile unit beside its global and worst-row gates"""
    a, w, bias = gemm_operands(M, N, K, seed=N + K + 8)
    packed = ops.rows_n_pack(w)
    resid = rows_scaled(M, N, seed=4, offset=3.0)
    eps = 1e-6
    y, xh, mean, rstd = nan(M, N, dtype=torch.float32), nan(M, N), nan(M, dtype=torch.float32), nan(M, dtype=torch.float32)
    ops.rows_resid_ln(a, packed, bias, resid, y, xh, mean, rstd, eps)
    tag = f'{M}x{K}x{N}'
    st = {}

    def parts(r0, r1):
        x, amp = prod(a, w, bias, r0, r1)
        rd = resid[r0:r1].double()
        v = x + rd
        mag = amp + bias.double().abs() + rd.abs()
        by = LE.elementwise_bound(v, amp, K, LE.R_F32, ops=2, mag64=mag)      # y as the tile kernel's residual epilogue
        # two-pass statistics of the kernel's fp32 row: mean: the elements' own error + an N-term fp32 sum; variance: 2 |y - mu| (d y + d mu)
        # averaged + (N + 3) 2^-24 relative; rsqrt to 2 ulp
        mu = v.mean(-1, keepdim=True)
        dmu = by.mean(-1, keepdim=True) + (N + 1) * U * v.abs().mean(-1, keepdim=True)
        var = ((v - mu) ** 2).mean(-1, keepdim=True)
        rs = torch.rsqrt(var + eps)
        dvar = 2 * ((v - mu).abs() * (by + dmu)).mean(-1, keepdim=True) + (N + 3) * U * var
        drs = rs * (0.5 * dvar / (var + eps) + 2.0 ** -22)
        return v, by, mu, dmu, rs, drs

    def ref_y(r0, r1):
        v, by = parts(r0, r1)[:2]
        return v, by

    def ref_xhat(r0, r1):
        # xhat = T((y - mean) rstd): the errors of y, mean and rstd above, two fp32 operations, one bf16 rounding
        v, by, mu, dmu, rs, drs = parts(r0, r1)
        st[r0] = (mu, dmu, rs, drs)
        t = (v - mu) * rs
        return t, LE.R_BF16 * t.abs() + (1 + LE.R_BF16) * (rs * (by + dmu) + (v - mu).abs() * drs + 3 * U * t.abs())
    gate_once(f'rows_n.resid_ln.y.{tag}', y, ref_y, 'rows_n')
    gate_once(f'rows_n.resid_ln.xhat.{tag}', xh, ref_xhat, 'rows_n')
    for nm, got, i in (('mean', mean, 0), ('rstd', rstd, 2)):
        worst = dict(ratio=-1.0)
        for r0, r1 in LE.slabs(M):
            b = LE.row_abs_rel_check(got[r0:r1], st[r0][i][:, 0], st[r0][i + 1][:, 0], LE.R_F32)
            if b['ratio'] > worst['ratio']:
                worst = dict(b, row=b['row'] + r0)
        note(f'rows_n.resid_ln.{nm}.{tag}', 'bound', worst['ratio'], 1.0, worst['row'], 0)
        assert worst['ratio'] <= 1.0, f'rows_n.resid_ln.{nm}.{tag}: {LE.where(worst, "rows_n")}'
    # rows_lnbwd_t: dx_t = T(dres + rstd (acc - c1 - xhat c2)), c1 = mean_n(acc), c2 = mean_n(acc xhat) taken in the kernel
    dy, wt, _ = gemm_operands(M, N, K, seed=N + K + 9)
    xhat = rnd(M, N, seed=3, dtype=BF)
    rs_in = rnd(M, seed=5).abs() + 0.5
    dres = rows_scaled(M, N, seed=6).to(BF)
    dxt = nan(M, N)
    pk = ops.rows_n_pack(wt)
    ops.rows_lnbwd_t(dy, pk, xhat, rs_in, dres, dxt)

    def ref_ln(r0, r1):
        # d acc <= K 2^-24 amp per element; c1 and c2 inherit its row mean plus an N-term fp32 sum of |acc| (|acc xhat|); Lipschitz constant
        # rstd; five fp32 operations on values bounded by mag
        x, amp = prod(dy, wt, None, r0, r1)
        h, rs, dr = xhat[r0:r1].double(), rs_in[r0:r1].double()[:, None], dres[r0:r1].double()
        c1, c2 = x.mean(-1, keepdim=True), (x * h).mean(-1, keepdim=True)
        dc1 = (K * U * amp).mean(-1, keepdim=True) + (N + 1) * U * amp.mean(-1, keepdim=True)
        dc2 = (K * U * amp * h.abs()).mean(-1, keepdim=True) + (N + 2) * U * (amp * h.abs()).mean(-1, keepdim=True)
        v = dr + rs * (x - c1 - h * c2)
        mag = dr.abs() + rs * (amp + c1.abs() + (h * c2).abs())
        return v, LE.R_BF16 * v.abs() + (1 + LE.R_BF16) * (rs * (K * U * amp + dc1 + h.abs() * dc2) + 5 * U * mag)
    gate_once(f'rows_n.lnbwd_t.{tag}', dxt, ref_ln, 'rows_n')
    if M == M_STEP and N == 512:
        thrice(f'rows_n.{tag}', lambda: (ops.rows_resid_ln(a, packed, bias, resid, y, xh, mean, rstd, eps), ops.rows_lnbwd_t(dy, pk, xhat, rs_in, dres, dxt)),
               [y, xh, mean, rstd, dxt])


# ---------------------------------------------------------------------------------------------- fused MLP (mlp_fused.hip)
def _mlp64(opnd, stats_of, w1, b1, w2, b2, base, model, r0, r1, eps=1e-6):
    """float64 y for rows r0:r1: opnd the fc1 operand (float64; the model passes it rounded to bf16 where the kernel rounds it), stats_of the
    rows whose LayerNorm statistics normalise it (None: opnd is already normalised); the hidden goes through bf16 once in the model"""
    acc = opnd @ w1.double().t()
    if stats_of is not None:
        mu = stats_of.mean(-1, keepdim=True)
        rs = torch.rsqrt(((stats_of - mu) ** 2).mean(-1, keepdim=True) + eps)
        acc = rs * (acc - mu * w1.double().sum(1))
    g = LE.gelu64(acc + b1.double())
    if model:
        g = LE.bf16_round(g)
    return base + g @ w2.double().t() + b2.double()


@pytest.mark.parametrize('M,C', [(M_STEP, 512), (M_STEP, 256), (127, 512), (129, 512), (129, 256)])
def test_fused_mlp(ops, M, C):
    hidden, eps = 1024, 1e-6
    x = rows_scaled(M, C, seed=C + 1, offset=0.7)
    w1, w2 = rnd(hidden, C, seed=2, dtype=BF, scale=0.06), rnd(C, hidden, seed=3, dtype=BF, scale=0.04)
    b1, b2 = rnd(hidden, seed=4, scale=0.3), rnd(C, seed=5, scale=0.3)
    rsum = w1.float().sum(1)
    packed = ops.mlp_pack_weights(w1, w2)
    a_n = ((x - x.mean(-1, keepdim=True)) * torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + eps)).to(BF)
    a_raw = x.to(BF)
    o, wp, bp = rnd(M, C, seed=9, dtype=BF), rnd(C, C, seed=10, dtype=BF, scale=0.05), rnd(C, seed=11, scale=0.3)
    ppk = ops.proj_mlp_pack_weights(wp, w1, w2)
    ys = {k: nan(M, C, dtype=torch.float32) for k in ('norm', 'raw', 'from_x', 'proj')}
    ops.mlp_fused_fwd(a_n, False, packed, b1, b2, None, x, ys['norm'], None, eps, None, None)
    ops.mlp_fused_fwd(a_raw, True, packed, b1, b2, rsum, x, ys['raw'], None, eps, None, None)
    ops.mlp_fused_fwd(None, True, packed, b1, b2, rsum, x, ys['from_x'], None, eps, None, None)
    ops.proj_mlp_fused_fwd(o, ppk, bp, b1, b2, rsum, x, ys['proj'], eps)
    torch.cuda.synchronize()
    units = {'row': (1, C), 'tile': (32, 32), 'wave_rows': (32, C)}
    for form in ys:
        got, ex, md = [], [], []
        for r0, r1 in LE.slabs(M):
            xd = x[r0:r1].double()
            if form == 'norm':      # operands given in bf16: exact and model differ in the hidden's rounding only (mlp_fused.hip packs gelu(.) to bf16)
                base = xd
                e, m = (_mlp64(a_n[r0:r1].double(), None, w1, b1, w2, b2, xd, md_, r0, r1) for md_ in (False, True))
            elif form == 'raw':     # the statistics are those of the bf16 rows of a
                ad = a_raw[r0:r1].double()
                base = xd
                e, m = (_mlp64(ad, ad, w1, b1, w2, b2, xd, md_, r0, r1) for md_ in (False, True))
            else:                   # the operand is made in the kernel: T(row - row[0]) (mlp_fused.hip:185), statistics of the fp32 rows
                base = xd if form == 'from_x' else xd + o[r0:r1].double() @ wp.double().t() + bp.double()
                s = base - base[:, :1]
                e = _mlp64(s, s, w1, b1, w2, b2, base, False, r0, r1)
                m = _mlp64(LE.bf16_round(s), s, w1, b1, w2, b2, base, True, r0, r1)
            # judged on the branch y - (its fp32 residual): the residual carries no error and would only dilute the units
            got.append(ys[form][r0:r1].double() - base)
            ex.append(e - base)
            md.append(m - base)
        gate_model(f'mlp.{form}.M{M}.C{C}', torch.cat(got), torch.cat(ex), torch.cat(md), 'mlp', units)
    if M == M_STEP and C == 512:
        thrice(f'mlp.proj.M{M}.C{C}', lambda: ops.proj_mlp_fused_fwd(o, ppk, bp, b1, b2, rsum, x, ys['proj'], eps), [ys['proj']])
        thrice(f'mlp.from_x.M{M}.C{C}', lambda: ops.mlp_fused_fwd(None, True, packed, b1, b2, rsum, x, ys['from_x'], None, eps, None, None), [ys['from_x']])


# ---------------------------------------------------------------------------------------------- attention, resident and streamed
J = 17
DROP = (0.1, 0x1234567890ABCDEF)


def wave_lines(t, B, T, H, hd, tm):
    """[M, H hd] tokens -> one line per (problem, 32-row wave block) with one unit of 32 x hd values per head; the ragged last block is
    padded with zeros (mark them with the same function of a tensor of ones)"""
    L = T if tm else J
    nb = -(-L // 32)
    t = t.reshape(B, T, J, -1).permute(0, 2, 1, 3).reshape(B * J, T, -1) if tm else t.reshape(B * T, J, -1)
    return torch.nn.functional.pad(t, (0, 0, 0, nb * 32 - L)).reshape(-1, nb, 32, H, hd).permute(0, 1, 3, 2, 4).reshape(-1, H * 32 * hd)


def _attn_inputs(B, T, H, hd, seed=1, device=DEV):
    C, M = H * hd, B * T * J
    qkv = rnd(M, 3 * C, seed=seed, device=device)
    qkv[:, :C] *= 1.0 + 0.5 * rnd(M, 1, seed=seed + 1, device=device).abs().clamp_max(2.0)      # per-row scale on q in [1, 2]: row maxima, lse and delta differ from row to row,
    # and no softmax saturates (a one-hot row has dS = 0: its dq would sit on the floor of unit_errors; checked in tests/test_localerr.py)
    return qkv.to(BF), rnd(M, C, seed=seed + 2, dtype=BF, device=device), C, M


def _attention_case(ops, mode, B, T, H, hd, drop, stats, identical, seed=1):
    tm = mode == MODE_TEMPORAL
    L = T if tm else J
    geo = 'attn_stream' if L > 256 else 'attn'
    # which backward kernel runs, hence which rounding model (localerr.attn_bwd_ref cites the source lines)
    variant = 'small' if L <= 32 else ('split' if drop or L > 256 else 'fused')
    qkv, do, C, M = _attn_inputs(B, T, H, hd, seed)
    scale = hd ** -0.5
    tag = f'{"tm" if tm else "sp"}.B{B}T{T}H{H}d{hd}{".drop" if drop else ""}'
    seq_row = (lambda r: (r // J) % T) if tm else (lambda r: r % J)
    # float64 references a few clips at a time (the temporal score tensors are [b, J, H, T, T]); with dropout the mask index runs over
    # the whole batch, so those cases are small and taken in one piece
    step = B if drop else max(1, min(B, (1 << 27) // max(1, J * H * L * L) if tm else 16))
    ex_o, md_o, ex_l, ex_d, md_d = [], [], [], [], []
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        sl = slice(b0 * T * J, b1 * T * J)
        e_o, e_l = LE.attn_fwd_ref(qkv[sl], b1 - b0, T, J, H, scale, tm, False, drop)
        m_o, _ = LE.attn_fwd_ref(qkv[sl], b1 - b0, T, J, H, scale, tm, True, drop)
        ex_o.append(e_o), md_o.append(m_o), ex_l.append(e_l)
        o_in = LE.bf16_round(e_o)            # what the backward kernels are handed: the exact forward output, rounded once; lse in fp32
        ex_d.append(LE.attn_bwd_ref(qkv[sl], e_o, do[sl], e_l, b1 - b0, T, J, H, scale, tm, False, drop))
        md_d.append(LE.attn_bwd_ref(qkv[sl], o_in, do[sl], e_l.float(), b1 - b0, T, J, H, scale, tm, True, drop, variant=variant))
    ex_o, md_o, ex_l, ex_d, md_d = (torch.cat(t) for t in (ex_o, md_o, ex_l, ex_d, md_d))
    o, lse = nan(M, C), nan(M, H, dtype=torch.float32)
    ops.attn_fwd(qkv, o, lse, B, T, J, H, scale, mode, drop=drop)
    units = {'row': (1, C), 'row_head': (1, hd)}
    gate_model(f'attn_fwd.o.{tag}', o, ex_o, md_o, geo, units, seq_row)
    # 32-row wave block: 32 consecutive sequence positions of one problem -- regroup the tokens problem-major first
    nb = -(-L // 32)

    def wave_gate(name, got, exact, model):
        g, e, m = (wave_lines(t.double(), B, T, H, hd, tm) for t in (got, exact, model))
        ok = wave_lines(torch.ones_like(exact), B, T, H, hd, tm)
        gu, mu = LE.unit_errors(g, e, 1, 32 * hd, valid=ok, full=True), LE.unit_errors(m, e, 1, 32 * hd, valid=ok, full=True)
        note(name + '.wave_block_head', '2 x model', gu['worst'], mu['worst'], gu['row'], gu['col'], dict(problem=gu['row'] // nb, wave_block=gu['row'] % nb,
                                                                                                          exempt=mu['exempt']))
        assert mu['exempt'] <= LE.MAX_EXEMPT, name
        xs = LE.per_unit_excess(gu, mu, 1, 32 * hd)
        note(name + '.wave_block_head.per_unit', 'per unit', xs['excess'], 1.0, xs['row'], xs['col'], dict(units_over=xs['n_over']))
        assert xs['excess'] <= 1.0, f'{name}: wave block {xs["row"] % nb} of problem {xs["row"] // nb}, head {xs["col"] // (32 * hd)}: {xs["excess"]:.2f} x its own gate'
        assert gu['worst'] <= 2.0 * mu['worst'], (f'{name}: wave block {gu["row"] % nb} of problem {gu["row"] // nb}, head {gu["col"] // (32 * hd)}: kernel '
                                                  f'{gu["worst"]:.3e} > 2 x model {mu["worst"]:.3e}; {LE.locate(32 * (gu["row"] % nb), 0, geo)}')
    wave_gate(f'attn_fwd.o.{tag}', o, ex_o, md_o)
    # lse = m + log(l) in fp32: the scores carry hd exact products in fp32 (hd 2^-24 of their amplitude scale |q| |k|), the sum of L
    # exponentials L 2^-24 relative, exp2 / log at 2 ulp each, the result rounded to fp32
    q5, k5 = qkv[:, :C].double().reshape(M, H, hd), qkv[:, C:2 * C].double().reshape(B, T, J, H, hd)
    kmax = (k5.abs().amax(1, keepdim=True).expand(B, T, J, H, hd) if tm else k5.abs().amax(2, keepdim=True).expand(B, T, J, H, hd)).reshape(M, H, hd)
    lse_abs = (hd + 2) * U * scale * (q5.abs() * kmax).sum(-1) + (L + 8) * U
    b = LE.row_abs_rel_check(lse, ex_l, lse_abs, 2 * U)
    note(f'attn_fwd.lse.{tag}', 'bound', b['ratio'], 1.0, b['row'], b['col'])
    assert b['ratio'] <= 1.0, f'attn_fwd.lse.{tag}: {LE.where(b, geo, seq_row)}'
    o_in, lse_in = LE.bf16_round(ex_o).to(BF), ex_l.float()
    dq = nan(M, 3 * C)
    ops.attn_bwd(qkv, o_in, do, lse_in, dq, B, T, J, H, scale, mode, drop=drop)
    for i, n in enumerate(('dq', 'dk', 'dv')):
        sl = slice(i * C, (i + 1) * C)
        gate_model(f'attn_bwd.{n}.{tag}', dq[:, sl], ex_d[:, sl], md_d[:, sl], geo, units, seq_row)
        wave_gate(f'attn_bwd.{n}.{tag}', dq[:, sl], ex_d[:, sl], md_d[:, sl])
    if stats:
        bias_f, rsum = rnd(3 * C, seed=3, scale=0.3), rnd(3 * C, seed=4)
        d1, part = nan(M, 3 * C), nan(2 * H, M, 2, dtype=torch.float32)
        ops.attn_bwd_stats(qkv, o_in, do, lse_in, d1, bias_f, rsum, part, B, T, J, H, scale, mode)
        torch.cuda.synchronize()
        assert torch.equal(d1.view(torch.int16), dq.view(torch.int16)), f'attn_bwd_stats.{tag}: dqkv differs from mbx_attn_bwd'
        # the dots of the kernel's own rounded gradient (attention_common.h store_rowfrag_dot): 2 hd products and additions per dot in fp32
        own, amp = LE.attn_stats_ref(d1, qkv, bias_f, rsum, H)
        b = LE.row_abs_rel_check(part.reshape(2 * H * M, 2), own.reshape(2 * H * M, 2), 2 * (2 * hd) * U * amp.reshape(2 * H * M, 2), U)
        note(f'attn_bwd_stats.part.{tag}', 'bound', b['ratio'], 1.0, b['row'] % M, b['row'] // M)
        assert b['ratio'] <= 1.0, f'attn_bwd_stats.part.{tag}: token row {b["row"] % M}, block {b["row"] // M}: {b["ratio"]:.2f} x its bound'
    if identical:
        thrice(f'attn_fwd.{tag}', lambda: ops.attn_fwd(qkv, o, lse, B, T, J, H, scale, mode), [o, lse])
        thrice(f'attn_bwd.{tag}', lambda: ops.attn_bwd(qkv, o_in, do, lse_in, dq, B, T, J, H, scale, mode), [dq])


@pytest.mark.parametrize('hd', [64, 32])
@pytest.mark.parametrize('mode', [MODE_SPATIAL, MODE_TEMPORAL])
def test_attention_training_step(ops, mode, hd):
    """B = 64, T = 243: the step's 1,088 x H temporal and 15,552 x H spatial problems (C = 512 / 256)"""
    _attention_case(ops, mode, 64, 243, 8, hd, None, stats=True, identical=hd == 64)


@pytest.mark.parametrize('hd', [64, 32])
@pytest.mark.parametrize('T', [31, 32, 33, 255, 256])
def test_attention_resident_edges(ops, T, hd):
    # seeded by T; tests/test_localerr.py checks that no unit of these references sits on the floor (with 272 wave-block units a single
    # one-row tail block with a near-zero gradient row would already be 0.4 % of them)
    _attention_case(ops, MODE_TEMPORAL, 2, T, 4, hd, None, stats=True, identical=False, seed=T)


@pytest.mark.parametrize('mode,B,T,hd', [(MODE_SPATIAL, 3, 9, 64), (MODE_TEMPORAL, 1, 33, 32), (MODE_TEMPORAL, 1, 243, 64), (MODE_TEMPORAL, 1, 321, 64)])
def test_attention_probability_dropout(ops, mode, B, T, hd):
    _attention_case(ops, mode, B, T, 4, hd, DROP, stats=False, identical=False)


@pytest.mark.parametrize('hd', [64, 32])
@pytest.mark.parametrize('T,H', [(257, 4), (319, 4), (320, 4), (321, 4), (511, 2), (512, 2), (513, 2), (2048, 1)])
def test_attention_streamed(ops, T, H, hd):
    """block (256), wave-block (32) and stream-tile (64) edges +- 1, and one long sequence"""
    _attention_case(ops, MODE_TEMPORAL, 1, T, H, hd, None, stats=True, identical=T == 513 and hd == 64)
