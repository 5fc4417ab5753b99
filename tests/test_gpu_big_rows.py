"""Parity at the row count of the benchmark's 256-clip configurations, M = 256 x 243 x 17 = 1,057,536, where byte offsets pass 2^31 (every
activation) and 2^32 (the fp32 tensors of 1024 and 1536 columns), on a real MI355X.  The checks and their own tests: tests/bigerr.py,
tests/test_bigerr.py.

Every case
  * draws its operands on the device (seeded), rows with a scale and an offset of their own;
  * asserts the entry's own size checks before it launches anything at this size;
  * runs bigerr.quarters_equal: the launch on all rows against one launch per 64 clips on row slices of the same operands, outputs
    pre-filled with NaN, bit-identical over the whole tensor (a sub-launch has the same row arithmetic with small offsets);
  * gates the rows of bigerr.slabs_of_interest -- first, last, 512 either side of every crossing of every tensor the kernel addresses,
    ragged last tiles, 4,096 sampled -- against a float64 reference with the bound the family already has in tests/test_gpu_local_parity.py
    (localerr.elementwise_bound, the 2 x rounding-model gate, split_sum_bound), unchanged;
  * frees its tensors.
Where bit-equality across launch sizes is not a property of a kernel, the case says so and is judged otherwise:
  * weight gradients (and every other reduction over M: dgamma / dbeta, the fusion and head parameter gradients) contract over M and
    their split count or launch geometry follows M (TnPlan; the grid caps of the row kernels): gated against float64 over ALL rows
    with the family's bound for that structure, launched three times; the weight gradients once more on integer operands, where fp32 is
    exact in any order and every bit is decided (_integer_weight_gradient);
  * the dropout masks are a hash of the element's index in the whole tensor and the entries take no index offset: every keep decision
    and every value of the element-wise kernels is checked, slab by slab; the attention-probability dropout on the clips of interest,
    with the mask of their own indices in the full batch.

Everything measured, with the side of each crossing the worst row lies on and the test's peak device memory, goes to big_rows.json /
big_rows.txt in the directory MBX_REPORT_DIR names (default: reports/ in the repository root, git-ignored)."""
import json
import os
import time

import pytest
import torch

from motionbert_amd import engine
from motionbert_amd.engine import EPI_DGELU, EPI_GELU, EPI_RESID, EPI_STORE, EPI_TANH, MODE_SPATIAL, MODE_TEMPORAL
from tests import bigerr as BE
from tests import localerr as LE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
U = LE.U32
M256, CLIP, M_STEP = BE.M256, BE.CLIP, BE.M_STEP
J, T_FRAMES = 17, 243
REPORT = {}


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')
    os.makedirs(out, exist_ok=True)
    REPORT['_wall_seconds'] = time.time() - t0
    with open(os.path.join(out, 'big_rows.json'), 'w') as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'big_rows.txt'), 'w') as f:
        f.write(f'{"output":76s} {"gate":>10s} {"value":>10s} {"against":>10s} {"ratio":>7s}  worst unit (row, col), side of the crossings\n')
        for k in sorted(REPORT):
            v = REPORT[k]
            if isinstance(v, dict) and 'ratio' in v:
                f.write(f'{k:76s} {v["gate"]:>10s} {v["value"]:10.3e} {v["against"]:10.3e} {v["ratio"]:7.3f}  ({v["row"]}, {v["col"]}) {v.get("side", "")}\n')
        for k in sorted(REPORT):
            if k.endswith('.quarters_equal') or k.endswith('.three_launches_identical'):
                f.write(f'{k:76s} {REPORT[k]}\n')
        for k in sorted(REPORT):
            if k.endswith('.peak_gib'):
                f.write(f'{k:76s} {REPORT[k]:.1f} GiB, {REPORT[k[:-9] + ".seconds"]:.1f} s\n')
        f.write(f'wall time of the module: {REPORT["_wall_seconds"]:.1f} s\n')


@pytest.fixture(autouse=True)
def _memory(request):
    """peak device memory and wall time of every test into the report; nothing of a test outlives it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    REPORT[request.node.name + '.peak_gib'] = torch.cuda.max_memory_allocated() / 2 ** 30
    REPORT[request.node.name + '.seconds'] = time.time() - t0
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- operands and reporting
def rnd(*shape, seed=0, dtype=F32, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randn(*shape, device=DEV, generator=g)
    if scale != 1.0:
        t.mul_(scale)
    return t if dtype == F32 else t.to(dtype)


def rows_scaled(M, K, seed, offset=0.3, dtype=F32):
    """fp32 rows with a scale and an offset of their own (as tests/test_gpu_local_parity.py builds them), drawn on the device"""
    t = rnd(M, K, seed=seed)
    t.mul_(0.5 + rnd(M, 1, seed=seed + 101).abs_()).add_(rnd(M, 1, seed=seed + 102), alpha=offset)
    return t if dtype == F32 else t.to(dtype)


def gemm_operands(M, N, K, seed):
    return rows_scaled(M, K, seed, dtype=BF), rnd(N, K, seed=seed + 1, dtype=BF, scale=0.05), rnd(N, seed=seed + 2, scale=0.5)


def nan(*shape, dtype=BF):
    return torch.full(shape, float('nan'), device=DEV, dtype=dtype)


def note(name, gate, value, against, row, col, side='', extra=None):
    REPORT[name] = dict(gate=gate, value=value, against=against, ratio=value / max(against, 1e-300), row=row, col=col, side=side, **(extra or {}))


def prod(a_rows, w, bias):
    """float64 product of the given operand rows from their bf16 / fp32 bits, and its amplitude |a| . |w|^T"""
    ad, wd = a_rows.double(), w.double()
    x = ad @ wd.t()
    if bias is not None:
        x = x + bias.double()
    return x, ad.abs() @ wd.abs().t()


def rows_case(name, M, launch, outs, operand_row_bytes, refs, bitwise=True):
    """quarters_equal over all of `outs`, then the elementwise bound on slabs_of_interest: refs(idx) -> {output: (x64, bound64)} for the
    rows idx (a device index tensor).  The slabs follow the crossings of every output and of every operand (operand_row_bytes)."""
    if bitwise:
        widths = BE.quarters_equal(launch, M, outs, name=name + '.')
        REPORT[name + '.quarters_equal'] = 'identical: ' + ', '.join(f'{k} ({rb} B rows)' for k, rb in widths.items())
    else:
        for o in outs.values():
            o.fill_(float('nan'))
        launch(0, M)
        torch.cuda.synchronize()
        widths = {k: o[0].numel() * o.element_size() for k, o in outs.items()}
    sl = BE.slabs_of_interest(M, sorted(set(widths.values()) | set(operand_row_bytes)))
    rows = sl.rows()
    idx = torch.from_numpy(rows).to(DEV)
    bad = []
    for k, (x, bound) in refs(idx).items():
        got = outs[k][idx]
        res = BE.slab_gate(f'{name}.{k}', got.reshape(len(rows), -1), rows, x.reshape(len(rows), -1), bound.reshape(len(rows), -1), widths[k], check=False)
        note(f'{name}.{k}', 'bound', res['ratio'], 1.0, res['row'], res['col'], res['side'], dict(violations=res['violations'], rows_judged=res['rows_judged']))
        if res['violations']:
            bad.append(f'{k}: {res["violations"]} elements outside the elementwise bound, the worst at {res["ratio"]:.3g} x in row {res["row"]}, col {res["col"]} '
                       f'(byte offset {res["row"] * widths[k]:,}: {res["side"]})')
    assert not bad, f'{name}: ' + '; '.join(bad)
    return idx


def thrice(name, launch, outs):
    res = []
    for _ in range(3):
        for o in outs:
            o.fill_(float('nan'))
        launch()
        torch.cuda.synchronize()
        res.append([o.clone() for o in outs])
    same = all(BE.first_difference(a, b) is None for r in res[1:] for a, b in zip(res[0], r))
    REPORT[name + '.three_launches_identical'] = 'identical' if same else 'DIFFER'
    assert same, f'{name}: three launches differ'


def gemm_nt_fits(M, N, K):
    """mbx_gemm_nt's own size check (gemm.hip: M max(N, K) < 2^40 elements)"""
    return M * max(N, K) < 1 << 40


# ------------------------------------------------------------------------------------------------------------- 1. tile GEMMs, bf16
STEP_NK = [(1536, 512), (1024, 512), (768, 256), (1024, 256)]      # qkv, fc1 / fc2-dX at dim_feat 512 and 256 (tests/test_gpu_local_parity.py)
BIG_M = [(M256, n, k) for n, k in STEP_NK] + [(m, 1536, 512) for m in BE.M_RAGGED]


@pytest.mark.parametrize('M,N,K', BIG_M)
def test_tile256_forward_epilogues(ops, M, N, K):
    """gemm_nt STORE and GELU (both outputs), gemm_nt_gelu_d: gemm_nt_pp256_kernel"""
    assert gemm_nt_fits(M, N, K)
    a, w, bias = gemm_operands(M, N, K, seed=N + K)
    outs = dict(store=nan(M, N), gelu_u=nan(M, N), gelu_g=nan(M, N), gelu_d_d=nan(M, N), gelu_d_g=nan(M, N))

    def launch(r0, r1):
        ops.gemm_nt(a[r0:r1], w, bias, EPI_STORE, out_t=outs['store'][r0:r1])
        ops.gemm_nt(a[r0:r1], w, bias, EPI_GELU, out_t=outs['gelu_u'][r0:r1], out2_t=outs['gelu_g'][r0:r1])
        ops.gemm_nt_gelu_d(a[r0:r1], w, bias, outs['gelu_d_d'][r0:r1], outs['gelu_d_g'][r0:r1])

    def refs(idx):      # the bounds of test_tile256_store / test_tile256_gelu_forms
        x, amp = prod(a[idx], w, bias)
        mag = amp + bias.double().abs()
        st = (x, LE.elementwise_bound(x, amp, K, LE.R_BF16, lip=1.0, ops=1, mag64=mag))
        g = (LE.gelu64(x), LE.elementwise_bound(LE.gelu64(x), amp, K, LE.R_BF16, lip=LE.GELU_LIP, ops=3, eabs=LE.gelu_eabs(x), mag64=mag))
        d = (LE.gelu_grad64(x), LE.elementwise_bound(LE.gelu_grad64(x), amp, K, LE.R_BF16, lip=1.0, ops=1, eabs=LE.gelu_grad_eabs(x), mag64=mag))
        return dict(store=st, gelu_u=st, gelu_g=g, gelu_d_g=g, gelu_d_d=d)
    rows_case(f'tile256.fwd.{M}x{N}x{K}', M, launch, outs, [K * 2], refs)


@pytest.mark.parametrize('M,N,K', [(M256, 1024, 512), (M256, 1024, 256), (BE.M_RAGGED[1], 1024, 512)])
def test_tile256_backward_epilogues(ops, M, N, K):
    """fc2's dX with the GELU' epilogues: gemm_nt_mul, EPI_DGELU, gemm_nt_dgelu_stats (du and its row dots), and TANH (fp32 output)"""
    assert gemm_nt_fits(M, N, K)
    a, w, _ = gemm_operands(M, N, K, seed=N + K + 2)
    aux = rnd(M, N, seed=5, dtype=BF, scale=1.5)
    bias_f, rsum = rnd(N, seed=6, scale=0.3), rnd(N, seed=7)
    nb = N // 64
    # part is [N / 64, M, 2] in the kernel's layout (block-major): kept here row-major so that the quarters line up
    outs = dict(mul=nan(M, N), dgelu=nan(M, N), stats_du=nan(M, N), tanh=nan(M, N, dtype=F32), part=nan(M, nb, 2, dtype=F32))

    def launch(r0, r1):
        ops.gemm_nt_mul(a[r0:r1], w, aux[r0:r1], outs['mul'][r0:r1])
        ops.gemm_nt(a[r0:r1], w, None, EPI_DGELU, out_t=outs['dgelu'][r0:r1], aux_t=aux[r0:r1])
        part = nan(nb, r1 - r0, 2, dtype=F32)
        ops.gemm_nt_dgelu_stats(a[r0:r1], w, outs['stats_du'][r0:r1], aux[r0:r1], bias_f, rsum, part)
        outs['part'][r0:r1] = part.transpose(0, 1)
        ops.gemm_nt(a[r0:r1], w, None, EPI_TANH, out_f=outs['tanh'][r0:r1])

    def refs(idx):      # the bounds of test_tile256_backward_epilogues (tests/test_gpu_local_parity.py)
        x, amp = prod(a[idx], w, None)
        m = aux[idx].double()
        g = LE.gelu_grad64(m)
        dg = (x * g, LE.elementwise_bound(x * g, amp * g.abs(), K, LE.R_BF16, ops=1, eabs=x.abs() * LE.gelu_grad_eabs(m), mag64=amp * LE.GELU_LIP))
        t = torch.tanh(x)
        # part: fp32 dots of the kernel's OWN rounded output with bf16(rsum) and (aux - bf16(bias_f)) per 64-column block
        d = outs['stats_du'][idx].double()
        rb, bb = LE.bf16_round(rsum.double()), LE.bf16_round(bias_f.double())
        y = m - bb
        f = lambda v: v.reshape(len(idx), nb, 64).sum(-1)
        own = torch.stack([f(d * rb), f(d * y)], -1)
        pamp = torch.stack([f(d.abs() * rb.abs()), f(d.abs() * y.abs())], -1)
        return dict(mul=(x * m, LE.elementwise_bound(x * m, amp * m.abs(), K, LE.R_BF16, ops=1)), dgelu=dg, stats_du=dg,
                    tanh=(t, LE.elementwise_bound(t, amp, K, LE.R_F32, ops=0, eabs=2 * 2.0 ** -23 * t.abs())),
                    part=(own, 2 * 64 * U * pamp + U * own.abs()))
    rows_case(f'tile256.bwd.{M}x{N}x{K}', M, launch, outs, [K * 2, N * 2], refs)


@pytest.mark.parametrize('M,N,K', [(M256, 512, 512), (M256, 512, 1024), (M256, 512, 1536), (M256, 256, 1024), (BE.M_RAGGED[0], 512, 1024), (BE.M_RAGGED[1], 512, 1536)])
def test_tile128_resid_and_lnbwd(ops, M, N, K):
    """gemm_nt_pipe_kernel: the residual epilogue, gemm_nt_lnbwd (fp32 dres) and gemm_nt_lnbwd_t (bf16 dres), each with dx and dx_t"""
    assert gemm_nt_fits(M, N, K)
    a, w, bias = gemm_operands(M, N, K, seed=N + K + 3)
    resid = rows_scaled(M, N, seed=9, offset=3.0)
    xhat, rowc = rnd(M, N, seed=10, dtype=BF), rnd(M, 4, seed=11)
    dres32 = rows_scaled(M, N, seed=12)
    dres16 = rows_scaled(M, N, seed=13, dtype=BF)
    outs = dict(y=nan(M, N, dtype=F32), dx=nan(M, N, dtype=F32), dx_t=nan(M, N), t_dx=nan(M, N, dtype=F32), t_dx_t=nan(M, N))

    def launch(r0, r1):
        s = slice(r0, r1)
        ops.gemm_nt(a[s], w, bias, EPI_RESID, resid=resid[s], out_f=outs['y'][s])
        ops.gemm_nt_lnbwd(a[s], w, xhat[s], rowc[s], dres32[s], None, outs['dx'][s], outs['dx_t'][s])
        ops.gemm_nt_lnbwd(a[s], w, xhat[s], rowc[s], dres16[s], None, outs['t_dx'][s], outs['t_dx_t'][s])

    def refs(idx):      # the bounds of test_tile128_resid_and_lnbwd (tests/test_gpu_local_parity.py)
        x, amp = prod(a[idx], w, None)
        rd, bd = resid[idx].double(), bias.double()
        y = x + bd + rd
        c, xh = rowc[idx].double(), xhat[idx].double()

        def ln(dres, r):
            dr = dres[idx].double()
            v = dr + c[:, 0:1] * x - c[:, 1:2] - xh * c[:, 2:3]
            mag = c[:, 0:1].abs() * amp + c[:, 1:2].abs() + (xh * c[:, 2:3]).abs() + dr.abs()
            return v, r * v.abs() + (1 + r) * (K * U * c[:, 0:1].abs() * amp + 5 * U * mag)
        return dict(y=(y, LE.elementwise_bound(y, amp, K, LE.R_F32, ops=2, mag64=amp + bd.abs() + rd.abs())),
                    dx=ln(dres32, LE.R_F32), dx_t=ln(dres32, LE.R_BF16), t_dx=ln(dres16, LE.R_F32), t_dx_t=ln(dres16, LE.R_BF16))
    rows_case(f'tile128.{M}x{N}x{K}', M, launch, outs, [K * 2, N * 2, 16], refs)


# ------------------------------------------------------------------------------------------------------------- 2. row owners, bf16
@pytest.mark.parametrize('M,N,K', [(M256, 1536, 512), (M256, 768, 256), (BE.M_RAGGED[0], 1536, 512), (BE.M_RAGGED[1], 1536, 512)])
def test_rows_nk(ops, M, N, K):
    """gemm_rows.hip: rows_gemm_nk (plain and with given row constants) and rows_gemm_nk_ln (operand and statistics from the fp32 rows)"""
    a, w, bias = gemm_operands(M, N, K, seed=N + K + 6)
    packed = ops.rows_pack_nk(w)
    rsum = w.float().sum(1)
    mean, rstd = rnd(M, seed=5, scale=0.2), rnd(M, seed=6).abs() + 0.5
    eps = 1e-6
    x32 = rows_scaled(M, K, seed=7, offset=0.7)
    outs = dict(store=nan(M, N), raw_ln=nan(M, N), from_rows=nan(M, N))

    def launch(r0, r1):
        s = slice(r0, r1)
        ops.rows_gemm_nk(a[s], packed, bias, outs['store'][s])
        ops.rows_gemm_nk(a[s], packed, bias, outs['raw_ln'][s], rsum, mean[s], rstd[s])
        ops.rows_gemm_nk_ln(x32[s], packed, bias, rsum, eps, outs['from_rows'][s])

    def refs(idx):      # the bounds of test_rows_nk (tests/test_gpu_local_parity.py), derived there
        bd, rsd = bias.double(), rsum.double()
        x, amp = prod(a[idx], w, None)
        st = (x + bd, LE.elementwise_bound(x + bd, amp, K, LE.R_BF16, ops=1, mag64=amp + bd.abs()))
        mu, rs = mean[idx].double()[:, None], rstd[idx].double()[:, None]
        v = rs * (x - mu * rsd) + bd
        mag = rs * (amp + (mu * rsd).abs()) + bd.abs()
        ln = (v, LE.R_BF16 * v.abs() + (1 + LE.R_BF16) * (K * U * rs * amp + 4 * U * mag))
        xr = x32[idx]
        op = (xr - xr[:, :1]).to(BF)
        x, amp = prod(op, w, None)
        s = xr.double() - xr[:, :1].double()
        mu = s.mean(-1, keepdim=True)
        var = ((s - mu) ** 2).mean(-1, keepdim=True)
        rs = torch.rsqrt(var + eps)
        dmu = (K + 1) * U * s.abs().mean(-1, keepdim=True) + U * xr.double().abs().amax(-1, keepdim=True)
        drs = rs * (0.5 * ((2 * K + 8) * U + 2 * dmu * (s - mu).abs().mean(-1, keepdim=True) / (var + eps)) + 2.0 ** -22)
        v = rs * (x - mu * rsd) + bd
        mag = rs * (amp + (mu * rsd).abs()) + bd.abs()
        fx = (v, LE.R_BF16 * v.abs() + (1 + LE.R_BF16) * (K * U * rs * amp + 4 * U * mag + rs * dmu * rsd.abs() + drs * (x - mu * rsd).abs()))
        return dict(store=st, raw_ln=ln, from_rows=fx)
    rows_case(f'rows_nk.{M}x{N}x{K}', M, launch, outs, [K * 2, K * 4, 4], refs)


def _rows_n_case(ops, M, K, N, what):
    """rows_resid_ln (y, xhat, mean, rstd) and / or rows_lnbwd_t, with the bounds of test_rows_n (tests/test_gpu_local_parity.py)"""
    eps = 1e-6
    tag = f'{M}x{K}x{N}'
    if 'resid' in what:
        assert engine.rows_resid_ln_fits(M, N, K)
        a, w, bias = gemm_operands(M, N, K, seed=N + K + 8)
        packed = ops.rows_n_pack(w)
        resid = rows_scaled(M, N, seed=4, offset=3.0)
        outs = dict(y=nan(M, N, dtype=F32), xhat=nan(M, N), mean=nan(M, dtype=F32), rstd=nan(M, dtype=F32))

        def launch(r0, r1):
            s = slice(r0, r1)
            ops.rows_resid_ln(a[s], packed, bias, resid[s], outs['y'][s], outs['xhat'][s], outs['mean'][s], outs['rstd'][s], eps)

        def refs(idx):
            x, amp = prod(a[idx], w, bias)
            rd = resid[idx].double()
            v = x + rd
            mag = amp + bias.double().abs() + rd.abs()
            by = LE.elementwise_bound(v, amp, K, LE.R_F32, ops=2, mag64=mag)
            mu = v.mean(-1, keepdim=True)
            dmu = by.mean(-1, keepdim=True) + (N + 1) * U * v.abs().mean(-1, keepdim=True)
            var = ((v - mu) ** 2).mean(-1, keepdim=True)
            rs = torch.rsqrt(var + eps)
            dvar = 2 * ((v - mu).abs() * (by + dmu)).mean(-1, keepdim=True) + (N + 3) * U * var
            drs = rs * (0.5 * dvar / (var + eps) + 2.0 ** -22)
            t = (v - mu) * rs
            bt = LE.R_BF16 * t.abs() + (1 + LE.R_BF16) * (rs * (by + dmu) + (v - mu).abs() * drs + 3 * U * t.abs())
            # mean and rstd: test_rows_n gates them with row_abs_rel_check(abs, R_F32): the same bound, written elementwise
            return dict(y=(v, by), xhat=(t, bt), mean=(mu[:, 0], dmu[:, 0] + LE.R_F32 * mu[:, 0].abs()), rstd=(rs[:, 0], drs[:, 0] + LE.R_F32 * rs[:, 0].abs()))
        rows_case(f'rows_n.resid_ln.{tag}', M, launch, outs, [K * 2], refs)
        del a, w, bias, packed, resid, outs
    if 'lnbwd' in what:
        assert engine.rows_lnbwd_fits(M, N, K)
        dy, wt, _ = gemm_operands(M, N, K, seed=N + K + 9)
        xhat = rnd(M, N, seed=3, dtype=BF)
        rs_in = rnd(M, seed=5).abs_() + 0.5
        dres = rows_scaled(M, N, seed=6, dtype=BF)
        pk = ops.rows_n_pack(wt)
        outs = dict(dx_t=nan(M, N))

        def launch(r0, r1):
            s = slice(r0, r1)
            ops.rows_lnbwd_t(dy[s], pk, xhat[s], rs_in[s], dres[s], outs['dx_t'][s])

        def refs(idx):
            x, amp = prod(dy[idx], wt, None)
            h, rs, dr = xhat[idx].double(), rs_in[idx].double()[:, None], dres[idx].double()
            c1, c2 = x.mean(-1, keepdim=True), (x * h).mean(-1, keepdim=True)
            dc1 = (K * U * amp).mean(-1, keepdim=True) + (N + 1) * U * amp.mean(-1, keepdim=True)
            dc2 = (K * U * amp * h.abs()).mean(-1, keepdim=True) + (N + 2) * U * (amp * h.abs()).mean(-1, keepdim=True)
            v = dr + rs * (x - c1 - h * c2)
            mag = dr.abs() + rs * (amp + c1.abs() + (h * c2).abs())
            return dict(dx_t=(v, LE.R_BF16 * v.abs() + (1 + LE.R_BF16) * (rs * (K * U * amp + dc1 + h.abs() * dc2) + 5 * U * mag)))
        rows_case(f'rows_n.lnbwd_t.{tag}', M, launch, outs, [K * 2, 4], refs)


@pytest.mark.parametrize('M,K,N', [(M256, 1024, 512), (M256, 1536, 512), (M256, 512, 512), (M256, 1024, 256), (BE.M_RAGGED[0], 1536, 512), (BE.M_RAGGED[1], 1024, 512)])
def test_rows_n(ops, M, K, N):
    """gemm_rows_n.hip at the 256-clip row count: the bf16 [M, 1536] operand of qkv's dX lies between 2^31 and 2^32 bytes there, where the
    kernel's unsigned 32-bit lane offsets are all that addresses it"""
    _rows_n_case(ops, M, K, N, ('resid', 'lnbwd'))


LAST_LNBWD = (engine.ROW_OFFSET_LIMIT - 1) // (1536 * 2)      # 1,398,101 rows of bf16 [., 1536]
LAST_RESID = (engine.ROW_OFFSET_LIMIT - 1) // (512 * 4)       # 2,097,151 rows of fp32 [., 512] (and of bf16 [., 1024])


def test_rows_lnbwd_t_at_its_limit(ops):
    """the largest row count mbx_rows_lnbwd_t takes at K = 1536 -- the last rows sit just below 2^32 bytes -- and its refusal one row on"""
    assert LAST_LNBWD == 1398101
    _rows_n_case(ops, LAST_LNBWD, 1536, 512, ('lnbwd',))
    M = LAST_LNBWD + 1
    assert not engine.rows_lnbwd_fits(M, 512, 1536)
    dy, xhat, dres, dx = (torch.empty(M, n, device=DEV, dtype=BF) for n in (1536, 512, 512, 512))
    pk = ops.rows_n_pack(rnd(512, 1536, seed=1, dtype=BF))
    with pytest.raises(RuntimeError, match=f'rows_lnbwd_t: dy of M={M} x K=1536 exceeds the 32-bit lane offsets'):      # (checked before any launch)
        ops.rows_lnbwd_t(dy, pk, xhat, torch.empty(M, device=DEV), dres, dx)


def test_rows_resid_ln_at_its_limit(ops):
    assert LAST_RESID == 2 ** 21 - 1
    _rows_n_case(ops, LAST_RESID, 1024, 512, ('resid',))
    M = LAST_RESID + 1
    assert not engine.rows_resid_ln_fits(M, 512, 1024)
    a, xh = torch.empty(M, 1024, device=DEV, dtype=BF), torch.empty(M, 512, device=DEV, dtype=BF)
    resid, y = torch.empty(M, 512, device=DEV), torch.empty(M, 512, device=DEV)
    pk = ops.rows_n_pack(rnd(512, 1024, seed=1, dtype=BF))
    with pytest.raises(RuntimeError, match=f'rows_resid_ln: M={M} rows of 2048 bytes exceed the 32-bit row offsets'):
        ops.rows_resid_ln(a, pk, torch.empty(512, device=DEV), resid, y, xh, torch.empty(M, device=DEV), torch.empty(M, device=DEV), 1e-6)


def _mlp64(opnd, stats_of, w1, b1, w2, b2, base, model, eps=1e-6):
    """float64 y (tests/test_gpu_local_parity.py, _mlp64): the hidden goes through bf16 once in the model"""
    acc = opnd @ w1.double().t()
    if stats_of is not None:
        mu = stats_of.mean(-1, keepdim=True)
        rs = torch.rsqrt(((stats_of - mu) ** 2).mean(-1, keepdim=True) + eps)
        acc = rs * (acc - mu * w1.double().sum(1))
    g = LE.gelu64(acc + b1.double())
    if model:
        g = LE.bf16_round(g)
    return base + g @ w2.double().t() + b2.double()


@pytest.mark.parametrize('M,C', [(M256, 512), (M256, 256), (BE.M_RAGGED[0], 512), (BE.M_RAGGED[1], 512)])
def test_fused_mlp(ops, M, C):
    """mlp_fused_fwd in its three operand forms and proj_mlp_fused_fwd: quarters_equal, then the 2 x rounding-model gate of
    test_fused_mlp (tests/test_gpu_local_parity.py) on the slabs"""
    from tests.test_gpu_local_parity import REPORT as LP_REPORT, gate_model
    hidden, eps = 1024, 1e-6
    x = rows_scaled(M, C, seed=C + 1, offset=0.7)
    w1, w2 = rnd(hidden, C, seed=2, dtype=BF, scale=0.06), rnd(C, hidden, seed=3, dtype=BF, scale=0.04)
    b1, b2 = rnd(hidden, seed=4, scale=0.3), rnd(C, seed=5, scale=0.3)
    rsum = w1.float().sum(1)
    packed = ops.mlp_pack_weights(w1, w2)
    a_n = torch.empty(M, C, device=DEV, dtype=BF)
    for r0, r1 in BE.quarters(M):      # (a quarter at a time: the fp32 intermediates of torch stay small)
        xq = x[r0:r1]
        a_n[r0:r1] = ((xq - xq.mean(-1, keepdim=True)) * torch.rsqrt(xq.var(-1, unbiased=False, keepdim=True) + eps)).to(BF)
    a_raw = x.to(BF)
    o, wp, bp = rnd(M, C, seed=9, dtype=BF), rnd(C, C, seed=10, dtype=BF, scale=0.05), rnd(C, seed=11, scale=0.3)
    ppk = ops.proj_mlp_pack_weights(wp, w1, w2)
    ys = {k: nan(M, C, dtype=F32) for k in ('norm', 'raw', 'from_x', 'proj')}

    def launch(r0, r1):
        s = slice(r0, r1)
        ops.mlp_fused_fwd(a_n[s], False, packed, b1, b2, None, x[s], ys['norm'][s], None, eps, None, None)
        ops.mlp_fused_fwd(a_raw[s], True, packed, b1, b2, rsum, x[s], ys['raw'][s], None, eps, None, None)
        ops.mlp_fused_fwd(None, True, packed, b1, b2, rsum, x[s], ys['from_x'][s], None, eps, None, None)
        ops.proj_mlp_fused_fwd(o[s], ppk, bp, b1, b2, rsum, x[s], ys['proj'][s], eps)
    name = f'mlp.M{M}.C{C}'
    widths = BE.quarters_equal(launch, M, ys, name=name + '.')
    REPORT[name + '.quarters_equal'] = 'identical: ' + ', '.join(f'{k} ({rb} B rows)' for k, rb in widths.items())
    rows = BE.slabs_of_interest(M, [C * 4, C * 2]).rows()
    idx = torch.from_numpy(rows).to(DEV)
    xd = x[idx].double()
    units = {'row': (1, C), 'tile': (32, 32)}      # (the gathered rows are not consecutive: no 32-row wave unit; a tile here is 32 judged rows)
    for form in ys:
        if form == 'norm':
            base = xd
            e, m = (_mlp64(a_n[idx].double(), None, w1, b1, w2, b2, xd, md) for md in (False, True))
        elif form == 'raw':
            ad = a_raw[idx].double()
            base = xd
            e, m = (_mlp64(ad, ad, w1, b1, w2, b2, xd, md) for md in (False, True))
        else:
            base = xd if form == 'from_x' else xd + o[idx].double() @ wp.double().t() + bp.double()
            s = base - base[:, :1]
            e = _mlp64(s, s, w1, b1, w2, b2, base, False)
            m = _mlp64(LE.bf16_round(s), s, w1, b1, w2, b2, base, True)
        gate_model(f'{name}.{form}', ys[form][idx].double() - base, e - base, m - base, 'mlp', units)
        for u in units:
            v = LP_REPORT.pop(f'{name}.{form}.{u}')
            LP_REPORT.pop(f'{name}.{form}.{u}.per_unit', None)
            row = int(rows[v['row']])
            note(f'{name}.{form}.{u}', v['gate'], v['value'], v['against'], row, v['col'], BE.side(row, C * 4), dict(rows_judged=len(rows)))


# ------------------------------------------------------------------------------------------------------------- 3. weight gradients
def _integer_weight_gradient(ops, tag, M, N, K, kind):
    """The split-sum bound is a worst case: on random operands the measured error sits five orders below it, and rows read from the wrong
    place would still pass.  So the same launch once more on operands that make fp32 EXACT: integers in [-2, 2], every product an integer of
    magnitude <= 4, every partial sum of up to M of them below 2^24 (M x 4 < 2^24) -- exact in fp32 in any order and under any split
    plan.  dW and db must then equal the float64 product in every bit; a row read twice, skipped or paired with another row's partner does
    not (every row is drawn independently)."""
    assert 4 * M < 1 << 24
    g = torch.Generator(device=DEV).manual_seed(N + K)
    dy = torch.randint(-2, 3, (M, N), device=DEV, generator=g, dtype=torch.int8)
    a = torch.randint(-2, 3, (M, K), device=DEV, generator=g, dtype=torch.int8)
    dw, db = nan(N, K, dtype=F32), nan(N, dtype=F32)
    if kind == 'bf16':
        ops.gemm_tn(dy.to(BF), a.to(BF), dw, db)
    elif kind == 'fp32':
        ops.gemm_tn(dy.float(), a.float(), dw, db)
    else:      # the lo planes of integers are zero
        ops.gemm_tn(ops.split(dy.float()), ops.split(a.float()), dw, db)
    torch.cuda.synchronize()
    x = torch.zeros(N, K, device=DEV, dtype=torch.float64)
    s = torch.zeros(N, device=DEV, dtype=torch.float64)
    for r0, r1 in LE.slabs(M, 1 << 17):
        p = dy[r0:r1].double()
        x += p.t() @ a[r0:r1].double()
        s += p.sum(0)
    bad_w, bad_b = int((dw.double() != x).sum()), int((db.double() != s).sum())
    REPORT[tag + '.integer_operands'] = f'{bad_w} of {N * K} elements of dW and {bad_b} of {N} of db differ from the exact product'
    assert bad_w == 0 and bad_b == 0, f'{tag}: {REPORT[tag + ".integer_operands"]} (exact in fp32 whatever the order)'


@pytest.mark.parametrize('M,N,K', [(M256, 1536, 512), (M256, 512, 1024), (M256, 1024, 512), (BE.M_RAGGED[1], 512, 512)])
def test_weight_gradient(ops, M, N, K):
    """gemm_tn in bf16 with and without db.  The contraction runs over M and the split count follows M (localerr.tn_splits), so the quarters
    do not reproduce the bits: dW and db against the float64 product of ALL rows (a split that reads past a crossing from the wrong
    place fails the bound), and three launches bit-identical"""
    dy, a = rows_scaled(M, N, seed=N + 4, dtype=BF), rows_scaled(M, K, seed=K + 5, dtype=BF)
    dw, db = nan(N, K, dtype=F32), nan(N, dtype=F32)
    assert N * K < 1 << 31      # mbx_gemm_tn's own size check
    ops.gemm_tn(dy, a, dw, db)
    torch.cuda.synchronize()
    x = torch.zeros(N, K, device=DEV, dtype=torch.float64)
    amp = torch.zeros_like(x)
    s = torch.zeros(N, device=DEV, dtype=torch.float64)
    sa = torch.zeros_like(s)
    for r0, r1 in LE.slabs(M):
        p, q = dy[r0:r1].double(), a[r0:r1].double()
        x += p.t() @ q
        amp += p.abs().t() @ q.abs()
        s += p.sum(0)
        sa += p.abs().sum(0)
        del p, q
    splits = LE.tn_splits(M, N, K, False)
    assert int(ops.lib.mbx_gemm_tn_ws(M, N, K)) >= splits * (N * K + 4 * N) * 4 + 256
    tag = f'gemm_tn.bf16.{M}x{N}x{K}'
    b = LE.bound_check(dw, x, LE.split_sum_bound(x, amp, M, splits))
    note(tag + '.dw', 'bound', b['ratio'], 1.0, b['row'], b['col'], '', dict(violations=b['violations'], splits=splits))
    assert b['violations'] == 0, f'{tag}.dw: {b["violations"]} elements outside split_sum_bound, the worst at {b["ratio"]:.3g} x at ({b["row"]}, {b["col"]})'
    c = LE.row_abs_rel_check(db, s, (-(-M // splits) + 64 + 4 * splits) * U * sa, LE.R_F32)
    note(tag + '.db', 'bound', c['ratio'], 1.0, c['row'], 0)
    assert c['ratio'] <= 1.0, f'{tag}.db: column {c["row"]} at {c["ratio"]:.2f} x its bound'
    dw_nob = nan(N, K, dtype=F32)
    ops.gemm_tn(dy, a, dw_nob, None)
    torch.cuda.synchronize()
    assert BE.first_difference(dw_nob, dw) is None, f'{tag}: dw differs between the launches with and without db'
    thrice(tag, lambda: ops.gemm_tn(dy, a, dw, db), [dw, db])
    del dy, a
    _integer_weight_gradient(ops, tag, M, N, K, 'bf16')


# ------------------------------------------------------------------------------------------------------------- 4. attention
B256, H8, HD = 256, 8, 64
DROP = (0.1, 0x1234567890ABCDEF)


def _attn_inputs(dtype, seed=1):
    """qkv [M256, 1536] with a per-row scale in [1, 2] on q (row maxima, lse and delta differ from row to row; no softmax saturates) and dO"""
    C = H8 * HD
    qkv = rnd(M256, 3 * C, seed=seed)
    qkv[:, :C] *= 1.0 + 0.5 * rnd(M256, 1, seed=seed + 1).abs_().clamp_max_(2.0)
    return (qkv if dtype == F32 else qkv.to(dtype)), rnd(M256, C, seed=seed + 2, dtype=dtype), C


def _clips_of_interest(row_bytes):
    """whole clips: the first, the last, those within 512 rows of a crossing of the given tensors, one sampled"""
    rows = BE.slabs_of_interest(M256, row_bytes, unit=CLIP, sample=CLIP).rows()
    clips = sorted(set((rows // CLIP).tolist()))
    return clips, torch.from_numpy(rows).to(DEV), rows


def _lse_bound(qkv_rows, n, tm, C, scale):
    """|lse - exact| <= abs + 2^-23 |lse| (test_gpu_local_parity.py, _attention_case): hd exact products per score in fp32, L exponentials"""
    L = T_FRAMES if tm else J
    q5, k5 = qkv_rows[:, :C].double().reshape(-1, H8, HD), qkv_rows[:, C:2 * C].double().reshape(n, T_FRAMES, J, H8, HD)
    kmax = (k5.abs().amax(1, keepdim=True) if tm else k5.abs().amax(2, keepdim=True)).expand(n, T_FRAMES, J, H8, HD).reshape(-1, H8, HD)
    return (HD + 2) * U * scale * (q5.abs() * kmax).sum(-1) + (L + 8) * U


@pytest.mark.parametrize('mode', [MODE_SPATIAL, MODE_TEMPORAL])
def test_attention_bf16(ops, mode):
    """attn_fwd, attn_bwd and attn_bwd_stats at B = 256, T = 243: quarters_equal over clips, and the 2 x rounding-model gate on the clips
    that hold the crossing of qkv / dqkv (bf16 [M, 1536]: row 699,051), the first and the last clip and a sampled one"""
    from tests.test_gpu_local_parity import REPORT as LP_REPORT, gate_model
    tm = mode == MODE_TEMPORAL
    qkv, do, C = _attn_inputs(BF)
    scale = HD ** -0.5
    name = f'attn.bf16.{"tm" if tm else "sp"}.B{B256}'
    clips, idx, rows = _clips_of_interest([3 * C * 2, C * 2, H8 * 4])
    n = len(clips)
    assert {0, B256 - 1}.issubset(clips) and all(r // CLIP in clips for r in BE.crossings(M256, 3 * C * 2).values())      # (row 699,051)
    # float64 on the chosen clips: exact and rounding model (localerr.attn_fwd_ref / attn_bwd_ref), a clip at a time
    ex_o, md_o, ex_l, ex_d, md_d = [], [], [], [], []
    variant = 'fused' if tm else 'small'
    for c in clips:
        sl = slice(c * CLIP, (c + 1) * CLIP)
        e_o, e_l = LE.attn_fwd_ref(qkv[sl], 1, T_FRAMES, J, H8, scale, tm, False)
        m_o, _ = LE.attn_fwd_ref(qkv[sl], 1, T_FRAMES, J, H8, scale, tm, True)
        ex_o.append(e_o), md_o.append(m_o), ex_l.append(e_l)
        ex_d.append(LE.attn_bwd_ref(qkv[sl], e_o, do[sl], e_l, 1, T_FRAMES, J, H8, scale, tm, False))
        md_d.append(LE.attn_bwd_ref(qkv[sl], LE.bf16_round(e_o), do[sl], e_l.float(), 1, T_FRAMES, J, H8, scale, tm, True, variant=variant))
    ex_o, md_o, ex_l, ex_d, md_d = (torch.cat(t) for t in (ex_o, md_o, ex_l, ex_d, md_d))
    # forward
    fwd = dict(o=nan(M256, C), lse=nan(M256, H8, dtype=F32))

    def launch_fwd(r0, r1):
        ops.attn_fwd(qkv[r0:r1], fwd['o'][r0:r1], fwd['lse'][r0:r1], (r1 - r0) // CLIP, T_FRAMES, J, H8, scale, mode)
    w = BE.quarters_equal(launch_fwd, M256, fwd, name=name + '.fwd.')
    REPORT[name + '.fwd.quarters_equal'] = 'identical: ' + ', '.join(f'{k} ({rb} B rows)' for k, rb in w.items())
    seq_row = (lambda r: (int(rows[r]) // J) % T_FRAMES) if tm else (lambda r: int(rows[r]) % J)
    units = {'row': (1, C), 'row_head': (1, HD)}

    def judged(tag, got, exact, model, rb):
        gate_model(tag, got, exact, model, 'attn', units, seq_row)
        for u in units:
            v = LP_REPORT.pop(f'{tag}.{u}')
            LP_REPORT.pop(f'{tag}.{u}.per_unit', None)
            row = int(rows[v['row']])
            note(f'{tag}.{u}', v['gate'], v['value'], v['against'], row, v['col'], BE.side(row, rb), dict(clips=clips))
    judged(name + '.fwd.o', fwd['o'][idx], ex_o, md_o, C * 2)
    b = LE.row_abs_rel_check(fwd['lse'][idx], ex_l, _lse_bound(qkv[idx], n, tm, C, scale), 2 * U)
    note(name + '.fwd.lse', 'bound', b['ratio'], 1.0, int(rows[b['row']]), b['col'], BE.side(int(rows[b['row']]), 3 * C * 2))
    assert b['ratio'] <= 1.0, f'{name}.fwd.lse: token row {int(rows[b["row"]])} at {b["ratio"]:.2f} x its bound'
    # backward: fed with the kernel's own forward output, except on the judged clips, which get the exact output rounded once and the
    # exact lse (what the rounding model assumes) -- inside the same launches on all rows
    o_in, lse_in = fwd['o'].clone(), fwd['lse'].clone()
    o_in[idx], lse_in[idx] = LE.bf16_round(ex_o).to(BF), ex_l.float()
    del fwd
    bias_f, rsum = rnd(3 * C, seed=3, scale=0.3), rnd(3 * C, seed=4)
    bwd = dict(dqkv=nan(M256, 3 * C), stats_dqkv=nan(M256, 3 * C), part=nan(M256, 2 * H8, 2, dtype=F32))

    def launch_bwd(r0, r1):
        s, nb = slice(r0, r1), (r1 - r0) // CLIP
        ops.attn_bwd(qkv[s], o_in[s], do[s], lse_in[s], bwd['dqkv'][s], nb, T_FRAMES, J, H8, scale, mode)
        part = nan(2 * H8, r1 - r0, 2, dtype=F32)      # block-major in the kernel's layout: kept row-major here so that the quarters line up
        ops.attn_bwd_stats(qkv[s], o_in[s], do[s], lse_in[s], bwd['stats_dqkv'][s], bias_f, rsum, part, nb, T_FRAMES, J, H8, scale, mode)
        bwd['part'][s] = part.transpose(0, 1)
    w = BE.quarters_equal(launch_bwd, M256, bwd, name=name + '.bwd.')
    REPORT[name + '.bwd.quarters_equal'] = 'identical: ' + ', '.join(f'{k} ({rb} B rows)' for k, rb in w.items())
    assert BE.first_difference(bwd['dqkv'], bwd['stats_dqkv']) is None, f'{name}: attn_bwd_stats writes another dqkv than attn_bwd'
    dq = bwd['dqkv'][idx]
    for i, nm in enumerate(('dq', 'dk', 'dv')):
        cs = slice(i * C, (i + 1) * C)
        judged(f'{name}.bwd.{nm}', dq[:, cs], ex_d[:, cs], md_d[:, cs], 3 * C * 2)
    own, amp = LE.attn_stats_ref(dq, qkv[idx], bias_f, rsum, H8)      # [2H, rows, 2]
    got = bwd['part'][idx].transpose(0, 1)
    m = len(rows)
    b = LE.row_abs_rel_check(got.reshape(2 * H8 * m, 2), own.reshape(2 * H8 * m, 2), 2 * (2 * HD) * U * amp.reshape(2 * H8 * m, 2), U)
    row = int(rows[b['row'] % m])
    note(name + '.bwd.part', 'bound', b['ratio'], 1.0, row, b['row'] // m, BE.side(row, 3 * C * 2))
    assert b['ratio'] <= 1.0, f'{name}.bwd.part: token row {row}, block {b["row"] // m}: {b["ratio"]:.2f} x its bound'


@pytest.mark.parametrize('mode', [MODE_SPATIAL, MODE_TEMPORAL])
def test_attention_probability_dropout(ops, mode):
    """The mask of dropmask.py is a hash of the element's index in the reference's attention tensor, which runs over the whole batch: at 256
    clips up to 2,055,849,984 (temporal; below 2^31 -- tests/test_bigerr.py).  The entries take no mask offset, so a quarter cannot
    reproduce it: judged on the chosen clips, whose masks are built from their own indices in the full batch."""
    from tests.test_gpu_local_parity import REPORT as LP_REPORT, gate_model
    tm = mode == MODE_TEMPORAL
    assert BE.attn_mask_elements(B256, T_FRAMES, J, H8, tm) < BE.MARK31
    qkv, do, C = _attn_inputs(BF, seed=11)
    scale = HD ** -0.5
    name = f'attn.bf16.{"tm" if tm else "sp"}.B{B256}.drop'
    clips, idx, rows = _clips_of_interest([3 * C * 2, C * 2, H8 * 4])
    variant = 'split' if tm else 'small'
    ex_o, md_o, ex_l, ex_d, md_d = [], [], [], [], []
    for c in clips:
        sl = slice(c * CLIP, (c + 1) * CLIP)
        drop = DROP + ([c],)      # (p, seed, the clip's number in the batch the mask index runs over)
        e_o, e_l = LE.attn_fwd_ref(qkv[sl], 1, T_FRAMES, J, H8, scale, tm, False, drop)
        m_o, _ = LE.attn_fwd_ref(qkv[sl], 1, T_FRAMES, J, H8, scale, tm, True, drop)
        ex_o.append(e_o), md_o.append(m_o), ex_l.append(e_l)
        ex_d.append(LE.attn_bwd_ref(qkv[sl], e_o, do[sl], e_l, 1, T_FRAMES, J, H8, scale, tm, False, drop))
        md_d.append(LE.attn_bwd_ref(qkv[sl], LE.bf16_round(e_o), do[sl], e_l.float(), 1, T_FRAMES, J, H8, scale, tm, True, drop, variant=variant))
    ex_o, md_o, ex_l, ex_d, md_d = (torch.cat(t) for t in (ex_o, md_o, ex_l, ex_d, md_d))
    o, lse = nan(M256, C), nan(M256, H8, dtype=F32)
    ops.attn_fwd(qkv, o, lse, B256, T_FRAMES, J, H8, scale, mode, drop=DROP)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
    seq_row = (lambda r: (int(rows[r]) // J) % T_FRAMES) if tm else (lambda r: int(rows[r]) % J)
    units = {'row': (1, C), 'row_head': (1, HD)}

    def judged(tag, got, exact, model, rb):
        gate_model(tag, got, exact, model, 'attn', units, seq_row)
        for u in units:
            v = LP_REPORT.pop(f'{tag}.{u}')
            LP_REPORT.pop(f'{tag}.{u}.per_unit', None)
            row = int(rows[v['row']])
            note(f'{tag}.{u}', v['gate'], v['value'], v['against'], row, v['col'], BE.side(row, rb), dict(clips=clips))
    judged(name + '.fwd.o', o[idx], ex_o, md_o, C * 2)
    o[idx], lse[idx] = LE.bf16_round(ex_o).to(BF), ex_l.float()
    dqkv = nan(M256, 3 * C)
    ops.attn_bwd(qkv, o, do, lse, dqkv, B256, T_FRAMES, J, H8, scale, mode, drop=DROP)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv).all())
    dq = dqkv[idx]
    for i, nm in enumerate(('dq', 'dk', 'dv')):
        cs = slice(i * C, (i + 1) * C)
        judged(f'{name}.bwd.{nm}', dq[:, cs], ex_d[:, cs], md_d[:, cs], 3 * C * 2)


@pytest.mark.parametrize('mode', [MODE_SPATIAL, MODE_TEMPORAL])
def test_attention_fp32(ops, mode):
    """fp32 attention (qkv and dqkv fp32 [M, 1536]: 6144-byte rows, crossings at rows 349,526 and 699,051): quarters_equal, the lse bound on
    the clips of interest, and the operand planes of the backward bit for bit the split of its fp32 output.  There is no rounding model
    for the fp32 kernels (localerr.py); their whole-tensor comparison stays with tests/test_gpu_kernels.py."""
    tm = mode == MODE_TEMPORAL
    qkv, do, C = _attn_inputs(F32, seed=21)
    scale = HD ** -0.5
    name = f'attn.fp32.{"tm" if tm else "sp"}.B{B256}'
    clips, idx, rows = _clips_of_interest([3 * C * 4, C * 4, H8 * 4])
    assert {0, B256 - 1}.issubset(clips) and all(r // CLIP in clips for r in BE.crossings(M256, 3 * C * 4).values())
    fwd = dict(o=nan(M256, C, dtype=F32), lse=nan(M256, H8, dtype=F32))

    def launch_fwd(r0, r1):
        ops.attn_fwd(qkv[r0:r1], fwd['o'][r0:r1], fwd['lse'][r0:r1], (r1 - r0) // CLIP, T_FRAMES, J, H8, scale, mode)
    w = BE.quarters_equal(launch_fwd, M256, fwd, name=name + '.fwd.')
    REPORT[name + '.fwd.quarters_equal'] = 'identical: ' + ', '.join(f'{k} ({rb} B rows)' for k, rb in w.items())
    ex_l = torch.cat([LE.attn_fwd_ref(qkv[c * CLIP:(c + 1) * CLIP], 1, T_FRAMES, J, H8, scale, tm, False)[1] for c in clips])
    # fp32 operands: the hd products of a score are rounded too (fused multiply-adds: one rounding each, bounded by the same amplitude)
    b = LE.row_abs_rel_check(fwd['lse'][idx], ex_l, _lse_bound(qkv[idx], len(clips), tm, C, scale), 2 * U)
    note(name + '.fwd.lse', 'bound', b['ratio'], 1.0, int(rows[b['row']]), b['col'], BE.side(int(rows[b['row']]), 3 * C * 4))
    assert b['ratio'] <= 1.0, f'{name}.fwd.lse: token row {int(rows[b["row"]])} at {b["ratio"]:.2f} x its bound'
    o, lse = fwd['o'], fwd['lse']
    bwd = dict(dqkv=nan(M256, 3 * C, dtype=F32), hi=nan(M256, 3 * C), lo=nan(M256, 3 * C))

    def launch_bwd(r0, r1):
        s, nb = slice(r0, r1), (r1 - r0) // CLIP
        ops.attn_bwd(qkv[s], o[s], do[s], lse[s], bwd['dqkv'][s], nb, T_FRAMES, J, H8, scale, mode)
        ops.attn_bwd(qkv[s], o[s], do[s], lse[s], (bwd['hi'][s], bwd['lo'][s]), nb, T_FRAMES, J, H8, scale, mode)
    w = BE.quarters_equal(launch_bwd, M256, bwd, name=name + '.bwd.')
    REPORT[name + '.bwd.quarters_equal'] = 'identical: ' + ', '.join(f'{k} ({rb} B rows)' for k, rb in w.items())
    hi, lo = ops.split(bwd['dqkv'])
    torch.cuda.synchronize()
    for k, t in (('hi', hi), ('lo', lo)):
        row = BE.first_difference(bwd[k], t)
        assert row is None, f'{name}: plane {k} differs from the split of the fp32 dqkv first in row {row} ({BE.side(row, 3 * C * 2)} of the plane)'


# ------------------------------------------------------------------------------------------------------------- 7. the fp32 class
@pytest.mark.parametrize('N,K', [(1536, 512), (1024, 512)])
def test_gemm_nt_fp32_and_x3(ops, N, K):
    """fp32 outputs [M, 1536] and [M, 1024] (6144- and 4096-byte rows: both marks inside the tensor): gemm_nt in fp32 and gemm_nt_x3, STORE and
    GELU, with the fp32 bounds of test_tile256_x3 (R_F32; K terms for the fp32 kernel, 3 K for the three bf16 passes)"""
    M = M256
    assert gemm_nt_fits(M, N, K)
    a32, w32, bias = rows_scaled(M, K, seed=N), rnd(N, K, seed=N + 1, scale=0.05), rnd(N, seed=N + 2, scale=0.5)
    (ah, al), (wh, wl) = ops.split(a32), ops.split(w32)
    outs = dict(f32_store=nan(M, N, dtype=F32), f32_gelu=nan(M, N, dtype=F32), x3_store=nan(M, N, dtype=F32), x3_gelu=nan(M, N, dtype=F32))

    def launch(r0, r1):
        s = slice(r0, r1)
        ops.gemm_nt(a32[s], w32, bias, EPI_STORE, out_t=outs['f32_store'][s])
        ops.gemm_nt(a32[s], w32, bias, EPI_GELU, out_t=None, out2_t=outs['f32_gelu'][s])
        ops.gemm_nt((ah[s], al[s]), (wh, wl), bias, EPI_STORE, out_t=outs['x3_store'][s])
        ops.gemm_nt((ah[s], al[s]), (wh, wl), bias, EPI_GELU, out_t=None, out2_t=outs['x3_gelu'][s])

    def refs(idx):
        bd = bias.double()
        x, amp = prod(a32[idx], w32, bias)      # fp32 operands: K fused multiply-adds, each rounded once and bounded by the amplitude
        f_st = (x, LE.elementwise_bound(x, amp, K, LE.R_F32, ops=3, mag64=amp + bd.abs()))
        f_g = (LE.gelu64(x), LE.elementwise_bound(LE.gelu64(x), amp, K, LE.R_F32, lip=LE.GELU_LIP, ops=5, eabs=LE.gelu_eabs(x), mag64=amp + bd.abs()))
        Hh, Ll, WH, WL = ah[idx].double(), al[idx].double(), wh.double(), wl.double()
        x = Hh @ WH.t() + Hh @ WL.t() + Ll @ WH.t() + bd
        amp = Hh.abs() @ WH.abs().t() + Hh.abs() @ WL.abs().t() + Ll.abs() @ WH.abs().t()
        x_st = (x, LE.elementwise_bound(x, amp, 3 * K, LE.R_F32, ops=3, mag64=amp + bd.abs()))
        x_g = (LE.gelu64(x), LE.elementwise_bound(LE.gelu64(x), amp, 3 * K, LE.R_F32, lip=LE.GELU_LIP, ops=5, eabs=LE.gelu_eabs(x), mag64=amp + bd.abs()))
        return dict(f32_store=f_st, f32_gelu=f_g, x3_store=x_st, x3_gelu=x_g)
    rows_case(f'fp32class.gemm_nt.{M}x{N}x{K}', M, launch, outs, [K * 4, K * 2], refs)


@pytest.mark.parametrize('kind', ['fp32', 'x3'])
def test_weight_gradient_fp32_class(ops, kind):
    """gemm_tn in fp32 and gemm_tn_x3 at M256 x 1536 x 512 (dY fp32 [M, 1536] passes both marks), gated like the bf16 weight gradient.  x3:
    split_sum_bound with the restated split count, as test_weight_gradient.  fp32: the launch plan of the fp32 kernels has no restatement
    in localerr.py, so the bound is the one that holds for ANY order of summing the M products in fp32 (split_sum_bound with one split)."""
    M, N, K = M256, 1536, 512
    dy32, a32 = rows_scaled(M, N, seed=N + 4), rows_scaled(M, K, seed=K + 5)
    dw, db = nan(N, K, dtype=F32), nan(N, dtype=F32)
    if kind == 'x3':
        dyp, ap = ops.split(dy32), ops.split(a32)
        del dy32, a32
        args = (dyp, ap)
        terms, col = [(dyp[0], ap[0]), (dyp[0], ap[1]), (dyp[1], ap[0])], [dyp[0], dyp[1]]
        splits = LE.tn_splits(M, N, K, True)
        assert int(ops.lib.mbx_gemm_tn_x3_workspace(M, N, K)) == splits * (N * K + 4 * N) * 4 + 256
    else:
        args = (dy32, a32)
        terms, col = [(dy32, a32)], [dy32]
        splits = 1
    ops.gemm_tn(*args, dw, db)
    torch.cuda.synchronize()
    x = torch.zeros(N, K, device=DEV, dtype=torch.float64)
    amp = torch.zeros_like(x)
    for r0, r1 in LE.slabs(M):
        for p, q in terms:
            pd, qd = p[r0:r1].double(), q[r0:r1].double()
            x += pd.t() @ qd
            amp += pd.abs().t() @ qd.abs()
    tag = f'gemm_tn.{kind}.{M}x{N}x{K}'
    b = LE.bound_check(dw, x, LE.split_sum_bound(x, amp, len(terms) * M, splits))
    note(tag + '.dw', 'bound', b['ratio'], 1.0, b['row'], b['col'], '', dict(violations=b['violations'], splits=splits))
    assert b['violations'] == 0, f'{tag}.dw: {b["violations"]} elements outside split_sum_bound, the worst at {b["ratio"]:.3g} x at ({b["row"]}, {b["col"]})'
    s = sum(c.double().sum(0) for c in col)
    sa = sum(c.double().abs().sum(0) for c in col)
    c = LE.row_abs_rel_check(db, s, (-(-len(col) * M // splits) + 64 + 4 * splits) * U * sa, LE.R_F32)
    note(tag + '.db', 'bound', c['ratio'], 1.0, c['row'], 0)
    assert c['ratio'] <= 1.0, f'{tag}.db: column {c["row"]} at {c["ratio"]:.2f} x its bound'
    thrice(tag, lambda: ops.gemm_tn(*args, dw, db), [dw, db])
    del args, terms, col
    _integer_weight_gradient(ops, tag, M, N, K, kind)


# ------------------------------------------------------------------------------------------------------------- 8. the model
FULL = dict(dim_in=3, dim_out=3, dim_feat=512, dim_rep=512, depth=5, num_heads=8, mlp_ratio=2, num_joints=17, maxlen=243)


def test_full_model_256_clips_equal_four_times_64():
    """The full model in bf16 with recompute (the mode of the benchmark's full_model_b256) at [256, 243, 17, 3]: the output of the 256-clip
    forward is, bit for bit, the outputs of the four 64-clip forwards -- in the training sequencing and under no_grad; the parameter
    gradients are the sum of the four sub-batches' within the split-additivity gate of test_full_size_properties (rel < 2e-3: different
    token counts, different dW split counts); everything is finite."""
    from tests.helpers import build_model, make_input, trained_like
    model = build_model(FULL, seed=0)
    trained_like(model, 1)
    model = model.to(DEV)
    model.precision = 'bf16'
    model.recompute = True
    x = make_input(B256, T_FRAMES, J, 77).to(DEV)
    cot = torch.randn(B256, T_FRAMES, J, 3, generator=torch.Generator().manual_seed(78)).to(DEV)

    def fwd_bwd(xx, cc):
        model.zero_grad(set_to_none=True)
        out = model(xx)
        (out * cc).sum().backward()
        return out.detach(), torch.cat([p.grad.flatten() for p in model.parameters()])
    out, g = fwd_bwd(x, cot)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
    with torch.no_grad():
        out_ng = model(x)
    assert bool(torch.isfinite(out_ng).all())
    gsum = torch.zeros_like(g)
    for q in range(4):
        s = slice(64 * q, 64 * (q + 1))
        oq, gq = fwd_bwd(x[s], cot[s])
        row = BE.first_difference(out[s].reshape(M_STEP, 3), oq.reshape(M_STEP, 3))
        assert row is None, f'training forward: clips {64 * q}:{64 * q + 64} differ from the 256-clip forward first in token row {64 * q * CLIP + row}'
        gsum += gq
        with torch.no_grad():
            oq = model(x[s])
        row = BE.first_difference(out_ng[s].reshape(M_STEP, 3), oq.reshape(M_STEP, 3))
        assert row is None, f'no-grad forward: clips {64 * q}:{64 * q + 64} differ from the 256-clip forward first in token row {64 * q * CLIP + row}'
    rel = float((gsum - g).norm() / g.norm())
    REPORT['full_model_b256.split_additivity.recompute'] = rel
    assert rel < 2e-3, rel


# ------------------------------------------------------------------------------------------------------------- the engine's row limit
@pytest.mark.parametrize('name', ['lite_2x81', 'full_1x243'])
def test_folded_backward_on_the_tile_fallback(ops, monkeypatch, name):
    """engine.ROW_OFFSET_LIMIT patched below the fixtures' sizes: the engine takes the tile kernels (gemm_nt_lnbwd with its row dots,
    the residual GEMM + LayerNorm) where it would have taken mbx_rows_lnbwd_t / mbx_rows_resid_ln, and the fixtures of
    test_folded_backward_equals_plain_backward pass their gates on that path"""
    from tests.test_gpu_fold import test_folded_backward_equals_plain_backward as gates
    monkeypatch.setattr(engine, 'ROW_OFFSET_LIMIT', 1 << 16)      # the fixtures' tensors: 2,754 x 256 x 2 bytes and more
    calls = dict(rows=0, tile=0)

    def spy(fn, key):
        def f(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return f
    for nm in ('rows_lnbwd_t', 'rows_resid_ln'):
        monkeypatch.setattr(ops, nm, spy(getattr(ops, nm), 'rows'), raising=False)
    monkeypatch.setattr(ops, 'gemm_nt_lnbwd', spy(ops.gemm_nt_lnbwd, 'tile'), raising=False)
    gates(name)
    assert calls['rows'] == 0 and calls['tile'] > 0, calls


# ------------------------------------------------------------------------------------------------------------- 5. row-wise kernels
def _row_case(name, M, launch, outs):
    widths = BE.quarters_equal(launch, M, outs, name=name + '.')
    REPORT[name + '.quarters_equal'] = 'identical: ' + ', '.join(f'{k} ({rb} B rows)' for k, rb in widths.items())
    return widths


def _gate_b(name, got, ref64, model, rows, rb):
    """rowerr.gate_rows (worst row within 2 x the rounding model's, every row within per_unit_excess), as tests/test_gpu_row_parity.py"""
    from tests import rowerr as RE
    g, m, px, ok, msg = RE.gate_rows(got, ref64, model)
    row = int(rows[g['row']])
    note(name, '2 x model', g['worst'], m['worst'], row, 0, BE.side(row, rb), dict(exempt=m['exempt'], per_unit_excess=px['excess'], rows_judged=len(rows)))
    assert m['exempt'] == 0 and ok, f'{name}: {msg} (row {g["row"]} of the judged rows is row {row}: {BE.side(row, rb)})'


def _gate_a(name, got, x64, bound64, rows, rb):
    b = LE.bound_check(got.reshape(len(got), -1), x64.reshape(len(got), -1), bound64.expand(x64.shape).reshape(len(got), -1))
    row = int(rows[b['row']]) if rows is not None else b['row']
    note(name, 'bound', b['ratio'], 1.0, row, b['col'], BE.side(row, rb) if rows is not None else '', dict(violations=b['violations']))
    assert b['violations'] == 0, f'{name}: {b["violations"]} elements outside the bound, the worst at {b["ratio"]:.3f} x in row {row}'


@pytest.mark.parametrize('C', [512, 1024])
def test_layernorm_rows(ops, C):
    """layernorm_fwd (fp32 and bf16 output, and the operand planes) and layernorm_bwd (bf16 and fp32 gradients; dx is fp32: at C = 1024 its
    4096-byte rows pass both marks) at M256 rows, with the gates of tests/test_gpu_row_parity.py on the slabs; dgamma / dbeta, reduced
    over all rows, against float64 over all rows with rowerr.ln_bwd_param_bounds"""
    from tests import rowerr as RE
    M, eps = M256, RE.f32(1e-6)
    x = rows_scaled(M, C, seed=C, offset=0.0)
    gamma, beta = 1.0 + 0.2 * rnd(C, seed=1), 0.3 * rnd(C, seed=2)
    fwd = dict(y32=nan(M, C, dtype=F32), y16=nan(M, C), hi=nan(M, C), lo=nan(M, C), mean=nan(M, dtype=F32), rstd=nan(M, dtype=F32),
               mean16=nan(M, dtype=F32), rstd16=nan(M, dtype=F32), mean_p=nan(M, dtype=F32), rstd_p=nan(M, dtype=F32))

    def launch(r0, r1):
        s = slice(r0, r1)
        ops.layernorm_fwd(x[s], gamma, beta, eps, fwd['y32'][s], fwd['mean'][s], fwd['rstd'][s])
        ops.layernorm_fwd(x[s], gamma, beta, eps, fwd['y16'][s], fwd['mean16'][s], fwd['rstd16'][s])
        ops.layernorm_fwd(x[s], gamma, beta, eps, (fwd['hi'][s], fwd['lo'][s]), fwd['mean_p'][s], fwd['rstd_p'][s])
    name = f'ln.M{M}.C{C}'
    _row_case(name + '.fwd', M, launch, fwd)
    for k in ('mean16', 'mean_p'):
        assert BE.first_difference(fwd[k], fwd['mean']) is None and BE.first_difference(fwd['rstd' + k[4:]], fwd['rstd']) is None, k
    for r0, r1 in BE.quarters(M):      # the planes are the split of the fp32 output, the bf16 output its rounding: over the whole tensor
        hi, lo = RE.split_planes(fwd['y32'][r0:r1])
        assert RE.same_bits(fwd['hi'][r0:r1], hi) and RE.same_bits(fwd['lo'][r0:r1], lo), f'{name}: planes differ from the split of y in rows {r0}:{r1}'
    rows = BE.slabs_of_interest(M, [C * 4, C * 2]).rows()
    idx = torch.from_numpy(rows).to(DEV)
    xs = x[idx]
    ref, mu64, rs64 = RE.ln_fwd_ref64(xs, gamma, beta, eps)
    bm, br = RE.ln_stat_bounds(xs, eps)
    _gate_b(name + '.fwd.y32', fwd['y32'][idx], ref, RE.ln_fwd_model(xs, gamma, beta, eps, F32)[0], rows, C * 4)
    _gate_b(name + '.fwd.y16', fwd['y16'][idx], ref, RE.ln_fwd_model(xs, gamma, beta, eps, BF)[0], rows, C * 4)
    _gate_a(name + '.fwd.mean', fwd['mean'][idx], mu64, bm, rows, C * 4)
    _gate_a(name + '.fwd.rstd', fwd['rstd'][idx], rs64, br, rows, C * 4)
    mean, rstd = fwd['mean'], fwd['rstd']
    del fwd
    dres = rnd(M, C, seed=5)
    for dt in (BF, F32):
        dy = rnd(M, C, seed=4, dtype=dt)
        bwd = dict(dx=nan(M, C, dtype=F32), dx_t=nan(M, C, dtype=dt))
        dg, db = nan(C, dtype=F32), nan(C, dtype=F32)

        def launch_b(r0, r1):
            s = slice(r0, r1)
            ops.layernorm_bwd(dy[s], x[s], mean[s], rstd[s], gamma, dres[s], None, bwd['dx'][s], bwd['dx_t'][s],
                              dg if r1 - r0 == M else torch.empty_like(dg), db if r1 - r0 == M else torch.empty_like(db))
        t = f'{name}.bwd.{"bf16" if dt == BF else "fp32"}'
        _row_case(t, M, launch_b, bwd)
        r64 = RE.ln_bwd_ref64(dy[idx], xs, mean[idx], rstd[idx], gamma, dres[idx], None)
        model = RE.ln_bwd_model(dy[idx], xs, mean[idx], rstd[idx], gamma, dres[idx], None)
        _gate_b(t + '.dx', bwd['dx'][idx], r64[0], model[0], rows, C * 4)
        for r0, r1 in BE.quarters(M):
            want = RE.bf16_store(bwd['dx'][r0:r1]) if dt == BF else bwd['dx'][r0:r1]
            assert RE.same_bits(bwd['dx_t'][r0:r1], want), f'{t}: dx_t is not the copy of dx in rows {r0}:{r1}'
        # dgamma / dbeta of the launch on all rows (the first of quarters_equal; the quarters wrote scratch): float64 over all rows, slab by slab
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, dres, None, bwd['dx'], bwd['dx_t'], dg, db)
        torch.cuda.synchronize()
        g64, b64 = torch.zeros(C, device=DEV, dtype=torch.float64), torch.zeros(C, device=DEV, dtype=torch.float64)
        ga, ba = torch.zeros_like(g64), torch.zeros_like(g64)
        for r0, r1 in LE.slabs(M, 1 << 17):
            d = dy[r0:r1].double()
            xh = (x[r0:r1].double() - mean[r0:r1].double()[:, None]) * rstd[r0:r1].double()[:, None]
            g64 += (d * xh).sum(0)
            b64 += d.sum(0)
            ga += (d * xh).abs().sum(0)
            ba += d.abs().sum(0)
        grid, per_wave = RE.grid_rows(M, RE.LN_BLOCKS)
        L = per_wave + 2 + RE.SE.colsum_chain(grid, True)      # rowerr.ln_bwd_param_bounds, with the sums taken slab by slab
        _gate_a(t + '.dgamma', dg[None], g64[None], RE.gam(L + 2) * ga[None], None, 0)
        _gate_a(t + '.dbeta', db[None], b64[None], RE.gam(L) * ba[None], None, 0)
        del dy, bwd


def test_elementwise_copies(ops):
    """gelu_fwd (bf16 [M, 1024]), split (fp32 [M, 1536] -> two planes: the element index passes 2^30, the byte offset both marks), average and
    average_bwd: element-wise kernels whose index runs over the whole tensor -- quarters_equal, and each against its restatement"""
    from tests import rowerr as RE
    M = M256
    u = rnd(M, 1024, seed=1, dtype=BF, scale=1.5)
    g = dict(g=nan(M, 1024))
    _row_case('gelu_fwd.M256x1024', M, lambda r0, r1: ops.gelu_fwd(u[r0:r1], g['g'][r0:r1]), g)
    rows = BE.slabs_of_interest(M, [2048]).rows()
    idx = torch.from_numpy(rows).to(DEV)
    # the gate tests/test_gpu_fold_parity.py has for this kernel (folderr.gelu_gate: every 4-element vector against the fp32 erf form)
    from tests import folderr as FE
    us = u[idx].reshape(-1)
    r = FE.gelu_gate(g['g'][idx].reshape(-1), FE.gelu_ref64(us), FE.gelu_model(us), us)
    row = int(rows[r['unit'] * 4 // 1024])
    note('gelu_fwd.M256x1024', '4 x model', r['ratio'], 1.0, row, r['unit'] * 4 % 1024, BE.side(row, 2048), dict(n_over=r['n_over'], rows_judged=len(rows)))
    assert r['ratio'] <= 1.0, f'gelu_fwd: {r["n_over"]} vectors over their gate, the worst at {r["ratio"]:.3f} x in row {row} ({BE.side(row, 2048)})'
    del u, g
    t = rows_scaled(M, 1536, seed=2)
    pl = dict(hi=nan(M, 1536), lo=nan(M, 1536))

    def launch_split(r0, r1):
        hi, lo = ops.split(t[r0:r1])
        pl['hi'][r0:r1], pl['lo'][r0:r1] = hi, lo
    _row_case('split.M256x1536', M, launch_split, pl)
    for r0, r1 in BE.quarters(M):
        hi, lo = RE.split_planes(t[r0:r1])
        assert RE.same_bits(pl['hi'][r0:r1], hi) and RE.same_bits(pl['lo'][r0:r1], lo), f'split: planes differ from bf16(t), bf16(t - hi) in rows {r0}:{r1}'
    del pl
    t2 = rows_scaled(M, 1536, seed=3)
    av = dict(out=nan(M, 1536, dtype=F32))
    _row_case('average.M256x1536', M, lambda r0, r1: ops.average(t[r0:r1], t2[r0:r1], av['out'][r0:r1]), av)
    for r0, r1 in BE.quarters(M):      # (a + b) / 2 in fp32: one addition, an exact halving
        assert RE.same_bits(av['out'][r0:r1], (t[r0:r1] + t2[r0:r1]) * 0.5), f'average: rows {r0}:{r1}'
    del av, t2
    ab = dict(d_st=nan(M, 1536, dtype=F32), d_ts=nan(M, 1536, dtype=F32), d_st_t=nan(M, 1536), d_ts_t=nan(M, 1536))
    _row_case('average_bwd.M256x1536', M, lambda r0, r1: ops.average_bwd(t[r0:r1], *(ab[k][r0:r1] for k in ('d_st', 'd_ts', 'd_st_t', 'd_ts_t'))), ab)
    for r0, r1 in BE.quarters(M):
        h = t[r0:r1] * 0.5
        assert RE.same_bits(ab['d_st'][r0:r1], h) and RE.same_bits(ab['d_ts'][r0:r1], h), f'average_bwd: rows {r0}:{r1}'
        assert RE.same_bits(ab['d_st_t'][r0:r1], RE.bf16_store(h)) and RE.same_bits(ab['d_ts_t'][r0:r1], RE.bf16_store(h)), f'average_bwd (bf16): rows {r0}:{r1}'


def test_fusion_head_and_tanh_rows(ops):
    """fuse_fwd, fuse_ln_fwd, fuse_bwd / fuse_bwd_pair, head_fwd / head_bwd and tanh_bwd at M256 rows of 512 channels, with the gates of
    tests/test_gpu_row_parity.py: quarters_equal on every row output, rowerr's gates on the slabs, and the parameter gradients -- reduced
    over all rows -- against float64 over all rows with rowerr's bounds for the launch geometry at this M"""
    from tests import rowerr as RE
    M, C, eps = M256, 512, RE.f32(1e-6)
    x_st, x_ts = rnd(M, C, seed=1), rnd(M, C, seed=2)
    w = rnd(2, 2 * C, seed=3, scale=0.5 / (2 * C) ** 0.5)      # logits of standard deviation 0.5 (rowerr.fuse_inputs)
    b = rnd(2, seed=4, scale=0.1)
    fw = dict(out=nan(M, C, dtype=F32), alpha=nan(M, 2, dtype=F32), out2=nan(M, C, dtype=F32), alpha2=nan(M, 2, dtype=F32), xn1=nan(M, C),
              mean=nan(M, dtype=F32), rstd=nan(M, dtype=F32))

    def launch(r0, r1):
        s = slice(r0, r1)
        ops.fuse_fwd(x_st[s], x_ts[s], w, b, fw['out'][s], fw['alpha'][s])
        ops.fuse_ln_fwd(x_st[s], x_ts[s], w, b, fw['out2'][s], fw['alpha2'][s], None, None, fw['xn1'][s], None, None, None, eps, fw['mean'][s], fw['rstd'][s])
    _row_case('fuse_fwd.M256', M, launch, fw)
    assert BE.first_difference(fw['out2'], fw['out']) is None and BE.first_difference(fw['alpha2'], fw['alpha']) is None, 'fuse_ln_fwd: another fused row than fuse_fwd'
    rows = BE.slabs_of_interest(M, [C * 4, C * 2]).rows()
    idx = torch.from_numpy(rows).to(DEV)
    a_s, t_s = x_st[idx], x_ts[idx]
    out64, a64, _, amp = RE.fuse_fwd_ref64(a_s, t_s, w, b)
    m_out, m_alpha = RE.fuse_fwd_model(a_s, t_s, w, b)
    _gate_a('fuse_fwd.M256.alpha', fw['alpha'][idx], a64, RE.fuse_alpha_bound(amp, C, m_alpha, a64).expand(len(rows), 2), rows, C * 4)
    _gate_b('fuse_fwd.M256.out', fw['out'][idx], out64, m_out, rows, C * 4)
    outs = fw['out'][idx]
    bm, br = RE.ln_stat_bounds(outs, eps)
    _, mu64, rs64 = RE.ln_fwd_ref64(outs, None, None, eps)
    _gate_a('fuse_ln_fwd.M256.mean', fw['mean'][idx], mu64, bm, rows, C * 4)
    _gate_a('fuse_ln_fwd.M256.rstd', fw['rstd'][idx], rs64, br, rows, C * 4)
    _gate_b('fuse_ln_fwd.M256.xn1', fw['xn1'][idx], RE.ln_fwd_ref64(outs, None, None, eps)[0], RE.ln_fwd_model(outs, None, None, eps, BF)[0], rows, C * 4)
    alpha = fw['alpha']
    del fw
    # backward: from an fp32 gradient and from a bf16 pair (the same bits as from the pair's fp32 sum)
    dh_a, dh_b = rnd(M, C, seed=7, dtype=BF), rnd(M, C, seed=8, dtype=BF, scale=0.3)
    dh = dh_a.float() + dh_b.float()
    bw = dict(d_st=nan(M, C, dtype=F32), d_ts=nan(M, C, dtype=F32), d_st_t=nan(M, C), d_ts_t=nan(M, C), p_st_t=nan(M, C), p_ts_t=nan(M, C))
    dw, db, dw_p, db_p = nan(2, 2 * C, dtype=F32), nan(2, dtype=F32), nan(2, 2 * C, dtype=F32), nan(2, dtype=F32)

    def launch_b(r0, r1):
        s, full = slice(r0, r1), r1 - r0 == M
        g = (dw, db, dw_p, db_p) if full else tuple(torch.empty_like(t) for t in (dw, db, dw_p, db_p))
        ops.fuse_bwd(dh[s], x_st[s], x_ts[s], alpha[s], w, bw['d_st'][s], bw['d_ts'][s], bw['d_st_t'][s], bw['d_ts_t'][s], g[0], g[1])
        ops.fuse_bwd_pair(dh_a[s], dh_b[s], x_st[s], x_ts[s], alpha[s], w, bw['p_st_t'][s], bw['p_ts_t'][s], g[2], g[3])
    _row_case('fuse_bwd.M256', M, launch_b, bw)
    for k in ('st', 'ts'):
        assert BE.first_difference(bw[f'p_{k}_t'], bw[f'd_{k}_t']) is None, f'fuse_bwd_pair: d_{k}_t differs from fuse_bwd on the pair sum'
        for r0, r1 in BE.quarters(M):
            assert RE.same_bits(bw[f'd_{k}_t'][r0:r1], RE.bf16_store(bw[f'd_{k}'][r0:r1])), f'fuse_bwd: d_{k}_t is not the copy of d_{k} in rows {r0}:{r1}'
    ops.fuse_bwd(dh, x_st, x_ts, alpha, w, bw['d_st'], bw['d_ts'], bw['d_st_t'], bw['d_ts_t'], dw, db)      # (the quarters wrote scratch gradients)
    ops.fuse_bwd_pair(dh_a, dh_b, x_st, x_ts, alpha, w, bw['p_st_t'], bw['p_ts_t'], dw_p, db_p)
    torch.cuda.synchronize()
    assert RE.same_bits(dw_p, dw) and RE.same_bits(db_p, db), 'fuse_bwd_pair: dw / db differ from fuse_bwd on the pair sum'
    r64 = RE.fuse_bwd_ref64(dh[idx], a_s, t_s, alpha[idx], w)
    _, model, _ = RE.fuse_bwd_dot_form(bw['d_st'][idx], dh[idx], a_s, t_s, alpha[idx], w)
    _gate_b('fuse_bwd.M256.d_st', bw['d_st'][idx], r64[0], model[0], rows, C * 4)
    _gate_b('fuse_bwd.M256.d_ts', bw['d_ts'][idx], r64[1], model[1], rows, C * 4)
    del bw
    g64 = torch.zeros(2, 2 * C, device=DEV, dtype=torch.float64)
    b64, gb, bb = torch.zeros(2, device=DEV, dtype=torch.float64), torch.zeros(2, 2 * C, device=DEV, dtype=torch.float64), torch.zeros(2, device=DEV, dtype=torch.float64)
    for r0, r1 in BE.quarters(M):      # float64 and rowerr's bounds a quarter at a time: both are sums over rows
        s = slice(r0, r1)
        q = RE.fuse_bwd_ref64(dh[s], x_st[s], x_ts[s], alpha[s], w)
        g64 += q[2]
        b64 += q[3]
        del q
    # the bound follows the launch geometry at M rows (rows per wave, partial rows of the column sum): taken once over all rows
    pw, pb = RE.fuse_bwd_param_bounds(dh, x_st, x_ts, alpha, w)
    _gate_a('fuse_bwd.M256.dw', dw, g64, pw, None, 0)
    _gate_a('fuse_bwd.M256.db', db[None], b64[None], pb[None] if pb.dim() else pb.reshape(1, 1), None, 0)
    del dh, dh_a, dh_b, x_st, x_ts, alpha, pw, pb
    # head and tanh backward
    R, D = 512, 3
    rep = torch.tanh(rnd(M, R, seed=11, scale=1.5))
    rep[0, 0], rep[M - 1, R - 1], rep[M // 2, 5] = 1.0, -1.0, 0.0
    hw, hb, dout, drep = rnd(D, R, seed=12, scale=0.1), rnd(D, seed=13, scale=0.1), rnd(M, D, seed=14), rnd(M, R, seed=15)
    hd = dict(out=nan(M, D, dtype=F32), dpre=nan(M, R), dpre32=nan(M, R, dtype=F32), tanh_bwd=nan(M, R), tanh_bwd32=nan(M, R, dtype=F32))
    hdw, hdb = nan(D, R, dtype=F32), nan(D, dtype=F32)

    def launch_h(r0, r1):
        s, full = slice(r0, r1), r1 - r0 == M
        g = (hdw, hdb) if full else (torch.empty_like(hdw), torch.empty_like(hdb))
        ops.head_fwd(rep[s], hw, hb, hd['out'][s])
        ops.head_bwd(dout[s], rep[s], hw, hd['dpre'][s], *g)
        ops.head_bwd(dout[s], rep[s], hw, hd['dpre32'][s], torch.empty_like(hdw), torch.empty_like(hdb))
        ops.tanh_bwd(drep[s], rep[s], hd['tanh_bwd'][s])
        ops.tanh_bwd(drep[s], rep[s], hd['tanh_bwd32'][s])
    _row_case('head.M256', M, launch_h, hd)
    ops.head_bwd(dout, rep, hw, hd['dpre'], hdw, hdb)
    torch.cuda.synchronize()
    rp, do_s = rep[idx], dout[idx]
    _gate_a('head_fwd.M256.out', hd['out'][idx], RE.head_fwd_ref64(rp, hw, hb), RE.head_fwd_bound(rp, hw, hb), rows, R * 4)
    dpre64 = RE.head_bwd_ref64(do_s, rp, hw)[0]
    _gate_a('head_bwd.M256.dpre.bf16', hd['dpre'][idx], dpre64, RE.head_dpre_bound(do_s, rp, hw, LE.R_BF16), rows, R * 2)
    _gate_a('head_bwd.M256.dpre.f32', hd['dpre32'][idx], dpre64, RE.head_dpre_bound(do_s, rp, hw, LE.R_F32), rows, R * 4)
    _gate_a('tanh_bwd.M256.bf16', hd['tanh_bwd'][idx], RE.tanh_bwd_ref64(drep[idx], rp), RE.tanh_bwd_bound(drep[idx], rp, LE.R_BF16), rows, R * 2)
    _gate_a('tanh_bwd.M256.f32', hd['tanh_bwd32'][idx], RE.tanh_bwd_ref64(drep[idx], rp), RE.tanh_bwd_bound(drep[idx], rp, LE.R_F32), rows, R * 4)
    del hd
    _, dw64, db64 = RE.head_bwd_ref64(dout, rep, hw)
    pw, pb = RE.head_bwd_param_bounds(dout, rep, M, R, D)
    _gate_a('head_bwd.M256.dw', hdw, dw64, pw, None, 0)
    _gate_a('head_bwd.M256.db', hdb[None], db64[None], pb[None] if pb.dim() == 1 else pb, None, 0)


def test_embed_forward(ops):
    """embed_fwd at 256 clips: h fp32 [M, 512] (the last 8,960 rows past 2^31), quarters_equal over clips, rowerr's bound on the slabs"""
    from tests import rowerr as RE
    B, T, C, Din = B256, T_FRAMES, 512, 3
    x = rnd(M256, Din, seed=1)
    w, b = rnd(C, Din, seed=2, scale=0.5), rnd(C, seed=3, scale=0.1)
    pos = rnd(1, J, C, seed=4, scale=0.1) + torch.arange(J, device=DEV).reshape(1, J, 1) * 0.25
    temp = rnd(1, T + 3, 1, C, seed=5, scale=0.1) - torch.arange(T + 3, device=DEV).reshape(1, T + 3, 1, 1) * 0.125
    h = dict(h=nan(M256, C, dtype=F32))
    _row_case('embed_fwd.B256', M256, lambda r0, r1: ops.embed_fwd(x[r0:r1], w, b, pos, temp, h['h'][r0:r1], (r1 - r0) // CLIP, T, J), h)
    rows = BE.slabs_of_interest(M256, [C * 4], unit=CLIP, sample=CLIP).rows()
    idx = torch.from_numpy(rows).to(DEV)
    n = len(rows) // CLIP
    ref = RE.embed_fwd_ref64(x[idx], w, b, pos, temp, n, T, J)
    _gate_a('embed_fwd.B256', h['h'][idx], ref, RE.embed_fwd_bound(x[idx], w, b, pos, temp, n, T, J), rows, C * 4)


def test_embed_backward(ops):
    """embed_bwd and embed_bwd_pair at 256 clips (dh fp32 [M, 512]; the pair two bf16 tensors): the tables' gradients are reductions over clips
    -- float64 over ALL rows with rowerr.embed_bwd_bounds for this batch; dx, a row output, over the whole tensor and by quarters"""
    from tests import rowerr as RE
    B, T, C, Din, M = B256, T_FRAMES, 512, 3, M256
    x, w = rnd(M, Din, seed=1), rnd(C, Din, seed=2, scale=0.5)
    dh_a, dh_b = rnd(M, C, seed=7, dtype=BF), rnd(M, C, seed=8, dtype=BF, scale=0.3)
    dh = dh_a.float() + dh_b.float()
    mk = lambda: dict(dw=nan(C, Din, dtype=F32), db=nan(C, dtype=F32), dpos=nan(1, J, C, dtype=F32), dtemp=nan(1, T + 3, 1, C, dtype=F32))
    got, pair = mk(), mk()
    dx = dict(dx=nan(M, Din, dtype=F32), dx_pair=nan(M, Din, dtype=F32))

    def launch(r0, r1):
        s, nb, full = slice(r0, r1), (r1 - r0) // CLIP, r1 - r0 == M
        g, q = (got, pair) if full else (mk(), mk())
        ops.embed_bwd(dh[s], x[s], w, g['dw'], g['db'], g['dpos'], g['dtemp'], dx['dx'][s], nb, T, J)
        ops.embed_bwd_pair(dh_a[s], dh_b[s], x[s], w, q['dw'], q['db'], q['dpos'], q['dtemp'], dx['dx_pair'][s], nb, T, J)
    _row_case('embed_bwd.B256', M, launch, dx)
    assert BE.first_difference(dx['dx_pair'], dx['dx']) is None
    for k in got:
        assert RE.same_bits(pair[k], got[k]), f'embed_bwd_pair: {k} differs from embed_bwd on the pair sum'
    assert float(got['dtemp'][0, T:].abs().max()) == 0.0
    ref, bnd = RE.embed_bwd_ref64(dh, x, w, B, T, J), RE.embed_bwd_bounds(dh, x, w, B, T, J)
    for k in ('dw', 'db', 'dpos'):
        _gate_a(f'embed_bwd.B256.{k}', got[k].reshape(ref[k].shape).reshape(-1, ref[k].shape[-1]), ref[k].reshape(-1, ref[k].shape[-1]),
                bnd[k].reshape(-1, ref[k].shape[-1]), None, 0)
    _gate_a('embed_bwd.B256.dtemp', got['dtemp'][0, :T, 0], ref['dtemp'], bnd['dtemp'], None, 0)
    _gate_a('embed_bwd.B256.dx', dx['dx'], ref['dx'], bnd['dx'], torch.arange(M).numpy(), Din * 4)


# ------------------------------------------------------------------------------------------------------------- 6. step kernels
ELEMS = 1 << 24      # elements of a float64 slab (tests/test_gpu_step_parity.py)
SEEDS = (0x1234567890ABCDEF, 0x0FEDCBA987654321)


def _away_from_zero(*shape, seed, dtype=F32):
    x = rnd(*shape, seed=seed)
    return (torch.where(x < 0, -1.0, 1.0) * (0.5 + x.abs())).to(dtype)


@pytest.mark.parametrize('dtype', [F32, BF], ids=['fp32', 'bf16'])
def test_dropout(ops, dtype):
    """dropout at n = M256 x 1024 elements (the MLP's hidden): the element index passes 2^30, the byte offset 2^31 (both types) and 2^32
    (fp32).  The mask is a hash of the element index, so a sub-launch cannot reproduce it: EVERY keep decision against dropmask.keep and
    every kept value within one rounding, slab by slab, as test_dropout of tests/test_gpu_step_parity.py"""
    from tests import steperr as SE
    n, (p, seed) = M256 * 1024, (0.1, SEEDS[0])
    x0 = _away_from_zero(n, seed=7, dtype=dtype)
    y = nan(n, dtype=dtype)
    ops.dropout(x0, y, p, seed)
    torch.cuda.synchronize()
    sc = SE.scale32(p)
    es = x0.element_size()
    kept, worst, bad = 0, dict(ratio=-1.0), 0
    for i0 in range(0, n, ELEMS):
        i1 = min(n, i0 + ELEMS)
        want = SE.keep_range(i0, i1, p, seed, DEV)
        nbad, first = SE.mask_mismatch(y[i0:i1] != 0, want)
        assert nbad == 0, (f'dropout: {nbad} keep decisions differ from dropmask.keep, the first at element {i0 + first} (byte offset {(i0 + first) * es:,}: '
                           f'{BE.side(i0 + first, es)})')
        kept += int(want.sum())
        ref = x0[i0:i1].double() * sc * want
        bound = (U * ref.abs()) if dtype == F32 else (LE.R_BF16 * ref.abs() + (1 + LE.R_BF16) * U * ref.abs())
        b = LE.bound_check(y[i0:i1].reshape(-1, 1), ref.reshape(-1, 1), bound.reshape(-1, 1))
        bad += b['violations']
        if b['ratio'] > worst['ratio']:
            worst = dict(b, row=b['row'] + i0)
    tag = f'dropout.{"bf16" if dtype == BF else "fp32"}.n{n}'
    note(tag, 'bound', worst['ratio'], 1.0, worst['row'], 0, BE.side(worst['row'], es), dict(violations=bad, kept_fraction=kept / n))
    assert bad == 0, f'{tag}: {bad} kept values outside one rounding, element {worst["row"]} ({BE.side(worst["row"], es)})'
    assert SE.kept_fraction_ok(kept, n, SE.f32(p))
    thrice(tag, lambda: ops.dropout(x0, y, p, seed), [y])


def test_residual_and_grad_drop(ops):
    """residual_drop and grad_drop (fp32 and bf16 output) at M256 rows x 1024: every keep decision (element mask on row * C + col, DropPath on
    row // 17) and every value, slab by slab, with the bounds of test_residual_and_grad_drop (tests/test_gpu_step_parity.py)"""
    from tests import steperr as SE
    rows_n, C, rps, (p, pp) = M256, 1024, J, (0.1, 0.2)
    seed, seed_path = SEEDS
    x = rnd(rows_n, C, seed=3)
    branch = _away_from_zero(rows_n, C, seed=4)
    y = x + branch
    y0 = y.clone()
    ops.residual_drop(y, x, rps, p, seed, pp, seed_path)
    d32, d16 = nan(rows_n, C, dtype=F32), nan(rows_n, C)
    ops.grad_drop(branch, d32, rps, p, seed, pp, seed_path)
    ops.grad_drop(branch, d16, rps, p, seed, pp, seed_path)
    torch.cuda.synchronize()
    mult = SE.branch_mult32(p, pp)
    worst = {k: dict(ratio=-1.0) for k in ('residual', 'grad32', 'grad16')}
    viol = dict.fromkeys(worst, 0)
    step = ELEMS // C
    for r0 in range(0, rows_n, step):
        r1 = min(rows_n, r0 + step)
        want = SE.branch_keep(r0, r1, C, rps, p, seed, pp, seed_path, DEV)
        fwd, b32, b16 = y[r0:r1] != x[r0:r1], d32[r0:r1] != 0, d16[r0:r1] != 0
        for nm, k in (('residual_drop', fwd), ('grad_drop fp32', b32), ('grad_drop bf16', b16)):
            nbad, first = SE.mask_mismatch(k, want)
            assert nbad == 0, (f'{nm}: {nbad} keep decisions differ from dropmask.keep, the first at row {r0 + first // C}, col {first % C} '
                               f'({BE.side(r0 + first // C, C * 4)} of the fp32 rows)')
        xd, dd = x[r0:r1].double(), y0[r0:r1].double() - x[r0:r1].double()
        ref = xd + dd * mult * want
        bound = (U * dd.abs() * mult * want + U * ref.abs()) * (1 + U)
        gref = branch[r0:r1].double() * mult * want
        for nm, got, rf, bd in (('residual', y[r0:r1], ref, bound), ('grad32', d32[r0:r1], gref, U * gref.abs()),
                                ('grad16', d16[r0:r1], gref, LE.R_BF16 * gref.abs() + (1 + LE.R_BF16) * U * gref.abs())):
            b = LE.bound_check(got, rf, bd)
            viol[nm] += b['violations']
            if b['ratio'] > worst[nm]['ratio']:
                worst[nm] = dict(b, row=b['row'] + r0)
    for nm in worst:
        rb = C * (2 if nm == 'grad16' else 4)
        note(f'{nm}_drop.rows{rows_n}.C{C}', 'bound', worst[nm]['ratio'], 1.0, worst[nm]['row'], worst[nm]['col'], BE.side(worst[nm]['row'], rb), dict(violations=viol[nm]))
        assert viol[nm] == 0, f'{nm}: {viol[nm]} values outside their bound, the worst at row {worst[nm]["row"]}, col {worst[nm]["col"]} ({BE.side(worst[nm]["row"], rb)})'


def test_pool_kernels(ops):
    """pool_rep_fwd and tanh_pool_bwd over the 256 clips as 128 samples of two persons (rep fp32 [M256, 512]: the last 8,960 rows past 2^31):
    every element of both, the mask of both passes against dropmask.keep, with the bounds of test_pool_kernels (tests/test_gpu_step_parity.py)"""
    from tests import steperr as SE
    N, Mp, T, R, (p, seed) = B256 // 2, 2, T_FRAMES, 512, (0.1, SEEDS[1])
    ntok, K = N * Mp * T * J, Mp * T
    assert ntok == M256
    rep = torch.tanh(rnd(ntok, R, seed=1))
    dpool = rnd(N, J, R, seed=2)
    pooled, d32, d16 = nan(N, J, R, dtype=F32), nan(ntok, R, dtype=F32), nan(ntok, R)
    ops.pool_rep_fwd(rep, pooled, N, Mp, T, J, p, seed)
    ops.tanh_pool_bwd(dpool, rep, d32, N, Mp, T, J, p, seed)
    ops.tanh_pool_bwd(dpool, rep, d16, N, Mp, T, J, p, seed)
    # with rep = 0 and dpooled = 1 the backward writes keep x s per element: the mask itself
    back = nan(ntok, R, dtype=F32)
    ops.tanh_pool_bwd(torch.ones(N, J, R, device=DEV), torch.zeros(ntok, R, device=DEV), back, N, Mp, T, J, p, seed)
    torch.cuda.synchronize()
    s64 = 1.0 / (1.0 - SE.f32(p)) / K
    per = Mp * T * J * R
    nstep = max(1, ELEMS // per)
    for n0 in range(0, N, nstep):
        n1 = min(N, n0 + nstep)
        sl = slice(n0 * K * J, n1 * K * J)
        rows = torch.arange(n0 * K * J, n1 * K * J).numpy()
        keep = SE.keep_range(n0 * per, n1 * per, p, seed, DEV).reshape(n1 - n0, K, J, R).double()
        r5 = rep[sl].double().reshape(n1 - n0, K, J, R)
        x, amp = (r5 * keep).sum(1) * s64, (r5.abs() * keep).sum(1) * s64
        _gate_a(f'pool_rep_fwd.B256.n{n0}', pooled[n0:n1].reshape(-1, R), x.reshape(-1, R), ((4 * U * x.abs() + K * U * amp) * (1 + U)).reshape(-1, R), None, 0)
        assert torch.equal(back[sl].reshape(n1 - n0, K, J, R) != 0, keep != 0), \
            f'tanh_pool_bwd: the mask differs from dropmask.keep in samples {n0}:{n1} ({BE.side(n0 * K * J, R * 4)})'
        dd = dpool[n0:n1].double()[:, None] * s64 * keep
        xb = dd * (1.0 - r5 * r5)
        bb = (5 * U * xb.abs() + 2 * U * dd.abs()) * (1 + U)
        _gate_a(f'tanh_pool_bwd.fp32.B256.n{n0}', d32[sl], xb.reshape(-1, R), bb.reshape(-1, R), rows, R * 4)
        _gate_a(f'tanh_pool_bwd.bf16.B256.n{n0}', d16[sl], xb.reshape(-1, R), (LE.R_BF16 * xb.abs() + (1 + LE.R_BF16) * bb).reshape(-1, R), rows, R * 2)
    thrice('pool.B256', lambda: (ops.pool_rep_fwd(rep, pooled, N, Mp, T, J, p, seed), ops.tanh_pool_bwd(dpool, rep, d32, N, Mp, T, J, p, seed)), [pooled, d32])
