"""The local-error checker (tests/localerr.py) is tested before it is trusted -- on the CPU, with the torch restatement of the kernel
set (MockOps: bf16 operands, fp32 product, output rounded as the kernel's is) standing in for the kernel:

  * the clean output passes every new gate (the elementwise bound of a once-rounded output; 2 x the rounding model's worst unit for
    outputs that are rounded inside the kernel) -- the proof that the reference alone stays inside the gates;
  * seeded corruptions with small support fail them, and the result names the corrupted unit;
  * for each corruption the existing global relative L2 is evaluated too, scaled by sqrt(elements) to the family's largest GPU shape
    and recorded in GLOBAL_VIEW; where it stays under today's global gate the test asserts that it does -- that is the gap the
    per-unit gates close, kept visible.

No corruption here touches a kernel: every one is applied to a tensor on the CPU."""
import math

import pytest
import torch

from motionbert_amd.engine import EPI_GELU, EPI_STORE, MODE_SPATIAL, MODE_TEMPORAL
from tests import localerr as LE
from tests.mock_ops import MockOps

BF = torch.bfloat16
GLOBAL_VIEW = {}          # corruption -> dict(rel here, rel scaled to the largest GPU shape, today's gate)


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def record_global(name, clean, bad, ref64, n_large, gate, expect_under):
    """global rel-L2 of the corrupted output, the defect's part of it scaled to n_large elements and recombined with the clean level"""
    e_clean, e_bad = LE.rel(clean, ref64), LE.rel(bad.nan_to_num(nan=0.0), ref64)
    defect = math.sqrt(max(e_bad ** 2 - e_clean ** 2, 0.0))
    at_large = math.sqrt(e_clean ** 2 + LE.scaled_global(defect, ref64.numel(), n_large) ** 2)
    GLOBAL_VIEW[name] = dict(clean=e_clean, corrupt=e_bad, at_largest_gpu_shape=at_large, gate=gate)
    print(f'{name}: global rel-l2 clean {e_clean:.2e}, corrupt {e_bad:.2e}, at the largest GPU shape {at_large:.2e} (gate {gate:.1e})')
    if expect_under:
        assert at_large < gate, f'{name}: the global gate would have seen it ({at_large:.2e} >= {gate:.1e}); update the record'


# ---------------------------------------------------------------------------------------------- unit_errors / locate themselves
def test_unit_errors_finds_the_unit_and_keeps_ragged_blocks():
    ref = rnd(70, 100, seed=1).double() + 3.0
    got = ref.clone()
    got[69, 96:] += 1.0                       # inside the ragged corner block of a 32 x 32 grid
    u = LE.unit_errors(got, ref, 32, 32)
    assert u['unit'] == (2, 3) and (u['row'], u['col']) == (64, 96) and u['n_units'] == 3 * 4 and u['worst'] > 0
    assert LE.unit_errors(ref.clone(), ref, 1, 8)['worst'] == 0.0
    got = ref.clone()
    got[5, 8:16] = float('nan')
    u = LE.unit_errors(got, ref, *LE.unit_shape('frag', 100))
    assert u['worst'] == float('inf') and (u['row'], u['col']) == (5, 8)


def test_unit_errors_floor_exempts_near_zero_units_and_reports_the_share():
    ref = rnd(400, 64, seed=2).double()
    ref[7] *= 1e-9                            # a row whose exact value is (nearly) zero
    got = ref + 1e-6
    u = LE.unit_errors(got, ref, 1, 64)
    assert u['worst'] < 1e-4 and abs(u['exempt'] - 1 / 400) < 1e-12      # judged against 5 % of the RMS row norm, and counted
    u0 = LE.unit_errors(got, ref, 1, 64, floor_frac=0.0)
    assert u0['row'] == 7 and u0['worst'] > 1.0


def test_locate_reads_the_geometry_of_the_kernel_sources():
    p = LE.locate(300, 700, 'pp256')          # 256 x 256 workgroup tile, waves of 128 x 64
    assert p['wg'] == (1, 2) and p['wave'] == (0, 2 * 64 // 64 + (700 % 256 - 128) // 64) and p['mfma_tile'] == (9, 21)
    p = LE.locate(300, 200, 'pipe')           # 256 x 128, waves of 64 x 64
    assert p['wg'] == (1, 1) and p['wave'] == (0, 1)
    p = LE.locate(1000, 5, 'rows_n')          # 128 complete rows per workgroup, 32 per wave
    assert p['wg'] == (7, 0) and p['wave'] == (3, 0) and p['row_in_wave'] == 1000 % 32
    p = LE.locate(321, 0, 'attn_stream')      # 256-row block, 32-row wave block, 64-row stream tile
    assert p['wg'] == (1, 0) and p['wave'] == (2, 0) and p['stream_tile'] == 5
    assert LE.locate(243 - 1, 0, 'attn')['wave'] == (7, 0)
    # the constants are the sources' own
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'motionbert_amd', 'csrc')
    src = lambda f: open(os.path.join(csrc, f)).read()
    assert int(re.search(r'R_BM = (\d+)', src('gemm_rows.hip')).group(1)) == LE.GEOMETRY['rows_nk']['wg'][0]
    assert int(re.search(r'RN_BM = (\d+)', src('gemm_rows_n.hip')).group(1)) == LE.GEOMETRY['rows_n']['wg'][0]
    assert int(re.search(r'F_BM = (\d+)', src('mlp_fused.hip')).group(1)) == LE.GEOMETRY['mlp']['wg'][0]
    assert int(re.search(r'MBX_STREAM_TILE = (\d+)', src('attention_stream.hip')).group(1)) == LE.GEOMETRY['attn_stream']['stream_tile']
    assert 'MBX_STREAM_BLOCK = 32 * MBX_STREAM_THREADS / 64' in src('attention_stream.hip')


# ---------------------------------------------------------------------------------------------- one final rounding: the GEMMs
M_G, N_G, K_G = 1031, 512, 512            # ragged in rows of every geometry (1031 = 4 * 256 + 7)
N_LARGE_TILE = 70227 * 1536               # the largest shape of the tile GEMM tests today
N_LARGE_ROWS = 264384 * 512               # ... of the N-resident row owners (and of every family after this change)


def _gemm_case(epi=EPI_STORE):
    a = (rnd(M_G, K_G, seed=1) * (0.5 + rnd(M_G, 1, seed=2).abs()) + 0.3 * rnd(M_G, 1, seed=3)).to(BF)      # per-row scale and offset
    w, bias = rnd(N_G, K_G, seed=4, dtype=BF, scale=0.05), rnd(N_G, seed=5, scale=0.5)
    out, out2 = torch.empty(M_G, N_G, dtype=BF), torch.empty(M_G, N_G, dtype=BF)
    MockOps().gemm_nt(a, w, bias, epi, out_t=out, out2_t=out2 if epi == EPI_GELU else None)
    u = a.double() @ w.double().t() + bias.double()
    amp = a.double().abs() @ w.double().abs().t()
    return a, w, bias, (out2 if epi == EPI_GELU else out), u, amp


def _store_bound(u, amp, bias):
    # STORE: x = acc + bias, one fp32 add after the accumulation (ops = 1), Lipschitz constant 1, bf16 output
    return LE.elementwise_bound(u, amp, K_G, LE.R_BF16, lip=1.0, ops=1, mag64=amp + bias.double().abs())


def test_clean_gemm_outputs_pass_the_elementwise_bound():
    a, w, bias, out, u, amp = _gemm_case()
    b = LE.bound_check(out, u, _store_bound(u, amp, bias))
    assert b['violations'] == 0 and b['ratio'] <= 1.0, b
    # GELU: Lipschitz constant sup |gelu'| = 1.129 at u = sqrt 2, the absolute error gelu_fast.h states for its erf forms, one add (bias)
    a, w, bias, g, u, amp = _gemm_case(EPI_GELU)
    bound = LE.elementwise_bound(LE.gelu64(u), amp, K_G, LE.R_BF16, lip=LE.GELU_LIP, ops=1, eabs=LE.gelu_eabs(u), mag64=amp + bias.double().abs())
    b = LE.bound_check(g, LE.gelu64(u), bound)
    assert b['violations'] == 0, b
    # the units the GPU module reports stay at the bf16 level on a clean output, and nothing sits on the floor
    for unit in ('row', 'tile', 'frag'):
        r = LE.unit_errors(out, u, *LE.unit_shape(unit, N_G))
        assert r['worst'] < 2 * LE.R_BF16 and r['exempt'] <= LE.MAX_EXEMPT, (unit, r)      # no unit can exceed the elementwise r (+ the fp32 term)


def _corruptions(a, w, bias, out):
    """name -> (corrupted output, the unit that must be named as (row, col) of a (rows x cols) grid, grid)"""
    c = {}
    bad = out.clone()
    bad[517] = out[516]
    c['row_from_neighbour'] = (bad, (517, 0), (1, N_G))
    bad = out.clone()
    bad[700, 264:272] = 0
    c['fragment_zeroed'] = (bad, (700, 264), (1, 8))
    # one 32 x 32 tile computed with one k-step (BK = 32) of stale operand: the a fragment of the PREVIOUS 256-row block
    r0, c0, k0 = 32 * 20, 32 * 9, LE.BK * 5
    a2 = a[r0:r0 + 32].float().clone()
    a2[:, k0:k0 + LE.BK] = a[r0 - 256:r0 - 224, k0:k0 + LE.BK].float()
    bad = out.clone()
    bad[r0:r0 + 32, c0:c0 + 32] = (a2 @ w[c0:c0 + 32].float().t() + bias[c0:c0 + 32]).to(BF)
    c['tile_one_stale_kstep'] = (bad, (r0, c0), (32, 32))
    bad = out.clone()
    bad[M_G - 1] = float('nan')
    c['ragged_tail_row_left_at_sentinel'] = (bad, (M_G - 1, 0), (1, N_G))
    return c


@pytest.mark.parametrize('name', ['row_from_neighbour', 'fragment_zeroed', 'tile_one_stale_kstep', 'ragged_tail_row_left_at_sentinel'])
def test_corrupted_gemm_output_fails_and_the_unit_is_named(name):
    a, w, bias, out, u, amp = _gemm_case()
    bad, (row, col), (ur, uc) = _corruptions(a, w, bias, out)[name]
    b = LE.bound_check(bad, u, _store_bound(u, amp, bias))
    assert b['violations'] > 0 and b['ratio'] > 1.0, f'{name}: the elementwise bound let it through'
    assert row <= b['row'] < row + ur and col <= b['col'] < col + uc, (name, b)
    r = LE.unit_errors(bad, u, ur, uc)
    assert (r['row'], r['col']) == (row, col), (name, r)
    clean_worst = LE.unit_errors(out, u, ur, uc)['worst']
    assert r['worst'] > 10 * clean_worst, (name, r['worst'], clean_worst)
    msg = LE.where(r, 'pp256')
    assert f"'mfma_tile': ({row // 32}, {col // 32})" in msg and f"'wg': ({row // 256}, {col // 256})" in msg, msg
    # what the global norm makes of it at the largest shape the tile GEMMs are tested at today (gate 4e-3); a non-finite row is seen by
    # check()'s isfinite assertion, so it is recorded with the row zeroed and not asserted
    record_global(f'gemm.{name}', out, bad, u, N_LARGE_TILE, 4e-3, expect_under=name in ('fragment_zeroed', 'tile_one_stale_kstep', 'row_from_neighbour'))


# ---------------------------------------------------------------------------------------------- rounded inside the kernel: attention
ATT_CPU = [(MODE_TEMPORAL, 1, 243, 3, 2, 64), (MODE_TEMPORAL, 2, 40, 2, 2, 32), (MODE_SPATIAL, 3, 5, 17, 2, 64)]
N_LARGE_ATT = 243 * 17 * 8                # (row, head) outputs of the existing B = 1, T = 243 case


def _attn_case(mode, B, T, J, H, hd, seed=1):
    C, M = H * hd, B * T * J
    qkv = rnd(M, 3 * C, seed=seed)
    qkv[:, :C] *= 1.0 + 0.5 * rnd(M, 1, seed=seed + 1).abs().clamp_max(2.0)      # per-row scale on q in [1, 2]: row maxima, lse and delta differ from row to row,
    # and no softmax saturates (a one-hot row has dS = 0: its dq would sit on the floor of unit_errors)
    return qkv.to(BF), rnd(M, C, seed=seed + 2, dtype=BF), C, M


def _attn_units(got, exact, H, hd, T_or_J):
    C = exact.shape[1]
    return {'row': LE.unit_errors(got, exact, 1, C), 'row_head': LE.unit_errors(got, exact, 1, hd)}


@pytest.mark.parametrize('mode,B,T,J,H,hd', ATT_CPU)
def test_clean_attention_passes_twice_the_rounding_model(mode, B, T, J, H, hd):
    """forward o and backward dq / dk / dv of the restatement (fp32, P not rounded, output rounded once) against the exact float64
    result: every worst unit within 2 x the rounding model's own worst unit; lse within its derived bound; exempt share within 0.1 %."""
    qkv, do, C, M = _attn_case(mode, B, T, J, H, hd)
    tm = mode == MODE_TEMPORAL
    scale = hd ** -0.5
    o, lse = torch.empty(M, C, dtype=BF), torch.empty(M, H)
    MockOps().attn_fwd(qkv, o, lse, B, T, J, H, scale, mode)
    ex_o, ex_l = LE.attn_fwd_ref(qkv, B, T, J, H, scale, tm, model=False)
    md_o, _ = LE.attn_fwd_ref(qkv, B, T, J, H, scale, tm, model=True)
    for unit, (ur, uc) in {'row': (1, C), 'row_head': (1, hd)}.items():
        g, m = LE.unit_errors(o, ex_o, ur, uc), LE.unit_errors(md_o, ex_o, ur, uc)
        assert g['worst'] <= 2 * m['worst'] and m['exempt'] <= LE.MAX_EXEMPT, (unit, g, m)
        assert m['worst'] < 1.6 * m['mean'] + 1e-3, ('the model worst unit sits near its own mean', unit, m)
    # lse: fp32 log-sum-exp of scores that carry K 2^-24 of their amplitude: |s| <= scale |q| |k|; abs 1e-5 covers hd <= 64 at these magnitudes
    assert LE.row_abs_rel_check(lse, ex_l, 2e-5, 2 * LE.U32)['ratio'] <= 1.0
    dq = torch.empty(M, 3 * C, dtype=BF)
    MockOps().attn_bwd(qkv, o, do, lse, dq, B, T, J, H, scale, mode)
    ex_d = LE.attn_bwd_ref(qkv, ex_o, do, ex_l, B, T, J, H, scale, tm, model=False)
    md_d = LE.attn_bwd_ref(qkv, LE.bf16_round(ex_o), do, ex_l, B, T, J, H, scale, tm, model=True)
    for i, n in enumerate(('dq', 'dk', 'dv')):
        sl = slice(i * C, (i + 1) * C)
        for unit, (ur, uc) in {'row': (1, C), 'row_head': (1, hd)}.items():
            g, m = LE.unit_errors(dq[:, sl], ex_d[:, sl], ur, uc), LE.unit_errors(md_d[:, sl], ex_d[:, sl], ur, uc)
            assert g['worst'] <= 2 * m['worst'] and m['exempt'] <= LE.MAX_EXEMPT, (n, unit, g, m)


def test_corrupted_attention_fails_and_the_unit_is_named():
    mode, B, T, J, H, hd = ATT_CPU[0]
    qkv, do, C, M = _attn_case(mode, B, T, J, H, hd)
    scale = hd ** -0.5
    o, lse = torch.empty(M, C, dtype=BF), torch.empty(M, H)
    MockOps().attn_fwd(qkv, o, lse, B, T, J, H, scale, mode)
    ex_o, ex_l = LE.attn_fwd_ref(qkv, B, T, J, H, scale, True, model=False)
    md_o, _ = LE.attn_fwd_ref(qkv, B, T, J, H, scale, True, model=True)
    gate = {u: 2 * LE.unit_errors(md_o, ex_o, *s)['worst'] for u, s in {'row_head': (1, hd), 'row': (1, C), 'wave_rows': (32, C)}.items()}
    # (a) one (row, head) takes the neighbouring head's value
    bad = o.clone()
    bad[300, hd:2 * hd] = o[300, 0:hd]
    r = LE.unit_errors(bad, ex_o, 1, hd)
    assert r['worst'] > gate['row_head'] and (r['row'], r['col']) == (300, hd), r
    assert LE.unit_errors(o, ex_o, 1, hd)['worst'] <= gate['row_head']
    record_global('attn.row_head_from_neighbour_head', o, bad, ex_o, N_LARGE_ATT * hd, 1.5e-2, expect_under=True)
    # (b) one key tile of 64 left out of one query block's softmax: problem (b 0, joint 1, head 1), queries 96 .. 127, keys 128 .. 191
    sk_o, sk_l = LE.attn_fwd_ref(qkv, B, T, J, H, scale, True, model=True, skip=((0, 1, 1), (96, 128), (128, 192)))
    r = LE.unit_errors(sk_o, ex_o, 1, hd)
    tok = lambda t: t * J + 1                  # token row of frame t, joint 1
    assert r['worst'] > gate['row_head'] and r['col'] == hd and r['row'] in [tok(t) for t in range(96, 128)], r
    assert LE.locate((r['row'] - 1) // J, r['col'], 'attn')['wave'] == (3, 0)      # the message names query block 3
    record_global('attn.key_tile_skipped', md_o, sk_o, ex_o, N_LARGE_ATT * hd, 1.5e-2, expect_under=True)
    # (c) one row's lse taken from the row above
    bad_l = lse.clone()
    bad_l[tok(50)] = lse[tok(50) - 1]
    b = LE.row_abs_rel_check(bad_l, ex_l, 2e-5, 2 * LE.U32)
    assert b['ratio'] > 1.0 and b['row'] == tok(50), b
    e_l = LE.rel(bad_l, ex_l)
    GLOBAL_VIEW['attn.lse_row_from_row_above'] = dict(corrupt=e_l, at_largest_gpu_shape=LE.scaled_global(e_l, ex_l.numel(), N_LARGE_ATT), gate=1e-4)
    # (d) one row's delta taken from the row above: dq of that row is wrong
    ex_d = LE.attn_bwd_ref(qkv, ex_o, do, ex_l, B, T, J, H, scale, True, model=False)
    ob = LE.bf16_round(ex_o)
    md_d = LE.attn_bwd_ref(qkv, ob, do, ex_l, B, T, J, H, scale, True, model=True)
    bad_d = LE.attn_bwd_ref(qkv, ob, do, ex_l, B, T, J, H, scale, True, model=True, delta_rows=(tok(60) - 1, tok(60)))
    g, m = LE.unit_errors(bad_d[:, :C], ex_d[:, :C], 1, C), LE.unit_errors(md_d[:, :C], ex_d[:, :C], 1, C)
    assert g['worst'] > 2 * m['worst'] and g['row'] == tok(60), (g, m)
    record_global('attn.delta_row_from_row_above', md_d[:, :C], bad_d[:, :C], ex_d[:, :C], N_LARGE_ATT * hd, 2e-2, expect_under=True)
    # (e) the last row of the sequence left at the sentinel
    bad = o.clone()
    bad[M - 1] = 9.0
    r = LE.unit_errors(bad, ex_o, 1, C)
    assert r['row'] == M - 1 and r['worst'] > gate['row'], r


# ---------------------------------------------------------------------------------------------- rounded inside the kernel: the fused MLP
def test_fused_mlp_model_and_a_swapped_row():
    M, C, HID = 300, 256, 512
    a = (rnd(M, C, seed=1) * (0.5 + rnd(M, 1, seed=2).abs())).to(BF)
    w1, w2 = rnd(HID, C, seed=3, dtype=BF, scale=0.08), rnd(C, HID, seed=4, dtype=BF, scale=0.05)
    b1, b2 = rnd(HID, seed=5, scale=0.3), rnd(C, seed=6, scale=0.3)
    resid = rnd(M, C, seed=7) * (0.5 + rnd(M, 1, seed=8).abs())
    y = torch.empty(M, C)
    MockOps().mlp_fused_fwd(a, False, (w1, w2), b1, b2, None, resid, y, None, 1e-6, None, None)
    exact, model = LE.mlp_ref(a, w1, b1, w2, b2, resid, False), LE.mlp_ref(a, w1, b1, w2, b2, resid, True)
    # judged on the branch y - resid: the residual carries no error and would only dilute the units
    br = lambda t: t.double() - resid.double()
    for ur, uc in ((1, C), (32, 32), (32, C)):
        g, m = LE.unit_errors(br(y), br(exact), ur, uc), LE.unit_errors(br(model), br(exact), ur, uc)
        assert g['worst'] <= 2 * m['worst'] and m['exempt'] <= LE.MAX_EXEMPT, (ur, uc, g, m)
    bad = y.clone()
    bad[129] = y[128]
    g, m = LE.unit_errors(br(bad), br(exact), 1, C), LE.unit_errors(br(model), br(exact), 1, C)
    assert g['worst'] > 2 * m['worst'] and g['row'] == 129, (g, m)
    assert LE.locate(g['row'], 0, 'mlp')['wg'] == (1, 0) and LE.locate(g['row'], 0, 'mlp')['row_in_wave'] == 1
    record_global('mlp.row_from_neighbour', br(y), br(bad), br(exact), 264384 * C, 4e-3, expect_under=True)


def test_the_inputs_of_the_gpu_module_keep_the_reference_off_the_floor():
    """The per-row scale and offset of the GPU module's operands (test_gpu_local_parity._gemm_operands) leave no row, tile or fragment
    of the reference on the floor of unit_errors beyond 0.1 % -- checked here at a CPU size with the same construction."""
    from tests.test_gpu_local_parity import gemm_operands
    a, w, bias = gemm_operands(4131, 512, 512, seed=3, device='cpu')
    u = a.double() @ w.double().t() + bias.double()
    for unit in ('row', 'tile', 'frag'):
        assert LE.unit_errors(u.float(), u, *LE.unit_shape(unit, 512))['exempt'] <= LE.MAX_EXEMPT, unit


@pytest.mark.parametrize('hd', [64, 32])
@pytest.mark.parametrize('T', [31, 32, 33])
def test_the_attention_edge_inputs_keep_the_reference_off_the_floor(T, hd):
    """The short-sequence edge cases of the GPU module have few units (2 x 17 problems): their seeded inputs leave no (row, head) and no
    (wave block, head) unit of the exact o / dq / dk / dv on the floor -- a property of the reference alone."""
    from tests.test_gpu_local_parity import J, _attn_inputs, wave_lines
    B, H = 2, 4
    qkv, do, C, M = _attn_inputs(B, T, H, hd, seed=T, device='cpu')
    scale = hd ** -0.5
    ex_o, ex_l = LE.attn_fwd_ref(qkv, B, T, J, H, scale, True, model=False)
    ex_d = LE.attn_bwd_ref(qkv, ex_o, do, ex_l, B, T, J, H, scale, True, model=False)
    for t in (ex_o, ex_d[:, :C], ex_d[:, C:2 * C], ex_d[:, 2 * C:]):
        assert LE.unit_errors(t, t, 1, hd)['exempt'] <= LE.MAX_EXEMPT
        lines = wave_lines(t, B, T, H, hd, True)
        assert LE.unit_errors(lines, lines, 1, 32 * hd, valid=wave_lines(torch.ones_like(t), B, T, H, hd, True))['exempt'] <= LE.MAX_EXEMPT


# ---------------------------------------------------------------------------------------------- once-rounded fp32 output: the weight gradient
def test_weight_gradient_bound_sees_a_fragment_and_a_tile_at_the_training_step():
    """dW at M = 264,384 tokens (N = K = 64 keeps it affordable): a stand-in with the kernel's structure (64 token splits accumulated in fp32,
    partials summed in fp32) passes localerr.split_sum_bound; a zeroed 16-byte fragment (four fp32 values) and a 32 x 32 tile taken from
    the neighbouring tile fail it and are named.  (A bound over the whole contraction, M 2^-24 amp, exceeds |dW| itself and sees neither.)"""
    M, N, K, splits = 264384, 64, 64, 64
    from tests.test_gpu_local_parity import rows_scaled
    dy, a = rows_scaled(M, N, seed=1, device='cpu').to(BF), rows_scaled(M, K, seed=2, device='cpu').to(BF)
    x = dy.double().t() @ a.double()
    amp = dy.double().abs().t() @ a.double().abs()
    per = -(-M // splits)
    dw = torch.stack([dy[i:i + per].float().t() @ a[i:i + per].float() for i in range(0, M, per)]).sum(0)
    bound = LE.split_sum_bound(x, amp, M, splits)
    assert LE.bound_check(dw, x, bound)['violations'] == 0
    assert float((bound / x.abs()).median()) < 0.2, 'the bound must be well below the values it guards'
    bad = dw.clone()
    bad[40, 8:12] = 0
    b = LE.bound_check(bad, x, bound)
    assert b['violations'] > 0 and b['row'] == 40 and 8 <= b['col'] < 12, b
    bad = dw.clone()
    bad[32:, :32] = dw[32:, 32:]
    b = LE.bound_check(bad, x, bound)
    assert b['violations'] > 900 and b['row'] >= 32 and b['col'] < 32, b
    u = LE.unit_errors(bad, x, 32, 32)
    assert (u['row'], u['col']) == (32, 0) and LE.locate(u['row'], u['col'], 'tn')['mfma_tile'] == (1, 0)
    loose = LE.elementwise_bound(x, amp, M, LE.R_F32, ops=0)
    assert LE.bound_check(bad, x, loose)['violations'] < 16      # the whole-contraction bound: kept visible


def test_small_backward_model_and_the_per_unit_gate():
    """L <= 32 (every spatial problem): the model of attn_bwd_small_kernel (delta from the unrounded P.dP, dS rounded with the scale); the
    clean restatement passes the per-unit gate at (row, head) and (wave block, head); one (row, head) of dq taking the neighbouring
    head's value fails it and is named, whatever the model's own worst unit is; a wrong row dot of attn_bwd_stats is named by its bound."""
    from tests.test_gpu_local_parity import wave_lines
    mode, B, T, J, H, hd = MODE_SPATIAL, 3, 5, 17, 2, 64
    qkv, do, C, M = _attn_case(mode, B, T, J, H, hd)
    scale = hd ** -0.5
    o, lse = torch.empty(M, C, dtype=BF), torch.empty(M, H)
    MockOps().attn_fwd(qkv, o, lse, B, T, J, H, scale, mode)
    ex_o, ex_l = LE.attn_fwd_ref(qkv, B, T, J, H, scale, False, model=False)
    dq = torch.empty(M, 3 * C, dtype=BF)
    # the stand-in for this kernel takes delta from the UNROUNDED output, as rowsum(P o dP) is (the restatement computes dO . o)
    MockOps().attn_bwd(qkv, ex_o.float(), do, lse, dq, B, T, J, H, scale, mode)
    ex_d = LE.attn_bwd_ref(qkv, ex_o, do, ex_l, B, T, J, H, scale, False, model=False)
    md_d = LE.attn_bwd_ref(qkv, LE.bf16_round(ex_o), do, ex_l, B, T, J, H, scale, False, model=True, variant='small')
    old = LE.attn_bwd_ref(qkv, LE.bf16_round(ex_o), do, ex_l, B, T, J, H, scale, False, model=True, variant='fused')
    e = ex_d[:, :C]
    m = LE.unit_errors(md_d[:, :C], e, 1, hd, full=True)
    assert m['worst'] < LE.unit_errors(old[:, :C], e, 1, hd)['worst']      # the model of the other kernel carries a rounding this one lacks
    g = LE.unit_errors(dq[:, :C], e, 1, hd, full=True)
    assert LE.per_unit_excess(g, m, 1, hd)['excess'] <= 1.0
    bad = dq[:, :C].clone()
    bad[100, hd:] = dq[100, :hd]
    x = LE.per_unit_excess(LE.unit_errors(bad, e, 1, hd, full=True), m, 1, hd)
    assert x['excess'] > 10 and (x['row'], x['col']) == (100, hd) and x['n_over'] == 1, x
    ok = wave_lines(torch.ones_like(e), B, T, H, hd, False)
    wl = lambda t: wave_lines(t.double(), B, T, H, hd, False)
    mw = LE.unit_errors(wl(md_d[:, :C]), wl(e), 1, 32 * hd, valid=ok, full=True)
    assert LE.per_unit_excess(LE.unit_errors(wl(dq[:, :C]), wl(e), 1, 32 * hd, valid=ok, full=True), mw, 1, 32 * hd)['excess'] <= 1.0
    x = LE.per_unit_excess(LE.unit_errors(wl(bad), wl(e), 1, 32 * hd, valid=ok, full=True), mw, 1, 32 * hd)
    assert x['excess'] > 1.0 and x['row'] == 100 // J and x['col'] == 32 * hd, x      # problem 100 // 17 (its only wave block), head 1
    bias_f, rsum = rnd(3 * C, seed=8, scale=0.3), rnd(3 * C, seed=9)
    part = torch.empty(2 * H, M, 2)
    MockOps().attn_bwd_stats(qkv, o, do, lse, dq, bias_f, rsum, part, B, T, J, H, scale, mode)
    own, amp = LE.attn_stats_ref(dq, qkv, bias_f, rsum, H)
    tol = 2 * (2 * hd) * LE.U32 * amp.reshape(2 * H * M, 2)
    assert LE.row_abs_rel_check(part.reshape(2 * H * M, 2), own.reshape(2 * H * M, 2), tol, LE.U32)['ratio'] <= 1.0
    part[3, 77] = part[3, 76]
    b = LE.row_abs_rel_check(part.reshape(2 * H * M, 2), own.reshape(2 * H * M, 2), tol, LE.U32)
    assert b['ratio'] > 1.0 and b['row'] == 3 * M + 77, b
