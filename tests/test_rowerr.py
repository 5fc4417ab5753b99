"""The gates of tests/test_gpu_row_parity.py are shown to bite before they are trusted -- on the CPU, with the torch restatements of
tests/rowerr.py standing in for the kernels of csrc/elementwise.hip.  The uncorrupted restatement passes each gate; each of these fails it:

  1. LayerNorm, second row of a wave: rows [4096, M) of y left at their sentinel; the same rows computed with the mean / rstd of row - 4096
  2. dgamma / dbeta missing one row of 12,291
  3. embed_fwd: the first row after a clip wrap takes temp[t_prev + 1] instead of temp[0]
  4. embed_bwd: one LDS slice's clips dropped from dpos, dw and db
  5. fusion dw / db: one block's partial row dropped
  6. a bf16 copy rounded toward zero instead of to nearest even
  7. alpha swapped on one row

Every corruption is applied to a restatement's output, never to a kernel.  Each test prints the whole-tensor relative L2 the corruption
produces next to the tolerance tests/test_gpu_kernels.py holds that output to (pytest -s shows the lines)."""
import torch

from tests import localerr as LE
from tests import rowerr as RE

EPS = RE.f32(1e-6)


def _bound_ok(got, x64, bound):
    return LE.bound_check(got.reshape(-1, 1), x64.reshape(-1, 1), bound.reshape(-1, 1))


# ---------------------------------------------------------------------------------------------- 1. LayerNorm second row
def test_layernorm_second_row_unwritten_or_with_stale_statistics_fails():
    M, C = 4131, 64
    for offset in (0.0, 40.0):
        x, g, b = RE.ln_inputs(M, C, seed=1, device='cpu', offset=offset)
        ref, mu64, rs64 = RE.ln_fwd_ref64(x, g, b, EPS)
        for dt in (torch.float32, torch.bfloat16):
            y, mu, rs = RE.ln_fwd_model(x, g, b, EPS, dt)
            gu, mu_, px, ok, msg = RE.gate_rows(y, ref, y)
            assert ok and mu_['exempt'] == 0, msg
            assert RE.gate_rows(ref.float().to(dt), ref, y)[3]          # the float64 result rounded once passes too
            bm, br = RE.ln_stat_bounds(x, EPS)
            assert _bound_ok(mu, mu64, bm)['violations'] == 0 and _bound_ok(rs, rs64, br)['violations'] == 0
            # (a) the second row of every wave never written
            left = y.clone()
            left[4096:] = float('nan')
            gu, _, _, ok, msg = RE.gate_rows(left, ref, y)
            assert not ok and gu['row'] >= 4096 and not bool(torch.isfinite(left.float()).all()), msg
            print(RE.old_gate(f'ln_fwd.y rows 4096.. unwritten ({dt}, offset {offset})', left.float(), ref, 2e-5 if dt == torch.float32 else 4e-3))
            # (b) ... or written from the statistics of row - 4096
            stale, mu_s, rs_s = RE.ln_fwd_model(x, g, b, EPS, dt, stats_shift=4096)
            gu, _, _, ok, msg = RE.gate_rows(stale, ref, y)
            assert not ok and gu['row'] >= 4096, msg
            assert _bound_ok(mu_s, mu64, bm)['row'] >= 4096 and _bound_ok(rs_s, rs64, br)['violations'] > 0
            print(RE.old_gate(f'ln_fwd.y rows 4096.. with the statistics of row - 4096 ({dt}, offset {offset})', stale.float(), ref,
                              2e-5 if dt == torch.float32 else 4e-3))


def test_layernorm_stat_bounds_are_small_and_absolute():
    x, _, _ = RE.ln_inputs(257, 260, seed=2, device='cpu', offset=-300.0)
    _, mu64, rs64 = RE.ln_fwd_ref64(x, None, None, EPS)
    bm, br = RE.ln_stat_bounds(x, EPS)
    assert float((bm / mu64.abs()).max()) < 1e-5 and float((br / rs64).max()) < 1e-5
    _, mu, rs = RE.ln_fwd_model(x, None, None, EPS, torch.float32)
    assert _bound_ok(mu, mu64, bm)['violations'] == 0 and _bound_ok(rs, rs64, br)['violations'] == 0
    assert _bound_ok(mu * (1 + 1e-4), mu64, bm)['violations'] > 0 and _bound_ok(rs * (1 + 1e-4), rs64, br)['violations'] == rs.numel()


# ---------------------------------------------------------------------------------------------- 2. dgamma missing one row
def test_dgamma_missing_one_row_of_12291_fails_the_structured_bound():
    M, C = 12291, 64
    x, g, b = RE.ln_inputs(M, C, seed=3, device='cpu')
    _, mean, rstd = RE.ln_fwd_model(x, g, b, EPS, torch.float32)
    gen = torch.Generator().manual_seed(4)
    dy = torch.randn(M, C, generator=gen)
    dx64, dg64, db64 = RE.ln_bwd_ref64(dy, x, mean, rstd, g, None, None)
    dx, dg, db = RE.ln_bwd_model(dy, x, mean, rstd, g, None, None)
    bg, bb = RE.ln_bwd_param_bounds(dy, x, mean, rstd)
    assert _bound_ok(dg, dg64, bg)['violations'] == 0 and _bound_ok(db, db64, bb)['violations'] == 0
    assert RE.gate_rows(dx, dx64, dx)[3]
    grid, rows = RE.grid_rows(M, RE.LN_BLOCKS)
    assert (grid, rows) == (1024, 4) and RE.SE.colsum_chain(1024, True) == 16 + 2 + 15
    for row in (0, 4096, 8192, M - 1):        # first row, second row of a wave, second iteration, last row
        _, dg_bad, db_bad = RE.ln_bwd_model(dy, x, mean, rstd, g, None, None, drop_row=row)
        vg, vb = _bound_ok(dg_bad, dg64, bg), _bound_ok(db_bad, db64, bb)
        assert vg['violations'] > C // 2 and vb['violations'] > C // 2, (row, vg, vb)
        print(RE.old_gate(f'ln_bwd.dg without row {row} of {M}', dg_bad, dg64, 5e-5))
    # the form the issue calls vacuous: n_terms U sum |terms| exceeds the largest single term
    d_abs = (dy.double() * ((x.double() - mean.double()[:, None]) * rstd.double()[:, None])).abs()
    vacuous = M * RE.U * d_abs.sum(0)
    assert bool((vacuous > 0.5 * d_abs.median(0).values).all()) and bool((bg < 0.1 * d_abs.median(0).values).all())


# ---------------------------------------------------------------------------------------------- 3. embed_fwd clip wrap
def test_embed_fwd_clip_wrap_reading_the_next_temporal_row_fails():
    B, T, J, Din, C = 3, 7, 17, 3, 64
    x, w, b, pos, temp = RE.embed_inputs(B, T, J, Din, C, seed=5, device='cpu')
    assert temp.shape[1] == T + 3
    ref = RE.embed_fwd_ref64(x, w, b, pos, temp, B, T, J)
    bound = RE.embed_fwd_bound(x, w, b, pos, temp, B, T, J)
    good = RE.embed_fwd_model(x, w, b, pos, temp, B, T, J)
    assert _bound_ok(good, ref, bound)['violations'] == 0 and _bound_ok(ref.float(), ref, bound)['violations'] == 0
    bad = RE.embed_fwd_model(x, w, b, pos, temp, B, T, J, wrap_bug=True)
    v = _bound_ok(bad, ref, bound)
    assert v['violations'] == (B - 1) * C and v['row'] % (T * J * C) < C, v      # only the first rows of clips 1.. are hit
    first, last = RE.clip_edges(bad, B, T, J)
    rf, rl = RE.clip_edges(ref, B, T, J)
    bf, bl = RE.clip_edges(bound, B, T, J)
    assert _bound_ok(first, rf, bf)['violations'] == (B - 1) * C and _bound_ok(last, rl, bl)['violations'] == 0
    print(RE.old_gate('embed_fwd with the wrap reading temp[T]', bad, ref, 1e-6))
    big = LE.scaled_global(LE.rel(bad, ref), B * T * J, 64 * 243 * 17)
    print(f'   ... one such row per clip at 64 x 243 x 17 rows: global rel-l2 {big:.2e}')


# ---------------------------------------------------------------------------------------------- 4. embed_bwd dropped slice
def test_embed_bwd_dropped_lds_slice_fails():
    for (C, B, T, J) in ((512, 17, 3, 17), (64, 129, 3, 17)):
        Din = 3
        x, w, _, _, _ = RE.embed_inputs(B, T, J, Din, C, seed=6, device='cpu')
        dh = torch.randn(B * T * J, C, generator=torch.Generator().manual_seed(7))
        ref, good, bnd = RE.embed_bwd_ref64(dh, x, w, B, T, J), RE.embed_bwd_model(dh, x, w, B, T, J), RE.embed_bwd_bounds(dh, x, w, B, T, J)
        for k in ('dw', 'db', 'dpos', 'dtemp', 'dx'):
            assert _bound_ok(good[k], ref[k], bnd[k])['violations'] == 0, k
        nq, ns = RE.embed_slices(C)
        assert B > 8 * ns or C == 512 and ns == 2
        bad = RE.embed_bwd_model(dh, x, w, B, T, J, drop_slice=(1, ns - 1))
        for k, tol in (('dpos', 2e-5), ('dw', 2e-5), ('db', 2e-5)):
            v = _bound_ok(bad[k], ref[k], bnd[k])
            assert v['violations'] > ref[k].numel() // 2, (k, v)
            print(RE.old_gate(f'embed_bwd.{k} C={C} B={B} without slice {ns - 1} of frame 1', bad[k], ref[k], tol))
        # one single clip of one frame
        one = dh.reshape(B, T, J, C).clone()
        one[B - 1, 2] = 0
        bad1 = RE.embed_bwd_model(one.reshape(-1, C), x, w, B, T, J)
        for k in ('dpos', 'dw', 'db', 'dtemp'):
            assert _bound_ok(bad1[k], ref[k], bnd[k])['violations'] > 0, k


# ---------------------------------------------------------------------------------------------- 5. fusion dw dropped block
def test_fusion_dw_dropped_block_fails():
    for M, C in ((8193, 64), (1030, 260)):
        x_st, x_ts, w, b = RE.fuse_inputs(M, C, seed=8, device='cpu')
        _, alpha = RE.fuse_fwd_model(x_st, x_ts, w, b)
        dh = torch.randn(M, C, generator=torch.Generator().manual_seed(9))
        r64 = RE.fuse_bwd_ref64(dh, x_st, x_ts, alpha, w)
        good = RE.fuse_bwd_model(dh, x_st, x_ts, alpha, w)
        bw, bb = RE.fuse_bwd_param_bounds(dh, x_st, x_ts, alpha, w)
        assert _bound_ok(good[2], r64[2], bw)['violations'] == 0 and _bound_ok(good[3], r64[3], bb)['violations'] == 0
        for i in (0, 1):
            gu, mu, px, ok, msg = RE.gate_rows(good[i], r64[i], good[i])
            assert ok and mu['exempt'] == 0, msg
        grid, rows = RE.grid_rows(M, RE.FUSE_BLOCKS)
        db_seen = 0
        for blk in (0, grid - 1):
            bad = RE.fuse_bwd_model(dh, x_st, x_ts, alpha, w, drop_block=blk)
            vw, vb = _bound_ok(bad[2], r64[2], bw), _bound_ok(bad[3], r64[3], bb)
            assert vw['violations'] > bw.numel() // 2, (M, C, blk, vw, vb)
            db_seen += vb['violations'] > 0
            print(RE.old_gate(f'fuse_bwd.dw M={M} C={C} without the partial row of block {blk} of {grid}', bad[2], r64[2], 5e-5))
        # db is two columns, each the signed sum of a block's four or five dl: a block whose dl happen to cancel hides there, not in dw
        assert db_seen >= 1


# ---------------------------------------------------------------------------------------------- 6. bf16 copy rounding
def test_bf16_copy_rounded_toward_zero_fails_the_bit_equality():
    x = torch.randn(4097, 64, generator=torch.Generator().manual_seed(10))
    good, bad = RE.bf16_store(x), RE.bf16_trunc(x)
    assert RE.same_bits(good, x.to(torch.bfloat16)) and not RE.same_bits(bad, good)
    assert float((bad.float().abs() <= x.abs()).float().mean()) == 1.0            # it IS a rounding toward zero
    frac = float((RE.bits(bad) != RE.bits(good)).float().mean())
    assert 0.4 < frac < 0.6, frac
    print(RE.old_gate('a bf16 copy rounded toward zero', bad.float(), x, 4e-3))
    # ties go to even: 1 + 2^-8 lies between 1 and 1 + 2^-7
    tie = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    assert RE.bf16_store(tie).float().tolist() == [1.0, 1.0 + 2.0 ** -6]
    hi, lo = RE.split_planes(x)
    assert RE.same_bits(hi, good) and RE.same_bits(lo, (x - good.float()).to(torch.bfloat16))
    assert float((hi.double() + lo.double() - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())


# ---------------------------------------------------------------------------------------------- 7. alpha swapped
def test_alpha_swapped_on_one_row_fails():
    M, C = 8193, 64
    x_st, x_ts, w, b = RE.fuse_inputs(M, C, seed=11, device='cpu')
    rows, gaps = [3, 100, 101, 4097, 4098, 8190, 8192], [0.0, 10.0, -10.0, 40.0, -40.0, 90.0, -90.0]
    x_st = RE.fuse_plant_logit_gaps(x_st, x_ts, w, b, rows, gaps)
    out64, a64, l64, amp = RE.fuse_fwd_ref64(x_st, x_ts, w, b)
    assert float(((l64[rows, 0] - l64[rows, 1]) - torch.tensor(gaps, dtype=torch.float64)).abs().max()) < 1e-4
    out, alpha = RE.fuse_fwd_model(x_st, x_ts, w, b)
    ab = RE.fuse_alpha_bound(amp, C, alpha, a64)
    assert bool(torch.isfinite(out).all()) and _bound_ok(alpha, a64, ab.expand(M, 2))['violations'] == 0
    gu, mu, px, ok, msg = RE.gate_rows(out, out64, out)
    assert ok and mu['exempt'] == 0, msg
    assert float(ab.max()) < 1e-4, 'the alpha bound is absolute and small'
    for row in (5, 101, 8192):
        bad_out, bad_alpha = RE.fuse_fwd_model(x_st, x_ts, w, b, swap_row=row)
        v = _bound_ok(bad_alpha, a64, ab.expand(M, 2))
        assert v['violations'] == 2 and v['row'] // 2 == row, v
        gu, _, _, ok, msg = RE.gate_rows(bad_out, out64, out)
        assert not ok and gu['row'] == row, msg
        print(RE.old_gate(f'fuse_fwd.alpha swapped on row {row} of {M}', bad_alpha, a64, 1e-5))
    # a swap on the row whose gap is 0 changes nothing that can be seen: alpha0 = alpha1 there
    assert abs(float(a64[3, 0] - a64[3, 1])) < 1e-4


# ---------------------------------------------------------------------------------------------- head, tanh backward, average, sentinels
def test_head_and_tanh_bounds_hold_for_the_restatements_and_catch_a_wrong_row():
    M, R, D = 4097, 64, 3
    rep, w, b, dout = RE.head_inputs(M, R, D, seed=12, device='cpu')
    assert int((rep.abs() == 1).sum()) >= 4 and int((rep == 0).sum()) >= 1
    out64 = RE.head_fwd_ref64(rep, w, b)
    out = RE.head_fwd_model(rep, w, b)
    bo = RE.head_fwd_bound(rep, w, b)
    assert _bound_ok(out, out64, bo)['violations'] == 0
    shifted = out.clone()
    shifted[4096] = out[0]                       # the row past the grid cap takes row 0's value
    assert _bound_ok(shifted, out64, bo)['row'] // D == 4096
    dpre64, dw64, db64 = RE.head_bwd_ref64(dout, rep, w)
    bw, bb = RE.head_bwd_param_bounds(dout, rep, M, R, D)
    for dt, r in ((torch.float32, LE.R_F32), (torch.bfloat16, LE.R_BF16)):
        dpre, dw, db = RE.head_bwd_model(dout, rep, w, dt)
        assert _bound_ok(dpre, dpre64, RE.head_dpre_bound(dout, rep, w, r))['violations'] == 0
        assert _bound_ok(dw, dw64, bw)['violations'] == 0 and _bound_ok(db, db64, bb)['violations'] == 0
        t = RE.tanh_bwd_model(dout[:, :1].expand(M, R).contiguous(), rep, dt)
        assert _bound_ok(t, RE.tanh_bwd_ref64(dout[:, :1].expand(M, R), rep), RE.tanh_bwd_bound(dout[:, :1].expand(M, R), rep, r))['violations'] == 0
    assert float(dpre64.reshape(-1)[0]) == 0.0 and float(RE.head_dpre_bound(dout, rep, w, LE.R_F32).reshape(-1)[0]) > 0
    keep = torch.ones(M, 1)
    keep[M - 1] = 0
    assert _bound_ok((dout * keep).t() @ rep, dw64, bw)['violations'] > 0 and _bound_ok((dout * keep).sum(0), db64, bb)['violations'] > 0


def test_average_is_one_rounding_and_the_sentinels_see_an_unwritten_or_overrun_output():
    u, v = torch.randn(1028), torch.randn(1028)
    assert _bound_ok((u + v) * 0.5, (u.double() + v.double()) * 0.5, RE.average_bound(u, v))['violations'] == 0
    assert _bound_ok(u * 0.5, u.double() * 0.5, RE.average_bwd_bound(u))['violations'] == 0
    out, buf = RE.guarded((257, 4), torch.float32, 'cpu')
    assert buf.numel() == 1028 + RE.GUARD and bool(torch.isnan(out).all()) and RE.guard_intact(buf)
    out.copy_(u.reshape(257, 4))
    assert RE.guard_intact(buf) and bool(torch.isfinite(out).all())
    buf[1028] = 0.0
    assert not RE.guard_intact(buf)
    for dt in (torch.bfloat16, torch.float32):
        o2, b2 = RE.guarded((8,), dt, 'cpu')
        b2[-1] = float('inf')
        assert not RE.guard_intact(b2)
