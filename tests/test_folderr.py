"""The gates of tests/test_gpu_fold_parity.py are shown to bite before they are trusted -- on the CPU, with the restatements of
tests/folderr.py standing in for the kernels.  Every restatement passes every gate on every shape the GPU test uses, and each of the
eleven named corruptions (folderr.CORRUPTIONS) fails at least one:

   1. rsum_unrounded             rsum summed from the fp32 product w gamma instead of the rounded W'
   2. bias_from_previous         bias_f of a bias-less descriptor picks up the previous descriptor's bias
   3. wt_ragged_column_lost      W'^T (and prep_weights' dst_t) without the columns of the ragged last tile
   4. lo_from_truncated_hi       the lo plane taken from the hi rounded toward zero
   5. rowc_odd_block_dropped     lnbwd_rowc without the odd last block
   6. rowc_invc_of_k             1 / K of the GEMM in place of 1 / C
   7. dgamma_after_update        dgamma formed from dw after the in-place update
   8. dbeta_db_beta              dbeta = sum db beta in place of sum w db
   9. dgamma_ragged_block_lost   the ragged last 64-row block missing from dgamma
  10. rsum_one_row_one_step      one row of one descriptor's rsum off by one bf16 step of its largest term
  11. second_pass_skipped        split / gelu without the elements of the second grid pass

Every corruption is applied to a restatement, never to a kernel."""
import pytest
import torch

from tests import folderr as FE
from tests import localerr as LE
from tests import rowerr as RE

BF, F32 = torch.bfloat16, torch.float32
SEEN = set()


@pytest.fixture(scope='module')
def fold_set():
    return FE.fold_inputs(FE.DESC_SET, FE.DESC_BIAS, seed=101, device='cpu')


def _rows_ok(d, bias_f, rsum):
    bf64, rs64 = FE.fold_rows_ref64(d)
    bb, br = FE.fold_rows_bounds(d)
    return FE.bound_gate(bias_f, bf64, bb), FE.bound_gate(rsum, rs64, br)


# ---------------------------------------------------------------------------------------------- prep_weights, W' and W'^T
@pytest.mark.parametrize('kind', sorted(FE.PREP_KINDS))
def test_prep_restatement_and_its_corruptions(kind):
    for shapes in (FE.DESC_SET, FE.DESC_SINGLE):
        for w in FE.prep_inputs(shapes, seed=102, device='cpu'):
            N, K = w.shape
            for need_t in (False, True):
                dn, dt = FE.prep_model(w, kind, need_t)
                assert dn.dtype == FE.PREP_KINDS[kind][1] and (dt is None) == (not need_t)
                assert bool(torch.isfinite(dn.float()).all())
                if need_t:
                    assert RE.same_bits(dt, dn.t().contiguous())           # the conversion is elementwise: T(w^T) = T(w)^T
            w64 = w.double()
            if kind == 'lo':        # hi + lo restores w to 2^-16 (two bf16 roundings), and the truncated hi does not pass for the rounded one
                hi = RE.bf16_store(w)
                assert float((hi.double() + dn.double() - w64).abs().max()) <= 2.0 ** -16 * float(w.abs().max())
                bad = FE.prep_model(w, kind, True, corrupt='lo_from_truncated_hi')
                if N * K >= 64:
                    assert not RE.same_bits(bad[0], dn) and not RE.same_bits(bad[1], dt)
                    SEEN.add('lo_from_truncated_hi')
            else:
                assert float((dn.double() - w64).abs().max()) <= (2.0 ** -8 if kind == 'bf16' else 0.0) * float(w.abs().max())
            bad_t = FE.prep_model(w, kind, True, corrupt='wt_ragged_column_lost')[1]
            assert RE.same_bits(bad_t, dt) == (N % 32 == 0)
            if N % 32:
                assert FE.diff_count(bad_t, dt)[0] == K * (N % 32)
                SEEN.add('wt_ragged_column_lost')
    if kind == 'lo':
        tie = torch.tensor(FE.SPLIT_PLANT).reshape(2, 2)
        assert RE.bf16_store(tie).float().reshape(-1).tolist() == [1.0, 1.0 + 2.0 ** -6, -0.375, 2.0 ** -120]
        assert FE.cvt(tie, 'lo').float().reshape(-1).tolist() == [2.0 ** -8, -(2.0 ** -8), 0.0, 0.0]
        assert FE.cvt(tie, 'lo', 'lo_from_truncated_hi').float().reshape(-1).tolist() == [2.0 ** -8, 2.0 ** -8, 0.0, 0.0]


def test_folded_weights_keep_the_sign_of_zero_and_lose_no_ragged_column(fold_set):
    for d, (N, K) in zip(fold_set, FE.DESC_SET):
        wn, wt = FE.fold_w_model(d, True)
        assert RE.same_bits(wt, wn.t().contiguous()) and FE.fold_w_model(d, False)[1] is None
        z = wn[:, K // 3]
        assert bool((z == 0).all()) and RE.same_bits(z, torch.where(d['w'][:, K // 3] < 0, -0.0, 0.0).to(BF))
        if N > 1:
            assert len(set(RE.bits(z).tolist())) == 2                      # both zeros occur
        neg = (2 * K) // 3
        assert bool(((wn[:, neg].float() * d['w'][:, neg]) <= 0).all())
        bad = FE.fold_w_model(d, True, corrupt='wt_ragged_column_lost')[1]
        assert RE.same_bits(bad, wt) == (N % 32 == 0)


# ---------------------------------------------------------------------------------------------- bias_f and rsum
def test_fold_rows_restatement_is_inside_its_bounds_and_has_no_ties(fold_set):
    single = FE.fold_inputs(FE.DESC_SINGLE, (True,), seed=103, device='cpu')
    for d in fold_set + single:
        bias_f, rsum, ties = FE.fold_rows_model(d)
        assert ties == 0, 'the seeds are chosen so that fma32 is fmaf on every step: the GPU test then allows no exception'
        vb, vr = _rows_ok(d, bias_f, rsum)
        assert vb['violations'] == 0 and vr['violations'] == 0, (d['w'].shape, vb, vr)
        bf64, rs64 = FE.fold_rows_ref64(d)
        vb, vr = _rows_ok(d, bf64.float(), rs64.float())                   # the float64 result rounded once passes too
        assert vb['violations'] == 0 and vr['violations'] == 0
        bb, br = FE.fold_rows_bounds(d)
        assert float((br / rs64.abs().clamp_min(1e-3)).median()) < 1e-4     # the bounds are small: 1e-6-class of sum |terms|


def test_rsum_from_the_unrounded_product_fails(fold_set):
    for d, (N, K) in zip(fold_set, FE.DESC_SET):
        _, rsum, _ = FE.fold_rows_model(d, corrupt='rsum_unrounded')
        vr = _rows_ok(d, FE.fold_rows_model(d)[0], rsum)[1]
        if K >= 33:
            assert vr['violations'] > N // 2, (N, K, vr)
            SEEN.add('rsum_unrounded')
        print(RE.old_gate(f'rsum of the unrounded product, {N} x {K}', rsum, FE.fold_rows_ref64(d)[1], 2e-6))


def test_bias_of_the_previous_descriptor_fails(fold_set):
    for i, (d, has_b) in enumerate(zip(fold_set, FE.DESC_BIAS)):
        bias_f, rsum, _ = FE.fold_rows_model(d, corrupt='bias_from_previous', prev=fold_set[i - 1] if i else None)
        vb = _rows_ok(d, bias_f, rsum)[0]
        if has_b:
            assert vb['violations'] == 0
        else:
            assert vb['violations'] >= max(1, d['w'].shape[0] * 9 // 10), vb
            SEEN.add('bias_from_previous')


def test_one_row_of_rsum_off_by_one_bf16_step(fold_set):
    """The point of the work.  One row of the 1536 x 512 descriptor's rsum moved by one bf16 step of its largest term (2^-10 here): the
    row's bound is 50 x smaller, so the elementwise gate sees it; over the 1536 rows it is 2.2e-5 of the norm, which the old tolerance of
    2e-6 still sees at this size (2^-10 / |rsum| with |rsum| = 46; it would take 8e7 weights for the step to pass).  What the old gate
    lets through is any single row off by less than 2e-6 of the whole norm: the same row off by 1e-6 of the norm, 4.6e-5 or a twentieth
    of that bf16 step, passes the whole-tensor gate and fails the elementwise one."""
    d = fold_set[0]
    bf64, rs64 = FE.fold_rows_ref64(d)
    good = FE.fold_rows_model(d)[1]
    for row in (0, 777, 1535):
        bad = FE.fold_rows_model(d, corrupt='rsum_one_row_one_step', row=row)[1]
        vr = _rows_ok(d, bf64.float(), bad)[1]
        assert vr['violations'] == 1 and vr['row'] == row and vr['ratio'] > 10, vr
        u = LE.unit_errors(bad.reshape(-1, 1), rs64.reshape(-1, 1), 1, 1)
        assert u['row'] == row
        print(RE.old_gate(f'rsum row {row} off by one bf16 step of its largest term', bad, rs64, 2e-6))
        half = 1e-6 * float(rs64.norm())           # half of what the old tolerance admits, in one row
        small = good.clone()
        small[row] += half
        old = LE.rel(small, rs64)
        vs = _rows_ok(d, bf64.float(), small)[1]
        print(f'   ... by 1e-6 of the whole norm ({half:.2e}): global rel-l2 {old:.2e} against 2e-06, bound ratio {vs["ratio"]:.1f}')
        assert old < 2e-6, 'the old whole-tensor gate lets this through'
        assert vs['violations'] == 1 and vs['row'] == row, vs
    SEEN.add('rsum_one_row_one_step')


# ---------------------------------------------------------------------------------------------- lnbwd_rowc
@pytest.mark.parametrize('nb,M,C', FE.ROWC_CASES)
def test_rowc_restatement_and_its_corruptions(nb, M, C):
    part, rstd = FE.rowc_inputs(nb, M, seed=104 + nb, device='cpu')
    good = FE.rowc_model(part, rstd, C)
    assert good.shape == (M, 4) and RE.same_bits(good[:, 0], rstd) and RE.same_bits(good[:, 3], torch.zeros(M))
    assert FE.bound_gate(good, FE.rowc_ref64(part, rstd, C), FE.rowc_sanity_bound(part, rstd, C))['violations'] == 0
    bad = FE.rowc_model(part, rstd, C, corrupt='rowc_invc_of_k', K=3 * C)
    assert FE.diff_count(bad, good)[0] >= M
    SEEN.add('rowc_invc_of_k')
    bad = FE.rowc_model(part, rstd, C, corrupt='rowc_odd_block_dropped')
    assert RE.same_bits(bad, good) == (nb % 2 == 0)
    if nb % 2:
        assert FE.diff_count(bad, good)[0] >= M
        SEEN.add('rowc_odd_block_dropped')


def test_rowc_cases_are_the_cross_the_gate_asks_for():
    nbs, Ms, Cs = zip(*FE.ROWC_CASES)
    assert set(nbs) == {1, 2, 3, 16, 25} and set(Ms) == {1, 255, 256, 257, 4131} and set(Cs) == {192, 512}
    assert len(set(FE.ROWC_CASES)) == len(FE.ROWC_CASES) < 20 and any(nb % 2 and M == 257 for nb, M, _ in FE.ROWC_CASES)


# ---------------------------------------------------------------------------------------------- unfold_norm_grads
@pytest.mark.parametrize('N,K,vec', [s + (v,) for s, v in zip(FE.UNFOLD_SHAPES, FE.UNFOLD_VEC)])
def test_unfold_restatement_and_its_corruptions(N, K, vec):
    assert FE.unfold_vec(K) == vec
    dwp, db, w, gamma, beta = FE.unfold_inputs(N, K, seed=105, device='cpu')
    assert float(db[N // 2]) == 0.0 and float(beta[K // 2]) == 0.0
    keep = dwp.clone()
    dw64, dg64, db64 = FE.unfold_ref64(dwp, db, w, gamma, beta)
    dw, dg, dbt, ties_dw, ties_chain = FE.unfold_model(dwp, db, w, gamma, beta)
    assert RE.same_bits(dwp, keep) and ties_dw == 0 and ties_chain == 0
    bg, bb = FE.unfold_bounds(dwp, db, w)
    assert FE.unfold_chain(N, K) == 16 + 2 + RE.SE.colsum_chain(RE.cdiv(N, 64), vec)
    assert FE.bound_gate(dg, dg64, bg)['violations'] == 0 and FE.bound_gate(dbt, db64, bb)['violations'] == 0
    assert FE.bound_gate(dg64.float(), dg64, bg)['violations'] == 0 and FE.bound_gate(dbt, db64, bb)['violations'] == 0
    assert float((dw.double() - dw64).abs().max()) <= 2 * RE.U * float((gamma.double() * dwp.double()).abs().max() + (db.double()[:, None] * beta.double()).abs().max())
    assert RE.same_bits(dw[N // 2], (gamma * dwp[N // 2]))            # the zero row of db: dw = gamma dw' exactly
    # the colsum restatement against a plain sum of the same partial rows
    part = torch.randn(RE.cdiv(N, 64) + 70, 2 * K, generator=torch.Generator().manual_seed(1))
    cs = FE.colsum_model(part, vec)
    assert float((cs.double() - part.double().sum(0)).abs().max()) <= RE.gam(RE.SE.colsum_chain(part.shape[0], vec)) * float(part.double().abs().sum(0).max())

    bad = FE.unfold_model(dwp, db, w, gamma, beta, corrupt='dgamma_after_update')
    assert RE.same_bits(bad[0], dw) and RE.same_bits(bad[2], dbt)
    assert FE.bound_gate(bad[1], dg64, bg)['violations'] >= max(1, K * 9 // 10)
    SEEN.add('dgamma_after_update')
    bad = FE.unfold_model(dwp, db, w, gamma, beta, corrupt='dbeta_db_beta')
    assert RE.same_bits(bad[1], dg)
    assert FE.bound_gate(bad[2], db64, bb)['violations'] >= max(1, K * 9 // 10) or N == 1
    if N > 1:
        SEEN.add('dbeta_db_beta')
    else:           # one row whose db is the planted zero: both forms are exactly 0, there is nothing to see
        assert float(db[0]) == 0.0
    bad = FE.unfold_model(dwp, db, w, gamma, beta, corrupt='dgamma_ragged_block_lost')
    if N % 64:
        assert FE.bound_gate(bad[1], dg64, bg)['violations'] >= max(1, K * 9 // 10)
        print(RE.old_gate(f'dgamma {N} x {K} without the ragged last block', bad[1], dg64, 2e-5))
        SEEN.add('dgamma_ragged_block_lost')
    else:
        assert RE.same_bits(bad[1], dg)


# ---------------------------------------------------------------------------------------------- split_bf16, gelu_fwd
@pytest.mark.parametrize('n', FE.FLAT_N)
def test_split_restatement_and_the_skipped_second_pass(n):
    x = FE.split_inputs(n, seed=106, device='cpu')
    hi, lo = FE.split_model(x)
    assert RE.same_bits(hi, x.to(BF)) and RE.same_bits(lo, (x - hi.float()).to(BF))
    assert float((hi.double() + lo.double() - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())
    bh, bl = FE.split_model(x, corrupt='second_pass_skipped')
    past = n - FE.first_pass(n)
    assert past == (8 if n > FE.GRID_CAP * 1024 else 0)
    assert FE.diff_count(bh, hi)[0] == past and FE.diff_count(bl, lo)[0] == past
    if past:
        SEEN.add('second_pass_skipped')


@pytest.mark.parametrize('dtype', [F32, BF])
@pytest.mark.parametrize('n', FE.FLAT_N)
def test_gelu_model_passes_its_gate_and_a_wrong_unit_fails(n, dtype):
    u = FE.gelu_inputs(n, dtype, seed=107, device='cpu')
    if n >= len(FE.GELU_PLANT):
        assert u[:12].float().tolist() == torch.tensor(FE.GELU_PLANT).to(dtype).float().tolist()
    ref, model = FE.gelu_ref64(u), FE.gelu_model(u)
    g = FE.gelu_gate(model, ref, model, u)
    assert g['n_over'] == 0 and g['ratio'] <= 1.0 / FE.GELU_MULT + 1e-12, g
    assert FE.gelu_gate(ref.to(dtype), ref, model, u)['n_over'] == 0          # float64 rounded once passes
    bad = FE.gelu_model(u, corrupt='second_pass_skipped')
    past = n - FE.first_pass(n)
    gb = FE.gelu_gate(bad, ref, model, u)
    assert gb['n_over'] == past // 4 and (past == 0 or gb['unit'] >= FE.first_pass(n) // 4)
    if n >= 1028:           # one lane of one vector takes its neighbour's value; the tanh form of GELU everywhere
        k = 4 * 200 + 1
        one = model.clone()
        one[k] = model[k - 1]
        g1 = FE.gelu_gate(one, ref, model, u)
        assert g1['n_over'] == 1 and g1['unit'] == 200, g1
        if dtype == F32:    # (5e-4 at the most: below half a bf16 step of the values it occurs at, so nothing for the bf16 gate to see)
            tanh = torch.nn.functional.gelu(u, approximate='tanh')
            assert FE.gelu_gate(tanh, ref, model, u)['n_over'] > n // 40


def test_every_named_corruption_was_caught():
    """runs last in the module: each name of folderr.CORRUPTIONS failed a gate in one of the tests above"""
    assert sorted(SEEN) == sorted(FE.CORRUPTIONS), sorted(set(FE.CORRUPTIONS) - SEEN)
