"""The gates of tests/test_gpu_step_parity.py are shown to bite before they are trusted -- on the CPU, with the torch restatements of
tests/steperr.py standing in for the kernels of csrc/train_step.hip:

  * the uncorrupted restatements pass the gates (the fp32 model itself, and the float64 result rounded once to fp32);
  * a pose-loss gradient whose last frame of one clip takes a velocity term across the clip boundary fails the per-frame gate and the
    clip-boundary gate, and the frame is named;
  * an AdamW restatement that skips one trailing scalar fails the per-element gates;
  * a DropPath index taken as row // (rows_per_sample + 1) fails the mask equality.

No corruption here touches a kernel."""
import torch

from tests import localerr as LE
from tests import steperr as SE

U = LE.U32


# ---------------------------------------------------------------------------------------------- pose loss
def _pose_case(B=6, T=9, J=17, ls=0.5, lv=20.0, gs=1.5):
    pred, gt = SE.pose_inputs(B, T, J, seed=11, device='cpu')
    ref_l, ref_g = SE.pose_ref64(pred, gt, ls, lv, gs)
    return pred, gt, ref_l, ref_g, SE.pose_model(pred, gt, ls, lv, gs), (B, T, J, ls, lv, gs)


def test_pose_inputs_plant_what_they_promise():
    pred, gt = SE.pose_inputs(10, 9, 17, seed=3, device='cpu')
    assert float(gt[:, :, 0].abs().max()) == 0.0
    assert bool((pred[0, 2] == gt[0, 2]).all()) and bool((pred[8, 2] == gt[8, 2]).all())      # whole frames
    r = pred.double() - gt.double()
    assert bool((r[1, 5] == r[1, 4]).all()) and bool((r[9, 5] == r[9, 4]).all())                # zero velocity norm, exactly, in float64 too
    assert float(((pred[1, 5] - pred[1, 4]) - (gt[1, 5] - gt[1, 4])).abs().max()) == 0.0        # ... and in fp32, in the kernel's order
    iso = ((pred == gt).all(-1) & (gt != 0).any(-1))
    assert int(iso.sum()) >= 10 + 2 * 16


def test_pose_restatement_passes_and_a_velocity_term_across_a_clip_boundary_fails():
    pred, gt, ref_l, ref_g, model, (B, T, J, ls, lv, gs) = _pose_case()
    F = B * T
    fr = lambda x: x.reshape(F, -1)
    for clean in (model, ref_g.float()):
        assert SE.gate_units(fr(clean), fr(ref_g), fr(model), J * 3)[2]
        assert SE.gate_units(SE.boundary_pairs(clean, B, T), SE.boundary_pairs(ref_g, B, T), SE.boundary_pairs(model, B, T), 2 * J * 3)[2]
    bad = SE.pose_model(pred, gt, ls, lv, gs, leak=2)
    g, m, ok, msg = SE.gate_units(fr(bad), fr(ref_g), fr(model), J * 3)
    assert not ok and g['row'] == 2 * T + T - 1 and g['worst'] > 1e4 * m['worst'], msg
    g, m, ok, msg = SE.gate_units(SE.boundary_pairs(bad, B, T), SE.boundary_pairs(ref_g, B, T), SE.boundary_pairs(model, B, T), 2 * J * 3)
    assert not ok and g['row'] == 2, msg
    # what today's global gate (relative L2 < 2e-5 over the whole gradient) makes of the same defect at the benchmark's 64 x 243 frames
    at_step = LE.scaled_global(LE.rel(bad, ref_g), F, 64 * 243)
    print(f'velocity term across a clip boundary: global rel-l2 {LE.rel(bad, ref_g):.2e} here, {at_step:.2e} at 64 x 243 frames')


def test_pose_loss_bounds_hold_for_an_fp32_evaluation_and_are_small():
    from tests.test_gpu_train import _ref_losses
    pred, gt, ref_l, ref_g, model, (B, T, J, ls, lv, gs) = _pose_case()
    bound = SE.pose_loss_bounds(pred, gt, ls, lv)
    got = torch.stack(_ref_losses(pred, gt, ls, lv)).double()
    assert bool(((got - ref_l).abs() <= bound).all()), (got - ref_l, bound)
    assert bool((bound / ref_l < 1e-4).all()), 'the bound must be far below the value it guards'
    assert bool(((ref_l * (1 + 1e-3) - ref_l).abs() > bound).all()), 'a loss that is off by 0.1 % fails'
    # the chain of the column sum follows the launch: 15,552 partials
    assert SE.colsum_chain(15552, True) == 243 + 2 + 15 and SE.colsum_chain(15552, False) == 972 + 4


def test_loss_2d_restatement_passes_and_a_wrong_confidence_fails():
    B, T, J = 4, 9, 17
    pred, batch = SE.loss2d_inputs(B, T, J, seed=5, device='cpu')
    conf = batch[..., 2]
    assert int((conf == 0).sum()) > 0
    ref_l, ref_g = SE.loss2d_ref64(pred, batch, conf, 1.5)
    model = SE.loss2d_model(pred, batch, conf, 1.5)
    fr = lambda x: x.reshape(B * T, -1)
    assert SE.gate_units(fr(model), fr(ref_g), fr(model), J * 3)[2] and SE.gate_units(fr(ref_g.float()), fr(ref_g), fr(model), J * 3)[2]
    assert float(model[..., 2].abs().max()) == 0.0
    c2 = conf.clone()
    c2[2, 3, 5] = conf[2, 3, 6] + 0.3      # one joint reads its neighbour's confidence (an off-by-one in the stride arithmetic)
    g, m, ok, msg = SE.gate_units(fr(SE.loss2d_model(pred, batch, c2, 1.5)), fr(ref_g), fr(model), J * 3)
    assert not ok and g['row'] == 2 * T + 3, msg
    got = ((pred[..., :2] - batch[..., :2]) * conf[..., None]).norm(dim=-1).mean().double()
    assert abs(float(got - ref_l)) <= float(SE.loss2d_bound(pred, batch, conf)) < 1e-4 * float(ref_l)


# ---------------------------------------------------------------------------------------------- AdamW
HYP = dict(lr=SE.f32(1e-3), b1=SE.f32(0.9), b2=SE.f32(0.999), eps=SE.f32(1e-8), wd=SE.f32(0.01))


def test_adamw_restatement_passes_and_a_skipped_trailing_scalar_fails():
    n = 1031
    gen = torch.Generator().manual_seed(1)
    p = torch.randn(n, generator=gen) * 0.05
    g = 10.0 ** (torch.rand(n, generator=gen) * 10 - 8) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    m, v = torch.zeros(n), torch.zeros(n)
    for t in (1, 2, 3):
        ref = SE.adamw_ref64(p, g, m, v, t, **HYP)
        mod = SE.adamw_model(p, g, m, v, t, **HYP)
        once = [r.float() for r in ref]
        bad = SE.adamw_model(p, g, m, v, t, **HYP, skip_last=True)
        p64 = p.double()
        for clean in (mod, once):
            assert SE.adamw_gate_elements(clean[0].double() - p64, ref[0] - p64, mod[0].double() - p64, 0.0)[2]
            assert SE.adamw_gate_elements(clean[1], ref[1], mod[1], 0.0)[2] and SE.adamw_gate_elements(clean[2], ref[2], mod[2], 0.0)[2]
        gu, mu, ok, msg = SE.adamw_gate_elements(bad[0].double() - p64, ref[0] - p64, mod[0].double() - p64, 0.0)
        assert not ok and gu['row'] == n - 1, msg
        for i in (1, 2):
            gu, mu, ok, msg = SE.adamw_gate_elements(bad[i], ref[i], mod[i], 0.0)
            assert not ok and gu['row'] == n - 1, msg
        # gate A on the moments: the once-rounded float64 result is inside, the skipped scalar is not
        bm, bv = SE.adamw_moment_bounds(g, ref[1], ref[2], HYP['b1'], HYP['b2'])
        for got, rf, bd in ((once[1], ref[1], bm), (once[2], ref[2], bv)):
            assert LE.bound_check(got[:, None], rf[:, None], bd[:, None])['violations'] == 0
        for got, rf, bd in ((bad[1], ref[1], bm), (bad[2], ref[2], bv)):
            b = LE.bound_check(got[:, None], rf[:, None], bd[:, None])
            assert b['row'] == n - 1 and b['ratio'] > 1e3, b
        p, m, v = mod
    # the bias-correction term the comparison with torch.optim.AdamW derives: |b2_f32 - b2| / (1 - b2) at t = 1
    d = abs(HYP['b2'] - 0.999) / (1.0 - 0.999)
    assert 1e-5 < d < 2e-5, d


# ---------------------------------------------------------------------------------------------- dropout / DropPath
def test_droppath_index_off_by_one_in_rows_per_sample_fails_the_mask_equality():
    rows, C, rps = 33 * 17 + 5, 64, 17
    for p, pp, seed, sp in ((0.1, 0.2, 7, 2 ** 40 + 12345), (0.0, 0.2, 987654321012345, 7), (0.5, 0.5, 2 ** 40 + 12345, 7)):
        want = SE.branch_keep(0, rows, C, rps, p, seed, pp, sp, 'cpu')
        two = torch.cat([SE.branch_keep(0, 100, C, rps, p, seed, pp, sp, 'cpu'), SE.branch_keep(100, rows, C, rps, p, seed, pp, sp, 'cpu')])
        assert SE.mask_mismatch(two, want) == (0, -1)                      # the restatement, in slabs, passes
        x = torch.randn(rows, C)
        y = x + torch.where(torch.randn(rows, C) < 0, -1.0, 1.0) * (0.5 + torch.randn(rows, C).abs())
        out = x + (y - x) * (SE.branch_mult32(p, pp) * want)
        assert SE.mask_mismatch(out != x, want)[0] == 0                    # the zero pattern of a restated residual_drop IS the mask
        n, first = SE.mask_mismatch(SE.branch_keep(0, rows, C, rps, p, seed, pp, sp, 'cpu', rps_off=1), want)
        assert n > 0 and first // C >= rps, (n, first)                     # frame 0 = rows 0 .. 16 has the same index under both
    # DropPath off: the corruption has nothing to corrupt, the element mask alone remains
    assert SE.mask_mismatch(SE.branch_keep(0, rows, C, rps, 0.1, 7, 0.0, 1, 'cpu', rps_off=1), SE.branch_keep(0, rows, C, rps, 0.1, 7, 0.0, 1, 'cpu'))[0] == 0


def test_scales_and_kept_fraction_helpers():
    assert SE.scale32(0.0) == 1.0 and SE.branch_mult32(0.0, 0.0) == 1.0
    assert abs(SE.scale32(0.1) - 1 / 0.9) < 2 * 2 * U * (1 / 0.9) + 1e-8      # two roundings, + the rounding of p itself
    n = 1 << 22
    for p, seed in ((0.1, 7), (0.5, 2 ** 40 + 12345), (0.05, 987654321012345)):
        kept = int(SE.keep_range(0, n, p, seed, 'cpu').sum())
        assert SE.kept_fraction_ok(kept, n, SE.f32(p)), (p, seed, kept / n)
    assert not SE.kept_fraction_ok(int(0.89 * n), n, 0.1)
