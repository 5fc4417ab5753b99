"""tests/supconerr.py checked on the CPU: the float64 restatements against the reference's own loss_supcon.py (tests/golden/supcon.npz,
tools/mint_supcon.py), the rounding model against both gates, seeded corruptions of the model against the gates (every one must FAIL), and
the conditions the GPU test puts on its inputs, which involve the reference alone."""
import math
import os

import numpy as np
import pytest
import torch

from tests import supconerr as SC
from tests.helpers import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'supcon.npz'), allow_pickle=False)


@pytest.mark.parametrize('shape', SC.GPU_SHAPES)
def test_restatement_equals_the_reference_fixture(golden, shape):
    """1e-12 relative: of the loss (its scale: the larger of |loss| and 1, the size of one log-probability -- the loss of (2, 1, 1) is 0)
    and of the gradient (its scale: the largest element of the kept rows)"""
    bsz, nv, D = shape
    tag = 'sc.%d.%d.%d' % shape
    feat, lab = SC.supcon_inputs(bsz, nv, D, SC.case_seed(shape))
    assert np.array_equal(golden[tag + '.labels'], lab.numpy())
    assert tuple(golden['tau']) == (SC.f32(SC.FIXTURE_TAUS[0]), SC.f32(SC.FIXTURE_TAUS[1]))
    rows = SC.fixture_rows(bsz * nv, D)
    assert np.array_equal(golden[tag + '.rows'], rows.numpy())
    for n in (0, 1):
        loss, d = SC.supcon_ref64(feat, lab, *SC.FIXTURE_TAUS, bool(n))
        fl = float(golden[f'{tag}.n{n}.loss'])
        assert abs(float(loss) - fl) <= 1e-12 * max(abs(fl), 1.0), (n, float(loss), fl)
        fd = torch.from_numpy(golden[f'{tag}.n{n}.dfeat'])
        err = float((d.reshape(bsz * nv, D)[rows] - fd).abs().max())
        assert err <= 1e-12 * float(fd.abs().max()) or err == 0.0, (n, err, float(fd.abs().max()))


@pytest.mark.parametrize('shape', SC.NN_SHAPES)
def test_nn_restatement_equals_the_fixture(golden, shape):
    a, al, t, tl = SC.nn_inputs(*shape, SC.case_seed(shape), SC.NN_NOISE[shape])
    idx, sims, pred, acc = SC.nn_ref64(a, al, t, tl)
    assert np.array_equal(golden['nn.%d.%d.%d.argmax' % shape], idx.numpy().astype(np.int32))
    assert acc == float(golden['nn.%d.%d.%d.acc' % shape])


def test_cosine_similarity_clamps_each_norm(golden):
    """the formula mbx_nn_cosine restates: (a . t) / (max(|a|, 1e-8) max(|t|, 1e-8)) -- [3, 4] against [1, 0] gives 0.6, a zero row 0, and
    argmax takes the lowest index of a tie and the first NaN"""
    a = torch.tensor([[3.0, 4.0], [0.0, 0.0]], dtype=torch.float64)
    t = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    s = torch.nn.functional.cosine_similarity(a.unsqueeze(1), t.unsqueeze(0), dim=-1)
    assert abs(float(s[0, 0]) - 0.6) < 1e-15 and float(s[1, 0]) == 0.0
    assert int(torch.argmax(torch.tensor([0.5, 0.7, 0.7]))) == 1
    assert int(torch.argmax(torch.tensor([0.5, math.nan, 0.9, math.nan]))) == 1


MODEL_CASES = [(s, n, tt) for s in ((2, 1, 1), (3, 2, 5), (4, 2, 8), (6, 2, 33), (17, 2, 129), (32, 1, 2048), (128, 1, 4096)) for n in (False, True)
               for tt in SC.TAUS]


@pytest.mark.parametrize('shape,normalize,taus', MODEL_CASES)
def test_model_passes_both_gates(shape, normalize, taus):
    feat, lab = SC.supcon_inputs(*shape, SC.case_seed(shape), spread=(1e-3, 1e3) if normalize and shape[2] > 1 else None)
    for gs in (1.0, 3.0):
        rl, rd = SC.supcon_ref64(feat, lab, *taus, normalize, gs)
        ml, md = SC.supcon_model(feat, lab, *taus, normalize, gs)
        rloss, rrow, ok = SC.supcon_gate(ml, md, rl, rd, *SC.supcon_bounds(feat, lab, *taus, normalize, gs))
        assert ok, (shape, normalize, taus, gs, rloss, rrow)


@pytest.mark.parametrize('corrupt', SC.CORRUPTIONS)
@pytest.mark.parametrize('shape', ((4, 2, 8), (6, 2, 33), (17, 2, 129)))
def test_every_corruption_fails_a_gate(shape, corrupt):
    """tau / tau_b = 0.1 / 0.07 (the trainer's), so a dropped ratio shows; n_views = 2, so the two ways of labelling a row differ"""
    for normalize in (False, True):
        if corrupt == 'no_projection' and not normalize:
            continue
        feat, lab = SC.supcon_inputs(*shape, SC.case_seed(shape))
        rl, rd = SC.supcon_ref64(feat, lab, 0.1, 0.07, normalize)
        bounds = SC.supcon_bounds(feat, lab, 0.1, 0.07, normalize)
        assert SC.supcon_gate(*SC.supcon_model(feat, lab, 0.1, 0.07, normalize), rl, rd, *bounds)[2]
        rloss, rrow, ok = SC.supcon_gate(*SC.supcon_model(feat, lab, 0.1, 0.07, normalize, corrupt=corrupt), rl, rd, *bounds)
        print(shape, corrupt, normalize, f'loss ratio {rloss:.3g} row ratio {rrow:.3g}')
        assert not ok and max(rloss, rrow) > 10.0, (shape, corrupt, normalize, rloss, rrow)


def test_zero_row_and_clamped_norm():
    """an all-zero row under normalize: x = 0, the row's gradient is g / 1e-12 (F.normalize's clamp passes no projection); the model follows"""
    feat, lab = SC.supcon_inputs(6, 2, 33, 77)
    feat[2, 1] = 0
    rl, rd = SC.supcon_ref64(feat, lab, 0.1, 0.07, True)
    assert bool(torch.isfinite(rd).all()) and float(rd[2, 1].abs().max()) > 1e8
    ml, md = SC.supcon_model(feat, lab, 0.1, 0.07, True)
    assert SC.supcon_gate(ml, md, rl, rd, *SC.supcon_bounds(feat, lab, 0.1, 0.07, True))[2]


def test_an_anchor_without_a_positive_is_nan_in_the_reference():
    feat, _ = SC.supcon_inputs(6, 2, 33, 78)
    lab = torch.tensor([0, 0, 1, 1, 2, 2])
    loss, d = SC.supcon_ref64(feat[:, :1].contiguous(), torch.tensor([0, 0, 1, 1, 2, 3]), 0.1, 0.07, False)
    assert math.isnan(float(loss)) and bool(torch.isnan(d).all())
    loss, d = SC.supcon_ref64(feat[:, :1].contiguous(), lab, 0.1, 0.07, False)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(d).all())
    ml, md = SC.supcon_model(feat[:, :1].contiguous(), torch.tensor([0, 0, 1, 1, 2, 3]), 0.1, 0.07, False)
    assert math.isnan(float(ml)) and bool(torch.isnan(md).all())


@pytest.mark.parametrize('shape', SC.NN_SHAPES)
def test_nn_inputs_meet_the_conditions_of_the_gpu_test(shape):
    """on the float64 reference alone: the accuracy of the clustered cases lies in [0.5, 0.9], at most 2 % of the rows have a top-two
    margin below twice the similarity bound"""
    a, al, t, tl = SC.nn_inputs(*shape, SC.case_seed(shape), SC.NN_NOISE[shape])
    idx, sims, pred, acc = SC.nn_ref64(a, al, t, tl)
    bound = SC.nn_sim_bound(a, t)
    margin, unit = SC.nn_margin(sims, bound)
    print(shape, 'accuracy', acc, 'largest bound', float(bound.max()), 'under the margin', float((~unit).double().mean()))
    lo, hi = SC.NN_ACCURACY[shape]
    assert lo <= acc <= hi, acc
    assert float((~unit).double().mean()) <= SC.MAX_UNDER_MARGIN
    assert float(bound.max()) < 1e-4
