"""The ragged restatements and gates of tests/raggederr.py, checked on the CPU: the ragged forward through `model.run` with RaggedMockOps
equals the per-clip forwards through the plain MockOps bit for bit; the uncorrupted provider passes every gate; each seeded corruption
fails one."""
import numpy as np
import pytest
import torch

from motionbert_amd import model as M
from motionbert_amd.augment import FLIP_PERM
from oracle.augment_oracle import flip_data
from oracle.torch_ops import MockOps
from tests import raggederr as RE
from tests.helpers import build_model, make_input, trained_like

CFG = dict(dim_in=3, dim_out=3, dim_feat=64, dim_rep=64, depth=2, num_heads=2, mlp_ratio=2, num_joints=17, maxlen=48)
LENS = [33, 9, 1, 40, 17]           # both sides of the 32-key fragment edge, a single frame, the longest last but one
SCALE = 32 ** -0.5


@pytest.fixture(scope='module')
def net():
    m = build_model(CFG, seed=3)
    trained_like(m, 4)
    m.precision = 'fp32'
    return m.eval()


@pytest.fixture(scope='module')
def x():
    return make_input(1, sum(LENS), 17, 21)[0]


def _ragged(net, x, lens, what, ops):
    tab, ft = RE.tables(lens)
    with torch.no_grad():
        return M.run(ops, net, x[None], what, None, ragged=(torch.from_numpy(tab), torch.from_numpy(ft), len(lens), max(lens)))[0]


def _per_clip(net, x, lens, what):
    outs, at = [], 0
    with torch.no_grad():
        for L in lens:
            outs.append(M.run(MockOps(), net, x[at:at + L][None].contiguous(), what)[0])
            at += L
    return torch.cat(outs)


@pytest.mark.parametrize('what', [False, True])
def test_ragged_forward_equals_the_per_clip_forwards(net, x, what):
    ops = RE.RaggedMockOps()
    got = _ragged(net, x, LENS, what, ops)
    want = _per_clip(net, x, LENS, what)
    assert got.shape == want.shape == (sum(LENS), 17, 64 if what else 3)
    assert RE.model_check(got, want) == 0
    assert ops.calls.count('embed_fwd_ragged') == 1 and ops.calls.count('attn_fwd_ragged') == 2 * CFG['depth'] and 'embed_fwd' not in ops.calls
    assert float(got.std()) > 1e-3


def test_ragged_flip_form_equals_two_forwards_per_clip(net, x):
    perm = torch.tensor(FLIP_PERM, dtype=torch.int32)
    got = _ragged(net, x, LENS, ('tta', perm), RE.RaggedMockOps())
    want = (_per_clip(net, x, LENS, False) + flip_data(_per_clip(net, flip_data(x[None])[0], LENS, False)[None])[0]) / 2.0
    assert RE.model_check(got, want) == 0


def test_ragged_is_an_inference_path(net, x):
    tab, ft = RE.tables(LENS)
    ragged = (torch.from_numpy(tab), torch.from_numpy(ft), len(LENS), max(LENS))
    with pytest.raises(RuntimeError, match='inference'):
        M.run(RE.RaggedMockOps(), net, x[None], False, None, ragged=ragged)                    # grad mode on
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='pooled'):
            M.run(RE.RaggedMockOps(), net, x[None], ('pool', 1, 0.0, 0), None, ragged=ragged)
        with pytest.raises(RuntimeError, match='x \\[1,F,J,C\\]'):
            M.run(RE.RaggedMockOps(), net, torch.cat([x[None], x[None]]), False, None, ragged=ragged)
        with pytest.raises(RuntimeError, match='max_len'):
            M.run(RE.RaggedMockOps(), net, x[None], False, None, ragged=ragged[:3] + (CFG['maxlen'] + 1,))


# ------------------------------------------------------------------------------------------------ the gates and the corruptions
def _attn_case(corrupt, lens=LENS, Jn=3, H=2, hd=32, seed=5):
    qkv = RE.attn_inputs(lens, Jn, H, hd, seed)
    o, lse = RE.run_attn(RE.RaggedMockOps(corrupt), qkv, lens, Jn, H, SCALE)
    return RE.attn_check(o, lse, qkv, lens, Jn, H, SCALE)


def _embed_case(corrupt, tta=False, lens=LENS, seed=6):
    inp = RE.embed_inputs(lens, 17, 3, 64, CFG['maxlen'], seed)
    tab, ft = RE.tables(lens)
    F = sum(lens)
    h = torch.full(((2 if tta else 1) * F * 17, 64), float('nan'))
    ops = RE.RaggedMockOps(corrupt)
    if tta:
        ops.embed_fwd_tta_ragged(inp['x'], torch.tensor(FLIP_PERM, dtype=torch.int32), inp['w'], inp['b'], inp['pos'], inp['temp'], torch.from_numpy(ft), h, F, 17)
        a = RE.embed_check(h[:F * 17], inp, torch.from_numpy(ft))
        b = RE.embed_check(h[F * 17:], dict(inp, x=flip_data(inp['x'])), torch.from_numpy(ft))
        return dict(ratio=max(a['ratio'], b['ratio']), nan=a['nan'] + b['nan'])
    ops.embed_fwd_ragged(inp['x'], inp['w'], inp['b'], inp['pos'], inp['temp'], torch.from_numpy(ft), h, F, 17)
    return RE.embed_check(h, inp, torch.from_numpy(ft))


OUT_CLIPS, OUT_TRACKS = [9, 9, 3, 9, 1, 5], [21, 10, 5]          # three tracks: clips 9 + 9 + 3 | 9 + 1 | 5


def _output_case(corrupt, **kw):
    case = RE.output_case(OUT_CLIPS, OUT_TRACKS, 31, **kw)
    return RE.run_output(RE.RaggedMockOps(corrupt), 'cpu', case, track_start=case['track_start'])


def _tta_case(net, x, corrupt):
    perm = torch.tensor(FLIP_PERM, dtype=torch.int32)
    got = _ragged(net, x, LENS, ('tta', perm), RE.RaggedMockOps(corrupt))
    return RE.model_check(got, _ragged(net, x, LENS, ('tta', perm), RE.RaggedMockOps()))


def test_the_uncorrupted_provider_passes_every_gate():
    res = _attn_case(None)
    assert RE.attn_passes(res), res
    for tta in (False, True):
        e = _embed_case(None, tta)
        assert e['ratio'] <= 1.0 and e['nan'] == 0, e
    for kw in (dict(), dict(rootrel=True), dict(gt_2d=True, xc=2), dict(vid_size=(1920, 1080)), dict(gt_2d=True, vid_size=(720, 1280))):
        assert _output_case(None, **kw) == dict(out=0, pred_kept=True), kw


def test_an_untrusted_table_row_is_skipped():
    """a row outside [0, F), an empty one and one longer than max_len: the other clips keep their bits, the three stay untouched"""
    lens, Jn, H, hd = LENS, 3, 2, 32
    qkv = RE.attn_inputs(lens, Jn, H, hd, 5)
    o0, l0 = RE.run_attn(RE.RaggedMockOps(), qkv, lens, Jn, H, SCALE)
    tab = RE.tables(lens)[0].copy()
    tab[0, 0], tab[2, 1], tab[3, 1] = -1, 0, 41
    o1, l1 = RE.run_attn(RE.RaggedMockOps(), qkv, lens, Jn, H, SCALE, tab=tab, max_len=40)
    for i, (r0, r1, L) in enumerate(RE.rows_of(lens, Jn)):
        if i in (0, 2, 3):
            assert torch.isnan(o1[r0:r1]).all() and torch.isnan(l1[r0:r1]).all()
        else:
            assert torch.equal(o1[r0:r1], o0[r0:r1]) and torch.equal(l1[r0:r1], l0[r0:r1])


@pytest.mark.parametrize('corrupt', RE.CORRUPTIONS)
def test_every_corruption_fails_a_gate(net, x, corrupt):
    if corrupt == 'global_t':                      # the row of the batch instead of the frame of the clip as temporal position
        for tta in (False, True):
            e = _embed_case(corrupt, tta)
            assert e['ratio'] > 1e3, e
    elif corrupt in ('neighbour_keys', 'last_key_masked', 'frag_off_by_one'):
        res = _attn_case(corrupt)
        assert res['row'] > 10.0 and res['missing'] == 0, res
    elif corrupt == 'lse_wrong_row':
        res = _attn_case(corrupt)
        assert res['row'] <= 1.0 and (res['lse'] > 10.0 or res['stray'] > 0), res
    elif corrupt == 'clip_skipped':
        res = _attn_case(corrupt)
        assert res['missing'] == LENS[-1] * 3, res
    elif corrupt == 'z_track_starts':
        assert _output_case(corrupt)['out'] == len(OUT_CLIPS) - len(OUT_TRACKS)      # one z per clip that opens no track
        assert _output_case(corrupt, rootrel=True)['out'] == 0                       # rootrel zeroes joint 0 anyway
    elif corrupt == 'z_every_frame':
        assert _output_case(corrupt)['out'] == sum(OUT_CLIPS) - len(OUT_CLIPS)
    elif corrupt == 'tta_unshifted':
        assert _tta_case(net, x, corrupt) > 0
    else:
        raise AssertionError(corrupt)
    assert len(RE.CORRUPTIONS) >= 8


def test_the_restatement_is_per_clip():
    """the softmax of a query runs over the keys of its clip only: moving another clip's keys does not move a bit of this clip's rows"""
    lens, Jn, H, hd = [5, 33, 7], 3, 2, 32
    qkv = RE.attn_inputs(lens, Jn, H, hd, 9, pad=0)
    o0, l0 = RE.attn_ref(qkv, lens, Jn, H, SCALE)
    q2 = qkv.clone()
    r0, r1, _ = RE.rows_of(lens, Jn)[1]
    q2[r0:r1] = torch.randn(r1 - r0, qkv.shape[1], generator=torch.Generator().manual_seed(1))
    o1, l1 = RE.attn_ref(q2, lens, Jn, H, SCALE)
    keep = np.r_[0:r0, r1:qkv.shape[0]]
    assert torch.equal(o0[keep], o1[keep]) and torch.equal(l0[keep], l1[keep]) and not torch.equal(o0[r0:r1], o1[r0:r1])
