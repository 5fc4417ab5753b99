"""Ragged batches on a real MI355X: mbx_attn_fwd_ragged, mbx_embed_fwd_ragged / _tta_ragged, `DSTformer.forward_ragged`, the ragged
`flip_tta` and `wild.infer(batching='ragged')` (restatements, inputs and CPU checks: tests/raggederr.py, tests/test_raggederr.py).

Gates.
  kernels     EQUAL BITS with the per-clip calls (mbx_attn_fwd(B = 1, T = L), mbx_embed_fwd / _tta on the clip's rows): the ragged kernels
              run the per-clip kernels' body on every problem, so this is derived, not measured.  Outputs are NaN-filled first: every row
              inside the table is written, no row outside it is.  Attention also against float64: bf16 through the per-unit gate of
              tests/localerr.py as tests/test_gpu_local_parity.py applies it to attn_fwd (units row and (row, head); 2 x the rounding model,
              and per unit), clip by clip since that gate normalises by the mean norm of ONE sequence length; a clip of one frame has
              o = v exactly and the model error 0, so there the kernel error must be 0 too.  fp32 through raggederr.attn_check.
  model       fp32: 1e-6 absolute on normalised output against the per-clip forwards, the gate tests/test_gpu_augment.py:76 uses when the
              same network runs at another batch composition (the GEMMs see F J rows instead of L J).  bf16: the ragged output against
              the fp32 ragged output under TOL_BF16_OUT of tests/test_gpu_model.py (4e-2 relative L2); the bf16 ragged-against-per-clip
              difference is recorded only.
  wild.infer  1e-6 (times min(w, h) / 2 in pixel mode) against the reference's batch-1 loop through the same model and against
              batching='equal'; the number of network calls is ceil(frames / (max_batch clip_len)).
The model is tests/golden/tiny_trained with its temporal embedding (16 rows in the fixture) continued to 256 rows by a seeded draw of the
initialiser's scale: clips of 243 frames need them, and the fixture's rows stay where they are.
What was measured goes to ragged_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd.engine import MODE_TEMPORAL
from tests import localerr as LE
from tests import raggederr as RE
from tests import wilderr as WE
from tests.helpers import build_model, load_golden, make_input, rel_l2, trained_like

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
GATE = 1e-6
TOL_BF16_OUT = 4e-2           # tests/test_gpu_model.py
VID = (1920, 1080)
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'ragged_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'ragged_parity.txt'), 'w') as f:
        f.write('ragged batches: elements whose bits differ from the per-clip calls (0 passes), errors as a share of their gate (<= 1 passes),\n'
                'and recorded differences (no gate)\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + '  '.join(f'{n} {v:.4g}' if isinstance(v, float) else f'{n} {v}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, math.nan, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ mbx_attn_fwd_ragged
def _per_clip_attn(ops, qkv, lens, Jn, H, scale):
    o, lse = nan(qkv.shape[0], qkv.shape[1] // 3, dtype=qkv.dtype), nan(qkv.shape[0], H)
    for r0, r1, L in RE.rows_of(lens, Jn):
        ops.attn_fwd(qkv[r0:r1], o[r0:r1], lse[r0:r1], 1, L, Jn, H, scale, MODE_TEMPORAL)
    return o, lse


@pytest.mark.parametrize('dtype', [BF, torch.float32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('form', ['shared', 'private'])
def test_attn_fwd_ragged_equals_the_per_clip_calls(ops, form, hd, dtype):
    lens = RE.SHARED_LENS if form == 'shared' else RE.PRIVATE_LENS
    Jn, H, scale = 3, 2, hd ** -0.5
    tag = f'attn.{form}.d{hd}.{"bf16" if dtype == BF else "fp32"}'
    qkv = RE.attn_inputs(lens, Jn, H, hd, 40 + hd, dtype=dtype).to(DEV)
    n = sum(lens) * Jn
    o, lse = RE.run_attn(ops, qkv, lens, Jn, H, scale)
    want_o, want_l = _per_clip_attn(ops, qkv, lens, Jn, H, scale)
    torch.cuda.synchronize()
    rec = dict(o_bits=int((bits(o[:n]) != bits(want_o[:n])).sum()), lse_bits=int((bits(lse[:n]) != bits(want_l[:n])).sum()),
               missing=int(torch.isnan(o[:n].float()).any(1).sum() + torch.isnan(lse[:n]).any(1).sum()),
               stray=int((~torch.isnan(o[n:].float())).sum() + (~torch.isnan(lse[n:])).sum()))
    # one table row out of range: its clip is not written, the other clips keep their bits
    tab = RE.tables(lens)[0].copy()
    bad = len(lens) // 2
    tab[bad, 0] = qkv.shape[0] // Jn - lens[bad] + 1
    o2, lse2 = RE.run_attn(ops, qkv, lens, Jn, H, scale, tab=tab)
    torch.cuda.synchronize()
    r0, r1, _ = RE.rows_of(lens, Jn)[bad]
    keep = torch.ones(qkv.shape[0], dtype=torch.bool, device=DEV)
    keep[r0:r1] = False
    rec['skip_written'] = int((~torch.isnan(o2[~keep].float())).sum() + (~torch.isnan(lse2[~keep])).sum())
    rec['skip_others'] = int((bits(o2[keep]) != bits(o[keep])).sum() + (bits(lse2[keep]) != bits(lse[keep])).sum())
    # against float64
    if dtype == BF:
        ex_o, _ = RE.attn_ref(qkv, lens, Jn, H, scale)
        md_o, _ = RE.attn_ref(qkv, lens, Jn, H, scale, model=True)
        worst = 0.0
        for c0, c1, L in RE.rows_of(lens, Jn):
            for shp in ((1, H * hd), (1, hd)):
                g = LE.unit_errors(o[c0:c1], ex_o[c0:c1], *shp, full=True)
                m = LE.unit_errors(md_o[c0:c1], ex_o[c0:c1], *shp, full=True)
                if m['worst'] == 0.0:
                    assert L == 1 and g['worst'] == 0.0, (tag, L, g['worst'])
                    continue
                x = LE.per_unit_excess(g, m, *shp)
                worst = max(worst, x['excess'], g['worst'] / (2.0 * m['worst']))
                assert m['exempt'] <= LE.MAX_EXEMPT, (tag, L, shp, m['exempt'])
                assert g['worst'] <= 2.0 * m['worst'] and x['excess'] <= 1.0, (tag, L, shp, g['worst'], m['worst'], x)
        rec['f64_share'] = worst
    else:
        res = RE.attn_check(o, lse, qkv[:n], lens, Jn, H, scale)
        rec.update(f64_share=res['row'], f64_lse_share=res['lse'])
        assert RE.attn_passes(dict(res, stray=0)), (tag, res)
    print(tag, rec)
    REPORT[tag] = rec
    assert rec['o_bits'] == 0 and rec['lse_bits'] == 0, (tag, rec)
    assert rec['missing'] == 0 and rec['stray'] == 0, (tag, rec)
    assert rec['skip_written'] == 0 and rec['skip_others'] == 0, (tag, rec)


def test_attn_fwd_ragged_refuses_long_clips(ops):
    qkv = torch.zeros(300 * 3, 3 * 64, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match='256'):
        RE.run_attn(ops, qkv, [257], 3, 2, 0.17, tab=np.array([[0, 257]], dtype=np.int32), max_len=257)


# ------------------------------------------------------------------------------------------------ the embedding
@pytest.mark.parametrize('C', [512, 72], ids=['rows_kernel', 'generic_kernel'])       # the two kernels mbx_embed_fwd chooses between
def test_embed_ragged_equals_the_per_clip_calls(ops, C):
    from motionbert_amd.augment import FLIP_PERM
    lens, Jn, Din, n_temp = RE.EMBED_LENS, 17, 3, 243
    inp = {k: v.to(DEV) for k, v in RE.embed_inputs(lens, Jn, Din, C, n_temp, 50 + C).items()}
    ft = torch.from_numpy(RE.tables(lens)[1]).to(DEV)
    perm = torch.tensor(FLIP_PERM, dtype=torch.int32, device=DEV)
    F = sum(lens)
    h, h2 = nan(F * Jn, C), nan(2 * F * Jn, C)
    ops.embed_fwd_ragged(inp['x'], inp['w'], inp['b'], inp['pos'], inp['temp'], ft, h, F, Jn)
    ops.embed_fwd_tta_ragged(inp['x'], perm, inp['w'], inp['b'], inp['pos'], inp['temp'], ft, h2, F, Jn)
    want, want2 = nan(F * Jn, C), nan(2 * F * Jn, C)
    for r0, r1, L in RE.rows_of(lens, Jn):
        xc = inp['x'][r0 // Jn:r1 // Jn].contiguous()
        ops.embed_fwd(xc, inp['w'], inp['b'], inp['pos'], inp['temp'], want[r0:r1], 1, L, Jn)
        both = nan(2 * L * Jn, C)
        ops.embed_fwd_tta(xc, perm, inp['w'], inp['b'], inp['pos'], inp['temp'], both, 1, L, Jn)
        want2[r0:r1], want2[F * Jn + r0:F * Jn + r1] = both[:L * Jn], both[L * Jn:]
    torch.cuda.synchronize()
    e = RE.embed_check(h.cpu(), {k: v.cpu() for k, v in inp.items()}, ft.cpu())
    rec = dict(bits=int((bits(h) != bits(want)).sum()), tta_bits=int((bits(h2) != bits(want2)).sum()), nan=int(torch.isnan(h).sum() + torch.isnan(h2).sum()),
               f64_share=e['ratio'])
    print(f'embed.C{C}', rec)
    REPORT[f'embed.C{C}'] = rec
    assert rec['bits'] == 0 and rec['tta_bits'] == 0 and rec['nan'] == 0 and e['ratio'] <= 1.0, rec


# ------------------------------------------------------------------------------------------------ the model
def _long_tiny():
    zt, cfg = load_golden('tiny_trained')
    m = build_model(dict(cfg, maxlen=256))
    sd = {k[2:]: torch.from_numpy(zt[k]) for k in zt.files if k.startswith('w.')}
    temp = torch.randn(1, 256, 1, cfg['dim_feat'], generator=torch.Generator().manual_seed(77)) * 0.02
    temp[:, :cfg['maxlen']] = sd['temp_embed']
    sd['temp_embed'] = temp
    m.load_state_dict(sd, strict=True)
    m.precision = 'fp32'
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def model():
    return _long_tiny()


@pytest.fixture(scope='module')
def per_clip(model):
    """x [F,17,3] and the per-clip fp32 references, computed once: model(x[None]) and flip_tta(model, x[None]) clip by clip"""
    from motionbert_amd.augment import flip_tta
    lens = RE.MODEL_LENS
    x = make_input(1, sum(lens), 17, 60)[0].to(DEV)
    plain, tta, at = [], [], 0
    with torch.no_grad():
        for L in lens:
            xc = x[at:at + L][None].contiguous()
            plain.append(model(xc)[0]), tta.append(flip_tta(model, xc)[0])
            at += L
    return x, torch.cat(plain), torch.cat(tta)


def test_forward_ragged_fp32(model, per_clip):
    from motionbert_amd.augment import flip_tta
    x, plain, tta = per_clip
    with torch.no_grad():
        got = model.forward_ragged(x, RE.MODEL_LENS)
        rep = model.forward_ragged(x, RE.MODEL_LENS, return_rep=True)
    got_t = flip_tta(model, x, clip_lens=RE.MODEL_LENS)
    assert got.shape == plain.shape == (sum(RE.MODEL_LENS), 17, 3) and rep.shape == (sum(RE.MODEL_LENS), 17, 64) and float(plain.std()) > 1e-3
    rec = dict(plain=float((got - plain).abs().max()) / GATE, tta=float((got_t - tta).abs().max()) / GATE)
    print('model.fp32', rec)
    REPORT['model.fp32'] = rec
    assert rec['plain'] <= 1.0 and rec['tta'] <= 1.0, rec
    got[:, 0, :] = 0                                                       # callers write into it (infer_wild.py:82)
    with pytest.raises(RuntimeError, match='inference'):
        model.forward_ragged(x, RE.MODEL_LENS)                             # not under no_grad


def _bf16_case(tag, m, x, lens):
    with torch.no_grad():
        m.precision = 'fp32'
        ref = m.forward_ragged(x, lens)
        m.precision = 'bf16'
        got = m.forward_ragged(x, lens)
        clips, at = [], 0
        for L in lens:
            clips.append(m(x[at:at + L][None].contiguous())[0])
            at += L
        m.precision = 'fp32'
    rec = dict(vs_fp32=rel_l2(got.cpu().numpy(), ref.cpu().numpy()) / TOL_BF16_OUT, vs_per_clip_recorded=float((got - torch.cat(clips)).abs().max()))
    print(tag, rec)
    REPORT[tag] = rec
    assert np.isfinite(got.cpu().numpy()).all() and rec['vs_fp32'] <= 1.0, rec


def test_forward_ragged_bf16(model, per_clip):
    _bf16_case('model.bf16.tiny', model, per_clip[0], RE.MODEL_LENS)


def test_forward_ragged_bf16_no_grad_sequencing():
    """dim_feat 256: the row-owner qkv and the fused MLP of the no-grad path run on the F J rows of a ragged batch"""
    cfg = dict(dim_in=3, dim_out=3, dim_feat=256, dim_rep=64, depth=1, num_heads=8, mlp_ratio=4, num_joints=17, maxlen=256)
    m = build_model(cfg, seed=1)
    trained_like(m, 2)
    lens = [243, 33, 1]
    _bf16_case('model.bf16.c256', m.to(DEV).eval(), make_input(1, sum(lens), 17, 61)[0].to(DEV), lens)


# ------------------------------------------------------------------------------------------------ wild.infer
class Recorder:
    """the model, with its network calls counted"""

    def __init__(self, model):
        self.model, self.num_joints, self.maxlen, self.calls = model, model.num_joints, model.maxlen, []

    def parameters(self):
        return self.model.parameters()

    def eval(self):
        self.model.eval()
        return self

    def forward(self, x, return_rep=False):
        self.calls.append(tuple(x.shape))
        return self.model.forward(x, return_rep=return_rep)

    __call__ = forward

    def forward_ragged(self, x, clip_lens, return_rep=False, tables=None):
        self.calls.append(tuple(clip_lens))
        return self.model.forward_ragged(x, clip_lens, return_rep=return_rep, tables=tables)


@pytest.fixture(scope='module')
def crowd():
    return {k: WE.detections(n, 8800 + k) for k, n in enumerate(RE.TRACK_LENS)}


@pytest.mark.parametrize('flip,pixel', [(False, False), (False, True), (True, False), (True, True)])
def test_infer_ragged_with_the_real_model(model, crowd, flip, pixel):
    from motionbert_amd import wild
    L, mb = 243, 2
    tag = f'infer.flip{int(flip)}.pixel{int(pixel)}'
    rec = Recorder(model)
    got = wild.infer(rec, crowd, clip_len=L, vid_size=VID, pixel=pixel, flip=flip, max_batch=mb, batching='ragged')
    total = sum(RE.TRACK_LENS)
    assert len(rec.calls) == math.ceil(total / (mb * L)) == 3 and sum(sum(c) for c in rec.calls) == total      # not one call per distinct length
    same = wild.infer(model, crowd, clip_len=L, vid_size=VID, pixel=pixel, flip=flip, max_batch=mb, batching='equal')
    gate = GATE * (min(VID) / 2.0 if pixel else 1.0)
    worst_loop = worst_equal = 0.0
    for k, kp in crowd.items():
        motion = WE.input_ref(kp, VID if pixel else None, None if pixel else [1, 1])[0]
        want = WE.reference_loop(model, motion, L, flip, False, False, False, VID if pixel else None, device=DEV)
        assert got[k].shape == want.shape == (len(kp), 17, 3) and got[k].dtype == np.float32 and np.isfinite(got[k]).all()
        worst_loop = max(worst_loop, float(np.abs(got[k].astype(np.float64) - want.astype(np.float64)).max()))
        worst_equal = max(worst_equal, float(np.abs(got[k].astype(np.float64) - same[k].astype(np.float64)).max()))
    REPORT[tag] = dict(loop_share=worst_loop / gate, equal_share=worst_equal / gate, calls=len(rec.calls))
    print(tag, REPORT[tag])
    assert worst_loop <= gate and worst_equal <= gate, (tag, worst_loop, worst_equal, gate)


def test_wild_output_ragged_equals_the_restatement_bit_for_bit(ops):
    worst = 0
    for kw in (dict(), dict(rootrel=True), dict(gt_2d=True, xc=2), dict(vid_size=VID), dict(gt_2d=True, vid_size=(720, 1280))):
        res = RE.run_output(ops, DEV, RE.output_case([243, 100, 1, 33, 9], [343, 1, 42], 70, **kw))
        worst = max(worst, res['out'])
        assert res == dict(out=0, pred_kept=True), (kw, res)
    REPORT['output'] = dict(differing=worst)
