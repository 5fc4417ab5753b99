"""Restatements, inputs and gates for ragged batches: clips of different lengths in one inference forward (csrc/attention.hip
`attn_fwd_ragged_kernel`, csrc/elementwise.hip `embed_fwd_ragged_kernel`, csrc/wild.hip `wild_output_ragged_kernel`,
`Engine.forward(ragged=)`, `DSTformer.forward_ragged`, `wild.infer(batching='ragged')`).  Plain module, no fixtures:
tests/test_gpu_ragged.py applies it to the kernels on the GPU, tests/test_raggederr.py to seeded corruptions on the CPU,
tests/test_ragged.py runs the host side on the CPU stand-ins.

  attn_ref / embed_ref        float64: temporal attention per clip -- the softmax of a query runs over the keys of ITS clip only -- and
                              the embedding with the temporal row temp[index of the frame inside its clip]
  output_eq_ragged            infer_wild.py:81-88 for a packed batch, in numpy: z of joint 0 is zeroed at frame 0 of every clip
  RaggedMockOps               oracle.torch_ops.MockOps + the four ragged provider entries in torch (+ flip_average, which the flip form
                              of the engine needs and MockOps lacks), with seeded corruptions
  RaggedWildOps / RaggedNet   wilderr's numpy provider + wild_output_ragged, and its element-wise network + a forward_ragged that loops
                              over the clips
  attn_check / embed_check / output_check / model_check   the gates

Gates.  The ragged kernels add no arithmetic: a problem of length L is the per-clip call's problem, so the GPU gate is EQUAL BITS with
the per-clip calls (tests/test_gpu_ragged.py).  The checks here decide against float64 instead, so that they can see a restatement
that is wrong in the same way on both sides:
  attention   fp32 operands, fp32 arithmetic: a score carries hd products, the row sum L terms, exp and log a few ulp each; a row of o is
              within ATTN_ROW (hd + L) 2^-24 of the exact row in relative L2, lse within the same share of max(1, |lse|).  bf16 on the
              GPU goes through the per-row gate of tests/localerr.py (2 x the rounding model, per unit) instead.
  embedding   Din + 3 fp32 operations per element: |h - exact| <= (Din + 3) 2^-24 (|x| |w| + |b| + |pos| + |temp|) per element.
  output      single IEEE operations in a fixed order: equal bits.
  model       the ragged forward against the per-clip forwards through the same provider: equal bits on the CPU (every kernel of
              MockOps is row-wise or per clip).
Every output is filled with a sentinel (NaN) first: a row inside the table that stays NaN and a row outside it that does not both fail."""
import math

import numpy as np
import torch

from motionbert_amd.engine import MODE_TEMPORAL
from oracle.augment_oracle import flip_data
from oracle.torch_ops import MockOps
from tests import localerr as LE
from tests import wilderr as WE

J = 17
U = 2.0 ** -24
ATTN_ROW = 64.0                 # see the module docstring
SHARED_LENS = [1, 17, 32, 33, 64, 100, 243, 256]      # max_len > 32: one workgroup per problem; 1 / 32 / 33 / 256 are the fragment edges
PRIVATE_LENS = [1, 5, 32, 17, 9]                      # max_len <= 32: one problem per wave; with J = 3, H = 2: 30 problems, not a multiple of 4
EMBED_LENS = [1, 2, 33, 243]
MODEL_LENS = [243, 100, 33, 32, 1]
TRACK_LENS = [500, 243, 130, 77, 33, 1]
CORRUPTIONS = ('global_t', 'neighbour_keys', 'last_key_masked', 'frag_off_by_one', 'lse_wrong_row', 'z_track_starts', 'z_every_frame',
               'tta_unshifted', 'clip_skipped')


def tables(clip_lens):
    """(clip_tab [n,2] int32, frame_t [F] int32) on the host"""
    from motionbert_amd.model import ragged_tables
    tab, ft, _ = ragged_tables(clip_lens)
    return tab, ft


def rows_of(clip_lens, Jn=J):
    """[(first token row, end token row, frames)] per clip"""
    out, at = [], 0
    for L in clip_lens:
        out.append((at * Jn, (at + L) * Jn, L))
        at += L
    return out


# ------------------------------------------------------------------------------------------------ float64 restatements
def attn_ref(qkv, clip_lens, Jn, H, scale, model=False):
    """(o [M,C], lse [M,H]) in float64: clip after clip `localerr.attn_fwd_ref` (temporal) on the clip's own rows.  model=True: with the
    bf16 roundings of attn_fwd_kernel."""
    o, l = [], []
    for r0, r1, L in rows_of(clip_lens, Jn):
        a, b = LE.attn_fwd_ref(qkv[r0:r1], 1, L, Jn, H, scale, True, model)
        o.append(a), l.append(b)
    return torch.cat(o), torch.cat(l)


def embed_ref(x, w, b, pos, temp, frame_t):
    """(h [F J,C] float64, per-element bound): x [F,J,Din], w [C,Din], b [C], pos [J,C], temp [n_temp,C], frame_t [F]"""
    x, w, b, pos, temp = (t.double() for t in (x, w, b, pos, temp))
    F, Jn, Din = x.shape
    tt = temp[frame_t.long()][:, None, :]
    h = x @ w.t() + b + pos[None] + tt
    amp = x.abs() @ w.abs().t() + b.abs() + pos.abs()[None] + tt.abs()
    return h.reshape(F * Jn, -1), ((Din + 3) * U * amp).reshape(F * Jn, -1)


def output_eq_ragged(pred, x, frame_t, rootrel, gt_2d, corrupt=None, track_start=None):
    """infer_wild.py:81-88 for a packed batch pred [Fb,17,3] float32 (a copy is returned): the loop of the reference sees one clip per
    iteration, so `[:, 0, 0, 2] = 0` lands on frame 0 of EVERY clip -- the frames with frame_t == 0.  track_start [Fb] bool: the frames
    that open a track (the 'z_track_starts' corruption zeroes only those)."""
    p = np.array(pred, dtype=np.float32, copy=True)
    ft = np.asarray(frame_t)
    if rootrel:
        p[:, 0, :] = 0                                      # :82
    elif corrupt == 'z_track_starts':
        p[np.asarray(track_start, dtype=bool), 0, 2] = 0
    elif corrupt == 'z_every_frame':
        p[:, 0, 2] = 0
    else:
        p[ft == 0, 0, 2] = 0                                # :84
    if gt_2d:
        p[..., :2] = x[..., :2]                             # :87
    return p


# ------------------------------------------------------------------------------------------------ the provider in torch
class RaggedMockOps(MockOps):
    """MockOps + the ragged entries of HipOps, same argument lists.  Every entry is the per-clip restatement: attention calls
    MockOps.attn_fwd on each clip's rows, so the bits are those of the per-clip forward.  `corrupt`: one of CORRUPTIONS."""

    def __init__(self, corrupt=None):
        super().__init__()
        assert corrupt is None or corrupt in CORRUPTIONS
        self.corrupt = corrupt

    def attn_fwd_ragged(self, qkv, o, lse, clip_tab, n_clips, F, max_len, Jn, H, scale):
        self._log('attn_fwd_ragged')
        assert clip_tab.dtype == torch.int32 and qkv.shape[0] == F * Jn and 1 <= max_len <= 256
        tab = clip_tab.reshape(-1, 2)[:n_clips].tolist()
        c = self.corrupt
        for i, (first, L) in enumerate(tab):
            if c == 'tta_unshifted' and i >= n_clips // 2 and n_clips % 2 == 0 and first >= F // 2:
                first -= F // 2                                              # the doubled batch read through the table of the first half
            if c == 'clip_skipped' and i == n_clips - 1:
                continue
            if first < 0 or L < 1 or L > max_len or first + L > F:
                continue                                                     # a row that cannot be trusted is skipped
            r0, r1 = first * Jn, (first + L) * Jn
            if c in ('neighbour_keys', 'last_key_masked', 'frag_off_by_one'):
                self._attn_corrupt(qkv, o, lse, first, L, F, Jn, H, scale)
                continue
            self.attn_fwd(qkv[r0:r1], o[r0:r1], lse[r0:r1], 1, L, Jn, H, scale, MODE_TEMPORAL)
        if c == 'lse_wrong_row':
            lse.copy_(torch.roll(lse, 1, 0))

    def _attn_corrupt(self, qkv, o, lse, first, L, F, Jn, H, scale):
        """one clip with the wrong set of keys: 'neighbour_keys' sees up to 4 frames of the clip that follows, 'last_key_masked' loses its
        last key, 'frag_off_by_one' loses key 32 (the first key of the second 32-key fragment)"""
        c = self.corrupt
        extra = min(4, F - first - L) if c == 'neighbour_keys' else 0
        Lk = L + extra
        q, k, v = self._split(qkv[first * Jn:(first + Lk) * Jn], 1, Lk, Jn, H)
        s = torch.einsum('bsjhd,btjhd->bjhst', q[:, :L], k) * scale
        if c == 'last_key_masked' and L > 1:
            s[..., L - 1] = -math.inf
        if c == 'frag_off_by_one' and L > 32:
            s[..., 32] = -math.inf
        l = torch.logsumexp(s, -1)
        oo = torch.einsum('bjhst,btjhd->bsjhd', torch.exp(s - l[..., None]), v)
        r0, r1 = first * Jn, (first + L) * Jn
        o[r0:r1] = oo.reshape(L * Jn, -1).to(o.dtype)
        lse[r0:r1] = l.permute(0, 3, 1, 2).reshape(L * Jn, H)

    def _embed(self, x, perm, w, b, pos, temp, frame_t, h, F, Jn):
        assert frame_t.dtype == torch.int32 and frame_t.numel() == F
        t = frame_t.long()
        if self.corrupt == 'global_t':
            t = torch.arange(F).clamp_max(temp.numel() // h.shape[-1] - 1)   # the row of the batch instead of the frame of the clip
        tt = temp.reshape(-1, h.shape[-1])[t][:, None, :]
        x3 = x.reshape(F, Jn, -1)
        views = [x3] if perm is None else [x3, flip_data(x3)]
        y = torch.cat([(v @ w.t() + b + pos.reshape(1, Jn, -1)) + tt for v in views])
        h.copy_(y.reshape(h.shape))

    def embed_fwd_ragged(self, x, w, b, pos, temp, frame_t, h, F, Jn):
        self._log('embed_fwd_ragged')
        self._embed(x, None, w, b, pos, temp, frame_t, h, F, Jn)

    def embed_fwd_tta_ragged(self, x, perm, w, b, pos, temp, frame_t, h, F, Jn):
        self._log('embed_fwd_tta_ragged')
        self._embed(x, perm, w, b, pos, temp, frame_t, h, F, Jn)

    def flip_average(self, out2, perm, out):
        self._log('flip_average')
        B = out.shape[0]
        out.copy_((out2[:B] + flip_data(out2[B:])) / 2.0)

    def wild_output_ragged(self, pred, x, frame_t, dst0, flags, pix_scale, half_w, half_h, out, track_start=None):
        self._log('wild_output_ragged')
        assert pred.dtype == torch.float32 and out.dtype == torch.float32 and frame_t.dtype == torch.int32
        Fb = pred.shape[0]
        assert frame_t.numel() == Fb and 0 <= dst0 <= out.shape[0] - Fb
        p = output_eq_ragged(pred.numpy(), None if x is None else x.numpy(), frame_t.numpy(), bool(flags & WE.ROOTREL), bool(flags & WE.GT_2D),
                             self.corrupt, track_start)
        if flags & WE.OUT_PIXEL:                                # infer_wild.py:95-96 with the constants as the kernel gets them
            p = p * np.float32(pix_scale)
            p[..., :2] = p[..., :2] + np.array([half_w, half_h])
        out[dst0:dst0 + Fb] = torch.from_numpy(p)


class RaggedWildOps(WE.NumpyWildOps):
    """wilderr.NumpyWildOps + wild_output_ragged"""

    def wild_output_ragged(self, pred, x, frame_t, dst0, flags, pix_scale, half_w, half_h, out):
        self.calls.append(('wild_output_ragged', tuple(pred.shape), int(flags), int(dst0)))
        RaggedMockOps().wild_output_ragged(pred, x, frame_t, dst0, flags, pix_scale, half_w, half_h, out)


class RaggedNet(WE.FixedNet):
    """wilderr.FixedNet + forward_ragged: the clips one at a time, batch 1, through the same element-wise function"""

    def forward_ragged(self, x, clip_lens, return_rep=False, tables=None):
        assert x.dim() == 3 and sum(clip_lens) == x.shape[0] and tables is not None
        tab, ft = tables
        assert tab.dtype == torch.int32 and tab.shape == (len(clip_lens), 2) and tab[:, 1].tolist() == list(clip_lens) and ft.numel() == x.shape[0]
        assert tab[:, 0].tolist() == [sum(clip_lens[:i]) for i in range(len(clip_lens))]
        tta = return_rep == 'flip_tta'
        self.calls.append((('tta',) if tta else ()) + ('ragged', tuple(clip_lens), x.shape[2]))
        outs, at = [], 0
        for L in clip_lens:
            xi = x[at:at + L][None]
            outs.append(((self._f(xi) + flip_data(self._f(flip_data(xi)))) / 2.0 if tta else self._f(xi))[0])
            at += L
        return torch.cat(outs)


# ------------------------------------------------------------------------------------------------ seeded inputs
def attn_inputs(clip_lens, Jn, H, hd, seed, dtype=torch.float32, pad=2):
    """qkv [(F + pad) Jn, 3C] with a scale of its own per q row (no two rows share a maximum), `pad` frames behind the last clip that no
    table row names"""
    g = torch.Generator().manual_seed(seed)
    M, C = (sum(clip_lens) + pad) * Jn, H * hd
    qkv = torch.randn(M, 3 * C, generator=g)
    qkv[:, :C] *= 1.0 + 0.5 * torch.randn(M, 1, generator=g).abs().clamp_max(2.0)
    return qkv.to(dtype)


def embed_inputs(clip_lens, Jn, Din, C, n_temp, seed):
    g = torch.Generator().manual_seed(seed)
    F = sum(clip_lens)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k
    return dict(x=r(F, Jn, Din), w=r(C, Din, k=0.3), b=r(C, k=0.1), pos=r(Jn, C, k=0.02), temp=r(n_temp, C, k=0.02))


def output_case(clip_lens, track_lens, seed, xc=3, rootrel=False, gt_2d=False, vid_size=None):
    """a packed batch for wild_output_ragged: dict(pred [Fb,17,3], x [Fb,17,xc], frame_t, track_start, dst0, F, ...)"""
    r = np.random.RandomState(seed)
    Fb = sum(clip_lens)
    assert sum(track_lens) == Fb
    start = np.zeros(Fb, dtype=bool)
    start[np.cumsum([0] + list(track_lens[:-1]))] = True
    return dict(pred=r.normal(0, 0.4, (Fb, 17, 3)).astype(np.float32), x=r.uniform(-1, 1, (Fb, 17, xc)).astype(np.float32), frame_t=tables(clip_lens)[1],
                track_start=start, dst0=5, F=Fb + 9, rootrel=rootrel, gt_2d=gt_2d, vid_size=vid_size)


def output_ref(case):
    p = output_eq_ragged(case['pred'], case['x'], case['frame_t'], case['rootrel'], case['gt_2d'])
    out = np.full((case['F'], 17, 3), np.nan, dtype=np.float32)
    out[case['dst0']:case['dst0'] + len(p)] = p
    return WE.pixel_eq(out, case['vid_size']) if case['vid_size'] else out


# ------------------------------------------------------------------------------------------------ the gates
def run_attn(ops, qkv, clip_lens, Jn, H, scale, tab=None, max_len=None):
    """ops.attn_fwd_ragged into NaN-filled o / lse -> (o, lse) on the device of qkv"""
    M, C = qkv.shape[0], qkv.shape[1] // 3
    o = torch.full((M, C), math.nan, dtype=qkv.dtype, device=qkv.device)
    lse = torch.full((M, H), math.nan, dtype=torch.float32, device=qkv.device)
    tab = torch.from_numpy(tables(clip_lens)[0] if tab is None else tab).to(qkv.device)
    ops.attn_fwd_ragged(qkv, o, lse, tab, tab.shape[0], M // Jn, max_len or max(clip_lens), Jn, H, scale)
    return o, lse


def attn_check(o, lse, qkv, clip_lens, Jn, H, scale):
    """fp32 case: dict(row = worst row error of o as a share of its gate, lse = the same for lse, missing = rows inside the table still
    NaN, stray = rows outside it that were written)"""
    hd = qkv.shape[1] // 3 // H
    ex_o, ex_l = attn_ref(qkv, clip_lens, Jn, H, scale)
    n = ex_o.shape[0]
    oo, ll = o[:n].double(), lse[:n].double()
    missing = int((torch.isnan(oo).any(1) | torch.isnan(ll).any(1)).sum())
    stray = int((~torch.isnan(o[n:].double())).any(1).sum() + (~torch.isnan(lse[n:])).any(1).sum())
    gate = torch.cat([torch.full((r1 - r0,), ATTN_ROW * (hd + L) * U, dtype=torch.float64) for r0, r1, L in rows_of(clip_lens, Jn)]).to(oo.device)
    oo, ll = torch.nan_to_num(oo, nan=1e30), torch.nan_to_num(ll, nan=1e30)
    row = ((oo - ex_o).norm(dim=1) / ex_o.norm(dim=1).clamp_min(1e-300)) / gate
    el = ((ll - ex_l).abs() / ex_l.abs().clamp_min(1.0)).amax(1) / gate
    return dict(row=float(row.max()), lse=float(el.max()), missing=missing, stray=stray)


def attn_passes(res):
    return res['row'] <= 1.0 and res['lse'] <= 1.0 and res['missing'] == 0 and res['stray'] == 0


def embed_check(h, inp, frame_t):
    """dict(ratio = worst |h - exact| / bound, nan)"""
    ex, bound = embed_ref(inp['x'], inp['w'], inp['b'], inp['pos'], inp['temp'], frame_t)
    hh = h.double().reshape(ex.shape)
    return dict(ratio=float(((torch.nan_to_num(hh, nan=1e30) - ex).abs() / bound.clamp_min(1e-300)).max()), nan=int(torch.isnan(hh).sum()))


def run_output(ops, device, case, **kw):
    """ops.wild_output_ragged into a NaN-filled [F,17,3] -> differing elements against the restatement (rows outside the batch must stay NaN)"""
    buf = torch.full((case['F'], 17, 3), math.nan, dtype=torch.float32, device=device)
    hw, hh, ps = WE.consts(case['vid_size'])
    flags = (WE.ROOTREL if case['rootrel'] else 0) | (WE.GT_2D if case['gt_2d'] else 0) | (WE.OUT_PIXEL if case['vid_size'] else 0)
    pred = torch.from_numpy(case['pred']).to(device)
    ops.wild_output_ragged(pred, torch.from_numpy(case['x']).to(device) if case['gt_2d'] else None, torch.from_numpy(case['frame_t']).to(device), case['dst0'],
                           flags, ps, hw, hh, buf, **kw)
    return dict(out=WE.differing(buf.cpu().numpy(), output_ref(case)), pred_kept=WE.differing(pred.cpu().numpy(), case['pred']) == 0)


def model_check(got, want):
    """elements of the ragged forward whose bits differ from the concatenated per-clip forwards (NaN counts)"""
    return WE.differing(got.detach().cpu().numpy(), want.detach().cpu().numpy())
