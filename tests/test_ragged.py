"""Ragged batches on the CPU: the plan (`wild.ragged_plan`), the argument checks of `DSTformer.forward_ragged`, `wild.infer(batching=
'ragged')` on the stand-ins of tests/raggederr.py against `batching='equal'` bit for bit over the switch combinations of
tests/test_wild.py, and the symbols of the library."""
import itertools
import math

import numpy as np
import pytest
import torch

from motionbert_amd import wild
from tests import raggederr as RE
from tests import wilderr as WE
from tests.helpers import build_model

L = WE.CLIP_LEN
VID = (1920, 1080)


def _dataset_clips(seq_lens, clip_len):
    """(first row, frames) of every clip in the order `WildDetDataset` yields them (dataset_wild.py:94-102), track after track"""
    out, start = [], 0
    for n in seq_lens:
        for index in range(math.ceil(n / clip_len)):
            st, end = index * clip_len, min((index + 1) * clip_len, n)
            out.append((start + st, end - st))
        start += n
    return out


@pytest.mark.parametrize('seq_lens,clip_len,max_frames', [([500, 243, 130, 77, 33, 1], 243, 243 * 4), ([500, 243, 130, 77, 33, 1], 243, 243),
                                                           ([5, 0, 31, 9, 9, 1, 1, 1], 9, 27), ([1], 9, 9), ([0, 0], 9, 9), ([100], 7, 20),
                                                           (list(np.random.RandomState(5).randint(20, 401, 30)), 243, 243 * 64)])
def test_ragged_plan_properties(seq_lens, clip_len, max_frames):
    plan = wild.ragged_plan(seq_lens, clip_len, max_frames)
    clips = [(row0 + sum(cl[:i]), c) for row0, cl in plan for i, c in enumerate(cl)]
    assert clips == _dataset_clips(seq_lens, clip_len)                                   # the reference's clips in its order: none spans a track
    seen = np.zeros(sum(seq_lens), dtype=np.int64)
    for f0, c in clips:
        seen[f0:f0 + c] += 1
    assert (seen == 1).all()                                                             # every frame exactly once
    ends = np.cumsum(seq_lens)
    for f0, c in clips:
        t = int(np.searchsorted(ends, f0, side='right'))
        assert 1 <= c <= clip_len and f0 + c <= ends[t]
    at = 0
    for row0, cl in plan:
        assert row0 == at and cl and sum(cl) <= max_frames
        at += sum(cl)
    # greedy: a batch is closed only when the next clip does not fit
    for (_, a), (_, b) in zip(plan, plan[1:]):
        assert sum(a) + b[0] > max_frames
    assert len(plan) >= math.ceil(sum(seq_lens) / max_frames)


def test_ragged_plan_argument_errors():
    with pytest.raises(ValueError, match='max_frames'):
        wild.ragged_plan([10], 9, 8)
    with pytest.raises(ValueError, match='clip_len'):
        wild.ragged_plan([10], 0, 8)
    with pytest.raises(ValueError, match='seq_lens'):
        wild.ragged_plan([], 9, 9)


def test_ragged_tables():
    from motionbert_amd.model import ragged_tables
    tab, ft, mx = ragged_tables([3, 1, 4])
    assert tab.dtype == np.int32 and tab.tolist() == [[0, 3], [3, 1], [4, 4]] and ft.dtype == np.int32 and ft.tolist() == [0, 1, 2, 0, 0, 1, 2, 3] and mx == 4
    for bad in ([], [0], [3, -1], [257], [2.5], ['a'], None):
        with pytest.raises(ValueError, match='clip_lens'):
            ragged_tables(bad)
    with pytest.raises(ValueError, match='clip_lens'):
        ragged_tables([17], maxlen=16)
    assert ragged_tables([256])[2] == 256


def test_forward_ragged_argument_errors():
    m = build_model(dict(dim_in=3, dim_out=3, dim_feat=64, dim_rep=64, depth=1, num_heads=2, mlp_ratio=2, num_joints=17, maxlen=16)).eval()
    x = torch.zeros(10, 17, 3)
    with torch.no_grad():
        with pytest.raises(ValueError, match='ragged batch'):
            m.forward_ragged(x[None], [10])
        with pytest.raises(ValueError, match='ragged batch'):
            m.forward_ragged(x[:, :16], [10])
        for bad in ([], [0, 10], [17], [5, 5.5]):
            with pytest.raises(ValueError, match='clip_lens'):
                m.forward_ragged(torch.zeros(17, 17, 3), bad)
        with pytest.raises(ValueError, match='sum to'):
            m.forward_ragged(x, [4, 5])
        with pytest.raises(RuntimeError, match='no CPU path'):
            m.forward_ragged(x, [4, 6])
    from motionbert_amd.augment import flip_tta
    with pytest.raises(ValueError, match='sum to'):
        flip_tta(m, x, clip_lens=[3])
    big = build_model(dict(dim_in=3, dim_out=3, dim_feat=64, dim_rep=64, depth=1, num_heads=2, mlp_ratio=2, num_joints=17, maxlen=300)).eval()
    with torch.no_grad(), pytest.raises(ValueError, match='256'):
        big.forward_ragged(torch.zeros(257, 17, 3), [257])                               # beyond the resident attention kernels, whatever maxlen says


TRACKS = (L - 4, 2 * L, L + 1, 1, 3)


@pytest.fixture(scope='module')
def tracks():
    return {k: WE.detections(n, 8700 + k) for k, n in enumerate(TRACKS)}


@pytest.mark.parametrize('flip,rootrel,gt_2d,no_conf,pixel', list(itertools.product((False, True), repeat=5)))
def test_ragged_infer_equals_equal_length_batching(tracks, flip, rootrel, gt_2d, no_conf, pixel):
    kw = dict(clip_len=L, vid_size=VID if pixel else None, pixel=pixel, flip=flip, rootrel=rootrel, gt_2d=gt_2d, no_conf=no_conf)
    want = wild.infer(RE.RaggedNet(), tracks, max_batch=64, ops=RE.RaggedWildOps(), **kw)
    for mb in (1, 2, 64):
        net, ops = RE.RaggedNet(), RE.RaggedWildOps()
        got = wild.infer(net, tracks, max_batch=mb, batching='ragged', ops=ops, **kw)
        assert list(got) == list(tracks)
        for k in tracks:
            assert got[k].dtype == np.float32 and WE.differing(got[k], want[k]) == 0, (k, mb)
        plan = wild.ragged_plan(TRACKS, L, mb * L)
        xc = 2 if no_conf else 3
        assert net.evals == 1 and net.calls == [(('tta',) if flip else ()) + ('ragged', tuple(cl), xc) for _, cl in plan]
        assert len(plan) == {1: 5, 2: 3, 64: 1}[mb]                                      # [5] [9] [9] [9] [1 1 3]; [5 9] [9 9] [1 1 3]; one call for all
        assert [c[0] for c in ops.calls] == ['wild_input'] + ['wild_output_ragged'] * len(plan)
        assert [c[3] for c in ops.calls[1:]] == [row0 for row0, _ in plan]
    # one person, an array in and an array out
    one = wild.infer(RE.RaggedNet(), tracks[1], max_batch=2, batching='ragged', ops=RE.RaggedWildOps(), **kw)
    assert isinstance(one, np.ndarray) and WE.differing(one, wild.infer(WE.FixedNet(), tracks[1], max_batch=2, ops=WE.NumpyWildOps(), **kw)) == 0


def test_ragged_infer_batches_are_views_and_tables_go_up_once(tracks, monkeypatch):
    seen = []

    class Net(RE.RaggedNet):
        def forward_ragged(self, x, clip_lens, return_rep=False, tables=None):
            seen.append((x, tables))
            return super().forward_ragged(x, clip_lens, return_rep, tables)

    wild.infer(Net(), tracks, clip_len=L, max_batch=2, flip=False, batching='ragged', ops=RE.RaggedWildOps())
    base = seen[0][0].data_ptr()
    at = 0
    for x, (tab, ft) in seen:
        assert x.is_contiguous() and x.data_ptr() == base + at * 17 * 3 * 4              # no gather: the batch is a view of the input stage's output
        assert ft.data_ptr() == seen[0][1][1].data_ptr() + at * 4 and tab.untyped_storage().data_ptr() == ft.untyped_storage().data_ptr()      # one upload
        at += x.shape[0]
    assert at == sum(TRACKS)


def test_ragged_infer_argument_errors(tracks):
    ops = RE.RaggedWildOps()
    with pytest.raises(ValueError, match='256'):
        wild.infer(RE.RaggedNet(maxlen=300), tracks, clip_len=257, batching='ragged', ops=ops)
    with pytest.raises(ValueError, match='batching'):
        wild.infer(RE.RaggedNet(), tracks, clip_len=L, batching='padded', ops=ops)
    with pytest.raises(TypeError, match='forward_ragged'):
        wild.infer(WE.FixedNet(), tracks, clip_len=L, batching='ragged', ops=ops)
    # the default is the equal-length path
    net = RE.RaggedNet()
    wild.infer(net, tracks, clip_len=L, ops=ops)
    assert all('ragged' not in c for c in net.calls)


def test_library_symbols_and_version():
    from motionbert_amd import hip_ops
    lib = hip_ops.load_library()
    for name in ('mbx_attn_fwd_ragged', 'mbx_embed_fwd_ragged', 'mbx_embed_fwd_tta_ragged', 'mbx_wild_output_ragged'):
        assert name in hip_ops.SIGNATURES and getattr(lib, name) is not None
    assert lib.mbx_version() >= 190
    # refused on the host, before anything is launched: clips beyond the resident kernels, and a batch that does not fit its rows
    assert lib.mbx_attn_fwd_ragged(1, 1, 1, 1, 1, 300, 257, 17, 8, 64, 0.125, 0, None) != 0 and b'256' in lib.mbx_last_error()
    assert lib.mbx_wild_output_ragged(1, None, 0, 1, 5, 3, 7, 0, 1.0, 0.0, 0.0, 1, None) != 0 and b'does not fit' in lib.mbx_last_error()
    for m in ('attn_fwd_ragged', 'embed_fwd_ragged', 'embed_fwd_tta_ragged', 'wild_output_ragged'):
        assert callable(getattr(hip_ops.HipOps, m))
