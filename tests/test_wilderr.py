"""tests/wilderr.py on the CPU: its float64 restatement of the input stage against the reference's own code (tests/golden/wild.npz,
tools/mint_wild.py) bit for bit, `wild.clip_plan` against the clip shapes of the reference's WildDetDataset, `wild.read_alphapose`
against the seeded JSON files, and every seeded corruption of the numpy stand-in provider against the gates (each must fail at least one).
No kernel runs here; the argument checks of the two C entry points come before any launch and are exercised without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from motionbert_amd import wild
from tests import wilderr as WE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fixture():
    return WE.load_fixture()


@pytest.fixture(scope='module')
def cases():
    return WE.input_cases()


def test_chunk_size_is_one_number():
    header = open(os.path.join(ROOT, 'include', 'mbx.h')).read()
    assert int(re.search(r'#define MBX_WILD_CHUNK (\d+)', header).group(1)) == wild.CHUNK_FRAMES == WE.CHUNK
    assert (wild.PIXEL, wild.CROP, wild.ROOTREL, wild.GT_2D, wild.OUT_PIXEL) == (WE.PIXEL, WE.CROP, WE.ROOTREL, WE.GT_2D, WE.OUT_PIXEL)


def test_fixture_covers_every_case(fixture, cases):
    assert sorted(fixture.files) == sorted(f'in.{n}.{k}' for n in cases for k in ('out', 'clips', 'box'))
    C = WE.CHUNK
    for F in (C - 1, C, C + 1, 2 * C + 1):
        for plant in WE.PLANTS:
            assert fixture[f'in.chunk.{F}.{plant}.out'].shape == (F, 17, 3)
    # the planted cases do what their names say
    assert not fixture['in.valid3.out'].any() and fixture['in.valid3.box'].tolist() == [0, 0, 0, 3]
    assert fixture['in.valid4.out'].any() and fixture['in.valid4.box'][3] == 4
    assert not fixture['in.coincident.out'].any() and fixture['in.coincident.box'].tolist() == [0, 0, 0, 5]
    assert fixture['in.neck_hip_0.box'][3] == 5 * 17 - 2 * 3
    assert fixture['in.conf_gt1.crop.out'][..., 2].max() == 1.0 and fixture['in.conf_gt1.pixel.out'][..., 2].max() == 1.75
    assert fixture['in.conf_gt1.pixel.out'][0, 7, 2] == 1.125
    for F in (C - 1, 2 * C + 1):        # the undetected joint lies outside the box of the rest: clipped, and the box is not the planted one
        out = fixture[f'in.chunk.{F}.invalid.out']
        assert out[F // 2, 13].tolist() == [-1.0, 1.0, 0.0] and fixture[f'in.chunk.{F}.invalid.box'][0] > 500


def test_restatement_equals_the_reference_bit_for_bit(fixture, cases):
    for name, case in cases.items():
        out, box = WE.input_ref(WE.case_kp(case), case['vid_size'], case['scale_range'])
        assert WE.differing(out, fixture[f'in.{name}.out']) == 0, name
        assert WE.differing(box.reshape(4), fixture[f'in.{name}.box']) == 0, name


def test_clip_plan_equals_the_reference_clips(fixture, cases):
    for name in cases:
        F = fixture[f'in.{name}.out'].shape[0]
        plan = wild.clip_plan([F], WE.CLIP_LEN)
        clips = sorted((o, T) for T, offs in plan for o in offs)
        assert [T for _, T in clips] == fixture[f'in.{name}.clips'].tolist(), name
        assert [o for o, _ in clips] == [i * WE.CLIP_LEN for i in range(len(clips))], name


def test_clip_plan_pools_tracks():
    L = 9
    plan = wild.clip_plan([5, 18, 10, 0, 14, 9], L)
    assert plan == [(9, [5, 14, 23, 33, 47]), (5, [0, 42]), (1, [32])]
    covered = sorted(f for T, offs in plan for o in offs for f in range(o, o + T))
    assert covered == list(range(56))
    assert wild.clip_plan([4], L) == [(4, [0])] and wild.clip_plan([0], L) == []
    with pytest.raises(ValueError):
        wild.clip_plan([], L)
    with pytest.raises(ValueError):
        wild.clip_plan([3], 0)
    with pytest.raises(ValueError):
        wild.clip_plan([-1], L)


def test_chunk_table():
    C = wild.CHUNK_FRAMES
    tab, ptr = wild.chunk_table([C + 1, 0, 3, 2 * C])
    assert tab.dtype == np.int32 and ptr.dtype == np.int32
    assert tab.tolist() == [[0, 0, C], [0, C, 1], [2, C + 1, 3], [3, C + 4, C], [3, 2 * C + 4, C]] and ptr.tolist() == [0, 2, 2, 3, 5]


def test_read_alphapose(tmp_path, cases):
    its, keys = WE.persons_cases()
    path = WE.write_json(str(tmp_path / 'persons.json'), its)
    tracks = wild.read_alphapose(path, by_track=True)
    assert list(tracks) == keys == [3, 7, 1] and [len(v) for v in tracks.values()] == list(WE.PERSON_LENS.values())
    for k in keys:
        want = WE.case_kp(cases[f'persons.crop.focus{k}'])
        got = wild.read_alphapose(path, focus=k)
        assert got.dtype == np.float64 and got.shape == (WE.PERSON_LENS[k], 26, 3)
        assert WE.differing(got, want) == 0 and WE.differing(tracks[k], want) == 0
    everything = wild.read_alphapose(path)
    assert everything.shape == (sum(WE.PERSON_LENS.values()), 26, 3)
    assert WE.differing(everything[:3], np.stack([tracks[k][0] for k in keys])) == 0          # file order
    with pytest.raises(ValueError, match='no detections'):
        wild.read_alphapose(path, focus=99)
    bad = [dict(it) for it in its[:2]]
    bad[1]['keypoints'] = bad[1]['keypoints'][:51]
    with pytest.raises(ValueError, match='17 joints'):
        wild.read_alphapose(WE.write_json(str(tmp_path / 'coco.json'), bad))
    bad = [dict(it) for it in its[:2]]
    bad[0]['keypoints'] = [float('nan')] + bad[0]['keypoints'][1:]
    with pytest.raises(ValueError, match='non-finite'):
        wild.read_alphapose(WE.write_json(str(tmp_path / 'nan.json'), bad))
    with pytest.raises(ValueError, match='no detections'):
        wild.read_alphapose(WE.write_json(str(tmp_path / 'empty.json'), []))


# ------------------------------------------------------------------------------------------------ the gates on the stand-in
def _input_results(ops, fixture, cases):
    return {n: WE.input_check(ops, 'cpu', c, fixture[f'in.{n}.out'], fixture[f'in.{n}.box']) for n, c in cases.items()}


def test_stand_in_passes_every_gate(fixture, cases):
    ops = WE.NumpyWildOps()
    for name, res in _input_results(ops, fixture, cases).items():
        assert WE.passes(res), (name, res)
    for name, case in WE.output_cases().items():
        res = WE.output_check(ops, 'cpu', case)
        assert res == dict(out=0, clean=True, pred_kept=True), (name, res)


@pytest.mark.parametrize('corrupt', WE.INPUT_CORRUPTIONS)
def test_input_corruptions_fail_a_gate(fixture, cases, corrupt):
    failed = [n for n, res in _input_results(WE.NumpyWildOps(corrupt), fixture, cases).items() if not WE.passes(res)]
    print(corrupt, 'fails', failed)
    assert failed, f'{corrupt}: no case noticed'
    if corrupt == 'float32':        # fractional detections: float32 arithmetic is visible in the crop AND in the pixel mode
        assert any('pixel' in n for n in failed) and any(n.startswith('chunk.') for n in failed)
    if corrupt == 'threshold_le4':
        assert failed == ['valid4']
    if corrupt in ('wh_swapped', 'max_wh'):
        assert all(cases[n]['vid_size'] for n in failed)


@pytest.mark.parametrize('corrupt', WE.OUTPUT_CORRUPTIONS)
def test_output_corruptions_fail_a_gate(corrupt):
    ops = WE.NumpyWildOps(corrupt)
    failed = [n for n, case in WE.output_cases().items() if WE.output_check(ops, 'cpu', case)['out']]
    print(corrupt, 'fails', failed)
    assert failed, f'{corrupt}: no case noticed'
    if corrupt == 'gt2d_wrong_clip':
        assert all('gt2d' in n or n == 'big' for n in failed)


def test_multi_track_stand_in_equals_the_focus_cases(fixture):
    """three interleaved persons as ONE call with seq_lens: every track gets its own box"""
    its, keys = WE.persons_cases()
    tracks = WE.case_kp(dict(items=its, focus=None), by_track=True)
    kp, lens = np.concatenate(list(tracks.values())), [len(v) for v in tracks.values()]
    for mode, vid, rng in (('crop', None, [1, 1]), ('pixel', (1920, 1080), None)):
        y, box = wild.wild_input(kp, vid_size=vid, scale_range=rng, seq_lens=lens, return_box=True, ops=WE.NumpyWildOps())
        assert y.dtype == torch.float32 and tuple(y.shape) == (sum(lens), 17, 3) and tuple(box.shape) == (3, 4)
        want = np.concatenate([fixture[f'in.persons.{mode}.focus{k}.out'] for k in keys])
        assert WE.differing(y.numpy(), want) == 0
        assert WE.differing(box.numpy(), np.stack([fixture[f'in.persons.{mode}.focus{k}.box'] for k in keys])) == 0


# ------------------------------------------------------------------------------------------------ the C entry points refuse bad arguments
def test_arguments_are_refused_before_any_launch():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 150
    p = 4096       # stands for a non-null, aligned pointer: every call below is refused before it is used

    def inp(kp=p, tab=p, n_chunks=1, ptr=p, S=1, F=4, hw=960.0, hh=540.0, ps=540.0, ratio=1.0, flags=3, channels=3, y=p, box=None, ws=p, ws_bytes=1 << 20):
        return lib.mbx_wild_input(kp, tab, n_chunks, ptr, S, F, hw, hh, ps, ratio, flags, channels, y, box, ws, ws_bytes, None)

    def outp(pred=p, x=p, xc=3, dst=p, n=1, T=9, flags=0, out=p):
        return lib.mbx_wild_output(pred, x, xc, dst, n, T, flags, 540.0, 960.0, 540.0, out, None)

    assert inp(F=0) == 0 and outp(n=0) == 0                                     # no-ops
    C = wild.CHUNK_FRAMES
    for what, call, word in [('null kp', lambda: inp(kp=None), b'null'), ('null y', lambda: inp(y=None), b'null'), ('null ws', lambda: inp(ws=None), b'null'),
                             ('no track', lambda: inp(S=0), b'bad sizes'), ('no chunk', lambda: inp(n_chunks=0), b'bad sizes'),
                             ('more chunks than frames', lambda: inp(n_chunks=5), b'chunks'), ('negative F', lambda: inp(F=-1), b'frame count'),
                             ('too many chunks', lambda: inp(F=4 * C, n_chunks=7), b'chunks'), ('no mode', lambda: inp(flags=0), b'flags'),
                             ('unknown flag', lambda: inp(flags=4), b'flags'), ('one channel', lambda: inp(channels=1), b'channels'),
                             ('pixel scale 0', lambda: inp(ps=0.0), b'pixel mode'), ('ratio nan', lambda: inp(ratio=float('nan')), b'ratio'),
                             ('odd ws', lambda: inp(ws=p + 4), b'aligned'), ('small ws', lambda: inp(ws_bytes=16), b'workspace'),
                             ('null pred', lambda: outp(pred=None), b'null'), ('null out', lambda: outp(out=None), b'null'),
                             ('T = 0', lambda: outp(T=0), b'bad shape'), ('unknown flag', lambda: outp(flags=8), b'flags'),
                             ('gt_2d without x', lambda: outp(flags=2, x=None), b'gt_2d'), ('gt_2d with one channel', lambda: outp(flags=2, xc=1), b'gt_2d')]:
        rc = call()
        assert rc != 0 and word in lib.mbx_last_error(), (what, rc, lib.mbx_last_error())
    assert lib.mbx_wild_input_ws(0, 1) > 0 and lib.mbx_wild_input_ws(2 * C + 1, 3) >= ((2 + 3 + 1) * 5 + 3 * 4) * 8
