"""The crowd rasteriser on a real MI355X (mbx_scene_project and mbx_scene_raster in csrc/scene.hip, motionbert_amd.render / .video): the gates
of tests/sceneerr.py (its own checks on the CPU: tests/test_sceneerr.py, tests/test_scene.py) applied to the kernels.

Gates.  Projected integers, prim_id and rgb: equal bits with the host reference; there is no tolerance.  Every output is sentinel-filled
beforehand (two different sentinels in two runs) and must be written everywhere; guard rows behind each buffer must be untouched; two runs and a
frame on its own give the bits of the whole.  Reduction (a): one person per frame on a square white image is mbx_skeleton_raster itself, on the
device.  Reduction (b): a crowd is the host reference's single-person pictures painted over the background in list order.  What was measured goes
to scene_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from motionbert_amd import video as V
from tests import jpegerr as J
from tests import sceneerr as SC
from tests import skelerr as SE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = SC.CHUNK
GUARD_ROWS = 2
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'scene_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'scene_parity.txt'), 'w') as f:
        f.write('crowd rasteriser against the host reference.  `failed`: gate messages (0 passes).  jq / prim_id / rgb are gated on equal bits.\n'
                '`covered`: share of samples inside a primitive; `prims_seen`: ids that win a sample; `most`: the longest list of a frame;\n'
                '`values`: projected integers; `dropped`: joints that project to the sentinel.\n')
        for k in sorted(REPORT):
            f.write(f'{k:34s} ' + '  '.join(f'{n} {v:.4g}' if isinstance(v, float) else f'{n} {v}' for n, v in sorted(REPORT[k].items())) + '\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def _guarded(shape, dtype, fill):
    """a sentinel-filled tensor of `shape` with GUARD_ROWS more leading rows behind it: (view, whole)"""
    whole = torch.full((shape[0] + GUARD_ROWS,) + tuple(shape[1:]), fill, dtype=dtype, device=DEV)
    return whole[:shape[0]], whole


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raster(ops, jq, table, bones, palette, radii, W, H, ss, background, fills=(7, -77)):
    """mbx_scene_raster on numpy inputs into sentinel-filled, guarded buffers -> dict of numpy arrays; asserts the guards"""
    Fv = len(table[0]) - 1
    rgb, rgb_all = _guarded((Fv, H, W, 3), torch.uint8, fills[0])
    pid, pid_all = _guarded((Fv, H * ss, W * ss), torch.int32, fills[1])
    bg = _dev(background) if isinstance(background, np.ndarray) else background
    ops.scene_raster(_dev(np.asarray(jq, np.int32)), *(_dev(np.asarray(t, np.int32)) for t in table), _dev(np.asarray(bones, np.int32)),
                     _dev(np.asarray(palette, np.uint8)), radii, W, H, ss, bg, rgb, pid)
    torch.cuda.synchronize()
    assert (rgb_all[Fv:] == fills[0]).all() and (pid_all[Fv:] == fills[1]).all(), 'guard rows were written'
    return dict(rgb=rgb.cpu().numpy(), prim_id=pid.cpu().numpy())


def _check(ops, name, jq, table, bones, palette, radii, W, H, ss, background):
    """gates, every element written (two sentinel values), run-to-run bits, a frame on its own, reduction (b)"""
    args = (jq, table, bones, palette, radii, W, H, ss)
    ref = SC.raster(*args, background)
    got = _raster(ops, *args, background)
    rep = {}
    failed = SC.gate_all(got, ref, rep)
    again = _raster(ops, *args, background, fills=(9, -99))                  # an element left unwritten keeps a different sentinel each time
    for k in got:
        if not np.array_equal(got[k], again[k]):
            failed.append(f'{k}: two runs differ (or an element is not written)')
    ptr = np.asarray(table[0])
    for f in range(len(ptr) - 1):
        bg = background[f:f + 1] if isinstance(background, np.ndarray) and background.shape[0] > 1 else background
        one = _raster(ops, jq, (ptr[f:f + 2], table[1], table[2]), bones, palette, radii, W, H, ss, bg)
        for k in got:
            if not np.array_equal(got[k][f:f + 1], one[k]):
                failed.append(f'{k}: frame {f} on its own differs from the whole')
    failed += SC.reduction_b(got, *args, background)
    cut = np.clip(ptr, 0, len(table[1]))                                     # as the kernel cuts them
    REPORT[name] = dict(rep, failed=len(failed), most=int(np.maximum(np.diff(cut), 0).max()) if len(ptr) > 1 else 0)
    assert not failed, failed
    return got, ref


# ------------------------------------------------------------------------------------------------ the projection
def test_projection_bits(ops):
    """pixel coordinates in and around a 1920 x 1080 frame with NaN, infinities, halves, negatives and joints at and beyond the guard, with and
    without a z column"""
    g = np.random.default_rng(3)
    x = g.uniform(-300, 2300, (23, 17, 3)).astype(np.float32)
    x[0, :9, 0] = [np.nan, np.inf, -np.inf, 8192.0, 8192.0625, -8192.0, 16384.0, 16384.03125, 1e30]
    x[1, :6, 1] = [0.5, -0.5, 0.46875, -0.03125, 1079.96875, np.nan]
    x[2, :, 2] = np.nan                                                      # z is not read
    R_, J_ = x.shape[:2]
    for ss in (1, 2):
        for cols in (3, 2):
            src = np.ascontiguousarray(x[..., :cols])
            ref = SC.project(src, ss)
            assert (ref[0, [0, 1, 2, 8]] == SC.OUTSIDE).all() and (ref[0, 7, 0] == SC.OUTSIDE) and (ref[2] != SC.OUTSIDE).all()
            assert (ref[0, 4, 0] == SC.OUTSIDE) == (ss == 2) and ref[0, 3, 0] == 8192 * 16 * ss and (ref[1, 5] == SC.OUTSIDE).all()
            tx, outs = _dev(src), []
            for fill in (-5, -6):
                out, whole = _guarded((R_, J_, 2), torch.int32, fill)
                ops.scene_project(tx, ss, out)
                torch.cuda.synchronize()
                assert (whole[R_:] == fill).all(), 'guard rows were written'
                outs.append(out.cpu().numpy())
            failed = SC.gate_equal('jq', outs[0], ref) + SC.gate_equal('jq (second run)', outs[1], ref)
            for r in (0, R_ - 1):
                one, _ = _guarded((1, J_, 2), torch.int32, -7)
                ops.scene_project(tx[r:r + 1].contiguous(), ss, one)
                failed += SC.gate_equal(f'jq of row {r} alone', one.cpu().numpy(), ref[r:r + 1])
            REPORT[f'project.ss{ss}.c{cols}'] = dict(failed=len(failed), values=int(ref.size), dropped=int((ref[..., 0] == SC.OUTSIDE).sum()))
            assert not failed, failed


# ------------------------------------------------------------------------------------------------ crowds around the chunk capacity
@pytest.mark.parametrize('ss', [1, 2])
@pytest.mark.parametrize('W,H', [(72, 40), (40, 72)])
def test_crowd(ops, W, H, ss):
    """lists of 0, 1, C and C + 1 persons in four frames over the video's own frames, then of 2 C + 1, 0 and 1 in three frames over one frame
    and over a colour; the long lists carry the crafted entries of sceneerr.crafted_case (outside, across a tile corner, sentinel joints, twins, a marker
    that only touches a tile, entries that name no row or no palette row)"""
    case = SC.crafted_case(W, H, ss, counts=(0, 1, C, C + 1))
    assert np.diff(case['table'][0]).tolist() == [0, 1, C, C + 1]
    args = (case['jq'], case['table'], case['bones'], case['palette'], case['radii'], W, H, ss)
    got, ref = _check(ops, f'crowd.{W}x{H}.ss{ss}.frames', *args, SC.backdrop(4, W, H, seed=ss))
    np_, n0 = 3 * len(SC.BONES5), case['R'] - 6
    for f in (2, 3):
        mine = case['table'][1][case['table'][0][f]:case['table'][0][f + 1]].tolist()
        seen = set((np.unique(got['prim_id'][f][got['prim_id'][f] >= 0]) // np_).tolist())
        assert mine.index(n0 + 4) in seen and mine.index(n0 + 3) not in seen and mine.index(n0) not in seen      # twins; outside
        assert {mine.index(n0 + 1), mine.index(n0 + 2), mine.index(n0 + 5)} <= seen
        assert not {k for k, r in enumerate(mine) if not 0 <= r < case['R']} & seen
    assert (got['prim_id'][0] == -1).all() and max(seen) >= C                # the second chunk of the last frame is seen
    many = SC.crafted_case(W, H, ss, counts=(2 * C + 1, 0, 1), seed=9)
    assert np.diff(many['table'][0]).tolist() == [2 * C + 1, 0, 1]
    args = (many['jq'], many['table'], many['bones'], many['palette'], many['radii'], W, H, ss)
    got, _ = _check(ops, f'crowd.{W}x{H}.ss{ss}.one_frame', *args, SC.backdrop(1, W, H, seed=5))
    assert got['prim_id'][0].max() // np_ >= 2 * C                           # the third chunk
    _check(ops, f'crowd.{W}x{H}.ss{ss}.colour', *args, (30, 90, 200))
    # one palette row: everybody in it
    _check(ops, f'crowd.{W}x{H}.ss{ss}.one_row', many['jq'], many['table'], many['bones'], many['palette'][:1], many['radii'], W, H, ss, (0, 0, 0))


def test_empty_tables(ops):
    """no rows at all, and a table without entries: every pixel is background"""
    W, H = 72, 40
    bg = SC.backdrop(2, W, H)
    none = (np.zeros(3, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    for name, jq in (('no_rows', np.zeros((0, 17, 2), np.int32)), ('no_entries', SC.project(SC.crowd_pixels((2,), W, H)[0], 1))):
        got, _ = _check(ops, f'empty.{name}', jq, none, SC.BONES5, R.track_palette(2, SC.BONES5), (16, 32, 8), W, H, 2, bg)
        assert (got['prim_id'] == -1).all() and np.array_equal(got['rgb'], bg)
    # a table whose pointers do not describe its entries is cut to them
    jq = SC.project(SC.crowd_pixels((3,), W, H, seed=2)[0], 1)
    wild = (np.array([-5, 2, 1, 99], np.int32), np.array([0, 1, 2], np.int32), np.array([0, 1, 0], np.int32))
    _check(ops, 'empty.wild_pointers', jq, wild, SC.BONES5, R.track_palette(2, SC.BONES5), (16, 32, 8), W, H, 1, (5, 6, 7))


# ------------------------------------------------------------------------------------------------ reduction (a), on the device
@pytest.mark.parametrize('ss', [1, 2])
def test_one_person_per_frame_is_the_skeleton_kernel(ops, ss):
    """a square scene with the identity table and white: mbx_skeleton_raster on the same jq, bit for bit"""
    size = 72

    def skeleton(jq, bones, colors, radii, size, ss):
        rgb = torch.full((jq.shape[0], size, size, 3), 3, dtype=torch.uint8, device=DEV)
        pid = torch.full((jq.shape[0], size * ss, size * ss), -3, dtype=torch.int32, device=DEV)
        ops.skeleton_raster(_dev(jq), _dev(np.asarray(bones, np.int32)), _dev(np.asarray(colors, np.uint8)), radii, size, ss, rgb, pid)
        return dict(rgb=rgb.cpu().numpy(), prim_id=pid.cpu().numpy())

    scene = lambda *a: _raster(ops, *a)      # noqa: E731
    jq = SE.project(SE.walking(3, seed=4), R.SKELETON_VIEW, size * ss)
    failed = SC.reduction_a(scene, jq, np.array(R.SKELETON_BONES, np.int32), np.array(R.SKELETON_COLORS, np.uint8),
                            tuple(ss * r for r in R.skeleton_radii(256)), size, ss, skeleton_fn=skeleton)
    for name, (jq, bones, colors, radii) in SE.crafted_cases(size, ss).items():
        failed += [f'{name}: {m}' for m in SC.reduction_a(scene, jq, bones, colors, radii, size, ss, skeleton_fn=skeleton)]
    REPORT[f'reduction_a.ss{ss}'] = dict(failed=len(failed), cases=1 + len(SE.crafted_cases(size, ss)))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ through the API
def _tracks(W, H, seed=0):
    """three tracks that enter and leave over four video frames, in pixels, as wild.infer(pixel=True) gives them"""
    g = np.random.default_rng(seed)
    ids = {3: np.array([0, 1, 2, 3]), 8: np.array([1, 2]), 1: np.array([0, 3])}
    x3d = {}
    for n, (k, v) in enumerate(ids.items()):
        at = np.array([W * (0.3 + 0.2 * n), H * 0.55, 0.0])
        x3d[k] = np.stack([at + [0.02 * W * t, 0, 0] + 0.4 * H * SE.POSE + g.normal(0, 0.2, SE.POSE.shape) for t in v]).astype(np.float32)
    return x3d, ids


@pytest.mark.parametrize('W,H,ss', [(72, 40, 2), (37, 21, 1), (1920, 1080, 1)])
def test_render_scene_and_chunks(ops, W, H, ss):
    """the dict of tracks through render_scene, a palette row per person, the video's frames behind them; 37 x 21: rows that are no whole
    number of dwords; 1920 x 1080: the size of the README's crowd"""
    x3d, ids = _tracks(W, H)
    table, palette, bg = R.scene_table(ids), R.track_palette(3), SC.backdrop(4, W, H, seed=1)
    got = R.render_scene(x3d, table, W, H, ss=ss, palette=palette, background=bg, want=('rgb', 'prim_id', 'jq'))
    torch.cuda.synchronize()
    jq = SC.project(np.concatenate(list(x3d.values())), ss)
    failed = SC.gate_equal('jq', got['jq'].cpu().numpy(), jq)
    rep = {}
    ref = SC.raster(jq, table, R.SKELETON_BONES, palette, R.skeleton_radii(min(W, H), ss), W, H, ss, bg)
    failed += SC.gate_all({k: got[k].cpu().numpy() for k in ('rgb', 'prim_id')}, ref, rep)
    REPORT[f'api.{W}x{H}.ss{ss}'] = dict(rep, failed=len(failed), most=int(np.diff(table[0]).max()))
    assert not failed, failed
    assert [set((np.unique(p[p >= 0]) // 48).tolist()) for p in ref['prim_id']] == [{0, 1}] * 4      # two persons in every frame, both seen
    chunks = [p.copy() for p in R.scene_chunks(x3d, table, W, H, ss=ss, palette=palette, background=bg, chunk=3)]
    assert [p.shape[0] for p in chunks] == [3, 1] and np.array_equal(np.concatenate(chunks), ref['rgb'])


def test_scene_video(ops, tmp_path):
    """the file's JPEG frames are video.encode_jpeg of the rendered frames, byte for byte"""
    W, H = 72, 40
    x3d, ids = _tracks(W, H, seed=2)
    table, palette, bg = R.scene_table(ids), R.track_palette(3), _dev(SC.backdrop(4, W, H, seed=6))
    path = str(tmp_path / 'crowd.avi')
    assert V.scene_video(path, x3d, table, W, H, 25, quality=80, background=bg, chunk=3, palette=palette) == (4, os.path.getsize(path))
    rgb = R.render_scene(x3d, table, W, H, palette=palette, background=bg)['rgb']
    files = V.frames_to_host(*V.encode_jpeg(rgb, 80, '420'))
    assert J.avi_frames(open(path, 'rb').read()) == files and len(files) == 4
    assert (rgb.cpu().numpy() != bg.cpu().numpy()).any()
    REPORT['video.72x40'] = dict(failed=0, frames=4, bytes=os.path.getsize(path))
