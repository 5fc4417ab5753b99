"""The crowd path end to end on the CPU through the reference providers (tests/sceneerr.RefOps, tests/jpegerr.RefOps): the frame ids of
`wild.read_alphapose`, `render.scene_table`, `render.render_scene` / `scene_chunks`, `video.scene_video` with the AVI fields checked as
tests/test_video.py checks them, validation, and the C ABI's refusals."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest
import torch

import motionbert_amd
from motionbert_amd import render as R
from motionbert_amd import video as V
from motionbert_amd import wild
from tests import jpegerr as J
from tests import sceneerr as SC
from tests import skelerr as SE

W, H = 56, 40


class Ops(J.RefOps, SC.RefOps):
    """the JPEG reference and the scene reference as one provider"""

    def __init__(self):
        J.RefOps.__init__(self)
        SC.RefOps.__init__(self)


# ------------------------------------------------------------------------------------------------ frame ids
def _item(idx, image_id, seed):
    kp = np.random.default_rng(seed).uniform(0, 100, (26, 3)).round(2)
    item = {'idx': idx, 'keypoints': kp.reshape(-1).tolist()}
    if image_id is not None:
        item['image_id'] = image_id
    return item


def _write(tmp_path, items, name='det.json'):
    path = str(tmp_path / name)
    with open(path, 'w') as f:
        json.dump(items, f)
    return path


def test_read_alphapose_frame_ids(tmp_path):
    items = [_item(1, '0.jpg', 0), _item(2, 1, 1), _item(1, 'frames/000001.jpg', 2), _item(1, '3.png', 3), _item(2, 3, 4), _item(7, '17', 5)]
    path = _write(tmp_path, items)
    det, ids = wild.read_alphapose(path, by_track=True, frames=True)
    assert list(det) == [1, 2, 7] == list(ids)
    assert [v.tolist() for v in ids.values()] == [[0, 1, 3], [1, 3], [17]] and all(v.dtype == np.int64 for v in ids.values())
    assert [v.shape for v in det.values()] == [(3, 26, 3), (2, 26, 3), (1, 26, 3)]
    one, frames = wild.read_alphapose(path, focus=2, frames=True)
    assert frames.tolist() == [1, 3] and frames.dtype == np.int64 and np.array_equal(one, det[2])
    # frames=False is what it was: the same arrays, and image_id is not looked at
    plain = wild.read_alphapose(path, by_track=True)
    assert list(plain) == [1, 2, 7] and all(np.array_equal(plain[k], det[k]) for k in det)
    assert np.array_equal(wild.read_alphapose(path, focus=1), det[1])
    bare = _write(tmp_path, [_item(1, None, 0), _item(1, 'x.jpg', 2)], 'bare.json')
    assert wild.read_alphapose(bare).shape == (2, 26, 3)
    # refusals name the item
    for bad, n in (('x.jpg', 1), ('1.5.jpg', 1), (1.0, 1), (True, 1), (None, 1), ('-3.jpg', 1), ('', 1)):
        with pytest.raises(ValueError, match=f'item {n} has image_id'):
            wild.read_alphapose(_write(tmp_path, [_item(1, 0, 0), _item(1, bad, 1)], 'bad.json'), frames=True)
    for second in (4, 3):                                                    # a repeated frame, and one that goes back
        with pytest.raises(ValueError, match='item 2 is frame'):
            wild.read_alphapose(_write(tmp_path, [_item(1, 4, 0), _item(2, 4, 1), _item(1, second, 2)], 'rep.json'), by_track=True, frames=True)
    with pytest.raises(ValueError, match='item 1 is frame'):                 # without tracks the whole selection is one track
        wild.read_alphapose(_write(tmp_path, [_item(1, 4, 0), _item(2, 4, 1)], 'two.json'), frames=True)


# ------------------------------------------------------------------------------------------------ the scene table
def test_scene_table():
    ids = {5: np.array([0, 2, 3]), 9: np.array([2, 5]), 4: np.array([], np.int64)}
    ptr, rows, person = R.scene_table(ids)
    assert all(a.dtype == np.int32 for a in (ptr, rows, person))
    assert ptr.tolist() == [0, 1, 1, 3, 4, 4, 5] and rows.tolist() == [0, 1, 3, 2, 4] and person.tolist() == [0, 0, 1, 0, 1]      # frames 1 and 4: nobody
    assert [a.tolist() for a in R.scene_table(list(ids.values()))] == [ptr.tolist(), rows.tolist(), person.tolist()]
    ptr7, rows7, _ = R.scene_table(ids, n_frames=8)
    assert ptr7.tolist() == [0, 1, 1, 3, 4, 4, 5, 5, 5] and rows7.tolist() == rows.tolist()
    # order: ascending and stable inside a frame; frame 2 holds rows 1 and 3
    assert R.scene_table(ids, order=[0, 5, 0, 1, 0])[1].tolist() == [0, 3, 1, 2, 4]
    assert R.scene_table(ids, order=[0, 5, 0, 1, 0])[2].tolist() == [0, 1, 0, 0, 1]
    assert R.scene_table(ids, order=np.array([0, 1, 0, 1, 0], np.float32))[1].tolist() == rows.tolist()        # a tie keeps the track order
    empty = R.scene_table({})
    assert [a.tolist() for a in empty] == [[0], [], []] and R.scene_table([], n_frames=2)[0].tolist() == [0, 0, 0]
    for bad, match in ((dict(frame_ids=[np.array([0, -1])]), 'negative'), (dict(n_frames=5), 'n_frames'), (dict(n_frames=-1), 'n_frames'),
                       (dict(order=[0, 1]), 'order'), (dict(order=[0, 1, np.nan, 0, 0]), 'order'), (dict(order=['a'] * 5), 'order'),
                       (dict(frame_ids=[np.array([0.5])]), 'integer'), (dict(frame_ids=[np.zeros((2, 2), np.int64)]), '1-D')):
        kw = dict(frame_ids=ids)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            R.scene_table(**kw)


def test_scene_table_refuses_more_persons_than_the_id_holds(monkeypatch):
    assert R.MAX_PERSONS_PER_FRAME == 1 << 23 and R.MAX_PERSONS_PER_FRAME * 3 * R.MAX_BONES <= 2 ** 31
    monkeypatch.setattr(R, 'MAX_PERSONS_PER_FRAME', 3)
    crowd = [np.array([1])] * 3 + [np.array([0])]
    assert R.scene_table(crowd)[0].tolist() == [0, 1, 4]
    with pytest.raises(ValueError, match='4 persons in frame 1'):
        R.scene_table(crowd + [np.array([1])])


def test_track_palette():
    p = R.track_palette(1440)
    assert p.shape == (1440, 16, 3) and p.dtype == np.uint8 and len({r.tobytes() for r in p}) == 1440 and not (p == 255).all(-1).any()
    assert p[0, 6].tolist() == [235, 23, 23] and p[1, 6].tolist() == [23, 235, 83] and p[0, 0].tolist() == [235, 107, 107] and p[0, 3].tolist() == [141, 13, 13]
    assert all(len({tuple(c) for c in r.tolist()}) == 3 for r in p)          # left, right and middle differ
    assert R.track_palette(0).shape == (0, 16, 3) and R.track_palette(2, SC.BONES5).shape == (2, 5, 3)
    assert np.array_equal(R.track_palette(7), p[:7])
    for bad in (-1, 1441, 2.0):
        with pytest.raises(ValueError, match='track_palette'):
            R.track_palette(bad)


# ------------------------------------------------------------------------------------------------ the API
@pytest.fixture(scope='module')
def crowd():
    """three video frames, three tracks that enter and leave: pixel coordinates as wild.infer(pixel=True) gives them, z present and unused"""
    g = np.random.default_rng(5)
    ids = {3: np.array([0, 1, 2]), 8: np.array([1, 2]), 1: np.array([0, 2])}
    x3d = {}
    for n, (k, v) in enumerate(ids.items()):
        at = np.array([14 + 14 * n, 20, 0.0])
        x3d[k] = np.stack([at + [2 * t, 0, 0] + 22 * SE.POSE + g.normal(0, 0.2, SE.POSE.shape) for t in v]).astype(np.float32)
    return x3d, ids, R.scene_table(ids)


def _ref(x3d, table, ss=1, palette=None, background=(255, 255, 255), radii=None, width=W, height=H):
    jq = SC.project(np.concatenate(list(x3d.values())), ss)
    palette = np.array(R.SKELETON_COLORS, np.uint8)[None] if palette is None else palette
    return jq, SC.raster(jq, table, R.SKELETON_BONES, palette, radii or R.skeleton_radii(min(width, height), ss), width, height, ss, background)


def test_render_scene_matches_the_reference(crowd):
    x3d, ids, table = crowd
    ops = SC.RefOps()
    got = R.render_scene(x3d, table, W, H, ss=2, want=('rgb', 'prim_id', 'jq'), ops=ops)
    assert ops.calls == [('scene_project', 7), ('scene_raster', 3)]
    assert got['rgb'].shape == (3, H, W, 3) and got['rgb'].dtype == torch.uint8 and got['prim_id'].shape == (3, 2 * H, 2 * W) and got['jq'].shape == (7, 17, 2)
    jq, ref = _ref(x3d, table, ss=2)
    assert np.array_equal(got['jq'].numpy(), jq) and not SC.gate_all({k: got[k].numpy() for k in ('rgb', 'prim_id')}, ref)
    # everybody is seen in the frames they are in, and nowhere else
    seen = [set((np.unique(ref['prim_id'][f][ref['prim_id'][f] >= 0]) // 48).tolist()) for f in range(3)]
    assert seen == [{0, 1}, {0, 1}, {0, 1, 2}]
    # a palette row per person, the video's frames behind them, `out`, a device tensor for x3d and for the table
    palette, bg = R.track_palette(3), SC.backdrop(3, W, H)
    out = torch.zeros(3, H, W, 3, dtype=torch.uint8)
    x = torch.from_numpy(np.concatenate(list(x3d.values())))
    res = R.render_scene(x[..., :2].contiguous(), tuple(torch.from_numpy(t) for t in table), W, H, palette=palette, background=bg, out=out, ops=SC.RefOps())
    _, ref = _ref(x3d, table, palette=palette, background=bg)
    assert set(res) == {'rgb'} and res['rgb'] is out and np.array_equal(out.numpy(), ref['rgb'])
    assert (out.numpy()[ref['prim_id'] < 0] == bg[ref['prim_id'] < 0]).all()
    colours = {tuple(c) for c in out.numpy()[ref['prim_id'] >= 0].tolist()}
    assert colours <= {tuple(c) for c in palette.reshape(-1, 3).tolist()} | {(255, 255, 255)} and len(colours) >= 7
    one_bg = R.render_scene(x3d, table, W, H, background=torch.from_numpy(bg[1:2]), radii=(20, 30, 10), ops=SC.RefOps())['rgb'].numpy()
    assert np.array_equal(one_bg, _ref(x3d, table, background=bg[1:2], radii=(20, 30, 10))[1]['rgb'])
    tall = R.render_scene(x3d, table, H, W, background=(1, 2, 3), ops=SC.RefOps())['rgb']
    assert tall.shape == (3, W, H, 3) and np.array_equal(tall.numpy(), _ref(x3d, table, background=(1, 2, 3), width=H, height=W)[1]['rgb'])
    # `order` changes who is on top, not who is there
    flipped = R.scene_table(ids, order=-np.arange(7.0))
    thick = (24, 40, 12)
    a, b = _ref(x3d, table, palette=palette, radii=thick)[1], _ref(x3d, flipped, palette=palette, radii=thick)[1]
    assert np.array_equal(a['prim_id'] >= 0, b['prim_id'] >= 0) and not np.array_equal(a['rgb'], b['rgb'])
    assert np.array_equal(R.render_scene(x3d, flipped, W, H, palette=palette, radii=thick, ops=SC.RefOps())['rgb'].numpy(), b['rgb'])


def test_chunks_equal_the_whole(crowd):
    x3d, _, table = crowd
    bg = SC.backdrop(3, W, H, seed=2)
    whole = R.render_scene(x3d, table, W, H, background=bg, ops=SC.RefOps())['rgb'].numpy()
    for chunk in (1, 2, 3, 32):
        ops = SC.RefOps()
        parts = [p.copy() for p in R.scene_chunks(x3d, table, W, H, background=bg, chunk=chunk, ops=ops)]
        assert [p.shape for p in parts] == [(min(chunk, 3 - a), H, W, 3) for a in range(0, 3, chunk)]
        assert np.array_equal(np.concatenate(parts), whole), chunk               # the background frames are sliced with the chunk
        assert ops.calls == [('scene_project', 7)] + [('scene_raster', p.shape[0]) for p in parts]
    assert list(R.scene_chunks(x3d, R.scene_table({}), W, H, ops=SC.RefOps())) == []


def test_no_frames_no_launch_and_no_persons_is_the_background(crowd):
    x3d, _, _ = crowd
    ops = SC.RefOps()
    got = R.render_scene(x3d, R.scene_table({}), W, H, ss=2, want=('rgb', 'prim_id'), ops=ops)
    assert got['rgb'].shape == (0, H, W, 3) and got['prim_id'].shape == (0, 2 * H, 2 * W) and not [c for c in ops.calls if c[0] == 'scene_raster']
    none = R.render_scene(torch.zeros(0, 17, 3), R.scene_table([], n_frames=2), W, H, background=(9, 8, 7), want=('rgb', 'prim_id'), ops=SC.RefOps())
    assert (none['prim_id'] == -1).all() and (none['rgb'].reshape(-1, 3) == torch.tensor([9, 8, 7], dtype=torch.uint8)).all()


def test_validation(crowd):
    x3d, _, table = crowd
    ops = SC.RefOps()
    x = torch.from_numpy(np.concatenate(list(x3d.values())))
    for bad, match in ((dict(x3d=x.double()), 'float32'), (dict(x3d=x[0]), 'x3d'), (dict(x3d=x[..., :1]), 'x3d'), (dict(x3d={}), 'dict'),
                       (dict(x3d={1: x3d[3], 2: x3d[3][:, :5]}), 'dict'), (dict(x3d=torch.zeros(2, 33, 3)), 'x3d'),
                       (dict(width=0), 'width'), (dict(height=2049), 'height'), (dict(width=64.0), 'width'), (dict(ss=3), 'ss'),
                       (dict(table=table[:2]), 'table'), (dict(table=(table[0].astype(np.int64), table[1], table[2])), 'frame_ptr'),
                       (dict(table=(table[0], table[1], table[2][:3])), 'table'), (dict(table=(table[0][:0], table[1], table[2])), 'table'),
                       (dict(bones=[(0, 1)]), 'palette'), (dict(palette=np.zeros((1, 15, 3), np.uint8)), 'palette'),
                       (dict(palette=np.full((1, 16, 3), 300)), 'palette'), (dict(palette=np.zeros((16, 3), np.uint8)), 'palette'),
                       (dict(radii=(1, 2)), 'radii'), (dict(radii=(1, 2, 3)), 'radii'), (dict(want=('depth',)), 'want'),
                       (dict(background=(1, 2)), 'background'), (dict(background=(1, 2, 256)), 'background'),
                       (dict(background=np.zeros((2, H, W, 3), np.uint8)), 'background'), (dict(background=np.zeros((3, W, H, 3), np.uint8)), 'background'),
                       (dict(background=torch.zeros(3, H, W, 3)), 'background'),
                       (dict(out=torch.zeros(3, H, W, 3)), 'out'), (dict(out=torch.zeros(3, W, H, 3, dtype=torch.uint8)), 'out')):
        kw = dict(x3d=x3d, table=table, width=W, height=H, ops=ops)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            R.render_scene(**kw)
    with pytest.raises(ValueError, match='chunk'):
        list(R.scene_chunks(x3d, table, W, H, chunk=0, ops=ops))
    assert ops.calls == []
    with pytest.raises(RuntimeError, match='ROCm device'):                   # host data without a provider: no CPU path
        R.render_scene(x, table, W, H)
    assert {'render_scene', 'scene_chunks', 'scene_table', 'track_palette', 'scene_video'} <= set(motionbert_amd.__all__)
    assert motionbert_amd.scene_video is V.scene_video and motionbert_amd.render_scene is R.render_scene
    assert R.SCENE_CHUNK == SC.CHUNK


# ------------------------------------------------------------------------------------------------ the file
def _fields(path):
    """the AVI's fixed fields, as tests/test_video.py reads them"""
    data = open(path, 'rb').read()
    top = J.riff(data)
    assert len(top) == 1 and top[0]['id'] == b'RIFF' and top[0]['form'] == b'AVI ' and top[0]['size'] == len(data) - 8
    hdrl, movi, idx1 = top[0]['chunks']
    assert (hdrl['id'], hdrl['form'], movi['id'], movi['form'], idx1['id']) == (b'LIST', b'hdrl', b'LIST', b'movi', b'idx1')
    avih, strl = hdrl['chunks']
    assert avih['id'] == b'avih' and avih['size'] == 56 and (strl['id'], strl['form']) == (b'LIST', b'strl')
    strh, strf = strl['chunks']
    assert (strh['id'], strh['size'], strf['id'], strf['size']) == (b'strh', 56, b'strf', 40)
    return data, struct.unpack('<14I', avih['data']), strh['data'], struct.unpack('<IiiHH4sIiiII', strf['data']), movi, idx1


def test_scene_video_end_to_end(tmp_path, crowd):
    x3d, _, table = crowd
    palette, bg = R.track_palette(3), SC.backdrop(3, W, H, seed=4)
    ops, path = Ops(), str(tmp_path / 'crowd.avi')
    assert V.scene_video(path, x3d, table, W, H, 25, quality=75, background=bg, chunk=2, palette=palette, ops=ops) == (3, os.path.getsize(path))
    assert [c for c in ops.calls if c[0] in ('scene_project', 'scene_raster', 'emit')] == \
        [('scene_project', 7), ('scene_raster', 2), ('scene_raster', 1), ('emit', 2), ('emit', 1)]
    rgb = R.render_scene(x3d, table, W, H, palette=palette, background=bg, ops=SC.RefOps())['rgb'].numpy()
    data, avih, strh, strf, movi, idx1 = _fields(path)
    files = [J.encode(f, 75, '420') for f in rgb]
    assert J.avi_frames(data) == files and [c['id'] for c in movi['chunks']] == [b'00dc'] * 3 and idx1['size'] == 48
    largest = max(len(f) for f in files)
    assert avih == (40000, sum(len(f) for f in files) * 25000 // 3000, 0, 0x10, 3, 0, 1, largest, W, H, 0, 0, 0, 0)
    assert strh[:8] == b'vidsMJPG' and struct.unpack('<IHHIIIIIIII4H', strh[8:]) == (0, 0, 0, 0, 1000, 25000, 0, 3, largest, 0xffffffff, 0, 0, 0, W, H)
    assert strf == (40, W, H, 1, 24, b'MJPG', W * H * 3, 0, 0, 0, 0)
    # the chunking does not show; 4:4:4 with a restart interval and ss = 2 over a colour
    other = str(tmp_path / 'other.avi')
    V.scene_video(other, x3d, table, W, H, 25, quality=75, background=torch.from_numpy(bg), chunk=3, palette=palette, ops=Ops())
    assert open(other, 'rb').read() == data
    V.scene_video(other, x3d, table, W, H, 30, subsampling='444', restart=2, background=(20, 30, 40), ss=2, ops=Ops())
    soft = R.render_scene(x3d, table, W, H, ss=2, background=(20, 30, 40), ops=SC.RefOps())['rgb'].numpy()
    assert J.avi_frames(open(other, 'rb').read()) == [J.encode(f, 90, '444', 2) for f in soft]
    assert V.scene_video(other, x3d, R.scene_table({}), W, H, 25, ops=Ops()) == (0, V.MJPEGWriter.HEADER + 8)
    for bad, match in ((dict(chunk=0), 'chunk'), (dict(quality=0), 'quality'), (dict(subsampling='411'), 'subsampling'), (dict(width=0), 'width')):
        with pytest.raises(ValueError, match=match):
            V.scene_video(str(tmp_path / 'never.avi'), x3d, table, **{**dict(width=W, height=H, fps=25, ops=Ops()), **bad})
    assert not os.path.exists(tmp_path / 'never.avi')


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_refuses_bad_arguments():
    """no launch is made: the checks come first"""
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 240
    p = lambda *a: lib.mbx_scene_project(None, *a, None, None)      # noqa: E731  (R, J, C, ss)
    assert p(1, 17, 4, 1) != 0 and b'C=4' in lib.mbx_last_error()
    assert p(1, 33, 3, 1) != 0 and b'J=33' in lib.mbx_last_error()
    assert p(-1, 17, 3, 1) != 0 and b'R=-1' in lib.mbx_last_error()
    assert p(1, 17, 3, 3) != 0 and b'ss' in lib.mbx_last_error()
    assert p(1, 17, 2, 1) != 0 and b'null' in lib.mbx_last_error()
    assert p(0, 17, 2, 2) == 0

    def r(Fv=1, R_=1, n=1, J_=17, Nb=16, P=1, radii=(1, 2, 1), W_=64, H_=48, ss=1, bg=None, bg_n=1, bg_rgb=0xffffff):
        return lib.mbx_scene_raster(None, None, None, None, n, None, None, Fv, R_, J_, Nb, P, *radii, W_, H_, ss, bg, bg_n, bg_rgb, None, None, None)
    fake = ctypes.c_void_p(4096)
    for kw, word in ((dict(Nb=0), b'Nb=0'), (dict(Nb=65), b'Nb=65'), (dict(J_=0), b'J=0'), (dict(P=0), b'P=0'), (dict(n=-1), b'entries=-1'),
                     (dict(Fv=-1), b'Fv=-1'), (dict(R_=(1 << 24) + 1), b'R='), (dict(radii=(2049, 2, 1)), b'radius'), (dict(radii=(1, 2, 3)), b'radius'),
                     (dict(W_=0), b'W=0'), (dict(H_=2049), b'H=2049'), (dict(ss=4), b'ss 4'), (dict(bg_rgb=1 << 24), b'background'),
                     (dict(bg_rgb=-1), b'background'), (dict(bg=fake, bg_n=2, Fv=3), b'background'), (dict(bg=fake, bg_n=0), b'background'),
                     (dict(), b'null')):
        assert r(**kw) != 0 and word in lib.mbx_last_error(), (kw, lib.mbx_last_error())
    assert r(Fv=0) == 0 and r(Fv=0, bg=fake, bg_n=1) == 0
    assert R.SCENE_CHUNK == 64 and 'define MBX_SCENE_CHUNK 64' in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                    'include', 'mbx.h')).read()
