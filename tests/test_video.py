"""motionbert_amd.video end to end on the CPU through the reference providers (tests/jpegerr.RefOps with the rasterisers' RefOps): encode_jpeg,
its refusals, the AVI container field by field, and the two *_video functions.  No AVI reader exists on the machines this is tested on: the
container is checked against its specification (RIFF / AVI 1.0), not played."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from motionbert_amd import video as V
from tests import jpegerr as J
from tests import rendererr as RE
from tests import skelerr as SE

SIZE = 40


class Ops(J.RefOps, SE.RefOps, RE.RefOps):
    """the JPEG reference and both rasteriser references as one provider"""


@pytest.fixture(scope='module')
def frames():
    return np.stack([J.content(k, 33, 17, seed=3) for k in ('noise', 'render', 'ramp')])


# ------------------------------------------------------------------------------------------------ encode_jpeg
def test_encode_jpeg_offsets_and_bytes(frames):
    ops = J.RefOps()
    data, off = V.encode_jpeg(torch.from_numpy(frames), 75, '420', 3, ops=ops)
    assert ops.calls == [('blocks', 3), ('sizes', 3), ('emit', 3)]
    assert data.dtype == torch.uint8 and off.dtype == torch.int64 and off.shape == (4,) and off[0] == 0 and off[3] == data.numel()
    files = [J.encode(f, 75, '420', 3) for f in frames]
    assert off.tolist() == [0] + list(np.cumsum([len(f) for f in files])) and V.frames_to_host(data, off) == files
    # the defaults: quality 90, 4:2:0, one MCU row per restart interval
    assert V.frames_to_host(*V.encode_jpeg(torch.from_numpy(frames), ops=J.RefOps())) == [J.encode(f, 90, '420', 2) for f in frames]
    assert J.parse(files[0], decode=False)['restart'] == 3 and V.geometry(33, 17, '420') == (2, 3, 6) == J.geometry(33, 17, '420')
    assert V.HEADER_BYTES == len(J.header(33, 17, 75, '420', 3))


def test_no_frames_no_launch(frames):
    ops = J.RefOps()
    data, off = V.encode_jpeg(torch.from_numpy(frames[:0]), ops=ops)
    assert ops.calls == [] and data.shape == (0,) and data.dtype == torch.uint8 and off.tolist() == [0] and V.frames_to_host(data, off) == []


def test_refusals(frames):
    ops, rgb = J.RefOps(), torch.from_numpy(frames)
    for bad, match in ((dict(rgb=rgb.float()), 'uint8'), (dict(rgb=rgb[0]), 'rgb'), (dict(rgb=rgb[..., :2]), 'rgb'), (dict(rgb=frames), 'rgb'),
                       (dict(rgb=rgb.permute(0, 2, 1, 3)), 'contiguous'), (dict(rgb=torch.zeros(1, 2049, 1, 3, dtype=torch.uint8)), '2048'),
                       (dict(rgb=torch.zeros(1, 0, 4, 3, dtype=torch.uint8)), 'height'),
                       (dict(quality=0), 'quality'), (dict(quality=101), 'quality'), (dict(quality=90.0), 'quality'),
                       (dict(subsampling='422'), 'subsampling'), (dict(subsampling=2), 'subsampling'),
                       (dict(restart=0), 'restart'), (dict(restart=65536), 'restart'), (dict(restart=2.0), 'restart')):
        kw = dict(rgb=rgb, ops=ops)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            V.encode_jpeg(kw.pop('rgb'), **kw)
    assert ops.calls == []
    with pytest.raises(RuntimeError, match='ROCm device'):               # host tensors without a provider: no CPU path
        V.encode_jpeg(rgb)
    with pytest.raises(RuntimeError, match='ROCm device'):
        V.skeleton_video(os.devnull, torch.from_numpy(SE.walking(2, seed=1)), 25, size=SIZE)


def test_library_refuses_bad_arguments():
    """no launch is made: the checks come first"""
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 230
    b = lambda *a: lib.mbx_jpeg_blocks(None, *a, None, None)      # noqa: E731  (F, H, W, quality, sub)
    assert b(1, 0, 8, 90, 1) != 0 and b'H=0' in lib.mbx_last_error()
    assert b(1, 8, 2049, 90, 1) != 0 and b'W=2049' in lib.mbx_last_error()
    assert b(65536, 8, 8, 90, 1) != 0 and b'F=65536' in lib.mbx_last_error()
    assert b(-1, 8, 8, 90, 1) != 0 and b'F=-1' in lib.mbx_last_error()
    assert b(1, 8, 8, 0, 1) != 0 and b'quality' in lib.mbx_last_error()
    assert b(1, 8, 8, 101, 0) != 0 and b'quality' in lib.mbx_last_error()
    assert b(1, 8, 8, 90, 2) != 0 and b'subsampling' in lib.mbx_last_error()
    assert b(1, 8, 8, 90, 1) != 0 and b'null' in lib.mbx_last_error()
    assert b(0, 8, 8, 90, 1) == 0
    s = lambda *a: lib.mbx_jpeg_entropy_sizes(None, *a, None, None, 0, None)      # noqa: E731  (F, H, W, sub, quality, restart)
    e = lambda *a: lib.mbx_jpeg_entropy(None, *a, None, None, 0, None, 0, None)      # noqa: E731
    for f in (s, e):
        assert f(1, 8, 8, 1, 90, 0) != 0 and b'restart' in lib.mbx_last_error()
        assert f(1, 8, 8, 1, 90, 65536) != 0 and b'restart' in lib.mbx_last_error()
        assert f(1, 8, 8, 3, 90, 1) != 0 and b'subsampling' in lib.mbx_last_error()
        assert f(1, 8, 8, 1, 0, 1) != 0 and b'quality' in lib.mbx_last_error()
        assert f(1, 4096, 8, 1, 90, 1) != 0 and b'H=4096' in lib.mbx_last_error()
        assert f(1, 8, 8, 1, 90, 1) != 0 and b'null' in lib.mbx_last_error()
        assert f(0, 8, 8, 1, 90, 1) == 0
    # a workspace or a data buffer that is too small is refused (the pointers are only compared, never followed)
    ws = lib.mbx_jpeg_entropy_ws(2, 64, 64, 1, 4)
    assert ws >= 2 * (16 * 6 * 2 + 4 * 8 + 4) and lib.mbx_jpeg_entropy_ws(2, 64, 64, 1, 0) == 0 and lib.mbx_jpeg_entropy_ws(2, 0, 64, 1, 1) == 0
    fake = ctypes.c_void_p(4096)
    assert lib.mbx_jpeg_entropy_sizes(fake, 2, 64, 64, 1, 90, 4, fake, fake, ws - 1, None) != 0 and b'workspace' in lib.mbx_last_error()
    assert lib.mbx_jpeg_entropy(fake, 2, 64, 64, 1, 90, 4, fake, fake, 100, fake, ws, None) != 0 and b'cannot hold' in lib.mbx_last_error()
    assert lib.mbx_jpeg_entropy(ctypes.c_void_p(4100), 2, 64, 64, 1, 90, 4, fake, fake, 1 << 20, fake, ws, None) != 0 and b'aligned' in lib.mbx_last_error()
    # the header is built on the host: the one libjpeg writes
    buf = (ctypes.c_ubyte * V.HEADER_BYTES)()
    for H, W, q, sub, rs in ((33, 17, 25, 1, 3), (2048, 1, 100, 0, 65535), (250, 250, 75, 1, 16)):
        assert lib.mbx_jpeg_header(H, W, q, sub, rs, buf) == 0 and bytes(buf) == J.header(H, W, q, '420' if sub else '444', rs)
    assert lib.mbx_jpeg_header(8, 8, 90, 1, 1, None) != 0 and b'null' in lib.mbx_last_error()


# ------------------------------------------------------------------------------------------------ the container
def _fields(path):
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


def test_writer_every_field(tmp_path, frames):
    files = [J.encode(f, 75, '444', 1) for f in frames] + [J.encode(frames[0], 25, '420', 1)]
    assert {len(f) & 1 for f in files} == {0, 1}                         # odd and even lengths: the padding shows
    path = str(tmp_path / 'a.avi')
    with V.MJPEGWriter(path, 17, 33, 29.97) as w:
        w.write(np.frombuffer(b''.join(files[:3]), np.uint8), np.cumsum([0] + [len(f) for f in files[:3]]))
        w.write(b'junk' + files[3], [4, 4 + len(files[3])])
        assert w.frames == 4
    assert w.closed and w.bytes == os.path.getsize(path)
    w.close()                                                            # a second close is nothing
    with pytest.raises(ValueError, match='closed'):
        w.write(files[0], [0, len(files[0])])
    data, avih, strh, strf, movi, idx1 = _fields(path)
    largest = max(len(f) for f in files)
    assert avih == (33367, sum(len(f) for f in files) * 29970 // 4000, 0, 0x10, 4, 0, 1, largest, 17, 33, 0, 0, 0, 0)
    assert strh[:8] == b'vidsMJPG'
    assert struct.unpack('<IHHIIIIIIII4H', strh[8:]) == (0, 0, 0, 0, 1000, 29970, 0, 4, largest, 0xffffffff, 0, 0, 0, 17, 33)
    assert strf == (40, 17, 33, 1, 24, b'MJPG', 17 * 33 * 3, 0, 0, 0, 0)
    assert movi['offset'] == V.MJPEGWriter.HEADER - 12 and [c['id'] for c in movi['chunks']] == [b'00dc'] * 4
    assert [c['data'] for c in movi['chunks']] == files == J.avi_frames(data)
    entries = [struct.unpack('<4sIII', idx1['data'][16 * k:16 * k + 16]) for k in range(4)]
    assert idx1['size'] == 64
    for c, f, (cid, flags, at, n) in zip(movi['chunks'], files, entries):
        assert (cid, flags, n) == (b'00dc', 0x10, len(f)) and at == c['offset'] - (movi['offset'] + 8)      # relative to the 'movi' fourcc
        assert c['offset'] % 2 == 0 and data[movi['offset'] + 8 + at:][:8] == b'00dc' + struct.pack('<I', len(f))
        if len(f) & 1:
            assert data[c['offset'] + 8 + len(f)] == 0
    assert entries[0][2] == 4
    # an empty file is still a complete one
    with V.MJPEGWriter(str(tmp_path / 'e.avi'), 8, 8, 25):
        pass
    _, avih, strh, _, movi, idx1 = _fields(str(tmp_path / 'e.avi'))
    assert avih[:5] == (40000, 0, 0, 0x10, 0) and movi['chunks'] == [] and idx1['size'] == 0


def test_writer_refusals(tmp_path, frames):
    f = J.encode(frames[0], 75, '444', 1)
    for bad in (dict(width=0), dict(height=70000), dict(width=8.0), dict(fps=0), dict(fps=float('nan')), dict(fps='25')):
        kw = dict(width=8, height=8, fps=25)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.MJPEGWriter(str(tmp_path / 'never.avi'), **kw)
    assert not os.path.exists(tmp_path / 'never.avi')
    with V.MJPEGWriter(str(tmp_path / 'b.avi'), 17, 33, 25) as w:
        for data, off in ((f, [0, len(f) + 1]), (f, [5, 5 + len(f) - 5]), (f, []), (f, [0, 1]), (np.zeros(4, np.int32), [0, 4])):
            with pytest.raises(ValueError):
                w.write(data, off)
        assert w.frames == 0


def test_two_gigabytes_are_refused_before_writing(tmp_path, frames, monkeypatch):
    f = J.encode(frames[0], 75, '444', 1)
    per = 8 + len(f) + (len(f) & 1) + 16
    assert V.MJPEGWriter.MAX_BYTES == 2 ** 31 - 1
    monkeypatch.setattr(V.MJPEGWriter, 'MAX_BYTES', V.MJPEGWriter.HEADER + 8 + 3 * per)          # room for exactly three frames
    path = str(tmp_path / 'big.avi')
    with V.MJPEGWriter(path, 17, 33, 25) as w:
        w.write(f * 2, [0, len(f), 2 * len(f)])
        w.file.flush()
        before = os.path.getsize(path)
        with pytest.raises(ValueError, match='AVI 1.0 ends'):
            w.write(f * 2, [0, len(f), 2 * len(f)])                      # two more would pass the end: none is written
        w.file.flush()
        assert os.path.getsize(path) == before and w.frames == 2
        w.write(f, [0, len(f)])
    assert os.path.getsize(path) == V.MJPEGWriter.MAX_BYTES == w.bytes and len(J.avi_frames(open(path, 'rb').read())) == 3
    # at the real limit: the arithmetic alone, nothing of that size is written
    monkeypatch.undo()
    with V.MJPEGWriter(str(tmp_path / 'c.avi'), 17, 33, 25) as w:
        w.movi_bytes = 2 ** 31 - 1 - w.HEADER - 8 - per + 4
        w.write(f, [0, len(f)])
        w.index.pop()
        w.movi_bytes = 2 ** 31 - 1 - w.HEADER - 8 - per + 4 + 1
        with pytest.raises(ValueError, match='AVI 1.0 ends'):
            w.write(f, [0, len(f)])
        w.movi_bytes, w.index = 4, []


# ------------------------------------------------------------------------------------------------ render, encode, write
def test_skeleton_video_end_to_end(tmp_path):
    x = torch.from_numpy(SE.walking(5, seed=2))
    ops, path = Ops(), str(tmp_path / 'x3d.avi')
    radii = R.skeleton_radii(256)
    assert V.skeleton_video(path, x, 25, quality=75, chunk=2, size=SIZE, radii=radii, ops=ops) == (5, os.path.getsize(path))
    # the host runs one chunk ahead: the next render is queued before the emission of the chunk whose sizes it waits for
    assert [c for c in ops.calls if c[0] in ('raster', 'emit')] == [('raster', 2), ('raster', 2), ('emit', 2), ('raster', 1), ('emit', 2), ('emit', 1)]
    rgb = R.render_skeleton(x, size=SIZE, radii=radii, ops=SE.RefOps())['rgb'].numpy()
    assert (rgb != 255).any()
    data, avih, strh, strf, _, _ = _fields(path)
    assert J.avi_frames(data) == [J.encode(f, 75, '420') for f in rgb]
    assert avih[4] == 5 and avih[8:10] == (SIZE, SIZE) and struct.unpack('<II', strh[20:28]) == (1000, 25000)
    # the chunking does not show; 4:4:4 and a restart interval of the caller's
    other = str(tmp_path / 'y.avi')
    V.skeleton_video(other, x.numpy(), 25, quality=75, chunk=5, size=SIZE, radii=radii, ops=Ops())
    assert open(other, 'rb').read() == data
    V.skeleton_video(other, x, 25, quality=75, subsampling='444', restart=2, chunk=3, size=SIZE, radii=radii, ops=Ops())
    assert J.avi_frames(open(other, 'rb').read()) == [J.encode(f, 75, '444', 2) for f in rgb]
    assert V.skeleton_video(other, x[:0], 25, size=SIZE, ops=Ops()) == (0, V.MJPEGWriter.HEADER + 8)
    for bad, match in ((dict(chunk=0), 'chunk'), (dict(quality=0), 'quality'), (dict(subsampling='411'), 'subsampling'), (dict(size=0), 'size')):
        with pytest.raises(ValueError, match=match):
            V.skeleton_video(str(tmp_path / 'never.avi'), x, 25, ops=Ops(), **{**dict(size=SIZE), **bad})
    assert not os.path.exists(tmp_path / 'never.avi')


def test_mesh_video_end_to_end(tmp_path):
    verts, faces = RE.deformed_icosphere(5, seed=1)
    tv, tf = torch.from_numpy(verts), torch.from_numpy(faces)
    ops, path = Ops(), str(tmp_path / 'mesh.avi')
    assert V.mesh_video(path, tv, tf, 30, chunk=2, size=SIZE, seq_lens=[3, 2], ops=ops) == (5, os.path.getsize(path))
    assert [c[1] for c in ops.calls if c[0] == 'emit'] == [2, 2, 1]
    rgb = R.render_mesh(tv, tf, size=SIZE, seq_lens=[3, 2], ops=RE.RefOps())['rgb'].numpy()
    assert (rgb != 255).any()
    assert J.avi_frames(open(path, 'rb').read()) == [J.encode(f, 90, '420') for f in rgb]      # the cube of the whole motion, whatever the chunking
