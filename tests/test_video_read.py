"""Reading video on the CPU through the reference provider (tests/jpegdecerr.RefOps): `video.decode_jpeg`, `video.MJPEGReader` on the files
`MJPEGWriter` writes and on hand-built variants of the container, `scene_video` / `scene_chunks` over a reader, and the C ABI's refusals."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from motionbert_amd import video as V
from tests import jpegdecerr as D
from tests import jpegerr as J
from tests import sceneerr as SC
from tests.test_scene import crowd      # noqa: F401  (the fixture)

W, H = 56, 40


class Ops(D.RefOps, SC.RefOps):
    """the JPEG references and the scene reference as one provider"""

    def __init__(self):
        D.RefOps.__init__(self)
        SC.RefOps.__init__(self)


@pytest.fixture(scope='module')
def frames():
    rgb = np.stack([J.content(k, H, W, seed=9 + i) for i, k in enumerate(('noise', 'render', 'ramp', 'noise', 'render'))])
    files = [J.encode(f, 90, '420') for f in rgb]
    return files, np.stack([D.decode(f) for f in files])


# ------------------------------------------------------------------------------------------------ decode_jpeg
def test_decode_jpeg_forms_and_hooks(frames):
    files, ref = frames
    ops = D.RefOps()
    rgb = V.decode_jpeg(files, ops=ops)
    assert rgb.dtype == torch.uint8 and np.array_equal(rgb.numpy(), ref)
    assert [c for c in ops.calls if c[0].startswith('dec')] == [('dec_index', 5), ('dec_entropy', 5), ('dec_pixels', 5)]      # one group
    data, off = np.frombuffer(b''.join(files), np.uint8).copy(), np.concatenate([[0], np.cumsum([len(f) for f in files])])
    assert torch.equal(V.decode_jpeg(torch.from_numpy(data), torch.from_numpy(off), ops=D.RefOps()), rgb)
    assert torch.equal(V.decode_jpeg(data, off, ops=D.RefOps()), rgb)
    out = torch.zeros(5, H, W, 3, dtype=torch.uint8)
    assert V.decode_jpeg(files, out=out, ops=D.RefOps()) is out and torch.equal(out, rgb)
    res = V.decode_jpeg(files[:2], want=('coef', 'status', 'pos'), ops=D.RefOps())
    for f in range(2):
        coef, status, pos = D.entropy(files[f])
        assert np.array_equal(res['coef'][f].numpy(), coef) and not res['status'].any()
        assert np.array_equal(res['pos'][f].numpy() - (0 if f == 0 else len(files[0])), pos)
    none = V.decode_jpeg([], ops=(ops := D.RefOps()))
    assert none.shape == (0, 0, 0, 3) and not ops.calls


def test_decode_jpeg_groups_frames_that_share_tables(frames):
    files, ref = frames
    rgb = J.content('noise', H, W, seed=3)
    mixed = [files[0], files[1], J.encode(rgb, 75, '444', 3), J.encode(rgb, 75, '444', 3), files[2]]
    ops = D.RefOps()
    got = V.decode_jpeg(mixed, ops=ops)
    assert [c for c in ops.calls if c[0] == 'dec_entropy'] == [('dec_entropy', 2), ('dec_entropy', 2), ('dec_entropy', 1)]
    assert all(np.array_equal(got[i].numpy(), D.decode(f)) for i, f in enumerate(mixed))
    with pytest.raises(ValueError, match='test hooks'):
        V.decode_jpeg(mixed, want=('coef',), ops=D.RefOps())


def test_decode_jpeg_refusals(frames):
    files, _ = frames
    ops = D.RefOps()
    with pytest.raises(ValueError, match='different sizes'):
        V.decode_jpeg([files[0], J.encode(J.content('noise', 8, 8), 90, '420')], ops=ops)
    with pytest.raises(ValueError, match='want'):
        V.decode_jpeg(files, want=('pixels',), ops=ops)
    with pytest.raises(ValueError, match='offsets'):
        V.decode_jpeg(torch.zeros(10, dtype=torch.uint8), [0, 20], ops=ops)
    with pytest.raises(ValueError, match='list of'):
        V.decode_jpeg(torch.zeros(10, dtype=torch.uint8), ops=ops)
    with pytest.raises(ValueError, match='out must be'):
        V.decode_jpeg(files, out=torch.zeros(5, H, W, 4, dtype=torch.uint8), ops=ops)
    assert not ops.calls
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            V.decode_jpeg(files)
    bad, k, st = D.malformed()['cut']
    res = V.decode_jpeg([bad], want=('status', 'coef'), ops=D.RefOps())                  # with the hook the status is returned, not raised
    assert res['status'][0].tolist() == [0, st, 0] and np.array_equal(res['coef'][0].numpy(), D.entropy(bad)[0])


# ------------------------------------------------------------------------------------------------ the container
def test_reader_gives_back_what_the_writer_wrote(tmp_path, frames):
    files, ref = frames
    assert any(len(f) & 1 for f in files) and any(not len(f) & 1 for f in files)         # odd chunks are padded: both kinds are here
    path = str(tmp_path / 'v.avi')
    with V.MJPEGWriter(path, W, H, 29.97) as w:
        w.write(b''.join(files[:2]), np.cumsum([0] + [len(f) for f in files[:2]]))
        w.write(b''.join(files[2:]), np.cumsum([0] + [len(f) for f in files[2:]]))
    with V.MJPEGReader(path) as r:
        assert (r.width, r.height, r.frames, r.fps) == (W, H, 5, 29.97)
        assert [r.frame_bytes(f) for f in range(5)] == files
        assert np.array_equal(r.read(ops=D.RefOps()).numpy(), ref) and np.array_equal(r.read(1, 4, ops=D.RefOps()).numpy(), ref[1:4])
        assert r.read(2, 2, ops=D.RefOps()).shape == (0, H, W, 3)
        for chunk in (1, 2, 5, 7):
            parts = [p.clone() for p in r.chunks(chunk, ops=D.RefOps())]
            assert [len(p) for p in parts] == [min(chunk, 5 - a) for a in range(0, 5, chunk)] and np.array_equal(torch.cat(parts).numpy(), ref)
        for a, b in ((-1, 2), (3, 2), (0, 6)):
            with pytest.raises(ValueError, match='frames'):
                r.read(a, b, ops=D.RefOps())
        with pytest.raises(ValueError, match='chunk'):
            next(r.chunks(0, ops=D.RefOps()))
    with pytest.raises(ValueError, match='closed'):
        r.read(ops=D.RefOps())
    one, zero = str(tmp_path / 'one.avi'), str(tmp_path / 'zero.avi')
    with V.MJPEGWriter(one, W, H, 25) as w:
        w.write(files[3], [0, len(files[3])])
    V.MJPEGWriter(zero, W, H, 25).close()
    with V.MJPEGReader(one) as r:
        assert r.frames == 1 and np.array_equal(r.read(ops=D.RefOps())[0].numpy(), ref[3])
    with V.MJPEGReader(zero) as r:
        assert r.frames == 0 and r.read(ops=D.RefOps()).shape == (0, H, W, 3) and list(r.chunks(4, ops=D.RefOps())) == []


def _chunk(cid, data):
    return cid + struct.pack('<I', len(data)) + data + (b'\0' if len(data) & 1 else b'')


def _avi(files, index='movi', junk=False, rec=False, handler=b'MJPG', compression=b'MJPG', avix=False, audio_first=False, empty=()):
    """an AVI file built by hand, chunk by chunk, in the shapes other writers give it"""
    avih = struct.pack('<14I', 40000, 0, 0, 0x10, len(files), 0, 1 + audio_first, 0, W, H, 0, 0, 0, 0)
    strh = b'vids' + handler + struct.pack('<IHHIIIIIIII4H', 0, 0, 0, 0, 1001, 30000, 0, len(files), 0, 0xffffffff, 0, 0, 0, W, H)
    strf = struct.pack('<IiiHH4sIiiII', 40, W, H, 1, 24, compression, W * H * 3, 0, 0, 0, 0)
    strl = _chunk(b'LIST', b'strl' + _chunk(b'strh', strh) + _chunk(b'strf', strf) + (_chunk(b'JUNK', b'\0' * 13) if junk else b''))
    auds = _chunk(b'LIST', b'strl' + _chunk(b'strh', b'auds' + b'\0' * 52) + _chunk(b'strf', b'\0' * 18))
    hdrl = _chunk(b'LIST', b'hdrl' + _chunk(b'avih', avih) + (auds + strl if audio_first else strl))
    sid = b'01dc' if audio_first else b'00dc'
    movi, entries = b'movi', []
    for f, data in enumerate(files):
        data = b'' if f in empty else data
        one = (_chunk(b'01wb' if not audio_first else b'00wb', b'\1\2\3') if junk else b'') + _chunk(sid, data)
        at = len(movi) + (12 if rec else 0) + (len(one) - len(_chunk(sid, data)))
        entries.append((at, len(data)))
        movi += _chunk(b'LIST', b'rec ' + one) if rec else one
        if junk and f == 1:
            movi += _chunk(b'JUNK', b'\0' * 7)
    head = b'AVI ' + hdrl + (_chunk(b'JUNK', b'\0' * 20) if junk else b'')
    base = 12 + len(head) - 4 + 8                                        # where the 'movi' fourcc lies in the file
    body = head + _chunk(b'LIST', movi)
    if index:
        body += _chunk(b'idx1', b''.join(sid + struct.pack('<III', 0x10, at + (base if index == 'file' else 0), n) for at, n in entries))
    out = b'RIFF' + struct.pack('<I', len(body)) + body
    return out + (b'RIFF' + struct.pack('<I', 4) + b'AVIX' if avix else b'')


@pytest.mark.parametrize('kw', [dict(), dict(index=None), dict(index='file'), dict(junk=True), dict(rec=True), dict(rec=True, index=None, junk=True),
                                dict(handler=b'mjpg'), dict(handler=b'\0\0\0\0', compression=b'mjpg'), dict(audio_first=True),
                                dict(audio_first=True, index=None, junk=True), dict(index='file', junk=True, rec=True)],
                         ids=lambda kw: '.'.join(f'{k}={v}' for k, v in kw.items()) or 'plain')
def test_reader_on_hand_built_variants(tmp_path, frames, kw):
    files, ref = frames
    path = str(tmp_path / 'v.avi')
    open(path, 'wb').write(_avi(files, **kw))
    with V.MJPEGReader(path) as r:
        assert (r.frames, r.width, r.height) == (5, W, H) and abs(r.fps - 30000 / 1001) < 1e-12
        assert [r.frame_bytes(f) for f in range(5)] == files
        assert np.array_equal(r.read(3, 5, ops=D.RefOps()).numpy(), ref[3:5])


def test_reader_refusals_and_repeats(tmp_path, frames):
    files, ref = frames
    path = str(tmp_path / 'v.avi')
    for kw, match in ((dict(handler=b'H264', compression=b'H264'), 'not MJPG'), (dict(avix=True), 'OpenDML')):
        open(path, 'wb').write(_avi(files, **kw))
        with pytest.raises(ValueError, match=match):
            V.MJPEGReader(path)
    open(path, 'wb').write(b'RIFF\x04\0\0\0WAVE')
    with pytest.raises(ValueError, match='AVI'):
        V.MJPEGReader(path)
    open(path, 'wb').write(_avi(files)[:-4] + struct.pack('<I', 1 << 30))      # the index names a frame that runs past the end
    with pytest.raises(ValueError, match='past the end'):
        V.MJPEGReader(path)
    open(path, 'wb').write(_avi(files, index=None)[:-10])                 # and so does the last chunk of a file cut short
    with pytest.raises(ValueError, match='past the end'):
        V.MJPEGReader(path)
    for index in ('movi', None):                                          # a chunk of length 0 repeats the frame before it
        open(path, 'wb').write(_avi(files, index=index, empty=(2,)))
        with V.MJPEGReader(path) as r:
            assert np.array_equal(r.read(ops=D.RefOps()).numpy(), ref[[0, 1, 1, 3, 4]])
    open(path, 'wb').write(_avi([J.encode(J.content('noise', 8, 8), 90, '420')] * 2))      # the container says 40 x 56
    with V.MJPEGReader(path) as r, pytest.raises(ValueError, match='are expected'):
        r.read(ops=D.RefOps())


# ------------------------------------------------------------------------------------------------ the scene over a reader
def test_scene_video_over_a_reader_writes_the_same_bytes(tmp_path, crowd):      # noqa: F811
    x3d, _, table = crowd
    bg = SC.backdrop(3, W, H, seed=4)
    src, a, b = str(tmp_path / 'in.avi'), str(tmp_path / 'a.avi'), str(tmp_path / 'b.avi')
    files = [J.encode(f, 90, '420') for f in bg]
    with V.MJPEGWriter(src, W, H, 25) as w:
        w.write(b''.join(files), np.cumsum([0] + [len(f) for f in files]))
    decoded = np.stack([D.decode(f) for f in files])
    with V.MJPEGReader(src) as r:
        ops = Ops()
        assert V.scene_video(a, x3d, table, W, H, 25, background=r, chunk=2, ops=ops) == (3, os.path.getsize(a))
        assert [c for c in ops.calls if c[0] in ('dec_pixels', 'scene_raster')] == [('dec_pixels', 2), ('scene_raster', 2), ('dec_pixels', 1), ('scene_raster', 1)]
        V.scene_video(b, x3d, table, W, H, 25, background=torch.from_numpy(decoded), chunk=2, ops=Ops())
        assert open(a, 'rb').read() == open(b, 'rb').read()
        whole = R.render_scene(x3d, table, W, H, background=r, ops=Ops())['rgb'].numpy()
        assert np.array_equal(whole, R.render_scene(x3d, table, W, H, background=decoded, ops=Ops())['rgb'].numpy())
        parts = [p.copy() for p in R.scene_chunks(x3d, table, W, H, background=r, chunk=2, ops=Ops())]
        assert np.array_equal(np.concatenate(parts), whole)
        ops = Ops()
        for kw, match in ((dict(width=W + 8), 'background video'), (dict(table=R.scene_table({3: np.array([0, 1])})), 'background video')):
            with pytest.raises(ValueError, match=match):
                V.scene_video(str(tmp_path / 'never.avi'), **{**dict(x3d=x3d, table=table, width=W, height=H, fps=25, background=r, ops=ops), **kw})
        assert not ops.calls and not os.path.exists(tmp_path / 'never.avi')


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_refuses_bad_arguments():
    """no launch is made: the checks come first"""
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 250
    fake = ctypes.c_void_p(4096)
    assert lib.mbx_jpeg_dec_ws(1, 16, 16, 1) == 16 * 16 * 3 // 2 and lib.mbx_jpeg_dec_ws(2, 17, 33, 2) == 2 * 3 * 3 * 4 * 64 and lib.mbx_jpeg_dec_ws(1, 8, 8, 3) == 0
    assert lib.mbx_jpeg_dec_index(None, 0, None, 0, 1, None, None, None) == 0
    assert lib.mbx_jpeg_dec_index(fake, 10, fake, 1, 0, fake, fake, None) != 0 and b'n_int=0' in lib.mbx_last_error()
    assert lib.mbx_jpeg_dec_index(fake, 10, None, 1, 1, fake, fake, None) != 0 and b'null' in lib.mbx_last_error()
    e = lambda F=1, H_=16, W_=16, sub=1, rs=1, p=fake: lib.mbx_jpeg_dec_entropy(p, 10, p, p, F, H_, W_, sub, rs, p, p, None)      # noqa: E731
    for kw, word in ((dict(H_=0), b'H=0'), (dict(W_=2049), b'W=2049'), (dict(sub=3), b'subsampling 3'), (dict(rs=-1), b'restart'), (dict(rs=65536), b'restart'),
                     (dict(F=65536), b'F=65536'), (dict(p=None), b'null'), (dict(p=ctypes.c_void_p(4098)), b'aligned')):
        assert e(**kw) != 0 and word in lib.mbx_last_error(), (kw, lib.mbx_last_error())
    assert e(F=0, p=None) == 0
    q = (ctypes.c_ubyte * 192)(*([1] * 192))
    px = lambda F=1, H_=16, W_=16, sub=1, ws=1 << 20, p=fake, q_=q: lib.mbx_jpeg_dec_pixels(p, q_, F, H_, W_, sub, p, p, ws, None)      # noqa: E731
    for kw, word in ((dict(H_=0), b'H=0'), (dict(sub=-1), b'subsampling'), (dict(ws=383), b'workspace'), (dict(p=None), b'null'),
                     (dict(q_=(ctypes.c_ubyte * 192)()), b'quantisation'), (dict(p=ctypes.c_void_p(4104)), b'aligned')):
        assert px(**kw) != 0 and word in lib.mbx_last_error(), (kw, lib.mbx_last_error())
    assert px(F=0, p=None) == 0
    ops = hip_ops.HipOps(lib)
    tab = ops.jpeg_dec_tables(None).numpy().view(np.uint32)
    assert tab.shape == (6, 228) and np.array_equal(tab[0], tab[0]) and np.array_equal(tab[2], tab[4]) and not np.array_equal(tab[0], tab[2])
    look = tab[1, :128].copy().view(np.uint16)                            # AC luminance: '00' is symbol 1, '1010' is EOB
    assert look[0] == (2 << 8 | 1) and look[0b10100000] == (4 << 8 | 0) and look[0xff] == 0
    assert np.array_equal(ops.jpeg_dec_tables(D.annex_k()).numpy(), ops.jpeg_dec_tables(None).numpy())
    bad = D.annex_k()
    bad[0, 16] = 16                                                       # a DC symbol above 15
    with pytest.raises(ValueError, match='table 0'):
        ops.jpeg_dec_tables(bad)
    bad = D.annex_k()
    bad[3, 0] = 3                                                         # three codes of length 1
    with pytest.raises(ValueError, match='table 3'):
        ops.jpeg_dec_tables(bad)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mbx.h')).read()
    for name, v in (('OK', D.OK), ('TRUNCATED', D.TRUNCATED), ('BAD_CODE', D.BAD_CODE), ('RUN', D.RUN), ('LEFTOVER', D.LEFTOVER), ('MARKERS', D.MARKERS)):
        assert f'#define MBX_JPEG_DEC_{name} {v}\n' in src
    assert V.DEC_STATUS == D.STATUS and '#define MBX_JPEG_DEC_TABLE_WORDS 228' in src
