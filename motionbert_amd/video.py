"""Video files from the device: the frames of motionbert_amd.render compressed where they were drawn (csrc/jpeg.hip) and written as Motion-JPEG
in an AVI container: the `X3D.mp4` / `mesh.mp4` of infer_wild.py / infer_wild_mesh.py (`render_and_save`) as a file this package writes itself.
An Instinct has no fixed-function encoder; the frames are compressed by compute, as they were drawn by compute, and only the compressed bytes
cross the host link.

    encode_jpeg(rgb, quality, subsampling, restart)   rgb uint8 [F,H,W,3] on the device -> (data uint8 [total], offsets int64 [F+1]), both on the
                                                      device: F complete baseline JFIF files back to back, each byte for byte the file libjpeg
                                                      writes for the same pixels and settings (include/mbx.h has the definition)
    frames_to_host(data, offsets)                     -> a list of F `bytes`
    MJPEGWriter(path, width, height, fps)             AVI 1.0 (RIFF 'AVI ', hdrl / avih / strl / strh / strf, movi with one 00dc chunk per frame,
                                                      idx1); `.write(host_bytes, offsets)`, `.close()`, a context manager; at most 2^31 - 1 bytes
    mesh_video(path, verts, faces, fps, ...)          render.render_mesh + encode_jpeg + MJPEGWriter, `chunk` frames at a time -> (frames, bytes)
    skeleton_video(path, x3d, fps, ...)               render.render_skeleton likewise
    scene_video(path, x3d, table, W, H, fps, ...)     render.render_scene likewise: every tracked person in one video of the input's size

One host synchronisation per encode: the sizes of the files are computed on the device first, the host reads their total and allocates, then the
bytes are emitted straight into place.  In the *_video functions that wait falls under the copy of the chunk before.

Not here: inter-frame codecs, optimised Huffman tables, progressive / 12-bit / grayscale JPEG, AVI beyond 2 GB (OpenDML), audio, decoding.  No AVI
reader exists where this was developed: the container is checked field by field against its specification and has not been played.

There is no CPU path: without an injected kernel provider (`ops=`), tensors that are not on a ROCm device raise."""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import hip_ops
from . import render as R

MAX_SIZE, MAX_FRAMES, HEADER_BYTES = 2048, 65535, 629
SUBSAMPLINGS = ('444', '420')          # the index is the `sub` of the C ABI


def geometry(H: int, W: int, subsampling: str):
    """(MCU columns, MCU rows, blocks per MCU) of a frame"""
    m = 16 if subsampling == '420' else 8
    return -(-W // m), -(-H // m), 6 if subsampling == '420' else 3


def _check_coding(H, W, quality, subsampling, restart, where):
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"{where}: subsampling must be '420' or '444', got {subsampling!r}")
    if not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f'{where}: quality must be an int in [1, 100], got {quality!r}')
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f'{where}: frames of {H} x {W}: height and width must be in [1, {MAX_SIZE}]')
    restart = geometry(H, W, subsampling)[0] if restart is None else restart          # one MCU row
    if not isinstance(restart, int) or not 1 <= restart <= 65535:
        raise ValueError(f'{where}: restart must be an int in [1, 65535] (MCUs), got {restart!r}')
    return restart


def _encode(prov, rgb, quality, sub, restart, coef=None):
    """the three stages on the current stream up to the sizes: (coef, offsets, ws)"""
    F, H, W = rgb.shape[:3]
    mx, my, bpm = geometry(H, W, SUBSAMPLINGS[sub])
    if coef is None:
        coef = torch.empty(F, mx * my, bpm, 64, dtype=torch.int16, device=rgb.device)
    offsets = torch.empty(F + 1, dtype=torch.int64, device=rgb.device)
    ws = prov.jpeg_ws(F, H, W, sub, restart, rgb.device)
    prov.jpeg_blocks(rgb, quality, sub, coef)
    prov.jpeg_sizes(coef, H, W, sub, quality, restart, offsets, ws)
    return coef, offsets, ws


def encode_jpeg(rgb, quality: int = 90, subsampling: str = '420', restart=None, ops=None):
    """rgb uint8 [F,H,W,3], contiguous, on the device (1 <= H, W <= 2048, F <= 65535) -> (data uint8 [total], offsets int64 [F+1]) on the device:
    frame f is the baseline JFIF file data[offsets[f]:offsets[f+1]].  `quality` 1 .. 100 scales the Annex K tables the IJG way; `subsampling`
    '420' or '444'; `restart`: the restart interval in MCUs (default: one MCU row), the unit of parallel work.  Four kernel calls and ONE host
    synchronisation, the read of the total size between the sizing and the emission; F = 0 returns empty tensors without a launch."""
    where = 'video.encode_jpeg'
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3 or not rgb.is_contiguous():
        raise ValueError(f'{where}: rgb must be a contiguous uint8 tensor [F,H,W,3], got '
                         f'{tuple(rgb.shape) if hasattr(rgb, "shape") else type(rgb).__name__} {getattr(rgb, "dtype", "")}')
    F, H, W = rgb.shape[:3]
    if F > MAX_FRAMES:
        raise ValueError(f'{where}: {F} frames in one call, at most {MAX_FRAMES}')
    restart = _check_coding(H, W, quality, subsampling, restart, where)
    prov = hip_ops.provider(ops, 'motionbert_amd.' + where, rgb)
    if F == 0:
        return torch.empty(0, dtype=torch.uint8, device=rgb.device), torch.zeros(1, dtype=torch.int64, device=rgb.device)
    sub = SUBSAMPLINGS.index(subsampling)
    coef, offsets, ws = _encode(prov, rgb, quality, sub, restart)
    data = torch.empty(int(offsets[F]), dtype=torch.uint8, device=rgb.device)              # the one host synchronisation
    prov.jpeg_emit(coef, H, W, sub, quality, restart, offsets, data, ws)
    return data, offsets


def frames_to_host(data, offsets):
    """the F files of `encode_jpeg` as a list of `bytes`"""
    d, o = data.cpu().numpy(), offsets.cpu().numpy()
    return [d[o[f]:o[f + 1]].tobytes() for f in range(len(o) - 1)]


# ------------------------------------------------------------------------------------------------ the container
class MJPEGWriter:
    """An AVI 1.0 file of Motion-JPEG frames.  `write(host_bytes, offsets)` appends the frames host_bytes[offsets[f]:offsets[f+1]] (complete JFIF
    files of width x height), one '00dc' chunk each, padded to even length; `close()` writes 'idx1' (flag 0x10, offsets relative to the 'movi'
    fourcc) and patches the frame count and the sizes into the headers.  The rate is round(fps 1000) / 1000.  A file that would pass MAX_BYTES =
    2^31 - 1 bytes raises before the frames are written (OpenDML is not written)."""
    MAX_BYTES = 2 ** 31 - 1
    HEADER = 12 + 12 + 64 + 12 + 64 + 48 + 12          # RIFF, LIST hdrl, avih, LIST strl, strh, strf, LIST movi: the first chunk lies here

    def __init__(self, path, width: int, height: int, fps: float):
        if not (isinstance(width, int) and isinstance(height, int) and 1 <= width <= 65535 and 1 <= height <= 65535):
            raise ValueError(f'MJPEGWriter: width and height must be ints in [1, 65535], got {width!r} x {height!r}')
        if not (isinstance(fps, (int, float)) and np.isfinite(fps) and round(fps * 1000) >= 1 and round(fps * 1000) < 2 ** 32):
            raise ValueError(f'MJPEGWriter: fps must be a finite rate of at least 0.001, got {fps!r}')
        self.path, self.width, self.height, self.rate, self.scale = path, width, height, int(round(fps * 1000)), 1000
        self.index, self.movi_bytes, self.largest, self.closed = [], 4, 0, False          # movi_bytes counts from the 'movi' fourcc
        self.file = open(path, 'wb')
        self.file.write(self._headers())

    @property
    def frames(self):
        return len(self.index)

    @property
    def bytes(self):
        """the size of the file if it were closed now"""
        return self.HEADER - 4 + self.movi_bytes + 8 + 16 * len(self.index)

    def _headers(self):
        n, w, h = len(self.index), self.width, self.height
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        per_sec = min((sum(s for _, s in self.index) * self.rate) // (self.scale * n), 0xffffffff) if n else 0
        avih = struct.pack('<14I', usec, per_sec, 0, 0x10, n, 0, 1, self.largest, w, h, 0, 0, 0, 0)
        strh = b'vidsMJPG' + struct.pack('<IHHIIIIIIII4H', 0, 0, 0, 0, self.scale, self.rate, 0, n, self.largest, 0xffffffff, 0, 0, 0, w, h)
        strf = struct.pack('<IiiHH4sIiiII', 40, w, h, 1, 24, b'MJPG', w * h * 3, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        head = b'RIFF' + struct.pack('<I', self.bytes - 8) + b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl
        head += b'LIST' + struct.pack('<I', self.movi_bytes) + b'movi'
        assert len(head) == self.HEADER
        return head

    def write(self, host_bytes, offsets):
        if self.closed:
            raise ValueError('MJPEGWriter.write: the file is closed')
        buf = np.frombuffer(host_bytes, np.uint8) if isinstance(host_bytes, (bytes, bytearray, memoryview)) else np.asarray(host_bytes)
        off = np.asarray(offsets, np.int64)
        if buf.dtype != np.uint8 or buf.ndim != 1 or off.ndim != 1 or off.size < 1 or off[0] < 0 or off[-1] > buf.size or (np.diff(off) < 2).any():
            raise ValueError(f'MJPEGWriter.write: offsets {off.tolist()[:6]} do not frame files inside {buf.size} bytes')
        sizes = np.diff(off)
        grown = int((8 + sizes + (sizes & 1)).sum())
        if self.bytes + grown + 16 * len(sizes) > self.MAX_BYTES:
            raise ValueError(f'MJPEGWriter.write: {len(sizes)} more frames make a file of {self.bytes + grown + 16 * len(sizes)} bytes; AVI 1.0 ends at '
                             f'{self.MAX_BYTES} (start another file)')
        for f, n in enumerate(sizes.tolist()):
            frame = buf[off[f]:off[f + 1]]
            if frame[0] != 0xff or frame[1] != 0xd8:
                raise ValueError(f'MJPEGWriter.write: frame {f} of this call does not start with SOI')
            self.file.write(b'00dc' + struct.pack('<I', n))
            self.file.write(frame.tobytes() + (b'\0' if n & 1 else b''))
            self.index.append((self.movi_bytes, n))
            self.movi_bytes += 8 + n + (n & 1)
            self.largest = max(self.largest, n)

    def close(self):
        if self.closed:
            return
        self.closed = True
        self.file.write(b'idx1' + struct.pack('<I', 16 * len(self.index)))
        self.file.write(b''.join(b'00dc' + struct.pack('<III', 0x10, at, n) for at, n in self.index))
        self.file.seek(0)
        self.file.write(self._headers())
        self.file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ------------------------------------------------------------------------------------------------ render, encode, copy, write
def _video_pipeline(writer, prov, F, chunk, H, W, dev, span, quality, sub, restart):
    """The frames of `span(a, b, rgb)` (which launches the render of frames a .. b - 1 into the device tensor rgb) into `writer`, `chunk` frames
    at a time: the structure of render._pipeline with the encoder between the render and the copy.  Per chunk, on the current stream: render,
    coefficients, sizes (`first`); once the host has read the sizes (its one wait per chunk) it makes room and launches the emission.  The
    host runs one chunk ahead: the render of chunk i + 1 is queued BEFORE the wait for the sizes of chunk i, so the device never waits for
    the host; the emission of chunk i follows that render, and the copy of its compressed bytes to pinned memory runs on a side stream under
    the render after that, while the chunk before is appended to the file.  One frame buffer; two of everything that outlives a render
    (coefficients, sizes, device and pinned byte buffers, which grow to the largest chunk)."""
    spans = [(a, min(a + chunk, F)) for a in range(0, F, chunk)]
    piped = dev.type == 'cuda'
    n_max, n_buf = min(chunk, F), min(2, len(spans))
    mx, my, bpm = geometry(H, W, SUBSAMPLINGS[sub])
    rgb_buf = torch.empty(n_max, H, W, 3, dtype=torch.uint8, device=dev)
    coef_buf = [torch.empty(n_max, mx * my, bpm, 64, dtype=torch.int16, device=dev) for _ in range(n_buf)]
    off_host = [torch.empty(n_max + 1, dtype=torch.int64, pin_memory=True) for _ in range(n_buf)] if piped else None
    dbuf, hbuf, copied = [None, None], [None, None], [None, None]
    side = torch.cuda.Stream(device=dev) if piped else None

    def first(i):
        (a, b), k = spans[i], i % n_buf
        rgb = rgb_buf[:b - a]
        span(a, b, rgb)
        _, offsets, ws = _encode(prov, rgb, quality, sub, restart, coef_buf[k][:b - a])
        if not piped:
            return offsets, ws, None
        off_host[k][:b - a + 1].copy_(offsets, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        return offsets, ws, ev

    def room(bufs, k, n, **kw):
        if bufs[k] is None or bufs[k].numel() < n:
            bufs[k] = torch.empty(n + n // 4, dtype=torch.uint8, **kw)
        return bufs[k][:n]

    pending, done = first(0), None
    for i, (a, b) in enumerate(spans):
        ahead = first(i + 1) if i + 1 < len(spans) else None             # the next render, queued before the wait below
        offsets, ws, ev = pending
        k = i % n_buf
        if ev is not None:
            ev.synchronize()                                             # the sizes of this chunk: the one wait
            off = off_host[k][:b - a + 1].numpy().copy()
        else:
            off = offsets.numpy().copy()
        total = int(off[-1])
        if copied[k] is not None:
            copied[k].synchronize()                                      # the copy that last read this device buffer: two chunks back, long done
        data = room(dbuf, k, total, device=dev)
        prov.jpeg_emit(coef_buf[k][:b - a], H, W, sub, quality, restart, offsets, data, ws)
        if piped:
            host = room(hbuf, k, total, pin_memory=True)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                host.copy_(data, non_blocking=True)
                copied[k] = torch.cuda.Event()
                copied[k].record(side)
        else:
            host = data
        if done is not None:                                             # append the chunk before, under the device's work
            if done[2] is not None:
                done[2].synchronize()
            writer.write(done[0].numpy(), done[1])
        done, pending = (host, off, copied[k]), ahead
    if done[2] is not None:
        done[2].synchronize()
    writer.write(done[0].numpy(), done[1])


def _run(path, fps, F, chunk, size, dev, span, prov, quality, subsampling, restart, where):
    """`size`: an int (square frames) or (H, W)"""
    H, W = (size, size) if isinstance(size, int) else size
    if not isinstance(chunk, int) or not 1 <= chunk <= MAX_FRAMES:
        raise ValueError(f'{where}: chunk must be an int in [1, {MAX_FRAMES}], got {chunk!r}')
    restart = _check_coding(H, W, quality, subsampling, restart, where)
    with MJPEGWriter(path, W, H, fps) as writer:
        if F:
            _video_pipeline(writer, prov, F, chunk, H, W, dev, span, quality, SUBSAMPLINGS.index(subsampling), restart)
        frames = writer.frames
    return frames, writer.bytes


def mesh_video(path, verts, faces, fps: float, quality: int = 90, subsampling: str = '420', restart=None, chunk: int = 32, cube=None, seq_lens=None,
               size: int = 1024, ss: int = 1, color=R.MESH_COLOR, alpha: float = R.MESH_ALPHA, ops=None):
    """The frames of `render.render_mesh(verts, faces, ...)` as the Motion-JPEG AVI file `path` at `fps` frames per second -> (frames, bytes of
    the file).  Each chunk of `chunk` frames is rendered into a device buffer and encoded there; only the compressed bytes are copied to the
    host, under the render of the next chunk.  The cube is that of the whole motion (per track), whatever the chunking."""
    where = 'video.mesh_video'
    _, lens, prov = R._check(verts, faces, cube, seq_lens, size, ss, color, alpha, ('rgb',), ops, where)
    F, dev = verts.shape[0], verts.device
    verts, faces = verts.contiguous(), faces.contiguous()
    if F:
        cube = (R.frame_cube(verts, lens) if cube is None else cube).contiguous()
        ptr = R._seq_ptr(lens, dev)

    def span(a, b, rgb):
        R._render(prov, verts[a:b], faces, cube, (ptr - a).clamp_(0, b - a), size, ss, color, alpha, rgb, ('rgb',))
    return _run(path, fps, F, chunk, size, dev, span, prov, quality, subsampling, restart, where)


def skeleton_video(path, x3d, fps: float, quality: int = 90, subsampling: str = '420', restart=None, chunk: int = 32, size: int = 1024, ss: int = 1,
                   view=None, bones=None, colors=None, radii=None, ops=None):
    """The frames of `render.render_skeleton(x3d, ...)` as the Motion-JPEG AVI file `path` -> (frames, bytes of the file); see `mesh_video`."""
    where = 'video.skeleton_video'
    x3d, view, bones, colors, radii, _, prov = R._check_skeleton(x3d, size, ss, view, bones, colors, radii, ('rgb',), ops, where)

    def span(a, b, rgb):
        R._render_skeleton(prov, x3d[a:b], view, bones, colors, radii, size, ss, rgb, ('rgb',))
    return _run(path, fps, x3d.shape[0], chunk, size, x3d.device, span, prov, quality, subsampling, restart, where)


def scene_video(path, x3d, table, width: int, height: int, fps: float, quality: int = 90, subsampling: str = '420', background=None, chunk: int = 32,
                restart=None, ss: int = 1, bones=None, palette=None, radii=None, ops=None):
    """The frames of `render.render_scene(x3d, table, width, height, ...)` as the Motion-JPEG AVI file `path` -> (frames, bytes of the file): every
    tracked person in one video of the input's size; see `mesh_video`.  Background frames given per video frame are sliced per chunk."""
    where = 'video.scene_video'
    x, tab, bones, palette, radii, background, _, prov = R._check_scene(x3d, table, width, height, ss, bones, palette, radii, background, ('rgb',), ops,
                                                                       where)
    Fv = tab[0].numel() - 1
    jq = R._project_scene(prov, x, ss) if Fv else None

    def span(a, b, rgb):
        R._render_scene(prov, jq, tab, a, b, bones, palette, radii, width, height, ss, background, rgb, ('rgb',))
    return _run(path, fps, Fv, chunk, (height, width), x.device, span, prov, quality, subsampling, restart, where)
