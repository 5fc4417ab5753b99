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

Reading is the other half (csrc/jpeg_dec.hip): the compressed bytes cross the host link and the frames are decoded where they are used.

    parse_jpeg(bytes)                                 the header facts of one baseline JFIF frame, on the host; raises ValueError naming the marker
                                                      of anything the decoder does not take
    decode_jpeg(data, offsets, device)                F files -> rgb uint8 [F,H,W,3] on the device, every pixel the one libjpeg's default path
                                                      decodes (include/mbx.h has the definition); one host synchronisation, the status read.
                                                      entropy='auto' | 'interval' | 'sync': one lane per restart interval, or the parallel
                                                      decode inside an interval (csrc/jpeg_sync.hip) that frames without DRI need
    MJPEGReader(path, entropy)                              RIFF 'AVI ' with an MJPG video stream: `.width .height .fps .frames`, `.read(a, b, device)`,
                                                      `.chunks(chunk, device)` (the upload of the next chunk under the decode of this one)
    scene_video(..., background=reader)               the video's own frames behind the skeletons, decoded chunk by chunk

Not here: inter-frame codecs, optimised Huffman tables when writing, progressive / arithmetic / 12-bit / grayscale / CMYK JPEG, libjpeg's error
recovery (a malformed restart interval raises), AVI beyond 2 GB (OpenDML: not written, refused when read), audio.  `MJPEGReader` opens the
files `MJPEGWriter` writes and gives back their frames; no third-party player or writer (ffmpeg, cv2, imageio) has been available where
this was developed, so files written by ffmpeg are handled by construction (file-specific Huffman tables, frames without DHT, 4:2:2, no
restart markers, file-relative index offsets, `LIST 'rec '`, `JUNK`) and by hand-built variants in the tests, not by a test on such a file.

There is no CPU path: without an injected kernel provider (`ops=`), tensors that are not on a ROCm device raise."""
from __future__ import annotations

import mmap
import re
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


# ------------------------------------------------------------------------------------------------ reading: the header of a frame
DEC_SUBSAMPLINGS = ('444', '420', '422')          # the index is the `sub` of the decoder's C ABI
DEC_STATUS = ('ok', 'the interval ends inside a symbol', 'no such Huffman code', 'a run past coefficient 63', 'whole bytes left over',
              'the restart markers of the frame are not the expected ones')
_MARKERS = {0xc0: 'SOF0', 0xc1: 'SOF1', 0xc2: 'SOF2', 0xc3: 'SOF3', 0xc4: 'DHT', 0xc5: 'SOF5', 0xc6: 'SOF6', 0xc7: 'SOF7', 0xc8: 'JPG', 0xc9: 'SOF9',
            0xca: 'SOF10', 0xcb: 'SOF11', 0xcc: 'DAC', 0xcd: 'SOF13', 0xce: 'SOF14', 0xcf: 'SOF15', 0xd8: 'SOI', 0xd9: 'EOI', 0xda: 'SOS', 0xdb: 'DQT',
            0xdc: 'DNL', 0xdd: 'DRI', 0xde: 'DHP', 0xdf: 'EXP', 0xfe: 'COM', 0x01: 'TEM'}
_NEXT_MARKER = re.compile(rb'\xff[^\x00\xd0-\xd7\xff]')          # inside a scan: 0xFF that is neither stuffed, nor RSTn, nor a fill byte


def _marker(m):
    return _MARKERS.get(m) or (f'APP{m - 0xe0}' if 0xe0 <= m <= 0xef else f'RST{m - 0xd0}' if 0xd0 <= m <= 0xd7 else f'marker {m:#04x}')


def parse_jpeg(data):
    """The header facts of one JPEG file (`bytes`, or anything `bytes()` takes) as the decoder needs them, on the host: a dict with H, W,
    subsampling ('444', '420' or '422'), restart (the interval in MCUs; 0: none), q (uint8 [3,64]: each component's quantisation table in
    zigzag order), dht (uint8 [6,272]: bits [16] and vals [256] of the DC and the AC table of each component; None where the file brings no
    Huffman table, as an AVI 'MJPG' frame may: Annex K applies) and scan = (the first entropy-coded byte, the position of EOI).
    Accepted: baseline sequential (SOF0), 8 bit, three components in one interleaved scan, luma sampling 1x1, 2x1 or 2x2 with chroma 1x1,
    8-bit DQT, DRI or not; APPn and COM are skipped.  Everything else raises ValueError naming the marker: SOF1 and above, DAC (arithmetic
    coding), 12 bit, a 16-bit DQT, one or four components, other sampling factors, a second scan, DNL, no SOI or no EOI."""
    where = 'video.parse_jpeg'
    data = data if isinstance(data, bytes) else data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    if data[:2] != b'\xff\xd8':
        raise ValueError(f'{where}: SOI: the file does not start with it')
    p, q, huff, restart, comps, size = 2, {}, {}, 0, None, None
    while True:
        while p + 1 < len(data) and data[p] == 0xff and data[p + 1] == 0xff:          # fill bytes
            p += 1
        if p + 4 > len(data):
            raise ValueError(f'{where}: SOS: the file ends at byte {len(data)} before a scan')
        if data[p] != 0xff:
            raise ValueError(f'{where}: no marker at byte {p}')
        m, n = data[p + 1], struct.unpack('>H', data[p + 2:p + 4])[0]
        name, seg = _marker(m), data[p + 4:p + 2 + n]
        if m in (0xd8, 0xd9) or 0xd0 <= m <= 0xd7 or m == 0x01:
            raise ValueError(f'{where}: {name} at byte {p}, before a scan')
        if n < 2 or len(seg) != n - 2:
            raise ValueError(f'{where}: {name} at byte {p} runs past the end of the file')
        if m == 0xdb:
            while seg:
                if seg[0] >> 4:
                    raise ValueError(f'{where}: DQT: table {seg[0] & 15} has 16-bit entries')
                if len(seg) < 65 or (seg[0] & 15) > 3:
                    raise ValueError(f'{where}: DQT: a short table, or an id above 3')
                q[seg[0] & 15], seg = np.frombuffer(seg[1:65], np.uint8), seg[65:]
        elif m == 0xc0:
            if comps is not None:
                raise ValueError(f'{where}: SOF0: a second frame header')
            if len(seg) < 6 or seg[0] != 8:
                raise ValueError(f'{where}: SOF0: {seg[0] if seg else "?"} bit samples (8 bit only)')
            if seg[5] != 3 or len(seg) != 15:
                raise ValueError(f'{where}: SOF0: {seg[5]} components (three only)')
            size = struct.unpack('>HH', seg[1:5])
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i], seg[8 + 3 * i]) for i in range(3)]
            if comps[0][1] not in (0x11, 0x21, 0x22) or comps[1][1] != 0x11 or comps[2][1] != 0x11:
                raise ValueError(f'{where}: SOF0: sampling factors {[hex(c[1]) for c in comps]} (luma 1x1, 2x1 or 2x2 with chroma 1x1 only)')
        elif 0xc1 <= m <= 0xcf and m != 0xc4:
            raise ValueError(f'{where}: {name}: only baseline sequential Huffman-coded JPEG (SOF0) is decoded')
        elif m == 0xc4:
            while seg:
                k = sum(seg[1:17])
                if len(seg) < 17 + k or k > 256 or (seg[0] >> 4) > 1 or (seg[0] & 15) > 3:
                    raise ValueError(f'{where}: DHT: a short table, a class above 1 or an id above 3')
                huff[seg[0]], seg = (seg[1:17], seg[17:17 + k]), seg[17 + k:]
        elif m == 0xdd:
            if len(seg) != 2:
                raise ValueError(f'{where}: DRI of {len(seg)} bytes')
            restart = struct.unpack('>H', seg)[0]
        elif m == 0xda:
            if comps is None:
                raise ValueError(f'{where}: SOS before SOF0')
            if not seg or seg[0] != 3 or len(seg) != 10 or [seg[1 + 2 * i] for i in range(3)] != [c[0] for c in comps]:
                raise ValueError(f'{where}: SOS: a scan of {seg[0] if seg else "?"} components (one interleaved scan of the three only)')
            if tuple(seg[7:10]) != (0, 63, 0):
                raise ValueError(f'{where}: SOS: spectral selection {tuple(seg[7:10])} (a baseline scan has 0, 63, 0)')
            select = [seg[2 + 2 * i] for i in range(3)]
            p += 2 + n
            break
        elif m == 0xdc:
            raise ValueError(f'{where}: DNL is not taken')
        elif not (0xe0 <= m <= 0xef or m == 0xfe):
            raise ValueError(f'{where}: {name} at byte {p} is not taken')
        p += 2 + n
    H, W = size
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f'{where}: SOF0: a frame of {H} x {W}: height and width must be in [1, {MAX_SIZE}] (DNL is not taken)')
    for c in comps:
        if c[2] not in q:
            raise ValueError(f'{where}: DQT: table {c[2]} of component {c[0]} is missing')
    dht = None
    if huff:
        dht = np.zeros((6, 272), np.uint8)
        for c, s in enumerate(select):
            for a, key in enumerate((s >> 4, 0x10 | (s & 15))):
                if key not in huff:
                    raise ValueError(f'{where}: DHT: the {"AC" if a else "DC"} table {key & 15} of component {comps[c][0]} is missing')
                bits, vals = huff[key]
                dht[2 * c + a, :16], dht[2 * c + a, 16:16 + len(vals)] = list(bits), list(vals)
    end = _NEXT_MARKER.search(data, p)
    if end is None:
        raise ValueError(f'{where}: EOI: the scan runs to the end of the file')
    if data[end.start() + 1] != 0xd9:
        raise ValueError(f'{where}: {_marker(data[end.start() + 1])} after the scan at byte {end.start()} (one scan only)')
    return dict(H=H, W=W, subsampling={0x11: '444', 0x22: '420', 0x21: '422'}[comps[0][1]], restart=restart, q=np.stack([q[c[2]] for c in comps]),
                dht=dht, scan=(p, end.start()))


def dec_geometry(H: int, W: int, subsampling: str):
    """(MCU columns, MCU rows, blocks per MCU) of a frame that is read"""
    h, v = {'444': (1, 1), '420': (2, 2), '422': (2, 1)}[subsampling]
    return -(-W // (8 * h)), -(-H // (8 * v)), h * v + 2


# ------------------------------------------------------------------------------------------------ reading: frames
def _host_files(data, offsets, where):
    """-> (host uint8 array of all files back to back, int64 offsets [F+1], the device tensor if `data` was one)"""
    if isinstance(data, (list, tuple)):
        if offsets is not None or not all(isinstance(b, (bytes, bytearray, memoryview)) for b in data):
            raise ValueError(f'{where}: a list of frames holds `bytes` and takes no offsets')
        off = np.concatenate([[0], np.cumsum([len(b) for b in data])]).astype(np.int64)
        host = np.empty(int(off[-1]), np.uint8)
        for f, b in enumerate(data):
            host[off[f]:off[f + 1]] = np.frombuffer(b, np.uint8)
        return host, off, None
    if isinstance(data, np.ndarray):
        data = torch.from_numpy(np.ascontiguousarray(data))
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1 or offsets is None:
        raise ValueError(f'{where}: data must be a list of `bytes`, or a 1-D uint8 tensor with offsets [F+1]')
    off = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets).astype(np.int64)
    if off.ndim != 1 or off.size < 1 or off[0] < 0 or off[-1] > data.numel() or (np.diff(off) < 0).any():
        raise ValueError(f'{where}: offsets {off.tolist()[:6]} do not frame files inside {data.numel()} bytes')
    return (data.cpu() if data.is_cuda else data).contiguous().numpy(), off, data.contiguous() if data.is_cuda else None


ENTROPY = ('auto', 'interval', 'sync')


def _entropy_route(entropy, prov, where):
    """`entropy` checked against the provider: 'auto' is 'interval' where the provider has no jpeg_dec_entropy_sync; 'sync' then raises"""
    if entropy not in ENTROPY:
        raise ValueError(f'{where}: entropy must be one of {ENTROPY}, got {entropy!r}')
    if not (hasattr(prov, 'jpeg_dec_entropy_sync') and hasattr(prov, 'jpeg_dec_sync_ws')):
        if entropy == 'sync':
            raise RuntimeError(f"{where}: entropy='sync' needs a provider with jpeg_dec_entropy_sync and jpeg_dec_sync_ws; {type(prov).__name__} has none")
        return 'interval'
    return entropy


def _decode(prov, host, off, dev, dev_data, want, out, where, size=None, entropy='auto'):
    """F files host[off[f]:off[f+1]] -> the dict of `want`.  dev_data: the same bytes on the device where they are there already, else they
    are uploaded here, once.  Consecutive frames that share geometry, quantisation and Huffman tables and restart interval go through the
    kernels together.  Nothing is launched before every header is parsed; the ONE host synchronisation is the read of the status."""
    F = len(off) - 1
    facts = [parse_jpeg(host[off[f]:off[f + 1]]) for f in range(F)]
    if F and any((p['H'], p['W']) != (facts[0]['H'], facts[0]['W']) for p in facts):
        raise ValueError(f'{where}: the frames have different sizes: {sorted({(p["H"], p["W"]) for p in facts})}')
    if F and size is not None and (facts[0]['H'], facts[0]['W']) != tuple(size):
        raise ValueError(f'{where}: frames of {facts[0]["H"]} x {facts[0]["W"]} where {size[0]} x {size[1]} are expected')
    H, W = (facts[0]['H'], facts[0]['W']) if F else (size or (0, 0))
    if out is None:
        out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (F, H, W, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f'{where}: out must be a contiguous uint8 tensor [{F},{H},{W},3] on {dev}')
    res = dict(rgb=out, coef=None, status=None, pos=None, route=None)
    entropy = _entropy_route(entropy, prov, where)
    if F == 0:
        return {k: res[k] for k in want}

    def key(p):
        return (p['subsampling'], p['restart'], p['q'].tobytes(), None if p['dht'] is None else p['dht'].tobytes())
    groups, a = [], 0
    for f in range(1, F + 1):
        if f == F or key(facts[f]) != key(facts[a]):
            groups.append((a, f))
            a = f
    if len(groups) > 1 and any(k in want for k in ('coef', 'status', 'pos', 'route')):
        raise ValueError(f'{where}: the test hooks {want!r} need frames that share subsampling, tables and restart interval')
    tables = [prov.jpeg_dec_tables(facts[a]['dht']) for a, _ in groups]              # host; a bad table raises before any launch
    scans = np.array([[off[f] + p['scan'][0], off[f] + p['scan'][1]] for f, p in enumerate(facts)], np.int64)
    if dev_data is None:
        dev_data = torch.from_numpy(host).to(dev, non_blocking=True) if dev.type == 'cuda' else torch.from_numpy(host)
    scans_dev = torch.from_numpy(scans).to(dev)
    stats, routes = [], []
    for (a, b), tab in zip(groups, tables):
        p = facts[a]
        sub = DEC_SUBSAMPLINGS.index(p['subsampling'])
        mx, my, bpm = dec_geometry(H, W, p['subsampling'])
        n_int = -(-mx * my // p['restart']) if p['restart'] else 1
        pos = torch.empty(b - a, n_int + 1, dtype=torch.int64, device=dev)
        status = torch.empty(b - a, n_int, dtype=torch.int32, device=dev)
        coef = torch.empty(b - a, mx * my, bpm, 64, dtype=torch.int16, device=dev)
        prov.jpeg_dec_index(dev_data, scans_dev[a:b], n_int, pos, status)
        route = torch.zeros(b - a, n_int, dtype=torch.int32, device=dev)
        if entropy == 'sync' or (entropy == 'auto' and n_int == 1):      # a frame that is one interval would be one lane of the other route
            longest = max(q['scan'][1] - q['scan'][0] for q in facts[a:b])          # the host's parsed scan lengths bound every interval
            prov.jpeg_dec_entropy_sync(dev_data, pos, tab.to(dev), H, W, sub, p['restart'], longest, coef, status, route,
                                       prov.jpeg_dec_sync_ws(b - a, n_int, longest, dev))
        else:
            prov.jpeg_dec_entropy(dev_data, pos, tab.to(dev), H, W, sub, p['restart'], coef, status)
        if 'rgb' in want:
            prov.jpeg_dec_pixels(coef, p['q'], H, W, sub, out[a:b], prov.jpeg_dec_ws(b - a, H, W, sub, dev))
        stats.append(status)
        routes.append(route)
        res.update(coef=coef, status=status, pos=pos)
    both = torch.cat([s.reshape(-1) for s in stats + routes]).cpu().numpy()           # the one host synchronisation: status and route together
    flat = both[:both.size // 2]
    if 'route' in want:
        res['route'] = torch.from_numpy(both[both.size // 2:].reshape(routes[-1].shape).copy())
    if flat.any() and 'status' not in want:
        i = int(np.nonzero(flat)[0][0])
        for (a, b), s in zip(groups, stats):
            if i < s.numel():
                raise ValueError(f'{where}: frame {a + i // s.shape[1]}, restart interval {i % s.shape[1]} of {s.shape[1]}: status {flat[i]} '
                                 f'({DEC_STATUS[flat[i]] if 0 <= flat[i] < len(DEC_STATUS) else "unknown"}); {int((flat != 0).sum())} intervals in all')
            i, flat = i - s.numel(), flat[s.numel():]
    return {k: res[k] for k in want}


def decode_jpeg(data, offsets=None, device=None, want=('rgb',), out=None, ops=None, entropy='auto'):
    """F baseline JPEG files -> rgb uint8 [F,H,W,3] on the device, every pixel the one libjpeg's default path decodes.  `data`: a list of
    `bytes`, or a 1-D uint8 tensor or array (host or device) that holds the files back to back with `offsets` [F+1]; all frames must have
    one size; what `parse_jpeg` refuses raises before anything is launched.  `device`: where to decode (default: that of a device tensor,
    else the current ROCm device).  Host bytes are uploaded once; a device tensor is also read back once, for its headers.  With the
    default `want` the result is the rgb tensor (`out`, where one is given); any other `want` gives a dict: 'coef' (int16 [F, n_mcu, blocks
    per MCU, 64], zigzag: the encoder's layout), 'pos', 'status' (then a malformed interval does not raise) and 'route' (int32 [F, n_int] on
    the host: how mbx_jpeg_dec_entropy_sync decoded each interval, zeros on the other route) are test hooks.  `entropy`: 'interval' decodes
    one restart interval per lane; 'sync' decodes inside the intervals in parallel (csrc/jpeg_sync.hip), with the same result for every
    input; 'auto' takes 'sync' for the frames that are one interval (no DRI, or one that covers the frame), 'interval' otherwise and where
    the provider has no jpeg_dec_entropy_sync.  ONE host synchronisation, the read of the status (and route): an interval that is malformed
    raises ValueError naming frame, interval and code."""
    where = 'video.decode_jpeg'
    plain = want == ('rgb',) or want == 'rgb'
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in ('rgb', 'coef', 'status', 'pos', 'route') for k in want):
        raise ValueError(f"{where}: want must name some of ('rgb', 'coef', 'status', 'pos', 'route'), got {want!r}")
    host, off, dev_data = _host_files(data, offsets, where)
    device = _dec_device(dev_data.device if device is None and dev_data is not None else device, ops, where)
    if dev_data is not None and dev_data.device != device:
        dev_data = None
    prov = hip_ops.provider(ops, 'motionbert_amd.' + where)
    res = _decode(prov, host, off, device, dev_data, want, out, where, entropy=entropy)
    return res['rgb'] if plain else res


# ------------------------------------------------------------------------------------------------ reading: the container
class MJPEGReader:
    """The Motion-JPEG video stream of an AVI 1.0 file.  The constructor walks RIFF 'AVI ': `avih`, the first `strl` whose `strh` is 'vids' with
    handler or compression 'MJPG' (either case) and its `strf`; other streams are ignored.  The frames are located through `idx1` (offsets
    relative to the 'movi' fourcc or to the file: whichever names the stream's chunk, as players decide it), or by walking `movi` when there
    is no index; `LIST 'rec '` is descended, `JUNK` and everything else skipped; a chunk of length 0 repeats the frame before it.
    `.width .height .fps .frames`; `.frame_bytes(f)`; `.read(a, b, device)` -> uint8 [b - a, height, width, 3] on the device;
    `.chunks(chunk, device)` yields them `chunk` at a time.  `entropy`: as `decode_jpeg`'s, for every read.  A context manager.  OpenDML files
    (a RIFF 'AVIX' after the first) are refused."""

    def __init__(self, path, entropy='auto'):
        if entropy not in ENTROPY:
            raise ValueError(f'MJPEGReader: entropy must be one of {ENTROPY}, got {entropy!r}')
        self.path, self.entropy = path, entropy
        self.file = open(path, 'rb')
        try:
            self.map = mmap.mmap(self.file.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:
            self.file.close()
            raise ValueError(f'MJPEGReader: {path} is empty')
        try:
            self._walk()
        except Exception:
            self.close()
            raise

    def _chunks(self, a, b):
        """(fourcc, payload start, size as the chunk states it) of the chunks in [a, b)"""
        d = self.map
        while a + 8 <= b:
            cid, size = d[a:a + 4], struct.unpack('<I', d[a + 4:a + 8])[0]
            yield cid, a + 8, size
            a += 8 + size + (size & 1)

    def _walk(self):
        d, n = self.map, len(self.map)
        if n < 12 or d[:4] != b'RIFF' or d[8:12] != b'AVI ':
            raise ValueError(f'MJPEGReader: {self.path} is no RIFF \'AVI \' file')
        end = min(n, 8 + struct.unpack('<I', d[4:8])[0])
        for cid, at, size in self._chunks(end + (end & 1), n):
            if cid == b'RIFF' and d[at:at + 4] == b'AVIX':
                raise ValueError(f'MJPEGReader: {self.path} is an OpenDML file (RIFF \'AVIX\'); only AVI 1.0 is read')
        avih = stream = strf = movi = idx1 = None
        n_streams = 0
        for cid, at, size in self._chunks(12, end):
            if cid == b'LIST' and d[at:at + 4] == b'hdrl':
                for c2, a2, s2 in self._chunks(at + 4, min(at + size, end)):
                    if c2 == b'avih':
                        avih = d[a2:a2 + s2]
                    elif c2 == b'LIST' and d[a2:a2 + 4] == b'strl':
                        strh = fmt = None
                        for c3, a3, s3 in self._chunks(a2 + 4, min(a2 + s2, end)):
                            strh, fmt = (d[a3:a3 + s3], fmt) if c3 == b'strh' else (strh, d[a3:a3 + s3]) if c3 == b'strf' else (strh, fmt)
                        if stream is None and strh is not None and len(strh) >= 36 and strh[:4] == b'vids':
                            codecs = {strh[4:8].upper(), fmt[16:20].upper() if fmt is not None and len(fmt) >= 20 else b''}
                            if b'MJPG' not in codecs:
                                raise ValueError(f'MJPEGReader: the video stream of {self.path} is {strh[4:8]!r} / '
                                                 f'{fmt[16:20] if fmt is not None else b""!r}, not MJPG')
                            stream, strf, head = n_streams, fmt, strh
                        n_streams += 1
            elif cid == b'LIST' and d[at:at + 4] == b'movi':
                movi = (at, min(at + size, end))                                   # from the 'movi' fourcc to the end of the list
            elif cid == b'idx1':
                idx1 = (at, min(size, end - at))
        if stream is None or movi is None:
            raise ValueError(f'MJPEGReader: {self.path} has no MJPG video stream, or no \'movi\' list')
        scale, rate = struct.unpack('<II', head[20:28])
        if scale == 0 or rate == 0:
            if avih is None or len(avih) < 4 or struct.unpack('<I', avih[:4])[0] == 0:
                raise ValueError(f'MJPEGReader: {self.path} names no frame rate')
            scale, rate = struct.unpack('<I', avih[:4])[0], 1000000
        self.fps = rate / scale
        if strf is not None and len(strf) >= 12:
            w, h = struct.unpack('<ii', strf[4:12])
            self.width, self.height = w, abs(h)
        elif avih is not None and len(avih) >= 40:
            self.width, self.height = struct.unpack('<II', avih[32:40])
        else:
            raise ValueError(f'MJPEGReader: {self.path} names no frame size')
        ids = (b'%02ddc' % stream, b'%02ddb' % stream)
        self.index = []                                                  # (start, size) of every frame's payload in the file
        if idx1 is not None and idx1[1] >= 16:
            ent = np.frombuffer(d[idx1[0]:idx1[0] + idx1[1] - idx1[1] % 16], np.dtype([('id', 'S4'), ('flags', '<u4'), ('at', '<u4'), ('size', '<u4')]))
            ent = ent[(ent['id'] == ids[0]) | (ent['id'] == ids[1])]
            if len(ent):
                first = int(ent['at'][0])
                if d[movi[0] + first:movi[0] + first + 4] in ids:
                    base = movi[0]
                elif d[first:first + 4] in ids:
                    base = 0
                else:
                    raise ValueError(f'MJPEGReader: the index of {self.path} points at no chunk of the video stream, relative to \'movi\' or to the file')
                self.index = [(base + int(a) + 8, int(s)) for a, s in zip(ent['at'], ent['size'])]
        else:
            def walk(a, b):
                for cid, at, size in self._chunks(a, b):
                    if cid == b'LIST' and d[at:at + 4] == b'rec ':
                        walk(at + 4, min(at + size, b))
                    elif cid in ids:
                        self.index.append((at, size))
            walk(movi[0] + 4, movi[1])
        for f, (at, size) in enumerate(self.index):
            if at + size > n:
                raise ValueError(f'MJPEGReader: frame {f} of {self.path} ({size} bytes at {at}) runs past the end of the file')
            if size == 0:
                if f == 0:
                    raise ValueError(f'MJPEGReader: the first frame of {self.path} is empty')
                self.index[f] = self.index[f - 1]
        self.frames = len(self.index)
        if self.frames > 0 and not (1 <= self.width <= MAX_SIZE and 1 <= self.height <= MAX_SIZE):
            raise ValueError(f'MJPEGReader: frames of {self.height} x {self.width}: height and width must be in [1, {MAX_SIZE}]')

    def frame_bytes(self, f: int) -> bytes:
        at, size = self.index[f]
        return self.map[at:at + size]

    def _span(self, a, b, where):
        if not (isinstance(a, int) and isinstance(b, int) and 0 <= a <= b <= self.frames):
            raise ValueError(f'{where}: frames {a!r} .. {b!r} of {self.frames}')
        if self.map is None:
            raise ValueError(f'{where}: the file is closed')

    def _gather(self, a, b, buf=None):
        """the payloads of frames a .. b - 1 back to back -> (host uint8 array, offsets); into the pinned tensor `buf` where it is large enough"""
        off = np.concatenate([[0], np.cumsum([self.index[f][1] for f in range(a, b)])]).astype(np.int64)
        host = np.empty(int(off[-1]), np.uint8) if buf is None else buf.numpy()[:int(off[-1])]
        for f in range(a, b):
            at, size = self.index[f]
            host[off[f - a]:off[f - a + 1]] = np.frombuffer(self.map, np.uint8, size, at)
        return host, off

    def read(self, a: int = 0, b=None, device=None, out=None, ops=None):
        """frames a .. b - 1 (default: to the end) -> uint8 [b - a, height, width, 3] on the device (`out` where given)"""
        where = 'video.MJPEGReader.read'
        b = self.frames if b is None else b
        self._span(a, b, where)
        device = _dec_device(device, ops, where)
        host, off = self._gather(a, b)
        return _decode(hip_ops.provider(ops, 'motionbert_amd.' + where), host, off, device, None, ('rgb',), out, where, (self.height, self.width),
                       self.entropy)['rgb']

    def chunks(self, chunk: int = 32, device=None, ops=None):
        """A generator of device tensors uint8 [n, height, width, 3], n <= `chunk` frames at a time, in frame order.  The structure of
        render._pipeline turned round: the compressed bytes of chunk i + 1 are gathered into one of two pinned buffers and uploaded on a
        side stream under the decode of chunk i.  A tensor is valid until the generator is advanced twice."""
        where = 'video.MJPEGReader.chunks'
        if not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f'{where}: chunk must be a positive int, got {chunk!r}')
        device = _dec_device(device, ops, where)
        prov = hip_ops.provider(ops, 'motionbert_amd.' + where)
        spans = [(a, min(a + chunk, self.frames)) for a in range(0, self.frames, chunk)]
        self._span(0, self.frames, where)
        piped = device.type == 'cuda'
        room = max((sum(self.index[f][1] for f in range(a, b)) for a, b in spans), default=0)
        n_buf = min(2, len(spans))
        hbuf = [torch.empty(room, dtype=torch.uint8, pin_memory=piped) for _ in range(n_buf)]
        dbuf = [torch.empty(room, dtype=torch.uint8, device=device) for _ in range(n_buf)] if piped else hbuf
        rgb = [torch.empty(min(chunk, self.frames), self.height, self.width, 3, dtype=torch.uint8, device=device) for _ in range(n_buf)]
        side = torch.cuda.Stream(device=device) if piped else None

        def upload(i):
            (a, b), k = spans[i], i % n_buf
            host, off = self._gather(a, b, hbuf[k])                      # the decode that last read dbuf[k] has been waited for (its status)
            if not piped:
                return host, off, None
            with torch.cuda.stream(side):
                dbuf[k][:host.size].copy_(hbuf[k][:host.size], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
            return host, off, ev

        ahead = upload(0) if spans else None
        for i, (a, b) in enumerate(spans):
            (host, off, ev), k = ahead, i % n_buf
            ahead = upload(i + 1) if i + 1 < len(spans) else None
            if ev is not None:
                torch.cuda.current_stream(device).wait_event(ev)
            yield _decode(prov, host, off, device, dbuf[k][:host.size], ('rgb',), rgb[k][:b - a], where, (self.height, self.width), self.entropy)['rgb']

    def close(self):
        if getattr(self, 'map', None) is not None:
            self.map.close()
            self.map = None
        self.file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _dec_device(device, ops, where):
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device()) if ops is None and torch.cuda.is_available() else torch.device('cpu')
    device = torch.device(device)
    if ops is None and device.type != 'cuda':
        raise RuntimeError(f'motionbert_amd.{where} runs on the ROCm device; there is no CPU path')
    if device.type == 'cuda' and device.index is None:                   # 'cuda' and 'cuda:0' compare unequal
        device = torch.device('cuda', torch.cuda.current_device())
    return device


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
    tracked person in one video of the input's size; see `mesh_video`.  Background frames given per video frame are sliced per chunk; an
    `MJPEGReader` as `background` (the input video: as many frames, of this size) is decoded chunk by chunk into one chunk-sized buffer just
    before the chunk's render, so the whole background never exists on the device."""
    where = 'video.scene_video'
    x, tab, bones, palette, radii, background, _, prov = R._check_scene(x3d, table, width, height, ss, bones, palette, radii, background, ('rgb',), ops,
                                                                       where)
    Fv = tab[0].numel() - 1
    jq = R._project_scene(prov, x, ss) if Fv else None

    def span(a, b, rgb):
        R._render_scene(prov, jq, tab, a, b, bones, palette, radii, width, height, ss, background, rgb, ('rgb',))
    return _run(path, fps, Fv, chunk, (height, width), x.device, span, prov, quality, subsampling, restart, where)
