"""Baseline JPEG as libjpeg writes it by default, restated in numpy: the reference of csrc/jpeg.hip and motionbert_amd/video.py.

Every stage is integer arithmetic, so the gate is byte equality with libjpeg-turbo's own file (tests/golden/jpeg_pil.npz, minted by
tools/mint_jpeg.py from Pillow with optimize=False); there is no tolerance anywhere.

    front(rgb, quality, sub)              rgb uint8 [H,W,3] -> quantised coefficients int16 [n_mcu, blocks_per_mcu, 64], zigzag, MCU order
    scan(coef, sub, restart)              -> the entropy-coded bytes of the scan (restart intervals joined by RSTn)
    header(H, W, quality, sub, restart)   -> SOI .. SOS as libjpeg writes them
    encode(rgb, quality, sub, restart)    -> the complete file
    parse(file)                           -> the header's fields, the scan's bytes and the decoded coefficients
    riff(file)                            -> the chunk tree of an AVI file
    gate_files / gate_equal               -> messages (none passes) that name the frame, the restart interval and the first differing byte
    RefOps                                -> the kernel provider of motionbert_amd.video on host tensors

`corrupt` names seeded errors (CORRUPTIONS); each must fail a gate (tests/test_jpegerr.py)."""
import struct

import numpy as np
import torch

CORRUPTIONS = ('bias_swapped', 'replicate_first', 'dummy_transformed', 'half_even', 'no_stuffing', 'rst_not_mod8', 'pred_not_reset',
               'pad_zero', 'eob_after_63', 'zrl_trailing')

# ------------------------------------------------------------------------------------------------ tables (ITU-T T.81 Annex K)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFF = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)          # in the order of the header's DHT segments


def derive(bits, vals):
    """canonical codes: (code, size) per symbol, size 0 where the table has no code"""
    code, size, c, k = np.zeros(256, np.int64), np.zeros(256, np.int64), 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c, k = c + 1, k + 1
        c <<= 1
    return code, size


DERIVED = tuple(derive(*t) for t in HUFF)


def sub_code(subsampling):
    if subsampling not in ('420', '444'):
        raise ValueError(f"subsampling must be '420' or '444', got {subsampling!r}")
    return 1 if subsampling == '420' else 0


def geometry(H, W, sub):
    """(MCU columns, MCU rows, blocks per MCU) of a frame; sub: '420' or '444'"""
    m = 16 if sub == '420' else 8
    return -(-W // m), -(-H // m), 6 if sub == '420' else 3


def default_restart(H, W, sub):
    return geometry(H, W, sub)[0]


def quant_tables(quality):
    """[2,64] in natural order: luminance, chrominance, scaled the IJG way"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((t * s + 50) // 100, 1, 255) for t in (Q_LUMA, Q_CHROMA)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ front stage
C = dict(c298=2446, c390=3196, c541=4433, c765=6270, c899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069, c2053=16819, c2562=20995,
         c3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """one pass of the slow-integer DCT along the last axis (int64 [...,8])"""
    n = 11 if first else 15
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * C['c541']
    o[2] = _descale(z1 + t13 * C['c765'], n)
    o[6] = _descale(z1 - t12 * C['c1847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C['c1175']
    t4, t5, t6, t7 = t4 * C['c298'], t5 * C['c2053'], t6 * C['c3072'], t7 * C['c1501']
    z1, z2, z3, z4 = -z1 * C['c899'], -z2 * C['c2562'], -z3 * C['c1961'] + z5, -z4 * C['c390'] + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(blocks):
    """samples [...,8,8] (0..255) -> coefficients scaled by 8, int64: rows first, then columns"""
    d = _pass(blocks.astype(np.int64) - 128, True)
    return np.swapaxes(_pass(np.swapaxes(d, -1, -2), False), -1, -2)


def quantise(c, q, corrupt=()):
    """c [...,64] natural order scaled by 8, q [64] -> sign(c) ((|c| + (8 q >> 1)) / (8 q))"""
    q8, a = 8 * q, np.abs(c)
    r = (a + (q8 >> 1)) // q8
    if 'half_even' in corrupt:
        r = r - (((2 * a + q8) % (2 * q8) == 0) & (r % 2 == 1))
    return np.where(c < 0, -r, r)


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)          # [by, bx, 8, 8]


def _edge(plane, h, w):
    return np.pad(plane, ((0, h - plane.shape[0]), (0, w - plane.shape[1])), mode='edge')


def front(rgb, quality, sub, corrupt=()):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    mx, my, bpm = geometry(H, W, sub)
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    Y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    Cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    Cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    q = quant_tables(quality)

    def coefs(plane, table):
        c = fdct(_blocks(plane)).reshape(plane.shape[0] // 8, plane.shape[1] // 8, 64)
        return quantise(c, q[table], corrupt)[..., ZIGZAG]

    if sub == '444':
        planes = [coefs(_edge(p, 8 * my, 8 * mx), int(k > 0)) for k, p in enumerate((Y, Cb, Cr))]
        return np.stack(planes, 2).reshape(mx * my, 3, 64).astype(np.int16)
    y = coefs(_edge(Y, 16 * my, 16 * mx), 0)                              # [2 my, 2 mx, 64]
    if 'dummy_transformed' not in corrupt:
        nbx, nby = -(-W // 8), -(-H // 8)
        y = y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64).copy()
        if nbx < 2 * mx:                                                  # the last block column is beyond the image
            y[:, -1, 1], y[:, -1, 3] = 0, 0
            y[:, -1, 1, 0], y[:, -1, 3, 0] = y[:, -1, 0, 0], y[:, -1, 2, 0]
        if nby < 2 * my:                                                  # the last block row: both take the DC of the block before the row
            y[-1, :, 2:] = 0
            y[-1, :, 2, 0] = y[-1, :, 3, 0] = y[-1, :, 1, 0]
    else:
        y = y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
    bias = np.tile([2, 1] if 'bias_swapped' in corrupt else [1, 2], 4 * mx)

    def chroma(p):
        p = _edge(p, 16 * my if 'replicate_first' in corrupt else H + (H & 1), 16 * mx)
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        return coefs(_edge(d, 8 * my, 8 * mx), 1)                        # [my, mx, 64]
    mcu = np.concatenate([y, chroma(Cb)[:, :, None], chroma(Cr)[:, :, None]], 2)
    return mcu.reshape(mx * my, 6, 64).astype(np.int16)


# ------------------------------------------------------------------------------------------------ entropy coder
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, size):
        self.acc, self.n = (self.acc << size) | code, self.n + size
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xff)
        self.acc &= (1 << self.n) - 1

    def flush(self, ones=True):
        if self.n:
            self.put((1 << (8 - self.n)) - 1 if ones else 0, 8 - self.n)


def _magnitude(v):
    """(category, the bits that follow the code)"""
    nb = int(abs(v)).bit_length()
    return nb, (v if v >= 0 else v - 1) & ((1 << nb) - 1)


def _component(k, bpm):
    return (0 if k < 4 else k - 3) if bpm == 6 else k


def encode_block(bw, blk, pred, dc, ac, corrupt=()):
    """one block of 64 zigzag coefficients into the bit writer; returns its DC"""
    nb, extra = _magnitude(int(blk[0]) - pred)
    assert nb <= 11 and dc[1][nb], 'DC difference outside the baseline range'
    bw.put(int(dc[0][nb]), int(dc[1][nb]))
    bw.put(extra, nb)
    run = 0
    nz = np.nonzero(blk[1:])[0] + 1
    last = 0
    for k in nz:
        run = int(k) - last - 1
        last = int(k)
        while run >= 16:
            bw.put(int(ac[0][0xf0]), int(ac[1][0xf0]))
            run -= 16
        nb, extra = _magnitude(int(blk[k]))
        assert nb <= 10, 'AC coefficient outside the baseline range'
        bw.put(int(ac[0][run << 4 | nb]), int(ac[1][run << 4 | nb]))
        bw.put(extra, nb)
    if last < 63:
        if 'zrl_trailing' in corrupt:
            for _ in range((63 - last) // 16):
                bw.put(int(ac[0][0xf0]), int(ac[1][0xf0]))
        bw.put(int(ac[0][0]), int(ac[1][0]))
    elif 'eob_after_63' in corrupt:
        bw.put(int(ac[0][0]), int(ac[1][0]))
    return int(blk[0])


def intervals(coef, restart, corrupt=()):
    """coef [n_mcu, bpm, 64] -> the stuffed, padded bytes of every restart interval"""
    n_mcu, bpm = coef.shape[:2]
    out, pred = [], [0, 0, 0]
    for a in range(0, n_mcu, restart):
        bw = _Bits()
        if 'pred_not_reset' not in corrupt:
            pred = [0, 0, 0]
        for m in range(a, min(a + restart, n_mcu)):
            for k in range(bpm):
                c = _component(k, bpm)
                pred[c] = encode_block(bw, coef[m, k], pred[c], DERIVED[2 * (c > 0)], DERIVED[2 * (c > 0) + 1], corrupt)
        bw.flush('pad_zero' not in corrupt)
        raw = bytes(bw.out)
        out.append(raw if 'no_stuffing' in corrupt else raw.replace(b'\xff', b'\xff\x00'))
    return out


def join(parts, corrupt=()):
    out = bytearray()
    for i, p in enumerate(parts):
        if i:
            out += bytes([0xff, 0xd0 + ((i - 1) if 'rst_not_mod8' in corrupt else (i - 1) % 8)])
        out += p
    return bytes(out)


def scan(coef, restart, corrupt=()):
    return join(intervals(coef, restart, corrupt), corrupt)


# ------------------------------------------------------------------------------------------------ header and file
def header(H, W, quality, sub, restart):
    q = quant_tables(quality)
    out = bytearray(b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(2):
        out += b'\xff\xdb\x00\x43' + bytes([t]) + bytes(int(v) for v in q[t][ZIGZAG])
    out += b'\xff\xc0\x00\x11\x08' + struct.pack('>HH', H, W) + b'\x03' + bytes([1, 0x22 if sub == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for (bits, vals), tc in zip(HUFF, (0x00, 0x10, 0x01, 0x11)):
        out += b'\xff\xc4' + struct.pack('>H', 19 + len(vals)) + bytes([tc]) + bytes(bits) + bytes(vals)
    out += b'\xff\xdd\x00\x04' + struct.pack('>H', restart)
    out += b'\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'
    return bytes(out)


def check_params(H, W, quality, sub, restart):
    sub_code(sub)
    if not (1 <= H <= 2048 and 1 <= W <= 2048 and 1 <= quality <= 100 and 1 <= restart <= 65535):
        raise ValueError(f'bad JPEG parameters H={H} W={W} quality={quality} restart={restart}')


def encode(rgb, quality=90, sub='420', restart=None, corrupt=()):
    H, W = rgb.shape[:2]
    restart = default_restart(H, W, sub) if restart is None else restart
    check_params(H, W, quality, sub, restart)
    return header(H, W, quality, sub, restart) + scan(front(rgb, quality, sub, corrupt), restart, corrupt) + b'\xff\xd9'


def encode_frames(rgb, quality=90, sub='420', restart=None):
    """rgb [F,H,W,3] -> (data uint8 [total], offsets int64 [F+1])"""
    files = [encode(f, quality, sub, restart) for f in rgb]
    return np.frombuffer(b''.join(files), np.uint8).copy(), np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ parser and entropy decoder
def parse(data, decode=True):
    """a baseline JFIF file of three components as this encoder (or libjpeg) writes it -> dict: H, W, sub, restart, q [2,64] (zigzag order),
    huff (the four (bits, vals) in file order), header_len, scan (bytes between SOS and EOI), intervals (the scan split at RSTn) and, with
    `decode`, coef [n_mcu, bpm, 64]"""
    data = bytes(data)
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9', 'no SOI / EOI'
    res, p, q, huff = dict(restart=0), 2, {}, []
    while True:
        assert data[p] == 0xff, f'no marker at {p}'
        m, n = data[p + 1], struct.unpack('>H', data[p + 2:p + 4])[0]
        seg = data[p + 4:p + 2 + n]
        if m == 0xdb:
            q[seg[0]] = np.frombuffer(seg[1:65], np.uint8).astype(np.int64)
        elif m == 0xc0:
            assert seg[0] == 8 and seg[5] == 3, 'not 8-bit, three components'
            res['H'], res['W'] = struct.unpack('>HH', seg[1:5])
            res['sub'] = {0x22: '420', 0x11: '444'}[seg[7]]
            assert seg[10] == 0x11 and seg[13] == 0x11
        elif m == 0xc4:
            huff.append((seg[0], list(seg[1:17]), list(seg[17:])))
        elif m == 0xdd:
            res['restart'] = struct.unpack('>H', seg)[0]
        elif m == 0xda:
            p += 2 + n
            break
        else:
            assert m in (0xe0,), f'unexpected marker {m:#x}'
        p += 2 + n
    res.update(q=np.stack([q[0], q[1]]), huff=huff, header_len=p, scan=data[p:-2])
    parts, a, s = [], 0, res['scan']
    i = s.find(b'\xff')
    while i >= 0:
        if 0xd0 <= s[i + 1] <= 0xd7:
            parts.append((s[a:i], s[i + 1] - 0xd0))
            a = i + 2
        i = s.find(b'\xff', i + 2)
    parts.append((s[a:], None))
    res['intervals'] = [x for x, _ in parts]
    res['rst'] = [n for _, n in parts[:-1]]
    if decode:
        res['coef'] = decode_scan(res)
    return res


def decode_scan(res):
    mx, my, bpm = geometry(res['H'], res['W'], res['sub'])
    n_mcu = mx * my
    restart = res['restart'] or n_mcu
    look = {}
    for tc, bits, vals in res['huff']:
        code, size = derive(bits, vals)
        look[tc] = {(int(size[v]), int(code[v])): v for v in vals}
    coef = np.zeros((n_mcu, bpm, 64), np.int16)
    assert len(res['intervals']) == -(-n_mcu // restart), 'interval count'
    for i, raw in enumerate(res['intervals']):
        raw = raw.replace(b'\xff\x00', b'\xff')
        word, nbits, pos = int.from_bytes(raw, 'big'), 8 * len(raw), 0

        def take(n):
            nonlocal pos
            pos += n
            assert pos <= nbits, 'the interval ends inside a symbol'
            return (word >> (nbits - pos)) & ((1 << n) - 1)

        def symbol(table):
            c = 0
            for length in range(1, 17):
                c = (c << 1) | take(1)
                if (length, c) in table:
                    return table[(length, c)]
            raise AssertionError('no Huffman code')

        def extend(v, n):
            return v if n == 0 or v >> (n - 1) else v - (1 << n) + 1
        pred = [0, 0, 0]
        for m in range(i * restart, min((i + 1) * restart, n_mcu)):
            for k in range(bpm):
                c = _component(k, bpm)
                n = symbol(look[c > 0])
                pred[c] += extend(take(n), n)
                coef[m, k, 0] = pred[c]
                z = 1
                while z < 64:
                    rs = symbol(look[0x10 | (c > 0)])
                    if rs == 0:
                        break
                    z += rs >> 4
                    if rs & 15:
                        coef[m, k, z] = extend(take(rs & 15), rs & 15)
                    z += 1
        rem = nbits - pos
        assert rem < 8 and take(rem) == (1 << rem) - 1, 'an interval is not padded with 1-bits to a byte'
    return coef


# ------------------------------------------------------------------------------------------------ AVI
LISTS = (b'RIFF', b'LIST')


def riff(data, a=0, b=None):
    """the chunks of data[a:b] as a list of dicts: id, offset (of the chunk's fourcc), size, and for RIFF / LIST `form` and `chunks`, else
    `data`.  Raises where a chunk runs past its parent."""
    b = len(data) if b is None else b
    out = []
    while a < b:
        assert a + 8 <= b, f'chunk header at {a} runs past {b}'
        cid, size = data[a:a + 4], struct.unpack('<I', data[a + 4:a + 8])[0]
        assert a + 8 + size <= b, f'chunk {cid!r} at {a} with {size} bytes runs past {b}'
        ch = dict(id=cid, offset=a, size=size)
        if cid in LISTS:
            ch['form'] = data[a + 8:a + 12]
            ch['chunks'] = riff(data, a + 12, a + 8 + size)
        else:
            ch['data'] = data[a + 8:a + 8 + size]
        out.append(ch)
        a += 8 + size + (size & 1)
    return out


# ------------------------------------------------------------------------------------------------ gates
def gate_equal(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return [f'{name}: {got.shape} {got.dtype} against {ref.shape} {ref.dtype}']
    bad = np.nonzero((got != ref).reshape(-1))[0]
    return [f'{name}: {len(bad)} of {ref.size} elements differ, the first at {np.unravel_index(bad[0], ref.shape)}: {got.reshape(-1)[bad[0]]} '
            f'against {ref.reshape(-1)[bad[0]]}'] if len(bad) else []


def gate_file(name, got, ref):
    """two complete files: no message where every byte agrees, else where the first difference lies"""
    got, ref = bytes(got), bytes(ref)
    if got == ref:
        return []
    n = next((i for i, (x, y) in enumerate(zip(got, ref)) if x != y), min(len(got), len(ref)))
    where = f'byte {n} (lengths {len(got)} against {len(ref)})'
    try:
        p = parse(ref, decode=False)
        if n < p['header_len']:
            where += ', in the header'
        else:
            at, k = p['header_len'], 0
            for k, part in enumerate(p['intervals']):
                if n < at + len(part) + 2:
                    break
                at += len(part) + 2
            where += f', restart interval {k} of {len(p["intervals"])}, byte {n - at} of its {len(p["intervals"][k])}'
    except Exception as e:                                                # the reference itself does not parse: still name the byte
        where += f' (reference not parsed: {e})'
    return [f'{name}: differs at {where}']


def gate_files(name, data, offsets, refs):
    """F files back to back against a list of reference files"""
    data, offsets = np.asarray(data), np.asarray(offsets)
    if offsets.shape != (len(refs) + 1,) or offsets[0] != 0 or offsets[-1] != data.size or (np.diff(offsets) < 0).any():
        return [f'{name}: offsets {offsets.tolist()[:8]} do not frame {data.size} bytes of {len(refs)} files']
    out = []
    for f, ref in enumerate(refs):
        out += gate_file(f'{name} frame {f}', data[offsets[f]:offsets[f + 1]].tobytes(), ref)
    return out


# ------------------------------------------------------------------------------------------------ contents, crafted blocks
def content(kind, H, W, seed=0):
    """test frames uint8 [H,W,3]"""
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == 'ramp':
        i, j = np.mgrid[0:H, 0:W]
        return np.stack([(255 * j) // max(W - 1, 1), (255 * i) // max(H - 1, 1), (255 * (i + j)) // max(H + W - 2, 1)], -1).astype(np.uint8)
    if kind == 'white':
        return np.full((H, W, 3), 255, np.uint8)
    if kind == 'black':
        return np.zeros((H, W, 3), np.uint8)
    assert kind == 'render'
    img = np.full((H, W, 3), 255, np.uint8)
    img[H // 4:H // 4 + max(H // 3, 1), W // 5:W // 5 + max(W // 3, 1)] = (166, 188, 218)
    i, j = np.mgrid[0:H, 0:W]
    img[np.abs(i * max(W, 2) - j * max(H, 2) // 2 - H) < 2 * max(W, 2)] = (0x2F, 0x70, 0xAF)         # a line about 3 pixels thick
    return img


def crafted_blocks():
    """name -> (coef int16 [n_mcu, 3, 64] as 4:4:4 MCUs, restart): the corners of the entropy coder"""
    def mcus(n):
        return np.zeros((n, 3, 64), np.int16)
    out = {}
    c = mcus(2); c[:, :, 63] = (5, -3, 1); out['only_63'] = (c, 2)
    c = mcus(2); c[:, :, 63] = 7; c[:, :, 1] = -1; c[:, :, 20] = 1023; c[0, :, 0] = 100; out['63_among_others'] = (c, 1)
    c = mcus(4); c[0::2, :, 0] = 1023; c[1::2, :, 0] = -1024; c[:, 0, 5] = 1023; c[:, 1, 6] = -1023; c[:, 2, 62] = -1023; out['extremes'] = (c, 4)
    for run in (16, 31, 32, 47):
        c = mcus(2); c[:, :, 1 + run] = (1, -2, 3); c[1, :, 2 + run] = 4; out[f'run_{run}'] = (c, 2)
    c = mcus(3); c[:, :, 1:] = 1023; c[:, :, 0] = (1023, -1024, 1023); c[1] = -c[1] - 1; c[1, :, 1:] = -1023; out['longest_block'] = (c, 3)
    rng = np.random.default_rng(3)
    c = (rng.integers(-40, 41, (21, 3, 64)) * (rng.random((21, 3, 64)) < 0.2)).astype(np.int16); out['many_intervals'] = (c, 2)
    c = mcus(300); c[:, :, 0] = rng.integers(-1024, 1024, (300, 3)); c[:, :, 1:4] = -1; out['ff_bytes'] = (c, 140)
    return out


# ------------------------------------------------------------------------------------------------ the provider on host tensors
class RefOps:
    """the provider methods of motionbert_amd.video on host tensors, from the reference (with an optional seeded corruption)"""

    def __init__(self, corrupt=()):
        self.corrupt = tuple(corrupt)
        self.calls = []
        self._files = {}                                                 # per offsets tensor: the sizing and the emission are two calls

    def jpeg_ws(self, F, H, W, sub, restart, device):
        return torch.empty(16, dtype=torch.uint8)

    def jpeg_blocks(self, rgb, quality, sub, coef):
        self.calls.append(('blocks', rgb.shape[0]))
        for f in range(rgb.shape[0]):
            coef[f].copy_(torch.from_numpy(front(rgb[f].numpy(), quality, '420' if sub else '444', self.corrupt)))

    def jpeg_sizes(self, coef, H, W, sub, quality, restart, offsets, ws):
        self.calls.append(('sizes', coef.shape[0]))
        s = '420' if sub else '444'
        files = self._files[offsets.data_ptr()] = [header(H, W, quality, s, restart) + scan(c.numpy(), restart, self.corrupt) + b'\xff\xd9' for c in coef]
        offsets.copy_(torch.from_numpy(np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)))

    def jpeg_emit(self, coef, H, W, sub, quality, restart, offsets, data, ws):
        self.calls.append(('emit', coef.shape[0]))
        data.copy_(torch.from_numpy(np.frombuffer(b''.join(self._files.pop(offsets.data_ptr())), np.uint8).copy()))


# ------------------------------------------------------------------------------------------------ the fixture
def load_fixture(path):
    """tests/golden/jpeg_pil.npz (tools/mint_jpeg.py) -> a list of dicts: H, W, quality, sub ('420' / '444'), restart, kind, rgb, file (bytes),
    coef; and the versions that wrote it"""
    with np.load(path, allow_pickle=False) as z:
        cases = [dict(H=int(p[0]), W=int(p[1]), quality=int(p[2]), sub='420' if p[3] else '444', restart=int(p[4]), kind=str(k),
                      rgb=z[f'rgb_{i}'], file=z[f'file_{i}'].tobytes(), coef=z[f'coef_{i}'])
                 for i, (p, k) in enumerate(zip(z['params'], z['kinds']))]
        return cases, [str(v) for v in z['versions']]


def case_name(c):
    return f'{c["H"]}x{c["W"]}.{c["kind"]}.q{c["quality"]}.{c["sub"]}.r{c["restart"]}'


def avi_frames(data):
    """the payloads of the '00dc' chunks of an AVI file, in order"""
    top = riff(data)
    movi = next(c for c in top[0]['chunks'] if c['id'] == b'LIST' and c['form'] == b'movi')
    return [c['data'] for c in movi['chunks'] if c['id'] == b'00dc']
