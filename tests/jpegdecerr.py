"""Baseline JPEG as libjpeg decodes it by default, restated in numpy: the reference of csrc/jpeg_dec.hip and of the reading half of
motionbert_amd/video.py.  Every stage is integer arithmetic, so the gate is equality with the pixels libjpeg-turbo decodes
(tests/golden/jpeg_dec_pil.npz, minted by tools/mint_jpeg_dec.py from Pillow); there is no tolerance anywhere.  include/mbx.h has the definition.

    parse(file)                             -> the header's facts: H, W, sub ('444' / '420' / '422'), restart (0: none), q [3,64] per component in
                                               zigzag order, dht (uint8 [6,272]: bits and vals of the DC and AC table per component; None: the file
                                               has no DHT, Annex K applies), scan = (first entropy-coded byte, position of EOI)
    positions(data, scan, n_int)            -> (pos [n_int+1], markers ok): where every restart interval lies
    decode_interval(raw, tables, ...)       -> the coefficients of one interval and its status
    entropy(file or parsed)                 -> (coef int16 [n_mcu, bpm, 64] in zigzag order, status int32 [n_int], pos)
    pixels(coef, q, H, W, sub)              -> rgb uint8 [H,W,3]: dequantise, jpeg_idct_islow, range limit, fancy upsampling, colour
    decode(file)                            -> rgb
    RefOps                                  -> the decoding half of the kernel provider of motionbert_amd.video, on host tensors

`corrupt` names seeded errors (CORRUPTIONS); each must fail a gate (tests/test_jpegdecerr.py)."""
import struct

import numpy as np
import torch

from tests import jpegerr as J

CORRUPTIONS = ('fancy_small', 'bias_swapped', 'row_clamp_padded', 'clamp_not_table', 'rows_first', 'dequant_natural', 'pred_not_reset',
               'stuffing_kept', 'extend_off', 'g_no_round', 'annex_k_forced', 'h2v1_bias_swapped')
OK, TRUNCATED, BAD_CODE, RUN, LEFTOVER, MARKERS = range(6)
STATUS = ('ok', 'the interval ends inside a symbol', 'no such Huffman code', 'a run past coefficient 63', 'whole bytes left over',
          'the restart markers of the frame are not the expected ones')
SAMPLING = {'444': (1, 1), '420': (2, 2), '422': (2, 1)}
SUB_CODE = {'444': 0, '420': 1, '422': 2}
SUB_NAME = {v: k for k, v in SUB_CODE.items()}


def geometry(H, W, sub):
    """(MCU columns, MCU rows, blocks per MCU)"""
    h, v = SAMPLING[sub]
    return -(-W // (8 * h)), -(-H // (8 * v)), h * v + 2


def annex_k():
    """the dht [6,272] of a frame without DHT segments: luminance tables for component 0, chrominance for 1 and 2"""
    out = np.zeros((6, 272), np.uint8)
    for c in range(3):
        for a in range(2):
            bits, vals = J.HUFF[2 * (c > 0) + a]
            out[2 * c + a, :16], out[2 * c + a, 16:16 + len(vals)] = bits, vals
    return out


# ------------------------------------------------------------------------------------------------ the header
def parse(data):
    """strict and small: what Pillow, this package and the hand-built variants of the tests write.  Raises ValueError on anything else."""
    data = bytes(data)
    if data[:2] != b'\xff\xd8':
        raise ValueError('no SOI')
    p, q, huff, res, comps = 2, {}, {}, dict(restart=0), None
    while True:
        if p + 4 > len(data) or data[p] != 0xff:
            raise ValueError(f'no marker at byte {p}')
        m, n = data[p + 1], struct.unpack('>H', data[p + 2:p + 4])[0]
        seg = data[p + 4:p + 2 + n]
        if m == 0xdb:
            while seg:
                if seg[0] >> 4:
                    raise ValueError('16-bit DQT')
                q[seg[0]], seg = np.frombuffer(seg[1:65], np.uint8), seg[65:]
        elif m == 0xc0:
            if seg[0] != 8 or seg[5] != 3:
                raise ValueError('SOF0 not 8 bit, three components')
            res['H'], res['W'] = struct.unpack('>HH', seg[1:5])
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i], seg[8 + 3 * i]) for i in range(3)]
            sub = {0x11: '444', 0x22: '420', 0x21: '422'}.get(comps[0][1])
            if sub is None or comps[1][1] != 0x11 or comps[2][1] != 0x11:
                raise ValueError('SOF0 sampling factors')
            res['sub'] = sub
        elif m == 0xc4:
            while seg:
                k = int(sum(seg[1:17]))
                huff[seg[0]], seg = (list(seg[1:17]), list(seg[17:17 + k])), seg[17 + k:]
        elif m == 0xdd:
            res['restart'] = struct.unpack('>H', seg)[0]
        elif m == 0xda:
            if comps is None or seg[0] != 3 or [seg[1 + 2 * i] for i in range(3)] != [c[0] for c in comps] or tuple(seg[7:10]) != (0, 63, 0):
                raise ValueError('SOS is not one interleaved baseline scan of the three components')
            sel = [seg[2 + 2 * i] for i in range(3)]
            p += 2 + n
            break
        elif not (0xe0 <= m <= 0xef or m == 0xfe):
            raise ValueError(f'marker {m:#x}')
        p += 2 + n
    res['q'] = np.stack([q[c[2]] for c in comps])
    if huff:
        dht = np.zeros((6, 272), np.uint8)
        for c, s in enumerate(sel):
            for a, key in enumerate((s >> 4, 0x10 | (s & 15))):
                bits, vals = huff[key]
                dht[2 * c + a, :16], dht[2 * c + a, 16:16 + len(vals)] = bits, vals
        res['dht'] = dht
    else:
        res['dht'] = None
    end = p
    while True:                                                           # the first marker that is neither a stuffed 0xFF nor RSTn
        end = data.find(b'\xff', end)
        if end < 0 or end + 1 >= len(data):
            raise ValueError('no EOI')
        if data[end + 1] == 0 or 0xd0 <= data[end + 1] <= 0xd7:
            end += 2
        elif data[end + 1] == 0xff:
            end += 1
        else:
            break
    if data[end + 1] != 0xd9:
        raise ValueError(f'marker {data[end + 1]:#x} after the scan')
    res['scan'] = (p, end)
    return res


def n_intervals(H, W, sub, restart):
    mx, my, _ = geometry(H, W, sub)
    return -(-mx * my // restart) if restart else 1


def positions(data, scan, n_int):
    """pos int64 [n_int + 1] (interval k is data[pos[k]:pos[k+1] - 2]) and whether the n_int - 1 markers are there with n = k mod 8"""
    a, b = scan
    d = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
    a, b = min(max(a, 0), d.size), min(max(b, min(max(a, 0), d.size)), d.size)
    s = d[a:b]
    at = np.nonzero((s[:-1] == 0xff) & ((s[1:] & 0xf8) == 0xd0))[0] if s.size > 1 else np.zeros(0, np.int64)
    ok = len(at) == n_int - 1 and all(int(s[i + 1]) == 0xd0 + (k & 7) for k, i in enumerate(at))
    pos = np.full(n_int + 1, b + 2, np.int64)
    pos[0] = a
    m = min(len(at), n_int - 1)
    pos[1:1 + m] = at[:m] + a + 2
    return pos, ok


# ------------------------------------------------------------------------------------------------ entropy decoding
def lookup(bits, vals):
    code, size = J.derive(bits, vals)
    return {(int(size[v]), int(code[v])): int(v) for v in vals[:int(sum(bits))]}


def tables_of(dht):
    """dht [6,272] -> six dicts (length, code) -> symbol"""
    return [lookup([int(b) for b in row[:16]], [int(v) for v in row[16:]]) for row in np.asarray(dht)]


class _Reader:
    def __init__(self, raw, corrupt=()):
        self.b = bytes(raw) if 'stuffing_kept' in corrupt else bytes(raw).replace(b'\xff\x00', b'\xff')
        self.i, self.acc, self.n = 0, 0, 0

    def left(self):
        return self.n + 8 * (len(self.b) - self.i)

    def peek(self, k):
        while self.n < k and self.i < len(self.b):
            self.acc, self.i, self.n = (self.acc << 8) | self.b[self.i], self.i + 1, self.n + 8
        return ((self.acc >> (self.n - k)) if self.n >= k else (self.acc << (k - self.n))) & ((1 << k) - 1)

    def drop(self, k):
        self.n -= k
        self.acc &= (1 << self.n) - 1

    def symbol(self, table):
        """the symbol, or minus a status"""
        code, left = self.peek(16), self.left()
        for length in range(1, 17):
            v = table.get((length, code >> (16 - length)))
            if v is not None:
                if length > left:
                    return -TRUNCATED
                self.drop(length)
                return v
        return -TRUNCATED if left < 16 else -BAD_CODE

    def receive(self, s, corrupt=()):
        """s more bits, extended; None where the interval ends first"""
        if s == 0:
            return 0
        v = self.peek(s)
        if s > self.left():
            return None
        self.drop(s)
        return v if v >> (s - 1) else v - (1 << s) + (0 if 'extend_off' in corrupt else 1)


def decode_interval(raw, tables, n_mcu, bpm, pred=None, corrupt=()):
    """raw: the interval's bytes as the file has them -> (coef int16 [n_mcu, bpm, 64], status).  The block an error lies in and the blocks
    behind it are zero."""
    r, coef, ny = _Reader(raw, corrupt), np.zeros((n_mcu, bpm, 64), np.int16), bpm - 2
    pred = [0, 0, 0] if pred is None else pred
    for m in range(n_mcu):
        for k in range(bpm):
            c = 0 if k < ny else k - ny + 1
            blk = np.zeros(64, np.int64)
            s = r.symbol(tables[2 * c])
            if s < 0:
                return coef, -s
            d = r.receive(s & 15, corrupt)
            if d is None:
                return coef, TRUNCATED
            pred[c] += d
            blk[0] = pred[c]
            z = 1
            while z < 64:
                s = r.symbol(tables[2 * c + 1])
                if s < 0:
                    return coef, -s
                if s == 0:
                    break
                z += s >> 4
                if s & 15:
                    if z > 63:
                        return coef, RUN
                    v = r.receive(s & 15, corrupt)
                    if v is None:
                        return coef, TRUNCATED
                    blk[z] = v
                elif s >> 4 != 15:
                    return coef, BAD_CODE
                elif z > 63:
                    return coef, RUN
                z += 1
            coef[m, k] = blk.astype(np.int16)                             # a DC value is stored modulo 2^16
    return coef, LEFTOVER if r.left() >= 8 else OK


def entropy(p, data=None, corrupt=()):
    """p: a file, or (with `data`) its parsed header -> (coef [n_mcu, bpm, 64], status [n_int], pos [n_int + 1])"""
    if data is None:
        p, data = parse(p), bytes(p)
    mx, my, bpm = geometry(p['H'], p['W'], p['sub'])
    n_mcu, n_int = mx * my, n_intervals(p['H'], p['W'], p['sub'], p['restart'])
    per = p['restart'] or n_mcu
    pos, ok = positions(data, p['scan'], n_int)
    coef, status = np.zeros((n_mcu, bpm, 64), np.int16), np.full(n_int, OK if ok else MARKERS, np.int32)
    tables = tables_of(annex_k() if p['dht'] is None or 'annex_k_forced' in corrupt else p['dht'])
    pred = [0, 0, 0]
    for k in range(n_int if ok else 0):
        a, b = k * per, min(k * per + per, n_mcu)
        pred = pred if 'pred_not_reset' in corrupt else [0, 0, 0]
        coef[a:b], status[k] = decode_interval(data[pos[k]:max(pos[k + 1] - 2, pos[k])], tables, b - a, bpm, pred, corrupt)
    return coef, status, pos


# ------------------------------------------------------------------------------------------------ pixels
LIMIT = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)]).astype(np.int64)


def _ipass(d, shift):
    """one pass of jpeg_idct_islow along the last axis (int64 [...,8])"""
    c = J.C
    z1 = (d[..., 2] + d[..., 6]) * c['c541']
    e2, e3 = z1 - d[..., 6] * c['c1847'], z1 + d[..., 2] * c['c765']
    e0, e1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * c['c1175']
    t0, t1, t2, t3 = t0 * c['c298'], t1 * c['c2053'], t2 * c['c3072'], t3 * c['c1501']
    z1, z2, z3, z4 = -z1 * c['c899'], -z2 * c['c2562'], -z3 * c['c1961'] + z5, -z4 * c['c390'] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(x + (1 << (shift - 1))) >> shift for x in o], -1)


def idct(coef, q, corrupt=()):
    """coef [...,64] zigzag, q [64] zigzag -> samples int64 [...,8,8]"""
    c = coef.astype(np.int64)
    nat = np.zeros_like(c)
    if 'dequant_natural' in corrupt:
        nat[..., J.ZIGZAG] = c
        nat = nat * q.astype(np.int64)
    else:
        nat[..., J.ZIGZAG] = c * q.astype(np.int64)
    b = nat.reshape(nat.shape[:-1] + (8, 8))
    if 'rows_first' in corrupt:
        b = np.swapaxes(_ipass(np.swapaxes(_ipass(b, 11), -1, -2), 18), -1, -2)
    else:
        b = _ipass(np.swapaxes(_ipass(np.swapaxes(b, -1, -2), 11), -1, -2), 18)
    return np.clip(b + 128, 0, 255) if 'clamp_not_table' in corrupt else LIMIT[b & 1023]


def planes(coef, q, H, W, sub, corrupt=()):
    """-> (Y, Cb, Cr) int64, whole MCUs wide and high"""
    h, v = SAMPLING[sub]
    mx, my, bpm = geometry(H, W, sub)
    ny = h * v
    y = idct(coef[:, :ny], q[0], corrupt).reshape(my, mx, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * v * 8, mx * h * 8)
    cs = [idct(coef[:, ny + c], q[1 + c], corrupt).reshape(my, mx, 8, 8).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8) for c in range(2)]
    return y, cs[0], cs[1]


def _h2(s, even_bias, odd_bias, shift, edge):
    """the horizontal triangle filter over the last axis: s [...,dw] -> [...,2 dw]"""
    left, right = np.concatenate([s[..., :1], s[..., :-1]], -1), np.concatenate([s[..., 1:], s[..., -1:]], -1)
    even, odd = (3 * s + left + even_bias) >> shift, (3 * s + right + odd_bias) >> shift
    even[..., 0], odd[..., -1] = (edge * s[..., 0] + even_bias) >> shift, (edge * s[..., -1] + odd_bias) >> shift
    return np.stack([even, odd], -1).reshape(s.shape[:-1] + (2 * s.shape[-1],))


def upsample(plane, H, W, sub, corrupt=()):
    h, v = SAMPLING[sub]
    dh, dw = -(-H // v), -(-W // h)
    if h == 1:
        return plane[:H, :W]
    c = plane[:dh, :dw]
    if dw <= 2 and 'fancy_small' not in corrupt:
        return np.repeat(np.repeat(c, v, 0), h, 1)[:H, :W]
    if v == 1:
        e, o = (2, 1) if 'h2v1_bias_swapped' in corrupt else (1, 2)
        out = _h2(c, e, o, 2, 1)
        out[..., 0], out[..., -1] = c[..., 0], c[..., -1]
        return out[:H, :W]
    rows = plane[:, :dw] if 'row_clamp_padded' in corrupt else c
    r = np.arange(dh)
    up, down = rows[np.maximum(r - 1, 0)], rows[np.minimum(r + 1, rows.shape[0] - 1)]
    s = np.stack([3 * c + up, 3 * c + down], 1).reshape(2 * dh, dw)
    e, o = (7, 8) if 'bias_swapped' in corrupt else (8, 7)
    return _h2(s, e, o, 4, 4)[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def colour(y, cb, cr, corrupt=()):
    cb, cr = cb - 128, cr - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + (0 if 'g_no_round' in corrupt else 32768) - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pixels(coef, q, H, W, sub, corrupt=()):
    y, cb, cr = planes(np.asarray(coef), np.asarray(q), H, W, sub, corrupt)
    return colour(y[:H, :W], upsample(cb, H, W, sub, corrupt), upsample(cr, H, W, sub, corrupt), corrupt)


def decode(data, corrupt=()):
    """a complete file -> rgb uint8 [H,W,3]; raises where an interval is malformed"""
    p = parse(data)
    coef, status, _ = entropy(p, bytes(data), corrupt)
    if status.any():
        k = int(np.nonzero(status)[0][0])
        raise ValueError(f'interval {k}: {STATUS[status[k]]}')
    return pixels(coef, p['q'], p['H'], p['W'], p['sub'], corrupt)


# ------------------------------------------------------------------------------------------------ the provider on host tensors
class RefOps(J.RefOps):
    """the encoding half of jpegerr.RefOps and the decoding half from this reference, on host tensors"""

    def jpeg_dec_tables(self, dht):
        return torch.from_numpy(annex_k() if dht is None or 'annex_k_forced' in self.corrupt else np.ascontiguousarray(dht, np.uint8).copy())

    def jpeg_dec_ws(self, F, H, W, sub, device):
        return torch.empty(16, dtype=torch.uint8)

    def jpeg_dec_index(self, data, scans, n_int, pos, status):
        self.calls.append(('dec_index', scans.shape[0]))
        d = data.numpy()
        for f in range(scans.shape[0]):
            p, ok = positions(d, (int(scans[f, 0]), int(scans[f, 1])), n_int)
            pos[f].copy_(torch.from_numpy(p))
            status[f].fill_(OK if ok else MARKERS)

    def jpeg_dec_entropy(self, data, pos, tables, H, W, sub, restart, coef, status):
        self.calls.append(('dec_entropy', coef.shape[0]))
        d, s = data.numpy().tobytes(), SUB_NAME[sub]
        mx, my, bpm = geometry(H, W, s)
        n_mcu, tabs = mx * my, tables_of(tables.numpy())
        per = restart or n_mcu
        coef.zero_()
        for f in range(coef.shape[0]):
            pred = [0, 0, 0]
            for k in range(status.shape[1]):
                if int(status[f, k]) != OK:
                    continue
                a, b = k * per, min(k * per + per, n_mcu)
                pred = pred if 'pred_not_reset' in self.corrupt else [0, 0, 0]
                lo, hi = int(pos[f, k]), int(pos[f, k + 1]) - 2
                c, st = decode_interval(d[lo:max(hi, lo)], tabs, b - a, bpm, pred, self.corrupt)
                coef[f, a:b].copy_(torch.from_numpy(c))
                status[f, k] = st

    def jpeg_dec_pixels(self, coef, q, H, W, sub, rgb, ws):
        self.calls.append(('dec_pixels', coef.shape[0]))
        for f in range(coef.shape[0]):
            rgb[f].copy_(torch.from_numpy(pixels(coef[f].numpy(), np.asarray(q), H, W, SUB_NAME[sub], self.corrupt)))


# ------------------------------------------------------------------------------------------------ the fixture
def load_fixture(path):
    """tests/golden/jpeg_dec_pil.npz (tools/mint_jpeg_dec.py) -> a list of dicts: H, W, quality, sub, restart, optimize, kind, file (bytes), rgb
    (the pixels Pillow decodes from the file); and the versions that wrote it"""
    with np.load(path, allow_pickle=False) as z:
        cases = [dict(H=int(p[0]), W=int(p[1]), quality=int(p[2]), sub=SUB_NAME[int(p[3])], restart=int(p[4]), optimize=bool(p[5]), kind=str(k),
                      file=z[f'file_{i}'].tobytes(), rgb=z[f'rgb_{i}'])
                 for i, (p, k) in enumerate(zip(z['params'], z['kinds']))]
        return cases, [str(v) for v in z['versions']]


def case_name(c):
    return f'{c["H"]}x{c["W"]}.{c["kind"]}.q{c["quality"]}.{c["sub"]}.r{c["restart"]}' + ('.opt' if c['optimize'] else '')


# ------------------------------------------------------------------------------------------------ malformed scans
def malformed():
    """name -> (file, interval, status): 4:4:4 files of 16 x 24 pixels (6 MCUs, restart interval 2: three intervals) with the Annex K tables
    whose interval `interval` is malformed in one way each and must give `status` there and zeros from the block the error lies in; with
    MARKERS every interval of the frame has it.  Ordinary inputs with a defined output."""
    rgb = J.content('noise', 16, 24, seed=11)
    head, parts = J.header(16, 24, 90, '444', 2), J.intervals(J.front(rgb, 90, '444'), 2)

    def put(bw, code_size):
        bw.put(int(code_size[0]), int(code_size[1]))

    def sym(table, s):
        return DERIVED[table][0][s], DERIVED[table][1][s]
    DERIVED = J.DERIVED
    bw = J._Bits()                                                        # DC 0, then ZRL ZRL ZRL and (15, 1): 49 + 15 = 64
    put(bw, sym(0, 0))
    for _ in range(3):
        put(bw, sym(1, 0xf0))
    put(bw, sym(1, 0xf1))
    bw.put(1, 1)
    bw.flush()
    run = bytes(bw.out).replace(b'\xff', b'\xff\x00')
    bw = J._Bits()                                                        # DC 0, then sixteen 1-bits: no code of the Annex K AC table
    put(bw, sym(0, 0))
    bw.put(0xffff, 16)
    bw.put(0xffff, 16)                                                    # and sixteen more, so that the interval does not end first
    bw.flush()
    unused = bytes(bw.out).replace(b'\xff', b'\xff\x00')
    out = dict(
        cut=(head + J.join([parts[0], parts[1][:len(parts[1]) // 2], parts[2]]) + b'\xff\xd9', 1, TRUNCATED),
        unused_code=(head + J.join([parts[0], parts[1], unused]) + b'\xff\xd9', 2, BAD_CODE),
        run_past_63=(head + J.join([run, parts[1], parts[2]]) + b'\xff\xd9', 0, RUN),
        trailing_byte=(head + J.join([parts[0], parts[1] + b'\x12', parts[2]]) + b'\xff\xd9', 1, LEFTOVER),
        missing_rst=(head + parts[0] + parts[1] + b'\xff\xd1' + parts[2] + b'\xff\xd9', 0, MARKERS),
        rst_out_of_order=(head + parts[0] + b'\xff\xd1' + parts[1] + b'\xff\xd0' + parts[2] + b'\xff\xd9', 2, MARKERS),
        empty_interval=(head + J.join([parts[0], b'', parts[2]]) + b'\xff\xd9', 1, TRUNCATED))
    return out


def crafted_range():
    """A file whose IDCT output leaves the part of the range-limit table that equals a clamp: coefficients written straight into a scan (DC 500
    at quality 75 is a sample of 628, which limit[v & 1023] turns into 0 where a clamp gives 255).  No picture reaches this at any quality
    (noise at quality 100 stays inside in every fixture case), and libjpeg-turbo does not agree with itself there: jidctint.c indexes the
    table, its SIMD kernels saturate.  The definition (include/mbx.h) is the C code's; this file is gated against the reference alone."""
    coef = np.zeros((2, 3, 64), np.int16)
    coef[0, 0, 0], coef[1, 0, 0], coef[1, 1, 0], coef[0, 2, 1] = 500, -600, 500, 300
    return J.header(8, 16, 75, '444', 1) + J.scan(coef, 1) + b'\xff\xd9'
