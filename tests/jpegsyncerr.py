"""The self-synchronising Huffman decode inside a restart interval (csrc/jpeg_sync.hip), restated in numpy on the RAW, stuffed bytes of an
interval.  include/mbx.h has the definition; the reference of the result is tests/jpegdecerr.py (`D.entropy`), which this model must equal in
every coefficient and status word.  `route` is a property of the bytes, the tables and the two constants S and CH, so the kernels are held
to the model's route exactly.

    Stream(raw, dht, bpm)                   -> one interval: the lenient and the strict decode of a subsequence from a state (p, k, z)
    plan(raw, dht, bpm)                     -> per subsequence the true entry, the speculative exit, the block and DC sums and their exclusive
                                               sums; per chunk whether it reproduced its stored exit; the route (0 or 1) that follows
    rounds(raw, dht, bpm, chunk)            -> the rounds the speculation of one chunk takes, simulated lane by lane (small inputs)
    entropy_sync(file, max_interval_bytes)  -> (coef, status, route) built from the plan, the fallback included
    SyncRefOps                              -> D.RefOps with jpeg_dec_sync_ws / jpeg_dec_entropy_sync, for CPU end-to-end tests

The rounds of the kernels end in a fixed point: lane i's entry is lane i - 1's exit.  The model walks to that fixed point directly: a lane
keeps the result it has while the entry it is handed equals the one it used, and from there on nothing behind it changes either.
`corrupt` names seeded errors (CORRUPTIONS); each must fail a gate (tests/test_jpegsyncerr.py)."""
import functools
import os
import re

import numpy as np
import torch

from tests import jpegdecerr as D

CORRUPTIONS = ('no_verify', 'k_ignored', 'z_ignored', 'stuffed_start', 'boundary_symbol_twice', 'dc_carry_dropped', 'block_count_off',
               'final_lenient', 'fallback_not_zeroed', 'long_interval_unflagged')
_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mbx.h')).read()
S = int(re.search(r'#define MBX_JPEG_SYNC_BYTES (\d+)', _HEADER).group(1))
CH = int(re.search(r'#define MBX_JPEG_SYNC_CHUNK (\d+)', _HEADER).group(1))
MAX_BYTES = 1 << 27


@functools.lru_cache(maxsize=16)
def _luts(dht_bytes):
    """six lists of 65536: (length << 8 | symbol) of the code at the head of 16 bits, 0 where none matches"""
    out = []
    for table in D.tables_of(np.frombuffer(dht_bytes, np.uint8).reshape(6, 272)):
        lut = np.zeros(65536, np.int64)
        for (length, code), sym in table.items():
            lut[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | sym
        out.append(lut.tolist())
    return out


def _extend(v, s):
    return 0 if s == 0 else v if v >> (s - 1) else v - (1 << s) + 1


class Stream:
    """one interval.  A position is a RAW bit position: 8 * (index of a byte that is data) + bit; behind the end the bytes are zeros and go on
    being counted.  Inside, the bits are read from the unstuffed bytes, and the two maps translate."""

    def __init__(self, raw, dht, bpm, corrupt=()):
        self.raw, self.bpm, self.corrupt = bytes(raw), bpm, corrupt
        r = np.frombuffer(self.raw, np.uint8)
        keep = np.ones(r.size, bool)
        keep[1:] = ~((r[:-1] == 0xff) & (r[1:] == 0))
        if 'stuffed_start' in corrupt:                                    # the 00 a subsequence begins on is read as data
            keep[S::S] = True
        self.keep = keep
        self.n = int(keep.sum())
        self.ub = r[keep].tobytes() + bytes(8)
        self.raw_of = np.nonzero(keep)[0].tolist()                        # unstuffed byte -> raw byte
        self.u_of = (np.cumsum(keep) - 1).tolist()                        # raw data byte -> unstuffed byte
        self.lut = _luts((D.annex_k() if dht is None else np.ascontiguousarray(dht, np.uint8)).tobytes())
        self.n_sub = -(-r.size // S)
        self.n_chunk = -(-self.n_sub // CH)

    def _u(self, p):
        b = p >> 3
        return ((self.u_of[b] if b < len(self.raw) else self.n + b - len(self.raw)) << 3) | (p & 7)

    def _p(self, u):
        b = u >> 3
        return ((self.raw_of[b] if b < self.n else len(self.raw) + b - self.n) << 3) | (u & 7)

    def end_bits(self, j):
        return 8 * min((j + 1) * S, len(self.raw))

    def first(self, j):
        """the speculative entry of subsequence j"""
        b = j * S
        if j and not self.keep[b]:
            b += 1
        return (8 * b, 0, 0)

    def decode(self, j, entry, strict=False, b0=0, total=0, last=False, coef=None, pre=(0, 0, 0), extra=0):
        """subsequence j from `entry` -> (exit, (blocks completed, DC sums of the three components), bad).  strict: with the checks of
        D.decode_interval, the values stored into coef [total, 64] from block b0 on with the DC predictors `pre`.  extra: symbols decoded
        behind the end (a corruption)."""
        p, k, z = entry
        end, ny, bpm = self.end_bits(j), self.bpm - 2, self.bpm
        nb, dc, blk, bad, done = 0, [0, 0, 0], b0, False, strict and b0 >= total
        ub, lut, real = self.ub, self.lut, 8 * self.n
        if not done and p < end:
            u = self._u(p)
            while True:
                c = 0 if k < ny else k - ny + 1
                w = (int.from_bytes(ub[u >> 3:(u >> 3) + 5], 'big') >> (8 - (u & 7))) & 0xffffffff if (u >> 3) + 5 <= len(ub) else 0
                e = lut[2 * c + (1 if z else 0)][w >> 16]
                if e == 0:
                    if strict:
                        bad = done = True
                        break
                    u += 1
                else:
                    length, sym = e >> 8, e & 255
                    s = sym & 15
                    v = (w >> (32 - length - s)) & ((1 << s) - 1)
                    if z == 0:
                        u += length + s
                        dc[c] = (dc[c] + _extend(v, s)) & 0xffffffff
                        if strict:
                            coef[blk, 0] = np.array((pre[c] + dc[c]) & 0xffff, np.uint16).astype(np.int16)
                        z = 1
                    elif sym == 0:
                        u += length
                        z = 64
                    elif strict:
                        u += length + s
                        z += sym >> 4
                        if s:
                            if z > 63:
                                bad = done = True
                                break
                            coef[blk, z] = _extend(v, s)
                        elif sym >> 4 != 15 or z > 63:
                            bad = done = True
                            break
                        z += 1
                    else:
                        u += length + s
                        z += (sym >> 4) + 1
                    if strict and u > real:                               # the interval ends inside the symbol
                        bad = done = True
                        break
                    if z >= 64:
                        z, nb, k = 0, nb + 1, (k + 1) % bpm
                        if strict:
                            blk += 1
                            if blk == total:
                                bad, done = real - u >= 8, True
                                break
                p = self._p(u)
                if p >= end:
                    if extra == 0:
                        break
                    extra -= 1
        if strict and last and not done:
            bad = True
        return (p, k, z), (nb, dc[0], dc[1], dc[2]), bad


def _same(a, b, corrupt):
    if 'k_ignored' in corrupt:
        return (a[0], a[2]) == (b[0], b[2])
    if 'z_ignored' in corrupt:
        return (a[0], a[1]) == (b[0], b[1])
    return a == b


def plan(raw, dht, bpm, corrupt=(), stream=None):
    st = stream or Stream(raw, dht, bpm, corrupt)
    n, extra = st.n_sub, 1 if 'boundary_symbol_twice' in corrupt else 0
    entry, exit_, cnt = [None] * n, [None] * n, [None] * n

    def walk(a, b, state, settled):
        """lanes a .. b - 1 to the fixed point from lane a's entry `state`.  A lane that is handed the entry it has used keeps its result;
        settled: the lanes behind it are at a fixed point already (B), so nothing else changes"""
        for j in range(a, b):
            if entry[j] is not None and _same(state, entry[j], corrupt):
                if settled:
                    return
                state = exit_[j]
                continue
            entry[j] = state
            exit_[j], c, _ = st.decode(j, state, extra=extra)
            cnt[j] = (c[0] + (1 if 'block_count_off' in corrupt and state[2] and j else 0),) + c[1:]
            state = exit_[j]

    spec_exit, chunk_exit = [], []
    for c in range(st.n_chunk):                                           # A
        a, b = c * CH, min(c * CH + CH, n)
        for j in range(a, b):
            entry[j] = st.first(j)
            exit_[j], cnt[j], _ = st.decode(j, entry[j], extra=extra)
        spec_exit += exit_[a:b]
        e0, entry[a] = entry[a], None
        walk(a, b, (0, 0, 0) if c == 0 else e0, False)
        chunk_exit.append(exit_[b - 1])
    ok = [True] * st.n_chunk
    for c in range(1, st.n_chunk):                                        # B: from the exit A stored, never from a verified one
        a, b = c * CH, min(c * CH + CH, n)
        if 'no_verify' in corrupt:                                        # the speculative exits are taken as true
            continue
        walk(a, b, chunk_exit[c - 1], True)
        ok[c] = _same(exit_[b - 1], chunk_exit[c], corrupt)
    pre, run = [], (0, 0, 0, 0)
    for j in range(n):
        pre.append(run)
        run = tuple((x + y) & 0xffffffff for x, y in zip(run, cnt[j]))
    return dict(stream=st, n_sub=n, n_chunk=st.n_chunk, entry=entry, exit=exit_, spec_exit=spec_exit, cnt=cnt, pre=pre, chunk_exit=chunk_exit,
                chunk_ok=ok, route=0 if all(ok) or 'no_verify' in corrupt else 1)


def rounds(raw, dht, bpm, chunk=0):
    """the rounds of kernel A on one chunk, lane by lane: 1 for the speculation and 1 for every round in which a lane decoded again"""
    st = Stream(raw, dht, bpm)
    a, b = chunk * CH, min(chunk * CH + CH, st.n_sub)
    entry = [st.first(j) for j in range(a, b)]
    if chunk == 0:
        entry[0] = (0, 0, 0)
    memo = {}

    def dec(j, e):
        if (j, e) not in memo:
            memo[j, e] = st.decode(j, e)[0]
        return memo[j, e]
    ex = [dec(a + i, e) for i, e in enumerate(entry)]
    n = 1
    while True:
        new = [entry[0]] + ex[:-1]
        if new == entry:
            return n
        entry = new
        ex = [dec(a + i, e) for i, e in enumerate(entry)]
        n += 1


def sync_interval(raw, dht, n_mcu, bpm, max_interval_bytes=None, corrupt=()):
    """one interval -> (coef [n_mcu, bpm, 64], status, route)"""
    total = n_mcu * bpm
    coef = np.zeros((total, 64), np.int16)
    limit = len(raw) if max_interval_bytes is None else max_interval_bytes
    route = 0
    if len(raw) > limit and 'long_interval_unflagged' not in corrupt:
        route = 3
    elif len(raw) == 0:
        route = 2
    else:
        cutting = len(raw) > limit                                        # the corruption: what the grid covers is decoded, unflagged
        p = plan(raw[:-(-limit // S) * S] if cutting else raw, dht, bpm, corrupt)
        route = p['route']
        if route == 0:
            st, bad = p['stream'], False
            for j in range(p['n_sub']):
                pre = p['pre'][j]
                dc = (0, 0, 0) if 'dc_carry_dropped' in corrupt and j else pre[1:]
                bad |= st.decode(j, p['entry'][j], strict=True, b0=pre[0], total=total, last=j + 1 == p['n_sub'] and not cutting, coef=coef, pre=dc)[2]
            route = 2 if bad and 'final_lenient' not in corrupt else 0
    if route == 0:
        return coef.reshape(n_mcu, bpm, 64), D.OK, 0
    ref, status = D.decode_interval(raw, D.tables_of(D.annex_k() if dht is None else dht), n_mcu, bpm)
    if 'fallback_not_zeroed' in corrupt:
        ref = np.where(ref.reshape(total, 64) != 0, ref.reshape(total, 64), coef).reshape(n_mcu, bpm, 64)
    return ref, status, route


def entropy_sync(data, max_interval_bytes=None, corrupt=()):
    """a file -> (coef [n_mcu, bpm, 64], status [n_int], route [n_int]) by the plan"""
    p, data = D.parse(data), bytes(data)
    mx, my, bpm = D.geometry(p['H'], p['W'], p['sub'])
    n_mcu, n_int = mx * my, D.n_intervals(p['H'], p['W'], p['sub'], p['restart'])
    per = p['restart'] or n_mcu
    pos, ok = D.positions(data, p['scan'], n_int)
    coef, status = np.zeros((n_mcu, bpm, 64), np.int16), np.full(n_int, D.OK if ok else D.MARKERS, np.int32)
    route = np.zeros(n_int, np.int32)
    for k in range(n_int if ok else 0):
        a, b = k * per, min(k * per + per, n_mcu)
        coef[a:b], status[k], route[k] = sync_interval(data[pos[k]:max(pos[k + 1] - 2, pos[k])], p['dht'], b - a, bpm, max_interval_bytes, corrupt)
    return coef, status, route


class SyncRefOps(D.RefOps):
    """D.RefOps with the two methods of the self-synchronising route, on host tensors"""

    def jpeg_dec_sync_ws(self, F, n_int, max_interval_bytes, device):
        return torch.empty(16, dtype=torch.uint8)

    def jpeg_dec_entropy_sync(self, data, pos, tables, H, W, sub, restart, max_interval_bytes, coef, status, route, ws):
        self.calls.append(('dec_entropy_sync', coef.shape[0]))
        d, s = data.numpy().tobytes(), D.SUB_NAME[sub]
        mx, my, bpm = D.geometry(H, W, s)
        n_mcu, dht = mx * my, tables.numpy()
        per = restart or n_mcu
        coef.zero_()
        route.zero_()
        for f in range(coef.shape[0]):
            for k in range(status.shape[1]):
                if int(status[f, k]) != D.OK:
                    continue
                a, b = k * per, min(k * per + per, n_mcu)
                lo, hi = int(pos[f, k]), int(pos[f, k + 1]) - 2
                c, st, rt = sync_interval(d[lo:max(hi, lo)], dht, b - a, bpm, int(max_interval_bytes), self.corrupt)
                coef[f, a:b].copy_(torch.from_numpy(c))
                status[f, k], route[f, k] = int(st), rt


# ------------------------------------------------------------------------------------------------ the inputs of both test files
def one_interval(rgb, quality, sub):
    """a file of the package's own encoder whose frame is ONE interval (its DRI covers the frame), as files without DRI are"""
    from tests import jpegerr as J
    return J.encode(rgb, quality, sub, 65535)


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> file.  sweep.*: 4:4:4 noise frames 8 x 8 n at quality 100, whose scan lengths cross many multiples of S (one is shorter than S);
    noise, noise.512: several chunks (three or more in the larger one), FF 00 pairs on subsequence boundaries; white.*: every MCU the same 32 bits, so a wrong k stays wrong; longest:
    J.crafted_blocks' block of 1,660 bits; cut: a one-interval noise file that ends in the middle of its scan; and D.malformed()."""
    from tests import jpegerr as J
    out = {f'sweep.{n:02d}': one_interval(J.content('noise', 8, 8 * n, seed=n), 100, '444') for n in range(1, 49)}
    out['noise'] = one_interval(J.content('noise', 256, 512, seed=1), 90, '420')
    out['noise.512'] = one_interval(J.content('noise', 512, 512, seed=2), 90, '420')
    out['white.64'] = one_interval(J.content('white', 64, 64), 90, '420')
    out['white.256'] = one_interval(J.content('white', 256, 256), 90, '420')
    out['white.2048'] = one_interval(J.content('white', 2048, 2048), 90, '420')
    coef, _ = J.crafted_blocks()['longest_block']
    out['longest'] = J.header(8, 8 * coef.shape[0], 90, '444', coef.shape[0]) + J.scan(coef, coef.shape[0]) + b'\xff\xd9'
    whole = one_interval(J.content('noise', 64, 64, seed=5), 90, '444')
    a, b = D.parse(whole)['scan']
    out['cut'] = whole[:a + (b - a) // 2] + b'\xff\xd9'
    for k, (data, _, _) in D.malformed().items():
        out['malformed.' + k] = data
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(coef, status) of D.entropy and (coef, status, route) of the model for inputs()[name], computed once"""
    f = inputs()[name]
    return D.entropy(f)[:2], entropy_sync(f)
