// What the entropy stages of the JPEG decoder share (jpeg_dec.hip: one lane per restart interval; jpeg_sync.hip: the self-synchronising
// decode inside an interval, whose fallback is the same one-lane body): the frame geometry, the bit reader, one Huffman symbol, EXTEND,
// and the decode of one whole interval by one lane, which defines the result of every malformed scan.
#pragma once
#include "mbx_common.h"

#define TW MBX_JPEG_DEC_TABLE_WORDS

namespace {

struct DGeo {                         // a frame's MCU grid; sub 0 = 4:4:4, 1 = 4:2:0, 2 = 4:2:2
    int H, W, sub, mx, my, n_mcu, bpm, hs, vs, dw, dh, cw, yw;
    long long frame_bytes, y_bytes, c_bytes;
};
inline DGeo make_dgeo(int H, int W, int sub) {
    DGeo g;
    g.H = H; g.W = W; g.sub = sub;
    g.hs = sub ? 2 : 1; g.vs = sub == 1 ? 2 : 1;
    g.mx = (W + 8 * g.hs - 1) / (8 * g.hs); g.my = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.n_mcu = g.mx * g.my; g.bpm = g.hs * g.vs + 2;
    g.dw = (W + g.hs - 1) / g.hs; g.dh = (H + g.vs - 1) / g.vs;       // the real chroma samples
    g.cw = g.mx * 8; g.yw = g.mx * 8 * g.hs;                            // plane widths, whole MCUs
    g.y_bytes = (long long)g.n_mcu * g.hs * g.vs * 64; g.c_bytes = (long long)g.n_mcu * 64;
    g.frame_bytes = g.y_bytes + 2 * g.c_bytes;
    return g;
}

struct BitReader {
    const unsigned char* data;
    long long at, end;                // the next byte, the interval's end: every read is checked against it
    unsigned long long acc;           // the low n bits are the next bits of the stream
    int n;
    __device__ __forceinline__ void fill() {
        while (n <= 48 && at < end) {
            const unsigned b = data[at++];
            if (b == 0xffu && at < end && data[at] == 0u) ++at;          // the stuffed byte
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    __device__ __forceinline__ unsigned peek(int k) const {             // the next k <= 16 bits; zeros behind the end
        return (unsigned)(n >= k ? acc >> (n - k) : acc << (k - n)) & ((1u << k) - 1u);
    }
};

// one Huffman symbol, or a negative status; the caller has filled the reader.  t: the table in LDS (look 256 x u16 | maxcode 18 |
// valoffset 18 | vals 256 x u8)
__device__ __forceinline__ int jpeg_symbol(BitReader& r, const unsigned* __restrict__ t) {
    const unsigned short* look = reinterpret_cast<const unsigned short*>(t);
    const int* maxcode = reinterpret_cast<const int*>(t + 128);
    const int* valoff = maxcode + 18;
    const unsigned char* vals = reinterpret_cast<const unsigned char*>(t + 164);
    const unsigned e = look[r.peek(8)];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (len < 1 || len > 8) {
        const int code = (int)r.peek(16);
        for (len = 9; len <= 16; ++len)
            if ((code >> (16 - len)) <= maxcode[len]) break;
        if (len > 16) return r.n < 16 ? -MBX_JPEG_DEC_TRUNCATED : -MBX_JPEG_DEC_BAD_CODE;
        sym = vals[((code >> (16 - len)) + valoff[len]) & 255];
    }
    if (len > r.n) return -MBX_JPEG_DEC_TRUNCATED;
    r.n -= len;
    return sym;
}

// `s` <= 15 more bits, sign-extended as T.81 F.2.2.1 (EXTEND); ok false where the interval ends first.  No refill: a filled reader holds
// 49 bits or all there are, a symbol and its bits take at most 16 + 15
__device__ __forceinline__ int jpeg_receive_extend(BitReader& r, int s, bool& ok) {
    if (s == 0) return 0;
    if (s > r.n) { ok = false; return 0; }
    const int v = (int)((r.acc >> (r.n - s)) & ((1u << s) - 1u));
    r.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The lanes of a wave are kept in step by making the SYMBOL the loop's body: one trip decodes one Huffman symbol with its extra bits,
// whether it is a DC difference or an AC (run, size), and then advances the lane's own (MCU, block, coefficient) state.  Nested loops over
// MCUs, blocks and coefficients would let every lane sit in another loop, and the wave would walk them one after the other.
// One interval t = (frame, interval) by one lane; tab: the six tables in LDS.  The caller has checked status[t] == MBX_JPEG_DEC_OK.
__device__ __forceinline__ void jpeg_decode_interval(const unsigned char* __restrict__ data, long long data_bytes, const long long* __restrict__ pos,
                                                     const unsigned* tab, const DGeo& g, int restart, int n_int, long long t,
                                                     short* __restrict__ coef, int* __restrict__ status) {
    const int f = (int)(t / n_int), iv = (int)(t % n_int);
    const long long* p = pos + (size_t)f * (n_int + 1) + iv;
    BitReader r;
    r.data = data;
    r.at = p[0] < 0 ? 0 : p[0] > data_bytes ? data_bytes : p[0];
    r.end = p[1] - 2 < r.at ? r.at : p[1] - 2 > data_bytes ? data_bytes : p[1] - 2;
    r.acc = 0; r.n = 0;
    const int per = restart ? restart : g.n_mcu;
    const long long m0 = (long long)iv * per;
    const int m1 = (int)(m0 + per < g.n_mcu ? m0 + per : g.n_mcu);
    const int ny = g.bpm - 2;
    unsigned pred0 = 0u, pred1 = 0u, pred2 = 0u;                          // wrap; only the low 16 bits are stored
    int st = MBX_JPEG_DEC_OK;
    int m = (int)m0, k = 0, z = 0;                                       // the next symbol belongs to coefficient z of block k of MCU m; z = 0: the DC
    short* blk = coef + ((size_t)f * g.n_mcu + m) * g.bpm * 64;
    bool busy = m < m1;
    while (busy) {
        r.fill();
        const int c = k < ny ? 0 : k - ny + 1;
        const bool dc = z == 0;
        bool ok = true;
        const int s = jpeg_symbol(r, tab + (2 * c + (dc ? 0 : 1)) * TW);
        if (s < 0) st = -s;
        else if (dc) {
            const int d = jpeg_receive_extend(r, s & 15, ok);          // the tables hold no DC symbol above 15 (mbx_jpeg_dec_tables)
            if (!ok) st = MBX_JPEG_DEC_TRUNCATED;
            else {
                const unsigned v = (c == 0 ? pred0 : c == 1 ? pred1 : pred2) + (unsigned)d;
                pred0 = c == 0 ? v : pred0; pred1 = c == 1 ? v : pred1; pred2 = c == 2 ? v : pred2;
                blk[0] = (short)v;
                z = 1;
            }
        } else if (s == 0) z = 64;                                       // EOB
        else {
            z += s >> 4;
            if (s & 15) {
                if (z > 63) st = MBX_JPEG_DEC_RUN;
                else {
                    const int v = jpeg_receive_extend(r, s & 15, ok);
                    if (!ok) st = MBX_JPEG_DEC_TRUNCATED;
                    else blk[z] = (short)v;
                }
            } else if ((s >> 4) != 15) st = MBX_JPEG_DEC_BAD_CODE;       // (r, 0) other than EOB and ZRL is no baseline symbol
            else if (z > 63) st = MBX_JPEG_DEC_RUN;                      // a ZRL whose zeros pass 63
            ++z;
        }
        if (st != MBX_JPEG_DEC_OK) {                                     // the block the error lies in is zero like those behind it
            uint4* b4 = reinterpret_cast<uint4*>(blk);
            for (int j = 0; j < 8; ++j) b4[j] = make_uint4(0u, 0u, 0u, 0u);
            busy = false;
        } else if (z >= 64) {                                            // the next block
            z = 0;
            blk += 64;
            if (++k == g.bpm) { k = 0; busy = ++m < m1; }
        }
    }
    if (st == MBX_JPEG_DEC_OK && (r.n >= 8 || r.at < r.end)) st = MBX_JPEG_DEC_LEFTOVER;
    status[t] = st;
}

}  // namespace
