// Baseline JPEG as compute: the frames of render.hip / skeleton.hip compressed where they were drawn, so that a video file's bytes and not its
// pixels cross the host link.  Every stage is integer arithmetic and reproduces libjpeg's default path bit for bit; include/mbx.h has the
// definitions.
//   mbx_jpeg_blocks         : one launch.  A workgroup owns JB_BLOCKS consecutive 8 x 8 blocks (whole MCUs); eight lanes per block.  Lane r
//                             converts and (4:2:0 chroma) downsamples row r, runs the row pass in registers and leaves it in LDS; after the
//                             barrier lane c runs the column pass on column c, quantises and leaves int16 in zigzag order in LDS; the dummy blocks
//                             of 4:2:0 take their DC; the workgroup's blocks leave as one contiguous run.
//   mbx_jpeg_entropy_sizes  : three launches.  jpeg_interval_kernel<false> codes every restart interval without storing it and counts its
//                             bytes after stuffing; jpeg_frame_scan_kernel turns the counts of a frame into positions; jpeg_offsets_kernel
//                             turns the frame sizes into offsets [F+1].  The caller reads offsets[F] (the ONE host synchronisation) and allocates.
//   mbx_jpeg_entropy        : one launch.  jpeg_interval_kernel<true> codes every interval again, straight into place; the first interval's
//                             workgroup also copies the header, every later one writes the RSTn in front of it, the last one EOI.
// The interval kernel.  One workgroup of JE_THREADS lanes per restart interval (byte-aligned, own predictors), in pieces of JE_THREADS blocks,
// one block per lane.  Per piece: the lane's code length (stored by the sizing pass, read by the emitting pass), a workgroup prefix sum for
// its bit position, the bits OR-ed into an LDS buffer that holds the worst case of a piece (JE_WORDS, proven in mbx.h), then the whole bytes of
// the piece leave four per lane and round with a second prefix sum over the 0xFF bytes; the up to seven bits left over open the next piece.
// Prefix sums are ballots over bit planes and v_mbcnt-style popcounts: no LDS crossbar, no cross-lane instruction besides the ballot.
#include "mbx_common.h"
#include "jpeg_tables.h"
#include <initializer_list>

#define JB_THREADS 256
#define JB_BLOCKS 30                  // 5 MCUs of 4:2:0 or 10 of 4:4:4
#define JB_PITCH 72                   // words per block in LDS: 64 + 8, so that the column pass of four blocks covers 32 banks
#define JE_THREADS 128
#define JE_WAVES (JE_THREADS / 64)
#define JE_WORDS ((JE_THREADS * MBX_JPEG_MAX_BLOCK_BITS + 14 + 31) / 32 + 2)      // a piece in the worst case + carried bits + padding

namespace {

// ---------------------------------------------------------------------------------------------------------------
// tables (ITU-T T.81 Annex K; jpeg_tables.h has the zigzag order and the Huffman tables), shared by the host (the header) and the device
// ---------------------------------------------------------------------------------------------------------------
constexpr unsigned char kQBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// the canonical codes of the four tables: entry = code | size << 16 per symbol, 0 where the table has none
struct HuffCodes { unsigned e[4][256]; };
constexpr HuffCodes derive_codes() {
    HuffCodes h = {};
    for (int t = 0; t < 4; ++t) {
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kBits[t][len - 1]; ++i) h.e[t][kVals[t][k++]] = code++ | (unsigned)len << 16;
            code <<= 1;
        }
    }
    return h;
}
__device__ const HuffCodes d_codes = derive_codes();

struct InvZigzag { unsigned char z[64]; };
constexpr InvZigzag derive_inv() {
    InvZigzag r = {};
    for (int i = 0; i < 64; ++i) r.z[kZigzag[i]] = (unsigned char)i;
    return r;
}
__device__ const InvZigzag d_inv_zigzag = derive_inv();              // natural index -> zigzag position
__device__ const unsigned char d_qbase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

__host__ __device__ inline int quant_entry(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (base * s + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

struct Geo {                          // a frame's MCU grid
    int H, W, sub, mx, my, n_mcu, bpm;
};
inline Geo make_geo(int H, int W, int sub) {
    Geo g;
    const int m = sub ? 16 : 8;
    g.H = H; g.W = W; g.sub = sub;
    g.mx = (W + m - 1) / m; g.my = (H + m - 1) / m;
    g.n_mcu = g.mx * g.my; g.bpm = sub ? 6 : 3;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------
// stage A: colour, downsample, DCT, quantise
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int jpeg_component(int r, int g, int b, int c) {
    return c == 0 ? (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
         : c == 1 ? (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
                  : (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}
__device__ __forceinline__ int jpeg_sample(const unsigned char* __restrict__ frame, int W, int y, int x, int c) {
    const unsigned char* p = frame + ((size_t)y * W + x) * 3;
    return jpeg_component(p[0], p[1], p[2], c);
}

template <bool FIRST> __device__ __forceinline__ void jpeg_dct_pass(int (&d)[8]) { MBX_JPEG_FDCT_PASS(d, FIRST); }

__global__ __launch_bounds__(JB_THREADS) void jpeg_blocks_kernel(const unsigned char* __restrict__ rgb, Geo g, int quality, long long n_mcu_all,
                                                                 short* __restrict__ coef) {
    __shared__ int tile[JB_BLOCKS * JB_PITCH];
    __shared__ short outb[JB_BLOCKS * 64];
    __shared__ unsigned short q8[2][64];                                // 8 q per natural index
    const int tid = threadIdx.x;
    if (tid < 128) q8[tid >> 6][tid & 63] = (unsigned short)(8 * quant_entry(d_qbase[tid >> 6][tid & 63], quality));
    const int b = tid >> 3, r = tid & 7;                                // block of the workgroup, row / column of the block
    const int mpw = JB_BLOCKS / g.bpm;
    const long long mcu = (long long)blockIdx.x * mpw + b / g.bpm;
    const int k = b % g.bpm;
    const bool live = b < JB_BLOCKS && mcu < n_mcu_all;
    const int f = live ? (int)(mcu / g.n_mcu) : 0, m = live ? (int)(mcu % g.n_mcu) : 0;
    const int my_ = m / g.mx, mx_ = m % g.mx;
    const int comp = g.sub ? (k < 4 ? 0 : k - 3) : k;
    bool dummy = false;
    if (live) {
        const unsigned char* frame = rgb + (size_t)f * g.H * g.W * 3;
        int d[8];
        if (g.sub && comp) {                                            // 4:2:0 chroma: rows padded to even, then 2 x 2 means, then the last row down
            const int cy = min(my_ * 8 + r, (g.H + 1) / 2 - 1);
            const int y0 = min(2 * cy, g.H - 1), y1 = min(2 * cy + 1, g.H - 1);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int cx = mx_ * 8 + j, x0 = min(2 * cx, g.W - 1), x1 = min(2 * cx + 1, g.W - 1);
                const int s = jpeg_sample(frame, g.W, y0, x0, comp) + jpeg_sample(frame, g.W, y0, x1, comp) +
                              jpeg_sample(frame, g.W, y1, x0, comp) + jpeg_sample(frame, g.W, y1, x1, comp);
                d[j] = ((s + 1 + (j & 1)) >> 2) - 128;
            }
        } else {
            const int bx = g.sub ? 2 * mx_ + (k & 1) : mx_, by = g.sub ? 2 * my_ + (k >> 1) : my_;
            dummy = bx >= (g.W + 7) / 8 || by >= (g.H + 7) / 8;       // only 4:2:0 luma can be
            const int y = min(by * 8 + r, g.H - 1);
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = dummy ? 0 : jpeg_sample(frame, g.W, y, min(bx * 8 + j, g.W - 1), comp) - 128;
        }
        jpeg_dct_pass<true>(d);
#pragma unroll
        for (int j = 0; j < 8; ++j) tile[b * JB_PITCH + r * 8 + j] = d[j];
    }
    __syncthreads();
    if (live) {
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = tile[b * JB_PITCH + i * 8 + r];
        jpeg_dct_pass<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = i * 8 + r;
            const unsigned q = q8[comp ? 1 : 0][n];
            const unsigned a = ((unsigned)abs(d[i]) + (q >> 1)) / q;
            outb[b * 64 + d_inv_zigzag.z[n]] = dummy ? (short)0 : (short)(d[i] < 0 ? -(int)a : (int)a);
        }
    }
    __syncthreads();
    if (live && g.sub && r == 0 && k == 0) {                            // the dummy blocks of this MCU take the DC in front of them
        const bool dx = 2 * mx_ + 1 >= (g.W + 7) / 8, dy = 2 * my_ + 1 >= (g.H + 7) / 8;
        short* o = outb + b * 64;
        if (dx) o[64] = o[0];
        if (dy) { o[128] = o[64]; o[192] = o[64]; }
        else if (dx) o[192] = o[128];
    }
    __syncthreads();
    // the workgroup's blocks are one contiguous run of the output
    const long long first = (long long)blockIdx.x * mpw * g.bpm, total = n_mcu_all * g.bpm;
    const long long left = total - first;
    const int nblk = left < (long long)(mpw * g.bpm) ? (int)left : mpw * g.bpm;
    unsigned* dst = reinterpret_cast<unsigned*>(coef + first * 64);
    const unsigned* src = reinterpret_cast<const unsigned*>(outb);
    for (int i = tid; i < nblk * 32; i += JB_THREADS) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------------------
// workgroup prefix sums from ballots: every lane of the workgroup must call
// ---------------------------------------------------------------------------------------------------------------
template <int WAVES, int PLANES, typename T> __device__ __forceinline__ T wg_scan(unsigned v, T* wave_tot, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    T pre = 0, tot = 0;
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
        const unsigned long long m = __ballot((v >> p) & 1u);
        pre += (T)__popcll(m & below) << p;
        tot += (T)__popcll(m) << p;
    }
    if (lane == 0) wave_tot[wave] = tot;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T t = wave_tot[w];
        before += w < wave ? t : (T)0;
        total += t;
    }
    __syncthreads();                                                     // wave_tot may be written again
    return pre + before;
}

// ---------------------------------------------------------------------------------------------------------------
// stage B: one restart interval per workgroup
// ---------------------------------------------------------------------------------------------------------------
// The symbols of one block, in order, to `put(code, size)`.  Coefficients beyond the baseline range are clamped (mbx.h): the proven
// worst case of a block then holds whatever the caller passes.
template <class Put> __device__ __forceinline__ void jpeg_block_symbols(const short* __restrict__ blk, int pred, const unsigned* __restrict__ dc,
                                                                        const unsigned* __restrict__ ac, Put&& put) {
    const uint4* p4 = reinterpret_cast<const uint4*>(blk);
    int run = 0;
    for (int j = 0; j < 8; ++j) {
        const uint4 v = p4[j];
        if (j && (v.x | v.y | v.z | v.w) == 0u) { run += 8; continue; }
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int c = (int)(short)(w[e >> 1] >> (16 * (e & 1)));
            if (j == 0 && e == 0) {
                c = max(-2047, min(2047, c - pred));
                const int nb = 32 - __clz(abs(c));                      // abs(0) -> clz 32 -> 0
                const unsigned t = dc[nb];
                put(((t & 0xffffu) << nb) | ((unsigned)(c < 0 ? c - 1 : c) & ((1u << nb) - 1u)), (int)(t >> 16) + nb);
            } else if (c == 0) {
                ++run;
            } else {
                c = max(-1023, min(1023, c));
                while (run >= 16) { const unsigned z = ac[0xf0]; put(z & 0xffffu, (int)(z >> 16)); run -= 16; }
                const int nb = 32 - __clz(abs(c));
                const unsigned t = ac[run << 4 | nb];
                put(((t & 0xffffu) << nb) | ((unsigned)(c < 0 ? c - 1 : c) & ((1u << nb) - 1u)), (int)(t >> 16) + nb);
                run = 0;
            }
        }
    }
    if (run > 0) { const unsigned z = ac[0]; put(z & 0xffffu, (int)(z >> 16)); }
}

__device__ __forceinline__ void jpeg_store(unsigned char* __restrict__ data, long long at, long long data_bytes, unsigned v) {
    if ((unsigned long long)at < (unsigned long long)data_bytes) data[at] = (unsigned char)v;      // never outside the caller's buffer
}

struct JpegHeader {
    unsigned char b[MBX_JPEG_HEADER_BYTES];
};

template <bool EMIT>
__global__ __launch_bounds__(JE_THREADS) void jpeg_interval_kernel(const short* __restrict__ coef, Geo g, int restart, int n_int,
                                                                   unsigned short* __restrict__ blk_bits, unsigned* __restrict__ int_bytes,
                                                                   const unsigned* __restrict__ int_off, const long long* __restrict__ offsets,
                                                                   unsigned char* __restrict__ data, long long data_bytes, JpegHeader hdr) {
    __shared__ unsigned buf[JE_WORDS];
    __shared__ unsigned codes[4][256];
    __shared__ unsigned wave_tot[JE_WAVES];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / n_int, iv = blockIdx.x % n_int;
    for (int i = tid; i < 1024; i += JE_THREADS) codes[i >> 8][i & 255] = d_codes.e[i >> 8][i & 255];
    const int mcu0 = iv * restart, mcu1 = min(mcu0 + restart, g.n_mcu);
    const int nblk = (mcu1 - mcu0) * g.bpm;
    const size_t blk0 = ((size_t)f * g.n_mcu + mcu0) * g.bpm;            // the interval's first block among all blocks

    long long pos = 0;                                                   // where the interval's next byte goes (EMIT)
    if (EMIT) {
        const long long base = offsets[f];
        pos = base + MBX_JPEG_HEADER_BYTES + int_off[(size_t)f * n_int + iv];
        if (iv == 0)
            for (int i = tid; i < MBX_JPEG_HEADER_BYTES; i += JE_THREADS)
                jpeg_store(data, base + i, data_bytes, hdr.b[i]);
        if (iv > 0 && tid < 2) jpeg_store(data, pos - 2 + tid, data_bytes, tid ? 0xd0u + ((iv - 1) & 7) : 0xffu);
    }
    unsigned carry_bits = 0, carry_val = 0;                              // the bits of an unfinished byte, left-aligned in a byte
    unsigned stuffed = 0, plain = 0;                                     // 0xFF bytes / bytes before stuffing so far
    __syncthreads();

    for (int piece = 0; piece < nblk; piece += JE_THREADS) {
        const int i = piece + tid;
        const bool have = i < nblk;
        const short* blk = coef + (blk0 + (have ? i : 0)) * 64;
        int pred = 0;
        unsigned comp = 0;
        if (have) {
            const int k = i % g.bpm, first = i < g.bpm;                   // first MCU of the interval: the predictors are 0
            comp = g.sub ? (k < 4 ? 0 : 1) : (k ? 1 : 0);
            const int back = g.sub ? (k == 0 ? 3 : k < 4 ? 1 : 6) : 3;    // the previous block of the same component
            if (!(first && (g.sub ? (k == 0 || k >= 4) : true))) pred = blk[-64 * back];
        }
        const unsigned* dc = codes[2 * comp];
        const unsigned* ac = codes[2 * comp + 1];
        unsigned nbits = 0;
        if (have) {
            if (EMIT) nbits = min((unsigned)blk_bits[blk0 + i], (unsigned)MBX_JPEG_MAX_BLOCK_BITS);      // as the sizing pass left it
            else {
                jpeg_block_symbols(blk, pred, dc, ac, [&](unsigned, int size) __attribute__((always_inline)) { nbits += (unsigned)size; });
                blk_bits[blk0 + i] = (unsigned short)nbits;
            }
        }
        unsigned total;
        unsigned at = wg_scan<JE_WAVES, 11, unsigned>(nbits, wave_tot, total) + carry_bits;
        total += carry_bits;
        const bool last = piece + JE_THREADS >= nblk;
        const unsigned padded = last ? (total + 7u) & ~7u : total;
        const unsigned words = (padded + 31u) / 32u + 1u;                 // <= JE_WORDS: a block is at most MBX_JPEG_MAX_BLOCK_BITS
        for (unsigned w = tid; w < words; w += JE_THREADS) buf[w] = 0u;
        __syncthreads();
        if (tid == 0) {
            if (carry_bits) atomicOr(&buf[0], carry_val << 24);
            if (padded > total) atomicOr(&buf[total >> 5], ((1u << (padded - total)) - 1u) << (32u - (total & 31u) - (padded - total)));      // 1-bits, inside one byte
        }
        if (have) {
            jpeg_block_symbols(blk, pred, dc, ac, [&](unsigned code, int size) __attribute__((always_inline)) {
                const unsigned long long x = (unsigned long long)code << (64 - (at & 31u) - size);
                const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
                atomicOr(&buf[at >> 5], hi);
                if (lo) atomicOr(&buf[(at >> 5) + 1], lo);
                at += (unsigned)size;
            });
        }
        __syncthreads();
        const unsigned nbytes = padded >> 3;
        for (unsigned b0 = 0; b0 < nbytes; b0 += 4 * JE_THREADS) {
            const unsigned mine = b0 + 4 * tid;
            const unsigned w = mine < nbytes ? buf[mine >> 2] : 0u;
            const unsigned valid = mine < nbytes ? min(4u, nbytes - mine) : 0u;
            unsigned ff = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) ff += (e < (int)valid && ((w >> (24 - 8 * e)) & 0xffu) == 0xffu) ? 1u : 0u;
            unsigned ff_all;
            const unsigned ff_before = wg_scan<JE_WAVES, 3, unsigned>(ff, wave_tot, ff_all);
            if (EMIT) {
                long long o = pos + plain + stuffed + mine + ff_before;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned byte = (w >> (24 - 8 * e)) & 0xffu;
                    if (e < (int)valid) {
                        jpeg_store(data, o++, data_bytes, byte);
                        if (byte == 0xffu) jpeg_store(data, o++, data_bytes, 0u);
                    }
                }
            }
            stuffed += ff_all;
        }
        plain += nbytes;
        carry_bits = padded & 7u;
        carry_val = carry_bits ? ((buf[nbytes >> 2] >> (24 - 8 * (nbytes & 3u))) & 0xffu) & (0xff00u >> carry_bits) : 0u;
        __syncthreads();                                                 // buf is cleared next
    }
    if (!EMIT && tid == 0) int_bytes[(size_t)f * n_int + iv] = plain + stuffed;
    if (EMIT && iv == n_int - 1 && tid < 2) {
        jpeg_store(data, pos + plain + stuffed + tid, data_bytes, tid ? 0xd9u : 0xffu);
    }
}

// int_bytes [F, n_int] -> int_off [F, n_int]: where an interval starts behind the header, the RSTn in front of it counted; frame_bytes [F]
// 32-bit sums suffice: a frame has at most 3 * 256 * 256 blocks of at most 2 * 208 bytes after stuffing, 82 MB with its markers.
__global__ __launch_bounds__(256) void jpeg_frame_scan_kernel(const unsigned* __restrict__ int_bytes, int n_int, unsigned* __restrict__ int_off,
                                                              unsigned* __restrict__ frame_bytes) {
    __shared__ unsigned wave_tot[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    unsigned run = 0;
    for (int i0 = 0; i0 < n_int; i0 += 256) {
        const int i = i0 + tid;
        const unsigned v = i < n_int ? int_bytes[(size_t)f * n_int + i] + (i ? 2u : 0u) : 0u;
        unsigned tot;
        const unsigned pre = wg_scan<4, 32, unsigned>(v, wave_tot, tot);
        if (i < n_int) int_off[(size_t)f * n_int + i] = run + pre + (i ? 2u : 0u);
        run += tot;
    }
    if (tid == 0) frame_bytes[f] = MBX_JPEG_HEADER_BYTES + run + 2u;
}

__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const unsigned* __restrict__ frame_bytes, int F, long long* __restrict__ offsets) {
    __shared__ unsigned long long wave_tot[4];
    const int tid = threadIdx.x;
    unsigned long long run = 0;
    for (int f0 = 0; f0 < F; f0 += 256) {
        const int f = f0 + tid;
        unsigned long long tot;
        const unsigned long long pre = wg_scan<4, 32, unsigned long long>(f < F ? frame_bytes[f] : 0u, wave_tot, tot);
        if (f < F) offsets[f] = (long long)(run + pre);
        run += tot;
    }
    if (tid == 0) offsets[F] = (long long)run;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int build_header(int H, int W, int quality, int sub, int restart, unsigned char* out) {
    unsigned char* p = out;
    auto put = [&](std::initializer_list<int> v) { for (int x : v) *p++ = (unsigned char)x; };
    put({0xff, 0xd8, 0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xdb, 0x00, 0x43, t});
        for (int i = 0; i < 64; ++i) *p++ = (unsigned char)quant_entry(kQBase[t][kZigzag[i]], quality);
    }
    put({0xff, 0xc0, 0x00, 0x11, 0x08, H >> 8, H & 255, W >> 8, W & 255, 3, 1, sub ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    const int tc[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        put({0xff, 0xc4, (19 + kNVals[t]) >> 8, (19 + kNVals[t]) & 255, tc[t]});
        for (int i = 0; i < 16; ++i) *p++ = kBits[t][i];
        for (int i = 0; i < kNVals[t]; ++i) *p++ = kVals[t][i];
    }
    put({0xff, 0xdd, 0x00, 0x04, restart >> 8, restart & 255});
    put({0xff, 0xda, 0x00, 0x0c, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3f, 0x00});
    return (int)(p - out);
}

int check_frames(const char* who, int F, int H, int W, int sub) {
    MBX_CHECK_ARG(F >= 0 && F <= MBX_JPEG_MAX_FRAMES && H >= 1 && H <= MBX_JPEG_MAX_SIZE && W >= 1 && W <= MBX_JPEG_MAX_SIZE,
                  "%s: bad sizes F=%d H=%d W=%d (0 <= F <= %d, 1 <= H, W <= %d)", who, F, H, W, MBX_JPEG_MAX_FRAMES, MBX_JPEG_MAX_SIZE);
    MBX_CHECK_ARG(sub == 0 || sub == 1, "%s: subsampling %d (0: 4:4:4, 1: 4:2:0)", who, sub);
    return 0;
}
int check_coding(const char* who, int quality, int restart) {
    MBX_CHECK_ARG(quality >= 1 && quality <= 100, "%s: quality %d (1 .. 100)", who, quality);
    MBX_CHECK_ARG(restart >= 1 && restart <= 65535, "%s: restart interval %d (1 .. 65535 MCUs)", who, restart);
    return 0;
}

struct WsLayout {
    size_t int_bytes, int_off, frame_bytes, blk_bits, total;
    int n_int;
};
WsLayout ws_layout(int F, const Geo& g, int restart) {
    WsLayout l;
    l.n_int = (g.n_mcu + restart - 1) / restart;
    const size_t ni = (size_t)F * l.n_int;
    l.int_bytes = 0;
    l.int_off = l.int_bytes + ni * 4;
    l.frame_bytes = l.int_off + ni * 4;
    l.blk_bits = l.frame_bytes + (size_t)F * 4;
    l.total = ((l.blk_bits + (size_t)F * g.n_mcu * g.bpm * 2) + 15) & ~(size_t)15;
    return l;
}

}  // namespace

extern "C" int mbx_jpeg_header(int H, int W, int quality, int sub, int restart, unsigned char* out) {
    if (check_frames("jpeg_header", 0, H, W, sub) || check_coding("jpeg_header", quality, restart)) return 1;
    MBX_CHECK_ARG(out, "jpeg_header: null pointer");
    const int n = build_header(H, W, quality, sub, restart, out);
    MBX_CHECK_ARG(n == MBX_JPEG_HEADER_BYTES, "jpeg_header: %d bytes, not %d", n, MBX_JPEG_HEADER_BYTES);
    return 0;
}

extern "C" int mbx_jpeg_blocks(const unsigned char* rgb, int F, int H, int W, int quality, int sub, short* coef, void* stream) {
    if (check_frames("jpeg_blocks", F, H, W, sub)) return 1;
    MBX_CHECK_ARG(quality >= 1 && quality <= 100, "jpeg_blocks: quality %d (1 .. 100)", quality);
    if (F == 0) return 0;
    MBX_CHECK_ARG(rgb && coef, "jpeg_blocks: null pointer");
    MBX_CHECK_ARG(((uintptr_t)coef & 15) == 0, "jpeg_blocks: coef must be 16-byte aligned");
    const Geo g = make_geo(H, W, sub);
    const long long n_mcu_all = (long long)F * g.n_mcu, mpw = JB_BLOCKS / g.bpm;
    const long long grid = (n_mcu_all + mpw - 1) / mpw;
    MBX_CHECK_ARG(grid <= 0x7fffffffll, "jpeg_blocks: %d frames of %d MCUs are too many for one launch", F, g.n_mcu);
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((unsigned)grid), dim3(JB_THREADS), 0, (hipStream_t)stream, rgb, g, quality, n_mcu_all, coef);
    MBX_LAUNCH_CHECK("jpeg_blocks");
    return 0;
}

extern "C" size_t mbx_jpeg_entropy_ws(int F, int H, int W, int sub, int restart) {
    if (F < 1 || F > MBX_JPEG_MAX_FRAMES || H < 1 || H > MBX_JPEG_MAX_SIZE || W < 1 || W > MBX_JPEG_MAX_SIZE || (sub != 0 && sub != 1) || restart < 1 ||
        restart > 65535)
        return 0;
    return ws_layout(F, make_geo(H, W, sub), restart).total;
}

static int entropy_common(const char* who, const short* coef, int F, int H, int W, int sub, int quality, int restart, const void* offsets, void* ws,
                          size_t ws_bytes, Geo* g, WsLayout* l) {
    if (check_frames(who, F, H, W, sub) || check_coding(who, quality, restart)) return 1;
    if (F == 0) return 0;
    MBX_CHECK_ARG(coef && offsets && ws, "%s: null pointer", who);
    MBX_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)offsets & 7) == 0,
                  "%s: coef and ws must be 16-byte aligned, offsets 8-byte aligned", who);
    *g = make_geo(H, W, sub);
    *l = ws_layout(F, *g, restart);
    MBX_CHECK_ARG(ws_bytes >= l->total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l->total);
    MBX_CHECK_ARG((long long)F * l->n_int <= 0x7fffffffll, "%s: %d frames of %d restart intervals are too many for one launch", who, F, l->n_int);
    return 0;
}

extern "C" int mbx_jpeg_entropy_sizes(const short* coef, int F, int H, int W, int sub, int quality, int restart, long long* offsets, void* ws,
                                      size_t ws_bytes, void* stream) {
    Geo g;
    WsLayout l;
    if (entropy_common("jpeg_entropy_sizes", coef, F, H, W, sub, quality, restart, offsets, ws, ws_bytes, &g, &l)) return 1;
    if (F == 0) return 0;
    char* w = (char*)ws;
    JpegHeader hdr = {};
    hipLaunchKernelGGL(jpeg_interval_kernel<false>, dim3(F * l.n_int), dim3(JE_THREADS), 0, (hipStream_t)stream, coef, g, restart, l.n_int,
                       (unsigned short*)(w + l.blk_bits), (unsigned*)(w + l.int_bytes), (const unsigned*)nullptr, (const long long*)nullptr,
                       (unsigned char*)nullptr, 0ll, hdr);
    MBX_LAUNCH_CHECK("jpeg_entropy_sizes");
    hipLaunchKernelGGL(jpeg_frame_scan_kernel, dim3(F), dim3(256), 0, (hipStream_t)stream, (const unsigned*)(w + l.int_bytes), l.n_int,
                       (unsigned*)(w + l.int_off), (unsigned*)(w + l.frame_bytes));
    MBX_LAUNCH_CHECK("jpeg_entropy_sizes (frames)");
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const unsigned*)(w + l.frame_bytes), F, offsets);
    MBX_LAUNCH_CHECK("jpeg_entropy_sizes (offsets)");
    return 0;
}

extern "C" int mbx_jpeg_entropy(const short* coef, int F, int H, int W, int sub, int quality, int restart, const long long* offsets,
                                unsigned char* data, long long data_bytes, void* ws, size_t ws_bytes, void* stream) {
    Geo g;
    WsLayout l;
    if (entropy_common("jpeg_entropy", coef, F, H, W, sub, quality, restart, offsets, ws, ws_bytes, &g, &l)) return 1;
    if (F == 0) return 0;
    MBX_CHECK_ARG(data && data_bytes >= (long long)F * (MBX_JPEG_HEADER_BYTES + 2), "jpeg_entropy: data of %lld bytes cannot hold %d files", data_bytes, F);
    char* w = (char*)ws;
    JpegHeader hdr;
    if (build_header(H, W, quality, sub, restart, hdr.b) != MBX_JPEG_HEADER_BYTES) return mbx_set_error("jpeg_entropy: header size");
    hipLaunchKernelGGL(jpeg_interval_kernel<true>, dim3(F * l.n_int), dim3(JE_THREADS), 0, (hipStream_t)stream, coef, g, restart, l.n_int,
                       (unsigned short*)(w + l.blk_bits), (unsigned*)(w + l.int_bytes), (const unsigned*)(w + l.int_off), offsets, data, data_bytes,
                       hdr);
    MBX_LAUNCH_CHECK("jpeg_entropy");
    return 0;
}
