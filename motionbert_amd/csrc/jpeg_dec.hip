// Baseline JPEG decoded as compute: the inverse of jpeg.hip, for the Motion-JPEG frames motionbert_amd/video.py reads.  Every stage is integer
// arithmetic and reproduces libjpeg's default decode path (jpeg_idct_islow, do_fancy_upsampling, the 16-bit colour tables) bit for bit;
// include/mbx.h has the definitions.  This code reads bytes it did not write: every read of `data` is checked against the interval's end,
// every coefficient index against 63, every table index is masked, and a malformed interval has a defined result (a status code and zeros).
//   mbx_jpeg_dec_tables  : host only.  (bits, vals) of the six tables of a scan (DC and AC per component) -> libjpeg's decode form: an 8-bit
//                          look-ahead table, maxcode / valoffset for the longer codes, the symbols.  Without a DHT: Annex K (jpeg_tables.h).
//   mbx_jpeg_dec_index   : one launch, one workgroup per frame.  Inside a scan 0xFF is followed only by 0x00 or a marker, so the RSTn are
//                          found by a byte compare; JI_BYTES bytes per lane and piece, a ballot prefix count gives every marker its rank,
//                          and marker k closes interval k: pos [F, n_int + 1].  A wrong count or a wrong n mod 8 sequence marks every
//                          interval of the frame MBX_JPEG_DEC_MARKERS.
//   mbx_jpeg_dec_entropy : a memset and one launch.  Huffman decoding inside a restart interval is sequential, so the interval is the unit
//                          of parallel work, ONE LANE per interval, one wave per workgroup.  The loop's body is one symbol, so the 64
//                          intervals of a wave run in step, each with its own bit reader, predictors and (MCU, block, coefficient)
//                          position, and diverge only inside a symbol.  The tables are staged in LDS once per workgroup.
//                          Coefficients are zero unless a lane stores them.  The lane's body lives in jpeg_dec_common.h, because it is also the
//                          fallback of mbx_jpeg_dec_entropy_sync (jpeg_sync.hip): the self-synchronising decode INSIDE an interval, for the
//                          frames without restart markers that are one interval, and one lane here.
//   mbx_jpeg_dec_pixels  : two launches.  jpeg_idct_kernel: eight lanes per block, dequantise and un-zigzag through LDS, columns, then
//                          rows through the 72-word pitch of the encoder's stage A, the range-limit table, eight samples per lane as one
//                          8-byte store into the component planes of the workspace (padded to whole MCUs).  jpeg_colour_kernel: four
//                          consecutive pixels per lane, fancy upsampling read from the planes (the halo of a block is its neighbour's
//                          samples, which only exist once every block of the frame is done), colour, three 4-byte stores.
#include "jpeg_dec_common.h"
#include "jpeg_tables.h"

#define JI_THREADS 256
#define JI_BYTES 16                   // bytes per lane and piece of the marker search: at most 8 markers, four ballot planes
#define JD_THREADS 64                 // one wave: 64 restart intervals
#define JP_THREADS 256
#define JP_BLOCKS (JP_THREADS / 8)
#define JP_PITCH 72                   // words per block in LDS: 64 + 8, so that the column pass of four blocks covers 32 banks
#define JC_THREADS 256

namespace {

// ---------------------------------------------------------------------------------------------------------------
// the restart markers of every frame
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JI_THREADS) void jpeg_index_kernel(const unsigned char* __restrict__ data, long long data_bytes,
                                                                const long long* __restrict__ scans, int n_int, long long* __restrict__ pos,
                                                                int* __restrict__ status) {
    __shared__ unsigned wave_tot[JI_THREADS / 64];
    __shared__ int bad;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long s0 = scans[2 * f], s1 = scans[2 * f + 1];
    s0 = s0 < 0 ? 0 : s0 > data_bytes ? data_bytes : s0;                 // the ranges come from a tensor: never outside the buffer
    s1 = s1 < s0 ? s0 : s1 > data_bytes ? data_bytes : s1;
    long long* p = pos + (size_t)f * (n_int + 1);
    if (tid == 0) bad = 0;
    __syncthreads();
    unsigned run = 0;                                                    // markers before this piece
    for (long long base = s0; base < s1; base += (long long)JI_THREADS * JI_BYTES) {
        const long long a = base + (long long)tid * JI_BYTES;
        unsigned mask = 0;
        for (int e = 0; e < JI_BYTES; ++e) {
            const long long i = a + e;
            if (i + 1 < s1 && data[i] == 0xffu && (data[i + 1] & 0xf8u) == 0xd0u) mask |= 1u << e;
        }
        const unsigned cnt = __popc(mask);
        unsigned pre = 0, tot = 0;
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned long long m = __ballot((cnt >> b) & 1u);
            pre += (unsigned)__popcll(m & below) << b;
            tot += (unsigned)__popcll(m) << b;
        }
        if (lane == 0) wave_tot[wave] = tot;
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < JI_THREADS / 64; ++w) {
            before += w < wave ? wave_tot[w] : 0u;
            all += wave_tot[w];
        }
        unsigned k = run + before + pre;
        while (mask) {
            const int e = __ffs(mask) - 1;
            mask &= mask - 1;
            if (data[a + e + 1] != 0xd0u + (k & 7u)) atomicOr(&bad, 1);
            if (k + 1 < (unsigned)n_int) p[k + 1] = a + e + 2;          // marker k closes interval k
            ++k;
        }
        run += all;
        __syncthreads();                                                 // wave_tot is written again
    }
    const bool wrong = bad != 0 || run != (unsigned)(n_int - 1);
    for (int k = tid; k <= n_int; k += JI_THREADS) {
        if (k == 0) p[0] = s0;
        else if (k == n_int || (unsigned)k > run) p[k] = s1 + 2;        // as if EOI were the marker that closes it
        if (k < n_int) status[(size_t)f * n_int + k] = wrong ? MBX_JPEG_DEC_MARKERS : MBX_JPEG_DEC_OK;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// entropy decoding: one lane per restart interval (the body: jpeg_decode_interval, jpeg_dec_common.h)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JD_THREADS) void jpeg_entropy_dec_kernel(const unsigned char* __restrict__ data, long long data_bytes,
                                                                      const long long* __restrict__ pos, const unsigned* __restrict__ tables,
                                                                      DGeo g, int restart, int n_int, long long n_all, short* __restrict__ coef,
                                                                      int* __restrict__ status) {
    __shared__ unsigned tab[6 * TW];
    for (int i = threadIdx.x; i < 6 * TW; i += JD_THREADS) tab[i] = tables[i];
    __syncthreads();
    const long long t = (long long)blockIdx.x * JD_THREADS + threadIdx.x;
    if (t >= n_all) return;
    if (status[t] != MBX_JPEG_DEC_OK) return;                            // the frame's markers are wrong: its coefficients stay zero
    jpeg_decode_interval(data, data_bytes, pos, tab, g, restart, n_int, t, coef, status);
}

// ---------------------------------------------------------------------------------------------------------------
// dequantise, IDCT, range limit -> component planes
// ---------------------------------------------------------------------------------------------------------------
struct QTables { unsigned short q[3][64]; };                            // per component, in zigzag order as the file has them

struct InvZig { unsigned char z[64]; };
constexpr InvZig derive_invzig() {
    InvZig r = {};
    for (int i = 0; i < 64; ++i) r.z[kZigzag[i]] = (unsigned char)i;
    return r;
}
__device__ const InvZig d_invzig = derive_invzig();                      // natural index -> zigzag position

__device__ __forceinline__ unsigned jpeg_range_limit(long long v) {
    const int i = (int)(v & 1023);
    return i < 128 ? 128u + i : i < 512 ? 255u : i < 896 ? 0u : (unsigned)(i - 896);
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_idct_kernel(const short* __restrict__ coef, DGeo g, QTables qt, long long n_blk,
                                                               unsigned char* __restrict__ planes) {
    __shared__ int tile[JP_BLOCKS * JP_PITCH];
    __shared__ __align__(16) short cin[JP_BLOCKS * 64];
    const int tid = threadIdx.x, b = tid >> 3, r = tid & 7;
    const long long blk = (long long)blockIdx.x * JP_BLOCKS + b;
    const bool live = blk < n_blk;
    const int per_frame = g.n_mcu * g.bpm;
    const int f = live ? (int)(blk / per_frame) : 0, rem = live ? (int)(blk % per_frame) : 0;
    const int m = rem / g.bpm, k = rem % g.bpm, ny = g.bpm - 2;
    const int comp = k < ny ? 0 : k - ny + 1;
    if (live) reinterpret_cast<uint4*>(cin)[tid] = reinterpret_cast<const uint4*>(coef + blk * 64)[r];
    __syncthreads();
    if (live) {                                                          // column r
        long long d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int zz = d_invzig.z[i * 8 + r];
            d[i] = (long long)cin[b * 64 + zz] * (long long)qt.q[comp][zz];
        }
        MBX_JPEG_IDCT_PASS(d, 11);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[b * JP_PITCH + i * 8 + r] = (int)d[i];
    }
    __syncthreads();
    if (live) {                                                          // row r
        long long d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = tile[b * JP_PITCH + r * 8 + j];
        MBX_JPEG_IDCT_PASS(d, 18);
        unsigned w[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j >> 2] |= jpeg_range_limit(d[j]) << (8 * (j & 3));
        const int my_ = m / g.mx, mx_ = m % g.mx;
        unsigned char* fr = planes + (size_t)f * g.frame_bytes;
        size_t at;
        if (comp == 0) {
            const int bx = g.hs * mx_ + (k % g.hs), by = g.vs * my_ + (k / g.hs);
            at = ((size_t)by * 8 + r) * g.yw + (size_t)bx * 8;
        } else {
            at = (size_t)g.y_bytes + (size_t)(comp - 1) * g.c_bytes + ((size_t)my_ * 8 + r) * g.cw + (size_t)mx_ * 8;
        }
        *reinterpret_cast<uint2*>(fr + at) = make_uint2(w[0], w[1]);    // 8-byte aligned: every width and plane size is a multiple of 8
    }
}

// ---------------------------------------------------------------------------------------------------------------
// fancy upsampling and colour: four consecutive pixels of the output per lane
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int jpeg_chroma(const unsigned char* __restrict__ c, const DGeo& g, int y, int x) {
    if (g.sub == 0) return c[(size_t)y * g.cw + x];
    const int cx = x >> 1;
    if (g.dw <= 2) return c[(size_t)(g.sub == 1 ? y >> 1 : y) * g.cw + cx];      // libjpeg replicates where the fancy filters have no room
    if (g.sub == 2) {
        const unsigned char* row = c + (size_t)y * g.cw;
        const int v = row[cx];
        if (x & 1) return cx == g.dw - 1 ? v : (3 * v + row[cx + 1] + 2) >> 2;
        return cx == 0 ? v : (3 * v + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    int ry = (y & 1) ? cy + 1 : cy - 1;
    ry = ry < 0 ? 0 : ry > g.dh - 1 ? g.dh - 1 : ry;                     // the last REAL row, not the padded plane's
    const unsigned char* r0 = c + (size_t)cy * g.cw;
    const unsigned char* r1 = c + (size_t)ry * g.cw;
    const int s = 3 * r0[cx] + r1[cx];
    if (x & 1) return cx == g.dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(JC_THREADS) void jpeg_colour_kernel(const unsigned char* __restrict__ planes, DGeo g, long long n_pix, int pad,
                                                                 unsigned char* __restrict__ rgb) {
    // group t holds pixels 4 t - pad .. 4 t - pad + 3: pad = the pixels missing in front so that every whole group starts at a 4-byte address
    const long long q0 = ((long long)blockIdx.x * JC_THREADS + threadIdx.x) * 4 - pad;
    const long long p0 = q0 < 0 ? 0 : q0;
    if (p0 >= n_pix) return;
    const long long row0 = p0 / g.W;
    int x = (int)(p0 % g.W), y = (int)(row0 % g.H);
    long long f = row0 / g.H;
    unsigned char out[12];
    const long long p1 = q0 + 4 < n_pix ? q0 + 4 : n_pix;
    const int n = (int)(p1 - p0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < n) {
            const unsigned char* fr = planes + (size_t)f * g.frame_bytes;
            const int Y = fr[(size_t)y * g.yw + x];
            const int cb = jpeg_chroma(fr + g.y_bytes, g, y, x) - 128, cr = jpeg_chroma(fr + g.y_bytes + g.c_bytes, g, y, x) - 128;
            out[3 * e] = (unsigned char)clamp255(Y + ((91881 * cr + 32768) >> 16));
            out[3 * e + 1] = (unsigned char)clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
            out[3 * e + 2] = (unsigned char)clamp255(Y + ((116130 * cb + 32768) >> 16));
            if (++x == g.W) { x = 0; if (++y == g.H) { y = 0; ++f; } }
        }
    }
    if (n == 4) {                                                        // 12 bytes at a 4-byte address
        unsigned* dst = reinterpret_cast<unsigned*>(rgb + 3 * p0);
#pragma unroll
        for (int j = 0; j < 3; ++j) dst[j] = out[4 * j] | out[4 * j + 1] << 8 | out[4 * j + 2] << 16 | (unsigned)out[4 * j + 3] << 24;
    } else {
        for (int j = 0; j < 3 * n; ++j) rgb[3 * p0 + j] = out[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int dec_check(const char* who, int F, int H, int W, int sub) {
    MBX_CHECK_ARG(F >= 0 && F <= MBX_JPEG_MAX_FRAMES && H >= 1 && H <= MBX_JPEG_MAX_SIZE && W >= 1 && W <= MBX_JPEG_MAX_SIZE,
                  "%s: bad sizes F=%d H=%d W=%d (0 <= F <= %d, 1 <= H, W <= %d)", who, F, H, W, MBX_JPEG_MAX_FRAMES, MBX_JPEG_MAX_SIZE);
    MBX_CHECK_ARG(sub >= 0 && sub <= 2, "%s: subsampling %d (0: 4:4:4, 1: 4:2:0, 2: 4:2:2)", who, sub);
    return 0;
}

// (bits [16], vals [256]) -> one table of TW words; 1 where they are no Huffman table
int derive_table(const unsigned char* bits, const unsigned char* vals, bool dc, unsigned* out) {
    unsigned short* look = reinterpret_cast<unsigned short*>(out);
    int* maxcode = reinterpret_cast<int*>(out + 128);
    int* valoff = maxcode + 18;
    unsigned char* v = reinterpret_cast<unsigned char*>(out + 164);
    for (int i = 0; i < TW; ++i) out[i] = 0u;
    int total = 0;
    for (int l = 0; l < 16; ++l) total += bits[l];
    if (total > 256) return 1;
    for (int i = 0; i < total; ++i) {
        if (dc && vals[i] > 15) return 1;
        v[i] = vals[i];
    }
    int code = 0, k = 0;
    maxcode[0] = -1; maxcode[17] = 0x7fffffff;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (code + n > (1 << l)) return 1;                               // more codes than the length has
        valoff[l] = k - code;
        if (l <= 8)
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < (1 << (8 - l)); ++j) look[((code + i) << (8 - l)) + j] = (unsigned short)(l << 8 | vals[k + i]);
        maxcode[l] = n ? code + n - 1 : -1;
        code = (code + n) << 1;
        k += n;
    }
    return 0;
}

}  // namespace

extern "C" int mbx_jpeg_dec_tables(const unsigned char* dht, unsigned* out) {
    MBX_CHECK_ARG(out, "jpeg_dec_tables: null pointer");
    for (int t = 0; t < 6; ++t) {
        unsigned char bits[16], vals[256] = {};
        if (dht) {
            for (int i = 0; i < 16; ++i) bits[i] = dht[t * 272 + i];
            for (int i = 0; i < 256; ++i) vals[i] = dht[t * 272 + 16 + i];
        } else {
            const int a = (t >= 2 ? 2 : 0) + (t & 1);                    // luminance tables for component 0, chrominance for 1 and 2
            for (int i = 0; i < 16; ++i) bits[i] = kBits[a][i];
            for (int i = 0; i < kNVals[a]; ++i) vals[i] = kVals[a][i];
        }
        MBX_CHECK_ARG(derive_table(bits, vals, (t & 1) == 0, out + t * TW) == 0,
                      "jpeg_dec_tables: table %d (%s of component %d) is no Huffman table a baseline scan can use", t, t & 1 ? "AC" : "DC", t / 2);
    }
    return 0;
}

extern "C" int mbx_jpeg_dec_index(const unsigned char* data, long long data_bytes, const long long* scans, int F, int n_int, long long* pos,
                                  int* status, void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= MBX_JPEG_MAX_FRAMES && n_int >= 1 && n_int <= MBX_JPEG_MAX_SIZE * MBX_JPEG_MAX_SIZE / 64 && data_bytes >= 0,
                  "jpeg_dec_index: bad sizes F=%d n_int=%d data_bytes=%lld", F, n_int, data_bytes);
    if (F == 0) return 0;
    MBX_CHECK_ARG(data && scans && pos && status, "jpeg_dec_index: null pointer");
    MBX_CHECK_ARG(((uintptr_t)scans & 7) == 0 && ((uintptr_t)pos & 7) == 0 && ((uintptr_t)status & 3) == 0, "jpeg_dec_index: misaligned pointer");
    hipLaunchKernelGGL(jpeg_index_kernel, dim3(F), dim3(JI_THREADS), 0, (hipStream_t)stream, data, data_bytes, scans, n_int, pos, status);
    MBX_LAUNCH_CHECK("jpeg_dec_index");
    return 0;
}

extern "C" int mbx_jpeg_dec_entropy(const unsigned char* data, long long data_bytes, const long long* pos, const unsigned* tables, int F, int H,
                                    int W, int sub, int restart, short* coef, int* status, void* stream) {
    if (dec_check("jpeg_dec_entropy", F, H, W, sub)) return 1;
    MBX_CHECK_ARG(restart >= 0 && restart <= 65535 && data_bytes >= 0, "jpeg_dec_entropy: restart interval %d (0: none, .. 65535 MCUs), data_bytes %lld",
                  restart, data_bytes);
    if (F == 0) return 0;
    MBX_CHECK_ARG(data && pos && tables && coef && status, "jpeg_dec_entropy: null pointer");
    MBX_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)pos & 7) == 0 && ((uintptr_t)tables & 3) == 0 && ((uintptr_t)status & 3) == 0,
                  "jpeg_dec_entropy: coef must be 16-byte aligned, pos 8-byte, tables and status 4-byte");
    const DGeo g = make_dgeo(H, W, sub);
    const int n_int = restart ? (g.n_mcu + restart - 1) / restart : 1;
    const long long n_all = (long long)F * n_int;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)F * g.n_mcu * g.bpm * 64 * sizeof(short), (hipStream_t)stream);
    if (e != hipSuccess) return mbx_set_error("jpeg_dec_entropy: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(jpeg_entropy_dec_kernel, dim3((unsigned)((n_all + JD_THREADS - 1) / JD_THREADS)), dim3(JD_THREADS), 0, (hipStream_t)stream,
                       data, data_bytes, pos, tables, g, restart, n_int, n_all, coef, status);
    MBX_LAUNCH_CHECK("jpeg_dec_entropy");
    return 0;
}

extern "C" size_t mbx_jpeg_dec_ws(int F, int H, int W, int sub) {
    if (F < 1 || F > MBX_JPEG_MAX_FRAMES || H < 1 || H > MBX_JPEG_MAX_SIZE || W < 1 || W > MBX_JPEG_MAX_SIZE || sub < 0 || sub > 2) return 0;
    return ((size_t)F * make_dgeo(H, W, sub).frame_bytes + 15) & ~(size_t)15;
}

extern "C" int mbx_jpeg_dec_pixels(const short* coef, const unsigned char* q, int F, int H, int W, int sub, unsigned char* rgb, void* ws,
                                   size_t ws_bytes, void* stream) {
    if (dec_check("jpeg_dec_pixels", F, H, W, sub)) return 1;
    if (F == 0) return 0;
    MBX_CHECK_ARG(coef && q && rgb && ws, "jpeg_dec_pixels: null pointer");
    MBX_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)ws & 15) == 0, "jpeg_dec_pixels: coef and ws must be 16-byte aligned");
    MBX_CHECK_ARG(ws_bytes >= mbx_jpeg_dec_ws(F, H, W, sub), "jpeg_dec_pixels: workspace of %zu bytes, %zu needed", ws_bytes, mbx_jpeg_dec_ws(F, H, W, sub));
    const DGeo g = make_dgeo(H, W, sub);
    QTables qt;
    for (int i = 0; i < 192; ++i) {
        MBX_CHECK_ARG(q[i] >= 1, "jpeg_dec_pixels: quantisation entry %d of component %d is 0", i & 63, i >> 6);
        qt.q[i >> 6][i & 63] = q[i];
    }
    const long long n_blk = (long long)F * g.n_mcu * g.bpm, n_pix = (long long)F * H * W;
    const int pad = (int)((4 - ((uintptr_t)rgb & 3)) & 3);              // rgb + 3 (4 t - pad) is a multiple of 4 for every t (a slice of frames starts anywhere)
    const long long grid_a = (n_blk + JP_BLOCKS - 1) / JP_BLOCKS, grid_b = ((n_pix + pad + 3) / 4 + JC_THREADS - 1) / JC_THREADS;
    MBX_CHECK_ARG(grid_a <= 0x7fffffffll && grid_b <= 0x7fffffffll, "jpeg_dec_pixels: %d frames of %d x %d are too many for one launch", F, H, W);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)grid_a), dim3(JP_THREADS), 0, (hipStream_t)stream, coef, g, qt, n_blk, (unsigned char*)ws);
    MBX_LAUNCH_CHECK("jpeg_dec_pixels (idct)");
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)grid_b), dim3(JC_THREADS), 0, (hipStream_t)stream, (const unsigned char*)ws, g, n_pix, pad, rgb);
    MBX_LAUNCH_CHECK("jpeg_dec_pixels (colour)");
    return 0;
}
