// Streamed attention for long sequences (L > 256: temporal attention over more than 256 frames) for gfx950.
//
// The resident kernels of attention.hip keep a whole problem's K / V (or Q / dO) in LDS and give each of at most eight waves one
// 32-row block.  Here the sequence is cut into blocks of 256 rows, one workgroup of eight waves each (32 rows per wave, in
// registers), and the other operand pair streams through a double-buffered LDS ring of 64-row tiles that all eight waves share:
//   attn_fwd_stream_kernel       lane = query; K / V tiles stream; the online softmax of attn_fwd_kernel
//   attn_bwd_dq_stream_kernel    lane = query; K / V tiles stream; delta = dO.O and lse are per-lane row constants
//   attn_bwd_dkv_stream_kernel   lane = key;   Q / dO tiles stream together with their rows' lse and delta = dO.O, the latter
//                                reduced (DPP) from the O chunks fetched beside the dO chunks of the tile fill
// grid = problems x ceil(L / 256), the blocks of one problem in consecutive workgroups (its tiles are shared in L2).  Per tile: the
// global loads of tile t + 1 are issued into registers, the MFMAs run on tile t, the registers go to the other ring slot, one
// barrier.  MFMA forms, probability arithmetic and the dropout mask index (over the full L) are those of the resident kernels
// (attention_common.h).  Padded rows of every tile are zero, which keeps padded keys out of dQ (zero K row) and padded queries out of
// dK / dV (zero Q and dO rows, lse = delta = 0); fragments wholly past L are skipped.  Outputs are staged in the ring (dead by then)
// and copied out as whole row segments.  With the row-dot output (bf16, st_part) the original q / k / v rows are staged first, so
// store_rowfrag_dot takes its dots exactly as in the resident kernels.
#include "attention_common.h"

constexpr int MBX_STREAM_THREADS = 512;                          // eight waves
constexpr int MBX_STREAM_BLOCK = 32 * MBX_STREAM_THREADS / 64;   // rows (queries or keys) per workgroup: 32 per wave
constexpr int MBX_STREAM_TILE = 64;                              // rows per streamed tile

// ring slot fill, split in two so that the loads of the next tile are in flight during the current tile's MFMAs.
// load(): rows row0 .. row0 + 64 of two sources (row stride rs elements) into registers, rows >= L as zeros; store(): into LDS
template <typename T, int HD> struct RingPair {
    static constexpr int CH = HD / AT<T>::EPC, RSTR = rm_stride<T>(HD);
    static constexpr int NPT = (MBX_STREAM_TILE * CH + MBX_STREAM_THREADS - 1) / MBX_STREAM_THREADS;
    uint4 a[NPT], b[NPT];
    __device__ __forceinline__ void load(const T* srcA, const T* srcB, size_t rs, int row0, int L, int tid) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int idx = tid + i * MBX_STREAM_THREADS, row = row0 + idx / CH, ch = idx % CH;
            a[i] = make_uint4(0u, 0u, 0u, 0u);
            b[i] = make_uint4(0u, 0u, 0u, 0u);
            if (idx < MBX_STREAM_TILE * CH && row < L) {
                a[i] = *reinterpret_cast<const uint4*>(srcA + (size_t)row * rs + ch * AT<T>::EPC);
                b[i] = *reinterpret_cast<const uint4*>(srcB + (size_t)row * rs + ch * AT<T>::EPC);
            }
        }
    }
    __device__ __forceinline__ void store(char* dstA, char* dstB, int tid) const {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int idx = tid + i * MBX_STREAM_THREADS, off = (idx / CH) * RSTR + (idx % CH) * 16;
            if (idx < MBX_STREAM_TILE * CH) {
                *reinterpret_cast<uint4*>(dstA + off) = a[i];
                *reinterpret_cast<uint4*>(dstB + off) = b[i];
            }
        }
    }
};

// dot of two 16-byte chunks (dO . O over 8 bf16 or 4 floats)
__device__ __forceinline__ float chunk_dot(const uint4& x, const uint4& y, bf16_t) {
    const uint32_t xa[4] = {x.x, x.y, x.z, x.w}, ya[4] = {y.x, y.y, y.z, y.w};
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d = fmaf(__uint_as_float(xa[i] << 16), __uint_as_float(ya[i] << 16), d);
        d = fmaf(__uint_as_float(xa[i] & 0xffff0000u), __uint_as_float(ya[i] & 0xffff0000u), d);
    }
    return d;
}
__device__ __forceinline__ float chunk_dot(const uint4& x, const uint4& y, float) {
    return fmaf(__uint_as_float(x.x), __uint_as_float(y.x), fmaf(__uint_as_float(x.y), __uint_as_float(y.y),
                fmaf(__uint_as_float(x.z), __uint_as_float(y.z), __uint_as_float(x.w) * __uint_as_float(y.w))));
}
// sum over the CH consecutive, CH-aligned lanes (CH in {4, 8, 16}) that hold the chunks of one row; every lane must be active
template <int CH> __device__ __forceinline__ float row_chunk_sum(float v) {
    v += dpp_mov<0xB1>(v, v);                         // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v, v);                         // quad_perm [2,3,0,1]
    if (CH >= 8) v += dpp_mov<0x141>(v, v);           // row_half_mirror: the other quad of eight lanes
    if (CH >= 16) v += dpp_mov<0x140>(v, v);          // row_mirror: the other eight of sixteen lanes
    return v;
}

// rows 0 .. nrows of one head's columns (bf16, row stride rs) into the row-major staging area: the originals the row dots are taken against
template <int HD>
__device__ __forceinline__ void stage_rows(char* stg, const bf16_t* src, size_t rs, int nrows, int tid) {
    constexpr int CH = HD / 8, RSTR = rm_stride<bf16_t>(HD);
    for (int idx = tid; idx < nrows * CH; idx += MBX_STREAM_THREADS) {
        const int r = idx / CH, ch = idx % CH;
        *reinterpret_cast<uint4*>(stg + r * RSTR + ch * 16) = *reinterpret_cast<const uint4*>(src + (size_t)r * rs + ch * 8);
    }
}
// staged rows -> global rows off0 + r * rs (elements of T), whole row segments per instruction; `lo` != null: fp32 rows leave as the
// two bf16 planes of the bf16x3 split (dst = the hi plane), as in the copy-out of attn_bwd_small_kernel
template <typename T, int HD>
__device__ __forceinline__ void copy_rows_out(const char* stg, void* dst, bf16_t* lo, size_t off0, size_t rs, int nrows, int tid) {
    constexpr int CH = HD * (int)sizeof(T) / 16, RSTR = rm_stride<T>(HD), EPC = 16 / (int)sizeof(T);
    for (int idx = tid; idx < nrows * CH; idx += MBX_STREAM_THREADS) {
        const int r = idx / CH, ch = idx % CH;
        const uint4 a = *reinterpret_cast<const uint4*>(stg + r * RSTR + ch * 16);
        const size_t eo = off0 + (size_t)r * rs + ch * EPC;
        if (sizeof(T) == 4 && lo) {
            const float v[4] = {__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)};
            store4_planes(reinterpret_cast<bf16_t*>(dst) + eo, lo + eo, v);
        } else {
            *reinterpret_cast<uint4*>(reinterpret_cast<T*>(dst) + eo) = a;
        }
    }
}

// ================================================================================================
// forward   (lane = query)
// ================================================================================================
template <typename T, int HD, bool DROP>
__global__ __launch_bounds__(MBX_STREAM_THREADS, (sizeof(T) == 2 && !DROP) ? 4 : 1) void attn_fwd_stream_kernel(
        const T* __restrict__ qkv, T* __restrict__ o, float* __restrict__ lse, int Tn, int J, int H, float scale, int mode, int nblk,
        MbxDrop dr) {
    constexpr int RSTR = rm_stride<T>(HD), TILE = MBX_STREAM_TILE * RSTR;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // ring: slot s = K tile at 2 s TILE, V tile behind it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5;
    const int C = H * HD, C3 = 3 * C;
    const Prob P = decode_prob((int)blockIdx.x / nblk, mode, Tn, J, H);
    const int q0 = ((int)blockIdx.x % nblk) * MBX_STREAM_BLOCK;
    const size_t rstride = (size_t)P.tstep * C3;
    const T* base = qkv + P.tok0 * C3 + (size_t)P.h * HD;
    const int q = q0 + wave * 32 + (lane & 31);
    const bool wact = q0 + wave * 32 < P.L;          // wave-uniform: this wave's block holds >= 1 query
    const bool qvalid = q < P.L;
    const size_t tok = P.tok0 + (size_t)min(q, P.L - 1) * P.tstep;
    BReg<T, HD> qreg;
    qreg.load(qkv + tok * C3 + (size_t)P.h * HD, g, qvalid);
    RingPair<T, HD> rg;
    rg.load(base + C, base + 2 * C, rstride, 0, P.L, tid);
    rg.store(smem, smem + TILE, tid);
    __syncthreads();

    const float c2 = scale * 1.44269504088896341f;
    f32x16_t oacc[HD / 32];
#pragma unroll
    for (int df = 0; df < HD / 32; ++df)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[df][r] = 0.f;
    float m2 = -INFINITY, l = 0.f;      // l: this lane's half of the row sum (lanes l, l^32 share a query)
    const int ntile = (P.L + MBX_STREAM_TILE - 1) / MBX_STREAM_TILE;
    for (int t = 0; t < ntile; ++t) {
        const char* kt = smem + (t & 1) * 2 * TILE;
        const char* vt = kt + TILE;
        const int k0 = t * MBX_STREAM_TILE;
        if (t + 1 < ntile) rg.load(base + C, base + 2 * C, rstride, k0 + MBX_STREAM_TILE, P.L, tid);
        if (wact) {
            const int nf = min(MBX_STREAM_TILE / 32, (P.L - k0 + 31) / 32);     // fragments with >= 1 valid key
            for (int f = 0; f < nf; ++f) {
                f32x16_t s;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = 0.f;
                MmaRows<T, HD>::run(kt, RSTR, 32 * f, qreg, lane, s);
                if (k0 + 32 * f + 32 > P.L) {   // wave-uniform: the last, partial fragment
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + 32 * f + (r & 3) + 8 * (r >> 2) + 4 * g;
                        s[r] = key < P.L ? s[r] : -INFINITY;
                    }
                }
                float mx = s[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
                mx = wave_halves<WaveMax>(mx);   // >= 1 valid key per fragment: finite
                const float mn2 = fmaxf(m2, mx * c2);
                const float corr = __builtin_amdgcn_exp2f(m2 - mn2);        // first fragment: 2^(-inf) = 0
                float ps = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -mn2));
                    ps += s[r];
                }
                l = fmaf(l, corr, ps);
                m2 = mn2;
                if (DROP) {       // the row sum above is the undropped one; what multiplies V carries the mask
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[r] *= drop_mul(dr, P.dbase, q, k0 + 32 * f + (r & 3) + 8 * (r >> 2) + 4 * g, P.L);
                }
#pragma unroll
                for (int df = 0; df < HD / 32; ++df) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[df][r] *= corr;
                    MmaCols<T>::run(vt, RSTR, df * 32, f, s, lane, oacc[df]);
                }
            }
        }
        if (t + 1 < ntile) {
            char* nk = smem + ((t + 1) & 1) * 2 * TILE;
            rg.store(nk, nk + TILE, tid);
        }
        __syncthreads();      // slot t + 1 is filled; every wave is done with slot t, which the next iteration refills
    }
    if (wact) {
        l = wave_halves<WaveAdd>(l);
        if (qvalid && g == 0) lse[tok * H + P.h] = (m2 + __builtin_amdgcn_logf(l)) * 0.69314718055994531f;   // natural-log units
        // the ring (4 tiles = 256 rows) is the staging area of the workgroup's 256 query rows
        store_rowfrag<T, HD>(reinterpret_cast<T*>(smem + (size_t)(wave * 32 + (lane & 31)) * RSTR), oacc, 1.0f / l, g);
    }
    __syncthreads();
    copy_rows_out<T, HD>(smem, o, nullptr, (P.tok0 + (size_t)q0 * P.tstep) * C + (size_t)P.h * HD, (size_t)P.tstep * C,
                         min(MBX_STREAM_BLOCK, P.L - q0), tid);
}

// ================================================================================================
// backward, dQ   (lane = query)
// ================================================================================================
template <typename T, int HD, bool DROP, bool STATS>
__global__ __launch_bounds__(MBX_STREAM_THREADS, 1) void attn_bwd_dq_stream_kernel(
        const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o, const float* __restrict__ lse, T* __restrict__ dqkv,
        int Tn, int J, int H, float scale, int mode, int nblk, MbxDrop dr, bf16_t* __restrict__ dq_lo, const float* __restrict__ st_bias,
        const float* __restrict__ st_rsum, float* __restrict__ st_part) {
    constexpr int RSTR = rm_stride<T>(HD), TILE = MBX_STREAM_TILE * RSTR;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // ring (4 tiles) | row-dot vectors (STATS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5;
    const int C = H * HD, C3 = 3 * C;
    const Prob P = decode_prob((int)blockIdx.x / nblk, mode, Tn, J, H);
    const int q0 = ((int)blockIdx.x % nblk) * MBX_STREAM_BLOCK;
    const size_t rstride = (size_t)P.tstep * C3;
    const T* base = qkv + P.tok0 * C3 + (size_t)P.h * HD;
    uint4* vec = reinterpret_cast<uint4*>(smem + 4 * TILE);
    if (STATS) fill_stat_vec<HD>(vec, st_rsum, st_bias, C, P.h, tid, MBX_STREAM_THREADS);
    const int q = q0 + wave * 32 + (lane & 31);
    const bool wact = q0 + wave * 32 < P.L;
    const bool qvalid = q < P.L;
    const size_t tok = P.tok0 + (size_t)min(q, P.L - 1) * P.tstep;
    RingPair<T, HD> rg;
    rg.load(base + C, base + 2 * C, rstride, 0, P.L, tid);
    BReg<T, HD> qreg, doreg;
    float delta, lq2;
    {
        BReg<T, HD> oreg;
        qreg.load(qkv + tok * C3 + (size_t)P.h * HD, g, qvalid);
        doreg.load(d_o + tok * C + (size_t)P.h * HD, g, qvalid);
        oreg.load(o + tok * C + (size_t)P.h * HD, g, qvalid);
        lq2 = qvalid ? lse[tok * H + P.h] * 1.44269504088896341f : 0.f;
        delta = wave_halves<WaveAdd>(BReg<T, HD>::dot(doreg, oreg));
    }
    rg.store(smem, smem + TILE, tid);
    __syncthreads();

    // p = 2^(s*c2 - lse*log2 e); no masks: an invalid query lane is never stored, a padded key has a zero K row (dS K = 0)
    const float c2 = scale * 1.44269504088896341f;
    f32x16_t dq[HD / 32];
#pragma unroll
    for (int df = 0; df < HD / 32; ++df)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[df][r] = 0.f;
    const int ntile = (P.L + MBX_STREAM_TILE - 1) / MBX_STREAM_TILE;
    for (int t = 0; t < ntile; ++t) {
        const char* kt = smem + (t & 1) * 2 * TILE;
        const char* vt = kt + TILE;
        const int k0 = t * MBX_STREAM_TILE;
        if (t + 1 < ntile) rg.load(base + C, base + 2 * C, rstride, k0 + MBX_STREAM_TILE, P.L, tid);
        if (wact) {
            const int nf = min(MBX_STREAM_TILE / 32, (P.L - k0 + 31) / 32);
            for (int f = 0; f < nf; ++f) {
                f32x16_t s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
                MmaRows<T, HD>::run(kt, RSTR, 32 * f, qreg, lane, s);
                MmaRows<T, HD>::run(vt, RSTR, 32 * f, doreg, lane, dp);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -lq2));
                    const float dpr = DROP ? dp[r] * drop_mul(dr, P.dbase, q, k0 + 32 * f + (r & 3) + 8 * (r >> 2) + 4 * g, P.L) : dp[r];
                    s[r] = p * (dpr - delta) * scale;  // dS
                }
#pragma unroll
                for (int df = 0; df < HD / 32; ++df) MmaCols<T>::run(kt, RSTR, df * 32, f, s, lane, dq[df]);
            }
        }
        if (t + 1 < ntile) {
            char* nk = smem + ((t + 1) & 1) * 2 * TILE;
            rg.store(nk, nk + TILE, tid);
        }
        __syncthreads();
    }
    const int nrows = min(MBX_STREAM_BLOCK, P.L - q0);
    const size_t off0 = (P.tok0 + (size_t)q0 * P.tstep) * C3 + (size_t)P.h * HD;
    char* stg = smem + (size_t)(wave * 32 + (lane & 31)) * RSTR;
    if constexpr (STATS) {
        stage_rows<HD>(smem, qkv + off0, rstride, nrows, tid);       // the q rows the dots are taken against
        __syncthreads();
        float p1 = 0.f, p2 = 0.f;
        if (wact) store_rowfrag_dot<HD>(reinterpret_cast<bf16_t*>(stg), dq, g, vec, p1, p2);
        p1 = wave_halves<WaveAdd>(p1);
        p2 = wave_halves<WaveAdd>(p2);
        if (qvalid && g == 0) {     // part[2 h + 0][token]
            const size_t Mtot = (size_t)(gridDim.x / nblk / H) * P.L;
            *reinterpret_cast<float2*>(st_part + ((size_t)(2 * P.h) * Mtot + tok) * 2) = make_float2(p1, p2);
        }
    } else {
        if (wact) store_rowfrag<T, HD>(reinterpret_cast<T*>(stg), dq, 1.0f, g);
    }
    __syncthreads();
    copy_rows_out<T, HD>(smem, dqkv, dq_lo, off0, rstride, nrows, tid);
}

// ================================================================================================
// backward, dK and dV   (lane = key)
// ================================================================================================
template <typename T, int HD, bool DROP, bool STATS>
__global__ __launch_bounds__(MBX_STREAM_THREADS, 1) void attn_bwd_dkv_stream_kernel(
        const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o, const float* __restrict__ lse, T* __restrict__ dqkv,
        int Tn, int J, int H, float scale, int mode, int nblk, MbxDrop dr, bf16_t* __restrict__ dq_lo, const float* __restrict__ st_bias,
        const float* __restrict__ st_rsum, float* __restrict__ st_part) {
    typedef RingPair<T, HD> Ring;
    constexpr int RSTR = rm_stride<T>(HD), TILE = MBX_STREAM_TILE * RSTR, CH = Ring::CH, NPT = Ring::NPT;
    constexpr int SLOT = 2 * TILE + 2 * MBX_STREAM_TILE * 4;         // Q tile | dO tile | lse (base 2) | delta
    extern __shared__ __attribute__((aligned(16))) char smem[];      // ring (2 slots >= 256 staging rows) | row-dot vectors (STATS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5;
    const int C = H * HD, C3 = 3 * C;
    const Prob P = decode_prob((int)blockIdx.x / nblk, mode, Tn, J, H);
    const int k0b = ((int)blockIdx.x % nblk) * MBX_STREAM_BLOCK;
    const size_t rstride = (size_t)P.tstep * C3, ostride = (size_t)P.tstep * C;
    const T* qbase = qkv + P.tok0 * C3 + (size_t)P.h * HD;
    const T* dobase = d_o + P.tok0 * C + (size_t)P.h * HD;
    const T* obase = o + P.tok0 * C + (size_t)P.h * HD;
    uint4* vec = reinterpret_cast<uint4*>(smem + 2 * SLOT);
    if (STATS) fill_stat_vec<HD>(vec, st_rsum, st_bias, C, P.h, tid, MBX_STREAM_THREADS);
    const int key = k0b + wave * 32 + (lane & 31);
    const bool wact = k0b + wave * 32 < P.L;
    const bool kvalid = key < P.L;
    const size_t ktok = P.tok0 + (size_t)min(key, P.L - 1) * P.tstep;

    // tile fill: the Q and dO chunks of the tile, the O chunk beside each dO chunk (for delta), lse by the row's first lane
    Ring rg;
    uint4 oc[NPT];
    float lsev[NPT];
    auto load = [&](int row0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int idx = tid + i * MBX_STREAM_THREADS, row = row0 + idx / CH, ch = idx % CH;
            rg.a[i] = rg.b[i] = oc[i] = make_uint4(0u, 0u, 0u, 0u);
            lsev[i] = 0.f;
            if (idx < MBX_STREAM_TILE * CH && row < P.L) {
                rg.a[i] = *reinterpret_cast<const uint4*>(qbase + (size_t)row * rstride + ch * AT<T>::EPC);
                rg.b[i] = *reinterpret_cast<const uint4*>(dobase + (size_t)row * ostride + ch * AT<T>::EPC);
                oc[i] = *reinterpret_cast<const uint4*>(obase + (size_t)row * ostride + ch * AT<T>::EPC);
                if (ch == 0) lsev[i] = lse[(P.tok0 + (size_t)row * P.tstep) * H + P.h];
            }
        }
    };
    auto store = [&](char* slot) __attribute__((always_inline)) {
        rg.store(slot, slot + TILE, tid);
        float* lse_s = reinterpret_cast<float*>(slot + 2 * TILE);
        float* del_s = lse_s + MBX_STREAM_TILE;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {       // every lane takes part in the DPP steps: chunks past the tile are zeros
            const int idx = tid + i * MBX_STREAM_THREADS, row = idx / CH, ch = idx % CH;
            const float dl = row_chunk_sum<CH>(chunk_dot(rg.b[i], oc[i], T()));
            if (ch == 0 && idx < MBX_STREAM_TILE * CH) {
                lse_s[row] = lsev[i] * 1.44269504088896341f;     // base-2 units: p = 2^(s*c2 - lse2)
                del_s[row] = dl;
            }
        }
    };
    load(0);
    BReg<T, HD> kreg, vreg;
    kreg.load(qkv + ktok * C3 + C + (size_t)P.h * HD, g, kvalid);
    vreg.load(qkv + ktok * C3 + 2 * C + (size_t)P.h * HD, g, kvalid);
    store(smem);
    __syncthreads();

    const float c2 = scale * 1.44269504088896341f;
    f32x16_t dk[HD / 32], dv[HD / 32];
#pragma unroll
    for (int df = 0; df < HD / 32; ++df)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[df][r] = 0.f; dv[df][r] = 0.f; }
    const int ntile = (P.L + MBX_STREAM_TILE - 1) / MBX_STREAM_TILE;
    for (int t = 0; t < ntile; ++t) {
        const char* qt = smem + (t & 1) * SLOT;
        const char* dot_ = qt + TILE;
        const float* lse_s = reinterpret_cast<const float*>(dot_ + TILE);
        const float* del_s = lse_s + MBX_STREAM_TILE;
        const int r0 = t * MBX_STREAM_TILE;
        if (t + 1 < ntile) load(r0 + MBX_STREAM_TILE);
        if (wact) {
            const int nf = min(MBX_STREAM_TILE / 32, (P.L - r0 + 31) / 32);     // fragments with >= 1 valid query
            for (int f = 0; f < nf; ++f) {
                f32x16_t s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
                MmaRows<T, HD>::run(qt, RSTR, 32 * f, kreg, lane, s);      // s[r]  <-> (query r0 + e(f,r,g), key = lane)
                MmaRows<T, HD>::run(dot_, RSTR, 32 * f, vreg, lane, dp);   // dP
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int ql = 32 * f + 8 * qd + 4 * g;
                    const float4 l4 = *reinterpret_cast<const float4*>(lse_s + ql);
                    const float4 d4 = *reinterpret_cast<const float4*>(del_s + ql);
                    const float la[4] = {l4.x, l4.y, l4.z, l4.w}, da[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * qd + e;
                        // no masks: padded queries have zero Q and dO rows and lse = delta = 0, invalid key lanes are not stored
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -la[e]));
                        const float km = DROP ? drop_mul(dr, P.dbase, r0 + ql + e, key, P.L) : 1.f;
                        dp[r] = p * (dp[r] * km - da[e]) * scale;  // dS
                        s[r] = p * km;                             // P (dropped: what multiplied V in forward)
                    }
                }
#pragma unroll
                for (int df = 0; df < HD / 32; ++df) {
                    MmaCols<T>::run(dot_, RSTR, df * 32, f, s, lane, dv[df]);   // dV^T += dO^T P
                    MmaCols<T>::run(qt, RSTR, df * 32, f, dp, lane, dk[df]);    // dK^T += Q^T dS
                }
            }
        }
        if (t + 1 < ntile) store(smem + ((t + 1) & 1) * SLOT);
        __syncthreads();
    }
    // dK, then dV, through the 256-row staging area (the ring)
    const int nrows = min(MBX_STREAM_BLOCK, P.L - k0b);
    const size_t off0 = (P.tok0 + (size_t)k0b * P.tstep) * C3 + (size_t)P.h * HD + C;
    char* stg = smem + (size_t)(wave * 32 + (lane & 31)) * RSTR;
    float p1 = 0.f, p2 = 0.f;
    auto out = [&](const f32x16_t (&acc)[HD / 32], int w) __attribute__((always_inline)) {
        if constexpr (STATS) {
            stage_rows<HD>(smem, qkv + off0 + w * C, rstride, nrows, tid);       // the k (v) rows the dots are taken against
            __syncthreads();
            if (wact) store_rowfrag_dot<HD>(reinterpret_cast<bf16_t*>(stg), acc, g, vec + (1 + w) * (HD / 4), p1, p2);
        } else {
            if (wact) store_rowfrag<T, HD>(reinterpret_cast<T*>(stg), acc, 1.0f, g);
        }
        __syncthreads();
        copy_rows_out<T, HD>(smem, dqkv, dq_lo, off0 + w * C, rstride, nrows, tid);
    };
    out(dk, 0);
    __syncthreads();      // the staging area is refilled by the dV pass
    out(dv, 1);
    if constexpr (STATS) {
        p1 = wave_halves<WaveAdd>(p1);
        p2 = wave_halves<WaveAdd>(p2);
        if (kvalid && g == 0) {     // part[2 h + 1][token]
            const size_t Mtot = (size_t)(gridDim.x / nblk / H) * P.L;
            *reinterpret_cast<float2*>(st_part + ((size_t)(2 * P.h + 1) * Mtot + ktok) * 2) = make_float2(p1, p2);
        }
    }
}

// ================================================================================================
// host side (argument checks: attn_fwd_impl / attn_bwd_impl in attention.hip)
// ================================================================================================
static int stream_grid(const char* who, int B, int T, int J, int H, int mode, int& nprob, int& nblk) {
    const long long np = mode == MBX_ATTN_SPATIAL ? (long long)B * T * H : (long long)B * J * H;
    const int L = mode == MBX_ATTN_SPATIAL ? J : T;
    nblk = (L + MBX_STREAM_BLOCK - 1) / MBX_STREAM_BLOCK;
    MBX_CHECK_ARG(np * nblk < (1LL << 31), "%s: %lld problems x %d sequence blocks exceed the launch grid", who, np, nblk);
    nprob = (int)np;
    return 0;
}

int mbx_launch_attn_fwd_stream(const void* qkv, void* o, float* lse, int B, int T, int J, int H, int hd, float scale, int mode, int dtype,
                               hipStream_t s, const MbxDrop& dr) {
    int nprob, nblk;
    if (stream_grid("attn_fwd", B, T, J, H, mode, nprob, nblk)) return 1;
    const dim3 grid((unsigned)(nprob * nblk)), block(MBX_STREAM_THREADS);
    return dispatch_attn(dtype, hd, dr.thresh != 0, [&](auto tag) {
        using E = typename decltype(tag)::type;
        const size_t shm = (size_t)4 * MBX_STREAM_TILE * rm_stride<E>(tag.HD);
        auto k = attn_fwd_stream_kernel<E, tag.HD, tag.DROP>;
        if (set_lds(k, shm, "attn_fwd_stream")) return 1;
        hipLaunchKernelGGL(k, grid, block, shm, s, (const E*)qkv, (E*)o, lse, T, J, H, scale, mode, nblk, dr);
        MBX_LAUNCH_CHECK("attn_fwd_stream");
        return 0;
    });
}

template <typename T, int HD, bool DROP, bool STATS>
static int launch_bwd_stream(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, int Tn, int J, int H,
                             float scale, int mode, int nprob, int nblk, hipStream_t s, const MbxDrop& dr, void* dq_lo,
                             const float* st_bias, const float* st_rsum, float* st_part) {
    constexpr int RSTR = rm_stride<T>(HD);
    const size_t vec = STATS ? (size_t)3 * HD * 4 : 0;      // 3 HD / 4 uint4
    const size_t shm1 = (size_t)4 * MBX_STREAM_TILE * RSTR + vec;
    const size_t shm2 = (size_t)2 * (2 * MBX_STREAM_TILE * RSTR + 2 * MBX_STREAM_TILE * 4) + vec;
    auto k1 = attn_bwd_dq_stream_kernel<T, HD, DROP, STATS>;
    auto k2 = attn_bwd_dkv_stream_kernel<T, HD, DROP, STATS>;
    if (set_lds(k1, shm1, "attn_bwd_dq_stream") || set_lds(k2, shm2, "attn_bwd_dkv_stream")) return 1;
    const dim3 grid((unsigned)(nprob * nblk)), block(MBX_STREAM_THREADS);
    hipLaunchKernelGGL(k1, grid, block, shm1, s, (const T*)qkv, (const T*)o, (const T*)d_o, lse, (T*)dqkv, Tn, J, H, scale, mode, nblk, dr,
                       (bf16_t*)dq_lo, st_bias, st_rsum, st_part);
    MBX_LAUNCH_CHECK("attn_bwd_dq_stream");
    hipLaunchKernelGGL(k2, grid, block, shm2, s, (const T*)qkv, (const T*)o, (const T*)d_o, lse, (T*)dqkv, Tn, J, H, scale, mode, nblk, dr,
                       (bf16_t*)dq_lo, st_bias, st_rsum, st_part);
    MBX_LAUNCH_CHECK("attn_bwd_dkv_stream");
    return 0;
}

int mbx_launch_attn_bwd_stream(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, int B, int T, int J, int H,
                               int hd, float scale, int mode, int dtype, hipStream_t s, const float* st_bias, const float* st_rsum,
                               float* st_part, const MbxDrop& dr, void* dq_lo) {
    int nprob, nblk;
    if (stream_grid("attn_bwd", B, T, J, H, mode, nprob, nblk)) return 1;
    auto launch = [&](auto tag, auto stats) {
        return launch_bwd_stream<typename decltype(tag)::type, tag.HD, tag.DROP, stats.value>(qkv, o, d_o, lse, dqkv, T, J, H, scale, mode, nprob, nblk, s,
                                                                                             dr, dq_lo, st_bias, st_rsum, st_part);
    };
    if (st_part) return dispatch_attn_hd<bf16_t, false>(hd, [&](auto tag) { return launch(tag, std::true_type{}); });   // bf16, no dropout (attn_bwd_impl)
    return dispatch_attn(dtype, hd, dr.thresh != 0, [&](auto tag) { return launch(tag, std::false_type{}); });
}
