// Device helpers shared by the attention kernels: the resident ones (attention.hip, L <= 256) and the streamed ones
// (attention_stream.hip, L > 256).  Layouts and conventions are described at the top of attention.hip.
#pragma once
#include "mbx_common.h"

// ------------------------------------------------------------------------------------------------
// per-type helpers
// ------------------------------------------------------------------------------------------------
template <typename T> struct AT;
template <> struct AT<bf16_t> { static constexpr int EPC = 8, RB = 8, SZ = 2; };
template <> struct AT<float>  { static constexpr int EPC = 4, RB = 4, SZ = 4; };

// B operand of the "rows" products: the d-vector of ONE sequence element, held by the two lanes
// (g = 0, 1) that own it.   bf16: v[s] = 8 bf16 at d = 16 s + 8 g;   fp32: v[c] = 2 floats at d = 4 c + 2 g
template <typename T, int HD> struct BReg;
template <int HD> struct BReg<bf16_t, HD> {
    uint4 v[HD / 16];
    __device__ __forceinline__ void load(const bf16_t* row, int g, bool valid) {
#pragma unroll
        for (int s = 0; s < HD / 16; ++s)
            v[s] = valid ? *reinterpret_cast<const uint4*>(row + 16 * s + 8 * g) : make_uint4(0u, 0u, 0u, 0u);
    }
    // sum_d a[d]*b[d] over this lane's half of the d range
    static __device__ __forceinline__ float dot(const BReg& a, const BReg& b) {
        float acc = 0.f;
        const uint32_t* x = reinterpret_cast<const uint32_t*>(a.v);
        const uint32_t* y = reinterpret_cast<const uint32_t*>(b.v);
#pragma unroll
        for (int i = 0; i < HD / 4; ++i) {
            acc = fmaf(__uint_as_float(x[i] << 16), __uint_as_float(y[i] << 16), acc);
            acc = fmaf(__uint_as_float(x[i] & 0xffff0000u), __uint_as_float(y[i] & 0xffff0000u), acc);
        }
        return acc;
    }
};
template <int HD> struct BReg<float, HD> {
    float2 v[HD / 4];
    __device__ __forceinline__ void load(const float* row, int g, bool valid) {
#pragma unroll
        for (int c = 0; c < HD / 4; ++c)
            v[c] = valid ? *reinterpret_cast<const float2*>(row + 4 * c + 2 * g) : make_float2(0.f, 0.f);
    }
    static __device__ __forceinline__ float dot(const BReg& a, const BReg& b) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < HD / 4; ++c) acc = fmaf(a.v[c].x, b.v[c].x, fmaf(a.v[c].y, b.v[c].y, acc));
        return acc;
    }
};

// acc[i][lane] += sum_d tile[row0 + i][d] * B[lane][d]     (tile row-major in LDS, `stride` bytes per row)
template <typename T, int HD> struct MmaRows;
template <int HD> struct MmaRows<bf16_t, HD> {
    static __device__ __forceinline__ void run(const char* tile, int stride, int row0, const BReg<bf16_t, HD>& b, int lane,
                                               f32x16_t& acc) {
        const char* p = tile + (size_t)(row0 + (lane & 31)) * stride + (lane >> 5) * 16;
#pragma unroll
        for (int s = 0; s < HD / 16; ++s) {
            const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(p + s * 32);
            const bf16x8_t bb = *reinterpret_cast<const bf16x8_t*>(&b.v[s]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bb, acc, 0, 0, 0);
        }
    }
};
template <int HD> struct MmaRows<float, HD> {
    static __device__ __forceinline__ void run(const char* tile, int stride, int row0, const BReg<float, HD>& b, int lane,
                                               f32x16_t& acc) {
        const char* p = tile + (size_t)(row0 + (lane & 31)) * stride + (lane >> 5) * 8;
#pragma unroll
        for (int c = 0; c < HD / 4; ++c) {
            const float2 a = *reinterpret_cast<const float2*>(p + c * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.v[c].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.v[c].y, acc, 0, 0, 0);
        }
    }
};

// acc[i][lane] += sum_{e in fragment f} X[e][d0 + i] * P[e][lane]
// P is a 32x32 accumulator fragment (16 registers): register r of lane (., g) belongs to sequence
// element  e(f, r, g) = 32 f + (r & 3) + 8 (r >> 2) + 4 g.
//   bf16: `tile` is the TRANSPOSED tile [d][e] (e contiguous): two 8-byte reads give the 8 elements of a k-step
//   fp32: `tile` is the ROW-MAJOR tile [e][d]: scalar reads, consecutive lanes -> consecutive d
template <typename T> struct MmaCols;
typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s_t lds_v4s_t;
template <> struct MmaCols<bf16_t> {
    static __device__ __forceinline__ void run(const char* tile, int stride, int d0, int f, const f32x16_t& p, int lane,
                                               f32x16_t& acc) {
        const int g = lane >> 5, r16 = lane & 15;
        // this lane's address: row base + (r16 >> 2), d-column block d0 + 16*((lane>>4)&1) + 4*(r16&3)
        const char* a0 = tile + (size_t)(32 * f + 4 * g + (r16 >> 2)) * stride + (d0 + 16 * ((lane >> 4) & 1) + 4 * (r16 & 3)) * 2;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            union { uint32_t u[4]; bf16x8_t v; } pb;
            union { v4s_t h[2]; bf16x8_t v; } a;
#pragma unroll
            for (int e = 0; e < 4; ++e) pb.u[e] = pack_bf2(p[8 * t + 2 * e], p[8 * t + 2 * e + 1]);
            a.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(a0 + (size_t)(16 * t) * stride));       // rows base .. base+3
            a.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(a0 + (size_t)(16 * t + 8) * stride));   // rows base+8 .. base+11
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, pb.v, acc, 0, 0, 0);
        }
    }
};
template <> struct MmaCols<float> {
    static __device__ __forceinline__ void run(const char* tile, int stride, int d0, int f, const f32x16_t& p, int lane,
                                               f32x16_t& acc) {
        const int g = lane >> 5;
        const char* col = tile + (size_t)(d0 + (lane & 31)) * 4;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int e = 32 * f + (r & 3) + 8 * (r >> 2) + 4 * g;
            const float a = *reinterpret_cast<const float*>(col + (size_t)e * stride);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[r], acc, 0, 0, 0);
        }
    }
};

// ---- LDS tile fills (cooperative over `gsize` threads, this thread = gtid) -------------------------
// Two row-major tiles at once: dstX[row][0..HD) = srcX[row * rstrideX + 0..HD) for row < L, zero for
// L <= row < KP.  All global loads of both tiles are issued before the first LDS store (the rows are
// kilobytes apart, so each load is a separate HBM/L2 round trip: they must overlap, not serialize).
// NPT = chunks per thread and tile: CH covers KP <= gsize; callers with KP <= gsize / 2 (32 rows per 64 lanes, <= 256 rows per 512
// threads) pass CH / 2 and keep half of the staging registers
template <typename T, int HD, int NPT = HD / AT<T>::EPC>
__device__ __forceinline__ void fill_two(char* dst0, const T* src0, size_t rs0, char* dst1, const T* src1, size_t rs1, int stride,
                                         int L, int KP, int gtid, int gsize, uint4 (&v0)[NPT], uint4 (&v1)[NPT]) {
    constexpr int CH = HD / AT<T>::EPC;   // 16-byte chunks per row
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int idx = gtid + i * gsize, row = idx / CH, ch = idx % CH;
        v0[i] = make_uint4(0u, 0u, 0u, 0u);
        v1[i] = make_uint4(0u, 0u, 0u, 0u);
        if (row < L) {
            v0[i] = *reinterpret_cast<const uint4*>(src0 + (size_t)row * rs0 + ch * AT<T>::EPC);
            v1[i] = *reinterpret_cast<const uint4*>(src1 + (size_t)row * rs1 + ch * AT<T>::EPC);
        }
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int idx = gtid + i * gsize, row = idx / CH, ch = idx % CH;
        if (row < KP) {
            *reinterpret_cast<uint4*>(dst0 + (size_t)row * stride + ch * 16) = v0[i];
            *reinterpret_cast<uint4*>(dst1 + (size_t)row * stride + ch * 16) = v1[i];
        }
    }
}
template <typename T, int HD, int NPT = HD / AT<T>::EPC>
__device__ __forceinline__ void fill_two(char* dst0, const T* src0, size_t rs0, char* dst1, const T* src1, size_t rs1, int stride,
                                         int L, int KP, int gtid, int gsize) {
    uint4 v0[NPT], v1[NPT];
    fill_two<T, HD, NPT>(dst0, src0, rs0, dst1, src1, rs1, stride, L, KP, gtid, gsize, v0, v1);
}
// store an accumulator pair/quad set: lane owns sequence element `row`, registers own d
template <typename T, int HD>
__device__ __forceinline__ void store_rowfrag(T* row, const f32x16_t (&acc)[HD / 32], float mul, int g) {
#pragma unroll
    for (int df = 0; df < HD / 32; ++df)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v[4] = {acc[df][4 * q] * mul, acc[df][4 * q + 1] * mul, acc[df][4 * q + 2] * mul, acc[df][4 * q + 3] * mul};
            store4<T>(row + df * 32 + 8 * q + 4 * g, v);
        }
}

// the same as the two bf16 planes of the bf16x3 operand split (fp32-class mode: dq / dk / dv are only read by split-operand GEMMs)
template <int HD>
__device__ __forceinline__ void store_rowfrag_planes(bf16_t* hi, bf16_t* lo, const f32x16_t (&acc)[HD / 32], int g) {
#pragma unroll
    for (int df = 0; df < HD / 32; ++df)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v[4] = {acc[df][4 * q], acc[df][4 * q + 1], acc[df][4 * q + 2], acc[df][4 * q + 3]};
            store4_planes(hi + df * 32 + 8 * q + 4 * g, lo + df * 32 + 8 * q + 4 * g, v);
        }
}

struct Prob {
    size_t tok0;
    size_t dbase;     // flat index of this problem's probability element (0, 0) in the reference's attn tensor (dropout masks)
    int tstep, L, h;
};
__device__ __forceinline__ Prob decode_prob(int prob, int mode, int Tn, int J, int H) {
    Prob p;
    p.h = prob % H;
    const int rest = prob / H;
    if (mode == MBX_ATTN_SPATIAL) {
        p.tok0 = (size_t)rest * J; p.tstep = 1; p.L = J;
        p.dbase = ((size_t)rest * H + p.h) * J * J;                       // attn [B T, H, J, J]       (DSTformer.py:180)
    } else {
        const int j = rest % J, b = rest / J;
        p.tok0 = (size_t)b * Tn * J + j; p.tstep = J; p.L = Tn;
        p.dbase = (((size_t)b * H + p.h) * J + j) * Tn * Tn;              // attn [B, H, J, T, T]      (DSTformer.py:194)
    }
    return p;
}
// Dropout on the attention probabilities (nn.Dropout(attn_drop), DSTformer.py:96,182,196): multiplier keep / (1 - p) of element
// (query qi, key ki) -- the counter-based mask of dropmask.py over the flat index of the reference's attn tensor.  The softmax
// statistics (row max, row sum, lse) are those of the UNdropped probabilities; in backward dP = mask (dO V^T) and
// delta = rowsum(dO O) as without dropout (O already carries the mask).
__device__ __forceinline__ float drop_mul(const MbxDrop& dr, size_t dbase, int qi, int ki, int L) {
    const size_t idx = dbase + (size_t)qi * L + ki;
    return drop_keep(dr.seed_lo, dr.seed_hi, (uint32_t)idx, (uint32_t)(idx >> 32), dr.thresh) ? dr.scale : 0.f;
}

template <typename T> __host__ __device__ constexpr int rm_stride(int HD) { return HD * AT<T>::SZ + 16; }   // row-major tile

// ------------------------------------------------------------------------------------------------
// Row dots for the folded LayerNorm backward (round 3; "LayerNorm folding" in elementwise.hip).  With `st_part` the bf16 backward
// kernels also leave, per (token, head), part[2 h + role][m] = { sum d rsum, sum d (y - b') } with role 0 = the head's q columns
// (d = dq, y = q) and role 1 = its k and v columns, d = the bf16-ROUNDED gradient being stored.  They are taken where the
// gradient rows are staged for the copy-out: the lane that writes a row fragment of dq / dk / dv into the LDS tile of q / k / v
// first reads the original values it is about to overwrite (same row, same columns, 8 bytes at a time) -- no extra pass, no
// global re-read (a first version re-read q, k, v in the copy-out loop: +21 % / +28 % on the two kernels), and as packed-bf16
// dot products (v_dot2c_f32_bf16: six VALU operations per four columns; the unpack / fma form cost +12 % / +26 %).  rsum / -b' of
// the head's 3 hd columns sit in LDS as bf16 pairs (`vec`); every lane of a half-wave reads the same address (broadcast).
// ------------------------------------------------------------------------------------------------
// All LDS reads of a 32-column half (originals and vectors) are issued before its first write: interleaved, every iteration
// waits a full LDS round trip on its own reads (the writes may alias as far as the compiler can tell) -- measured +14 % on the
// one-wave kernel.  One half at a time keeps the sixteen-wave kernel inside its 128 VGPRs.
template <int HD>
__device__ __forceinline__ void store_rowfrag_dot(bf16_t* __restrict__ row, const f32x16_t (&acc)[HD / 32], int g,
                                                  const uint4* __restrict__ vec, float& p1, float& p2) {
#pragma unroll
    for (int df = 0; df < HD / 32; ++df) {
        uint2 o[4];      // the original q / k / v values about to be overwritten
        uint4 vv[4];     // {rsum pair, rsum pair, -b' pair, -b' pair} of the same 4 columns
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d0 = df * 32 + 8 * q + 4 * g;
            o[q] = *reinterpret_cast<const uint2*>(row + d0);
            vv[q] = vec[d0 >> 2];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d0 = df * 32 + 8 * q + 4 * g;
            const uint32_t lo = pack_bf2(acc[df][4 * q], acc[df][4 * q + 1]), hi = pack_bf2(acc[df][4 * q + 2], acc[df][4 * q + 3]);
            p1 = dot2_bf16(lo, vv[q].x, dot2_bf16(hi, vv[q].y, p1));
            p2 = dot2_bf16(lo, o[q].x, dot2_bf16(hi, o[q].y, dot2_bf16(lo, vv[q].z, dot2_bf16(hi, vv[q].w, p2))));
            *reinterpret_cast<uint2*>(row + d0) = make_uint2(lo, hi);
        }
    }
}
// vec[j * HD / 4 + d / 4] = bf16 pairs {rsum[d], rsum[d+1]}, {rsum[d+2], rsum[d+3]}, {-b'[d], -b'[d+1]}, {-b'[d+2], -b'[d+3]} of the
// head's columns in tensor j = q, k, v (global column j C + h HD + d).  Rounding the two vectors to bf16 moves c1 / c2 by
// ~1e-3 / sqrt(C) of a gradient element (independent errors over the 3 hd columns): far below the bf16 noise of the data.
template <int HD>
__device__ __forceinline__ void fill_stat_vec(uint4* vec, const float* __restrict__ rsum, const float* __restrict__ bias, int C, int h,
                                              int gtid, int gsize) {
    for (int idx = gtid; idx < 3 * HD / 4; idx += gsize) {
        const int j = idx / (HD / 4), d = (idx % (HD / 4)) * 4;
        const float4 r = *reinterpret_cast<const float4*>(rsum + j * C + h * HD + d);
        const float4 b = *reinterpret_cast<const float4*>(bias + j * C + h * HD + d);
        vec[idx] = make_uint4(pack_bf2(r.x, r.y), pack_bf2(r.z, r.w), pack_bf2(-b.x, -b.y), pack_bf2(-b.z, -b.w));
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
template <typename K>
static int set_lds(K kernel, size_t bytes, const char* who) {
    if (bytes > 160 * 1024) return mbx_set_error("%s: needs %zu bytes of LDS (> 160 KiB)", who, bytes);
    return bytes > 64 * 1024 ? mbx_set_dyn_lds(reinterpret_cast<const void*>(kernel), bytes, who) : 0;
}

// runtime (dtype, head dim, dropout) -> compile-time, as dispatch_epi does for epilogues: f(AttnTag<T, HD, DROP>{}) and its return value.
// The arguments were checked by the caller (check_attn_args).  A launcher whose kernel exists for fewer combinations fixes the other axes
// itself and calls the narrower helper, so every instantiation is named where it is launched.
template <typename T, int HD_, bool DROP_> struct AttnTag { typedef T type; static constexpr int HD = HD_; static constexpr bool DROP = DROP_; };
template <typename T, bool DROP, class F> static inline int dispatch_attn_hd(int hd, F&& f) {
    return hd == 64 ? f(AttnTag<T, 64, DROP>{}) : f(AttnTag<T, 32, DROP>{});
}
template <bool DROP, class F> static inline int dispatch_attn_type(int dtype, int hd, F&& f) {
    return dtype == MBX_BF16 ? dispatch_attn_hd<bf16_t, DROP>(hd, f) : dispatch_attn_hd<float, DROP>(hd, f);
}
template <class F> static inline int dispatch_attn(int dtype, int hd, bool drop, F&& f) {
    return drop ? dispatch_attn_type<true>(dtype, hd, f) : dispatch_attn_type<false>(dtype, hd, f);
}

// the streamed kernels for sequences longer than 256 (attention_stream.hip); arguments are checked by the callers in attention.hip
int mbx_launch_attn_fwd_stream(const void* qkv, void* o, float* lse, int B, int T, int J, int H, int hd, float scale, int mode, int dtype,
                               hipStream_t s, const MbxDrop& dr);
int mbx_launch_attn_bwd_stream(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, int B, int T, int J, int H,
                               int hd, float scale, int mode, int dtype, hipStream_t s, const float* st_bias, const float* st_rsum,
                               float* st_part, const MbxDrop& dr, void* dq_lo);
