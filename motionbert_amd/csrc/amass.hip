// AMASS on the device: the 17 regressed joints of SMPL-H + DMPL (human_body_prior's BodyModel(num_betas=16, num_dmpls=8), linear blend
// skinning as smplx.lbs.lbs evaluates it) without the vertices (include/mbx.h: mbx_amass_joints).
// Only Q x is wanted, so the vertex sum is folded into the model once on the host (motionbert_amd/amass.py):
//   kp_j = sum_k ( G_k (P[j,k] . feat) + (Gt_k - G_k J_k) s[j,k] ) + qs[j] trans,   feat = [1, betas(16), dmpls(8), R_1 - I .. R_51 - I]
// over the pairs (j,k) whose folded weight is not zero.  One launch; a workgroup of eight waves owns MBX_AMASS_TILE = 16 frames:
//   1. Rodrigues of the 52 axis-angle vectors (smplx's form, angle = |r + 1e-8|) and feat into LDS, feat as [k / 4][frame][k % 4]: a
//      lane's four consecutive k of one frame are one 16-byte LDS read;
//   2. J = Jt + Jd c into LDS, then the kinematic chain (three threads per frame, one per matrix row) leaves A_k = [G_k | Gt_k - G_k J_k]
//      in LDS;
//   3. the product: a wave takes blocks of 16 pairs = 48 rows of P; per block 30 x 12 + 3 v_mfma_f32_16x16x4_f32 (the exact-fp32 MFMA:
//      the result is a k-ordered fmaf chain) with the frames as the 16 columns, P read from global memory (L2-resident: every
//      workgroup reads all of it) 16 bytes per lane, no LDS staging; the 48 x 16 results go to the wave's LDS scratch;
//   4. lanes (frame, component) walk the block's pairs in pair order, apply A_k and sum the pairs of one joint; a run's sum is a slot
//      of an LDS table, and after the last block one thread per (joint, component, frame) adds its joint's slots in block order.
// fp32, no atomics, fixed summation order; nothing a frame computes depends on another frame or on its position in the tile, so a
// launch over [0, F) equals the launches over its single frames bit for bit.  The plain-FMA form of the product (flags bit 1) is kept
// for the A/B of tools/amass_bench.py (which one is the default and why).
#include "mbx_common.h"
#include "smpl_math.h"

#define AM_J 52
#define AM_C 24            // 16 betas + 8 dmpls
#define AM_FEAT 484        // 1 + 24 + 51 * 9
#define AM_KG 121          // AM_FEAT / 4
#define AM_T MBX_AMASS_TILE
#define AM_MAXP (17 * 52)
#define AM_AS 625          // LDS frame stride of A (52 * 12 + 1: the chain's 16 threads hit 16 banks)
#define AM_JS 157          // ... of J and Gt (52 * 3 + 1)
#define AM_YS 17           // row stride of the product scratch
#define AM_SLOTS 88        // (block, joint) runs: slot = block + joint < 56 + 32
#define AM_BP 16           // pairs per block
#define AM_W 8             // waves per workgroup: two per SIMD keep the P loads of one wave under the MFMAs of the other
#define AM_NT (64 * AM_W)

static_assert(AM_T == 16, "the 16x16x4 MFMA carries the tile's frames as its 16 columns");

struct AmassTree { int p[AM_J]; };

// LDS carve, in floats
#define AM_OFF_FEAT 0
#define AM_OFF_A (AM_OFF_FEAT + AM_KG * AM_T * 4)
#define AM_OFF_J (AM_OFF_A + AM_T * AM_AS)
#define AM_OFF_GT (AM_OFF_J + AM_T * AM_JS)
#define AM_OFF_R0 (AM_OFF_GT + AM_T * AM_JS)
#define AM_OFF_Y (AM_OFF_R0 + AM_T * 9 + 4)
#define AM_OFF_PART (AM_OFF_Y + AM_W * 48 * AM_YS)
#define AM_OFF_JR (AM_OFF_PART + AM_SLOTS * 48)
#define AM_LDS_FLOATS (AM_OFF_JR + 64)
static_assert(AM_OFF_A % 4 == 0 && AM_LDS_FLOATS * 4 <= 160 * 1024, "LDS carve");

__device__ __forceinline__ int am_feat_at(int k, int f) { return ((k >> 2) * AM_T + f) * 4 + (k & 3); }

template <bool MFMA>
__global__ __launch_bounds__(AM_NT) void amass_joints_kernel(const float* __restrict__ poses, const float* __restrict__ betas, int betas_stride,
                                                           const float* __restrict__ dmpls, const float* __restrict__ trans,
                                                           const float* __restrict__ Jt, const float* __restrict__ Jd, AmassTree tree,
                                                           const int* __restrict__ pairs, const float* __restrict__ P,
                                                           const float* __restrict__ sw, const float* __restrict__ qs, int Np, int K,
                                                           int camera, float* __restrict__ kp, int F) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* feat = lds + AM_OFF_FEAT;
    float* A = lds + AM_OFF_A;
    float* Jl = lds + AM_OFF_J;
    float* Gt = lds + AM_OFF_GT;
    float* R0 = lds + AM_OFF_R0;
    float* part = lds + AM_OFF_PART;
    int* jr = reinterpret_cast<int*>(lds + AM_OFF_JR);          // [0,32) first pair of a joint, [32,64) one past its last
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * AM_T;

    // ---- 1. rotations and feat
    for (int i = tid; i < AM_T * AM_J; i += AM_NT) {
        const int f = i & (AM_T - 1), k = i >> 4;
        const int fr = f0 + f;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        if (fr < F) {
            const float* ps = poses + (size_t)fr * 156 + k * 3;
            r0 = ps[0]; r1 = ps[1]; r2 = ps[2];
        }
        float R[9];
        smplx_rodrigues(r0, r1, r2, R);
        if (k == 0) {
#pragma unroll
            for (int e = 0; e < 9; ++e) R0[f * 9 + e] = R[e];
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e) feat[am_feat_at(25 + (k - 1) * 9 + e, f)] = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f);
        }
    }
    for (int i = tid; i < AM_T * 25; i += AM_NT) {
        const int f = i & (AM_T - 1), k = i >> 4;
        const int fr = f0 + f;
        float v = 0.f;
        if (k == 0) v = 1.0f;
        else if (fr < F) {
            if (k <= 16) v = betas[(size_t)fr * betas_stride + (k - 1)];
            else if (dmpls) v = dmpls[(size_t)fr * 8 + (k - 17)];
        }
        feat[am_feat_at(k, f)] = v;
    }
    if (tid < 64) jr[tid] = tid < 32 ? Np : 0;
    for (int i = tid; i < AM_SLOTS * 48; i += AM_NT) part[i] = 0.f;
    __syncthreads();
    for (int p = tid; p < Np; p += AM_NT) {
        const int j = min(max(pairs[2 * p], 0), K - 1);
        if (p == 0 || min(max(pairs[2 * p - 2], 0), K - 1) != j) jr[j] = p;
        if (p == Np - 1 || min(max(pairs[2 * p + 2], 0), K - 1) != j) jr[32 + j] = p + 1;
    }

    // ---- 2. J = Jt + Jd c, then the chain
    for (int i = tid; i < AM_T * AM_J * 3; i += AM_NT) {
        const int f = i & (AM_T - 1), e = i >> 4;
        float v = Jt[e];
        const float* jd = Jd + e * AM_C;
#pragma unroll
        for (int m = 0; m < AM_C; ++m) v = fmaf(jd[m], feat[am_feat_at(1 + m, f)], v);
        Jl[f * AM_JS + e] = v;
    }
    __syncthreads();
    if (tid < 3 * AM_T) {
        // thread (frame f, row r): row r of G_k = G_p R_k and of Gt_k depends on row r of the parent alone, so the three rows of a
        // frame's chain run side by side without a barrier
        const int f = tid & (AM_T - 1), r = tid >> 4;
        float* Af = A + f * AM_AS + r * 4;
        const float* Jf = Jl + f * AM_JS;
        float* Gf = Gt + f * AM_JS + r;
        for (int k = 0; k < AM_J; ++k) {
            float g[3], t;
            const float j0 = Jf[k * 3], j1 = Jf[k * 3 + 1], j2 = Jf[k * 3 + 2];
            if (k == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = R0[f * 9 + r * 3 + c];
                t = Jf[r];
            } else {
                const int p = tree.p[k];
                float R[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) R[e] = feat[am_feat_at(25 + (k - 1) * 9 + e, f)] + ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f);
                const float g0 = Af[p * 12], g1 = Af[p * 12 + 1], g2 = Af[p * 12 + 2];
                const float d0 = j0 - Jf[p * 3], d1 = j1 - Jf[p * 3 + 1], d2 = j2 - Jf[p * 3 + 2];
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = g0 * R[c] + g1 * R[3 + c] + g2 * R[6 + c];
                t = g0 * d0 + g1 * d1 + g2 * d2 + Gf[p * 3];
            }
            Gf[k * 3] = t;
            Af[k * 12] = g[0]; Af[k * 12 + 1] = g[1]; Af[k * 12 + 2] = g[2];
            Af[k * 12 + 3] = t - (g[0] * j0 + g[1] * j1 + g[2] * j2);
        }
    }
    __syncthreads();

    // ---- 3. + 4. the product, block by block, and the per-pair transforms
    const int nblk = (Np + AM_BP - 1) / AM_BP, nrows = 3 * Np;
    const int iters = (nblk + AM_W - 1) / AM_W;
    float* ys = lds + AM_OFF_Y + wave * 48 * AM_YS;
    const int c16 = lane & 15, q = lane >> 4;
    const float4* feat4 = reinterpret_cast<const float4*>(feat);
    for (int it = 0; it < iters; ++it) {
        const int blk = it * AM_W + wave;
        const bool live = blk < nblk;               // wave-uniform
        if (live) {
            if constexpr (MFMA) {
                // A operand: lane (row c16, q) holds P[row][16 kc + 4 q + e] for the e-th MFMA of chunk kc; B: feat[the same k][frame c16]
                const float* pr[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) pr[m] = P + (size_t)min(blk * 48 + m * 16 + c16, nrows - 1) * AM_FEAT + q * 4;
                f32x4_t acc[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
                for (int kc = 0; kc < 30; ++kc) {
                    const float4 b = feat4[(kc * 4 + q) * AM_T + c16];
                    float4 a[3];
#pragma unroll
                    for (int m = 0; m < 3; ++m) a[m] = *reinterpret_cast<const float4*>(pr[m] + kc * 16);
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].x, b.x, acc[m], 0, 0, 0);
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].y, b.y, acc[m], 0, 0, 0);
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].z, b.z, acc[m], 0, 0, 0);
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].w, b.w, acc[m], 0, 0, 0);
                }
                {   // k = 480 + q: the last four columns in the MFMA's own k order
                    const float b = feat[(120 * AM_T + c16) * 4 + q];
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[m][480 - q * 4 + q], b, acc[m], 0, 0, 0);
                }
                // D: column = lane & 15 = frame, row = 4 (lane >> 4) + register
#pragma unroll
                for (int m = 0; m < 3; ++m)
#pragma unroll
                    for (int e = 0; e < 4; ++e) ys[(m * 16 + q * 4 + e) * AM_YS + c16] = acc[m][e];
            } else {
                // lane (frame c16, q): rows 12 q .. 12 q + 11 of the block, k in order
                float acc[12];
                const float* pr[12];
#pragma unroll
                for (int r = 0; r < 12; ++r) { acc[r] = 0.f; pr[r] = P + (size_t)min(blk * 48 + q * 12 + r, nrows - 1) * AM_FEAT; }
                for (int kg = 0; kg < AM_KG; ++kg) {
                    const float4 b = feat4[kg * AM_T + c16];
#pragma unroll
                    for (int r = 0; r < 12; ++r) {
                        const float4 a = *reinterpret_cast<const float4*>(pr[r] + kg * 4);
                        acc[r] = fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc[r]))));
                    }
                }
#pragma unroll
                for (int r = 0; r < 12; ++r) ys[(q * 12 + r) * AM_YS + c16] = acc[r];
            }
        }
        __syncthreads();
        if (live && lane < 48) {
            const int f = lane & 15, c = lane >> 4;
            const float* Af = A + f * AM_AS + c * 4;
            const int p0 = blk * AM_BP, p1 = min(p0 + AM_BP, Np);
            float acc = 0.f;
            int jcur = min(max(pairs[2 * p0], 0), K - 1);
            for (int p = p0; p < p1; ++p) {
                const int j = min(max(pairs[2 * p], 0), K - 1), k = min(max(pairs[2 * p + 1], 0), AM_J - 1);
                if (j != jcur) {
                    part[(blk + jcur) * 48 + lane] = acc;
                    acc = 0.f;
                    jcur = j;
                }
                const float* y = ys + (p - p0) * 3 * AM_YS + f;
                const float* a = Af + k * 12;
                acc += a[0] * y[0] + a[1] * y[AM_YS] + a[2] * y[2 * AM_YS] + a[3] * sw[p];
            }
            part[(blk + jcur) * 48 + lane] = acc;
        }
        __syncthreads();
    }

    // ---- the joints: a joint's slots in block order, then qs[j] trans; the camera step of convert_amass.py where asked for
    for (int i = tid; i < K * 48; i += AM_NT) {
        const int f = i & 15, oc = (i >> 4) % 3, j = i / 48;
        const int fr = f0 + f;
        if (fr >= F) continue;
        const int c = camera ? (oc == 0 ? 0 : 3 - oc) : oc;          // (x, y, z) -> (x, -z, y)
        float v = 0.f;
        const int pa = jr[j], pb = jr[32 + j];
        if (pa < pb)
            for (int blk = pa / AM_BP; blk <= (pb - 1) / AM_BP; ++blk) v += part[(blk + j) * 48 + c * 16 + f];
        if (trans) v = fmaf(qs[j], trans[(size_t)fr * 3 + c], v);
        if (camera) v = (oc == 1 ? -v : v) * 0.298f;
        kp[((size_t)fr * K + j) * 3 + oc] = v;
    }
}

extern "C" int mbx_amass_joints(const float* poses, const float* betas, int betas_per_frame, const float* dmpls, const float* trans,
                                const float* Jt, const float* Jd, const int* parents, const int* pairs, const float* P, const float* s,
                                const float* qs, int Np, int K, int flags, float* kp, int F, void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= (1 << 26), "amass_joints: bad frame count F=%d", F);
    MBX_CHECK_ARG(K >= 1 && K <= 32, "amass_joints: K=%d regressed joints (1 <= K <= 32)", K);
    MBX_CHECK_ARG(Np >= 0 && Np <= AM_MAXP, "amass_joints: Np=%d pairs (0 <= Np <= 17 * 52 = %d)", Np, AM_MAXP);
    MBX_CHECK_ARG((flags & ~3) == 0, "amass_joints: unknown flag bits %d", flags);
    MBX_CHECK_ARG(Jt && Jd && parents && qs && (Np == 0 || (pairs && P && s)), "amass_joints: null model array");
    AmassTree tree;
    MBX_CHECK_ARG(parents[0] == -1, "amass_joints: parents[0] must be -1, got %d", parents[0]);
    tree.p[0] = -1;
    for (int j = 1; j < AM_J; ++j) {
        MBX_CHECK_ARG(parents[j] >= 0 && parents[j] < j, "amass_joints: parents[%d] = %d is not a forward-ordered tree (0 <= parents[j] < j)", j,
                      parents[j]);
        tree.p[j] = parents[j];
    }
    if (F == 0) return 0;
    MBX_CHECK_ARG(poses && betas && kp, "amass_joints: null pointer (poses, betas, kp)");
    MBX_CHECK_ARG((((uintptr_t)poses | (uintptr_t)betas | (uintptr_t)dmpls | (uintptr_t)trans | (uintptr_t)Jt | (uintptr_t)Jd | (uintptr_t)pairs |
                    (uintptr_t)s | (uintptr_t)qs | (uintptr_t)kp) & 3) == 0 && ((uintptr_t)P & 15) == 0,
                  "amass_joints: pointers must be 4-byte aligned, P 16-byte aligned");
    const size_t bytes = (size_t)AM_LDS_FLOATS * sizeof(float);
    const int grid = (F + AM_T - 1) / AM_T;
    const int stride = betas_per_frame ? 16 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (flags & 2) {
        if (mbx_set_dyn_lds((const void*)amass_joints_kernel<false>, bytes, "amass_joints")) return 1;
        hipLaunchKernelGGL(amass_joints_kernel<false>, dim3(grid), dim3(AM_NT), bytes, st, poses, betas, stride, dmpls, trans, Jt, Jd, tree, pairs, P,
                           s, qs, Np, K, flags & 1, kp, F);
    } else {
        if (mbx_set_dyn_lds((const void*)amass_joints_kernel<true>, bytes, "amass_joints")) return 1;
        hipLaunchKernelGGL(amass_joints_kernel<true>, dim3(grid), dim3(AM_NT), bytes, st, poses, betas, stride, dmpls, trans, Jt, Jd, tree, pairs, P,
                           s, qs, Np, K, flags & 1, kp, F);
    }
    MBX_LAUNCH_CHECK("amass_joints");
    return 0;
}
