// The SMPL body model on the device: linear blend skinning as smplx.lbs.lbs evaluates it, forward and hand-written backward (include/mbx.h).
//   mbx_smpl_pack     : the transposed model table PT [3V,224] = [posedirs^T | shapedirs | 0] the backward reads with one lane per column.
// The three forward entries are one path, prepare (if any) -> chain -> vertices -> finish, through the same kernels: the chain kernel (one
// thread per parameter set: joints, the 24 transforms A_j [F,24,12], pf [F,207]), the vertex kernel smpl_verts_kernel<NP, STITCH> (64
// vertices x 8 parameter sets per wave, lane = vertex; pose blend, skinning, the tile's share of Q x; NP = 1 or 2 sets meet in one output
// frame, STITCH: the frame's row comes from dst_frames) and the tile-order keypoint sum sm_kp_sum; hence the same bits from all three.
//   mbx_smpl_fwd      : chain -> vertices <1, false> -> keypoint finish <1, false> (tile partials added in tile order, scaled).
//   mbx_mesh_gt       : the mesh targets of MotionSMPL.__getitem__ (lib/data/dataset_mesh.py:63-97) for a batch of clips: prepare kernel (clip
//                       flip of the 2D input and of theta, Rodrigues into the workspace) -> chain -> vertices <1, false> -> centring kernel
//                       (root = scale (Q x)[0] by sm_kp_sum, subtracted from verts in place and from the finished keypoints).
//   mbx_wild_mesh     : the paired SMPL stage of in-the-wild mesh recovery (infer_wild_mesh.py:115-141) for a batch of clips: prepare kernel
//                       (flip_thetas + Rodrigues of the flipped pass, the theta mean) -> chain over both parameter sets -> vertices
//                       <2, true>, whose waves evaluate both sets of their frames and store the mean once, to the clip's rows of the
//                       stitched result (<1, true> without a second pass) -> keypoint finish of the same <NP, STITCH>.
//   mbx_smpl_bwd      : chain kernel again (nothing but betas and rotmat is saved) -> vertex backward (64 vertices x 16 frames per step;
//                       phase 1, lane = vertex: vp, T, g, dvp recomputed into LDS; phase 2, lane = output column: d pf / d beta and d A
//                       accumulated in registers over the workgroup's vertex tiles) -> split sum -> chain backward (one thread per frame).
// Nothing of size [F,V,...] but verts exists in global memory: no transform tensor, no pose offsets, no v_posed.
// fp32 FMAs on the vector unit (the fp32 MFMA of gfx950 runs at the same rate), fixed summation order, no floating-point atomics: two
// calls on the same inputs give the same bits.  Frame-uniform operands (pf, A, betas, dkp) are read through wave-uniform addresses.
#include "mbx_common.h"
#include "aug_rng.h"
#include "smpl_math.h"

#define SM_J 24
#define SM_PF 207          // 23 * 9
#define SM_PFS 208         // row stride of the pf workspace
#define SM_A 288           // 24 * 12
#define SM_PT 224          // columns of PT: 207 posedirs rows, 10 shapedirs, 7 zero
#define SM_COLS 512        // partial / sum record per frame: [0,224) the PT columns, [224,512) d A
#define SM_VT 64           // vertices per tile
#define SM_FW 8            // forward: frames per wave (32 per workgroup)
#define SM_BW 4            // backward: frames per wave (16 per workgroup)
#define SM_BF (4 * SM_BW)
#define SM_ZS 20           // LDS row stride of the phase-1 values: 16 frames + 4 pad (16-byte aligned, conflict-free b128 writes)
#define SM_SPLITS 8

struct SmplTree { int p[SM_J]; };

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smpl_pack_kernel(const float* __restrict__ shapedirs, const float* __restrict__ posedirs,
                                                        float* __restrict__ pt, int V) {
    const size_t n = (size_t)3 * V * SM_PT;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t row = i / SM_PT;
        const int col = (int)(i % SM_PT);
        float v = 0.0f;
        if (col < SM_PF) v = posedirs[(size_t)col * 3 * V + row];
        else if (col < SM_PF + 10) v = shapedirs[row * 10 + (col - SM_PF)];
        pt[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// chain.  G: per-thread scratch [288][F] (frame-minor: coalesced), first [Grot_j | Gt_j], read back by the same thread for the children.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void smpl_joint(const float* __restrict__ Jt, const float* __restrict__ Jd, const float (&b)[10], int j, float (&J)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = Jt[j * 3 + c];
#pragma unroll
        for (int k = 0; k < 10; ++k) s += Jd[(j * 3 + c) * 10 + k] * b[k];
        J[c] = s;
    }
}

__global__ __launch_bounds__(64) void smpl_chain_fwd_kernel(const float* __restrict__ betas, const float* __restrict__ rotmat,
                                                            const float* __restrict__ Jt, const float* __restrict__ Jd, SmplTree tree, float scale,
                                                            float* __restrict__ Aws, float* __restrict__ PFws, float* G, float* __restrict__ joints,
                                                            int F) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    float b[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) b[k] = betas[(size_t)f * 10 + k];
    const float* R = rotmat + (size_t)f * 216;
    for (int k = 0; k < SM_PF; ++k) PFws[(size_t)f * SM_PFS + k] = R[9 + k] - (((k % 9) % 4 == 0) ? 1.0f : 0.0f);
    PFws[(size_t)f * SM_PFS + SM_PF] = 0.0f;
#define SM_G(j, e) G[(size_t)((j) * 12 + (e)) * F + f]
    for (int j = 0; j < SM_J; ++j) {
        float J[3], r[9];
        smpl_joint(Jt, Jd, b, j, J);
#pragma unroll
        for (int e = 0; e < 9; ++e) r[e] = R[j * 9 + e];
        if (j == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int d = 0; d < 3; ++d) SM_G(0, c * 4 + d) = r[c * 3 + d];
                SM_G(0, c * 4 + 3) = J[c];
            }
        } else {
            const int p = tree.p[j];
            float Jp[3], P[12], rel[3];
            smpl_joint(Jt, Jd, b, p, Jp);
#pragma unroll
            for (int e = 0; e < 12; ++e) P[e] = SM_G(p, e);
#pragma unroll
            for (int c = 0; c < 3; ++c) rel[c] = J[c] - Jp[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int d = 0; d < 3; ++d) SM_G(j, c * 4 + d) = P[c * 4] * r[d] + P[c * 4 + 1] * r[3 + d] + P[c * 4 + 2] * r[6 + d];
                SM_G(j, c * 4 + 3) = P[c * 4] * rel[0] + P[c * 4 + 1] * rel[1] + P[c * 4 + 2] * rel[2] + P[c * 4 + 3];
            }
        }
    }
    for (int j = 0; j < SM_J; ++j) {
        float J[3], g[12];
        smpl_joint(Jt, Jd, b, j, J);
#pragma unroll
        for (int e = 0; e < 12; ++e) g[e] = SM_G(j, e);
        float* A = Aws + (size_t)f * SM_A + j * 12;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int d = 0; d < 3; ++d) A[c * 4 + d] = g[c * 4 + d];
            A[c * 4 + 3] = g[c * 4 + 3] - (g[c * 4] * J[0] + g[c * 4 + 1] * J[1] + g[c * 4 + 2] * J[2]);
            if (joints) joints[(size_t)f * 72 + j * 3 + c] = scale * g[c * 4 + 3];
        }
    }
#undef SM_G
}

// ---------------------------------------------------------------------------------------------------------------
// the per-vertex values both directions need, lane = vertex, NF frames of the wave in registers
// ---------------------------------------------------------------------------------------------------------------
template <int NF>
__device__ __forceinline__ void smpl_vposed(const float* __restrict__ vt, const float* __restrict__ sd, const float* __restrict__ pd,
                                            const float* __restrict__ betas, const float* __restrict__ PFws, const int (&fi)[NF], int v, int V,
                                            float (&vp)[NF][3]) {
    // the offsets are summed from zero and the template is added last: 217 additions into a running value of template size would
    // each round at the template's ulp, and (vp - J) is what the skinning and its gradient see
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < NF; ++i) vp[i][c] = 0.0f;
    for (int k = 0; k < 10; ++k) {
        const float s0 = sd[(size_t)v * 30 + k], s1 = sd[(size_t)v * 30 + 10 + k], s2 = sd[(size_t)v * 30 + 20 + k];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const float bv = betas[(size_t)fi[i] * 10 + k];
            vp[i][0] += s0 * bv; vp[i][1] += s1 * bv; vp[i][2] += s2 * bv;
        }
    }
    const float* col = pd + (size_t)3 * v;
#pragma unroll 3
    for (int k = 0; k < SM_PF; ++k) {
        const float* row = col + (size_t)k * 3 * V;
        const float p0 = row[0], p1 = row[1], p2 = row[2];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const float pf = PFws[(size_t)fi[i] * SM_PFS + k];
            vp[i][0] += p0 * pf; vp[i][1] += p1 * pf; vp[i][2] += p2 * pf;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = vt[(size_t)v * 3 + c];
#pragma unroll
        for (int i = 0; i < NF; ++i) vp[i][c] += t;
    }
}

// T = sum_j w_j A_j over the joints some lane of the wave has a weight on (mask); a skipped term is an exact + 0
__device__ __forceinline__ void smpl_blend(const float (&w)[SM_J], unsigned mask, const float* __restrict__ A, float (&T)[12]) {
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0f;
#pragma unroll
    for (int j = 0; j < SM_J; ++j) {
        if (mask & (1u << j)) {
#pragma unroll
            for (int e = 0; e < 12; ++e) T[e] += w[j] * A[j * 12 + e];
        }
    }
}

// the row of frame f (of clip f / T) in the stitched results, -1 where the clip's entry does not fit [0,F)
__device__ __forceinline__ int wm_row(const int* __restrict__ dst_frames, int f, int T, int F) {
    const int clip = f / T;
    const int d = dst_frames[clip];
    return (d >= 0 && d <= F - T) ? d + (f - clip * T) : -1;
}
// (scale a + scale b) * 0.5 with every product and sum rounded: what (a' + b') / 2.0 of the two passes' fp32 tensors gives
__device__ __forceinline__ float wm_pair(float scale, float a, float b) {
#pragma clang fp contract(off)
    const float pa = scale * a;
    const float pb = scale * b;
    const float s = pa + pb;
    return s * 0.5f;
}

// The vertex kernel: workgroup = 64 vertices (lane = vertex) x 4 waves, SM_FW parameter sets per wave.  nF output frames; betas / Aws /
// PFws / kpart are indexed by parameter set, NP nF of them: [0,nF) pass A, [nF,2nF) pass B.  NP = 2: a wave's SM_FW sets are SM_FW / 2
// output frames of pass A and the same frames of pass B; the two x meet in registers and one store writes their mean.  STITCH: frame f
// goes to row wm_row(f) of the F rows of verts; otherwise to row f (dst_frames, T and F are not read).  The operation order per parameter
// set is the same in every instantiation.
template <int NP, bool STITCH>
__global__ __launch_bounds__(256) void smpl_verts_kernel(const float* __restrict__ vt, const float* __restrict__ sd, const float* __restrict__ pd,
                                                         const float* __restrict__ lbsw, const float* __restrict__ Q,
                                                         const float* __restrict__ betas, const float* __restrict__ Aws,
                                                         const float* __restrict__ PFws, float scale, float* __restrict__ verts,
                                                         float* __restrict__ kpart, int nF, int V, int K,
                                                         const int* __restrict__ dst_frames, int T, int F) {
    constexpr int NO = SM_FW / NP;              // output frames per wave
    __shared__ float qs[32 * 65];
    __shared__ float xs[4][3][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v0 = blockIdx.x * SM_VT;
    const bool live = v0 + lane < V;
    const int v = live ? v0 + lane : V - 1;
    const int f0 = blockIdx.y * (4 * NO) + wave * NO;
    const int FC = NP * nF;
    if (kpart) {
        for (int idx = tid; idx < K * 64; idx += 256) {
            const int k = idx >> 6, l = idx & 63;
            qs[k * 65 + l] = (v0 + l < V) ? Q[(size_t)k * V + v0 + l] : 0.0f;
        }
    }
    float w[SM_J];
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < SM_J; ++j) {
        w[j] = lbsw[(size_t)v * SM_J + j];
        if (__ballot(w[j] != 0.0f) != 0ull) mask |= 1u << j;
    }
    int fi[SM_FW];                              // parameter set of slot i: pass (i / NO), output frame f0 + i % NO
#pragma unroll
    for (int i = 0; i < SM_FW; ++i) fi[i] = min(f0 + (i % NO), nF - 1) + (i / NO) * nF;
    float vp[SM_FW][3];
    smpl_vposed<SM_FW>(vt, sd, pd, betas, PFws, fi, v, V, vp);
    __syncthreads();
    const int nout = 3 * K;
#pragma unroll
    for (int io = 0; io < NO; ++io) {
        const bool fl = f0 + io < nF;
        float x[NP][3];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int i = p * NO + io;
            float Tm[12];
            smpl_blend(w, mask, Aws + (size_t)fi[i] * SM_A, Tm);
#pragma unroll
            for (int c = 0; c < 3; ++c) x[p][c] = Tm[c * 4] * vp[i][0] + Tm[c * 4 + 1] * vp[i][1] + Tm[c * 4 + 2] * vp[i][2] + Tm[c * 4 + 3];
        }
        if (verts && live && fl) {
            const int row = STITCH ? wm_row(dst_frames, fi[io], T, F) : fi[io];         // wave-uniform
            if (!STITCH || row >= 0) {
                float* o = verts + ((size_t)row * V + v) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = NP == 2 ? wm_pair(scale, x[0][c], x[NP - 1][c]) : scale * x[0][c];
            }
        }
        if (kpart) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                xs[wave][0][lane] = x[p][0]; xs[wave][1][lane] = x[p][1]; xs[wave][2][lane] = x[p][2];
                __syncthreads();
                for (int o = lane; o < nout; o += 64) {
                    const int k = o / 3, c = o - 3 * k;
                    float s = 0.0f;
                    for (int l = 0; l < 64; ++l) s += qs[k * 65 + l] * xs[wave][c][l];
                    if (fl) kpart[((size_t)blockIdx.x * FC + fi[p * NO + io]) * nout + o] = s;
                }
                __syncthreads();
            }
        }
    }
}

// one (frame, output) record of kpart [tiles][tile_stride]: the tiles' partials added in tile order
__device__ __forceinline__ float sm_kp_sum(const float* __restrict__ kpart, int nvt, size_t tile_stride, size_t idx) {
    float s = 0.0f;
    for (int t = 0; t < nvt; ++t) s += kpart[(size_t)t * tile_stride + idx];
    return s;
}

// keypoints, n = nF * nout of them: scale * sum per pass (NP = 2: then the mean, as the vertices form it), to row f or to the clip's rows
template <int NP, bool STITCH>
__global__ __launch_bounds__(256) void smpl_kp_finish_kernel(const float* __restrict__ kpart, int nvt, float scale, float* __restrict__ kp,
                                                             size_t n, int nout, const int* __restrict__ dst_frames, int T, int F) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    size_t dst = i;
    if (STITCH) {
        const int f = (int)(i / nout), o = (int)(i - (size_t)f * nout);
        const int row = wm_row(dst_frames, f, T, F);
        if (row < 0) return;
        dst = (size_t)row * nout + o;
    }
    const float sa = sm_kp_sum(kpart, nvt, NP * n, i);
    kp[dst] = NP == 2 ? wm_pair(scale, sa, sm_kp_sum(kpart, nvt, NP * n, n + i)) : scale * sa;
}

// ---------------------------------------------------------------------------------------------------------------
// mesh targets (mbx_mesh_gt).  Prepare: 64 threads per frame, thread = joint (24: flip_thetas + Rodrigues), 2D joint (17: flip_data + the
// confidence clip), shape coefficient (10) or the clip's flag (1).  The flag belongs to the CLIP n = f / T.
// ---------------------------------------------------------------------------------------------------------------
#define MG_CF 8            // centring: frames per workgroup
#define MG_CV 2048         // centring: vertices per workgroup

__device__ __forceinline__ int mg_theta_src(int j) {      // utils_mesh.py:475: (1,2) (4,5) (7,8) (10,11) (13,14) (16,17) (18,19) (20,21) (22,23)
    if (j == 0) return 0;
    if (j < 18) return j % 3 == 1 ? j + 1 : (j % 3 == 2 ? j - 1 : j);
    return (j & 1) ? j - 1 : j + 1;
}
__device__ __forceinline__ int mg_joint_src(int j) {      // utils_data.py:61-65: left 4 5 6 11 12 13 <-> right 1 2 3 14 15 16
    if ((j >= 1 && j <= 3) || (j >= 11 && j <= 13)) return j + 3;
    if ((j >= 4 && j <= 6) || (j >= 14 && j <= 16)) return j - 3;
    return j;
}

__global__ __launch_bounds__(256) void mesh_gt_prepare_kernel(const float* __restrict__ pose, const float* __restrict__ shape,
                                                              const float* __restrict__ m2d, const unsigned char* __restrict__ flips,
                                                              uint32_t slo, uint32_t shi, float flip_prob, float* __restrict__ x2d,
                                                              float* __restrict__ theta, float* __restrict__ rot,
                                                              unsigned char* __restrict__ flips_used, int F, int T) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = threadIdx.x & 63;
    if (f >= F) return;
    const int n = f / T;
    const bool fl = flips ? flips[n] != 0 : aug_uniform(slo, shi, 0u, (uint32_t)n) < flip_prob;
    if (t < SM_J) {
        const float* p = pose + (size_t)f * 72 + (fl ? mg_theta_src(t) : t) * 3;
        float r0 = p[0], r1 = p[1], r2 = p[2];
        if (fl) { r1 = -r1; r2 = -r2; }
        if (theta) {
            float* o = theta + (size_t)f * 82 + t * 3;
            o[0] = r0; o[1] = r1; o[2] = r2;
        }
        if (rot) smplx_rodrigues(r0, r1, r2, rot + (size_t)f * 216 + t * 9);
    } else if (t < SM_J + 17) {
        if (x2d) {
            const int j = t - SM_J;
            const float* p = m2d + ((size_t)f * 17 + (fl ? mg_joint_src(j) : j)) * 3;
            const float cf = p[2];
            float* o = x2d + ((size_t)f * 17 + j) * 3;
            o[0] = fl ? -p[0] : p[0];
            o[1] = p[1];
            o[2] = cf < 0.0f ? 0.0f : (cf > 1.0f ? 1.0f : cf);      // np.clip(c, 0, 1): NaN stays NaN
        }
    } else if (t < SM_J + 27) {
        if (theta) theta[(size_t)f * 82 + 72 + (t - SM_J - 17)] = shape[(size_t)f * 10 + (t - SM_J - 17)];
    } else if (t == SM_J + 27) {
        if (flips_used && f == n * T) flips_used[n] = fl ? 1 : 0;
    }
}

// Centring: workgroup = MG_CF frames x MG_CV vertices.  Every workgroup forms the root of its frames from the tile partials of keypoint 0
// (scale * sm_kp_sum, what smpl_kp_finish_kernel stores), so all workgroups of a frame hold the same bits; verts -= root in place.  The
// workgroups of the first vertex chunk also finish the keypoints and subtract the root from them.
__global__ __launch_bounds__(256) void mesh_gt_centre_kernel(const float* __restrict__ kpart, int nvt, int nout, float scale, float* verts,
                                                             float* __restrict__ kp, int F, int V) {
    // no contraction here: scale * s has to round before the root comes off it, as it does where smpl_kp_finish_kernel stores it (a fused
    // multiply-subtract would leave the product's rounding error in keypoint 0 instead of an exact zero)
#pragma clang fp contract(off)
    __shared__ float root[MG_CF][3];
    const int tid = threadIdx.x;
    const int f0 = blockIdx.x * MG_CF;          // frame blocks on x: F / 8 of them, up to 2^17; vertex chunks on y: at most 512
    const size_t n = (size_t)F * nout;
    if (tid < MG_CF * 3) {
        const int i = tid / 3, c = tid - 3 * i;
        const int f = min(f0 + i, F - 1);
        root[i][c] = scale * sm_kp_sum(kpart, nvt, n, (size_t)f * nout + c);
    }
    __syncthreads();
    if (kp && blockIdx.y == 0) {
        for (int idx = tid; idx < MG_CF * nout; idx += 256) {
            const int i = idx / nout, o = idx - i * nout;
            const int f = f0 + i;
            if (f < F) {
                const size_t at = (size_t)f * nout + o;
                const float s = sm_kp_sum(kpart, nvt, n, at);
                kp[at] = scale * s - root[i][o % 3];
            }
        }
    }
    if (verts) {
        const int e0 = blockIdx.y * (3 * MG_CV);
        const int e1 = min(e0 + 3 * MG_CV, 3 * V);
        for (int i = 0; i < MG_CF; ++i) {
            if (f0 + i >= F) break;
            float* row = verts + (size_t)(f0 + i) * 3 * V;
            const float r0 = root[i][0], r1 = root[i][1], r2 = root[i][2];
#pragma unroll 4
            for (int e = e0 + tid; e < e1; e += 256) {
                const int c = e % 3;
                row[e] -= c == 0 ? r0 : (c == 1 ? r1 : r2);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// in-the-wild mesh recovery (mbx_wild_mesh): the model's pass on x (A) and its flipped-back pass on flip_data(x) (B), their mean written
// once to each clip's rows of the stitched results.  The chain kernel sees 2 nT parameter sets: [0,nT) pass A, [nT,2nT) pass B.
// ---------------------------------------------------------------------------------------------------------------
// 64 threads per frame: thread = joint (24: flip_thetas + Rodrigues of pass B, the theta mean), shape coefficient (10); all 64 copy pass
// A's rotations next to pass B's.  theta_b == NULL (single-pass mode, launched for theta alone): theta_a is copied to its rows.
__global__ __launch_bounds__(256) void wild_mesh_prepare_kernel(const float* __restrict__ rotmat_a, const float* __restrict__ betas_a,
                                                                const float* __restrict__ theta_a, const float* __restrict__ theta_b,
                                                                const int* __restrict__ dst_frames, float* __restrict__ rot2,
                                                                float* __restrict__ betas2, float* __restrict__ theta, int nT, int T, int F) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = threadIdx.x & 63;
    if (f >= nT) return;
    const int row = theta ? wm_row(dst_frames, f, T, F) : -1;
    if (theta_b) {
        for (int e = t; e < 216; e += 64) rot2[(size_t)f * 216 + e] = rotmat_a[(size_t)f * 216 + e];
        if (t < 10) betas2[(size_t)f * 10 + t] = betas_a[(size_t)f * 10 + t];
    }
    if (t < SM_J) {
        if (theta_b) {
            const float* p = theta_b + (size_t)f * 82 + mg_theta_src(t) * 3;
            const float r0 = p[0], r1 = -p[1], r2 = -p[2];
            smplx_rodrigues(r0, r1, r2, rot2 + (size_t)(nT + f) * 216 + t * 9);
            if (row >= 0) {
                const float* a = theta_a + (size_t)f * 82 + t * 3;
                float* o = theta + (size_t)row * 82 + t * 3;
                o[0] = (a[0] + r0) * 0.5f; o[1] = (a[1] + r1) * 0.5f; o[2] = (a[2] + r2) * 0.5f;
            }
        } else if (row >= 0) {
            const float* a = theta_a + (size_t)f * 82 + t * 3;
            float* o = theta + (size_t)row * 82 + t * 3;
            o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
        }
    } else if (t < SM_J + 10) {
        const int k = t - SM_J;
        if (theta_b) {
            const float sb = theta_b[(size_t)f * 82 + 72 + k];
            betas2[(size_t)(nT + f) * 10 + k] = sb;
            if (row >= 0) theta[(size_t)row * 82 + 72 + k] = (theta_a[(size_t)f * 82 + 72 + k] + sb) * 0.5f;
        } else if (row >= 0) {
            theta[(size_t)row * 82 + 72 + k] = theta_a[(size_t)f * 82 + 72 + k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// vertex backward.  zs[(val * 64 + vertex) * 20 + frame]: val 0 .. 2 g, 3 .. 5 vp, 6 .. 8 dvp of the 16 frames of the workgroup.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smpl_verts_bwd_kernel(const float* __restrict__ vt, const float* __restrict__ sd, const float* __restrict__ pd,
                                                             const float* __restrict__ pt, const float* __restrict__ lbsw,
                                                             const float* __restrict__ Q, const float* __restrict__ betas,
                                                             const float* __restrict__ Aws, const float* __restrict__ PFws,
                                                             const float* __restrict__ dverts, const float* __restrict__ dkp, float scale,
                                                             float* __restrict__ part, int F, int V, int K, int nvt, int S) {
    __shared__ __attribute__((aligned(16))) float zs[9 * 64 * SM_ZS];
    __shared__ float wl[64 * 25];
    __shared__ float qs[32 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x;
    const int f0 = blockIdx.y * SM_BF;
    const int kcol = min(tid, SM_PT - 1);
    const int ja = tid >> 3, fa = tid & 7;
    float accP[SM_BF];
    float accA[2][12];
#pragma unroll
    for (int i = 0; i < SM_BF; ++i) accP[i] = 0.0f;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int e = 0; e < 12; ++e) accA[r][e] = 0.0f;
    int fi[SM_BW];
#pragma unroll
    for (int i = 0; i < SM_BW; ++i) fi[i] = min(f0 + wave * SM_BW + i, F - 1);

    for (int t = split; t < nvt; t += S) {
        const int v0 = t * SM_VT;
        const bool live = v0 + lane < V;
        const int v = live ? v0 + lane : V - 1;
        __syncthreads();                                  // the previous tile's phase 2 is through with zs / wl / qs
        for (int idx = tid; idx < 64 * SM_J; idx += 256) {
            const int l = idx / SM_J, j = idx - l * SM_J;
            wl[l * 25 + j] = lbsw[(size_t)min(v0 + l, V - 1) * SM_J + j];
        }
        if (dkp) {
            for (int idx = tid; idx < K * 64; idx += 256) {
                const int k = idx >> 6, l = idx & 63;
                qs[idx] = (v0 + l < V) ? Q[(size_t)k * V + v0 + l] : 0.0f;
            }
        }
        __syncthreads();
        // ---- phase 1: lane = vertex, the wave's 4 frames
        {
            float w[SM_J];
            unsigned mask = 0;
#pragma unroll
            for (int j = 0; j < SM_J; ++j) {
                w[j] = wl[lane * 25 + j];
                if (__ballot(w[j] != 0.0f) != 0ull) mask |= 1u << j;
            }
            float vp[SM_BW][3], g[SM_BW][3], dvp[SM_BW][3];
            smpl_vposed<SM_BW>(vt, sd, pd, betas, PFws, fi, v, V, vp);
#pragma unroll
            for (int i = 0; i < SM_BW; ++i) {
                float T[12];
                smpl_blend(w, mask, Aws + (size_t)fi[i] * SM_A, T);
#pragma unroll
                for (int c = 0; c < 3; ++c) g[i][c] = dverts ? dverts[((size_t)fi[i] * V + v) * 3 + c] : 0.0f;
                if (dkp) {
                    const float* dk = dkp + (size_t)fi[i] * K * 3;
                    for (int k = 0; k < K; ++k) {
                        const float q = qs[k * 64 + lane];
                        g[i][0] += q * dk[3 * k]; g[i][1] += q * dk[3 * k + 1]; g[i][2] += q * dk[3 * k + 2];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) g[i][c] = live ? scale * g[i][c] : 0.0f;
#pragma unroll
                for (int d = 0; d < 3; ++d) dvp[i][d] = T[d] * g[i][0] + T[4 + d] * g[i][1] + T[8 + d] * g[i][2];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                *reinterpret_cast<float4*>(&zs[((0 + c) * 64 + lane) * SM_ZS + wave * SM_BW]) = make_float4(g[0][c], g[1][c], g[2][c], g[3][c]);
                *reinterpret_cast<float4*>(&zs[((3 + c) * 64 + lane) * SM_ZS + wave * SM_BW]) = make_float4(vp[0][c], vp[1][c], vp[2][c], vp[3][c]);
                *reinterpret_cast<float4*>(&zs[((6 + c) * 64 + lane) * SM_ZS + wave * SM_BW]) =
                    make_float4(dvp[0][c], dvp[1][c], dvp[2][c], dvp[3][c]);
            }
        }
        __syncthreads();
        // ---- phase 2, columns of PT: thread = column, 16 frames in registers, the tile's 192 (vertex, coordinate) rows in order
        {
            const int rows = min(3 * SM_VT, 3 * V - 3 * v0);
            const float* ptc = pt + (size_t)3 * v0 * SM_PT + kcol;
            for (int vc = 0; vc < rows; ++vc) {
                const float pv = ptc[(size_t)vc * SM_PT];
                const int l = vc / 3, c = vc - 3 * l;
                const float4* z = reinterpret_cast<const float4*>(&zs[((6 + c) * 64 + l) * SM_ZS]);
                const float4 d0 = z[0], d1 = z[1], d2 = z[2], d3 = z[3];
                accP[0] += pv * d0.x; accP[1] += pv * d0.y; accP[2] += pv * d0.z; accP[3] += pv * d0.w;
                accP[4] += pv * d1.x; accP[5] += pv * d1.y; accP[6] += pv * d1.z; accP[7] += pv * d1.w;
                accP[8] += pv * d2.x; accP[9] += pv * d2.y; accP[10] += pv * d2.z; accP[11] += pv * d2.w;
                accP[12] += pv * d3.x; accP[13] += pv * d3.y; accP[14] += pv * d3.z; accP[15] += pv * d3.w;
            }
        }
        // ---- phase 2, d A: thread = (joint, frame mod 8), two frames, the tile's vertices in order
        if (ja < SM_J) {
            for (int l = 0; l < SM_VT; ++l) {
                const float wv = wl[l * 25 + ja];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int fo = r * 8 + fa;
                    const float p0 = zs[(3 * 64 + l) * SM_ZS + fo], p1 = zs[(4 * 64 + l) * SM_ZS + fo], p2 = zs[(5 * 64 + l) * SM_ZS + fo];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float gw = wv * zs[(c * 64 + l) * SM_ZS + fo];
                        accA[r][c * 4] += gw * p0; accA[r][c * 4 + 1] += gw * p1; accA[r][c * 4 + 2] += gw * p2; accA[r][c * 4 + 3] += gw;
                    }
                }
            }
        }
    }
    if (tid < SM_PT) {
#pragma unroll
        for (int i = 0; i < SM_BF; ++i)
            if (f0 + i < F) part[((size_t)split * F + f0 + i) * SM_COLS + tid] = accP[i];
    }
    if (ja < SM_J) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int f = f0 + r * 8 + fa;
            if (f < F) {
                float* o = part + ((size_t)split * F + f) * SM_COLS + SM_PT + ja * 12;
#pragma unroll
                for (int e = 0; e < 12; ++e) o[e] = accA[r][e];
            }
        }
    }
}

__global__ __launch_bounds__(256) void smpl_split_sum_kernel(const float* __restrict__ part, int S, float* __restrict__ sums, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int t = 0; t < S; ++t) s += part[(size_t)t * n + i];
    sums[i] = s;
}

// chain backward, one thread per frame.  D: scratch [288][F] (d Grot_j [9], d Gt_j [3]); DJ: scratch [72][F] (d J_j).
__global__ __launch_bounds__(64) void smpl_chain_bwd_kernel(const float* __restrict__ betas, const float* __restrict__ rotmat,
                                                            const float* __restrict__ Jt, const float* __restrict__ Jd, SmplTree tree, float scale,
                                                            const float* __restrict__ Aws, const float* __restrict__ sums,
                                                            const float* __restrict__ djoints, float* D, float* DJ, float* __restrict__ drot,
                                                            float* __restrict__ dbetas, int F) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    float b[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) b[k] = betas[(size_t)f * 10 + k];
    const float* R = rotmat + (size_t)f * 216;
    const float* A = Aws + (size_t)f * SM_A;
    const float* sm = sums + (size_t)f * SM_COLS;
#define SM_D(j, e) D[(size_t)((j) * 12 + (e)) * F + f]
#define SM_DJ(j, c) DJ[(size_t)((j) * 3 + (c)) * F + f]
    for (int j = 0; j < SM_J; ++j) {
        float J[3], dA[12];
        smpl_joint(Jt, Jd, b, j, J);
#pragma unroll
        for (int e = 0; e < 12; ++e) dA[e] = sm[SM_PT + j * 12 + e];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int d = 0; d < 3; ++d) SM_D(j, c * 3 + d) = dA[c * 4 + d] - dA[c * 4 + 3] * J[d];
            SM_D(j, 9 + c) = dA[c * 4 + 3] + (djoints ? scale * djoints[(size_t)f * 72 + j * 3 + c] : 0.0f);
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) SM_DJ(j, m) = -(A[j * 12 + m] * dA[3] + A[j * 12 + 4 + m] * dA[7] + A[j * 12 + 8 + m] * dA[11]);
    }
    float* dR = drot + (size_t)f * 216;
    for (int j = SM_J - 1; j >= 1; --j) {
        const int p = tree.p[j];
        float J[3], Jp[3], rel[3], r[9], dG[9], dt[3], Gp[9];
        smpl_joint(Jt, Jd, b, j, J);
        smpl_joint(Jt, Jd, b, p, Jp);
#pragma unroll
        for (int c = 0; c < 3; ++c) rel[c] = J[c] - Jp[c];
#pragma unroll
        for (int e = 0; e < 9; ++e) { r[e] = R[j * 9 + e]; dG[e] = SM_D(j, e); Gp[e] = A[p * 12 + (e / 3) * 4 + (e % 3)]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) dt[c] = SM_D(j, 9 + c);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int m = 0; m < 3; ++m)
                SM_D(p, c * 3 + m) = SM_D(p, c * 3 + m) + (dG[c * 3] * r[m * 3] + dG[c * 3 + 1] * r[m * 3 + 1] + dG[c * 3 + 2] * r[m * 3 + 2]) + dt[c] * rel[m];
            SM_D(p, 9 + c) = SM_D(p, 9 + c) + dt[c];
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
                dR[j * 9 + m * 3 + d] = (Gp[m] * dG[d] + Gp[3 + m] * dG[3 + d] + Gp[6 + m] * dG[6 + d]) + sm[(j - 1) * 9 + m * 3 + d];
            const float drel = Gp[m] * dt[0] + Gp[3 + m] * dt[1] + Gp[6 + m] * dt[2];
            SM_DJ(j, m) = SM_DJ(j, m) + drel;
            SM_DJ(p, m) = SM_DJ(p, m) - drel;
        }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) dR[e] = SM_D(0, e);
#pragma unroll
    for (int c = 0; c < 3; ++c) SM_DJ(0, c) = SM_DJ(0, c) + SM_D(0, 9 + c);
    float db[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) db[k] = sm[SM_PF + k];
    for (int j = 0; j < SM_J; ++j) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float dj = SM_DJ(j, m);
#pragma unroll
            for (int k = 0; k < 10; ++k) db[k] += Jd[(j * 3 + m) * 10 + k] * dj;
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) dbetas[(size_t)f * 10 + k] = db[k];
#undef SM_D
#undef SM_DJ
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
static inline int sm_tiles(int V) { return (V + SM_VT - 1) / SM_VT; }
static inline int sm_splits(int V) { const int t = sm_tiles(V); return t < SM_SPLITS ? t : SM_SPLITS; }
static inline bool sm_dims_ok(int F, int V, int K) { return F >= 0 && F <= (1 << 20) && V >= 1 && V <= (1 << 20) && K >= 0 && K <= 32; }

// The workspace of every entry, for F parameter sets: A [F,288] | pf [F,208] | chain scratch [288,F] | tail.  The tail is
//   forward : keypoint partials [tiles,F,3K], then what the entry adds (mesh_gt: rotations [F,216]; wild_mesh with pass B: rotations
//             [F,216] and shapes [F,10] of both passes);
//   backward: d J scratch [72,F] | partials [S,F,512] | sums [F,512].
struct SmWs { float *A, *PF, *G, *tail; };
static inline size_t sm_common_floats(int F) { return (size_t)F * (SM_A + SM_PFS + SM_A); }
static inline size_t sm_fwd_floats(int F, int V, int K) { return sm_common_floats(F) + (size_t)sm_tiles(V) * F * 3 * K; }
static inline size_t sm_ws_bytes(size_t floats) { return floats * sizeof(float) + 256; }
static inline SmWs sm_carve(void* ws, int F) {
    SmWs w = {};
    if (!ws) return w;                          // an entry that needs the workspace has refused a null one before it launches
    w.A = (float*)ws;
    w.PF = w.A + (size_t)F * SM_A;
    w.G = w.PF + (size_t)F * SM_PFS;
    w.tail = w.A + sm_common_floats(F);
    return w;
}

extern "C" size_t mbx_smpl_fwd_ws(int F, int V, int K) {
    if (!sm_dims_ok(F, V, K) || F < 1) return 0;
    return sm_ws_bytes(sm_fwd_floats(F, V, K));
}

extern "C" size_t mbx_smpl_bwd_ws(int F, int V, int K) {
    if (!sm_dims_ok(F, V, K) || F < 1) return 0;
    return sm_ws_bytes(sm_common_floats(F) + (size_t)F * 72 + (size_t)(sm_splits(V) + 1) * F * SM_COLS);
}

extern "C" size_t mbx_mesh_gt_ws(int F, int V, int K) {
    if (!sm_dims_ok(F, V, K) || F < 1 || K < 1) return 0;
    return sm_ws_bytes(sm_fwd_floats(F, V, K) + (size_t)F * 216);
}

extern "C" size_t mbx_wild_mesh_ws(int nT, int V, int K, int pair) {
    if (nT < 1 || nT > (1 << 20) / (pair ? 2 : 1)) return 0;
    const int FC = pair ? 2 * nT : nT;
    if (!sm_dims_ok(FC, V, K)) return 0;
    return sm_ws_bytes(sm_fwd_floats(FC, V, K) + (pair ? (size_t)FC * 226 : 0));
}

// the model arrays every entry takes; Q may be null where no keypoints are asked for
struct SmModel { const float *v_template, *shapedirs, *posedirs, *Jt, *Jd, *lbs_weights, *Q; };
static inline bool sm_model_set(const SmModel& m) { return m.v_template && m.shapedirs && m.posedirs && m.Jt && m.Jd && m.lbs_weights; }
template <class... P>
static inline uintptr_t sm_or(P... p) { return (uintptr_t(0) | ... | (uintptr_t)p); }
// the model arrays and the entry's own pointers (rest: sm_or of them) 4-byte aligned, the workspace 16-byte
static int sm_check_align(const char* who, const SmModel& m, uintptr_t rest, const void* ws) {
    MBX_CHECK_ARG(((sm_or(m.v_template, m.shapedirs, m.posedirs, m.Jt, m.Jd, m.lbs_weights, m.Q) | rest) & 3) == 0 && ((uintptr_t)ws & 15) == 0,
                  "%s: pointers must be 4-byte aligned, the workspace 16-byte aligned", who);
    return 0;
}

extern "C" int mbx_smpl_pack(const float* shapedirs, const float* posedirs, float* packed_t, int V, void* stream) {
    MBX_CHECK_ARG(V >= 1 && V <= (1 << 20), "smpl_pack: bad vertex count V=%d", V);
    MBX_CHECK_ARG(shapedirs && posedirs && packed_t, "smpl_pack: null pointer");
    MBX_CHECK_ARG((((uintptr_t)shapedirs | (uintptr_t)posedirs | (uintptr_t)packed_t) & 3) == 0, "smpl_pack: pointers must be 4-byte aligned");
    const size_t n = (size_t)3 * V * SM_PT;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(smpl_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, shapedirs, posedirs, packed_t, V);
    MBX_LAUNCH_CHECK("smpl_pack");
    return 0;
}

static int sm_tree(const int* parents, SmplTree& tree, const char* who) {
    MBX_CHECK_ARG(parents, "%s: null parents", who);
    MBX_CHECK_ARG(parents[0] == -1, "%s: parents[0] must be -1, got %d", who, parents[0]);
    tree.p[0] = -1;
    for (int j = 1; j < SM_J; ++j) {
        MBX_CHECK_ARG(parents[j] >= 0 && parents[j] < j, "%s: parents[%d] = %d is not a forward-ordered tree (0 <= parents[j] < j)", who, j, parents[j]);
        tree.p[j] = parents[j];
    }
    return 0;
}

// The launches the entries are made of; `who` is the entry's name for the step, as a failed launch reports it.
static int sm_launch_chain(const char* who, hipStream_t s, const SmModel& m, const SmplTree& tree, const float* betas, const float* rotmat,
                           float scale, const SmWs& w, float* joints, int F) {
    hipLaunchKernelGGL(smpl_chain_fwd_kernel, dim3((F + 63) / 64), dim3(64), 0, s, betas, rotmat, m.Jt, m.Jd, tree, scale, w.A, w.PF, w.G, joints, F);
    MBX_LAUNCH_CHECK(who);
    return 0;
}

// nF output frames of NP parameter sets each; kpart: the tile partials of K keypoints (null: none); dst_frames / T / F: where STITCH
template <int NP, bool STITCH>
static int sm_launch_verts(const char* who, hipStream_t s, const SmModel& m, const float* betas, const SmWs& w, float scale, float* verts,
                           float* kpart, int nF, int V, int K, const int* dst_frames = nullptr, int T = 0, int F = 0) {
    constexpr int per_wg = 4 * (SM_FW / NP);
    hipLaunchKernelGGL((smpl_verts_kernel<NP, STITCH>), dim3(sm_tiles(V), (nF + per_wg - 1) / per_wg), dim3(256), 0, s, m.v_template, m.shapedirs,
                       m.posedirs, m.lbs_weights, m.Q, betas, (const float*)w.A, (const float*)w.PF, scale, verts, kpart, nF, V, K, dst_frames, T, F);
    MBX_LAUNCH_CHECK(who);
    return 0;
}

template <int NP, bool STITCH>
static int sm_launch_kp_finish(const char* who, hipStream_t s, const float* kpart, float scale, float* kp, int nF, int V, int K,
                               const int* dst_frames = nullptr, int T = 0, int F = 0) {
    const size_t n = (size_t)nF * 3 * K;
    hipLaunchKernelGGL((smpl_kp_finish_kernel<NP, STITCH>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kpart, sm_tiles(V), scale, kp, n,
                       3 * K, dst_frames, T, F);
    MBX_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int mbx_smpl_fwd(const float* v_template, const float* shapedirs, const float* posedirs, const float* Jt, const float* Jd,
                            const int* parents, const float* lbs_weights, const float* Q, int K, const float* betas, const float* rotmat,
                            float scale, float* verts, float* kp, float* joints, int F, int V, void* ws, size_t ws_bytes, void* stream) {
    const SmModel m = {v_template, shapedirs, posedirs, Jt, Jd, lbs_weights, Q};
    MBX_CHECK_ARG(sm_dims_ok(F, V, K), "smpl_fwd: bad sizes F=%d V=%d K=%d (V >= 1, K <= 32)", F, V, K);
    SmplTree tree;
    if (sm_tree(parents, tree, "smpl_fwd")) return 1;
    if (F == 0) return 0;
    MBX_CHECK_ARG(sm_model_set(m) && betas && rotmat && ws, "smpl_fwd: null pointer");
    MBX_CHECK_ARG(verts || kp || joints, "smpl_fwd: no output");
    MBX_CHECK_ARG(!kp || (Q && K >= 1), "smpl_fwd: kp needs a regressor Q [K,V] with K >= 1");
    const int Kv = kp ? K : 0;
    MBX_CHECK_ARG(ws_bytes >= mbx_smpl_fwd_ws(F, V, Kv), "smpl_fwd: workspace of %zu bytes, %zu needed", ws_bytes, mbx_smpl_fwd_ws(F, V, Kv));
    if (sm_check_align("smpl_fwd", m, sm_or(betas, rotmat, verts, kp, joints), ws)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const SmWs w = sm_carve(ws, F);
    float* kpart = kp ? w.tail : nullptr;
    if (sm_launch_chain("smpl_fwd (chain)", s, m, tree, betas, rotmat, scale, w, joints, F)) return 1;
    if (!verts && !kp) return 0;
    if (sm_launch_verts<1, false>("smpl_fwd (vertices)", s, m, betas, w, scale, verts, kpart, F, V, Kv)) return 1;
    if (kp && sm_launch_kp_finish<1, false>("smpl_fwd (keypoints)", s, kpart, scale, kp, F, V, K)) return 1;
    return 0;
}

extern "C" int mbx_mesh_gt(const float* pose, const float* shape, const float* motion_2d, const unsigned char* flips, uint64_t seed,
                           float flip_prob, const float* v_template, const float* shapedirs, const float* posedirs, const float* Jt,
                           const float* Jd, const int* parents, const float* lbs_weights, const float* Q, int K, float scale, float* x2d,
                           float* theta, float* kp_3d, float* verts, unsigned char* flips_used, int N, int T, int V, void* ws,
                           size_t ws_bytes, void* stream) {
    const SmModel m = {v_template, shapedirs, posedirs, Jt, Jd, lbs_weights, Q};
    MBX_CHECK_ARG(N >= 0 && T >= 1 && (long long)N * T <= (1 << 20), "mesh_gt: bad sizes N=%d T=%d (T >= 1, N T <= 2^20)", N, T);
    const int F = N * T;
    MBX_CHECK_ARG(sm_dims_ok(F, V, K) && K >= 1, "mesh_gt: bad sizes F=%d V=%d K=%d (V >= 1, 1 <= K <= 32)", F, V, K);
    SmplTree tree;
    if (sm_tree(parents, tree, "mesh_gt")) return 1;
    if (F == 0) return 0;
    MBX_CHECK_ARG(x2d || theta || kp_3d || verts || flips_used, "mesh_gt: no output");
    MBX_CHECK_ARG(flips || (flip_prob >= 0.0f && flip_prob <= 1.0f), "mesh_gt: flip_prob must lie in [0, 1]");
    const bool body = kp_3d || verts;
    MBX_CHECK_ARG(pose && shape, "mesh_gt: null pointer (pose, shape)");
    MBX_CHECK_ARG(!x2d || motion_2d, "mesh_gt: x2d needs motion_2d");
    MBX_CHECK_ARG(!x2d || x2d != motion_2d, "mesh_gt: x2d must not alias motion_2d (the flip permutes joints)");
    MBX_CHECK_ARG(!body || (sm_model_set(m) && Q && ws), "mesh_gt: null pointer (kp_3d and verts need the model arrays, Q and a workspace)");
    MBX_CHECK_ARG(!body || ws_bytes >= mbx_mesh_gt_ws(F, V, K), "mesh_gt: workspace of %zu bytes, %zu needed", ws_bytes, mbx_mesh_gt_ws(F, V, K));
    if (sm_check_align("mesh_gt", m, sm_or(pose, shape, motion_2d, x2d, theta, kp_3d, verts), body ? ws : nullptr)) return 1;
    hipStream_t s = (hipStream_t)stream;
    // the vertex kernel forms the partials of the Kv keypoints the caller reads: all K for kp_3d, the root alone for verts
    const int Kv = kp_3d ? K : 1;
    const SmWs w = sm_carve(body ? ws : nullptr, F);
    float* rot = body ? w.A + sm_fwd_floats(F, V, K) : nullptr;
    hipLaunchKernelGGL(mesh_gt_prepare_kernel, dim3((F + 3) / 4), dim3(256), 0, s, pose, shape, motion_2d, flips, (uint32_t)seed,
                       (uint32_t)(seed >> 32), flip_prob, x2d, theta, rot, flips_used, F, T);
    MBX_LAUNCH_CHECK("mesh_gt (prepare)");
    if (!body) return 0;
    if (sm_launch_chain("mesh_gt (chain)", s, m, tree, shape, rot, scale, w, nullptr, F)) return 1;
    if (sm_launch_verts<1, false>("mesh_gt (vertices)", s, m, shape, w, scale, verts, w.tail, F, V, Kv)) return 1;
    const int chunks = verts ? (V + MG_CV - 1) / MG_CV : 1;
    hipLaunchKernelGGL(mesh_gt_centre_kernel, dim3((F + MG_CF - 1) / MG_CF, chunks), dim3(256), 0, s, (const float*)w.tail, sm_tiles(V), 3 * Kv,
                       scale, verts, kp_3d, F, V);
    MBX_LAUNCH_CHECK("mesh_gt (centring)");
    return 0;
}

extern "C" int mbx_wild_mesh(const float* v_template, const float* shapedirs, const float* posedirs, const float* Jt, const float* Jd,
                             const int* parents, const float* lbs_weights, const float* Q, int K, const float* rotmat_a, const float* betas_a,
                             const float* theta_a, const float* theta_b, float scale, const int* dst_frames, int dst_max, int n, int T, int F,
                             float* verts, float* kp, float* theta, int V, void* ws, size_t ws_bytes, void* stream) {
    const SmModel m = {v_template, shapedirs, posedirs, Jt, Jd, lbs_weights, Q};
    const bool pair = theta_b != nullptr;
    MBX_CHECK_ARG(n >= 0 && T >= 1 && (long long)n * T * (pair ? 2 : 1) <= (1 << 20),
                  "wild_mesh: bad sizes n=%d T=%d (T >= 1, n T <= 2^20, 2 n T with pass B)", n, T);
    const int nT = n * T, FC = pair ? 2 * nT : nT;
    MBX_CHECK_ARG(sm_dims_ok(FC, V, K) && F >= 0, "wild_mesh: bad sizes n T=%d V=%d K=%d F=%d (V >= 1, K <= 32, F >= 0)", nT, V, K, F);
    SmplTree tree;
    if (sm_tree(parents, tree, "wild_mesh")) return 1;
    if (nT == 0) return 0;
    MBX_CHECK_ARG(dst_max >= 0 && (long long)dst_max + T <= F, "wild_mesh: a clip of %d frames at row %d does not fit the %d rows of the result",
                  T, dst_max, F);
    MBX_CHECK_ARG(verts || kp || theta, "wild_mesh: no output");
    MBX_CHECK_ARG(dst_frames && rotmat_a && betas_a, "wild_mesh: null pointer (dst_frames, rotmat_a, betas_a)");
    MBX_CHECK_ARG(!theta || theta_a, "wild_mesh: theta needs theta_a");
    const bool body = verts || kp;
    MBX_CHECK_ARG(!body || sm_model_set(m), "wild_mesh: null pointer (model arrays)");
    MBX_CHECK_ARG(!kp || (Q && K >= 1), "wild_mesh: kp needs a regressor Q [K,V] with K >= 1");
    MBX_CHECK_ARG(!(body || pair) || ws, "wild_mesh: null workspace");
    const int Kv = kp ? K : 0;
    MBX_CHECK_ARG(!(body || pair) || ws_bytes >= mbx_wild_mesh_ws(nT, V, Kv, pair), "wild_mesh: workspace of %zu bytes, %zu needed", ws_bytes,
                  mbx_wild_mesh_ws(nT, V, Kv, pair));
    if (sm_check_align("wild_mesh", m, sm_or(rotmat_a, betas_a, theta_a, theta_b, dst_frames, verts, kp, theta), ws)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const SmWs w = sm_carve(ws, FC);
    float* kpart = kp ? w.tail : nullptr;
    float* rot2 = pair ? w.A + sm_fwd_floats(FC, V, Kv) : nullptr;
    float* betas2 = pair ? rot2 + (size_t)FC * 216 : nullptr;
    if (pair || theta) {
        hipLaunchKernelGGL(wild_mesh_prepare_kernel, dim3((nT + 3) / 4), dim3(256), 0, s, rotmat_a, betas_a, theta_a, theta_b, dst_frames, rot2,
                           betas2, theta, nT, T, F);
        MBX_LAUNCH_CHECK("wild_mesh (prepare)");
    }
    if (!body) return 0;
    const float* betas = pair ? betas2 : betas_a;
    if (sm_launch_chain("wild_mesh (chain)", s, m, tree, betas, pair ? rot2 : rotmat_a, scale, w, nullptr, FC)) return 1;
    if (pair) {
        if (sm_launch_verts<2, true>("wild_mesh (vertices)", s, m, betas, w, scale, verts, kpart, nT, V, Kv, dst_frames, T, F)) return 1;
        if (kp && sm_launch_kp_finish<2, true>("wild_mesh (keypoints)", s, kpart, scale, kp, nT, V, K, dst_frames, T, F)) return 1;
    } else {
        if (sm_launch_verts<1, true>("wild_mesh (vertices)", s, m, betas, w, scale, verts, kpart, nT, V, Kv, dst_frames, T, F)) return 1;
        if (kp && sm_launch_kp_finish<1, true>("wild_mesh (keypoints)", s, kpart, scale, kp, nT, V, K, dst_frames, T, F)) return 1;
    }
    return 0;
}

extern "C" int mbx_smpl_bwd(const float* v_template, const float* shapedirs, const float* posedirs, const float* packed_t, const float* Jt,
                            const float* Jd, const int* parents, const float* lbs_weights, const float* Q, int K, const float* betas,
                            const float* rotmat, float scale, const float* dverts, const float* dkp, const float* djoints, float* drotmat,
                            float* dbetas, int F, int V, void* ws, size_t ws_bytes, void* stream) {
    const SmModel m = {v_template, shapedirs, posedirs, Jt, Jd, lbs_weights, Q};
    MBX_CHECK_ARG(sm_dims_ok(F, V, K), "smpl_bwd: bad sizes F=%d V=%d K=%d (V >= 1, K <= 32)", F, V, K);
    SmplTree tree;
    if (sm_tree(parents, tree, "smpl_bwd")) return 1;
    if (F == 0) return 0;
    MBX_CHECK_ARG(sm_model_set(m) && packed_t && betas && rotmat && drotmat && dbetas && ws, "smpl_bwd: null pointer");
    MBX_CHECK_ARG(!dkp || (Q && K >= 1), "smpl_bwd: dkp needs a regressor Q [K,V] with K >= 1");
    MBX_CHECK_ARG(ws_bytes >= mbx_smpl_bwd_ws(F, V, K), "smpl_bwd: workspace of %zu bytes, %zu needed", ws_bytes, mbx_smpl_bwd_ws(F, V, K));
    MBX_CHECK_ARG(drotmat != rotmat && dbetas != betas, "smpl_bwd: a gradient must not alias its input");
    if (sm_check_align("smpl_bwd", m, sm_or(packed_t, betas, rotmat, dverts, dkp, djoints, drotmat, dbetas), ws)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int nvt = sm_tiles(V), S = sm_splits(V);
    const SmWs w = sm_carve(ws, F);
    float* DJ = w.tail;
    float* part = DJ + (size_t)F * 72;
    float* sums = part + (size_t)S * F * SM_COLS;
    if (sm_launch_chain("smpl_bwd (chain)", s, m, tree, betas, rotmat, scale, w, nullptr, F)) return 1;
    hipLaunchKernelGGL(smpl_verts_bwd_kernel, dim3(S, (F + SM_BF - 1) / SM_BF), dim3(256), 0, s, v_template, shapedirs, posedirs, packed_t,
                       lbs_weights, Q, betas, (const float*)w.A, (const float*)w.PF, dverts, dkp, scale, part, F, V, dkp ? K : 0, nvt, S);
    MBX_LAUNCH_CHECK("smpl_bwd (vertices)");
    const size_t n = (size_t)F * SM_COLS;
    hipLaunchKernelGGL(smpl_split_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)part, S, sums, n);
    MBX_LAUNCH_CHECK("smpl_bwd (split sum)");
    hipLaunchKernelGGL(smpl_chain_bwd_kernel, dim3((F + 63) / 64), dim3(64), 0, s, betas, rotmat, Jt, Jd, tree, scale, (const float*)w.A,
                       (const float*)sums, djoints, w.G, DJ, drotmat, dbetas, F);
    MBX_LAUNCH_CHECK("smpl_bwd (chain backward)");
    return 0;
}
