// One-shot action recognition on the device (train_action_1shot.py:58-69,186-198; lib/model/loss_supcon.py:57-98).
//   mbx_supcon_loss : the supervised-contrastive loss of A = bsz * n_views anchors (contrast_mode 'all') and its gradient in one call,
//                     optionally through the L2 normalisation of the embedding head.  fp32, no floating-point atomics.
//   mbx_nn_cosine   : 1-nearest-neighbour classification of N test rows against M exemplars by cosine similarity; neither the
//                     [M,N,D] broadcast nor the [M,N] similarity matrix exists in memory.
// Every sum has a fixed order, so two calls on the same inputs return the same bits.  Dot products over D are BLOCKED: a chain of at
// most 32 fused multiply-adds starts at zero for every 32 columns and the chunk results are added in column order, which bounds the
// rounding error by (32 + D / 32) roundings instead of D (tests/supconerr.py derives its gates from this order).
#include "mbx_common.h"
#include <math.h>

#define OS_KC 32            // columns per chunk of a blocked dot product
#define SC_MAX_A 128        // anchors of mbx_supcon_loss
#define SC_MAX_SPLIT 128    // workgroups of the Gram pass

// ---------------------------------------------------------------------------------------------------------------
// supcon, pass 1: partial Gram products.  Workgroup s owns `cps` consecutive 32-column chunks of feat [A,D] and leaves
// part[s][i][j] = sum over its columns of z_ik z_jk.  256 threads as 16 x 16, thread (ti, tj) owns the R x R outputs
// (ti + 16 r, tj + 16 c): the chunk lies transposed in LDS with an odd row stride, so the 16 consecutive j of a wave read 16
// consecutive words, its 4 values of i are broadcasts, and the transposing store of the staging loop (32 consecutive k of one
// row) falls on 32 different banks.  The diagonal of the sum over s is |z_i|^2.
// ---------------------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void supcon_gram_kernel(const float* __restrict__ feat, float* __restrict__ part, int A, int D, int cps) {
    constexpr int AP = 16 * R + 1;
    __shared__ float xs[OS_KC * AP];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    float tot[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) tot[r][c] = 0.f;
    for (int q = 0; q < cps; ++q) {
        const int k0 = (blockIdx.x * cps + q) * OS_KC;
        if (k0 >= D) break;                                   // uniform over the workgroup
        __syncthreads();                                      // the previous chunk has been read
        for (int e = tid; e < 16 * R * OS_KC; e += 256) {
            const int i = e >> 5, k = e & (OS_KC - 1);
            xs[k * AP + i] = (i < A && k0 + k < D) ? feat[(size_t)i * D + k0 + k] : 0.f;
        }
        __syncthreads();
        float acc[R][R];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < R; ++c) acc[r][c] = 0.f;
#pragma unroll 4
        for (int k = 0; k < OS_KC; ++k) {
            float a[R], b[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { a[r] = xs[k * AP + ti + 16 * r]; b[r] = xs[k * AP + tj + 16 * r]; }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < R; ++c) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < R; ++c) tot[r][c] += acc[r][c];
    }
    float* out = part + (size_t)blockIdx.x * A * A;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int i = ti + 16 * r, j = tj + 16 * c;
            if (i < A && j < A) out[i * A + j] = tot[r][c];
        }
}

// sum / max over the 128 threads (two waves) of the row kernel; every thread of the workgroup calls it
template <typename Op> __device__ __forceinline__ float sc_block2(float v, float* red) {
    const float w = wave_reduce<Op>(v);
    __syncthreads();                                          // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    return Op::op(red[0], red[1]);
}

// ---------------------------------------------------------------------------------------------------------------
// supcon, pass 2: workgroup i = anchor row i, thread j = contrast column j (128 threads, j >= A idle but present in the wave
// reductions).  Adds the partial products in split order, forms the logits, the row maximum (diagonal included, as
// loss_supcon.py:73 includes it), the denominator without the diagonal, the positives, the row's loss and
//     G_ij = (tau / tau_b) / A * (softmax_{j != i}(S_i)_j - [j in P(i)] / n_i),   G_ii = 0
// A row without a positive has 1 / n_i = inf: 0 * inf = NaN in every G_ij of the row and 0 / 0 in its loss, the reference's 0 / 0.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void supcon_row_kernel(const float* __restrict__ part, int nsplit, const int* __restrict__ labels, int A,
                                                         int n_views, float tau, float ratio, int normalize, float* __restrict__ G,
                                                         float* __restrict__ inv_norm, float* __restrict__ norm, float* __restrict__ loss_row) {
    __shared__ float red[2];
    __shared__ float inv_i_sh;
    const int i = blockIdx.x, j = threadIdx.x;
    const bool valid = j < A;
    float dot = 0.f, n2 = 0.f;
    if (valid) {
        const size_t AA = (size_t)A * A;
        for (int s = 0; s < nsplit; ++s) dot += part[s * AA + (size_t)i * A + j];
        if (normalize)
            for (int s = 0; s < nsplit; ++s) n2 += part[s * AA + (size_t)j * A + j];
    }
    const float norm_j = sqrtf(n2);
    const float inv_j = normalize ? 1.0f / fmaxf(norm_j, 1e-12f) : 1.0f;         // F.normalize: z / max(|z|, 1e-12)
    if (j == i) inv_i_sh = inv_j;
    __syncthreads();
    const float inv_i = inv_i_sh;
    const float s_ij = normalize ? ((dot * inv_i) * inv_j) / tau : dot / tau;
    const float m = sc_block2<WaveMax>(valid ? s_ij : -INFINITY, red);
    const bool other = valid && j != i;
    const float a_ij = s_ij - m;
    const float e = other ? expf(a_ij) : 0.f;
    const float den = sc_block2<WaveAdd>(e, red);
    const float lse = logf(den);
    const bool pos = other && labels[j / n_views] == labels[i / n_views];
    const float n_i = sc_block2<WaveAdd>(pos ? 1.f : 0.f, red);
    const float sum_pos = sc_block2<WaveAdd>(pos ? a_ij - lse : 0.f, red);
    const float inv_n = 1.0f / n_i;
    if (valid) G[(size_t)i * A + j] = (ratio / (float)A) * (e / den - (pos ? 1.f : 0.f) * inv_n);
    if (j == i) { inv_norm[i] = inv_j; norm[i] = norm_j; }
    if (j == 0) loss_row[i] = -ratio * (sum_pos / n_i);
}

// ---------------------------------------------------------------------------------------------------------------
// supcon, pass 3: the last workgroup averages the row losses in a fixed tree; workgroup i < A (launched only with dfeat) owns row i
// of the gradient:  g_i = sum_j w_j x_j,  w_j = (G_ij + G_ji) / tau,  x_j = z_j / max(|z_j|, 1e-12) under `normalize`, j ascending.
// Under `normalize` the row goes back through the normalisation: dz = (g - x (x . g)) / |z|, or g / 1e-12 where the norm was
// clamped.  x . g needs the whole row, so g is parked in dfeat and read back by the thread that wrote it.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void supcon_grad_kernel(const float* __restrict__ feat, const float* __restrict__ G,
                                                          const float* __restrict__ inv_norm, const float* __restrict__ norm,
                                                          const float* __restrict__ loss_row, int A, int D,
                                                          float tau, int normalize, float grad_scale, float* __restrict__ loss,
                                                          float* __restrict__ dfeat) {
    __shared__ float w[SC_MAX_A];
    __shared__ float inv[SC_MAX_A];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        if (tid < SC_MAX_A) w[tid] = tid < A ? loss_row[tid] : 0.f;
        __syncthreads();
        for (int h = SC_MAX_A / 2; h > 0; h >>= 1) {
            if (tid < h) w[tid] += w[tid + h];
            __syncthreads();
        }
        if (tid == 0) loss[0] = w[0] / (float)A;
        return;
    }
    const int i = blockIdx.x;
    if (tid < A) {
        w[tid] = (G[(size_t)i * A + tid] + G[(size_t)tid * A + i]) / tau;
        inv[tid] = inv_norm[tid];
    }
    __syncthreads();
    const float inv_i = inv[i];
    float* drow = dfeat + (size_t)i * D;
    float pdot = 0.f;
    for (int k = tid; k < D; k += 256) {
        float g = 0.f;
        if (normalize) {
            for (int j = 0; j < A; ++j) g = fmaf(w[j], feat[(size_t)j * D + k] * inv[j], g);
            pdot = fmaf(feat[(size_t)i * D + k] * inv_i, g, pdot);
            drow[k] = g;
        } else {
            for (int j = 0; j < A; ++j) g = fmaf(w[j], feat[(size_t)j * D + k], g);
            drow[k] = grad_scale * g;
        }
    }
    if (!normalize) return;                                   // uniform over the grid
    const float ws = wave_sum(pdot);
    if ((tid & 63) == 0) red[tid >> 6] = ws;
    __syncthreads();
    const float xg = (red[0] + red[1]) + (red[2] + red[3]);
    const bool clamped = norm[i] < 1e-12f;                    // max(|z|, 1e-12) took the floor: the denominator is a constant
    for (int k = tid; k < D; k += 256) {
        const float g = drow[k];
        const float x = feat[(size_t)i * D + k] * inv_i;
        drow[k] = grad_scale * ((clamped ? g : g - x * xg) * inv_i);
    }
}

static inline int sc_chunks(int D) { return (D + OS_KC - 1) / OS_KC; }
static inline int sc_cps(int D) { return (sc_chunks(D) + SC_MAX_SPLIT - 1) / SC_MAX_SPLIT; }
static inline int sc_nsplit(int D) { return (sc_chunks(D) + sc_cps(D) - 1) / sc_cps(D); }

// ws: part [nsplit][A][A] | G [A][A] | inv_norm [A] | norm [A] | loss_row [A]
extern "C" size_t mbx_supcon_loss_ws(int A, int D) {
    if (A < 2 || A > SC_MAX_A || D < 1) return 0;
    return ((size_t)(sc_nsplit(D) + 1) * A * A + 3 * (size_t)A) * sizeof(float) + 256;
}

extern "C" int mbx_supcon_loss(const float* feat, const int* labels, int bsz, int n_views, int D, float temperature, float base_temperature,
                               int normalize, float grad_scale, float* loss, float* dfeat, void* ws, void* stream) {
    MBX_CHECK_ARG(feat && labels && loss && ws, "supcon_loss: null pointer");
    MBX_CHECK_ARG(bsz > 0 && n_views > 0 && D >= 1, "supcon_loss: bad shape bsz=%d n_views=%d D=%d", bsz, n_views, D);
    const long long A64 = (long long)bsz * n_views;
    MBX_CHECK_ARG(A64 >= 2 && A64 <= SC_MAX_A, "supcon_loss: %lld anchors (bsz * n_views); 2 <= anchors <= %d are supported", A64, SC_MAX_A);
    MBX_CHECK_ARG(temperature > 0.f && base_temperature > 0.f, "supcon_loss: temperature %g / base temperature %g must be > 0",
                  (double)temperature, (double)base_temperature);
    const int A = (int)A64;
    hipStream_t s = (hipStream_t)stream;
    const int cps = sc_cps(D), nsplit = sc_nsplit(D);
    float* part = (float*)ws;
    float* G = part + (size_t)nsplit * A * A;
    float* inv_norm = G + (size_t)A * A;
    float* norm = inv_norm + A;
    float* loss_row = norm + A;
    if (A <= 32)
        hipLaunchKernelGGL(supcon_gram_kernel<2>, dim3(nsplit), dim3(256), 0, s, feat, part, A, D, cps);
    else if (A <= 64)
        hipLaunchKernelGGL(supcon_gram_kernel<4>, dim3(nsplit), dim3(256), 0, s, feat, part, A, D, cps);
    else
        hipLaunchKernelGGL(supcon_gram_kernel<8>, dim3(nsplit), dim3(256), 0, s, feat, part, A, D, cps);
    MBX_LAUNCH_CHECK("supcon_loss (gram)");
    hipLaunchKernelGGL(supcon_row_kernel, dim3(A), dim3(128), 0, s, (const float*)part, nsplit, labels, A, n_views, temperature,
                       temperature / base_temperature, normalize ? 1 : 0, G, inv_norm, norm, loss_row);
    MBX_LAUNCH_CHECK("supcon_loss (rows)");
    hipLaunchKernelGGL(supcon_grad_kernel, dim3(dfeat ? A + 1 : 1), dim3(256), 0, s, feat, (const float*)G, (const float*)inv_norm,
                       (const float*)norm, (const float*)loss_row, A, D, temperature, normalize ? 1 : 0, grad_scale, loss, dfeat);
    MBX_LAUNCH_CHECK("supcon_loss (gradient)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// 1-NN by cosine similarity (train_action_1shot.py:58-69).  A workgroup owns 32 test rows and streams the exemplars in tiles of 32
// and D in chunks of 32: both chunks lie transposed in LDS (odd stride, as above), thread (tt, ta) of 16 x 16 owns the dots of test
// rows tt, tt + 16 with exemplars ta, ta + 16 of the tile.  The staging thread of an element also adds its square, blocked like
// the dots, so the norms cost no second pass over the rows: a test row's once, an exemplar's once per workgroup and tile.
//     sim = (a . t) / (max(|a|, 1e-8) max(|t|, 1e-8))
// After a tile the 32 x 32 similarities go through LDS to one thread per test row, which scans them in exemplar order: a value
// replaces the best only if it is greater, or NaN while the best is not (torch.argmax: ties to the lowest index, the first NaN wins).
// ---------------------------------------------------------------------------------------------------------------
#define NN_T 32
#define NN_AP (NN_T + 1)

// column k of test rows t0 + r0 + 8 q and exemplars m0 + r0 + 8 q, zero outside the matrices
__device__ __forceinline__ void nn_fetch(const float* __restrict__ test, const float* __restrict__ anchors, int t0, int m0, int N, int M, int D,
                                         int k, int r0, float (&tv)[4], float (&av)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + 8 * q;
        tv[q] = (k < D && t0 + r < N) ? test[(size_t)(t0 + r) * D + k] : 0.f;
        av[q] = (k < D && m0 + r < M) ? anchors[(size_t)(m0 + r) * D + k] : 0.f;
    }
}

__global__ __launch_bounds__(256) void nn_cosine_kernel(const float* __restrict__ anchors, const int* __restrict__ anchor_labels, int M,
                                                        const float* __restrict__ test, const int* __restrict__ test_labels, int N, int D,
                                                        int* __restrict__ pred_label, float* __restrict__ best_sim,
                                                        unsigned long long* __restrict__ hits) {
    __shared__ float ts[OS_KC * NN_AP];
    __shared__ float as[OS_KC * NN_AP];
    __shared__ float sq[2][NN_T][NN_AP];      // partial squares [test | exemplar][row][k mod 32]; then the similarities of the tile
    __shared__ float tnorm[NN_T], anorm[NN_T];
    const int tid = threadIdx.x, tt = tid & 15, ta = tid >> 4;
    const int kk = tid & 31, r0 = tid >> 5;   // staging: column kk of rows r0 + 8 q
    const int t0 = blockIdx.x * NN_T;
    float best = 0.f;
    int best_idx = -1;                        // thread tid < 32: the running argmax of test row t0 + tid
    for (int m0 = 0; m0 < M; m0 += NN_T) {
        float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
        float tsq[4] = {0.f, 0.f, 0.f, 0.f}, asq[4] = {0.f, 0.f, 0.f, 0.f};
        // the chunk after the one being multiplied is already on its way from memory: its loads are issued before the products
        float tv[4], av[4];
        nn_fetch(test, anchors, t0, m0, N, M, D, kk, r0, tv, av);
        for (int k0 = 0; k0 < D; k0 += OS_KC) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 8 * q;
                ts[kk * NN_AP + r] = tv[q];
                as[kk * NN_AP + r] = av[q];
                tsq[q] = fmaf(tv[q], tv[q], tsq[q]);
                asq[q] = fmaf(av[q], av[q], asq[q]);
            }
            __syncthreads();
            if (k0 + OS_KC < D) nn_fetch(test, anchors, t0, m0, N, M, D, k0 + OS_KC + kk, r0, tv, av);
            float c[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll 8
            for (int k = 0; k < OS_KC; ++k) {
                const float x0 = ts[k * NN_AP + tt], x1 = ts[k * NN_AP + tt + 16];
                const float y0 = as[k * NN_AP + ta], y1 = as[k * NN_AP + ta + 16];
                c[0][0] = fmaf(x0, y0, c[0][0]); c[0][1] = fmaf(x0, y1, c[0][1]);
                c[1][0] = fmaf(x1, y0, c[1][0]); c[1][1] = fmaf(x1, y1, c[1][1]);
            }
            acc[0][0] += c[0][0]; acc[0][1] += c[0][1]; acc[1][0] += c[1][0]; acc[1][1] += c[1][1];
        }
        // norms: the 32 per-column partial sums of a row, added in column order
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sq[0][r0 + 8 * q][kk] = tsq[q];
            sq[1][r0 + 8 * q][kk] = asq[q];
        }
        __syncthreads();
        if (tid < 2 * NN_T) {
            const int which = tid >> 5, r = tid & 31;
            float s = 0.f;
            for (int k = 0; k < OS_KC; ++k) s += sq[which][r][k];
            (which ? anorm : tnorm)[r] = fmaxf(sqrtf(s), 1e-8f);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) sq[0][tt + 16 * u][ta + 16 * v] = acc[u][v] / (anorm[ta + 16 * v] * tnorm[tt + 16 * u]);
        __syncthreads();
        if (tid < NN_T) {
            const int lim = M - m0 < NN_T ? M - m0 : NN_T;
            for (int a = 0; a < lim; ++a) {
                const float v = sq[0][tid][a];
                if (best_idx < 0 || v > best || (v != v && best == best)) { best = v; best_idx = m0 + a; }
            }
        }
    }
    // wave 0: one lane per test row (lanes 32..63 and rows past N count nothing)
    if (tid < MBX_WAVE) {
        float hit = 0.f;
        const int t = t0 + tid;
        if (tid < NN_T && t < N) {
            const int lab = anchor_labels[best_idx];
            pred_label[t] = lab;
            if (best_sim) best_sim[t] = best;
            if (test_labels && test_labels[t] == lab) hit = 1.f;
        }
        if (test_labels) {
            const float n = wave_sum(hit);
            if (tid == 0 && n > 0.f) atomicAdd(hits, (unsigned long long)n);
        }
    }
}

extern "C" int mbx_nn_cosine(const float* anchors, const int* anchor_labels, int M, const float* test, const int* test_labels, int N, int D,
                             int* pred_label, float* best_sim, long long* hits, void* stream) {
    MBX_CHECK_ARG(N >= 0, "nn_cosine: bad test row count N=%d", N);
    MBX_CHECK_ARG(M >= 1 && D >= 1, "nn_cosine: bad shape M=%d D=%d (at least one exemplar, one feature)", M, D);
    if (N == 0) return 0;
    MBX_CHECK_ARG(anchors && anchor_labels && test && pred_label, "nn_cosine: null pointer");
    MBX_CHECK_ARG(!test_labels || hits, "nn_cosine: test labels without a hit counter");
    MBX_CHECK_ARG(N <= (1 << 30), "nn_cosine: too many test rows N=%d", N);
    hipLaunchKernelGGL(nn_cosine_kernel, dim3((N + NN_T - 1) / NN_T), dim3(256), 0, (hipStream_t)stream, anchors, anchor_labels, M, test,
                       test_labels, N, D, pred_label, best_sim, (unsigned long long*)hits);
    MBX_LAUNCH_CHECK("nn_cosine");
    return 0;
}
