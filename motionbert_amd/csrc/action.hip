// Action recognition around the backbone (train_action.py:55-61,172-188; lib/data/dataset_action.py:76-112,173-182;
// lib/utils/utils_data.py:7-29; lib/utils/learning.py:25-37).
//   mbx_action_input : NTURGBD.__getitem__ for a batch -- random_move followed by crop_scale -- in ONE launch.  A workgroup owns a whole
//                      sample: pass 1 moves every joint and reduces the bounding box of the joints with confidence != 0, pass 2 moves
//                      them again, normalises, clips and writes.  The moved coordinates are never stored: the second read of the
//                      sample (99 KB at [2,243,17,3]) is served by the L2 that the first one filled, and recomputing two fused
//                      multiply-adds per joint is cheaper than keeping 66 KB per workgroup resident.  ONE path for every size.
//                      The per-frame transform (two sincosf and four interpolations) is computed once per frame into an LDS table of
//                      AI_FRAMES frames; longer clips walk the table in chunks.
//   mbx_xent_topk    : CrossEntropyLoss() (mean), its gradient and the top-1 / top-5 hit counts in ONE launch of ONE workgroup, one wave per
//                      row in turn.  Every sum has a fixed order: two calls on the same input return the same bits.
#include "mbx_common.h"
#include "aug_rng.h"
#include <math.h>

#define AI_THREADS 1024
#define AI_WAVES (AI_THREADS / MBX_WAVE)
#define AI_FRAMES 512       // frames of the per-frame transform table (8 KB of LDS)
#define AI_NPARAM 9         // A0 A1 S0 S1 Tx0 Tx1 Ty0 Ty1 ratio

struct AiRanges { float lo[4], hi[4]; };     // angle (degrees), scale, translation, crop ratio

// the moved coordinates of one joint: x' = c x - s y + tx, y' = s x + c y + ty with c = cos(a) scale, s = sin(a) scale.  Explicit fused
// multiply-adds: both passes must produce the same bits (the bounding box of pass 1 is the box of what pass 2 normalises).
__device__ __forceinline__ void ai_move(const float4 f, float x, float y, float& xo, float& yo) {
    xo = fmaf(f.x, x, fmaf(-f.y, y, f.z));
    yo = fmaf(f.y, x, fmaf(f.x, y, f.w));
}

// frames [t0, t0 + tc) of the table: a_t = (A0 + (A1 - A0) f_t) pi / 180 with f_t = t / (T - 1) (np.linspace with the end point; 0 for
// T = 1), likewise s_t, tx_t, ty_t
__device__ __forceinline__ void ai_fill_table(float4* tab, const float* p, int t0, int tc, int T, bool move) {
    for (int tl = threadIdx.x; tl < tc; tl += AI_THREADS) {
        float4 f = make_float4(1.f, 0.f, 0.f, 0.f);
        if (move) {
            const float ft = T > 1 ? (float)(t0 + tl) / (float)(T - 1) : 0.f;
            const float a = fmaf(p[1] - p[0], ft, p[0]) * 0.017453292519943295f;
            const float s = fmaf(p[3] - p[2], ft, p[2]);
            float sn, cs;
            sincosf(a, &sn, &cs);
            f = make_float4(cs * s, sn * s, fmaf(p[5] - p[4], ft, p[4]), fmaf(p[7] - p[6], ft, p[6]));
        }
        tab[tl] = f;
    }
}

__global__ __launch_bounds__(AI_THREADS) void action_input_kernel(const float* __restrict__ x, float* __restrict__ y, int M, int T, int J,
                                                                  const float* __restrict__ params_in, float* __restrict__ params_out,
                                                                  AiRanges rg, int flags, uint32_t slo, uint32_t shi) {
    __shared__ float4 tab[AI_FRAMES];
    __shared__ float red[AI_WAVES][5];
    const int n = blockIdx.x, tid = threadIdx.x;
    const bool move = flags & 1, crop = flags & 2;
    // the nine draws of the sample: every thread forms them (nine hashes), thread 0 reports them
    float p[AI_NPARAM];
#pragma unroll
    for (int k = 0; k < AI_NPARAM; ++k) {
        const int r = k < 4 ? k >> 1 : k < 8 ? 2 : 3;        // angle, scale, translation x and y, crop
        p[k] = params_in ? params_in[(size_t)n * AI_NPARAM + k]
                         : fminf(fmaf(rg.hi[r] - rg.lo[r], aug_uniform(slo, shi, (uint32_t)k, (uint32_t)n), rg.lo[r]), rg.hi[r]);
    }
    if (params_out && tid == 0)
#pragma unroll
        for (int k = 0; k < AI_NPARAM; ++k) params_out[(size_t)n * AI_NPARAM + k] = p[k];
    const size_t base = (size_t)n * M * T * J * 3;
    const float* xs = x + base;
    float* ys = y + base;

    bool zero = false;
    float scale = 1.f, ox = 0.f, oy = 0.f;
    if (crop) {
        // pass 1: count (saturating at 4: only "< 4" is asked) and bounding box of the moved joints with confidence != 0
        float cnt = 0.f, xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        for (int t0 = 0; t0 < T; t0 += AI_FRAMES) {
            const int tc = T - t0 < AI_FRAMES ? T - t0 : AI_FRAMES;
            __syncthreads();                                       // the previous chunk's table has been read
            ai_fill_table(tab, p, t0, tc, T, move);
            __syncthreads();
            for (int m = 0; m < M; ++m) {
                const float* xm = xs + ((size_t)m * T + t0) * J * 3;
                for (int r = tid; r < tc * J; r += AI_THREADS) {
                    const float c = xm[(size_t)r * 3 + 2];
                    if (c != 0.f) {
                        float xo, yo;
                        ai_move(tab[r / J], xm[(size_t)r * 3], xm[(size_t)r * 3 + 1], xo, yo);
                        cnt = fminf(cnt + 1.f, 4.f);
                        xmin = fminf(xmin, xo); xmax = fmaxf(xmax, xo);
                        ymin = fminf(ymin, yo); ymax = fmaxf(ymax, yo);
                    }
                }
            }
        }
        cnt = wave_sum(cnt);
        xmin = wave_min(xmin); xmax = wave_max(xmax);
        ymin = wave_min(ymin); ymax = wave_max(ymax);
        if ((tid & 63) == 0) {
            float* r = red[tid >> 6];
            r[0] = cnt; r[1] = xmin; r[2] = xmax; r[3] = ymin; r[4] = ymax;
        }
        __syncthreads();
        cnt = red[0][0]; xmin = red[0][1]; xmax = red[0][2]; ymin = red[0][3]; ymax = red[0][4];
        for (int w = 1; w < AI_WAVES; ++w) {
            cnt += red[w][0];
            xmin = fminf(xmin, red[w][1]); xmax = fmaxf(xmax, red[w][2]);
            ymin = fminf(ymin, red[w][3]); ymax = fmaxf(ymax, red[w][4]);
        }
        scale = fmaxf(xmax - xmin, ymax - ymin) * p[8];
        zero = cnt < 4.f || scale == 0.f;                          // utils_data.py:14-15,22-23: the whole sample is 0
        ox = (xmin + xmax - scale) / 2;
        oy = (ymin + ymax - scale) / 2;
    }
    // pass 2: move again, normalise and clip (all three channels: np.clip of the whole array), write
    for (int t0 = 0; t0 < T; t0 += AI_FRAMES) {
        const int tc = T - t0 < AI_FRAMES ? T - t0 : AI_FRAMES;
        __syncthreads();
        ai_fill_table(tab, p, t0, tc, T, move);
        __syncthreads();
        for (int m = 0; m < M; ++m) {
            const size_t off = ((size_t)m * T + t0) * J * 3;
            for (int r = tid; r < tc * J; r += AI_THREADS) {
                float xo = 0.f, yo = 0.f, c = 0.f;
                if (!zero) {
                    c = xs[off + (size_t)r * 3 + 2];
                    ai_move(tab[r / J], xs[off + (size_t)r * 3], xs[off + (size_t)r * 3 + 1], xo, yo);
                    if (crop) {
                        xo = ((xo - ox) / scale - 0.5f) * 2;
                        yo = ((yo - oy) / scale - 0.5f) * 2;
                        xo = fminf(fmaxf(xo, -1.f), 1.f);
                        yo = fminf(fmaxf(yo, -1.f), 1.f);
                        c = fminf(fmaxf(c, -1.f), 1.f);
                    }
                }
                ys[off + (size_t)r * 3] = xo;
                ys[off + (size_t)r * 3 + 1] = yo;
                ys[off + (size_t)r * 3 + 2] = c;
            }
        }
    }
}

extern "C" int mbx_action_input(const float* x, float* y, int N, int M, int T, int J, const float* params_in, float* params_out,
                                float angle_lo, float angle_hi, float scale_lo, float scale_hi, float trans_lo, float trans_hi,
                                float crop_lo, float crop_hi, int flags, uint64_t seed, void* stream) {
    MBX_CHECK_ARG(x && y, "action_input: null pointer");
    MBX_CHECK_ARG(N >= 1 && M >= 1 && T >= 1 && J >= 1 && J <= 32, "action_input: bad shape N=%d M=%d T=%d J=%d (all >= 1, J <= 32)", N, M, T, J);
    MBX_CHECK_ARG((long long)M * T * J <= (1ll << 28), "action_input: a sample of %lld joints is too large", (long long)M * T * J);
    MBX_CHECK_ARG((flags & ~3) == 0, "action_input: unknown flags %d (bit 0 move, bit 1 crop)", flags);
    MBX_CHECK_ARG(angle_lo <= angle_hi && scale_lo <= scale_hi && trans_lo <= trans_hi && crop_lo <= crop_hi,
                  "action_input: a range has lo > hi (angle %g..%g scale %g..%g translation %g..%g crop %g..%g)", (double)angle_lo,
                  (double)angle_hi, (double)scale_lo, (double)scale_hi, (double)trans_lo, (double)trans_hi, (double)crop_lo, (double)crop_hi);
    const AiRanges rg = {{angle_lo, scale_lo, trans_lo, crop_lo}, {angle_hi, scale_hi, trans_hi, crop_hi}};
    hipLaunchKernelGGL(action_input_kernel, dim3(N), dim3(AI_THREADS), 0, (hipStream_t)stream, x, y, M, T, J, params_in, params_out, rg, flags,
                       (uint32_t)seed, (uint32_t)(seed >> 32));
    MBX_LAUNCH_CHECK("action_input");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// cross-entropy, gradient and top-k hits.  Wave w of the one workgroup owns rows w, w + 16, ...; lane l the columns l, l + 64, ...
//   m = max_j z_j;  rank = #{j : z_j > z_y} + #{j < y : z_j == z_y};  s = sum_j exp(z_j - m);  loss = log s - (z_y - m)
//   dlogits_j = (exp(z_j - m) / s - [j == y]) grad_scale / N
// The row losses of a wave are added in row order in fp64, the 16 wave sums in wave order: the mean carries the rounding of the row
// losses and one conversion.  A label outside [0, C) is never used as an index: the row's loss and gradient are NaN and it counts no hit.
// ---------------------------------------------------------------------------------------------------------------
#define XE_THREADS 1024
#define XE_WAVES (XE_THREADS / MBX_WAVE)

__global__ __launch_bounds__(XE_THREADS) void xent_topk_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int N, int C,
                                                               float gscale, float* __restrict__ values, float* __restrict__ dlogits,
                                                               double* __restrict__ acc) {
    __shared__ double wsum[XE_WAVES];
    __shared__ float whit[XE_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double lsum = 0.0;
    float hit1 = 0.f, hit5 = 0.f;
    const float gn = gscale / (float)N;
    for (int row = wave; row < N; row += XE_WAVES) {                // uniform over the wave: every lane is active in the reductions
        const float* z = logits + (size_t)row * C;
        const int yl = labels[row];
        const bool ok = yl >= 0 && yl < C;
        const float zy = ok ? z[yl] : 0.f;
        float m = -INFINITY, above = 0.f;
        for (int j = lane; j < C; j += MBX_WAVE) {
            const float v = z[j];
            m = fmaxf(m, v);
            above += (v > zy || (v == zy && j < yl)) ? 1.f : 0.f;  // counts of at most 4096: exact in fp32
        }
        m = wave_max(m);
        const float rank = wave_sum(above);
        float s = 0.f;
        for (int j = lane; j < C; j += MBX_WAVE) s += expf(z[j] - m);
        s = wave_sum(s);
        const float loss = ok ? logf(s) - (zy - m) : NAN;
        lsum += (double)loss;
        if (ok && rank < 1.f) hit1 += 1.f;
        if (ok && rank < 5.f) hit5 += 1.f;
        if (dlogits) {
            float* d = dlogits + (size_t)row * C;
            for (int j = lane; j < C; j += MBX_WAVE) d[j] = ok ? (expf(z[j] - m) / s - (j == yl ? 1.f : 0.f)) * gn : NAN;
        }
    }
    if (lane == 0) { wsum[wave] = lsum; whit[wave][0] = hit1; whit[wave][1] = hit5; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        float h1 = 0.f, h5 = 0.f;
        for (int w = 0; w < XE_WAVES; ++w) { tot += wsum[w]; h1 += whit[w][0]; h5 += whit[w][1]; }
        values[0] = (float)(tot / (double)N);
        values[1] = h1;
        values[2] = h5;
        if (acc) { acc[0] += tot; acc[1] += (double)h1; acc[2] += (double)h5; acc[3] += (double)N; }
    }
}

extern "C" int mbx_xent_topk(const float* logits, const int* labels, int N, int C, float grad_scale, float* values, float* dlogits,
                             double* acc, void* stream) {
    MBX_CHECK_ARG(logits && labels && values, "xent_topk: null pointer");
    MBX_CHECK_ARG(N >= 1 && N <= 65536 && C >= 1 && C <= 4096, "xent_topk: bad shape N=%d C=%d (1 <= N <= 65536, 1 <= C <= 4096)", N, C);
    hipLaunchKernelGGL(xent_topk_kernel, dim3(1), dim3(XE_THREADS), 0, (hipStream_t)stream, logits, labels, N, C, grad_scale, values, dlogits,
                       acc);
    MBX_LAUNCH_CHECK("xent_topk");
    return 0;
}
