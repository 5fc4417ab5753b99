// The 2D half of pre-training (lib/data/dataset_motion_2d.py:116-147; train.py:162-172; lib/utils/utils_data.py:7-29,54-66).
//   mbx_motion2d_input : InstaVDataset2D.__getitem__ -- crop_scale with a random ratio, zeroing of the unseen joints, a random flip -- and
//                        the no_grad block of train_epoch for a 2D batch -- the confidence before augmentation, the root-relative target,
//                        Augmenter2D.augment2D -- in ONE launch, one workgroup per sample.  Between the host copy and the embedding the
//                        same result costs a crop-only mbx_action_input, a where, flip_batch (index_select, clone, negation, where), the
//                        root subtraction and mbx_augment2d, for clips of 6 KB (T = 30) and 16 KB (T = 81).
// Two paths, one per-joint code (m2d_joint).  A sample of at most M2D_RESIDENT joints is read from HBM once into LDS (18 KB); the box pass
// and the write pass read it there, and so does the flip, whose left / right permutation reads OTHER joints of the frame.  A larger sample
// is read twice, the second time from the L2 that the first read filled, as action_input_kernel does.  The crop has the operations of
// action_input_kernel's crop in the same order: the bits are the same.  The root joint that a joint's target needs is recomputed from the
// source (the flip maps joint 0 to itself), not stored: no third pass, no barrier between the joints of a frame.
#include "mbx_common.h"
#include "aug2d_point.h"
#include <math.h>

#define M2D_THREADS 256        // 510 (T = 30) to 1377 (T = 81) joints per sample: two to six per thread
#define M2D_WAVES (M2D_THREADS / MBX_WAVE)
#define M2D_RESIDENT MBX_MOTION2D_RESIDENT      // (mbx.h: 1536) joints (T J) of a sample kept in LDS: 3 floats each, 18 KB; covers T = 81, J = 17

enum { M2D_CROP = 1, M2D_ZERO = 2, M2D_FLIP = 4, M2D_NOISE = 8, M2D_MASK = 16, M2D_ROOTREL = 32, M2D_ALL = 63 };

// flip_data's joint table (utils_data.py:60-61, the 17-joint H36M layout): left 4 5 6 11 12 13 <-> right 1 2 3 14 15 16
__device__ __forceinline__ int m2d_flip_joint(int j) {
    return ((j >= 1 && j <= 3) || (j >= 11 && j <= 13)) ? j + 3 : ((j >= 4 && j <= 6) || (j >= 14 && j <= 16)) ? j - 3 : j;
}

struct M2dXf {
    float ox, oy, scale;
    bool zero, crop, unseen, flip;
};
// joint r (an index into the SOURCE sample, after the flip's permutation) of the data set's item: crop, clip, zeroing, negation
__device__ __forceinline__ void m2d_joint(const float* src, int r, const M2dXf& f, float& xo, float& yo, float& c) {
    xo = 0.f; yo = 0.f; c = 0.f;
    if (!f.zero) {
        xo = src[(size_t)r * 3]; yo = src[(size_t)r * 3 + 1]; c = src[(size_t)r * 3 + 2];
        if (f.crop) {
            xo = ((xo - f.ox) / f.scale - 0.5f) * 2;
            yo = ((yo - f.oy) / f.scale - 0.5f) * 2;
            xo = fminf(fmaxf(xo, -1.f), 1.f);
            yo = fminf(fmaxf(yo, -1.f), 1.f);
            c = fminf(fmaxf(c, -1.f), 1.f);
        }
        if (f.unseen && c == 0.f) { xo = 0.f; yo = 0.f; }          // motion_2d[motion_2d[:,:,2]==0] = 0 (dataset_motion_2d.py:143)
    }
    if (f.flip) xo = -xo;
}

template <bool RES>
__global__ __launch_bounds__(M2D_THREADS) void motion2d_input_kernel(const float* __restrict__ x, float* __restrict__ data, float* __restrict__ gt,
                                                                     float* __restrict__ conf, float* __restrict__ x_aug, int T, int J,
                                                                     const float* params_in, float* params_out, float rlo, float rhi,
                                                                     float flip_prob, Aug2dArgs A, int flags, uint32_t slo, uint32_t shi) {
    __shared__ float buf[RES ? M2D_RESIDENT * 3 : 1];
    __shared__ float red[M2D_WAVES][5];
    const int n = blockIdx.x, tid = threadIdx.x, TJ = T * J;
    const size_t base = (size_t)n * TJ * 3;
    const float* xs = x + base;
    // the two draws of the sample: every thread forms them, thread 0 reports them (after the barrier: params_out may be params_in)
    const float ratio = params_in ? params_in[(size_t)n * 2] : fminf(fmaf(rhi - rlo, aug_uniform(slo, shi, AUG_STREAM_RATIO, (uint32_t)n), rlo), rhi);
    const float uflip = params_in ? params_in[(size_t)n * 2 + 1] : aug_uniform(slo, shi, AUG_STREAM_FLIP, (uint32_t)n);
    if (RES)
        for (int k = tid; k < TJ * 3; k += M2D_THREADS) buf[k] = xs[k];
    __syncthreads();
    if (params_out && tid == 0) { params_out[(size_t)n * 2] = ratio; params_out[(size_t)n * 2 + 1] = uflip; }
    const float* src = RES ? buf : xs;

    M2dXf f;
    f.crop = flags & M2D_CROP; f.unseen = flags & M2D_ZERO; f.flip = (flags & M2D_FLIP) && uflip < flip_prob;
    f.zero = false; f.scale = 1.f; f.ox = 0.f; f.oy = 0.f;
    if (f.crop) {
        // pass 1: count (saturating at 4: only "< 4" is asked) and bounding box of the joints with confidence != 0
        float cnt = 0.f, xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        for (int r = tid; r < TJ; r += M2D_THREADS) {
            if (src[(size_t)r * 3 + 2] != 0.f) {
                const float xo = src[(size_t)r * 3], yo = src[(size_t)r * 3 + 1];
                cnt = fminf(cnt + 1.f, 4.f);
                xmin = fminf(xmin, xo); xmax = fmaxf(xmax, xo);
                ymin = fminf(ymin, yo); ymax = fmaxf(ymax, yo);
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
        for (int w = 1; w < M2D_WAVES; ++w) {
            cnt += red[w][0];
            xmin = fminf(xmin, red[w][1]); xmax = fmaxf(xmax, red[w][2]);
            ymin = fminf(ymin, red[w][3]); ymax = fmaxf(ymax, red[w][4]);
        }
        f.scale = fmaxf(xmax - xmin, ymax - ymin) * ratio;
        f.zero = cnt < 4.f || f.scale == 0.f;                     // utils_data.py:14-15,22-23: the whole sample is 0
        f.ox = (xmin + xmax - f.scale) / 2;
        f.oy = (ymin + ymax - f.scale) / 2;
    }
    // pass 2: the item, and from it the target, the confidence and the augmented input
    const bool rootrel = flags & M2D_ROOTREL;
    float x00, y00, c00 = 0.f;
    if (gt && !rootrel) m2d_joint(src, 0, f, x00, y00, c00);     // data[n,0,0,2] (train.py:170)
    for (int r = tid; r < TJ; r += M2D_THREADS) {
        const int t = r / J, j = r - t * J;
        float px, py, c;
        m2d_joint(src, f.flip ? t * J + m2d_flip_joint(j) : r, f, px, py, c);
        const size_t o = base + (size_t)r * 3;
        if (data) { data[o] = px; data[o + 1] = py; data[o + 2] = c; }
        if (gt) {
            float gx = px, gy = py, gc = c - c00;
            if (rootrel) {                                        // batch_gt - batch_gt[:, :, 0:1, :] (train.py:168): all three channels
                float rx, ry, rc;
                m2d_joint(src, t * J, f, rx, ry, rc);
                gx = px - rx; gy = py - ry; gc = c - rc;
            }
            gt[o] = gx; gt[o + 1] = gy; gt[o + 2] = gc;
        }
        if (conf) conf[(size_t)n * TJ + r] = c;
        if (x_aug) {
            aug2d_point(A, slo, shi, T, J, n, t, j, px, py, c);
            x_aug[o] = px; x_aug[o + 1] = py; x_aug[o + 2] = c;
        }
    }
}

static bool m2d_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + bbytes && b0 < a0 + abytes;
}

extern "C" int mbx_motion2d_input(const float* x, float* data, float* gt, float* conf, float* x_aug, int N, int T, int J,
                                  const float* params_in, float* params_out, float ratio_lo, float ratio_hi, float flip_prob,
                                  const float* noise_mean, const float* noise_std, const float* noise_weight, float uniform_range,
                                  float jitter_std, float d2c_a, float d2c_b, float d2c_m, float d2c_s, float mask_ratio,
                                  float mask_T_ratio, int flags, uint64_t seed, void* stream) {
    MBX_CHECK_ARG(x, "motion2d_input: null input");
    MBX_CHECK_ARG(data || gt || conf || x_aug, "motion2d_input: no output (data, gt, conf and x_aug are all null)");
    MBX_CHECK_ARG(N >= 1 && T >= 1 && J >= 1 && J <= 32, "motion2d_input: bad shape N=%d T=%d J=%d (all >= 1, J <= 32)", N, T, J);
    MBX_CHECK_ARG((flags & ~M2D_ALL) == 0, "motion2d_input: unknown flags %d (bits: 0 crop, 1 zero unseen, 2 flip, 3 noise, 4 mask, 5 rootrel)", flags);
    MBX_CHECK_ARG(ratio_lo <= ratio_hi, "motion2d_input: the crop range has lo > hi (%g..%g)", (double)ratio_lo, (double)ratio_hi);
    MBX_CHECK_ARG(flip_prob >= 0.f && flip_prob <= 1.f, "motion2d_input: flip_prob %g is not in [0, 1]", (double)flip_prob);
    MBX_CHECK_ARG(!(flags & M2D_FLIP) || J == 17, "motion2d_input: the flip uses the 17-joint left / right table, J = %d", J);
    MBX_CHECK_ARG(!(flags & M2D_NOISE) || (noise_mean && noise_std && noise_weight), "motion2d_input: noise needs mean / std / weight");
    MBX_CHECK_ARG((size_t)N * T * J < ((size_t)1 << 32), "motion2d_input: too many joints for 32-bit counters");
    MBX_CHECK_ARG((long long)T * J <= (1ll << 28), "motion2d_input: a sample of %lld joints is too large", (long long)T * J);
    const size_t bytes = (size_t)N * T * J * 3 * sizeof(float);
    MBX_CHECK_ARG(!m2d_overlap(x, bytes, data, bytes) && !m2d_overlap(x, bytes, gt, bytes) && !m2d_overlap(x, bytes, conf, bytes / 3) &&
                      !m2d_overlap(x, bytes, x_aug, bytes),
                  "motion2d_input: an output overlaps x (the flip reads other joints of the frame: no output may alias the input)");
    const Aug2dArgs A = {noise_mean, noise_std, noise_weight, uniform_range, jitter_std, d2c_a, d2c_b, d2c_m, d2c_s, mask_ratio, mask_T_ratio,
                         (flags & M2D_NOISE ? 1 : 0) | (flags & M2D_MASK ? 2 : 0)};
    if (T * J <= M2D_RESIDENT)
        hipLaunchKernelGGL(motion2d_input_kernel<true>, dim3(N), dim3(M2D_THREADS), 0, (hipStream_t)stream, x, data, gt, conf, x_aug, T, J,
                           params_in, params_out, ratio_lo, ratio_hi, flip_prob, A, flags, (uint32_t)seed, (uint32_t)(seed >> 32));
    else
        hipLaunchKernelGGL(motion2d_input_kernel<false>, dim3(N), dim3(M2D_THREADS), 0, (hipStream_t)stream, x, data, gt, conf, x_aug, T, J,
                           params_in, params_out, ratio_lo, ratio_hi, flip_prob, A, flags, (uint32_t)seed, (uint32_t)(seed >> 32));
    MBX_LAUNCH_CHECK("motion2d_input");
    return 0;
}
