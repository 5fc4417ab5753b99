// The per-point body of Augmenter2D.augment2D (lib/data/augmentation.py:29-81) as ONE device function, shared by mbx_augment2d
// (augment.hip: a batch already in its final form) and mbx_motion2d_input (motion2d.hip: the 2D data sets' per-clip stage and the
// augmentation in one launch).  Both kernels call it with the same (seed, sample, frame, joint) and so write the same bits.
#pragma once
#include "aug_rng.h"

// standard normal: Box-Muller on two uniforms of the streams (stream, stream + 1)
__device__ __forceinline__ float aug_normal(uint32_t slo, uint32_t shi, uint32_t stream, uint32_t idx) {
    const float u1 = aug_uniform(slo, shi, stream, idx), u2 = aug_uniform(slo, shi, stream + 1, idx);
    return sqrtf(-2.0f * logf(u1 + (1.0f / 33554432.0f))) * cosf(6.28318530717958647692f * u2);
}
// streams: 0 sel, 1-2 gaussian x, 3-4 gaussian y, 5 uniform x, 6 uniform y, 7-8 jitter x, 9-10 jitter y, 11-12 confidence shift,
//          13 joint mask, 14 frame mask;  16 crop ratio and 17 flip of mbx_motion2d_input (one draw per sample)
#define AUG_K 27
#define AUG_STREAM_RATIO 16
#define AUG_STREAM_FLIP 17

struct Aug2dArgs {
    const float *nmean, *nstd, *nweight;      // [J,2], [J,2], [J]; read only with flag bit 0
    float urange, jitter_std, a, b, m, s, mask_ratio, mask_T_ratio;
    int flags;                                // bit 0 add_noise, bit 1 add_mask
};

// point (bb, t, j) of a batch [B,T,J]: (px, py, conf) in, the augmented point out
__device__ __forceinline__ void aug2d_point(const Aug2dArgs& A, uint32_t slo, uint32_t shi, int T, int J, int bb, int t, int j, float& px,
                                            float& py, float& conf) {
    const size_t i = ((size_t)bb * T + t) * J + j;
    if (A.flags & 1) {          // add_noise (augmentation.py:29-66)
        // key-frame position of frame t: align_corners = True
        const float pos = T > 1 ? (float)t * (float)(AUG_K - 1) / (float)(T - 1) : 0.f;
        int k0 = (int)floorf(pos);
        if (k0 > AUG_K - 2) k0 = AUG_K - 2;
        const float wgt = pos - (float)k0;
        float d[2] = {0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint32_t ki = (uint32_t)((bb * AUG_K + k0 + kk) * J + j);
            const bool gauss = aug_uniform(slo, shi, 0, ki) < A.nweight[j];
            const float gx = aug_normal(slo, shi, 1, ki) * A.nstd[j * 2] + A.nmean[j * 2];
            const float gy = aug_normal(slo, shi, 3, ki) * A.nstd[j * 2 + 1] + A.nmean[j * 2 + 1];
            const float ux = (aug_uniform(slo, shi, 5, ki) - 0.5f) * A.urange, uy = (aug_uniform(slo, shi, 6, ki) - 0.5f) * A.urange;
            const float wk = kk == 0 ? 1.0f - wgt : wgt;
            d[0] += wk * (gauss ? gx : ux);
            d[1] += wk * (gauss ? gy : uy);
        }
        const uint32_t ti = (uint32_t)(t * J + j);                 // jitter: shared by the whole batch (augmentation.py:47)
        d[0] += aug_normal(slo, shi, 7, ti) * A.jitter_std;
        d[1] += aug_normal(slo, shi, 9, ti) * A.jitter_std;
        px += d[0];
        py += d[1];
        const float dis = sqrtf(d[0] * d[0] + d[1] * d[1]);
        conf = A.a / (dis + A.a) + A.b * dis + aug_normal(slo, shi, 11, (uint32_t)i) * A.s + A.m;   // dis2conf (augmentation.py:22-27)
        conf = fminf(fmaxf(conf, 0.f), 1.f);
    }
    if (A.flags & 2) {          // add_mask (augmentation.py:67-74): x * (rand > mask_ratio) * (rand_T > mask_T_ratio)
        const bool keep = aug_uniform(slo, shi, 13, (uint32_t)i) > A.mask_ratio && aug_uniform(slo, shi, 14, (uint32_t)t) > A.mask_T_ratio;
        if (!keep) { px = 0.f; py = 0.f; conf = 0.f; }
    }
}
