// the input stage of training / evaluation on the device.
//   mbx_augment2d     lib/data/augmentation.py:29-81 (Augmenter2D.add_noise + add_mask, the masked-reconstruction input of
//                     pre-training, train.py:171-172) as ONE kernel: per-keyframe mixture noise, 27 -> T linear interpolation
//                     (F.interpolate trilinear / align_corners over an axis-aligned volume is linear along time), per-frame
//                     jitter, distance -> confidence synthesis, joint and frame masks.  The reference builds eight random
//                     tensors on the HOST and copies them over, then runs ~25 element-wise kernels.
//   mbx_embed_fwd_tta + mbx_flip_average   flip test-time augmentation (train.py:67-72, infer_wild.py:75-80,
//                     lib/utils/utils_data.py:54-66): the flipped half of the batch is an index remap inside the embedding
//                     kernel and the flip-back + average is one pass over the [2B,T,J,3] output -- no deep copies.
// Random numbers are counter-based: u(stream, index) = hash(seed, stream, index) -- a value depends only on WHICH number it is,
// so the torch restatement in oracle/augment_oracle.py reproduces every draw.
#include "mbx_common.h"
#include "aug2d_point.h"

// the per-point body (and the stream table of the random numbers) is aug2d_point.h: mbx_motion2d_input calls the same function
__global__ __launch_bounds__(256) void augment2d_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int T, int J, int Cin,
                                                        const float* __restrict__ nmean, const float* __restrict__ nstd,
                                                        const float* __restrict__ nweight, float urange, float jitter_std, float a,
                                                        float b, float m, float s, float mask_ratio, float mask_T_ratio, int flags,
                                                        uint32_t slo, uint32_t shi) {
    const Aug2dArgs A = {nmean, nstd, nweight, urange, jitter_std, a, b, m, s, mask_ratio, mask_T_ratio, flags};
    const size_t total = (size_t)B * T * J;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int j = (int)(i % J), t = (int)((i / J) % T), bb = (int)(i / ((size_t)J * T));
        float px = x[i * Cin], py = x[i * Cin + 1], conf = Cin > 2 ? x[i * Cin + 2] : 1.0f;
        aug2d_point(A, slo, shi, T, J, bb, t, j, px, py, conf);
        y[i * 3] = px; y[i * 3 + 1] = py; y[i * 3 + 2] = conf;
    }
}
extern "C" int mbx_augment2d(const float* x, float* y, int B, int T, int J, int Cin, const float* noise_mean, const float* noise_std,
                             const float* noise_weight, float uniform_range, float jitter_std, float d2c_a, float d2c_b, float d2c_m,
                             float d2c_s, float mask_ratio, float mask_T_ratio, int flags, uint64_t seed, void* stream) {
    MBX_CHECK_ARG(x && y, "augment2d: null pointer");
    MBX_CHECK_ARG(B > 0 && T > 0 && J > 0 && (Cin == 2 || Cin == 3), "augment2d: bad shape (input channels must be 2 or 3)");
    MBX_CHECK_ARG(!(flags & 1) || (noise_mean && noise_std && noise_weight), "augment2d: noise needs mean / std / weight");
    MBX_CHECK_ARG((size_t)B * T * J < ((size_t)1 << 32), "augment2d: too many joints for 32-bit counters");
    const size_t want = ((size_t)B * T * J + 255) / 256;
    const int grid = (int)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(augment2d_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, y, B, T, J, Cin, noise_mean, noise_std,
                       noise_weight, uniform_range, jitter_std, d2c_a, d2c_b, d2c_m, d2c_s, mask_ratio, mask_T_ratio, flags,
                       (uint32_t)seed, (uint32_t)(seed >> 32));
    MBX_LAUNCH_CHECK("augment2d");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// flip test-time augmentation.  h for 2B samples from x [B,T,J,Din]: sample B + b is flip_data(x[b]) (utils_data.py:54-66):
// joint j takes the values of joint perm[j] (left <-> right) with the horizontal coordinate (channel 0) negated.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_fwd_tta_kernel(const float* __restrict__ x, const int* __restrict__ perm,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            const float* __restrict__ pos, const float* __restrict__ temp,
                                                            float* __restrict__ h, int Bsrc, int T, int J, int Din, int C) {
    const int c4n = C >> 2;
    const size_t total = (size_t)2 * Bsrc * T * J * c4n;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t mo = idx / c4n;
        const int c = (int)(idx % c4n) * 4;
        const int j = (int)(mo % J), t = (int)((mo / J) % T), b2 = (int)(mo / ((size_t)J * T));
        const bool flip = b2 >= Bsrc;
        const size_t ms = ((size_t)(flip ? b2 - Bsrc : b2) * T + t) * J + (flip ? perm[j] : j);
        const float4 bb = *reinterpret_cast<const float4*>(b + c);
        const float4 pp = *reinterpret_cast<const float4*>(pos + (size_t)j * C + c);
        const float4 tt = *reinterpret_cast<const float4*>(temp + (size_t)t * C + c);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int k = 0; k < Din; ++k) {
            float xv = x[ms * Din + k];
            if (flip && k == 0) xv = -xv;
            a0 = fmaf(xv, w[(size_t)(c + 0) * Din + k], a0);
            a1 = fmaf(xv, w[(size_t)(c + 1) * Din + k], a1);
            a2 = fmaf(xv, w[(size_t)(c + 2) * Din + k], a2);
            a3 = fmaf(xv, w[(size_t)(c + 3) * Din + k], a3);
        }
        *reinterpret_cast<float4*>(h + mo * C + c) =
            make_float4(((a0 + bb.x) + pp.x) + tt.x, ((a1 + bb.y) + pp.y) + tt.y, ((a2 + bb.z) + pp.z) + tt.z, ((a3 + bb.w) + pp.w) + tt.w);
    }
}
extern "C" int mbx_embed_fwd_tta(const float* x, const int* perm, const float* w, const float* b, const float* pos, const float* temp,
                                 float* h, int B, int T, int J, int Din, int C, void* stream) {
    MBX_CHECK_ARG(x && perm && w && b && pos && temp && h, "embed_fwd_tta: null pointer");
    MBX_CHECK_ARG(B > 0 && T > 0 && J > 0 && Din > 0 && C > 0 && C % 4 == 0, "embed_fwd_tta: bad shape (C %% 4 != 0?)");
    const size_t want = ((size_t)2 * B * T * J * (C / 4) + 255) / 256;
    const int grid = (int)(want < 256 * 16 ? want : 256 * 16);
    hipLaunchKernelGGL(embed_fwd_tta_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, perm, w, b, pos, temp, h, B, T, J, Din, C);
    MBX_LAUNCH_CHECK("embed_fwd_tta");
    return 0;
}
// out[b,t,j,:] = (o[b,t,j,:] + flip_back(o[B+b])[t,j,:]) / 2   (train.py:70-72)
__global__ __launch_bounds__(256) void flip_average_kernel(const float* __restrict__ o2, const int* __restrict__ perm, float* __restrict__ out,
                                                           int B, int T, int J, int D) {
    const size_t total = (size_t)B * T * J * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % D), j = (int)((i / D) % J);
        const size_t bt = i / ((size_t)D * J);
        const float f = o2[(((size_t)B * T + bt) * J + perm[j]) * D + d];
        out[i] = 0.5f * (o2[i] + (d == 0 ? -f : f));
    }
}
extern "C" int mbx_flip_average(const float* out2, const int* perm, float* out, int B, int T, int J, int D, void* stream) {
    MBX_CHECK_ARG(out2 && perm && out && B > 0 && T > 0 && J > 0 && D > 0, "flip_average: bad arguments");
    const size_t want = ((size_t)B * T * J * D + 255) / 256;
    const int grid = (int)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(flip_average_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out2, perm, out, B, T, J, D);
    MBX_LAUNCH_CHECK("flip_average");
    return 0;
}
