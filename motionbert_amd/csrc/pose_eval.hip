// H36M evaluation on the device (train.py:56-153; lib/model/loss.py:8-51; lib/data/datareader_h36m.py:125-136).
//   mbx_pose_errors : per frame, Protocol #1 (MPJPE) and Protocol #2 (MPJPE after the optimal similarity alignment) of the raw
//                     network output against the dataset's joints_2.5d_image, with the reference's preparation (root-relative
//                     output, 2D ground truth, denormalisation, 2.5D factor, root subtraction) folded in.  fp64 after the loads.
//   mbx_eval_reduce : mean over the clips that cover a test frame, mean over the frames of an action, mean over the actions,
//                     in a fixed summation order (no floating-point atomics): two runs give the same bits.
#include "mbx_common.h"
#include "pose_solve.h"

// ---------------------------------------------------------------------------------------------------------------
// pose errors.  A workgroup is ONE wave and owns 64 consecutive frames.  Their 64 * 3J floats of pred and of gt are one
// contiguous run of memory: the wave copies both runs to LDS with 16-byte loads (consecutive lanes, consecutive vectors), and
// from there lane l owns frame l.  The LDS row of a frame is 3J | 1 words long: an odd stride, so the 64 lanes of a
// "joint j, channel c" read fall on 64 different banks.  The run of a workgroup need not start on a 16-byte boundary (a batch
// of clips cut out of a larger buffer): vectors are taken from the aligned address below the run and the elements outside
// the run are left out; a vector that is not entirely inside the run is loaded element by element.
//
// Procrustes step (loss.py:23-51; X = gt, Y = pred): X0 = X - muX, Y0 = Y - muY, H = X0^T Y0 / (|X0| |Y0|) = U S V^T,
// R = V U^T with the last column of V flipped when det R < 0, a = (s0 + s1 +- s2) |X0| / |Y0|, aligned = a Y R + muX - a muY R,
// so that  aligned_j - X_j = a (Y_j - muY) R - (X_j - muX).
// V comes from 8 cyclic Jacobi sweeps on H^T H (a fixed count: no data-dependent loop, terminates on NaN); the two leading
// right vectors give u_i = H v_i / s_i; the third pair is v2 = v0 x v1, u2 = u0 x u1.  With both triples right-handed
// R = sum_i v_i u_i^T has det +1 -- the reference's matrix after its flip -- and the signed third singular value is
// u2 . H v2 (= det-sign * s2, and 0 for a planar pose, whose third vectors a division could not give).
// A frame whose pred or gt has zero extent divides 0 by 0 as the reference does: e2 is NaN there.  Every other pair of finite poses
// gives a finite e2, a pose on a line and J = 2 (H of rank one) included; pose_solve.h states the accuracy below s1 / s0 = 1e-3.
// ---------------------------------------------------------------------------------------------------------------
#define PE_FRAMES 64

// copy the run [beg, end) (element indices into src) to LDS rows of `stride` words, 3J elements per row
__device__ __forceinline__ void pe_stage(const float* __restrict__ src, const float* __restrict__ x2d, int xs, long long beg, long long end,
                                         int row, int stride, float* __restrict__ dst, int lane) {
    const int mis = (int)(((uintptr_t)(src + beg) >> 2) & 3);      // elements past the 16-byte boundary below the run
    const long long vbeg = beg - mis;
    const int nvec = (int)((end - vbeg + 3) >> 2);
    for (int v = lane; v < nvec; v += PE_FRAMES) {
        const long long e0 = vbeg + 4ll * v;
        float w[4];
        if (e0 >= beg && e0 + 4 <= end) {
            const float4 q = *reinterpret_cast<const float4*>(src + e0);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (e0 + k >= beg && e0 + k < end) ? src[e0 + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long e = e0 + k;
            if (e < beg || e >= end) continue;
            const int rel = (int)(e - beg);
            const int f = rel / row, r = rel - f * row;
            float val = w[k];
            if (x2d) {                                  // gt_2d: x and y of the prediction are the model input's (train.py:80-81)
                const int c = r % 3;
                if (c < 2) val = x2d[(e / 3) * xs + c];
            }
            dst[f * stride + r] = val;
        }
    }
}

__global__ __launch_bounds__(PE_FRAMES) void pose_errors_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const float* __restrict__ hw, const float* __restrict__ factor,
                                                                const float* __restrict__ x2d, int xs, int rootrel,
                                                                double* __restrict__ e1, double* __restrict__ e2, long long frames, int T,
                                                                int J) {
    extern __shared__ float pe_lds[];
    const int lane = threadIdx.x;
    const int row = 3 * J, stride = row | 1;
    float* lp = pe_lds;
    float* lg = pe_lds + PE_FRAMES * stride;
    const long long f0 = (long long)blockIdx.x * PE_FRAMES;
    const long long f1 = f0 + PE_FRAMES < frames ? f0 + PE_FRAMES : frames;
    pe_stage(pred, x2d, xs, f0 * row, f1 * row, row, stride, lp, lane);
    pe_stage(gt, nullptr, 0, f0 * row, f1 * row, row, stride, lg, lane);
    __syncthreads();
    const long long frame = f0 + lane;
    if (frame >= f1) return;
    const float* mp = lp + lane * stride;
    const float* mg = lg + lane * stride;

    // pred -> millimetres: p = (p + off) * sc (datareader_h36m.py:134-135 and the 2.5D factor, train.py:118-121)
    double sx = 1.0, sz = 1.0, oy = 0.0, ox = 0.0;
    if (hw) {
        const double w = (double)hw[(frame / T) * 2], h = (double)hw[(frame / T) * 2 + 1];
        sx = sz = w * 0.5;
        ox = 1.0;
        oy = h / w;
    }
    const double fac = factor ? (double)factor[frame] : 1.0;
    const bool keep_xy0 = !rootrel || x2d != nullptr;      // train.py:75-76, then :80-81 writes x, y of joint 0 again
    const bool keep_z0 = !rootrel;
#define PE_PRED(j, px, py, pz)                                                      \
    {                                                                               \
        double rx = (double)mp[3 * (j)], ry = (double)mp[3 * (j) + 1], rz = (double)mp[3 * (j) + 2]; \
        if ((j) == 0) { rx = keep_xy0 ? rx : 0.0; ry = keep_xy0 ? ry : 0.0; rz = keep_z0 ? rz : 0.0; } \
        if (hw) { rx = (rx + ox) * sx; ry = (ry + oy) * sx; rz = rz * sz; }          \
        if (factor) { rx *= fac; ry *= fac; rz *= fac; }                            \
        px = rx; py = ry; pz = rz;                                                  \
    }
    double p0x, p0y, p0z;
    PE_PRED(0, p0x, p0y, p0z);
    const double g0x = (double)mg[0], g0y = (double)mg[1], g0z = (double)mg[2];

    // ---- pass 1: Protocol #1 and the means of the root-relative poses
    double s1 = 0.0, mpx = 0.0, mpy = 0.0, mpz = 0.0, mgx = 0.0, mgy = 0.0, mgz = 0.0;
    for (int j = 0; j < J; ++j) {
        double px, py, pz;
        PE_PRED(j, px, py, pz);
        px -= p0x; py -= p0y; pz -= p0z;
        const double gx = (double)mg[3 * j] - g0x, gy = (double)mg[3 * j + 1] - g0y, gz = (double)mg[3 * j + 2] - g0z;
        const double dx = px - gx, dy = py - gy, dz = pz - gz;
        s1 += sqrt(dx * dx + dy * dy + dz * dz);
        mpx += px; mpy += py; mpz += pz;
        mgx += gx; mgy += gy; mgz += gz;
    }
    const double inv_j = 1.0 / (double)J;
    mpx = mpx * inv_j + p0x; mpy = mpy * inv_j + p0y; mpz = mpz * inv_j + p0z;      // means of the un-rooted poses: the root cancels below
    mgx = mgx * inv_j + g0x; mgy = mgy * inv_j + g0y; mgz = mgz * inv_j + g0z;

    // ---- pass 2: extents and M = X0^T Y0 (X = gt, Y = pred)
    double nx = 0.0, ny = 0.0;
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m10 = 0.0, m11 = 0.0, m12 = 0.0, m20 = 0.0, m21 = 0.0, m22 = 0.0;
    for (int j = 0; j < J; ++j) {
        double yx, yy, yz;
        PE_PRED(j, yx, yy, yz);
        yx -= mpx; yy -= mpy; yz -= mpz;
        const double xx = (double)mg[3 * j] - mgx, xy = (double)mg[3 * j + 1] - mgy, xz = (double)mg[3 * j + 2] - mgz;
        nx += xx * xx + xy * xy + xz * xz;
        ny += yx * yx + yy * yy + yz * yz;
        m00 += xx * yx; m01 += xx * yy; m02 += xx * yz;
        m10 += xy * yx; m11 += xy * yy; m12 += xy * yz;
        m20 += xz * yx; m21 += xz * yy; m22 += xz * yz;
    }
    const double normx = sqrt(nx), normy = sqrt(ny);
    const double hs = 1.0 / (normx * normy);               // 1/0 for a zero extent: 0 * inf = NaN below, as the reference's 0/0
    const double h00 = m00 * hs, h01 = m01 * hs, h02 = m02 * hs, h10 = m10 * hs, h11 = m11 * hs, h12 = m12 * hs, h20 = m20 * hs,
                 h21 = m21 * hs, h22 = m22 * hs;

    // ---- R = V U^T and the signed sum of the singular values (pose_solve.h)
    double ssum, q00, q01, q02, q10, q11, q12, q20, q21, q22;
    pe_rotation(h00, h01, h02, h10, h11, h12, h20, h21, h22, ssum, q00, q01, q02, q10, q11, q12, q20, q21, q22);
    const double scale = ssum * normx / normy;
    // a R
    const double r00 = scale * q00, r01 = scale * q01, r02 = scale * q02;
    const double r10 = scale * q10, r11 = scale * q11, r12 = scale * q12;
    const double r20 = scale * q20, r21 = scale * q21, r22 = scale * q22;

    // ---- pass 3: Protocol #2
    double s2 = 0.0;
    for (int j = 0; j < J; ++j) {
        double yx, yy, yz;
        PE_PRED(j, yx, yy, yz);
        yx -= mpx; yy -= mpy; yz -= mpz;
        const double dx = yx * r00 + yy * r10 + yz * r20 - ((double)mg[3 * j] - mgx);
        const double dy = yx * r01 + yy * r11 + yz * r21 - ((double)mg[3 * j + 1] - mgy);
        const double dz = yx * r02 + yy * r12 + yz * r22 - ((double)mg[3 * j + 2] - mgz);
        s2 += sqrt(dx * dx + dy * dy + dz * dz);
    }
#undef PE_PRED
    e1[frame] = s1 * inv_j;
    e2[frame] = s2 * inv_j;
}

extern "C" int mbx_pose_errors(const float* pred, const float* gt, const float* hw, const float* factor, const float* x, int x_channels,
                               int rootrel, int gt_2d, double* e1, double* e2, int N, int T, int J, void* stream) {
    MBX_CHECK_ARG(pred && gt && e1 && e2, "pose_errors: null pointer");
    MBX_CHECK_ARG(N > 0 && T > 0 && (long long)N * T < (1ll << 31) - PE_FRAMES, "pose_errors: bad shape N=%d T=%d", N, T);
    MBX_CHECK_ARG(J > 1 && J <= 64, "pose_errors: bad joint count J=%d (1 < J <= 64)", J);
    MBX_CHECK_ARG(!gt_2d || (x && x_channels >= 2), "pose_errors: gt_2d needs the model input x [N,T,J,>=2] (x=%p, channels=%d)", (const void*)x,
                  x_channels);
    MBX_CHECK_ARG((((uintptr_t)pred | (uintptr_t)gt) & 3) == 0, "pose_errors: pred / gt must be 4-byte aligned");
    const long long frames = (long long)N * T;
    const size_t shm = (size_t)2 * PE_FRAMES * ((3 * J) | 1) * sizeof(float);
    if (shm > 64 * 1024 && mbx_set_dyn_lds(reinterpret_cast<const void*>(pose_errors_kernel), shm, "pose_errors")) return 1;
    hipLaunchKernelGGL(pose_errors_kernel, dim3((unsigned)((frames + PE_FRAMES - 1) / PE_FRAMES)), dim3(PE_FRAMES), shm, (hipStream_t)stream,
                       pred, gt, hw, factor, gt_2d ? x : nullptr, x_channels, rootrel, e1, e2, frames, T, J);
    MBX_LAUNCH_CHECK("pose_errors");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// aggregation (train.py:100-149).  Three launches, every sum in a fixed order:
//   1. frame_mean: one thread per test frame walks its CSR row (clip order) and leaves the mean of e1 and of e2 over the clips
//      that cover it; a frame without a clip, or whose mean e1 is not > 0 (NaN included, train.py:132), is marked left out.
//   2. action_partial: workgroup (chunk c, action a) sums the kept frames of action a inside chunk c: a thread adds its
//      frames in index order, the 256 threads fold through LDS in a fixed tree.
//   3. finish: thread a adds the chunk partials of action a in chunk order; thread 0 then averages the actions in order.
// An action without a kept frame gives 0 / 0 = NaN, as np.mean of an empty list does, and so does the summary then.
// ws: frame means [2][F] f64, kept flags [F] i32 (as f64 slots), partials [A][chunks][3] f64.
// ---------------------------------------------------------------------------------------------------------------
#define ER_CHUNK 8192
static inline int er_chunks(int F) { return (F + ER_CHUNK - 1) / ER_CHUNK; }

__global__ __launch_bounds__(256) void eval_frame_mean_kernel(const double* __restrict__ e1, const double* __restrict__ e2, long long n_err,
                                                              const int* __restrict__ row_ptr, const int* __restrict__ slots, int nnz,
                                                              double* __restrict__ fm, int* __restrict__ kept, int F) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int b = row_ptr[f], e = row_ptr[f + 1];
    b = b < 0 ? 0 : b;
    e = e > nnz ? nnz : e;                     // a malformed table reads nothing outside `slots`
    double s1 = 0.0, s2 = 0.0;
    int n = 0;
    for (int k = b; k < e; ++k) {
        const int s = slots[k];
        if (s < 0 || s >= n_err) continue;     // nor outside e1 / e2
        s1 += e1[s];
        s2 += e2[s];
        ++n;
    }
    const double m1 = s1 / (double)n, m2 = s2 / (double)n;
    const bool keep = n > 0 && m1 > 0.0;
    fm[f] = keep ? m1 : 0.0;
    fm[(size_t)F + f] = keep ? m2 : 0.0;
    kept[f] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void eval_action_partial_kernel(const double* __restrict__ fm, const int* __restrict__ kept,
                                                                  const int* __restrict__ action, double* __restrict__ part, int F,
                                                                  int chunks) {
    __shared__ double red[3][256];
    const int c = blockIdx.x, a = blockIdx.y, tid = threadIdx.x;
    const int beg = c * ER_CHUNK, end = beg + ER_CHUNK < F ? beg + ER_CHUNK : F;
    double s1 = 0.0, s2 = 0.0, n = 0.0;
    for (int f = beg + tid; f < end; f += 256) {
        if (action[f] == a && kept[f]) {
            s1 += fm[f];
            s2 += fm[(size_t)F + f];
            n += 1.0;
        }
    }
    red[0][tid] = s1; red[1][tid] = s2; red[2][tid] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
            red[2][tid] += red[2][tid + w];
        }
        __syncthreads();
    }
    if (tid < 3) part[((size_t)a * chunks + c) * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void eval_finish_kernel(const double* __restrict__ part, int chunks, int A, double* __restrict__ per_action,
                                                          double* __restrict__ summary, int* __restrict__ count) {
    for (int a = threadIdx.x; a < A; a += 256) {
        double s1 = 0.0, s2 = 0.0, n = 0.0;
        for (int c = 0; c < chunks; ++c) {
            const double* p = part + ((size_t)a * chunks + c) * 3;
            s1 += p[0]; s2 += p[1]; n += p[2];
        }
        per_action[a] = s1 / n;
        per_action[A + a] = s2 / n;
        count[a] = (int)n;
    }
    __syncthreads();      // per_action was written by this workgroup: visible to thread 0 after the barrier
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int a = 0; a < A; ++a) { t1 += per_action[a]; t2 += per_action[A + a]; }
        summary[0] = t1 / (double)A;
        summary[1] = t2 / (double)A;
    }
}

extern "C" size_t mbx_eval_reduce_ws(int F, int A) {
    if (F <= 0 || A <= 0) return 0;
    return ((size_t)3 * F + (size_t)A * er_chunks(F) * 3) * sizeof(double) + 256;
}
extern "C" int mbx_eval_reduce(const double* e1, const double* e2, int n_err, const int* row_ptr, int n_row_ptr, const int* slots, int nnz,
                               const int* action, int F, int A, double* per_action, double* summary, int* count, void* ws, void* stream) {
    MBX_CHECK_ARG(e1 && e2 && row_ptr && action && per_action && summary && count && ws, "eval_reduce: null pointer");
    MBX_CHECK_ARG(slots || nnz == 0, "eval_reduce: null slot list with nnz=%d", nnz);
    MBX_CHECK_ARG(n_err > 0 && F > 0 && A > 0 && A <= 65535 && nnz >= 0, "eval_reduce: bad sizes n_err=%d F=%d A=%d nnz=%d", n_err, F, A, nnz);
    MBX_CHECK_ARG(n_row_ptr == F + 1, "eval_reduce: CSR row table has %d entries for %d test frames (F + 1 expected)", n_row_ptr, F);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = er_chunks(F);
    double* fm = (double*)ws;
    int* kept = (int*)(fm + (size_t)2 * F);
    double* part = fm + (size_t)3 * F;
    hipLaunchKernelGGL(eval_frame_mean_kernel, dim3((F + 255) / 256), dim3(256), 0, s, e1, e2, (long long)n_err, row_ptr, slots, nnz, fm, kept, F);
    MBX_LAUNCH_CHECK("eval_reduce (frame means)");
    hipLaunchKernelGGL(eval_action_partial_kernel, dim3(chunks, A), dim3(256), 0, s, (const double*)fm, (const int*)kept, action, part, F, chunks);
    MBX_LAUNCH_CHECK("eval_reduce (action partials)");
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, chunks, A, per_action, summary, count);
    MBX_LAUNCH_CHECK("eval_reduce (finish)");
    return 0;
}
