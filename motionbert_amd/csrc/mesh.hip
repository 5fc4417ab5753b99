// Mesh recovery around a user-supplied SMPL layer (lib/model/model_mesh.py:57-79; lib/model/loss_mesh.py:49-68; lib/utils/utils_mesh.py).
//   mbx_rot6d_theta_fwd / _bwd : the head's rotation chain 6D -> rotation matrix -> quaternion -> axis-angle, one thread per joint, and
//                                its pull-back (the forward is recomputed in registers, nothing is saved).
//   mbx_mesh_param_loss        : loss_pose (through batch_rodrigues on both sides), loss_shape, loss_norm, their weighted sum and its
//                                gradient with respect to the predicted theta, in one call.
//   mbx_mesh_errors            : per frame MPVE, MPJPE (17 / 14 joints) and Procrustes-aligned MPJPE (17 / 14 joints), fp64 after the loads.
// fp32 loads, fixed summation order, no floating-point atomics: two calls on the same inputs give the same bits.
#include "mbx_common.h"
#include "pose_solve.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------------
// rotation chain.  x6 row = (a1x, a2x, a1y, a2y, a1z, a2z): the reference's view(-1, 3, 2) (utils_mesh.py:317).
// ---------------------------------------------------------------------------------------------------------------
struct RotFwd {
    float a1[3], a2[3], n1, b1[3], dot, u[3], nu, b2[3], b3[3];
    int qcase;            // the quaternion case of rotation_matrix_to_quaternion (utils_mesh.py:206-209)
    float qs[4], t;       // the selected numerator and trace term
    float q[4];           // 0.5 * qs / sqrt(t)
    float s2, s, tt, k;   // sin^2, sin, 2 * theta, aa = q_xyz * k
    float aa[3];          // before the NaN rule
};

__device__ __forceinline__ void rot_forward(const float* __restrict__ x, RotFwd& r) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { r.a1[i] = x[2 * i]; r.a2[i] = x[2 * i + 1]; }
    r.n1 = sqrtf(r.a1[0] * r.a1[0] + r.a1[1] * r.a1[1] + r.a1[2] * r.a1[2]);
    const float d1 = fmaxf(r.n1, 1e-6f);                       // F.normalize(eps=1e-6): v / max(|v|, eps)
#pragma unroll
    for (int i = 0; i < 3; ++i) r.b1[i] = r.a1[i] / d1;
    r.dot = r.b1[0] * r.a2[0] + r.b1[1] * r.a2[1] + r.b1[2] * r.a2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) r.u[i] = r.a2[i] - r.dot * r.b1[i];
    r.nu = sqrtf(r.u[0] * r.u[0] + r.u[1] * r.u[1] + r.u[2] * r.u[2]);
    const float d2 = fmaxf(r.nu, 1e-6f);
#pragma unroll
    for (int i = 0; i < 3; ++i) r.b2[i] = r.u[i] / d2;
    r.b3[0] = r.b1[1] * r.b2[2] - r.b1[2] * r.b2[1];
    r.b3[1] = r.b1[2] * r.b2[0] - r.b1[0] * r.b2[2];
    r.b3[2] = r.b1[0] * r.b2[1] - r.b1[1] * r.b2[0];
    // m = R^T (utils_mesh.py:175): m_ij = R_ji, R = [b1 b2 b3] by columns, so row i of m is b_{i+1}
    const float m00 = r.b1[0], m01 = r.b1[1], m02 = r.b1[2];
    const float m10 = r.b2[0], m11 = r.b2[1], m12 = r.b2[2];
    const float m20 = r.b3[0], m21 = r.b3[1], m22 = r.b3[2];
    const bool d2m = m22 < 1e-6f, d0_d1 = m00 > m11, d0_nd1 = m00 < -m11;
    if (d2m && d0_d1) {
        r.qcase = 0;
        r.t = 1.f + m00 - m11 - m22;
        r.qs[0] = m12 - m21; r.qs[1] = r.t; r.qs[2] = m01 + m10; r.qs[3] = m20 + m02;
    } else if (d2m) {
        r.qcase = 1;
        r.t = 1.f - m00 + m11 - m22;
        r.qs[0] = m20 - m02; r.qs[1] = m01 + m10; r.qs[2] = r.t; r.qs[3] = m12 + m21;
    } else if (d0_nd1) {
        r.qcase = 2;
        r.t = 1.f - m00 - m11 + m22;
        r.qs[0] = m01 - m10; r.qs[1] = m20 + m02; r.qs[2] = m12 + m21; r.qs[3] = r.t;
    } else {
        r.qcase = 3;
        r.t = 1.f + m00 + m11 + m22;
        r.qs[0] = r.t; r.qs[1] = m12 - m21; r.qs[2] = m20 - m02; r.qs[3] = m01 - m10;
    }
    const float st = sqrtf(r.t);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.q[i] = (r.qs[i] / st) * 0.5f;
    r.s2 = r.q[1] * r.q[1] + r.q[2] * r.q[2] + r.q[3] * r.q[3];
    r.s = sqrtf(r.s2);
    const float c = r.q[0];
    r.tt = 2.0f * (c < 0.0f ? atan2f(-r.s, -c) : atan2f(r.s, c));
    r.k = r.s2 > 0.0f ? r.tt / r.s : 2.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) r.aa[i] = r.q[i + 1] * r.k;
}

__global__ __launch_bounds__(256) void rot6d_theta_fwd_kernel(const float* __restrict__ x6, float* __restrict__ rotmat, float* __restrict__ aa,
                                                              int M) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    RotFwd r;
    rot_forward(x6 + (size_t)j * 6, r);
    if (rotmat) {
        float* o = rotmat + (size_t)j * 9;
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[3 * i] = r.b1[i]; o[3 * i + 1] = r.b2[i]; o[3 * i + 2] = r.b3[i]; }
    }
    if (aa) {
#pragma unroll
        for (int i = 0; i < 3; ++i) aa[(size_t)j * 3 + i] = r.aa[i] != r.aa[i] ? 0.0f : r.aa[i];      // aa[isnan(aa)] = 0 (utils_mesh.py:82)
    }
}

// d v / max(|v|, eps) pulled back: (g - b (b . g)) / |v| above the clamp, g / eps below it
__device__ __forceinline__ void normalize_bwd(const float (&b)[3], float n, const float (&g)[3], float (&dv)[3]) {
    if (n >= 1e-6f) {
        const float bg = b[0] * g[0] + b[1] * g[1] + b[2] * g[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) dv[i] = (g[i] - b[i] * bg) / n;
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) dv[i] = g[i] / 1e-6f;
    }
}

__global__ __launch_bounds__(256) void rot6d_theta_bwd_kernel(const float* __restrict__ x6, const float* __restrict__ drotmat,
                                                              const float* __restrict__ daa, float* __restrict__ dx6, int M) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    RotFwd r;
    rot_forward(x6 + (size_t)j * 6, r);
    // cotangent of m = R^T, row i = b_{i+1}
    float dm[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) dm[i][c] = drotmat ? drotmat[(size_t)j * 9 + 3 * c + i] : 0.0f;
    if (daa) {
        float g[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float v = daa[(size_t)j * 3 + i];
            g[i] = r.aa[i] != r.aa[i] ? 0.0f : v;                // an element the NaN rule overwrote has no gradient
        }
        float dq[4];
        if (r.s2 > 0.0f) {
            const float dk = g[0] * r.q[1] + g[1] * r.q[2] + g[2] * r.q[3];
            const float dtt = dk / r.s;
            const float c = r.q[0];
            const float rr = r.s2 + c * c;
            // tt = 2 atan2(+-s, +-c): d tt / d s = 2 c / (s^2 + c^2), d tt / d c = -2 s / (s^2 + c^2) for both forms
            const float ds = -dk * r.tt / r.s2 + 2.0f * dtt * c / rr;
            dq[0] = -2.0f * dtt * r.s / rr;
            const float ds2 = ds / (2.0f * r.s);
#pragma unroll
            for (int i = 0; i < 3; ++i) dq[i + 1] = g[i] * r.k + 2.0f * r.q[i + 1] * ds2;
        } else {
            // sin^2 == 0: the reference's autograd is NaN here (0 * inf through the unselected k_pos); the continuous extension
            // of aa = 2 q_xyz (1 + O(|q_xyz|^2)) is used instead
            dq[0] = 0.0f;
#pragma unroll
            for (int i = 0; i < 3; ++i) dq[i + 1] = 2.0f * g[i];
        }
        // q = 0.5 qs / sqrt(t)
        const float st = sqrtf(r.t);
        float dqs[4];
        float dt = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dqs[i] = 0.5f * dq[i] / st;
            dt += dq[i] * r.qs[i];
        }
        dt = -0.25f * dt / (r.t * st);
        // numerators back to m; the trace term sits in slot 1 / 2 / 3 / 0 of the cases 0 .. 3
        if (r.qcase == 0) {
            dt += dqs[1];
            dm[1][2] += dqs[0]; dm[2][1] -= dqs[0];
            dm[0][1] += dqs[2]; dm[1][0] += dqs[2];
            dm[2][0] += dqs[3]; dm[0][2] += dqs[3];
            dm[0][0] += dt; dm[1][1] -= dt; dm[2][2] -= dt;
        } else if (r.qcase == 1) {
            dt += dqs[2];
            dm[2][0] += dqs[0]; dm[0][2] -= dqs[0];
            dm[0][1] += dqs[1]; dm[1][0] += dqs[1];
            dm[1][2] += dqs[3]; dm[2][1] += dqs[3];
            dm[0][0] -= dt; dm[1][1] += dt; dm[2][2] -= dt;
        } else if (r.qcase == 2) {
            dt += dqs[3];
            dm[0][1] += dqs[0]; dm[1][0] -= dqs[0];
            dm[2][0] += dqs[1]; dm[0][2] += dqs[1];
            dm[1][2] += dqs[2]; dm[2][1] += dqs[2];
            dm[0][0] -= dt; dm[1][1] -= dt; dm[2][2] += dt;
        } else {
            dt += dqs[0];
            dm[1][2] += dqs[1]; dm[2][1] -= dqs[1];
            dm[2][0] += dqs[2]; dm[0][2] -= dqs[2];
            dm[0][1] += dqs[3]; dm[1][0] -= dqs[3];
            dm[0][0] += dt; dm[1][1] += dt; dm[2][2] += dt;
        }
    }
    float db1[3], db2[3], db3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { db1[i] = dm[0][i]; db2[i] = dm[1][i]; db3[i] = dm[2][i]; }
    // b3 = b1 x b2:  d b1 += b2 x d b3,  d b2 += d b3 x b1
    db1[0] += r.b2[1] * db3[2] - r.b2[2] * db3[1];
    db1[1] += r.b2[2] * db3[0] - r.b2[0] * db3[2];
    db1[2] += r.b2[0] * db3[1] - r.b2[1] * db3[0];
    db2[0] += db3[1] * r.b1[2] - db3[2] * r.b1[1];
    db2[1] += db3[2] * r.b1[0] - db3[0] * r.b1[2];
    db2[2] += db3[0] * r.b1[1] - db3[1] * r.b1[0];
    float du[3], da1[3], da2[3];
    normalize_bwd(r.b2, r.nu, db2, du);
    // u = a2 - dot b1, dot = b1 . a2
    const float ddot = -(du[0] * r.b1[0] + du[1] * r.b1[1] + du[2] * r.b1[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        da2[i] = du[i] + ddot * r.b1[i];
        db1[i] += -r.dot * du[i] + ddot * r.a2[i];
    }
    normalize_bwd(r.b1, r.n1, db1, da1);
    float* o = dx6 + (size_t)j * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) { o[2 * i] = da1[i]; o[2 * i + 1] = da2[i]; }
}

extern "C" int mbx_rot6d_theta_fwd(const float* x6, float* rotmat, float* aa, int M, void* stream) {
    MBX_CHECK_ARG(M >= 0 && M <= (1 << 28), "rot6d_theta_fwd: bad joint count M=%d", M);
    if (M == 0) return 0;
    MBX_CHECK_ARG(x6 && (rotmat || aa), "rot6d_theta_fwd: null pointer (x6, and at least one of rotmat / aa)");
    MBX_CHECK_ARG((((uintptr_t)x6 | (uintptr_t)rotmat | (uintptr_t)aa) & 3) == 0, "rot6d_theta_fwd: pointers must be 4-byte aligned");
    hipLaunchKernelGGL(rot6d_theta_fwd_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, x6, rotmat, aa, M);
    MBX_LAUNCH_CHECK("rot6d_theta_fwd");
    return 0;
}

extern "C" int mbx_rot6d_theta_bwd(const float* x6, const float* drotmat, const float* daa, float* dx6, int M, void* stream) {
    MBX_CHECK_ARG(M >= 0 && M <= (1 << 28), "rot6d_theta_bwd: bad joint count M=%d", M);
    if (M == 0) return 0;
    MBX_CHECK_ARG(x6 && dx6, "rot6d_theta_bwd: null pointer (x6, dx6)");
    MBX_CHECK_ARG(dx6 != x6, "rot6d_theta_bwd: dx6 must not alias x6");
    MBX_CHECK_ARG((((uintptr_t)x6 | (uintptr_t)drotmat | (uintptr_t)daa | (uintptr_t)dx6) & 3) == 0,
                  "rot6d_theta_bwd: pointers must be 4-byte aligned");
    hipLaunchKernelGGL(rot6d_theta_bwd_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, x6, drotmat, daa, dx6, M);
    MBX_LAUNCH_CHECK("rot6d_theta_bwd");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// parameter losses.  A workgroup of 256 threads owns 8 frames, 32 slots each: slot j < 24 is joint j of the pose (batch_rodrigues
// on the prediction and on the ground truth, the 9 differences, the pull-back to the 3 pose elements), slot 24 the 10 shape
// elements, slots 25 .. 31 idle.  |theta| of a frame is the sum of the 25 slots' squares, added in slot order by every slot of
// the frame.  A workgroup leaves three partial sums (LDS tree); the finishing launch adds them in workgroup order.
// ---------------------------------------------------------------------------------------------------------------
#define ML_FRAMES 8
#define ML_SLOTS 32

// batch_rodrigues (utils_mesh.py:8-51) of one axis-angle vector: the normalised quaternion qn and what the pull-back needs
struct Rodrigues {
    float n, h, sh, ch, nq, qn[4];
};
// No fma contraction in here: the prediction and the target go through two inlined copies of this function, and a joint that is equal on
// both sides must give the same bits twice (an L1 difference of exactly 0 has the subgradient 0; one of an ulp has +-1).
__device__ __forceinline__ void rodrigues(const float (&a)[3], Rodrigues& o, float (&R)[9]) {
#pragma clang fp contract(off)
    const float e0 = a[0] + 1e-8f, e1 = a[1] + 1e-8f, e2 = a[2] + 1e-8f;
    o.n = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    o.h = o.n * 0.5f;
    o.ch = cosf(o.h);
    o.sh = sinf(o.h);
    float q[4];
    q[0] = o.ch;
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i + 1] = o.sh * (a[i] / o.n);
    o.nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) o.qn[i] = q[i] / o.nq;
    const float w = o.qn[0], x = o.qn[1], y = o.qn[2], z = o.qn[3];
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = w2 + x2 - y2 - z2; R[1] = 2.f * xy - 2.f * wz; R[2] = 2.f * wy + 2.f * xz;
    R[3] = 2.f * wz + 2.f * xy; R[4] = w2 - x2 + y2 - z2; R[5] = 2.f * yz - 2.f * wx;
    R[6] = 2.f * xz - 2.f * wy; R[7] = 2.f * wx + 2.f * yz; R[8] = w2 - x2 - y2 + z2;
}

__device__ __forceinline__ float ml_term(float d, int loss_type, float& g) {
    if (loss_type == 0) { g = 2.0f * d; return d * d; }
    g = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);            // torch's sign: 0 at 0 (NaN stays out of the comparison: 0)
    return fabsf(d);
}

__global__ __launch_bounds__(256) void mesh_param_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int loss_type,
                                                              float c_pose, float c_shape, float c_norm, float* __restrict__ part,
                                                              float* __restrict__ dtheta, int F) {
    __shared__ float ssq[256];
    __shared__ float red[3][256];
    const int tid = threadIdx.x, slot = tid & (ML_SLOTS - 1), fl = tid / ML_SLOTS;
    const int f = blockIdx.x * ML_FRAMES + fl;
    const bool live = f < F;
    const float* p = pred + (size_t)(live ? f : 0) * 82;
    const float* g = gt + (size_t)(live ? f : 0) * 82;
    float sum_pose = 0.f, sum_shape = 0.f, sq = 0.f;
    float a[3] = {0.f, 0.f, 0.f}, da[3] = {0.f, 0.f, 0.f};
    if (live && slot < 24) {
        float b[3], Rp[9], Rg[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) { a[i] = p[3 * slot + i]; b[i] = g[3 * slot + i]; }
        sq = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
        Rodrigues rp, rg;
        rodrigues(a, rp, Rp);
        rodrigues(b, rg, Rg);
        float d[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            float gi;
            sum_pose += ml_term(Rp[i] - Rg[i], loss_type, gi);
            d[i] = c_pose * gi;
        }
        if (dtheta) {
            const float w = rp.qn[0], x = rp.qn[1], y = rp.qn[2], z = rp.qn[3];
            float dqn[4];
            dqn[0] = 2.f * w * (d[0] + d[4] + d[8]) + 2.f * (-z * d[1] + y * d[2] + z * d[3] - x * d[5] - y * d[6] + x * d[7]);
            dqn[1] = 2.f * x * (d[0] - d[4] - d[8]) + 2.f * (y * d[1] + z * d[2] + y * d[3] - w * d[5] + z * d[6] + w * d[7]);
            dqn[2] = 2.f * y * (-d[0] + d[4] - d[8]) + 2.f * (x * d[1] + w * d[2] + x * d[3] + z * d[5] - w * d[6] + z * d[7]);
            dqn[3] = 2.f * z * (-d[0] - d[4] + d[8]) + 2.f * (-w * d[1] + x * d[2] + w * d[3] + y * d[5] + x * d[6] + y * d[7]);
            const float qd = rp.qn[0] * dqn[0] + rp.qn[1] * dqn[1] + rp.qn[2] * dqn[2] + rp.qn[3] * dqn[3];
            float dq[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dq[i] = (dqn[i] - rp.qn[i] * qd) / rp.nq;
            // q = (cos h, sin h * a / n), h = n / 2, n = |a + 1e-8|
            const float an0 = a[0] / rp.n, an1 = a[1] / rp.n, an2 = a[2] / rp.n;
            const float dh = -rp.sh * dq[0] + rp.ch * (an0 * dq[1] + an1 * dq[2] + an2 * dq[3]);
            const float dan0 = rp.sh * dq[1], dan1 = rp.sh * dq[2], dan2 = rp.sh * dq[3];
            const float dn = 0.5f * dh - (dan0 * a[0] + dan1 * a[1] + dan2 * a[2]) / (rp.n * rp.n);
            da[0] = dan0 / rp.n + dn * ((a[0] + 1e-8f) / rp.n);
            da[1] = dan1 / rp.n + dn * ((a[1] + 1e-8f) / rp.n);
            da[2] = dan2 / rp.n + dn * ((a[2] + 1e-8f) / rp.n);
        }
    } else if (live && slot == 24) {
        for (int i = 0; i < 10; ++i) {
            const float v = p[72 + i];
            sq += v * v;
        }
    }
    ssq[tid] = sq;
    __syncthreads();
    float n2 = 0.f;
    for (int s = 0; s < 25; ++s) n2 += ssq[fl * ML_SLOTS + s];
    const float nrm = sqrtf(n2);
    const float gn = nrm > 0.0f ? c_norm / nrm : 0.0f;          // d |theta| / d theta = theta / |theta|, 0 at the origin (torch.norm's rule)
    if (live && slot < 24 && dtheta) {
#pragma unroll
        for (int i = 0; i < 3; ++i) dtheta[(size_t)f * 82 + 3 * slot + i] = da[i] + gn * a[i];
    }
    if (live && slot == 24) {
        for (int i = 0; i < 10; ++i) {
            const float v = p[72 + i];
            float gi;
            sum_shape += ml_term(v - g[72 + i], loss_type, gi);
            if (dtheta) dtheta[(size_t)f * 82 + 72 + i] = c_shape * gi + gn * v;
        }
    }
    red[0][tid] = sum_pose;
    red[1][tid] = sum_shape;
    red[2][tid] = (live && slot == 0) ? nrm : 0.f;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
            red[2][tid] += red[2][tid + w];
        }
        __syncthreads();
    }
    if (tid < 3) part[(size_t)blockIdx.x * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void mesh_param_finish_kernel(const float* __restrict__ part, int nparts, float lambda_pose, float lambda_shape,
                                                                float lambda_norm, float* __restrict__ losses, int F) {
    __shared__ float red[3][256];
    const int tid = threadIdx.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int p = tid; p < nparts; p += 256) { s0 += part[(size_t)p * 3]; s1 += part[(size_t)p * 3 + 1]; s2 += part[(size_t)p * 3 + 2]; }
    red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
            red[2][tid] += red[2][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float lp = red[0][0] / ((float)F * 216.0f), ls = red[1][0] / ((float)F * 10.0f), ln = red[2][0] / (float)F;
        losses[0] = lp;
        losses[1] = ls;
        losses[2] = ln;
        losses[3] = lambda_pose * lp + lambda_shape * ls + lambda_norm * ln;
    }
}

static inline int ml_groups(int F) { return (F + ML_FRAMES - 1) / ML_FRAMES; }

extern "C" size_t mbx_mesh_param_loss_ws(int F) {
    if (F < 1) return 0;
    return (size_t)ml_groups(F) * 3 * sizeof(float) + 256;
}

extern "C" int mbx_mesh_param_loss(const float* pred_theta, const float* gt_theta, int loss_type, float lambda_pose, float lambda_shape,
                                   float lambda_norm, float grad_scale, float* losses, float* dtheta, int F, void* ws, void* stream) {
    MBX_CHECK_ARG(pred_theta && gt_theta && losses && ws, "mesh_param_loss: null pointer");
    MBX_CHECK_ARG(F >= 1 && F <= (1 << 24), "mesh_param_loss: bad frame count F=%d", F);
    MBX_CHECK_ARG(loss_type == 0 || loss_type == 1, "mesh_param_loss: loss_type %d (0 = MSE, 1 = L1)", loss_type);
    MBX_CHECK_ARG(dtheta != pred_theta && dtheta != gt_theta, "mesh_param_loss: dtheta must not alias an input");
    MBX_CHECK_ARG((((uintptr_t)pred_theta | (uintptr_t)gt_theta | (uintptr_t)losses | (uintptr_t)dtheta | (uintptr_t)ws) & 3) == 0,
                  "mesh_param_loss: pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int groups = ml_groups(F);
    float* part = (float*)ws;
    hipLaunchKernelGGL(mesh_param_loss_kernel, dim3(groups), dim3(256), 0, s, pred_theta, gt_theta, loss_type,
                       grad_scale * lambda_pose / ((float)F * 216.0f), grad_scale * lambda_shape / ((float)F * 10.0f),
                       grad_scale * lambda_norm / (float)F, part, dtheta, F);
    MBX_LAUNCH_CHECK("mesh_param_loss");
    hipLaunchKernelGGL(mesh_param_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)part, groups, lambda_pose, lambda_shape, lambda_norm,
                       losses, F);
    MBX_LAUNCH_CHECK("mesh_param_loss (finish)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// mesh errors (utils_mesh.py:333-438).  One workgroup of 256 threads per frame.  Thread v, v + 256, ... owns a vertex: its three
// coordinates of both sides, minus that side's joint 0, distance in fp64; the 256 partial sums fold through LDS in a fixed tree.
// Scalar 4-byte loads: a frame's base is only 8-byte aligned for odd frames at V = 6890, and the three strided loads of a wave
// cover one contiguous run of 768 bytes.  The joints go to LDS root-relative in fp64; lane 0 of wave 0 then solves the 17-joint
// alignment and lane 0 of wave 1 the 14-joint one, side by side.
// rigid_align (A = pred, B = gt): H = A0^T B0 / n = U S V^T, R = V U^T (last row of V^T flipped when det < 0), c = sum(s) / var(A),
// aligned_j = c R (A_j - muA) + muB.  With X = gt, Y = pred this is pose_solve.h's R applied to rows, and H is passed as
// X0^T Y0 / |Y0|^2, so that sum(s) is c itself.  |Y0| = 0 gives 0 * inf = NaN as the reference's 0 / 0; |X0| = 0 alone gives c = 0
// in the reference (aligned_j = muB): the rotation is left out there instead of dividing 0 by 0.
// ---------------------------------------------------------------------------------------------------------------
#define ME_J 17

__device__ __forceinline__ int me_joint(int k, bool subset) {      // h36m_17_to_14 = (1 .. 6, 8, 10 .. 16)
    return !subset ? k : (k < 6 ? k + 1 : (k == 6 ? 8 : k + 3));
}

// jp / jg: root-relative joints [17][3] in LDS.  Returns MPJPE and PA-MPJPE over the 17 joints or the 14-joint subset.
__device__ __forceinline__ void me_joint_errors(const double* jp, const double* jg, bool subset, double& e_mpjpe, double& e_pa) {
    const int n = subset ? 14 : ME_J;
    const double inv_n = 1.0 / (double)n;
    double s1 = 0.0, mpx = 0.0, mpy = 0.0, mpz = 0.0, mgx = 0.0, mgy = 0.0, mgz = 0.0;
    for (int k = 0; k < n; ++k) {
        const int j = me_joint(k, subset);
        const double px = jp[3 * j], py = jp[3 * j + 1], pz = jp[3 * j + 2];
        const double gx = jg[3 * j], gy = jg[3 * j + 1], gz = jg[3 * j + 2];
        const double dx = px - gx, dy = py - gy, dz = pz - gz;
        s1 += sqrt(dx * dx + dy * dy + dz * dz);
        mpx += px; mpy += py; mpz += pz;
        mgx += gx; mgy += gy; mgz += gz;
    }
    e_mpjpe = s1 * inv_n;
    mpx *= inv_n; mpy *= inv_n; mpz *= inv_n;
    mgx *= inv_n; mgy *= inv_n; mgz *= inv_n;
    double nx = 0.0, ny = 0.0;
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m10 = 0.0, m11 = 0.0, m12 = 0.0, m20 = 0.0, m21 = 0.0, m22 = 0.0;
    for (int k = 0; k < n; ++k) {
        const int j = me_joint(k, subset);
        const double yx = jp[3 * j] - mpx, yy = jp[3 * j + 1] - mpy, yz = jp[3 * j + 2] - mpz;
        const double xx = jg[3 * j] - mgx, xy = jg[3 * j + 1] - mgy, xz = jg[3 * j + 2] - mgz;
        nx += xx * xx + xy * xy + xz * xz;
        ny += yx * yx + yy * yy + yz * yz;
        m00 += xx * yx; m01 += xx * yy; m02 += xx * yz;
        m10 += xy * yx; m11 += xy * yy; m12 += xy * yz;
        m20 += xz * yx; m21 += xz * yy; m22 += xz * yz;
    }
    const double hs = 1.0 / ny;
    double c, r00, r01, r02, r10, r11, r12, r20, r21, r22;
    pe_rotation(m00 * hs, m01 * hs, m02 * hs, m10 * hs, m11 * hs, m12 * hs, m20 * hs, m21 * hs, m22 * hs, c, r00, r01, r02, r10, r11, r12,
                r20, r21, r22);
    const bool flat_gt = nx == 0.0 && ny > 0.0;
    r00 = flat_gt ? 0.0 : c * r00; r01 = flat_gt ? 0.0 : c * r01; r02 = flat_gt ? 0.0 : c * r02;
    r10 = flat_gt ? 0.0 : c * r10; r11 = flat_gt ? 0.0 : c * r11; r12 = flat_gt ? 0.0 : c * r12;
    r20 = flat_gt ? 0.0 : c * r20; r21 = flat_gt ? 0.0 : c * r21; r22 = flat_gt ? 0.0 : c * r22;
    double s2 = 0.0;
    for (int k = 0; k < n; ++k) {
        const int j = me_joint(k, subset);
        const double yx = jp[3 * j] - mpx, yy = jp[3 * j + 1] - mpy, yz = jp[3 * j + 2] - mpz;
        const double dx = yx * r00 + yy * r10 + yz * r20 - (jg[3 * j] - mgx);
        const double dy = yx * r01 + yy * r11 + yz * r21 - (jg[3 * j + 1] - mgy);
        const double dz = yx * r02 + yy * r12 + yz * r22 - (jg[3 * j + 2] - mgz);
        s2 += sqrt(dx * dx + dy * dy + dz * dz);
    }
    e_pa = s2 * inv_n;
}

__global__ __launch_bounds__(256) void mesh_errors_kernel(const float* __restrict__ vp, const float* __restrict__ vg,
                                                          const float* __restrict__ kp, const float* __restrict__ kg,
                                                          double* __restrict__ err, int F, int V) {
    __shared__ double jp[ME_J * 3], jg[ME_J * 3];
    __shared__ double red[256];
    const int tid = threadIdx.x, f = blockIdx.x;
    const float* kpf = kp + (size_t)f * ME_J * 3;
    const float* kgf = kg + (size_t)f * ME_J * 3;
    const double p0x = (double)kpf[0], p0y = (double)kpf[1], p0z = (double)kpf[2];
    const double g0x = (double)kgf[0], g0y = (double)kgf[1], g0z = (double)kgf[2];
    if (tid < ME_J * 3) {
        const int c = tid % 3;
        jp[tid] = (double)kpf[tid] - (c == 0 ? p0x : (c == 1 ? p0y : p0z));
        jg[tid] = (double)kgf[tid] - (c == 0 ? g0x : (c == 1 ? g0y : g0z));
    }
    double acc = 0.0;
    if (vp) {
        const float* a = vp + (size_t)f * V * 3;
        const float* b = vg + (size_t)f * V * 3;
        for (int v = tid; v < V; v += 256) {
            const double dx = ((double)a[3 * (size_t)v] - p0x) - ((double)b[3 * (size_t)v] - g0x);
            const double dy = ((double)a[3 * (size_t)v + 1] - p0y) - ((double)b[3 * (size_t)v + 1] - g0y);
            const double dz = ((double)a[3 * (size_t)v + 2] - p0z) - ((double)b[3 * (size_t)v + 2] - g0z);
            acc += sqrt(dx * dx + dy * dy + dz * dz);
        }
    }
    red[tid] = acc;
    __syncthreads();                                      // also: jp / jg are complete
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) err[f] = vp ? red[0] / (double)V : (double)NAN;
    if (tid == 0 || tid == MBX_WAVE) {
        const bool subset = tid != 0;
        double e1, e2;
        me_joint_errors(jp, jg, subset, e1, e2);
        err[(size_t)(subset ? 2 : 1) * F + f] = e1;
        err[(size_t)(subset ? 4 : 3) * F + f] = e2;
    }
}

extern "C" int mbx_mesh_errors(const float* verts_p, const float* verts_g, const float* kp_p, const float* kp_g, double* err, int F, int V,
                               void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= (1 << 24), "mesh_errors: bad frame count F=%d", F);
    if (F == 0) return 0;
    MBX_CHECK_ARG(kp_p && kp_g && err, "mesh_errors: null pointer (kp_p, kp_g, err)");
    MBX_CHECK_ARG((verts_p == nullptr) == (verts_g == nullptr), "mesh_errors: verts_p and verts_g must both be given or both be NULL");
    MBX_CHECK_ARG(V >= 1 && V <= (1 << 24), "mesh_errors: bad vertex count V=%d", V);
    MBX_CHECK_ARG((((uintptr_t)verts_p | (uintptr_t)verts_g | (uintptr_t)kp_p | (uintptr_t)kp_g) & 3) == 0 && ((uintptr_t)err & 7) == 0,
                  "mesh_errors: verts / kp must be 4-byte aligned, err 8-byte aligned");
    hipLaunchKernelGGL(mesh_errors_kernel, dim3(F), dim3(256), 0, (hipStream_t)stream, verts_p, verts_g, kp_p, kp_g, err, F, V);
    MBX_LAUNCH_CHECK("mesh_errors");
    return 0;
}
