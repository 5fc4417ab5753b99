// Device arithmetic the SMPL consumers share (smpl.hip: the prepare kernels of mbx_mesh_gt and mbx_wild_mesh; amass.hip).
#pragma once

// smplx batch_rodrigues: angle = |r + 1e-8|, d = r / angle, R = I + sin K + (1 - cos) K^2; r = 0 gives K = 0 and R = I exactly.
// Not the quaternion form of mesh.hip (the reference's own batch_rodrigues), which is another function with its own contraction rule.
__device__ __forceinline__ void smplx_rodrigues(float r0, float r1, float r2, float* __restrict__ R) {
    const float a0 = r0 + 1e-8f, a1 = r1 + 1e-8f, a2 = r2 + 1e-8f;
    const float angle = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
    const float x = r0 / angle, y = r1 / angle, z = r2 / angle;
    const float s = sinf(angle), c = 1.0f - cosf(angle);
    R[0] = 1.0f - c * (y * y + z * z); R[1] = c * (x * y) - s * z;         R[2] = s * y + c * (x * z);
    R[3] = s * z + c * (x * y);        R[4] = 1.0f - c * (x * x + z * z);  R[5] = c * (y * z) - s * x;
    R[6] = c * (x * z) - s * y;        R[7] = s * x + c * (y * z);         R[8] = 1.0f - c * (x * x + y * y);
}
