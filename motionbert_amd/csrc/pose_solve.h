// The 3x3 decomposition behind every Procrustes alignment of the library (pose_eval.hip: mbx_pose_errors; mesh.hip: mbx_mesh_errors).
// fp64, a fixed number of operations: no data-dependent loop, terminates on NaN input (NaN in, NaN out).
//
// Domain and accuracy, in the singular values s0 >= s1 >= |s2| of H.  For every finite H with s0 > 0 the result is a proper rotation
// (orthogonal to rounding, det +1) and a finite ssum:
//   s1 / s0 >= 1e-3          the aligned error agrees with a LAPACK SVD to 1e-10 of the larger of itself and the rms joint distance from
//                            the centroid (measured on the MI355X: 5e-13, profiles/procrustes_parity.txt).  Every human pose is here;
//                            s2 may be anything, 0 (a planar pose) and negative (a mirrored one) included.
//   2^-26 < s1 / s0 < 1e-3   a needle.  The right vectors come from H^T H, whose squaring leaves v1, v2 with a relative error of about
//                            2^-52 (s0 / s1)^2: the roll about the needle's axis degrades and is lost at the lower end.  u0, v0, the
//                            orthogonality of R and s0 are not affected, so the aligned error is off by at most
//                                (2 s1 |X0| + 2 min(|X0_T|, a |Y0_T|)) / sqrt(J)
//                            with X0_T, Y0_T the parts of the centred poses transverse to their leading axes (tests/procerr.py derives it).
//   s1 / s0 <= 2^-26         rank one: a pose on a line, or J = 2.  u1 is chosen orthogonal to u0 and s1 counts as 0.  The bound above
//                            holds; for an exactly collinear pose it is 0 and the result is the reference's to rounding.
// Taking V from H itself (one-sided Jacobi) would remove the middle band.
#pragma once

// one Jacobi rotation of the symmetric 3x3 matrix in the (p, q) plane; r is the third index.  V's columns p and q follow.
__device__ __forceinline__ void pe_jacobi(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p, double& v0q,
                                          double& v1p, double& v1q, double& v2p, double& v2q) {
    const double theta = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = theta < 0.0 ? -t : t;
    t = apq == 0.0 ? 0.0 : t;              // nothing to annihilate (theta = +-inf or NaN)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double pr = apr, qr = aqr;
    apr = c * pr - s * qr;
    aqr = s * pr + c * qr;
    double a, b;
    a = v0p; b = v0q; v0p = c * a - s * b; v0q = s * a + c * b;
    a = v1p; b = v1q; v1p = c * a - s * b; v1q = s * a + c * b;
    a = v2p; b = v2q; v2p = c * a - s * b; v2q = s * a + c * b;
}
__device__ __forceinline__ void pe_swap_if(bool sw, double& a, double& b) {
    const double x = sw ? b : a, y = sw ? a : b;
    a = x; b = y;
}

// H = U S V^T (any positive multiple of X0^T Y0)  ->  R = V U^T with det R = +1 (r_ik, row-major) and ssum = s0 + s1 +- s2.
// V comes from 8 cyclic Jacobi sweeps on H^T H; the two leading right vectors give u_i = H v_i / s_i; the third pair is
// v2 = v0 x v1, u2 = u0 x u1.  With both triples right-handed R = sum_i v_i u_i^T has det +1 -- the matrix a reference obtains after
// flipping the last singular vector when det < 0 -- and the signed third singular value is u2 . H v2 (= det-sign * s2, and 0 for a
// planar pose, whose third vectors a division could not give).
__device__ __forceinline__ void pe_rotation(double h00, double h01, double h02, double h10, double h11, double h12, double h20, double h21,
                                            double h22, double& ssum, double& r00, double& r01, double& r02, double& r10, double& r11,
                                            double& r12, double& r20, double& r21, double& r22) {
    // ---- A = H^T H = V S^2 V^T by cyclic Jacobi; V = (v_ij), column j the j-th right singular vector
    double a00 = h00 * h00 + h10 * h10 + h20 * h20, a01 = h00 * h01 + h10 * h11 + h20 * h21, a02 = h00 * h02 + h10 * h12 + h20 * h22;
    double a11 = h01 * h01 + h11 * h11 + h21 * h21, a12 = h01 * h02 + h11 * h12 + h21 * h22, a22 = h02 * h02 + h12 * h12 + h22 * h22;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int sweep = 0; sweep < 8; ++sweep) {
        pe_jacobi(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        pe_jacobi(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        pe_jacobi(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    // the two largest eigenvalues first (a compare with NaN swaps nothing)
    bool sw = a00 < a11;
    pe_swap_if(sw, a00, a11); pe_swap_if(sw, v00, v01); pe_swap_if(sw, v10, v11); pe_swap_if(sw, v20, v21);
    sw = a00 < a22;
    pe_swap_if(sw, a00, a22); pe_swap_if(sw, v00, v02); pe_swap_if(sw, v10, v12); pe_swap_if(sw, v20, v22);
    sw = a11 < a22;
    pe_swap_if(sw, a11, a22); pe_swap_if(sw, v01, v02); pe_swap_if(sw, v11, v12); pe_swap_if(sw, v21, v22);
    // v0, v1 unit and orthogonal to rounding; v2 = v0 x v1
    v02 = v10 * v21 - v20 * v11;
    v12 = v20 * v01 - v00 * v21;
    v22 = v00 * v11 - v10 * v01;
    // u0 = H v0 / s0,  u1 = H v1 / s1 (orthogonalised against u0),  u2 = u0 x u1
    double u00 = h00 * v00 + h01 * v10 + h02 * v20, u10 = h10 * v00 + h11 * v10 + h12 * v20, u20 = h20 * v00 + h21 * v10 + h22 * v20;
    const double sv0 = sqrt(u00 * u00 + u10 * u10 + u20 * u20);
    u00 /= sv0; u10 /= sv0; u20 /= sv0;
    double u01 = h00 * v01 + h01 * v11 + h02 * v21, u11 = h10 * v01 + h11 * v11 + h12 * v21, u21 = h20 * v01 + h21 * v11 + h22 * v21;
    const double dot = u00 * u01 + u10 * u11 + u20 * u21;
    u01 -= dot * u00; u11 -= dot * u10; u21 -= dot * u20;
    double sv1 = sqrt(u01 * u01 + u11 * u11 + u21 * u21);
    // rank one.  v1 is an eigenvector of H^T H, whose eigenvalues carry an error of 2^-52 lambda_0: at lambda_1 <= 2^-52 lambda_0, that is
    // s1 <= 2^-26 s0, v1 holds no information and H v1 is rounding noise or exactly 0 (a pose on a line, J = 2).  Then u1 is any unit
    // vector orthogonal to u0 -- u0 x e_k, k the axis of u0's smallest component, of length >= sqrt(2/3) before it is normalised -- and
    // s1 counts as 0.  Computed for every frame and selected: no branch.  Written as !(sv1 > thr * sv0), so that a NaN takes the
    // fallback and comes out of it as the NaN of u0.
    const double ax = fabs(u00), ay = fabs(u10), az = fabs(u20);
    const bool kx = ax <= ay && ax <= az, ky = ay <= az;
    double f0 = kx ? 0.0 : (ky ? -u20 : u10), f1 = kx ? u20 : (ky ? 0.0 : -u00), f2 = kx ? -u10 : (ky ? u00 : 0.0);
    const double fn = sqrt(f0 * f0 + f1 * f1 + f2 * f2);
    f0 /= fn; f1 /= fn; f2 /= fn;
    const bool rank_one = !(sv1 > 0x1p-26 * sv0);
    u01 = rank_one ? f0 : u01 / sv1; u11 = rank_one ? f1 : u11 / sv1; u21 = rank_one ? f2 : u21 / sv1;
    sv1 = rank_one ? 0.0 * sv0 : sv1;          // (0 * NaN = NaN)
    const double u02 = u10 * u21 - u20 * u11, u12 = u20 * u01 - u00 * u21, u22 = u00 * u11 - u10 * u01;
    const double w0 = h00 * v02 + h01 * v12 + h02 * v22, w1 = h10 * v02 + h11 * v12 + h12 * v22, w2 = h20 * v02 + h21 * v12 + h22 * v22;
    const double sv2 = u02 * w0 + u12 * w1 + u22 * w2;     // signed: negative when the best orthogonal map is a reflection
    ssum = sv0 + sv1 + sv2;
    // R = V U^T:  R[i][k] = sum_m v_im u_km
    r00 = v00 * u00 + v01 * u01 + v02 * u02; r01 = v00 * u10 + v01 * u11 + v02 * u12; r02 = v00 * u20 + v01 * u21 + v02 * u22;
    r10 = v10 * u00 + v11 * u01 + v12 * u02; r11 = v10 * u10 + v11 * u11 + v12 * u12; r12 = v10 * u20 + v11 * u21 + v12 * u22;
    r20 = v20 * u00 + v21 * u01 + v22 * u02; r21 = v20 * u10 + v21 * u11 + v22 * u12; r22 = v20 * u20 + v21 * u21 + v22 * u22;
}
