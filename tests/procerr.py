"""The Procrustes solver outside the region its fixtures guarantee (csrc/pose_solve.h: pe_rotation, behind Protocol #2 of mbx_pose_errors
and PA-MPJPE / PA-MPJPE-14 of mbx_mesh_errors): a model of the routine, input families from well conditioned to rank one, and the gate.
Plain module, no fixtures, no GPU: tests/test_procerr.py applies it to the model and its corruptions on the CPU, tests/test_gpu_procrustes.py
to the kernels.

  rotation_model         pe_rotation in numpy float64, batched over frames, operation for operation: the three pe_jacobi calls of a sweep,
                         8 sweeps, the three compare-swaps, v2 = v0 x v1, the single orthogonalisation, the rank-one guard, the signed sv2.
                         (mesherr._align_model takes its right vectors from np.linalg.eigh and so cannot show what a Jacobi sweep or a
                         missing guard does; it calls rank_one_guard below, so that the two models cannot drift.)
  p_mpjpe_model          e2 as pose_errors_kernel forms it: H = X0^T Y0 / (|X0| |Y0|), a = ssum |X0| / |Y0|
  rigid_align_model      e2 as mbx_mesh_errors forms it: H = X0^T Y0 / |Y0|^2, c = ssum
  reference_pose / reference_mesh   the reference on its LAPACK route: eval_fixture.NumpyOps.pose_errors and mesherr.rigid_align64
  families / cases       named seeded inputs (pred, gt) [203,J,3], fp32-representable, with reference, singular values and gate
  gate / ratios          the allowed |e2 - e2_ref| per frame, and the measured / allowed ratio (inf where e2 is not finite)

The gate.  X = gt, Y = pred, X0 / Y0 centred, nx = |X0|, H = X0^T Y0 / (|X0| |Y0|) with singular values s0 >= s1 >= s2, a the reference's
scale, sigma_i(.) the singular values of a centred pose [J,3].  All of it is numpy float64 on the inputs, nothing comes from the code
under test:

    floor   = GATE * max(e2_ref, nx / sqrt(J))                         GATE = 1e-10, the gate of mbx_pose_errors (tests/eval_fixture.py)
    B_X     = (2 s1 nx + 2 hypot(sigma_1(X0), sigma_2(X0))) / sqrt(J)
    B_Y     = (2 s1 nx + 2 a hypot(sigma_1(Y0), sigma_2(Y0))) / sqrt(J)
    allowed = floor                        where s1 / s0 >= 1e-3
            = floor + min(B_X, B_Y)        below

Above s1 / s0 = 1e-3 the squaring in H^T H costs at most six of the sixteen digits of the two trailing right vectors, and 1e-10 of the
larger of the error and the rms joint distance from the centroid (nx / sqrt(J): an error of exactly 0, pred == gt, has nothing else to be
relative to) is what tests/test_gpu_evaluate.py derives for a correct fp64 kernel.  Below it the eigenvalues lambda_1, lambda_2 of H^T H
sink towards the rounding error of lambda_0 and the solver can lose the roll about the leading axis.  What it still owes: v0 and u0 right
(lambda_0 is well separated), R orthogonal with det +1, and a scale off by at most the singular values it may miss.  Then its map
differs from the optimal one by an isometry of the planes transverse to u0 / v0 and by the scale:
  * the isometry moves the image of a joint by at most 2 |y_T| a, or, seen from the target's side (turn the target's transverse part
    instead), the residual by at most 2 |x_T|; the mean over the joints of |x_T| is at most rms |x_T| = hypot(sigma_1, sigma_2)(X0) /
    sqrt(J), the transverse plane being, to O(s1), the plane of the two trailing singular directions of the pose; likewise for Y0 with a;
  * ssum is off by at most |s1| + |s2| <= 2 s1, the scale by 2 s1 nx / ny, a joint's image by that times |y0|, whose rms is ny / sqrt(J):
    2 s1 nx / sqrt(J).
The smaller of the two sides holds.  B is 0 for an exactly collinear pose (sigma_1 = sigma_2 = 0 there and s1 = 0): any roll is as good
as the reference's, and the floor alone applies.  B holds only for a solver whose R is a proper rotation; a u1 that is NaN or that leans
on u0 breaks exactly that, which is what the families `line.*` and `J2.*` are for.

Zero-extent poses stay out: there the reference divides 0 by 0 (pose_eval.hip's header; mesherr's planted frame 2 tests it) and LAPACK
raises on the NaN matrix.

The issue's list has one more corruption, `one_orthogonalisation_unchecked`, for a fix that adds a second orthogonalisation.  The fix
is the guard alone (the model passes every family with it, tests/test_procerr.py), so there is no second step to leave out."""
import collections
import functools
import math

import numpy as np
import torch

from tests import eval_fixture as FX

GATE = FX.GATE
FRAMES = 203                      # no multiple of 64
WELL = 1e-3                       # s1 / s0 from which the floor alone applies
RANK_ONE = 2.0 ** -26             # pe_rotation's guard: s1 / s0 at which lambda_1 <= 2^-52 lambda_0 and v1 carries no information
NEEDLE_EPS = ('1e-2', '1e-4', '1e-6', '1e-8')
CORRUPTIONS = ('no_rank_one_guard', 'unsigned_s2', 'no_sort', 'two_sweeps', 'third_by_division')
# the families on which tests/test_procerr.py requires each corruption to fail, and how ('nan': a frame that is not finite)
CAUGHT_BY = {'no_rank_one_guard': (('line.pred.axis', 'nan'), ('line.gt.axis', 'nan'), ('J2.axis', 'nan'), ('line.gt.oblique', 'value')),
             'unsigned_s2': (('mirrored', 'value'), ('J4', 'value')),
             'no_sort': (('mirrored', 'value'), ('planar.gt', 'value'), ('line.pred.axis', 'nan')),
             'two_sweeps': (('conditioned', 'value'), ('equal.cube', 'value')),
             'third_by_division': (('planar.both', 'nan'), ('mirrored', 'value'))}


# ------------------------------------------------------------------------------------------------ the model of pe_rotation
def _jacobi(app, aqq, apq, apr, aqr, V, p, q):
    """pe_jacobi: one rotation in the (p, q) plane; V [F,3,3] follows in its columns p and q (in place).  Returns app, aqq, apq, apr, aqr."""
    theta = (aqq - app) / (2.0 * apq)
    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    t = np.where(theta < 0.0, -t, t)
    t = np.where(apq == 0.0, 0.0, t)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    a, b = V[:, :, p].copy(), V[:, :, q].copy()
    V[:, :, p] = c[:, None] * a - s[:, None] * b
    V[:, :, q] = s[:, None] * a + c[:, None] * b
    return app - t * apq, aqq + t * apq, np.zeros_like(apq), c * apr - s * aqr, s * apr + c * aqr


def _swap_if(sw, lam, V, i, j):
    li, lj = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
    lam[i], lam[j] = li, lj
    vi, vj = np.where(sw[:, None], V[:, :, j], V[:, :, i]), np.where(sw[:, None], V[:, :, i], V[:, :, j])
    V[:, :, i], V[:, :, j] = vi, vj


def _norm(u):
    return np.sqrt(u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1] + u[..., 2] * u[..., 2])


def rank_one_guard(u0, u1, sv0, sv1):
    """pe_rotation's guard, for one frame or a batch (u0 unit, u1 = H v1 orthogonalised against u0 and not yet normalised, sv1 = |u1|):
    (u1 / sv1, sv1) where sv1 > 2^-26 sv0; elsewhere (the unit vector u0 x e_k, k the axis of u0's smallest component; 0).  Written as
    not (sv1 > thr sv0): a NaN takes the second branch and comes back as NaN from u0."""
    u0, u1, sv0, sv1 = np.asarray(u0), np.asarray(u1), np.asarray(sv0), np.asarray(sv1)
    ax, ay, az = np.abs(u0[..., 0]), np.abs(u0[..., 1]), np.abs(u0[..., 2])
    zero = np.zeros_like(ax)
    kx, ky = (ax <= ay) & (ax <= az), ay <= az
    f = np.where(kx[..., None], np.stack([zero, u0[..., 2], -u0[..., 1]], -1),
                 np.where(ky[..., None], np.stack([-u0[..., 2], zero, u0[..., 0]], -1), np.stack([u0[..., 1], -u0[..., 0], zero], -1)))
    f = f / _norm(f)[..., None]
    deg = ~(sv1 > RANK_ONE * sv0)
    return np.where(deg[..., None], f, u1 / sv1[..., None]), np.where(deg, 0.0 * sv0, sv1)


def rotation_model(H, corrupt=None):
    """(ssum [F], R [F,3,3]) of H [F,3,3] float64 as pe_rotation computes them.  corrupt: one of CORRUPTIONS --
    'no_rank_one_guard' u1 = (H v1 - (u0 . H v1) u0) / its norm whatever that norm is (the code before the guard), 'unsigned_s2' |u2 . H v2|,
    'no_sort' the compare-swaps are left out, 'two_sweeps' 2 Jacobi sweeps instead of 8, 'third_by_division' u2 = H v2 / |H v2|, s2 = |H v2|."""
    assert corrupt is None or corrupt in CORRUPTIONS, corrupt
    H = np.array(H, np.float64).reshape(-1, 3, 3)
    with np.errstate(all='ignore'):
        h = lambda i, j: H[:, i, j]
        a00 = h(0, 0) * h(0, 0) + h(1, 0) * h(1, 0) + h(2, 0) * h(2, 0)
        a01 = h(0, 0) * h(0, 1) + h(1, 0) * h(1, 1) + h(2, 0) * h(2, 1)
        a02 = h(0, 0) * h(0, 2) + h(1, 0) * h(1, 2) + h(2, 0) * h(2, 2)
        a11 = h(0, 1) * h(0, 1) + h(1, 1) * h(1, 1) + h(2, 1) * h(2, 1)
        a12 = h(0, 1) * h(0, 2) + h(1, 1) * h(1, 2) + h(2, 1) * h(2, 2)
        a22 = h(0, 2) * h(0, 2) + h(1, 2) * h(1, 2) + h(2, 2) * h(2, 2)
        V = np.broadcast_to(np.eye(3), H.shape).copy()
        for _ in range(2 if corrupt == 'two_sweeps' else 8):
            a00, a11, a01, a02, a12 = _jacobi(a00, a11, a01, a02, a12, V, 0, 1)
            a00, a22, a02, a01, a12 = _jacobi(a00, a22, a02, a01, a12, V, 0, 2)
            a11, a22, a12, a01, a02 = _jacobi(a11, a22, a12, a01, a02, V, 1, 2)
        lam = [a00, a11, a22]
        if corrupt != 'no_sort':
            _swap_if(lam[0] < lam[1], lam, V, 0, 1)
            _swap_if(lam[0] < lam[2], lam, V, 0, 2)
            _swap_if(lam[1] < lam[2], lam, V, 1, 2)
        v0, v1 = V[:, :, 0], V[:, :, 1]
        v2 = np.stack([v0[:, 1] * v1[:, 2] - v0[:, 2] * v1[:, 1], v0[:, 2] * v1[:, 0] - v0[:, 0] * v1[:, 2],
                       v0[:, 0] * v1[:, 1] - v0[:, 1] * v1[:, 0]], -1)
        mul = lambda v: np.stack([h(i, 0) * v[:, 0] + h(i, 1) * v[:, 1] + h(i, 2) * v[:, 2] for i in range(3)], -1)
        u0 = mul(v0)
        sv0 = _norm(u0)
        u0 = u0 / sv0[:, None]
        u1 = mul(v1)
        dot = u0[:, 0] * u1[:, 0] + u0[:, 1] * u1[:, 1] + u0[:, 2] * u1[:, 2]
        u1 = u1 - dot[:, None] * u0
        sv1 = _norm(u1)
        if corrupt == 'no_rank_one_guard':
            u1 = u1 / sv1[:, None]
        else:
            u1, sv1 = rank_one_guard(u0, u1, sv0, sv1)
        w = mul(v2)
        if corrupt == 'third_by_division':
            sv2 = _norm(w)
            u2 = w / sv2[:, None]
        else:
            u2 = np.stack([u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1], u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2],
                           u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]], -1)
            sv2 = u2[:, 0] * w[:, 0] + u2[:, 1] * w[:, 1] + u2[:, 2] * w[:, 2]
            if corrupt == 'unsigned_s2':
                sv2 = np.abs(sv2)
        ssum = sv0 + sv1 + sv2
        R = v0[:, :, None] * u0[:, None, :] + v1[:, :, None] * u1[:, None, :] + v2[:, :, None] * u2[:, None, :]      # R[i][k] = sum_m v_im u_km
    return ssum, R


def _centred(pred, gt):
    X, Y = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    return X - X.mean(1, keepdims=True), Y - Y.mean(1, keepdims=True)


def p_mpjpe_model(pred, gt, corrupt=None):
    """e2 [F] of pred, gt [F,J,3] as pose_errors_kernel forms it"""
    X0, Y0 = _centred(pred, gt)
    with np.errstate(all='ignore'):
        nx, ny = np.sqrt((X0 ** 2).sum((1, 2))), np.sqrt((Y0 ** 2).sum((1, 2)))
        ssum, R = rotation_model(np.matmul(X0.transpose(0, 2, 1), Y0) * (1.0 / (nx * ny))[:, None, None], corrupt)
        return _norm(np.matmul(Y0, (ssum * nx / ny)[:, None, None] * R) - X0).mean(-1)


def rigid_align_model(A, B, corrupt=None):
    """mean |aligned_j - B_j| [F] of A (prediction), B (target) [F,n,3] as mbx_mesh_errors forms it (poses of non-zero extent)"""
    X0, Y0 = _centred(A, B)
    with np.errstate(all='ignore'):
        ssum, R = rotation_model(np.matmul(X0.transpose(0, 2, 1), Y0) * (1.0 / (Y0 ** 2).sum((1, 2)))[:, None, None], corrupt)
        return _norm(np.matmul(Y0, ssum[:, None, None] * R) - X0).mean(-1)


# ------------------------------------------------------------------------------------------------ the reference (LAPACK route)
def reference_pose(pred, gt):
    """(e1, e2) [F] of pred, gt [F,J,3]: eval_fixture.NumpyOps.pose_errors (lib/model/loss.py:8-51 restated)"""
    F = len(pred)
    e1, e2 = torch.empty(F, 1, dtype=torch.float64), torch.empty(F, 1, dtype=torch.float64)
    FX.NumpyOps().pose_errors(torch.from_numpy(np.ascontiguousarray(pred))[:, None], torch.from_numpy(np.ascontiguousarray(gt))[:, None], None,
                              None, None, False, e1, e2)
    return e1.numpy().reshape(-1), e2.numpy().reshape(-1)


def reference_mesh(A, B):
    """mean |rigid_align(A, B)_j - B_j| [F] of A, B [F,n,3]: mesherr.rigid_align64 (utils_mesh.py:333-355 restated)"""
    from tests import mesherr as ME
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return np.array([np.sqrt(((ME.rigid_align64(a, b) - b) ** 2).sum(-1)).mean() for a, b in zip(A, B)])


# ------------------------------------------------------------------------------------------------ the gate
def spectrum(pred, gt):
    """(s [F,3] of the normalised H, sigma(X0) [F,3], sigma(Y0) [F,3], nx [F], a [F]) in numpy float64 (LAPACK); a pose of fewer than
    three joints has its missing singular values as 0"""
    X0, Y0 = _centred(pred, gt)
    nx, ny = np.sqrt((X0 ** 2).sum((1, 2))), np.sqrt((Y0 ** 2).sum((1, 2)))
    H = np.matmul(X0.transpose(0, 2, 1), Y0) / (nx * ny)[:, None, None]
    U, s, Vt = np.linalg.svd(H)
    # LAPACK returns some 5e-17 for the zero singular values of a matrix with a single non-zero row or column.  Rows and columns of H that
    # are exactly zero (a pose in a coordinate plane or along a coordinate axis) are taken out first: the other singular values stay what
    # they are and the zeros are exact.
    for f in np.nonzero(((H == 0).all(1) | (H == 0).all(2)).any(1))[0]:
        h = H[f][np.ix_((H[f] != 0).any(1), (H[f] != 0).any(0))]
        t = np.linalg.svd(h, compute_uv=False)
        s[f] = np.concatenate([t, np.zeros(3 - len(t))])
    d = np.sign(np.linalg.det(np.matmul(Vt.transpose(0, 2, 1), U.transpose(0, 2, 1))))
    a = (s[:, 0] + s[:, 1] + d * s[:, 2]) * nx / ny
    pad = lambda v: np.concatenate([v, np.zeros((len(v), 3 - v.shape[1]))], 1)
    return s, pad(np.linalg.svd(X0, compute_uv=False)), pad(np.linalg.svd(Y0, compute_uv=False)), nx, a


def gate(pred, gt, e2_ref):
    """the allowed |e2 - e2_ref| [F] (module docstring).  pred, gt [F,J,3]."""
    s, sx, sy, nx, a = spectrum(pred, gt)
    rj = math.sqrt(pred.shape[1])
    floor = GATE * np.maximum(np.asarray(e2_ref, np.float64), nx / rj)
    bx = (2.0 * s[:, 1] * nx + 2.0 * np.hypot(sx[:, 1], sx[:, 2])) / rj
    by = (2.0 * s[:, 1] * nx + 2.0 * a * np.hypot(sy[:, 1], sy[:, 2])) / rj
    return np.where(s[:, 1] >= WELL * s[:, 0], floor, floor + np.minimum(bx, by))


def ratios(e2, e2_ref, allowed):
    """|e2 - e2_ref| / allowed per frame; inf where e2 is not finite (the reference is finite on every frame of every family)"""
    e2, e2_ref = np.asarray(e2, np.float64).reshape(-1), np.asarray(e2_ref, np.float64).reshape(-1)
    assert e2.shape == e2_ref.shape == allowed.shape and np.isfinite(e2_ref).all() and bool((allowed > 0).all())
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(e2), np.abs(e2 - e2_ref) / allowed, np.inf)


# ------------------------------------------------------------------------------------------------ the families
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


def _rot(rng, n):
    """n proper rotations, uniformly turned"""
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    return Q * np.sign(np.linalg.det(Q))[:, None, None]


def _conditioned(rng, J, n=FRAMES):
    """the generator of tests/test_gpu_evaluate.py::test_other_joint_counts"""
    gt = np.rint(rng.standard_normal((n, J, 3)) * rng.uniform(50.0, 300.0, size=(n, 1, 3)))
    R = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    pred = np.rint((rng.uniform(0.7, 1.3, size=(n, 1, 1)) * np.matmul(gt, R) + rng.standard_normal((n, 1, 3)) * 100 + rng.standard_normal((n, J, 3)) * 40) * 16) / 16
    return pred, gt


def _line(rng, J, oblique, n=FRAMES):
    """exactly collinear poses: an integer parameter per joint times an integer direction (a coordinate axis, cycling with the frame, or an
    oblique one with all three components non-zero) plus an integer offset"""
    t = rng.integers(-300, 301, size=(n, J, 1)).astype(np.float64)
    t[:, 0, 0], t[:, 1, 0] = -150.0, 150.0                                   # never of zero extent
    if oblique:
        d = rng.integers(1, 10, size=(n, 1, 3)) * rng.choice([-1, 1], size=(n, 1, 3))
    else:
        d = np.eye(3)[np.arange(n) % 3][:, None, :]
    return t * d + rng.integers(-500, 501, size=(n, 1, 3))


def _needle(rng, J, eps, n=FRAMES):
    """(needle, counterpart): poses of 300 mm along one axis and 300 eps mm across it, turned by a random rotation; the counterpart of the
    first half is an ordinary pose, of the second half the needle itself plus 0.5 mm noise"""
    needle = np.matmul(rng.standard_normal((n, J, 3)) * np.array([300.0, 300.0 * eps, 300.0 * eps]), _rot(rng, n))
    fat = _conditioned(rng, J, n)[0]
    near = needle + 0.5 * rng.standard_normal((n, J, 3))
    return needle, np.where((np.arange(n) < n // 2)[:, None, None], fat, near)


def families():
    """{name: generator() -> (pred, gt) [203,J,3] float32}.  Seeded by the family's position in the list; every value fp32-representable, so
    that the kernel and the float64 reference read the same numbers."""
    out = collections.OrderedDict()

    def family(name):
        def reg(fn):
            seed = 7000 + len(out)
            out[name] = lambda: tuple(_f32(a) for a in fn(np.random.default_rng(seed)))
            return fn
        return reg

    family('conditioned')(lambda r: _conditioned(r, 17))

    @family('planar.gt')
    def _(r):
        p, g = _conditioned(r, 17)
        g[:, :, 2] = 0.0
        return p, g

    @family('planar.pred')
    def _(r):
        p, g = _conditioned(r, 17)
        p[:, :, 2] = 0.0
        return p, g

    @family('planar.both')
    def _(r):
        p, g = _conditioned(r, 17)
        p[:, :, 2], g[:, :, 2] = 0.0, 0.0
        return p, g

    @family('planar.both.mirrored')
    def _(r):
        g = _conditioned(r, 17)[1]
        g[:, :, 2] = 0.0
        p = g * np.array([-1.0, 1.0, 0.0]) + np.rint(5.0 * r.standard_normal(g.shape) * 16) / 16 * np.array([1.0, 1.0, 0.0])
        return p, g

    def mirrored(r, thin):
        g = _conditioned(r, 17)[1] * np.array([1.0, 1.0, thin])
        p = (g * np.array([-1.0, 1.0, 1.0]) + 5.0 * r.standard_normal(g.shape) * np.array([1.0, 1.0, thin]))
        return np.matmul(p, _rot(r, FRAMES)) + 100.0 * r.standard_normal((FRAMES, 1, 3)), g
    family('mirrored')(lambda r: mirrored(r, 1.0))
    family('mirrored.thin')(lambda r: mirrored(r, 1e-6))

    @family('equal.cube')
    def _(r):
        corners = np.array([[x, y, z] for x in (-100.0, 100.0) for y in (-100.0, 100.0) for z in (-100.0, 100.0)])
        g = np.matmul(np.broadcast_to(corners, (FRAMES, 8, 3)), _rot(r, FRAMES))
        return np.matmul(g, _rot(r, FRAMES)) + 3.0 * r.standard_normal(g.shape), g

    @family('equal.identity')
    def _(r):
        g = _conditioned(r, 17)[1]
        return g.copy(), g

    @family('similarity')
    def _(r):
        g = _conditioned(r, 17)[1]
        return 2.0 * np.matmul(g, _rot(r, FRAMES)) + 100.0 * r.standard_normal((FRAMES, 1, 3)), g

    @family('units.metres')
    def _(r):
        p, g = _conditioned(r, 17)
        return p * 1e-3, g * 1e-3

    @family('units.far')
    def _(r):
        p, g = _conditioned(r, 17)
        return p * 300.0 + 1e5, g * 300.0 + 1e5

    @family('collapsed')
    def _(r):
        p, g = _conditioned(r, 17)
        return 1000.0 + 1e-4 * p, g

    family('J2.random')(lambda r: _conditioned(r, 2))

    @family('J2.axis')
    def _(r):
        return _line(r, 2, False), _conditioned(r, 2)[1]

    def few(r, J):
        """three or four random joints are now and then almost collinear: such frames are drawn again (to the conditioning the fixture of
        mbx_pose_errors asserts, second singular value of H >= 0.01), the thin poses have families of their own"""
        p, g = _conditioned(r, J)
        for _ in range(64):
            s = spectrum(p, g)[0]
            bad = s[:, 1] < 0.01
            if not bad.any():
                return p, g
            p[bad], g[bad] = _conditioned(r, J, int(bad.sum()))
        raise AssertionError(f'J = {J}: could not draw {FRAMES} conditioned frames')
    family('J3')(lambda r: few(r, 3))
    family('J4')(lambda r: few(r, 4))

    @family('J64.planar')
    def _(r):
        p, g = _conditioned(r, 64)
        p[:, :, 2], g[:, :, 2] = 0.0, 0.0
        return p, g
    family('line.pred.axis')(lambda r: (_line(r, 17, False), _conditioned(r, 17)[1]))
    family('line.pred.oblique')(lambda r: (_line(r, 17, True), _conditioned(r, 17)[1]))
    family('line.gt.axis')(lambda r: (_conditioned(r, 17)[0], _line(r, 17, False)))
    family('line.gt.oblique')(lambda r: (_conditioned(r, 17)[0], _line(r, 17, True)))
    family('line.both')(lambda r: (_line(r, 17, True), _line(r, 17, True)))
    for eps in NEEDLE_EPS:
        family('needle.gt.' + eps)(lambda r, e=float(eps): _needle(r, 17, e)[::-1])
        family('needle.pred.' + eps)(lambda r, e=float(eps): _needle(r, 17, e))
    return out


def group(name):
    """the family group a report line speaks of"""
    head = name.split('.')[0]
    return head if head in ('line', 'needle', 'planar', 'mirrored', 'equal', 'units') else ('small J' if head[0] == 'J' else name)


Case = collections.namedtuple('Case', 'name pred gt e1_ref e2_ref allowed s')


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case} of every family, with the reference's errors, the gate and the singular values of the normalised H; the conditions the
    families owe are asserted here: conditions on the inputs and on the reference, not tolerances.  Built once, shared, never written to."""
    out = collections.OrderedDict()
    for name, make in families().items():
        pred, gt = make()
        assert pred.shape == gt.shape and pred.shape[0] == FRAMES and pred.dtype == np.float32, name
        e1, e2 = reference_pose(pred, gt)
        assert np.isfinite(e1).all() and np.isfinite(e2).all(), f'{name}: the reference is not finite on every frame'
        allowed = gate(pred, gt, e2)
        s = spectrum(pred, gt)[0]
        assert np.isfinite(allowed).all() and bool((allowed > 0).all()), f'{name}: a frame without a gate'
        cond = s[:, 1] / s[:, 0]
        if name.split('.')[0] not in ('line', 'needle', 'J2'):
            assert cond.min() >= WELL, f'{name}: s1 / s0 reaches {cond.min():.3e}'
        if name in ('line.pred.axis', 'line.gt.axis', 'J2.axis'):
            assert bool((s[:, 1] == 0.0).all()), f'{name}: s1 is not exactly 0 ({s[:, 1].max():.3e})'
        if name.startswith('needle.'):
            assert cond.min() < WELL, f'{name}: s1 / s0 stays above {cond.min():.3e}'
        for a in (pred, gt, e1, e2, allowed, s):
            a.setflags(write=False)
        out[name] = Case(name, pred, gt, e1, e2, allowed, s)
    return out


MESH_FAMILIES = ('planar.', 'mirrored.thin', 'equal.identity', 'line.', 'needle.')


def mesh_names():
    """the J = 17 families mbx_mesh_errors is run on"""
    return [n for n in families() if n.startswith(MESH_FAMILIES)]
