"""Restatements, inputs, gates and a CPU provider for in-the-wild mesh recovery (mbx_wild_mesh in csrc/smpl.hip, mbx_scale_fit and
mbx_wild_mesh_place in csrc/wild.hip, motionbert_amd.wild.infer_mesh / solve_scale / place).  Plain module, no fixtures:
tests/test_gpu_wild_mesh.py applies it to the kernels on the GPU, tests/test_wildmesherr.py to seeded corruptions on the CPU,
tests/test_wild_mesh.py runs `wild.infer_mesh` on the CPU provider; tools/mint_wild_mesh.py records what the reference's own `solve_scale`
finds on the seeded problems (tests/golden/wild_mesh.npz).  It imports tests/meshgterr.py and tests/smplerr.py and changes neither.

  fit_problem / points      seeded reference motions and keypoints; x = ref - ref[:, :1] in float64, y = kp - kp[:, :1] in float32, widened
  objective / fit_ref       `err` of infer_wild_mesh.py:42-43 in numpy float64, and its minimiser by iteratively reweighted least squares run
                            to a parameter change of 1e-16 (or 200,000 iterations).  The objective is a mean of norms of a function affine
                            in p: convex, one optimum; the reference's 400 starts of a Gauss-Newton solver look for that optimum.
  pair_ref / pair_gates     the paired mesh stage of infer_wild_mesh.py:115-141 on the plain path of tests/smplerr.py (rodrigues_plain,
                            plain_lbs) in a chosen dtype; the theta mean exactly, in float32 numpy
  place_eq                  infer_wild_mesh.py:153-154 in numpy 2's arithmetic, rounded to float32 once
  WildMeshOps               meshgterr.MockOps + wilderr.NumpyWildOps + `wild_mesh`, `scale_fit`, `wild_mesh_place` on CPU tensors, same
                            argument lists as HipOps; `wm_corrupt` plants one of CORRUPTIONS
  mesh_check / fit_check / place_check   the gates

Gates.  Single pass: equal bits with SMPLLayer.forward_kp on the same inputs, stitched.  Theta, placement: equal bits with the
restatement.  Pair mode, per output array: max |error| / max |float64 value| at most 4 x what the float32 plain path shows against itself
in float64 on the same inputs, never less than 8 fp32 ulps (the standing rule of tests/mesherr.py); nothing read off a kernel enters it.
Scale fit: (a) the float64 objective of the fitted (s, t) is no greater than the reference's own best `fun` (the fixture) plus the
evaluation's rounding bound N 2^-53 relative -- the reference's ranking criterion, a condition; (b) scale, t (relative to max |y|) and
objective within 1e-10 relative of fit_ref, the project's gate for its fp64 kernels; (c) pooled and single-track calls give equal bits."""
import math
import os

import numpy as np
import torch

from motionbert_amd.smpl import SMPLModel
from tests import meshgterr as MG
from tests import smplerr as SE
from tests import wilderr as WE

F32, F64 = torch.float32, torch.float64
SCALE = 1000.0
GATE64 = 1e-10
DELTA, TOL, CAP = 1e-12, 1e-13, 2000          # MBX_SCALE_FIT_DELTA / _TOL / _CAP of include/mbx.h (asserted in tests/test_wildmesherr.py)
GUARD = 2

CORRUPTIONS = ('pair_without_half', 'b_without_flip', 'b_shape_from_a', 'kp_before_scale', 'wrong_row', 'irls_3_iterations', 'irls_no_floor',
               'y_not_rootrel', 'place_root_joint_1', 'place_double_round')
MESH_CORRUPTIONS = CORRUPTIONS[:5]
FIT_CORRUPTIONS = CORRUPTIONS[5:8]
PLACE_CORRUPTIONS = CORRUPTIONS[8:]


# ------------------------------------------------------------------------------------------------ scale fit: problems
FIXTURE_PROBLEMS = ('p340', 'p1020', 'p17')                  # minted with the reference's solve_scale
PROBLEMS = FIXTURE_PROBLEMS + ('p119', 'exact')
LARGE = 'p17425'                                             # 1,025 frames: more points than one pass of a workgroup covers, whatever its stride
POOL = ('p17', None, 'p340', 'p1190')                        # four tracks pooled: lengths (1, 0, 20, 70)
_SPEC = {'p340': (20, 8401, True), 'p1020': (60, 8402, False), 'p17': (1, 8403, True), 'p119': (7, 8404, False), 'exact': (5, 8405, False),
         'p1190': (70, 8406, True), 'p17425': (1025, 8407, False), 'p84320': (4960, 8408, False)}       # the last: tools/wild_mesh_bench.py
ON_KINK = {'p340': False, 'p1020': True}


def fit_problem(name):
    """(ref [F,17,3] float64, kp [F,17,3] float32): a skeleton of about unit size walking through a room, and keypoints in millimetres =
    850 x + noise of 12 mm around their own root.  With an offset of the non-root joints the optimum lies off the kink t = 0 ('p340',
    'p17'); without it and with enough frames the root points (one in 17, each contributing exactly |t|) pin t to 0 ('p1020').
    'exact': kp = 2 ref rounded to float32 values that float64 doubles exactly: every residual is 0 at the optimum."""
    F, seed, offset = _SPEC[name]
    r = np.random.RandomState(seed)
    skel = r.normal(0, 0.25, (1, 17, 3)) + r.normal(0, 0.03, (F, 17, 3))
    ref = skel + np.cumsum(r.normal(0, 0.02, (F, 1, 3)), axis=0) + np.array([0.3, -0.2, 4.0])
    if name == 'exact':
        ref = np.round(ref * 64.0) / 64.0                    # a few mantissa bits: 2 x, and the root-relative differences, are exact in float32
        return ref, (2.0 * ref).astype(np.float32)
    x = ref - ref[:, :1]
    y = 850.0 * x + r.normal(0, 12.0, (F, 17, 3))
    if offset:
        y[:, 1:] += np.array([15.0, -10.0, 5.0])
    y[:, 0] = 0.0
    kp = (y + r.normal(0, 300.0, (F, 1, 3))).astype(np.float32)        # the regressed root is anywhere; the fit sees root-relative values
    return ref, kp


def points(ref, kp, corrupt=None):
    """(x [N,3], y [N,3]) float64 as infer_wild_mesh.py:150-152 forms them: ref float64, kp float32 (reg3d_all), N = 17 F"""
    ref, kp = np.asarray(ref, dtype=np.float64), np.asarray(kp, dtype=np.float32)
    x = ref - ref[:, :1]
    y = kp if corrupt == 'y_not_rootrel' else kp - kp[:, :1]
    assert y.dtype == np.float32
    return x.reshape(-1, 3), y.astype(np.float64).reshape(-1, 3)


def objective(s, t, x, y):
    """err(p, x, y) of infer_wild_mesh.py:42-43"""
    return float(np.linalg.norm(s * x + np.asarray(t, dtype=np.float64) - y, axis=-1).mean())


def _irls(x, y, tol, cap, floor, stop_after):
    """(s, t [3], objective, iterations, status): w = 1 / max(r, DELTA max|y|), first iteration w = 1, every iteration the weighted
    similarity fit in closed form from ten sums; stops on |ds| <= tol max(|s|, 1e-300) and |dt|_inf <= tol max|y|.  Status as mbx_scale_fit:
    0, -1 no points, -2 no extent, -3 cap reached."""
    nan3 = np.full(3, np.nan)
    if len(x) == 0:
        return np.nan, nan3, np.nan, 0, -1
    ymax = float(np.abs(y).max())
    delta = DELTA * ymax
    s, t = 0.0, np.zeros(3)
    for it in range(cap):
        r = np.linalg.norm(s * x + t - y, axis=-1)
        w = np.ones(len(x)) if it == 0 else 1.0 / (np.maximum(r, delta) if floor else r)
        W, Sx, Sy = w.sum(), w @ x, w @ y
        Sxx, Sxy = float(w @ (x * x).sum(-1)), float(w @ (x * y).sum(-1))
        den = Sxx - float(Sx @ Sx) / W
        if not den > 1e-12 * Sxx:
            return np.nan, nan3, np.nan, it, -2
        sn = (Sxy - float(Sx @ Sy) / W) / den
        tn = (Sy - sn * Sx) / W
        ds, dt = abs(sn - s), float(np.abs(tn - t).max())
        s, t = sn, tn
        if stop_after is not None and it + 1 >= stop_after:
            return s, t, objective(s, t, x, y), it + 1, 0
        if it > 0 and ds <= tol * max(abs(sn), 1e-300) and dt <= tol * ymax:
            return s, t, objective(s, t, x, y), it + 1, 0
    return np.nan, nan3, np.nan, cap, -3


def irls(x, y, tol, cap, floor=True, stop_after=None):
    with np.errstate(divide='ignore', invalid='ignore'):     # without the floor a zero residual divides by zero: the corruption's NaN
        return _irls(x, y, tol, cap, floor, stop_after)


_FIT_REF = {}


def fit_ref(name):
    """(s, t, objective, iterations) of a named problem: IRLS to a parameter change of 1e-16 or 200,000 iterations (computed once)"""
    if name not in _FIT_REF:
        x, y = points(*fit_problem(name))
        s, t, obj, it, status = irls(x, y, 1e-16, 200000)
        if status == -3:                                     # the last bits flip between neighbours: 200,000 iterations stand
            s, t, obj, it, status = irls(x, y, 1e-16, 200000, stop_after=200000)
        assert status == 0
        _FIT_REF[name] = (s, t, obj, it)
    return _FIT_REF[name]


def fit_row(ref, kp, corrupt=None):
    """[6] float64 = what mbx_scale_fit writes for one track"""
    if len(ref) == 0:
        return np.array([np.nan] * 5 + [-1.0])
    x, y = points(ref, kp, corrupt)
    s, t, obj, it, status = irls(x, y, TOL, CAP, floor=corrupt != 'irls_no_floor', stop_after=3 if corrupt == 'irls_3_iterations' else None)
    if status < 0 or not np.isfinite([s, obj]).all():
        return np.array([np.nan] * 5 + [float(status if status < 0 else -3)])
    return np.array([s, t[0], t[1], t[2], obj, float(it)])


def fit_check(row, name, fixture=None):
    """dict of one fitted row [6] against a named problem: `b` = the worst of |s - s*| / |s*|, |t - t*|_inf / max|y|, |obj - obj*| / obj*
    over GATE64 (obj* = 0: absolute, against max|y|); `a` = (objective of (s, t) in numpy float64 - the reference's best fun) over the
    rounding bound, where the fixture has the problem (must be <= 1: no greater than the reference's best plus the bound)"""
    x, y = points(*fit_problem(name))
    s0, t0, o0, _ = fit_ref(name)
    ymax = float(np.abs(y).max())
    if not (np.isfinite(row).all() and row[5] >= 1):
        return dict(b=math.inf, a=math.inf, iterations=row[5])
    s, t, obj = row[0], row[1:4], row[4]
    ob = abs(obj - o0) / o0 if o0 > 1e-9 * ymax else abs(obj - o0) / ymax
    res = dict(b=max(abs(s - s0) / abs(s0), float(np.abs(t - t0).max()) / ymax, ob) / GATE64, iterations=int(row[5]), a=None)
    if fixture is not None and f'{name}.fun' in fixture:
        fun = float(fixture[f'{name}.fun'])
        mine = objective(s, t, x, y)
        res['a'] = (mine - fun) / (len(x) * 2.0 ** -53 * fun)
        res['below_reference'] = (fun - mine) / fun
    return res


def fit_passes(res):
    return res['b'] <= 1.0 and (res['a'] is None or res['a'] <= 1.0)


def load_fixture():
    from tests.helpers import GOLDEN
    return np.load(os.path.join(GOLDEN, 'wild_mesh.npz'), allow_pickle=False)


# ------------------------------------------------------------------------------------------------ placement
def place_eq(verts, kp, ref, scales, lens, corrupt=None):
    """infer_wild_mesh.py:153-154 per track in numpy 2's arithmetic: the float32 difference verts - kp[:, :1] is added to the float64
    root_cam = ref[:, :1] * scale; the float64 sum is rounded to float32 once"""
    verts, kp, ref = np.asarray(verts, dtype=np.float32), np.asarray(kp, dtype=np.float32), np.asarray(ref, dtype=np.float64)
    out, at = np.empty_like(verts), 0
    for n, sc in zip(lens, scales):
        v, k, r = verts[at:at + n], kp[at:at + n], ref[at:at + n]
        root = k[:, 1:2] if corrupt == 'place_root_joint_1' else k[:, :1]
        root_cam = r[:, :1] * np.float64(sc)
        if corrupt == 'place_double_round':
            out[at:at + n] = (v - root) + root_cam.astype(np.float32)
        else:
            d = v - root
            assert d.dtype == np.float32
            out[at:at + n] = (d + root_cam).astype(np.float32)
        at += n
    return out


# ------------------------------------------------------------------------------------------------ the paired mesh stage
def theta_pair(theta_a, theta_b, corrupt=None):
    """[nT,82] float32 numpy: (theta_a + [flip_thetas(pose_b) | shape_b]) * 0.5 with every operation rounded in float32, and the flipped
    theta of pass B itself"""
    tb = np.asarray(theta_b, dtype=np.float32)
    pose = tb[:, :72].reshape(-1, 24, 3)
    back = np.concatenate([(pose if corrupt == 'b_without_flip' else MG.flip_thetas(pose)).reshape(-1, 72), tb[:, 72:]], axis=1).astype(np.float32)
    mean = (np.asarray(theta_a, dtype=np.float32) + back) * np.float32(0.5)
    assert mean.dtype == np.float32
    return mean, back


def pair_ref(model, case, dtype, pair=True, scale=SCALE):
    """(verts [nT,V,3], kp [nT,K,3]) in `dtype` on the plain path from the fp32 bits of the case: pass A from rot_a / betas_a, pass B from
    flip_thetas + rodrigues_plain of theta_b and its shape, each `* scale`, the regressor, then (a + b) * 0.5"""
    m = SE.model_dict(model, dtype)
    Q = model.J_regressor_h36m.to(dtype)
    nT = case['betas_a'].shape[0]

    def one(betas, rot):
        v = SE.plain_lbs(m, betas, rot)[0] * scale
        return v, torch.matmul(Q[None].expand(nT, -1, -1), v)
    va, ka = one(case['betas_a'].to(dtype), case['rot_a'].to(dtype))
    if not pair:
        return va, ka
    back = torch.from_numpy(theta_pair(case['theta_a'].numpy(), case['theta_b'].numpy())[1]).to(dtype)
    vb, kb = one(back[:, 72:], SE.rodrigues_plain(back[:, :72].reshape(-1, 3)).reshape(nT, 24, 3, 3))
    return (va + vb) * 0.5, (ka + kb) * 0.5


def pair_gates(model, case, pair=True):
    """(ref64, gate) per array: the float64 plain path and 4 x the stat of the float32 plain path against it (floor 8 ulps)"""
    v64, k64 = pair_ref(model, case, F64, pair)
    v32, k32 = pair_ref(model, case, F32, pair)
    return dict(verts=v64, kp=k64), dict(verts=SE.gate32(SE.stat(v32, v64)), kp=SE.gate32(SE.stat(k32, k64)))


def mesh_case(V, n, T, seed, model=None):
    """seeded inputs of mbx_wild_mesh for n clips of T frames: rot_a [nT,24,3,3], betas_a [nT,10], theta_a [nT,82] (pass A), theta_b
    [nT,82] (pass B: the poses of meshgterr.inputs with their planted rows -- zero joints, a 1e-9 joint, rotations next to pi, a zero whose
    sign flips, the rest pose), destinations out of order with a gap of GUARD + 1 rows, F rows"""
    g = torch.Generator().manual_seed(seed)
    nT = n * T
    pose, shape, _ = MG.inputs(n, T, seed + 1)
    inp = SE.inputs(nT, V, 17, seed + 2)
    slots = np.roll(np.arange(n)[::-1], seed % n if n > 2 else 0)          # never in order for n >= 2
    gap = GUARD + 1
    dst = (slots * T + np.where(slots >= (n + 1) // 2, gap, 0)).astype(np.int32)
    return dict(model=model if model is not None else SMPLModel.synthetic(V, seed), n=n, T=T, F=nT + gap, dst=dst, rot_a=inp['rot'], betas_a=inp['betas'],
                theta_a=torch.cat([0.4 * torch.randn(nT, 72, generator=g), inp['betas']], dim=1).float().contiguous(),
                theta_b=torch.cat([pose.reshape(nT, 72), shape.reshape(nT, 10)], dim=1).float().contiguous())


def stitch(rows, dst, T, F):
    """[F,...] with clip i of rows [nT,...] at dst[i], NaN elsewhere"""
    rows = np.asarray(rows.detach().cpu() if torch.is_tensor(rows) else rows)
    out = np.full((F,) + rows.shape[1:], np.nan, dtype=rows.dtype)
    for i, d in enumerate(dst):
        out[d:d + T] = rows[i * T:(i + 1) * T]
    return out


def run_mesh(ops, device, layer, case, pair, with_theta=True, with_verts=True, with_kp=True):
    """`ops.wild_mesh` straight into NaN-filled outputs with GUARD rows before and after -> dict verts / kp / theta on the host (None where
    not asked for) and `clean`: the guard rows untouched"""
    V, F, T = layer.num_vertices, case['F'], case['T']
    Q = layer.J_regressor_h36m.to(device)

    def buf(*tail):
        return torch.full((F + 2 * GUARD,) + tail, math.nan, dtype=F32, device=device)
    bufs = dict(verts=buf(V, 3) if with_verts else None, kp=buf(17, 3) if with_kp else None, theta=buf(82) if with_theta else None)
    view = {k: (None if b is None else b[GUARD:GUARD + F]) for k, b in bufs.items()}
    ops.wild_mesh(layer.model_tensors(), Q, case['rot_a'].to(device).reshape(-1, 24, 9).contiguous(), case['betas_a'].to(device),
                  case['theta_a'].to(device) if with_theta else None, case['theta_b'].to(device) if pair else None, SCALE,
                  torch.from_numpy(case['dst']).to(device), int(case['dst'].max()), T, view['verts'], view['kp'], view['theta'])
    out, clean = {}, True
    for k, b in bufs.items():
        if b is None:
            out[k] = None
            continue
        h = b.cpu()
        clean = clean and bool(torch.isnan(h[:GUARD]).all() and torch.isnan(h[GUARD + F:]).all())
        out[k] = h[GUARD:GUARD + F].numpy()
    out['clean'] = clean
    return out


def mesh_check(got, case, pair, single_bits=None, gates=None, report=None):
    """the list of failed gates of one run_mesh result.  Rows no clip lands on must still be NaN (compared as bits against the stitched
    restatement).  theta: bits.  Single pass (`single_bits`: dict verts / kp [nT,...] of SMPLLayer.forward_kp on the same provider): bits.
    Pair mode (`gates` = pair_gates(...)): stat / gate per array, recorded in `report`."""
    failed = [] if got['clean'] else ['guard']
    dst, T, F = case['dst'], case['T'], case['F']
    if got.get('theta') is not None:
        want = case['theta_a'].numpy() if not pair else theta_pair(case['theta_a'].numpy(), case['theta_b'].numpy())[0]
        if WE.differing(got['theta'], stitch(want, dst, T, F)):
            failed.append('theta')
    for name in ('verts', 'kp'):
        if got.get(name) is None:
            continue
        if not pair:
            if WE.differing(got[name], stitch(single_bits[name], dst, T, F)):
                failed.append(name)
            continue
        ref64, gate = gates
        want = stitch(ref64[name], dst, T, F)
        hole = np.isnan(want)
        if (np.isnan(got[name]) != hole).any():
            failed.append(name + '.rows')
            continue
        r = SE.stat(np.where(hole, 0.0, got[name]), np.where(hole, 0.0, want)) / gate[name]
        if report is not None:
            report[name] = r
        if not r <= 1.0:
            failed.append(name)
    return failed


# ------------------------------------------------------------------------------------------------ gate runs (CPU provider or the library)
def mesh_gate_run(ops, device, case, report=None, tag=''):
    """every gate of mbx_wild_mesh on one case -> the list of failed gates.  Single pass with every output and with the keypoints alone;
    pair mode with every output, with the vertices alone and with theta alone."""
    from motionbert_amd.smpl import SMPLLayer
    layer = SMPLLayer(case['model'], ops=ops).to(device)
    with torch.no_grad():
        v, k = layer.forward_kp(case['betas_a'].to(device), case['rot_a'].to(device), None, SCALE, ops=ops)
    bits = dict(verts=v.cpu().numpy(), kp=k.cpu().numpy())
    gates = pair_gates(case['model'], case)
    failed = []
    for pair, part, kw in ((False, '', {}), (False, '.kp', dict(with_theta=False, with_verts=False)), (True, '', {}),
                           (True, '.verts', dict(with_theta=False, with_kp=False)), (True, '.theta', dict(with_verts=False, with_kp=False))):
        rep = {}
        got = run_mesh(ops, device, layer, case, pair, **kw)
        name = ('pair' if pair else 'single') + part
        failed += [f'{name}.{f}' for f in mesh_check(got, case, pair, single_bits=bits, gates=gates, report=rep)]
        if report is not None:
            report.update({f'{tag}{name}.{k}': v for k, v in rep.items()})
    return failed


def run_fit(ops, device, ref, kp, lens):
    """`ops.scale_fit` straight into a NaN-filled fit with a guard row on either side -> fit [S,6] on the host (asserts the guards)"""
    S = len(lens)
    buf = torch.full((S + 2, 6), math.nan, dtype=F64, device=device)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(device)
    ops.scale_fit(torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64)).to(device),
                  torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float32)).to(device), ptr, buf[1:-1])
    h = buf.cpu().numpy()
    assert np.isnan(h[0]).all() and np.isnan(h[-1]).all(), 'guard rows of fit written'
    return h[1:-1]


def pool_problem():
    """(ref, kp, lens) of the tracks POOL one after another"""
    parts = [(np.zeros((0, 17, 3)), np.zeros((0, 17, 3), np.float32)) if n is None else fit_problem(n) for n in POOL]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), [len(p[0]) for p in parts]


def no_extent_problem():
    """a reference motion whose joints all sit on the root: sum w |x - xbar|^2 = 0"""
    ref, kp = fit_problem('p119')
    return np.repeat(ref[:, :1], 17, axis=1), kp


def fit_gate_run(ops, device, fixture, names=PROBLEMS, report=None):
    """gates (a), (b) on the named problems, (c) pooled against single-track calls, and the statuses -> the list of failed gates"""
    failed = []
    for name in names:
        ref, kp = fit_problem(name)
        res = fit_check(run_fit(ops, device, ref, kp, [len(ref)])[0], name, fixture)
        if report is not None:
            report[f'fit.{name}'] = res
        if not fit_passes(res):
            failed.append(f'fit.{name}')
    ref, kp, lens = pool_problem()
    pooled = run_fit(ops, device, ref, kp, lens)
    at = 0
    for i, n in enumerate(lens):
        single = run_fit(ops, device, ref[at:at + n], kp[at:at + n], [n])
        if WE.differing(pooled[i:i + 1], single):
            failed.append(f'pool.{i}')
        at += n
    if not (pooled[1, 5] == -1 and np.isnan(pooled[1, :5]).all()):
        failed.append('status.empty')
    if not all(pooled[i, 5] >= 1 and np.isfinite(pooled[i]).all() for i in (0, 2, 3)):
        failed.append('pool.values')
    row = run_fit(ops, device, *no_extent_problem(), [7])[0]
    if not (row[5] == -2 and np.isnan(row[:5]).all()):
        failed.append('status.no_extent')
    return failed


def place_problem(V=65, seed=8450):
    """two tracks of 3 and 4 frames with different scales: (verts [7,V,3] f32, kp [7,17,3] f32, ref [7,17,3] f64, lens, fit [2,6])"""
    r = np.random.RandomState(seed)
    lens = [3, 4]
    verts = r.normal(0, 400.0, (7, V, 3)).astype(np.float32)
    kp = r.normal(0, 300.0, (7, 17, 3)).astype(np.float32)
    ref = r.normal(0, 0.5, (7, 17, 3)) + np.array([0.3, -0.2, 4.0])
    fit = np.zeros((2, 6))
    fit[:, 0], fit[:, 5] = [851.2884185745156, 1203.7170361], 10
    return verts, kp, ref, lens, fit


def place_gate_run(ops, device, V=65):
    """mbx_wild_mesh_place against place_eq: differing elements (bits), guard rows included"""
    verts, kp, ref, lens, fit = place_problem(V)
    buf = torch.full((7 + 2 * GUARD, V, 3), math.nan, dtype=F32, device=device)
    buf[GUARD:GUARD + 7] = torch.from_numpy(verts).to(device)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(device)
    ops.wild_mesh_place(buf[GUARD:GUARD + 7], torch.from_numpy(kp).to(device), torch.from_numpy(ref).to(device), ptr, torch.from_numpy(fit).to(device))
    h = buf.cpu().numpy()
    want = np.full_like(h, np.nan)
    want[GUARD:GUARD + 7] = place_eq(verts, kp, ref, fit[:, 0], lens)
    return WE.differing(h, want)


# ------------------------------------------------------------------------------------------------ a kernel provider on the CPU
class WildMeshOps(MG.MockOps):
    """meshgterr.MockOps plus `wild_input` / `wild_output` (wilderr.NumpyWildOps) and the three entries of in-the-wild mesh recovery on CPU
    tensors, same argument lists as HipOps: the body from smplerr.forward_eq in float32 (the model of the chain and vertex kernels) on
    meshgterr._rodrigues32, the fit from irls, the placement from place_eq.  `wm_corrupt` plants one of CORRUPTIONS."""

    def __init__(self, wm_corrupt=None):
        super().__init__()
        assert wm_corrupt is None or wm_corrupt in CORRUPTIONS
        self.wm_corrupt = wm_corrupt
        self.wild = WE.NumpyWildOps()
        self.mesh_calls = []

    def wild_input(self, *a):
        return self.wild.wild_input(*a)

    def wild_output(self, *a):
        return self.wild.wild_output(*a)

    def wild_mesh_ws(self, nT, V, K, pair, device):
        return torch.empty(16, dtype=torch.uint8)

    def wild_mesh(self, model, Q, rotmat_a, betas_a, theta_a, theta_b, scale, dst_frames, dst_max, T, verts, kp, theta, ws=None):
        self._count('wild_mesh')
        c = self.wm_corrupt
        nT, n = betas_a.shape[0], dst_frames.numel()
        assert dst_frames.dtype == torch.int32 and n * T == nT and betas_a.dtype == F32 and rotmat_a.dtype == F32
        self.mesh_calls.append((n, T, theta_b is not None))
        dst = dst_frames.numpy().copy()
        out_rows = (verts if verts is not None else kp if kp is not None else theta).shape[0]
        assert n == 0 or (int(dst.max()) == int(dst_max) and int(dst_max) + T <= out_rows)
        if c == 'wrong_row' and n >= 2:
            dst = np.roll(dst, 1)
        s = float(np.float32(scale))
        m = self._m(model)
        half = 1.0 if c == 'pair_without_half' else 0.5
        va, ka, _ = SE.forward_eq(m, betas_a, rotmat_a.reshape(nT, 24, 3, 3), Q, s)
        th = None if theta_a is None else theta_a.numpy()
        if theta_b is not None:
            mean, back = theta_pair(theta_b.numpy() if th is None else th, theta_b.numpy(), c)
            back = torch.from_numpy(back)
            betas_b = betas_a if c == 'b_shape_from_a' else back[:, 72:].contiguous()
            vb, kb, _ = SE.forward_eq(m, betas_b, MG._rodrigues32(back[:, :72].reshape(-1, 3)).reshape(nT, 24, 3, 3), Q, s)
            va = (va + vb) * half
            ka = (ka + kb / s) * half if c == 'kp_before_scale' else (ka + kb) * half
            th = mean if th is not None else None
        for i, d in enumerate(dst):
            d = int(d)
            if verts is not None:
                verts[d:d + T] = va[i * T:(i + 1) * T]
            if kp is not None:
                kp[d:d + T] = ka[i * T:(i + 1) * T]
            if theta is not None:
                theta[d:d + T] = torch.from_numpy(np.ascontiguousarray(th[i * T:(i + 1) * T]))

    def scale_fit(self, ref, kp, seq_ptr, fit):
        self._count('scale_fit')
        assert ref.dtype == F64 and kp.dtype == F32 and seq_ptr.dtype == torch.int32 and fit.dtype == F64
        ptr = seq_ptr.numpy()
        c = self.wm_corrupt if self.wm_corrupt in FIT_CORRUPTIONS else None
        for s in range(len(ptr) - 1):
            fit[s] = torch.from_numpy(fit_row(ref.numpy()[ptr[s]:ptr[s + 1]], kp.numpy()[ptr[s]:ptr[s + 1]], c))

    def wild_mesh_place(self, verts, kp, ref, seq_ptr, fit):
        self._count('wild_mesh_place')
        assert verts.dtype == F32 and kp.dtype == F32 and ref.dtype == F64 and fit.dtype == F64
        ptr = seq_ptr.numpy()
        c = self.wm_corrupt if self.wm_corrupt in PLACE_CORRUPTIONS else None
        verts.copy_(torch.from_numpy(place_eq(verts.numpy(), kp.numpy(), ref.numpy(), fit[:, 0].numpy(), np.diff(ptr), c)))


# ------------------------------------------------------------------------------------------------ the loop of infer_wild_mesh.py
def reference_loop(model, smpl, motion, clip_len, flip, ref_pose=None, scale=None):
    """infer_wild_mesh.py:108-154 on `motion` = WildDetDataset.vid_all [F,17,3] float32 through `model` (a MeshRegressor whose forward runs
    its own SMPL layer) and `smpl` (called with pose2rot=True for the flipped pass): batch 1, two forwards per clip, np.hstack +
    np.concatenate.  `scale`: what solve_scale returned (the fit itself is gated on its own).  Returns (verts_all, reg3d_all).
    (*) ONE deviation from the file: infer_wild_mesh.py:129-134 regresses the flipped pass's joints from its vertices in METRES and averages
    them with the first pass's joints in millimetres; train_mesh.py:97-99, which the block was copied from, scales first.  The scaled form
    is the one restated here and computed by mbx_wild_mesh ('kp_before_scale' plants the other)."""
    from motionbert_amd.mesh import flip_input, flip_thetas_batch
    verts_all, reg3d_all = [], []
    J_regressor = smpl.J_regressor_h36m
    with torch.no_grad():
        for index in range(math.ceil(len(motion) / clip_len)):
            batch_input = torch.from_numpy(motion[index * clip_len:min((index + 1) * clip_len, len(motion))])[None]
            batch_size, clip_frames = batch_input.shape[:2]
            output = model(batch_input)
            if flip:
                output_flip = model(flip_input(batch_input))
                output_flip_pose = flip_thetas_batch(output_flip[0]['theta'][:, :, :72]).reshape(-1, 72)
                output_flip_shape = output_flip[0]['theta'][:, :, 72:].reshape(-1, 10)
                output_flip_smpl = smpl(betas=output_flip_shape, body_pose=output_flip_pose[:, 3:], global_orient=output_flip_pose[:, :3], pose2rot=True)
                output_flip_verts = output_flip_smpl.vertices.detach() * 1000.0                      # (*)
                output_flip_kp3d = torch.matmul(J_regressor[None, :].expand(output_flip_verts.shape[0], -1, -1), output_flip_verts)
                back = {'verts': output_flip_verts.reshape(batch_size, clip_frames, -1, 3),
                        'kp_3d': output_flip_kp3d.reshape(batch_size, clip_frames, -1, 3)}
                output = [{k: (output[0][k] + v) / 2.0 for k, v in back.items()}]
            verts_all.append(output[0]['verts'].cpu().numpy())
            reg3d_all.append(output[0]['kp_3d'].cpu().numpy())
    verts_all = np.concatenate(np.hstack(verts_all))
    reg3d_all = np.concatenate(np.hstack(reg3d_all))
    if ref_pose is not None:
        root_cam = ref_pose[:, :1] * scale
        verts_all = verts_all - reg3d_all[:, :1] + root_cam
    return verts_all, reg3d_all
