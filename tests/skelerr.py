"""The host reference of the skeleton rasteriser (csrc/skeleton.hip, motionbert_amd/render.py `render_skeleton`), its gates and its inputs.

Reference.  `project`: numpy float64 in the order include/mbx.h states (x + 1 in float32 first), every operation rounded on its own.
`raster`: per primitive over the samples of its bounding box, numpy int64; Python integers (object arrays) as soon as a coordinate lies outside
the guard or a cross product reaches 2^31, so that no product can wrap.  `RefOps` offers both as a kernel provider, so that the module runs on
the CPU.  `corrupt=` seeds one wrong convention into the reference (CORRUPTIONS): tests/test_skelerr.py shows that each one fails a gate.

Gates.  jq, prim_id and rgb: equal bits (`gate_equal`).  Nothing in the picture is floating point after the projection, and the projection is
float64 in a stated order, so there is no tolerance anywhere."""
from fractions import Fraction

import numpy as np
import torch

from motionbert_amd import render as R

SUB, GUARD, OUTSIDE, TILE = 16, 1 << 18, 1 << 30, 32
CORRUPTIONS = ('lt_cap', 'half_sample', 'priority_reversed', 'ring_swapped', 'no_v_flip', 'no_swap', 'no_divide', 'fma', 'plus_one_f64',
               'ss_no_round', 'sentinel_drawn', 'lr_swapped')


# ------------------------------------------------------------------------------------------------ reference: projection
def _fma(a, b, c):
    """a b + c with one rounding, element by element (exact rationals)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.empty(a.shape, np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))) if np.isfinite(a[i] * b[i] + c[i]) else a[i] * b[i] + c[i]
    return out


def project(x, view, S, corrupt=()):
    """x [F,J,3] f32, view: 15 float64 values -> jq [F,J,2] i32"""
    x = np.asarray(x, np.float32)
    m = [np.float64(v) for v in view]
    u_lo, v_hi, inv_w = m[12], m[13], m[14]
    scale = np.float64(S * SUB)
    with np.errstate(all='ignore'):
        if 'plus_one_f64' in corrupt:
            ax, ay = x[..., 0].astype(np.float64) + 1.0, x[..., 1].astype(np.float64) + 1.0
        else:
            ax, ay = (x[..., 0] + np.float32(1)).astype(np.float64), (x[..., 1] + np.float32(1)).astype(np.float64)
            assert (x[..., 0] + np.float32(1)).dtype == np.float32
        z = x[..., 2].astype(np.float64)
        px, py, pz = -256.0 * ax, -256.0 * z, -256.0 * ay
        if 'no_swap' in corrupt:
            py, pz = pz, py
        rows = []
        for r in range(3):
            a, b, c, d = m[4 * r:4 * r + 4]
            if 'fma' in corrupt and r == 0:          # U as a compiler would contract it: b py rounded, then two fused multiply-adds
                rows.append(_fma(c, pz, _fma(a, px, b * py)) + d)
            else:
                rows.append(((a * px + b * py) + c * pz) + d)
        U, V, W = rows
        u, v = (U, V) if 'no_divide' in corrupt else (U / W, V / W)
        fx = np.floor(((u - u_lo) * inv_w) * scale)
        fy = np.floor(((v - (v_hi - 1.0 / inv_w)) * inv_w) * scale) if 'no_v_flip' in corrupt else np.floor(((v_hi - v) * inv_w) * scale)
        ok = np.isfinite(x).all(-1) & (W > 0) & (np.abs(fx) <= GUARD) & (np.abs(fy) <= GUARD)
    out = np.full(x.shape[:2] + (2,), OUTSIDE, np.int32)
    out[..., 0] = np.where(ok, np.where(ok, fx, 0), OUTSIDE).astype(np.int32)
    out[..., 1] = np.where(ok, np.where(ok, fy, 0), OUTSIDE).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------ reference: raster
def _ceil_div(a, b):
    return -((-a) // b)


def _covered(px, py, dx, dy, r, lt_cap=False):
    """the capsule test of include/mbx.h for arrays px, py (int64, or object arrays of Python integers) and Python integers dx, dy, r"""
    dd, r2 = dx * dx + dy * dy, r * r
    pp = px * px + py * py
    t = px * dx + py * dy
    ex, ey = px - dx, py - dy
    cross = px * dy - py * dx
    if cross.dtype != object and cross.size and int(np.abs(cross).max()) >= 1 << 31:
        cross = cross.astype(object)                                         # the square would not fit int64
    side = cross * cross <= r2 * dd
    cap_a = (pp < r2) if lt_cap else (pp <= r2)
    return np.where(t <= 0, cap_a, np.where(t >= dd, ex * ex + ey * ey <= r2, side)).astype(bool), pp


def raster(jq, bones, colors, radii, size, ss, corrupt=()):
    """-> dict: prim_id [F,S,S] i32 (-1 where empty); sample [F,S,S,3] u8; rgb [F,size,size,3] u8"""
    jq = np.asarray(jq, np.int64)
    bones = np.asarray(bones, np.int64)
    colors = np.asarray(colors, np.uint8).copy()
    if 'lr_swapped' in corrupt:
        left, right = (colors == R.COLOR_LEFT).all(1), (colors == R.COLOR_RIGHT).all(1)
        colors[left], colors[right] = R.COLOR_RIGHT, R.COLOR_LEFT
    r_line, r_out, r_in = (int(r) for r in radii)
    F, J = jq.shape[:2]
    S = size * ss
    Nb = bones.shape[0]
    off = 0 if 'half_sample' in corrupt else SUB // 2
    key = np.full((F, S, S), -1, np.int64)                                   # 2 rank + (inside the marker's centre); rank rises with priority
    for f in range(F):
        K = key[f]
        for k in range(Nb):
            ia, ib = int(bones[k, 0]), int(bones[k, 1])
            if not (0 <= ia < J and 0 <= ib < J):
                continue
            a, b = [int(v) for v in jq[f, ia]], [int(v) for v in jq[f, ib]]
            wide = max(abs(v) for v in a + b) > GUARD
            if wide and 'sentinel_drawn' not in corrupt:
                continue
            for part in range(3):
                c = b if part == 2 else a
                dx, dy = (b[0] - a[0], b[1] - a[1]) if part == 0 else (0, 0)
                r = r_line if part == 0 else r_out
                j0, j1 = max(_ceil_div(min(c[0], c[0] + dx) - r - off, SUB), 0), min((max(c[0], c[0] + dx) + r - off) // SUB, S - 1)
                i0, i1 = max(_ceil_div(min(c[1], c[1] + dy) - r - off, SUB), 0), min((max(c[1], c[1] + dy) + r - off) // SUB, S - 1)
                if j0 > j1 or i0 > i1:
                    continue
                px = (SUB * np.arange(j0, j1 + 1, dtype=np.int64) + off - c[0])[None, :] + np.zeros((i1 - i0 + 1, 1), np.int64)
                py = (SUB * np.arange(i0, i1 + 1, dtype=np.int64) + off - c[1])[:, None] + np.zeros((1, j1 - j0 + 1), np.int64)
                if wide:
                    px, py = px.astype(object), py.astype(object)
                cov, pp = _covered(px, py, dx, dy, r, 'lt_cap' in corrupt)
                inner = (pp <= r_in * r_in).astype(bool) if part else np.zeros(cov.shape, bool)
                if 'ring_swapped' in corrupt and part:
                    inner = ~inner
                prio = 3 * k + part
                rank = (3 * Nb - 1 - prio) if 'priority_reversed' in corrupt else prio
                sub = K[i0:i1 + 1, j0:j1 + 1]
                np.maximum(sub, np.where(cov, 2 * rank + inner, -1).astype(np.int64), out=sub)
    empty = key < 0
    rank = key >> 1
    prim = np.where(empty, -1, (3 * Nb - 1 - rank) if 'priority_reversed' in corrupt else rank)
    white = empty | ((key & 1) == 1)
    sample = np.where(white[..., None], np.uint8(255), colors[np.where(empty, 0, prim) // 3]).astype(np.uint8)
    return dict(prim_id=prim.astype(np.int32), sample=sample, rgb=downsample(sample, ss, 'ss_no_round' in corrupt))


def downsample(sample, ss, no_round=False):
    if ss == 1:
        return sample.copy()
    s = sample.astype(np.int64)
    return ((s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + (0 if no_round else 2)) >> 2).astype(np.uint8)


class RefOps:
    """the two provider methods on host tensors, from the reference (with an optional seeded corruption)"""

    def __init__(self, corrupt=()):
        self.corrupt = tuple(corrupt)
        self.calls = []

    def skeleton_project(self, x, view, size, ss, jq):
        self.calls.append(('project', x.shape[0]))
        jq.copy_(torch.from_numpy(project(x.numpy(), view, size * ss, self.corrupt)))

    def skeleton_raster(self, jq, bones, colors, radii, size, ss, rgb, prim_id=None):
        self.calls.append(('raster', jq.shape[0]))
        r = raster(jq.numpy(), bones.numpy(), colors.numpy(), radii, size, ss, self.corrupt)
        rgb.copy_(torch.from_numpy(r['rgb']))
        if prim_id is not None:
            prim_id.copy_(torch.from_numpy(r['prim_id']))


# ------------------------------------------------------------------------------------------------ gates
def gate_equal(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return [f'{name}: {got.shape} {got.dtype} against {ref.shape} {ref.dtype}']
    bad = int((got != ref).sum())
    return [f'{name}: {bad} of {ref.size} elements differ'] if bad else []


def gate_all(got, ref, rep=None):
    """got: dict with prim_id and rgb (numpy)"""
    if rep is not None:
        rep.update(covered=float((ref['prim_id'] >= 0).mean()), prims_seen=int(np.unique(ref['prim_id'][ref['prim_id'] >= 0]).size))
    return gate_equal('prim_id', got['prim_id'], ref['prim_id']) + gate_equal('rgb', got['rgb'], ref['rgb'])


# ------------------------------------------------------------------------------------------------ inputs
# a standing H36M pose in the normalised image coordinates of X3D (x right, y down, z away), limbs spread so that the left, the right and the
# middle bones are apart
POSE = np.array([[0, 0, 0], [-0.15, 0, 0.02], [-0.22, 0.3, 0.05], [-0.3, 0.6, 0.02], [0.15, 0, -0.02], [0.22, 0.3, -0.05], [0.3, 0.6, -0.02],
                 [0, -0.18, 0], [0, -0.36, 0], [0, -0.46, 0.01], [0, -0.58, 0], [0.13, -0.36, -0.02], [0.36, -0.3, -0.04], [0.56, -0.22, -0.02],
                 [-0.13, -0.36, 0.02], [-0.36, -0.3, 0.04], [-0.56, -0.22, 0.02]], np.float64)
VIEW_AT = ((-0.45, -0.3, 0.0), (0.45, -0.3, 0.0), (-0.45, 0.3, 0.0), (0.45, 0.3, 0.0), (0.0, 0.0, 0.6), (0.0, 0.0, -0.6),
           (0.3, 0.0, 0.0), (0.3, -0.25, 0.0), (-0.2, -0.25, 0.0))


def view_scene():
    """the orientation scene of tests/golden/skeleton_view.npz: POSE at 0.6 of its size placed at VIEW_AT[t], frame by frame: the four quadrants
    of the box, near and far, then a move along +x, one along -y and one along -x.  float32 [9,17,3]"""
    return np.stack([0.6 * POSE + np.array(at) for at in VIEW_AT]).astype(np.float32)


def walking(frames, seed=0):
    """POSE swaying and drifting over `frames` frames with a little noise: float32 [frames,17,3] inside the box"""
    g = np.random.default_rng(seed)
    out = []
    for t in range(frames):
        a = 0.6 * np.sin(2 * np.pi * t / 40 + seed)
        rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        out.append(0.8 * POSE @ rot.T + np.array([0.3 * np.sin(2 * np.pi * t / 90), 0.1 * np.cos(2 * np.pi * t / 25), 0.2 * np.sin(t / 7)])
                   + 0.01 * g.standard_normal(POSE.shape))
    return np.stack(out).astype(np.float32)


def joint_cloud(n, seed=0):
    """n random joints [n // 17 + 1, 17, 3] f32 in and around the box, with the special values in the first frame: NaN, infinities, a joint
    behind the eye (W <= 0), joints far outside the guard"""
    g = np.random.default_rng(seed)
    x = g.uniform(-1.2, 1.2, (n // 17 + 1, 17, 3)).astype(np.float32)
    x[0, 0] = [np.nan, 0, 0]
    x[0, 1] = [0, np.inf, 0]
    x[0, 2] = [0, 0, -np.inf]
    x[0, 3] = [0, 0, 25.0]               # plotted y = -6400: far away, W > 0
    x[0, 4] = [0, 0, -25.0]              # plotted y = +6400: behind the eye, W < 0
    x[0, 5] = [1e30, 0, 0]               # 5, 6: finite, in front, far outside the image; beyond the guard at 2048 x 2048, ss = 2
    x[0, 6] = [-60.0, 3.0, 0.5]
    x[0, 7] = [0, 0, -17.4375]           # W = 0 at z = -17.4403: just in front of the eye, beyond the guard at every size
    return x


# a view under which a contracted multiply-add shows in the integers (tests/test_skelerr.py): W = 1, the window [0, 1], and two rows whose
# first / third product is not exact.  For the joint FMA_JOINT (p = (-3, 3, 3) exactly):
#   U: fl((1 + 2^-52)(-3)) = -(3 + 2^-50), + 3 = -2^-50, + 3.5 2^-52 = -0.5 2^-52 < 0 -> xq = -1;   fused: -3 2^-52 + 3.5 2^-52 > 0 -> xq = 0
#   V: -3 + fl((1 + 2^-52) 3) = 2^-50, - 3.5 2^-52 = 0.5 2^-52 > 0 -> yq = floor(-v ..) = -1;         fused: 3 2^-52 - 3.5 2^-52 < 0 -> yq = 0
E52 = 2.0 ** -52
FMA_VIEW = (1 + E52, 1.0, 0.0, 3.5 * E52, 1.0, 0.0, 1 + E52, -3.5 * E52, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0)
FMA_JOINT = np.array([[[3 / 256 - 1, -3 / 256 - 1, -3 / 256]]], np.float32)


def c(j):
    """the centre of sample j in 1/16 sample"""
    return SUB * j + SUB // 2


def crafted_cases(size=72, ss=1):
    """name -> (jq [F,J,2] i32, bones [Nb,2] i32, colors [Nb,3] u8, radii): the integer-level cases, for S = size ss samples per side"""
    S = size * ss
    g = np.random.default_rng(S)
    col = lambda n: g.integers(0, 255, (n, 3)).astype(np.uint8)          # noqa: E731  (never 255 255 255: a colour is not the background)
    one = np.array([[0, 1]], np.int32)
    cases = {}
    # a single degenerate bone: the disc, its markers on top
    cases['degenerate'] = (np.array([[[c(20), c(30)], [c(20), c(30)]]], np.int32), one, col(1), (5 * SUB, 3 * SUB, SUB))
    # horizontal, vertical and diagonal bones whose ends and whose radius are whole samples: samples at distance exactly r along the sides and
    # at the caps; the 3-4-5 direction makes (p x d)^2 = r^2 dd hold exactly off the axes too
    j = np.array([[[c(10), c(8)], [c(50), c(8)], [c(8), c(20)], [c(8), c(60)], [c(20), c(20)], [c(50), c(60)], [c(30), c(16)], [c(62), c(40)]]], np.int32)
    cases['exact_r'] = (j, np.array([[0, 1], [2, 3], [4, 5], [7, 6]], np.int32), col(4), (5 * SUB, 0, 0))
    # a bone across the corner of four tiles
    cases['tile_corner'] = (np.array([[[c(TILE) - 8 - 90, c(TILE) - 8 - 70], [c(TILE) - 8 + 80, c(TILE) - 8 + 95]]], np.int32), one, col(1),
                            (2 * SUB + 3, 3 * SUB + 5, SUB + 1))
    # a radius of 40 samples: primitives that span tiles
    cases['radius_40'] = (np.array([[[c(30), c(34)], [c(45), c(40)]]], np.int32), one, col(1), (40 * SUB, 40 * SUB, 12 * SUB))
    # r = 0: only samples exactly on the segment (the diagonal and a horizontal bone through sample centres, a horizontal bone between them)
    cases['r_zero'] = (np.array([[[c(5), c(5)], [c(40), c(40)], [c(3), c(50)], [c(60), c(50)], [c(10), c(60) + 1], [c(30), c(60) + 1]]], np.int32),
                       np.array([[0, 1], [2, 3], [4, 5]], np.int32), col(3), (0, 0, 0))
    # a bone mostly outside the image, and one wholly outside
    cases['outside'] = (np.array([[[-3000, c(10)], [c(6), c(30)], [c(S) + 500, -900], [c(S) + 2000, c(S) + 800]]], np.int32),
                        np.array([[0, 1], [2, 3]], np.int32), col(2), (3 * SUB, 4 * SUB, 2 * SUB))
    # ends at the guard with the largest radius: the diagonal through the image (all covered), a line about 95 samples above it (the upper
    # part covered), and, plotted last, a line so far below that every cross product is beyond 2^31 (a square that wrapped would cover)
    cases['guard'] = (np.array([[[-GUARD, -GUARD], [GUARD, GUARD], [-GUARD, c(-90)], [GUARD, c(-100)], [GUARD, c(450)], [-GUARD, c(430)]]], np.int32),
                      np.array([[0, 1], [2, 3], [4, 5]], np.int32), col(3), (1 << 11, 1 << 11, 1 << 10))
    # a sentinel joint among drawn ones (its bones vanish), joints just inside and just outside the guard, a bad index; frame 1: all dropped
    j = np.array([[c(10), c(10)], [c(40), c(20)], [OUTSIDE, OUTSIDE], [c(60), c(60)], [GUARD + 1, c(30)], [c(30), -GUARD - 1], [GUARD, c(50)]], np.int32)
    dead = j.copy()
    dead[[0, 3, 6]] = [[OUTSIDE, OUTSIDE], [c(3), GUARD + 7], [-OUTSIDE, 5]]
    cases['sentinel'] = (np.stack([j, dead]), np.array([[0, 1], [1, 2], [2, 3], [3, 1], [4, 0], [5, 3], [6, 0], [0, 7], [-1, 1]], np.int32), col(9),
                         (2 * SUB, 3 * SUB, SUB))
    # 64 bones stacked on one spot that straddles a tile corner: the last plotted wins
    cases['stack'] = ((np.array([c(28 * ss), c(28 * ss)]) + g.integers(0, 8 * ss * SUB, (1, 32, 2))).astype(np.int32),
                      g.integers(0, 32, (64, 2)).astype(np.int32), col(64), (SUB, 2 * SUB, SUB))
    # a later bone's line over an earlier bone's marker, and an earlier line under a later marker
    cases['order'] = (np.array([[[c(10), c(35)], [c(36), c(35)], [c(36), c(10)], [c(36), c(64)], [c(20), c(35)]]], np.int32),
                      np.array([[0, 1], [2, 3], [4, 4]], np.int32), col(3), (2 * SUB, 4 * SUB, 2 * SUB))
    return cases
