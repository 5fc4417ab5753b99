"""The host reference of the mesh rasteriser (csrc/render.hip, motionbert_amd/render.py), its gates and its inputs.

Reference.  `project`: numpy float32 in the order include/mbx.h states, every operation rounded on its own.  `raster`: numpy int64 per face over
the samples of its bounding box (coverage, depth, winner), shading in float64.  `RefOps` offers both as a kernel provider, so that the module
runs on the CPU.  `corrupt=` seeds one wrong convention into the reference (CORRUPTIONS): tests/test_rendererr.py shows that each one fails a
gate.

Gates.  Projected integers, face_id and depth: equal bits (`gate_equal`).  rgb (`gate_rgb`): background exactly 255; a covered sample's channel
equals the float64 value rounded half up, except that it may be the neighbouring integer where the float64 value v lies within `bound` of the
half-integer that separates the two.  The bound is derived from the fp32 chain of the kernel, u = 2^-24, for a face with edge vectors a, b,
n = a x b and kappa = |a||b| / |n|:
    a, b: one subtraction per component, relative error u.  A component of n is p - q of two products: fl(p) = p (1 + u)^3, and
    |p| + |q| <= |a||b|, so |dn_k| <= (3u + u) |a||b| and |dn| <= 4 sqrt(3) u |a||b| < 7 u |a||b|.
    cos = |n_z| / |n|:  |dcos| <= |dn_z| / |n| + |d|n|| / |n| <= 11 u kappa, plus 4u for the sum of squares, the root and the divide.
    I = 0.35 + 0.65 cos: 2u.  channel = (alpha c) I + 255 (1 - alpha) + 0.5 with alpha c and 255 (1 - alpha) rounded to fp32: 5u of <= 255.
    => |dv| <= 255 u (11 kappa + 11); the gate takes bound = 255 u (16 kappa + 16).
A face that wins a sample with bound >= 0.5 (a sliver, kappa > 2000) is an unfit test input and raises.  At ss = 2 every sample's allowed
interval goes through the exact average (a + b + c + d + 2) >> 2, which is monotone in each argument: the pixel must lie between the average of
the lower ends and the average of the upper ends."""
import numpy as np
import torch

SUB, ZQ, GUARD, OUTSIDE, TILE = 16, 1 << 20, 1 << 17, 1 << 30, 32
EMPTY = np.int64(0x7fffffffffffffff)
U32 = 2.0 ** -24
COLOR, ALPHA = (166, 188, 218), 0.9
CORRUPTIONS = ('fma', 'half_sample', 'gt_edge', 'tie_high', 'truncated_list', 'depth_ceil', 'y_flip', 'no_z_rule', 'no_guard_rule', 'ss_no_round',
               'snapped_normal', 'back_face_cull')
TRUNCATE_AT = 64            # the list length of the 'truncated_list' corruption


# ------------------------------------------------------------------------------------------------ reference
def project(verts, cube, seq_ptr, S, corrupt=()):
    """verts [F,V,3] f32, cube [n_tracks,4] f32, seq_ptr [n_tracks+1] -> [F,V,3] i32"""
    verts = np.asarray(verts, np.float32)
    cube = np.asarray(cube, np.float32)
    seq_ptr = np.asarray(seq_ptr, np.int64)
    F = verts.shape[0]
    out = np.full(verts.shape, OUTSIDE, np.int32)
    scale = np.array([S * SUB, S * SUB, ZQ], np.float32)
    for s in range(cube.shape[0]):
        a, b = max(int(seq_ptr[s]), 0), min(int(seq_ptr[s + 1]), F)
        if b <= a:
            continue
        x, c, inv = verts[a:b], cube[s, :3], cube[s, 3]
        with np.errstate(all='ignore'):
            if 'y_flip' in corrupt:
                x = x.copy()
                x[..., 1] = np.float32(2) * c[1] - x[..., 1]
            if 'fma' in corrupt:      # (x - c) inv + 0.5 with one rounding, as a contracted multiply-add leaves it
                t = ((x - c).astype(np.float64) * np.float64(inv) + 0.5).astype(np.float32)
            else:
                t = (x - c) * inv + np.float32(0.5)
            p = t * scale
            assert p.dtype == np.float32
            ok = np.abs(p) < np.float32(2.0 ** 30)
            out[a:b] = np.where(ok, np.floor(np.where(ok, p, 0)), OUTSIDE).astype(np.int32)
    return out


def _ceil_div(a, b):
    return -((-a) // b)


def face_shade(v, face):
    """(cos, kappa) of one face in float64 from the fp32 vertices, indices taken in ascending order"""
    a, b, c = sorted(int(i) for i in face)
    e1, e2 = v[b].astype(np.float64) - v[a].astype(np.float64), v[c].astype(np.float64) - v[a].astype(np.float64)
    n = np.cross(e1, e2)
    l2 = float(n @ n)
    if not (l2 > 0 and np.isfinite(l2)):
        return 0.0, np.inf
    ln = np.sqrt(l2)
    return abs(n[2]) / ln, float(np.linalg.norm(e1) * np.linalg.norm(e2) / ln)


def raster(vq, verts, faces, size, ss, color=COLOR, alpha=ALPHA, corrupt=()):
    """-> dict: face_id, depth [F,S,S] i32; val [F,S,S,3] f64 (the channel before rounding; 255 where empty); bound [F,S,S] f64;
    sample [F,S,S,3] u8 (val rounded half up); rgb [F,size,size,3] u8"""
    vq = np.asarray(vq, np.int64)
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    F, V = vq.shape[:2]
    S = size * ss
    Nf = faces.shape[0]
    off = 0 if 'half_sample' in corrupt else SUB // 2
    key = np.full((F, S, S), EMPTY, np.int64)
    cosk = np.zeros((F, Nf, 2))
    nt = (S + TILE - 1) // TILE
    for f in range(F):
        P, K = vq[f], key[f]
        tile_fill = np.zeros((nt, nt), np.int64)
        for n in range(Nf):
            idx = faces[n]
            if idx.min() < 0 or idx.max() >= V:
                continue
            p = P[idx]
            if 'no_guard_rule' not in corrupt and np.abs(p[:, :2]).max() > GUARD:
                continue
            if np.abs(p[:, :2]).max() >= OUTSIDE:
                continue
            if 'no_z_rule' not in corrupt and (p[:, 2].min() < 0 or p[:, 2].max() > ZQ):
                continue
            a2 = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
            if a2 == 0:
                continue
            if a2 < 0:
                if 'back_face_cull' in corrupt:
                    continue
                p, a2 = p[[0, 2, 1]], -a2
            j0, j1 = max(_ceil_div(p[:, 0].min() - off, SUB), 0), min((p[:, 0].max() - off) // SUB, S - 1)
            i0, i1 = max(_ceil_div(p[:, 1].min() - off, SUB), 0), min((p[:, 1].max() - off) // SUB, S - 1)
            if j0 > j1 or i0 > i1:
                continue
            sx = (SUB * np.arange(j0, j1 + 1, dtype=np.int64) + off)[None, :]
            sy = (SUB * np.arange(i0, i1 + 1, dtype=np.int64) + off)[:, None]
            cov = True
            w = []
            for e, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
                dx, dy = p[b, 0] - p[a, 0], p[b, 1] - p[a, 1]
                we = dx * (sy - p[a, 1]) - dy * (sx - p[a, 0])
                owns = (dy > 0 or (dy == 0 and dx > 0)) and not ('gt_edge' in corrupt and e == 0)
                cov = cov & ((we >= 0) if owns else (we > 0))
                w.append(we)
            if 'truncated_list' in corrupt:      # a tile takes the first TRUNCATE_AT faces whose box meets it and ignores the rest
                t0x, t1x, t0y, t1y = j0 // TILE, j1 // TILE, i0 // TILE, i1 // TILE
                full = tile_fill[t0y:t1y + 1, t0x:t1x + 1] >= TRUNCATE_AT
                tile_fill[t0y:t1y + 1, t0x:t1x + 1] += 1
                ti = (np.arange(i0, i1 + 1) // TILE - t0y)[:, None]
                tj = (np.arange(j0, j1 + 1) // TILE - t0x)[None, :]
                cov = cov & ~full[ti, tj]
            if not np.any(cov):
                continue
            num = w[0] * p[0, 2] + w[1] * p[1, 2] + w[2] * p[2, 2]
            d = _ceil_div(num, a2) if 'depth_ceil' in corrupt else num // a2
            k = (d << 32) | ((Nf - 1 - n) if 'tie_high' in corrupt else n)
            sub = K[i0:i1 + 1, j0:j1 + 1]
            np.minimum(sub, np.where(cov, k, EMPTY), out=sub)
        won = np.unique(K[K != EMPTY] & 0xffffffff)
        for n in won:
            n = int(Nf - 1 - n) if 'tie_high' in corrupt else int(n)
            src = vq[f].astype(np.float32) if 'snapped_normal' in corrupt else verts[f]
            cosk[f, n] = face_shade(src, faces[n])
    empty = key == EMPTY
    low = key & 0xffffffff
    face_id = np.where(empty, -1, (Nf - 1 - low) if 'tie_high' in corrupt else low).astype(np.int32)
    depth = (key >> 32).astype(np.int32)
    fi = np.where(empty, 0, face_id)
    fr = np.arange(F)[:, None, None]
    I = 0.35 + 0.65 * cosk[fr, fi, 0]
    val = float(alpha) * np.asarray(color, np.float64) * I[..., None] + 255.0 * (1.0 - float(alpha))
    val = np.where(empty[..., None], 255.0, val)
    bound = np.where(empty, 0.0, 255.0 * U32 * (16.0 * cosk[fr, fi, 1] + 16.0))
    sample = np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)
    return dict(face_id=face_id, depth=depth, val=val, bound=bound, sample=sample, rgb=downsample(sample, ss, 'ss_no_round' in corrupt))


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

    def render_project(self, verts, cube, seq_ptr, size, ss, out):
        self.calls.append(('project', verts.shape[0]))
        out.copy_(torch.from_numpy(project(verts.numpy(), cube.numpy(), seq_ptr.numpy(), size * ss, self.corrupt)))

    def render_raster(self, vq, verts, faces, size, ss, color, alpha, rgb, face_id=None, depth=None):
        self.calls.append(('raster', vq.shape[0]))
        r = raster(vq.numpy(), verts.numpy(), faces.numpy(), size, ss, color, alpha, self.corrupt)
        rgb.copy_(torch.from_numpy(r['rgb']))
        if face_id is not None:
            face_id.copy_(torch.from_numpy(r['face_id']))
        if depth is not None:
            depth.copy_(torch.from_numpy(r['depth']))


# ------------------------------------------------------------------------------------------------ gates
def gate_equal(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return [f'{name}: {got.shape} {got.dtype} against {ref.shape} {ref.dtype}']
    bad = int((got != ref).sum())
    return [f'{name}: {bad} of {ref.size} elements differ'] if bad else []


def sample_interval(ref):
    """the allowed [lo, hi] of every sample channel, uint8 -> int64"""
    val, bound = ref['val'], ref['bound'][..., None]
    covered = (ref['face_id'] >= 0)[..., None]
    if np.any(covered & (bound >= 0.5)):
        raise AssertionError('unfit input: a face with kappa > 2000 wins a sample (its fp32 normal is not determined to half a level)')
    h = np.floor(val) + 0.5
    r = ref['sample'].astype(np.int64)
    up = val >= h                                       # rounded up: the neighbour is one below
    lo = np.where(covered & up & (val - h <= bound), r - 1, r)
    hi = np.where(covered & ~up & (h - val <= bound), r + 1, r)
    return np.clip(lo, 0, 255), np.clip(hi, 0, 255)


def gate_rgb(got, ref, ss, rep=None):
    got = np.asarray(got)
    if got.dtype != np.uint8 or got.shape != ref['rgb'].shape:
        return [f'rgb: {got.shape} {got.dtype} against {ref["rgb"].shape} uint8']
    lo, hi = sample_interval(ref)
    empty = ref['face_id'] < 0
    if ss == 2:
        def avg(s):
            return (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2
        lo, hi = avg(lo), avg(hi)
        empty = empty[:, 0::2, 0::2] & empty[:, 0::2, 1::2] & empty[:, 1::2, 0::2] & empty[:, 1::2, 1::2]
    g = got.astype(np.int64)
    out = []
    bg = int((g[empty] != 255).sum())
    if bg:
        out.append(f'rgb: {bg} background channels are not 255')
    bad = int(((g < lo) | (g > hi)).sum())
    if bad:
        out.append(f'rgb: {bad} of {g.size} channels outside their interval (worst {int(np.maximum(lo - g, g - hi).max())} levels)')
    if rep is not None:
        rep.update(rgb_off_by_one=int((g != ref['rgb']).sum()), rgb_channels=int(g.size), rgb_free=int((lo != hi).sum()),
                   covered=float(1 - (ref['face_id'] < 0).mean()), bound_max=float(ref['bound'].max()))
    return out


def gate_all(got, ref, ss, rep=None):
    """got: dict with face_id, depth, rgb (numpy)"""
    return gate_equal('face_id', got['face_id'], ref['face_id']) + gate_equal('depth', got['depth'], ref['depth']) + gate_rgb(got['rgb'], ref, ss, rep)


# ------------------------------------------------------------------------------------------------ inputs
def icosphere(levels=1):
    """42 vertices / 80 faces at one level (12 / 20 at none), unit radius, float64"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.stack(v), np.asarray(f, np.int32)


def uv_sphere(segments=84, rings=82):
    """a closed surface of 2 + segments rings vertices and 2 segments rings faces: 6,890 / 13,776 at the defaults, the counts of SMPL"""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None]], -1)
    v = np.concatenate([[[0, 1, 0]], ring.reshape(-1, 3), [[0, -1, 0]]])
    idx = 1 + np.arange(rings * segments).reshape(rings, segments)
    nxt = np.roll(idx, -1, axis=1)
    f = [np.stack([np.zeros(segments, np.int64), nxt[0], idx[0]], 1), np.stack([np.full(segments, len(v) - 1), idx[-1], nxt[-1]], 1)]
    for r in range(rings - 1):
        f += [np.stack([idx[r], nxt[r], nxt[r + 1]], 1), np.stack([idx[r], nxt[r + 1], idx[r + 1]], 1)]
    return v, np.concatenate(f).astype(np.int32)


def body_like(frames, seed=0):
    """the uv sphere stretched to a standing body's proportions (0.5 x 1.7 x 0.3 m, in millimetres), bumpy, swaying over `frames` frames:
    float32 [frames,6890,3] and faces [13776,3]"""
    v, f = uv_sphere()
    g = np.random.default_rng(seed)
    bump = 1 + 0.08 * np.sin(7 * v[:, 0] + 1) * np.cos(9 * v[:, 1]) + 0.01 * g.standard_normal(len(v))
    base = v * bump[:, None] * np.array([250.0, 850.0, 150.0])
    out = []
    for t in range(frames):
        a = 0.5 * np.sin(2 * np.pi * t / 60)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        out.append(base @ R.T + np.array([300.0 * np.sin(2 * np.pi * t / 120), 20.0 * np.cos(2 * np.pi * t / 30), 1000.0]))
    return np.stack(out).astype(np.float32), f


def deformed_icosphere(frames=3, seed=0):
    v, f = icosphere(1)
    g = np.random.default_rng(seed)
    out = []
    for t in range(frames):
        A = np.eye(3) + 0.25 * g.standard_normal((3, 3))
        out.append(v @ A.T * 100.0 + 20.0 * g.standard_normal(3) + 5.0 * g.standard_normal(v.shape))
    return np.stack(out).astype(np.float32), f


def verts_from_vq(vq, S):
    """fp32 vertices whose normals are well conditioned for crafted integer vertices: x, y as they are, z brought to the same scale"""
    v = np.asarray(vq, np.float64).copy()
    v[..., 2] *= S * SUB / ZQ
    return np.where(np.abs(v) < 2.0 ** 24, v, 0).astype(np.float32)


def crafted_cases(size=72, ss=1, seed=0):
    """name -> (vq [F,V,3] i32, faces [Nf,3] i32): the integer-level cases of the issue, for S = size ss samples per side"""
    S = size * ss
    g = np.random.default_rng(seed)
    c = lambda j: SUB * j + SUB // 2                                    # noqa: E731  (the sample centre)
    z = lambda: int(g.integers(0, ZQ + 1))                              # noqa: E731
    cases = {}
    # quads cut in two: corners on sample centres, so that both diagonals run through sample centres; both diagonals, mixed windings
    q = np.array([[c(3), c(2), 1000], [c(23), c(2), 90000], [c(23), c(22), 500000], [c(3), c(22), ZQ],
                  [c(30), c(30), 7], [c(50), c(30), 7], [c(50), c(60), 7], [c(30), c(60), 7],
                  [c(40) + 3, c(5) + 5, 70], [c(66) + 1, c(9) - 2, 700], [c(60), c(27) + 7, 7000], [c(38) - 5, c(25), 70000]], np.int32)
    cases['quads'] = (q[None], np.array([[0, 1, 2], [0, 2, 3], [4, 5, 7], [7, 5, 6], [8, 9, 10], [10, 11, 8]], np.int32))
    # one face over the whole image
    cases['whole'] = (np.array([[[-2000, -2000, 0], [2 * S * SUB + 4000, -2000, ZQ], [-2000, 2 * S * SUB + 4000, ZQ // 2]]], np.int32),
                      np.array([[0, 1, 2]], np.int32))
    # 2,000 small faces on one 8 x 8-pixel spot (more than any list in LDS), random depths, Nf no multiple of 256
    n = 2000
    base = np.array([c(28 * ss), c(28 * ss)])                           # the spot straddles a tile corner (sample 32 ss)
    v = np.concatenate([base + g.integers(0, 8 * ss * SUB, (3 * n, 2)), g.integers(0, ZQ + 1, (3 * n, 1))], 1).astype(np.int32)
    cases['stack'] = (v[None], np.arange(3 * n, dtype=np.int32).reshape(n, 3))
    # faces that straddle the corners of the tiles, and interpenetrating faces
    v, f = [], []
    for cx in (TILE, 2 * TILE):
        for cy in (TILE, 2 * TILE):
            k = len(v)
            v += [[c(cx) - 8 - 40, c(cy) - 8 - 25, z()], [c(cx) - 8 + 37, c(cy) - 8 - 9, z()], [c(cx) - 8 - 3, c(cy) - 8 + 44, z()]]
            f.append([k, k + 1, k + 2])
    k = len(v)
    v += [[c(4), c(4), 0], [c(68), c(10), ZQ], [c(8), c(66), ZQ], [c(66), c(66), 0], [c(2), c(12), ZQ], [c(60), c(3), ZQ // 3]]
    f += [[k, k + 1, k + 2], [k + 3, k + 4, k + 5]]
    cases['corners'] = (np.array(v, np.int32)[None], np.array(f, np.int32))
    # dropped faces among drawn ones: zero area, outside the guard, a bad index, z out of range; frame 1: every face dropped
    v = np.array([[c(5), c(5), 100], [c(40), c(8), 200], [c(10), c(50), 300],                 # 0-2 a drawn face
                  [c(20), c(20), 5], [c(30), c(30), 5], [c(40), c(40), 5],                    # 3-5 collinear
                  [GUARD + 1, c(3), 5], [-GUARD - 1, c(60), 5], [c(7), GUARD + 1, 5],         # 6-8 outside the guard
                  [c(60), c(60), -1], [c(70), c(50), ZQ + 1], [c(50), c(70), 50],             # 9-11 z out of range
                  [OUTSIDE, OUTSIDE, OUTSIDE], [c(64), c(2), ZQ], [c(71), c(2), ZQ], [c(71), c(30), 0]], np.int32)
    f = np.array([[0, 1, 2], [3, 4, 5], [3, 3, 4], [0, 1, 6], [7, 1, 2], [0, 8, 2], [9, 13, 14], [10, 13, 14], [0, 1, 16], [-1, 1, 2],
                  [12, 1, 2], [13, 14, 15], [2, 1, 0]], np.int32)
    dead = v.copy()
    dead[[0, 1, 13]] = [[GUARD + 5, 0, 0], [0, 0, ZQ + 7], [OUTSIDE, OUTSIDE, OUTSIDE]]
    cases['dropped'] = (np.stack([v, dead]), f)
    return cases


def property_quads():
    """quads cut in two for the exactly-once property: (vq [1,V,3], faces, the quad's sample rectangle or None)"""
    c = lambda j: SUB * j + SUB // 2                                    # noqa: E731
    out = []
    for (x0, y0, x1, y1) in ((2, 3, 18, 19), (1, 1, 30, 12), (5, 2, 9, 27)):                 # square: the diagonal passes through sample centres
        v = np.array([[c(x0), c(y0), 10], [c(x1), c(y0), 10], [c(x1), c(y1), 10], [c(x0), c(y1), 10]], np.int32)
        for f in ([[0, 1, 2], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[3, 0, 1], [3, 2, 1]]):
            out.append((v[None], np.array(f, np.int32), (x0, y0, x1, y1)))
    g = np.random.default_rng(5)
    while len(out) < 18:                                                # general position: vertices 1 and 3 on opposite sides of the edge 0 - 2
        v = np.concatenate([g.integers(SUB, 30 * SUB, (4, 2)), np.full((4, 1), 10)], 1).astype(np.int64)
        side = lambda k: (v[2, 0] - v[0, 0]) * (v[k, 1] - v[0, 1]) - (v[2, 1] - v[0, 1]) * (v[k, 0] - v[0, 0])      # noqa: E731
        if side(1) * side(3) < 0:
            out.append((v.astype(np.int32)[None], np.array([[0, 1, 2], [0, 2, 3]], np.int32), None))
    # a fan around a vertex on a sample centre
    hub = np.array([[c(16), c(16), 10]] + [[c(16) + int(200 * np.cos(a)), c(16) + int(200 * np.sin(a)), 10] for a in np.linspace(0, 2 * np.pi, 8)[:-1]], np.int32)
    out.append((hub[None], np.array([[0, 1 + k, 1 + (k + 1) % 7] for k in range(7)], np.int32), None))
    return out


VIEW_XY = ((-1, -1), (1, -1), (-1, 1), (1, 1), (0.1, 0.5), (0.6, 0.5), (0.6, -0.2))


def view_scene():
    """the orientation scene of tests/golden/render_view.npz: an icosahedron of radius 60 at 400 VIEW_XY[t] (x, y in mesh units), frame by
    frame: the four quadrants of the cube, then a move along +x and one along -y.  float32 [7,12,3], faces [20,3]"""
    v, f = icosphere(0)
    out = [60.0 * v + np.array([400.0 * x, 400.0 * y, 1000.0 + 50.0 * t]) for t, (x, y) in enumerate(VIEW_XY)]
    return np.stack(out).astype(np.float32), f
