"""The host reference of the crowd rasteriser (csrc/scene.hip, motionbert_amd/render.py `render_scene`), its gates, its two reductions to code
that exists, and its inputs.

Reference.  `project`: numpy float64, floor(double(x) (16 ss) + 0.5).  `raster`: a rectangular restatement of tests/skelerr.raster: per person
and primitive over the samples of its bounding box with the coverage predicate of tests/skelerr.py (`_covered`), persons painted in the order
of the frame's list, so that the later one replaces the earlier wherever it covers.  `RefOps` offers both as a kernel provider, so that the
module runs on the CPU.  `corrupt=` seeds one wrong convention into the reference (CORRUPTIONS): tests/test_sceneerr.py shows that each one
fails a gate.

Gates.  jq, prim_id and rgb: equal bits (`skelerr.gate_equal`).  Everything after the projection is integer, and the projection is float64 in
a stated order: there is no tolerance anywhere.

Reductions.  (a) `reduction_a`: a square scene with one person per frame, the identity table and a white background is `skelerr.raster` (or
mbx_skeleton_raster) on the same jq, in every bit.  (b) `reduction_b`: a scene of P persons is the P single-person pictures painted over the
background in list order; where a single picture has prim_id >= 0 it replaces what was there.  The single pictures are taken at ss = 1 on the
sample grid (W ss x H ss pixels, the same jq and radii), so that for ss = 2 the mean is taken after the painting, as the kernel takes it."""
import numpy as np
import torch

from motionbert_amd import render
from tests import skelerr as SE

SUB, GUARD, OUTSIDE, TILE = SE.SUB, SE.GUARD, SE.OUTSIDE, SE.TILE
CHUNK = render.SCENE_CHUNK                 # MBX_SCENE_CHUNK
CORRUPTIONS = ('rank_ignored', 'first_wins', 'bg_frame_off_by_one', 'chunk_second_dropped', 'cull_touch', 'wh_swapped', 'palette_wrong_person',
               'ss_mean_white', 'skipped_drawn', 'frame_ptr_late', 'no_half', 'truncated')
c = SE.c


# ------------------------------------------------------------------------------------------------ reference: projection
def project(x, ss, corrupt=()):
    """x [R,J,2|3] f32 in video pixels -> jq [R,J,2] i32"""
    x = np.asarray(x, np.float32)[..., :2]
    scale = 16 * ss
    with np.errstate(all='ignore'):
        q = x.astype(np.float64) * np.float64(scale) + (0.0 if 'no_half' in corrupt else 0.5)
        q = np.trunc(q) if 'truncated' in corrupt else np.floor(q)
        ok = (np.isfinite(x) & (np.abs(q) <= GUARD)).all(-1)
    return np.where(ok[..., None], np.where(ok[..., None], q, 0), OUTSIDE).astype(np.int32)


# ------------------------------------------------------------------------------------------------ reference: raster
def person_keys(j, bones, radii, SW, SH):
    """one skeleton j [J,2] (Python-int safe) over SW x SH samples -> key [SH,SW] int64 = 2 primitive + (inside the marker's white centre), -1
    where nothing covers; the winner inside a skeleton is the covering primitive of highest priority, as in skelerr.raster"""
    r_line, r_out, r_in = (int(r) for r in radii)
    J, off = j.shape[0], SUB // 2
    K = np.full((SH, SW), -1, np.int64)
    for k in range(bones.shape[0]):
        ia, ib = int(bones[k, 0]), int(bones[k, 1])
        if not (0 <= ia < J and 0 <= ib < J):
            continue
        a, b = [int(v) for v in j[ia]], [int(v) for v in j[ib]]
        if max(abs(v) for v in a + b) > GUARD:
            continue
        for part in range(3):
            p = b if part == 2 else a
            dx, dy = (b[0] - a[0], b[1] - a[1]) if part == 0 else (0, 0)
            r = r_line if part == 0 else r_out
            j0, j1 = max(SE._ceil_div(min(p[0], p[0] + dx) - r - off, SUB), 0), min((max(p[0], p[0] + dx) + r - off) // SUB, SW - 1)
            i0, i1 = max(SE._ceil_div(min(p[1], p[1] + dy) - r - off, SUB), 0), min((max(p[1], p[1] + dy) + r - off) // SUB, SH - 1)
            if j0 > j1 or i0 > i1:
                continue
            px = (SUB * np.arange(j0, j1 + 1, dtype=np.int64) + off - p[0])[None, :] + np.zeros((i1 - i0 + 1, 1), np.int64)
            py = (SUB * np.arange(i0, i1 + 1, dtype=np.int64) + off - p[1])[:, None] + np.zeros((1, j1 - j0 + 1), np.int64)
            cov, pp = SE._covered(px, py, dx, dy, r)
            inner = (pp <= r_in * r_in).astype(bool) if part else np.zeros(cov.shape, bool)
            sub = K[i0:i1 + 1, j0:j1 + 1]
            np.maximum(sub, np.where(cov, 2 * (3 * k + part) + inner, -1).astype(np.int64), out=sub)
    return K


def _strict_cull(K, j, radii, SW, SH):
    """the corruption 'cull_touch': per tile, a person whose box (its drawn joints grown by the largest radius) only touches the tile is dropped"""
    ok = (np.abs(j) <= GUARD).all(-1)
    if not ok.any():
        return K
    rmax, span = max(int(radii[0]), int(radii[1])), SUB * (TILE - 1)
    x0, x1, y0, y1 = (int(v) for v in (j[ok, 0].min() - rmax, j[ok, 0].max() + rmax, j[ok, 1].min() - rmax, j[ok, 1].max() + rmax))
    for ty in range(0, SH, TILE):
        for tx in range(0, SW, TILE):
            if not (x0 < c(tx) + span and x1 > c(tx) and y0 < c(ty) + span and y1 > c(ty)):
                K[ty:ty + TILE, tx:tx + TILE] = -1
    return K


def _bg_samples(background, f, W, H, ss, corrupt=()):
    """the colour an uncovered sample takes: [H ss, W ss, 3] u8"""
    if isinstance(background, np.ndarray) and background.ndim == 4:
        n = background.shape[0]
        frame = background[0 if n == 1 else ((f + 1) % n if 'bg_frame_off_by_one' in corrupt else f)]
        return np.repeat(np.repeat(frame, ss, axis=0), ss, axis=1)
    return np.broadcast_to(np.asarray(background, np.uint8), (H * ss, W * ss, 3)).copy()


def raster(jq, table, bones, palette, radii, W, H, ss, background=(255, 255, 255), corrupt=()):
    """jq [R,J,2] i32, table = (frame_ptr [Fv+1], rows [n], person [n]), palette [P,Nb,3] u8, background: three ints or u8 [Fv or 1,H,W,3]
    -> dict: prim_id [Fv, H ss, W ss] i32 (-1 where empty); rgb [Fv,H,W,3] u8"""
    jq = np.asarray(jq, np.int64)
    frame_ptr, rows, person = (np.asarray(t, np.int64) for t in table)
    bones, palette = np.asarray(bones, np.int64), np.asarray(palette, np.uint8)
    R_, P, n = jq.shape[0], palette.shape[0], rows.shape[0]
    Fv, np_, SW, SH = frame_ptr.shape[0] - 1, 3 * bones.shape[0], W * ss, H * ss
    kW, kH = (SH, SW) if 'wh_swapped' in corrupt else (SW, SH)
    prim_id = np.full((Fv, SH, SW), -1, np.int32)
    rgb = np.zeros((Fv, H, W, 3), np.uint8)
    for f in range(Fv):
        g = f + 1 if 'frame_ptr_late' in corrupt else f                      # past the end: an empty list
        lo = min(max(int(frame_ptr[g]), 0), n) if g < Fv else 0
        hi = min(max(int(frame_ptr[g + 1]), lo), n) if g < Fv else 0
        bg = _bg_samples(background, f, W, H, ss, corrupt)
        sample, pid = bg.copy(), prim_id[f]
        best = np.full((SH, SW), -1, np.int64)                               # 'rank_ignored': the winning primitive, whoever it belongs to
        for rank, k in enumerate(range(lo, hi)):
            row, per = int(rows[k]), int(person[k])
            if 'chunk_second_dropped' in corrupt and rank % CHUNK == 1:
                continue
            if not (0 <= row < R_ and (P == 1 or 0 <= per < P)):
                if 'skipped_drawn' not in corrupt or R_ == 0:
                    continue
                row, per = row % R_, per % P
            K = np.full((SH, SW), -1, np.int64)
            part = person_keys(jq[row], bones, radii, kW, kH)
            K[:min(SH, kH), :min(SW, kW)] = part[:min(SH, kH), :min(SW, kW)]
            if 'cull_touch' in corrupt:
                K = _strict_cull(K, jq[row], radii, SW, SH)
            m = K >= 0
            if 'first_wins' in corrupt:
                m &= pid < 0
            if 'rank_ignored' in corrupt:
                m &= (K >> 1) > best
            best[m] = (K >> 1)[m]
            colours = palette[0 if P == 1 else ((per + 1) % P if 'palette_wrong_person' in corrupt else per)]
            col = np.where(((K & 1) == 1)[..., None], np.uint8(255), colours[np.where(m, K >> 1, 0) // 3]).astype(np.uint8)
            sample[m] = col[m]
            pid[m] = (rank * np_ + (K >> 1))[m]
        if 'ss_mean_white' in corrupt and ss == 2:
            sample[pid < 0] = 255
        rgb[f] = SE.downsample(sample[None], ss)[0]
    return dict(prim_id=prim_id, rgb=rgb)


class RefOps:
    """the two provider methods on host tensors, from the reference (with an optional seeded corruption)"""

    def __init__(self, corrupt=()):
        self.corrupt = tuple(corrupt)
        self.calls = []

    def scene_project(self, x, ss, jq):
        self.calls.append(('scene_project', x.shape[0]))
        jq.copy_(torch.from_numpy(project(x.numpy(), ss, self.corrupt)))

    def scene_raster(self, jq, frame_ptr, rows, person, bones, palette, radii, width, height, ss, background, rgb, prim_id=None):
        self.calls.append(('scene_raster', frame_ptr.numel() - 1))
        bg = background.numpy() if isinstance(background, torch.Tensor) else background
        r = raster(jq.numpy(), (frame_ptr.numpy(), rows.numpy(), person.numpy()), bones.numpy(), palette.numpy(), radii, width, height, ss, bg, self.corrupt)
        rgb.copy_(torch.from_numpy(r['rgb']))
        if prim_id is not None:
            prim_id.copy_(torch.from_numpy(r['prim_id']))


# ------------------------------------------------------------------------------------------------ gates
gate_equal = SE.gate_equal


def gate_all(got, ref, rep=None):
    """got: dict with prim_id and rgb (numpy)"""
    if rep is not None:
        rep.update(covered=float((ref['prim_id'] >= 0).mean()) if ref['prim_id'].size else 0.0,
                   prims_seen=int(np.unique(ref['prim_id'][ref['prim_id'] >= 0]).size))
    return gate_equal('prim_id', got['prim_id'], ref['prim_id']) + gate_equal('rgb', got['rgb'], ref['rgb'])


# ------------------------------------------------------------------------------------------------ the two reductions
def identity_table(F):
    """one person per frame: row f in frame f"""
    return np.arange(F + 1, dtype=np.int32), np.arange(F, dtype=np.int32), np.zeros(F, np.int32)


def reduction_a(scene_fn, jq, bones, colors, radii, size, ss, skeleton_fn=SE.raster):
    """(a): `scene_fn(jq, table, bones, palette, radii, W, H, ss, background)` on a square image, the identity table and white equals
    `skeleton_fn(jq, bones, colors, radii, size, ss)` in every bit -> gate messages"""
    got = scene_fn(jq, identity_table(jq.shape[0]), bones, np.asarray(colors, np.uint8)[None], radii, size, size, ss, (255, 255, 255))
    ref = skeleton_fn(jq, bones, colors, radii, size, ss)
    return gate_equal('(a) prim_id', got['prim_id'], ref['prim_id']) + gate_equal('(a) rgb', got['rgb'], ref['rgb'])


def reduction_b(whole, jq, table, bones, palette, radii, W, H, ss, background, single_fn=raster):
    """(b): `whole` (dict prim_id, rgb: the scene as the code under test drew it) equals the single-person pictures of `single_fn` painted over
    the background in list order -> gate messages.  The singles of one video frame are one call: a scene of as many frames with one entry each,
    at ss = 1 on the sample grid, over that frame's background repeated ss times."""
    frame_ptr, rows, person = (np.asarray(t) for t in table)
    Fv, np_, n, SW, SH = frame_ptr.shape[0] - 1, 3 * np.asarray(bones).shape[0], rows.shape[0], W * ss, H * ss
    pid, rgb = np.full((Fv, SH, SW), -1, np.int32), np.zeros((Fv, H, W, 3), np.uint8)
    for f in range(Fv):
        lo = min(max(int(frame_ptr[f]), 0), n)
        hi = min(max(int(frame_ptr[f + 1]), lo), n)
        canvas = _bg_samples(background, f, W, H, ss)
        if hi > lo:
            one = single_fn(jq, (np.arange(hi - lo + 1, dtype=np.int32), rows[lo:hi].astype(np.int32), person[lo:hi].astype(np.int32)), bones, palette,
                            radii, SW, SH, 1, canvas[None].copy())
            for rank in range(hi - lo):
                m = one['prim_id'][rank] >= 0
                canvas[m] = one['rgb'][rank][m]
                pid[f][m] = rank * np_ + one['prim_id'][rank][m]
        rgb[f] = SE.downsample(canvas[None], ss)[0]
    return gate_equal('(b) prim_id', whole['prim_id'], pid) + gate_equal('(b) rgb', whole['rgb'], rgb)


# ------------------------------------------------------------------------------------------------ inputs
BONES5 = np.array([[0, 7], [7, 8], [8, 11], [8, 14], [0, 1]], np.int32)      # a few bones of the H36M list: crowds stay cheap for the host reference


def backdrop(n, W, H, seed=0):
    """n background frames [n,H,W,3] u8: a ramp per channel plus noise, different in every frame, never white"""
    g = np.random.default_rng(seed)
    i, j = np.mgrid[0:H, 0:W]
    return np.stack([np.stack([(3 * i + 5 * j + 40 * t) % 200, (7 * i + 2 * j + 90 * t) % 230, (i * j + 17 * t) % 250], -1) + g.integers(0, 5, (H, W, 3))
                     for t in range(n)]).astype(np.uint8)


def crowd_pixels(counts, W, H, seed=0):
    """a crowd in video pixels: frame f holds counts[f] persons, each its own track of one row: (x [R,17,2] f32, list of frame-id arrays).
    The persons stand in and around the image (some wholly outside, the first and the last of a frame inside), 12 to 30 pixels tall."""
    g = np.random.default_rng(seed)
    R = int(sum(counts))
    at = np.stack([g.uniform(-0.3 * W, 1.3 * W, R), g.uniform(-0.3 * H, 1.3 * H, R)], -1)
    ends = np.cumsum([0] + list(counts))
    sight = np.unique(np.concatenate([ends[:-1][np.asarray(counts) > 0], ends[1:][np.asarray(counts) > 0] - 1]))
    at[sight] = np.stack([g.uniform(0.3 * W, 0.7 * W, sight.size), g.uniform(0.4 * H, 0.6 * H, sight.size)], -1)      # in sight
    tall = g.uniform(12, 30, R)
    x = at[:, None, :] + tall[:, None, None] * SE.POSE[None, :, :2] + g.normal(0, 0.3, (R, 17, 2))
    return x.astype(np.float32), [np.array([f], np.int64) for f, n in enumerate(counts) for _ in range(n)]


def crafted_case(W, H, ss, counts=(0, 1, CHUNK, CHUNK + 1), seed=0):
    """the integer-level scene of the tests: the list of frame f holds exactly counts[f] entries (BONES5, a palette row each): random persons
    and, in every list of more than ten, these ten entries among them
        * a person wholly outside the image and one across the corner of four tiles,
        * a person with sentinel joints,
        * two persons on identical coordinates with different colours: the later rank must win everywhere,
        * a person whose marker ends exactly on the last sample centre of a tile: its box only touches that tile,
        * table entries that name no row, and entries of a drawn row that name no palette row: skipped, their ranks still counted.
    -> dict(jq, table, bones, palette, radii, R, P).  The special entries stand behind the random persons, the twins last; in the last frame
    they stand first, so that a crowd paints over them and the list ends with a person in sight."""
    SW, SH = W * ss, H * ss
    g = np.random.default_rng(seed + 1000 * ss + W)
    crowd = [n - 10 if n > 10 else n for n in counts]
    x, _ = crowd_pixels(crowd, W, H, seed + W)
    jq = [project(x, ss)]
    radii = (SUB * ss, 2 * SUB * ss, SUB * ss // 2)
    pose = lambda cx, cy, tall: np.round(np.array([cx, cy]) + tall * SUB * SE.POSE[:, :2]).astype(np.int32)      # noqa: E731  (in 1/16 sample)
    special = [pose(c(SW) + 60 * SUB, c(SH // 2), 14 * ss),                    # 0: wholly outside
               pose(c(TILE) - 8, c(TILE) - 8, 20 * ss),                        # 1: across the corner of four tiles
               pose(c(SW // 2), c(SH // 2), 16 * ss),                          # 2: with sentinel joints
               pose(c(SW // 3), c(SH // 2), 18 * ss), pose(c(SW // 3), c(SH // 2), 18 * ss),      # 3, 4: twins
               np.tile(np.array([[c(TILE - 1) + radii[1], c(10)]], np.int32), (17, 1))]            # 5: a marker that touches tile column 0
    special[2][[8, 1]] = [[OUTSIDE, OUTSIDE], [GUARD + 1, 5]]
    jq.append(np.stack(special))
    jq = np.concatenate(jq).astype(np.int32)
    R, n0 = jq.shape[0], int(sum(crowd))
    P = n0 + 6
    palette = render.track_palette(P, BONES5)
    entries, ptr, at = [], [0], 0                                            # (row, person)
    for f, n in enumerate(crowd):
        mine = [(r, r) for r in range(at, at + n)]
        at += n
        if counts[f] > 10:
            extra = [(n0 + 0, n0 + 0), (n0 + 1, n0 + 1), (R + 3, 0), (n0 + 2, n0 + 2), (n0 + 5, n0 + 5), (-1, 0), (n0 + 1, P), (n0 + 1, -2)]
            twins = [(n0 + 3, n0 + 3), (n0 + 4, n0 + 4)]
            mine = twins + extra + mine if f == len(counts) - 1 else mine + extra + twins
        entries += mine
        ptr.append(len(entries))
    rows, person = [e[0] for e in entries], [e[1] for e in entries]
    return dict(jq=jq, table=(np.array(ptr, np.int32), np.array(rows, np.int32), np.array(person, np.int32)), bones=BONES5, palette=palette,
                radii=radii, R=R, P=P)
