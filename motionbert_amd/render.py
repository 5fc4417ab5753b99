"""Video frames on the device: the last lines of infer_wild_mesh.py and infer_wild.py, `render_and_save` -> `vismo.motion2video_mesh`
(csrc/render.hip) and `vismo.motion2video_3d` (csrc/skeleton.hip), as compute.  An Instinct has no graphics pipeline; the frames are drawn
by exact fixed-point tile rasterisers instead (include/mbx.h has the definitions.  The mesh: orthographic along +z, image x right with mesh
x, image y down with mesh y, inside the bounding cube of the whole motion, z-buffered and flat-shaded, white background.  The skeleton: the
reference's perspective 3D axes as one constant matrix, bones and joints in the reference's plot order, white background).

    frame_cube(verts, seq_lens=None)        [n_tracks,4] = (cx, cy, cz, 1 / (2 R)) per track over ALL its frames, torch operations on the device
    render_mesh(verts, faces, ...)          verts [F,V,3] + faces [Nf,3] -> {'rgb': uint8 [F,size,size,3]} (+ the test hooks 'face_id', 'depth',
                                            'vq') as device tensors
    render_chunks(verts, faces, ...)        generator of host uint8 [n,size,size,3] arrays, `chunk` frames at a time through two pinned
                                            buffers: 4,960 frames at 1024 x 1024 are 15.6 GB and cannot be one tensor
    render_skeleton(x3d, ...)               x3d [F,J,3] (the X3D of `wild.infer`, device tensor or host array) -> {'rgb': uint8 [F,size,size,3]}
                                            (+ the test hooks 'prim_id', 'jq'): the reference's 3D axes view as the constant SKELETON_VIEW, bones as
                                            capsules and joints as ringed discs in the reference's plot order, exact in integers
    skeleton_chunks(x3d, ...)               the same frames through the pipeline of render_chunks
    skeleton_radii(size, ss)                the reference's line and marker widths scaled to the image
    scene_table(frame_ids, ...)             the frames of every track (`wild.read_alphapose(frames=True)`) -> (frame_ptr, rows, person): who is
                                            in which video frame, in drawing order (host, numpy)
    render_scene(x3d, table, W, H, ...)     every tracked person of a video frame in one image of W x H pixels (csrc/scene.hip): x3d in video
                                            pixels (`wild.infer(..., pixel=True)`: the dict of tracks, or a device tensor [R,J,2|3]) -> {'rgb': uint8
                                            [Fv,H,W,3]} (+ 'prim_id', 'jq'), over a colour or over the video's own frames
    scene_chunks(x3d, table, W, H, ...)     the same frames through the pipeline of render_chunks
    track_palette(n)                        n distinct colour rows [n,16,3] for the persons of a scene, from an integer formula

The file itself -- the frames compressed on the device and written as Motion-JPEG -- is motionbert_amd.video (`mesh_video`, `skeleton_video`, `scene_video`).

Not here: the 2D overlay of `motion2video`, matplotlib's panes, grid and anti-aliasing, smooth shading, other mesh cameras, several meshes
in one frame, track labels or text, ordering persons by estimated depth (the caller passes `order` to `scene_table`).  The input video behind
a scene is read by motionbert_amd.video (`MJPEGReader`, Motion-JPEG in AVI; csrc/jpeg_dec.hip) and passed as `background=`.

There is no CPU path: without an injected kernel provider (`ops=`), tensors that are not on a ROCm device raise."""
from __future__ import annotations

import numpy as np
import torch

from . import hip_ops

MAX_SIZE, SUB, ZQ = 2048, 16, 1 << 20
WANT_KEYS = ('rgb', 'face_id', 'depth', 'vq')
SKELETON_WANT_KEYS = ('rgb', 'prim_id', 'jq')
MAX_JOINTS, MAX_BONES, MAX_RADIUS = 32, 64, 1 << 11
CUBE_SLACK = 1.0 + 2.0 ** -16
MESH_COLOR, MESH_ALPHA = (166, 188, 218), 0.9      # vismo.py:323: the face colour of the reference's surface, alpha 0.9 over white


def _lens(seq_lens, F, where):
    lens = [F] if seq_lens is None else [int(n) for n in seq_lens]
    if not lens or any(n < 0 for n in lens) or sum(lens) != F:
        raise ValueError(f'{where}: seq_lens {lens} do not sum to the {F} frames of verts')
    return lens


def _check_verts(verts, where):
    if not isinstance(verts, torch.Tensor) or verts.dtype != torch.float32 or verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] < 1:
        raise ValueError(f'{where}: verts must be a float32 tensor [F, V >= 1, 3], got '
                         f'{tuple(verts.shape) if hasattr(verts, "shape") else type(verts).__name__} {getattr(verts, "dtype", "")}')


def frame_cube(verts: torch.Tensor, seq_lens=None) -> torch.Tensor:
    """The framing of motion2video_mesh (vismo.py:301-306) per track: c = (max + min) / 2 per axis and R = the largest extent / 2, both over
    all frames of the track -> [n_tracks,4] float32 = (cx, cy, cz, 1 / (2 R)) on the device of `verts`.  No host read.  R is widened by
    2^-16 of itself (half a sub-sample step at the largest image): in fp32 the outermost vertex of the largest axis would otherwise land at
    -2^-24 now and then, which for z is outside the depth range, where the dropped-face rule takes its faces.  A track without frames, or
    without extent, holds values that are not finite: its frames come out white."""
    _check_verts(verts, 'render.frame_cube')
    lens = _lens(seq_lens, verts.shape[0], 'render.frame_cube')
    rows, end = [], 0
    for n in lens:
        v = verts[end:end + n].reshape(-1, 3)
        end += n
        if n == 0:
            rows.append(torch.full((4,), float('nan'), dtype=torch.float32, device=verts.device))
            continue
        hi, lo = v.max(dim=0).values, v.min(dim=0).values
        rows.append(torch.cat([(hi + lo) / 2, 1.0 / ((hi - lo).max() * CUBE_SLACK).reshape(1)]))
    return torch.stack(rows).contiguous()


def _check(verts, faces, cube, seq_lens, size, ss, color, alpha, want, ops, where):
    _check_verts(verts, where)
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f'{where}: faces must be an int32 tensor [Nf,3], got '
                         f'{tuple(faces.shape) if hasattr(faces, "shape") else type(faces).__name__} {getattr(faces, "dtype", "")}')
    if faces.shape[0] < 1:
        raise ValueError(f'{where}: faces is empty')
    if not isinstance(size, int) or not 1 <= size <= MAX_SIZE:
        raise ValueError(f'{where}: size must be an int in [1, {MAX_SIZE}], got {size!r}')
    if ss not in (1, 2):
        raise ValueError(f'{where}: ss must be 1 or 2, got {ss!r}')
    if len(color) != 3 or not all(0 <= float(c) <= 255 for c in color) or not 0 <= float(alpha) <= 1:
        raise ValueError(f'{where}: color must be three values in [0, 255] and alpha in [0, 1], got {color!r} / {alpha!r}')
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in WANT_KEYS for k in want):
        raise ValueError(f'{where}: want must name some of {WANT_KEYS}, got {want!r}')
    lens = _lens(seq_lens, verts.shape[0], where)
    if faces.device != verts.device:
        raise ValueError(f'{where}: faces on {faces.device}, verts on {verts.device}')
    if cube is not None and (not isinstance(cube, torch.Tensor) or cube.dtype != torch.float32 or tuple(cube.shape) != (len(lens), 4)
                             or cube.device != verts.device):
        raise ValueError(f'{where}: cube must be a float32 tensor [{len(lens)},4] on {verts.device}, got '
                         f'{tuple(cube.shape) if hasattr(cube, "shape") else type(cube).__name__}')
    prov = hip_ops.provider(ops, 'motionbert_amd.' + where, verts, faces, cube)
    return want, lens, prov


def _seq_ptr(lens, dev):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(dev)


def _render(prov, verts, faces, cube, seq_ptr, size, ss, color, alpha, rgb, want):
    F, V, S, dev = verts.shape[0], verts.shape[1], size * ss, verts.device
    vq = torch.empty(F, V, 3, dtype=torch.int32, device=dev)
    res = {'rgb': rgb, 'vq': vq}
    for k in ('face_id', 'depth'):
        res[k] = torch.empty(F, S, S, dtype=torch.int32, device=dev) if k in want else None
    if F:
        prov.render_project(verts, cube, seq_ptr, size, ss, vq)
        prov.render_raster(vq, verts, faces, size, ss, color, alpha, rgb, res['face_id'], res['depth'])
    return res


def render_mesh(verts, faces, cube=None, seq_lens=None, size: int = 1024, ss: int = 1, color=MESH_COLOR, alpha: float = MESH_ALPHA, out=None,
                want=('rgb',), ops=None):
    """verts [F,V,3] float32 and faces [Nf,3] int32 on the device -> a dict of device tensors: 'rgb' uint8 [F,size,size,3] and, where `want`
    names them, the test hooks 'face_id' / 'depth' int32 [F,S,S] (S = size ss; -1 / 0x7fffffff where empty) and 'vq' int32 [F,V,3] (the
    projected vertices).  `cube` [n_tracks,4] as `frame_cube` gives it (default: computed here); `seq_lens`: the frames of every track, in
    order (default: one track).  `ss = 2` averages 2 x 2 samples per pixel.  `out`: a uint8 [F,size,size,3] tensor to write 'rgb' into.
    Two kernel calls (projection; raster and resolve); F = 0 returns empty tensors without a launch."""
    where = 'render.render_mesh'
    want, lens, prov = _check(verts, faces, cube, seq_lens, size, ss, color, alpha, want, ops, where)
    F, dev = verts.shape[0], verts.device
    if out is None:
        out = torch.empty(F, size, size, 3, dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (F, size, size, 3) or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f'{where}: out must be a contiguous uint8 tensor [{F},{size},{size},3] on {dev}')
    verts, faces = verts.contiguous(), faces.contiguous()
    if cube is None and F:
        cube = frame_cube(verts, lens)
    res = _render(prov, verts, faces, None if cube is None else cube.contiguous(), _seq_ptr(lens, dev) if F else None, size, ss, color, alpha, out, want)
    return {k: res[k] for k in want}


def _pipeline(F, chunk, size, dev, span):
    """The frames [F,size,size,3] (`size` an int) or [F,H,W,3] (`size` = (H, W)) of `span(a, b, rgb)` (which launches the render of frames a .. b - 1 into the device tensor rgb) as host
    arrays, `chunk` frames at a time.  On the device two frame buffers and two pinned host buffers alternate: the copy of one chunk runs on a
    side stream under the render of the next, and the host waits once per chunk, for that chunk's copy."""
    H, W = (size, size) if isinstance(size, int) else size
    spans = [(a, min(a + chunk, F)) for a in range(0, F, chunk)]
    n_buf = min(2, len(spans))
    piped = dev.type == 'cuda'
    dbuf = [torch.empty(min(chunk, F), H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n_buf)]
    hbuf = [torch.empty(min(chunk, F), H, W, 3, dtype=torch.uint8, pin_memory=True) for _ in range(n_buf)] if piped else dbuf
    side = torch.cuda.Stream(device=dev) if piped else None
    copied = [None] * n_buf

    def launch(i):
        a, b = spans[i]
        k = i % n_buf
        rgb = dbuf[k][:b - a]
        if copied[k] is not None:
            torch.cuda.current_stream(dev).wait_event(copied[k])      # the copy that last read this device buffer
        span(a, b, rgb)
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                hbuf[k][:b - a].copy_(rgb, non_blocking=True)
                copied[k] = torch.cuda.Event()
                copied[k].record(side)

    launch(0)
    for i, (a, b) in enumerate(spans):
        if i + 1 < len(spans):
            launch(i + 1)
        if copied[i % n_buf] is not None:
            copied[i % n_buf].synchronize()
        yield hbuf[i % n_buf][:b - a].numpy()


def render_chunks(verts, faces, cube=None, seq_lens=None, size: int = 1024, ss: int = 1, color=MESH_COLOR, alpha: float = MESH_ALPHA,
                  chunk: int = 32, ops=None):
    """A generator of host uint8 arrays [n,size,size,3], n <= `chunk` frames at a time, in frame order: the frames of `render_mesh` without
    ever holding them all.  The cube is that of the whole motion (per track), whatever the chunking.  The frames come through `_pipeline`:
    an array is valid until the generator is advanced again (its buffer is then reused)."""
    where = 'render.render_chunks'
    _, lens, prov = _check(verts, faces, cube, seq_lens, size, ss, color, alpha, ('rgb',), ops, where)
    if not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f'{where}: chunk must be a positive int, got {chunk!r}')
    F, dev = verts.shape[0], verts.device
    if F == 0:
        return
    verts, faces = verts.contiguous(), faces.contiguous()
    cube = (frame_cube(verts, lens) if cube is None else cube).contiguous()
    ptr = _seq_ptr(lens, dev)

    def span(a, b, rgb):
        _render(prov, verts[a:b], faces, cube, (ptr - a).clamp_(0, b - a), size, ss, color, alpha, rgb, ('rgb',))
    yield from _pipeline(F, chunk, size, dev, span)


# ------------------------------------------------------------------------------------------------ skeleton frames (csrc/skeleton.hip)
# vismo.py:262-269: Axes3D with limits x [-512, 0], y [-256, 256], z [-512, 0], view_init(elev=12, azim=80), default perspective.  With fixed
# limits and a fixed view Axes3D.get_proj() is one constant matrix M (matplotlib 3.10.8; tests/golden/skeleton_view.npz holds it as the
# reference's own run gave it): rows 0, 1 and 3 here, then the 2D window of a 3D axes, [-0.95 / dist, 0.9 / dist] at dist = 10, as u_lo, v_hi
# and 1 / width.  The tightly cropped image of the reference is that axes rectangle.
SKELETON_VIEW = tuple(float.fromhex(h) for h in (
    '-0x1.2c21c35e6b437p-9', '0x1.a75eec7dd4bbdp-12', '0x0.0p+0', '-0x1.2c21c35e6b439p-1',
    '-0x1.60184ec9e1feep-14', '-0x1.f33519d378183p-12', '0x1.bf2737751c729p-10', '0x1.a925b2887e52dp-2',
    '-0x1.9e1e7f32e9c01p-12', '-0x1.2592c2d6c7b64p-9', '-0x1.7c2e6ed07e176p-12', '0x1.39cb6623f9304p+3')) + (-0.095, 0.09, 1 / 0.185)
# vismo.py:252-258: the plot order, and the colours by the reference's membership lists
SKELETON_BONES = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (8, 11), (8, 14), (9, 10), (11, 12), (12, 13), (14, 15),
                  (15, 16))
_LEFT, _RIGHT = ((8, 11), (11, 12), (12, 13), (0, 4), (4, 5), (5, 6)), ((8, 14), (14, 15), (15, 16), (0, 1), (1, 2), (2, 3))
COLOR_LEFT, COLOR_RIGHT, COLOR_MID = (0x02, 0x31, 0x5E), (0x2F, 0x70, 0xAF), (0x00, 0x45, 0x7E)
SKELETON_COLORS = tuple(COLOR_LEFT if b in _LEFT else COLOR_RIGHT if b in _RIGHT else COLOR_MID for b in SKELETON_BONES)
REF_FRAME_PX = 924          # the reference's cropped frame: 0.77 of 10 inches at 120 dpi


def _round_div(num, den):
    return (2 * num + den) // (2 * den)


def skeleton_radii(size: int, ss: int = 1):
    """(r_line, r_out, r_in) in 1/16 sample: vismo.py:276 draws lw = 3 pt, markersize = 3 pt and markeredgewidth = 2 pt at 120 dpi (5, 5 and
    10/3 px) in a 924-px frame: line width 5 size / 924 px, marker outer diameter (5 + 10/3) size / 924 px, inner (5 - 10/3) size / 924 px.
    Half of each, in 1/16 of a sample (ss samples per pixel), rounded to nearest."""
    k = 16 * ss * size
    return _round_div(5 * k, 2 * REF_FRAME_PX), _round_div(25 * k, 6 * REF_FRAME_PX), _round_div(5 * k, 6 * REF_FRAME_PX)


def _table(t, dtype, cols, most, name, dev, where):
    """a small per-bone table as a contiguous device tensor [n,cols]: a tensor as it is, host data uploaded"""
    if not isinstance(t, torch.Tensor):
        a = np.asarray(t)
        if a.ndim != 2 or a.shape[1] != cols or a.dtype.kind not in 'iu' or (a.size and (a.min() < torch.iinfo(dtype).min or a.max() > torch.iinfo(dtype).max)):
            raise ValueError(f'{where}: {name} must be integers [n,{cols}] that fit {dtype}, got {a.shape} {a.dtype}')
        t = torch.from_numpy(a.astype(np.uint8 if dtype == torch.uint8 else np.int32)).to(dev)
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols or not 1 <= t.shape[0] <= most or t.device != dev:
        raise ValueError(f'{where}: {name} must be a {dtype} tensor [1 <= n <= {most},{cols}] on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}')
    return t.contiguous()


def _check_skeleton(x3d, size, ss, view, bones, colors, radii, want, ops, where):
    if isinstance(x3d, np.ndarray):                      # the result of `wild.infer` as it comes: uploaded once
        if x3d.dtype != np.float32:
            raise ValueError(f'{where}: x3d must be float32 [F, J, 3], got {x3d.shape} {x3d.dtype}')
        x3d = torch.from_numpy(np.ascontiguousarray(x3d))
        if ops is None:
            if not torch.cuda.is_available():
                raise RuntimeError(f'motionbert_amd.{where} runs on the ROCm device; there is no CPU path')
            x3d = x3d.cuda()
    if (not isinstance(x3d, torch.Tensor) or x3d.dtype != torch.float32 or x3d.dim() != 3 or x3d.shape[2] != 3
            or not 1 <= x3d.shape[1] <= MAX_JOINTS):
        raise ValueError(f'{where}: x3d must be a float32 tensor or array [F, 1 <= J <= {MAX_JOINTS}, 3], got '
                         f'{tuple(x3d.shape) if hasattr(x3d, "shape") else type(x3d).__name__} {getattr(x3d, "dtype", "")}')
    if not isinstance(size, int) or not 1 <= size <= MAX_SIZE:
        raise ValueError(f'{where}: size must be an int in [1, {MAX_SIZE}], got {size!r}')
    if ss not in (1, 2):
        raise ValueError(f'{where}: ss must be 1 or 2, got {ss!r}')
    view = SKELETON_VIEW if view is None else tuple(float(v) for v in np.asarray(view, np.float64).reshape(-1))
    if len(view) != 15 or not all(np.isfinite(view)):
        raise ValueError(f'{where}: view must be 15 finite values (rows 0, 1, 3 of M, u_lo, v_hi, inv_w), got {len(view)}')
    radii = skeleton_radii(size, ss) if radii is None else tuple(radii)
    if (len(radii) != 3 or not all(isinstance(r, (int, np.integer)) for r in radii)
            or not (0 <= radii[0] <= MAX_RADIUS and 0 <= radii[2] <= radii[1] <= MAX_RADIUS)):
        raise ValueError(f'{where}: radii must be ints (r_line, r_out, r_in) with 0 <= r_line <= {MAX_RADIUS} and 0 <= r_in <= r_out <= {MAX_RADIUS}, '
                         f'got {radii!r}')
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in SKELETON_WANT_KEYS for k in want):
        raise ValueError(f'{where}: want must name some of {SKELETON_WANT_KEYS}, got {want!r}')
    dev = x3d.device
    if colors is None and bones is not None:
        raise ValueError(f'{where}: colors must be given with bones, one colour for each')
    bones = _table(SKELETON_BONES if bones is None else bones, torch.int32, 2, MAX_BONES, 'bones', dev, where)
    colors = _table(SKELETON_COLORS if colors is None else colors, torch.uint8, 3, MAX_BONES, 'colors', dev, where)
    if colors.shape[0] != bones.shape[0]:
        raise ValueError(f'{where}: colors must give one colour for each of the {bones.shape[0]} bones, got {colors.shape[0]}')
    prov = hip_ops.provider(ops, 'motionbert_amd.' + where, x3d)
    return x3d.contiguous(), view, bones, colors, tuple(int(r) for r in radii), want, prov


def _render_skeleton(prov, x3d, view, bones, colors, radii, size, ss, rgb, want):
    F, J, S, dev = x3d.shape[0], x3d.shape[1], size * ss, x3d.device
    jq = torch.empty(F, J, 2, dtype=torch.int32, device=dev)
    res = {'rgb': rgb, 'jq': jq, 'prim_id': torch.empty(F, S, S, dtype=torch.int32, device=dev) if 'prim_id' in want else None}
    if F:
        prov.skeleton_project(x3d, view, size, ss, jq)
        prov.skeleton_raster(jq, bones, colors, radii, size, ss, rgb, res['prim_id'])
    return res


def render_skeleton(x3d, size: int = 1024, ss: int = 1, view=None, bones=None, colors=None, radii=None, out=None, want=('rgb',), ops=None):
    """x3d [F,J,3] float32, a device tensor or a host array (uploaded once): the X3D of `wild.infer` -> a dict of device tensors: 'rgb' uint8
    [F,size,size,3] and, where `want` names them, the test hooks 'prim_id' int32 [F,S,S] (S = size ss; the winning primitive 3 bone + (0 the
    line, 1 / 2 the marker at the first / second end), -1 where empty) and 'jq' int32 [F,J,2] (the projected joints).  `view`: 15 float64
    values (default SKELETON_VIEW, the reference's axes); `bones` [Nb,2] / `colors` [Nb,3]: joint pairs in plot order and their colours
    (default: the 16 H36M bones in the reference's colours); `radii` = (r_line, r_out, r_in) in 1/16 sample (default `skeleton_radii`).
    `ss = 2` averages 2 x 2 samples per pixel.  `out`: a uint8 [F,size,size,3] tensor to write 'rgb' into.  Two kernel calls; F = 0
    returns empty tensors without a launch.  One person per frame, in the reference's own view; every tracked person of a video frame in one
    image is `render_scene`."""
    where = 'render.render_skeleton'
    x3d, view, bones, colors, radii, want, prov = _check_skeleton(x3d, size, ss, view, bones, colors, radii, want, ops, where)
    F, dev = x3d.shape[0], x3d.device
    if out is None:
        out = torch.empty(F, size, size, 3, dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (F, size, size, 3) or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f'{where}: out must be a contiguous uint8 tensor [{F},{size},{size},3] on {dev}')
    res = _render_skeleton(prov, x3d, view, bones, colors, radii, size, ss, out, want)
    return {k: res[k] for k in want}


def skeleton_chunks(x3d, size: int = 1024, ss: int = 1, view=None, bones=None, colors=None, radii=None, chunk: int = 32, ops=None):
    """A generator of host uint8 arrays [n,size,size,3], n <= `chunk` frames at a time, in frame order: the frames of `render_skeleton`
    through `_pipeline`, without ever holding them all.  An array is valid until the generator is advanced again."""
    where = 'render.skeleton_chunks'
    x3d, view, bones, colors, radii, _, prov = _check_skeleton(x3d, size, ss, view, bones, colors, radii, ('rgb',), ops, where)
    if not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f'{where}: chunk must be a positive int, got {chunk!r}')
    F = x3d.shape[0]
    if F == 0:
        return

    def span(a, b, rgb):
        _render_skeleton(prov, x3d[a:b], view, bones, colors, radii, size, ss, rgb, ('rgb',))
    yield from _pipeline(F, chunk, size, x3d.device, span)


# ------------------------------------------------------------------------------------------------ crowd frames (csrc/scene.hip)
SCENE_WANT_KEYS = ('rgb', 'prim_id', 'jq')
SCENE_CHUNK = 64                    # MBX_SCENE_CHUNK: the persons a tile culls at a time (the tests place their cases around it)
MAX_PERSONS_PER_FRAME = 1 << 23     # prim_id packs rank 3 Nb + primitive into an int32


def scene_table(frame_ids, n_frames=None, order=None):
    """Who is in which video frame.  `frame_ids`: the dict idx -> int64 [F_idx] of `wild.read_alphapose(by_track=True, frames=True)`, or a
    list of such arrays: the video frame of every row of every track.  Tracks count in the dict's order (the track ordinal), rows count
    through the concatenated tracks, as the rows of the concatenated output of `wild.infer` do.  Returns numpy int32 arrays
    `(frame_ptr [Fv+1], rows [R], person [R])`: video frame f shows the rows `rows[frame_ptr[f]:frame_ptr[f+1]]` in drawing order (a later
    one is drawn on top) and `person[k]` is the track ordinal of entry k, its palette row.  Fv = `n_frames`, or 1 + the largest frame id.
    Drawing order: ascending track ordinal, or, with `order` (a float array [R], one value per row), ascending `order`, stable: for
    example each row's lowest image point, so that nearer people cover farther ones.  ValueError on negative ids, ids >= n_frames, an
    `order` that is not finite or not [R], and on more than 2^23 persons in one frame."""
    where = 'render.scene_table'
    tracks = list(frame_ids.values()) if isinstance(frame_ids, dict) else list(frame_ids)
    ids = []
    for n, t in enumerate(tracks):
        a = np.asarray(t)
        if a.ndim != 1 or (a.size and a.dtype.kind not in 'iu'):
            raise ValueError(f'{where}: the frame ids of track {n} must be a 1-D integer array, got {a.shape} {a.dtype}')
        ids.append(a.astype(np.int64))
    frame = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    person = np.concatenate([np.full(a.size, n, np.int64) for n, a in enumerate(ids)]) if ids else np.zeros(0, np.int64)
    R = frame.size
    if R and frame.min() < 0:
        raise ValueError(f'{where}: negative frame id {int(frame.min())}')
    if n_frames is None:
        Fv = int(frame.max()) + 1 if R else 0
    else:
        Fv = int(n_frames)
        if Fv < 0 or (R and frame.max() >= Fv):
            raise ValueError(f'{where}: frame id {int(frame.max()) if R else None} with n_frames = {n_frames!r}')
    if Fv >= 2 ** 31 - 1 or R >= 2 ** 31:
        raise ValueError(f'{where}: {Fv} frames / {R} rows do not fit the int32 table')
    if order is None:
        by = np.argsort(frame, kind='stable')                                # rows come in track order already
    else:
        order = np.asarray(order)
        if order.shape != (R,) or order.dtype.kind not in 'fiu' or not np.isfinite(order).all():
            raise ValueError(f'{where}: order must be {R} finite values, one per row, got {order.shape} {order.dtype}')
        by = np.lexsort((order.astype(np.float64), frame))                   # stable: by frame, then by order, then by row
    count = np.bincount(frame, minlength=Fv) if R else np.zeros(Fv, np.int64)
    if count.size and count.max() > MAX_PERSONS_PER_FRAME:
        raise ValueError(f'{where}: {int(count.max())} persons in frame {int(count.argmax())}, at most {MAX_PERSONS_PER_FRAME}')
    frame_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    return frame_ptr, by.astype(np.int32), person[by].astype(np.int32)


def _hsv(h, s, v):
    """integer HSV -> RGB: h in [0, 360), s and v in [0, 255]; floor divisions only"""
    k, rem = divmod(h, 60)
    p, q, t = v * (255 - s) // 255, v * (255 * 60 - s * rem) // (255 * 60), v * (255 * 60 - s * (60 - rem)) // (255 * 60)
    return ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[k]


def track_palette(n: int, bones=None):
    """n distinct colour rows for the persons of a scene -> numpy uint8 [n,Nb,3] (`bones` default: the 16 H36M bones).  Person i takes the hue
    137 i mod 360 (the golden angle in whole degrees: 360 hues before one repeats) at one of four saturation / value levels (i // 360), the
    middle bones in that colour, the left ones darker and the right ones paler, as the reference's three blues are.  Integer arithmetic with
    floor divisions only: no RNG and no rounding that numpy and another machine could see differently.  No colour is white.  ValueError for n
    outside [0, 1440]."""
    if not isinstance(n, (int, np.integer)) or not 0 <= n <= 1440:
        raise ValueError(f'render.track_palette: n must be an int in [0, 1440], got {n!r}')
    bones = SKELETON_BONES if bones is None else [tuple(int(j) for j in b) for b in np.asarray(bones).reshape(-1, 2)]
    out = np.zeros((n, len(bones), 3), np.uint8)
    for i in range(n):
        h, level = (137 * i) % 360, i // 360
        s, v = 230 - 40 * level, 235 - 25 * level
        mid, left, right = _hsv(h, s, v), _hsv(h, s, v * 3 // 5), _hsv(h, s * 3 // 5, v)
        for k, b in enumerate(bones):
            out[i, k] = left if b in _LEFT else right if b in _RIGHT else mid
    return out


def _check_scene(x3d, table, width, height, ss, bones, palette, radii, background, want, ops, where):
    """-> (x [R,J,C] on the device, (frame_ptr, rows, person) int32 tensors, bones, palette [P,Nb,3], radii, background (a triple of ints or a
    uint8 tensor [Fv or 1,H,W,3]), want, provider)"""
    if isinstance(x3d, dict):                            # the result of `wild.infer` for a dict of tracks: concatenated in its order
        parts = [v if isinstance(v, np.ndarray) else np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in x3d.values()]
        if not parts or any(a.dtype != np.float32 or a.ndim != 3 or a.shape[1:] != parts[0].shape[1:] for a in parts):
            raise ValueError(f'{where}: x3d as a dict must hold float32 arrays [F_idx, J, 2|3] of one J, got '
                             f'{[(a.shape, str(a.dtype)) for a in parts][:4]}')
        x3d = np.concatenate(parts)
    if isinstance(x3d, np.ndarray):
        if x3d.dtype != np.float32:
            raise ValueError(f'{where}: x3d must be float32 [R, J, 2|3], got {x3d.shape} {x3d.dtype}')
        x3d = torch.from_numpy(np.ascontiguousarray(x3d))
        if ops is None:
            if not torch.cuda.is_available():
                raise RuntimeError(f'motionbert_amd.{where} runs on the ROCm device; there is no CPU path')
            x3d = x3d.cuda()
    if (not isinstance(x3d, torch.Tensor) or x3d.dtype != torch.float32 or x3d.dim() != 3 or x3d.shape[2] not in (2, 3)
            or not 1 <= x3d.shape[1] <= MAX_JOINTS):
        raise ValueError(f'{where}: x3d must be a dict of tracks, or a float32 tensor or array [R, 1 <= J <= {MAX_JOINTS}, 2|3], got '
                         f'{tuple(x3d.shape) if hasattr(x3d, "shape") else type(x3d).__name__} {getattr(x3d, "dtype", "")}')
    dev = x3d.device
    for name, v in (('width', width), ('height', height)):
        if not isinstance(v, int) or not 1 <= v <= MAX_SIZE:
            raise ValueError(f'{where}: {name} must be an int in [1, {MAX_SIZE}], got {v!r}')
    if ss not in (1, 2):
        raise ValueError(f'{where}: ss must be 1 or 2, got {ss!r}')
    if not isinstance(table, (tuple, list)) or len(table) != 3:
        raise ValueError(f'{where}: table must be (frame_ptr, rows, person) as scene_table gives it')
    tab = []
    for name, t in zip(('frame_ptr', 'rows', 'person'), table):
        if not isinstance(t, torch.Tensor):
            a = np.asarray(t)
            if a.ndim != 1 or a.dtype != np.int32:
                raise ValueError(f'{where}: table {name} must be a 1-D int32 array, got {a.shape} {a.dtype}')
            t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if t.dtype != torch.int32 or t.dim() != 1 or t.device != dev:
            raise ValueError(f'{where}: table {name} must be a 1-D int32 tensor on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}')
        tab.append(t.contiguous())
    if tab[0].numel() < 1 or tab[1].numel() != tab[2].numel():
        raise ValueError(f'{where}: table of {tab[0].numel()} frame_ptr / {tab[1].numel()} rows / {tab[2].numel()} person entries')
    Fv = tab[0].numel() - 1
    radii = skeleton_radii(min(width, height), ss) if radii is None else tuple(radii)
    if (len(radii) != 3 or not all(isinstance(r, (int, np.integer)) for r in radii)
            or not (0 <= radii[0] <= MAX_RADIUS and 0 <= radii[2] <= radii[1] <= MAX_RADIUS)):
        raise ValueError(f'{where}: radii must be ints (r_line, r_out, r_in) with 0 <= r_line <= {MAX_RADIUS} and 0 <= r_in <= r_out <= {MAX_RADIUS}, '
                         f'got {radii!r}')
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in SCENE_WANT_KEYS for k in want):
        raise ValueError(f'{where}: want must name some of {SCENE_WANT_KEYS}, got {want!r}')
    if palette is None and bones is not None:
        raise ValueError(f'{where}: palette must be given with bones, one colour for each')
    bones = _table(SKELETON_BONES if bones is None else bones, torch.int32, 2, MAX_BONES, 'bones', dev, where)
    if palette is None:
        palette = np.array(SKELETON_COLORS, np.uint8)[None]
    if not isinstance(palette, torch.Tensor):
        a = np.asarray(palette)
        if a.ndim != 3 or a.dtype.kind not in 'iu' or (a.size and (a.min() < 0 or a.max() > 255)):
            raise ValueError(f'{where}: palette must be integers in [0, 255] [P,Nb,3], got {a.shape} {a.dtype}')
        palette = torch.from_numpy(a.astype(np.uint8)).to(dev)
    if palette.dtype != torch.uint8 or palette.dim() != 3 or palette.shape[0] < 1 or tuple(palette.shape[1:]) != (bones.shape[0], 3) or palette.device != dev:
        raise ValueError(f'{where}: palette must be a uint8 tensor [P >= 1,{bones.shape[0]},3] on {dev}, got {tuple(palette.shape)} {palette.dtype} '
                         f'on {palette.device}')
    if background is None:
        background = (255, 255, 255)
    if isinstance(background, _ReaderFrames):
        background = background.reader
    if hasattr(background, 'read') and hasattr(background, 'frames'):          # a video.MJPEGReader: the video's own frames, decoded per span
        if background.frames != Fv or (background.height, background.width) != (height, width):
            raise ValueError(f'{where}: the background video has {background.frames} frames of {background.height} x {background.width}, the scene '
                             f'{Fv} of {height} x {width}')
        prov = hip_ops.provider(ops, 'motionbert_amd.' + where, x3d)
        return x3d.contiguous(), tuple(tab), bones, palette.contiguous(), tuple(int(r) for r in radii), _ReaderFrames(background, dev, ops), want, prov
    if isinstance(background, np.ndarray) and background.ndim == 4:
        background = torch.from_numpy(np.ascontiguousarray(background)).to(dev)
    if isinstance(background, torch.Tensor):
        if (background.dtype != torch.uint8 or background.dim() != 4 or background.shape[0] not in (1, Fv)
                or tuple(background.shape[1:]) != (height, width, 3) or background.device != dev):
            raise ValueError(f'{where}: background frames must be a uint8 tensor [{Fv} or 1,{height},{width},3] on {dev}, got '
                             f'{tuple(background.shape)} {background.dtype} on {background.device}')
        background = background.contiguous()
    else:
        background = tuple(background)
        if len(background) != 3 or not all(isinstance(c, (int, np.integer)) and 0 <= c <= 255 for c in background):
            raise ValueError(f'{where}: background must be three ints in [0, 255] or uint8 frames [{Fv} or 1,{height},{width},3], got {background!r}')
        background = tuple(int(c) for c in background)
    prov = hip_ops.provider(ops, 'motionbert_amd.' + where, x3d)
    return x3d.contiguous(), tuple(tab), bones, palette.contiguous(), tuple(int(r) for r in radii), background, want, prov


class _ReaderFrames:
    """The background frames of a span from a video.MJPEGReader: decoded into one buffer that grows to the largest span asked for, just before
    the span's render and on its stream, so the whole background never exists on the device."""

    def __init__(self, reader, dev, ops):
        self.reader, self.dev, self.ops, self.buf = reader, dev, ops, None

    def span(self, a, b):
        if self.buf is None or self.buf.shape[0] < b - a:
            self.buf = torch.empty(b - a, self.reader.height, self.reader.width, 3, dtype=torch.uint8, device=self.dev)
        return self.reader.read(a, b, device=self.dev, out=self.buf[:b - a], ops=self.ops)


def _render_scene(prov, jq, tab, a, b, bones, palette, radii, width, height, ss, background, rgb, want):
    """video frames a .. b - 1: frame_ptr[a:b+1] keeps its offsets into the whole rows / person, so a span of frames is the same table"""
    Fv = tab[0].numel() - 1
    if isinstance(background, _ReaderFrames):
        background = background.span(a, b) if b > a else (255, 255, 255)
    elif isinstance(background, torch.Tensor) and background.shape[0] == Fv and Fv != 1:
        background = background[a:b]
    prim_id = torch.empty(b - a, height * ss, width * ss, dtype=torch.int32, device=tab[0].device) if 'prim_id' in want else None
    if b > a:
        prov.scene_raster(jq, tab[0][a:b + 1], tab[1], tab[2], bones, palette, radii, width, height, ss, background, rgb, prim_id)
    return prim_id


def _project_scene(prov, x, ss):
    jq = torch.empty(x.shape[0], x.shape[1], 2, dtype=torch.int32, device=x.device)
    if x.shape[0]:
        prov.scene_project(x, ss, jq)
    return jq


def render_scene(x3d, table, width: int, height: int, ss: int = 1, bones=None, palette=None, radii=None, background=None, out=None, want=('rgb',),
                 ops=None):
    """Every tracked person of a video frame in one image.  `x3d`: the dict idx -> float32 [F_idx,J,2|3] of `wild.infer(..., pixel=True)` (host
    arrays, concatenated in the dict's order and uploaded once) or a device tensor [R,J,2|3], in video pixels; z is not used.  `table` =
    (frame_ptr, rows, person) as `scene_table` gives it for the same tracks (arrays are uploaded, device tensors taken as they are).  Returns a
    dict of device tensors: 'rgb' uint8 [Fv,height,width,3] and, where `want` names them, the test hooks 'prim_id' int32 [Fv, height ss,
    width ss] (rank in the frame's list x 3 Nb + the primitive of `render_skeleton`; -1 where empty) and 'jq' int32 [R,J,2].
    `bones` [Nb,2] and `palette` [P,Nb,3] (or [1,Nb,3] for everybody): default the 16 H36M bones and the reference's three colours for
    everybody (`track_palette(n)` gives one row per person); `radii` default `skeleton_radii(min(width, height), ss)`; `background`: three
    ints (default white), uint8 frames [Fv or 1,height,width,3] (an array or a device tensor), or a `video.MJPEGReader` of Fv frames of that
    size: the video's own frames, decoded on the device.  A later entry of a
    frame's list covers an earlier one.  Table entries that name no row of x3d or no row of the palette are not drawn.  Two kernel calls;
    Fv = 0 returns empty frames without drawing (the projection runs only where 'jq' is wanted)."""
    where = 'render.render_scene'
    x, tab, bones, palette, radii, background, want, prov = _check_scene(x3d, table, width, height, ss, bones, palette, radii, background, want, ops,
                                                                        where)
    Fv, dev = tab[0].numel() - 1, x.device
    if out is None:
        out = torch.empty(Fv, height, width, 3, dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (Fv, height, width, 3) or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f'{where}: out must be a contiguous uint8 tensor [{Fv},{height},{width},3] on {dev}')
    res = {'rgb': out, 'jq': _project_scene(prov, x, ss) if Fv or 'jq' in want else None}
    res['prim_id'] = _render_scene(prov, res['jq'], tab, 0, Fv, bones, palette, radii, width, height, ss, background, out, want)
    return {k: res[k] for k in want}


def scene_chunks(x3d, table, width: int, height: int, ss: int = 1, bones=None, palette=None, radii=None, background=None, chunk: int = 32, ops=None):
    """A generator of host uint8 arrays [n,height,width,3], n <= `chunk` video frames at a time, in frame order: the frames of `render_scene`
    through `_pipeline`, without ever holding them all.  Background frames given per video frame are sliced per chunk; those of a
    `video.MJPEGReader` are decoded per chunk into one chunk-sized buffer, just before the chunk's render.  An array is valid
    until the generator is advanced again."""
    where = 'render.scene_chunks'
    x, tab, bones, palette, radii, background, _, prov = _check_scene(x3d, table, width, height, ss, bones, palette, radii, background, ('rgb',), ops,
                                                                     where)
    if not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f'{where}: chunk must be a positive int, got {chunk!r}')
    Fv = tab[0].numel() - 1
    if Fv == 0:
        return
    jq = _project_scene(prov, x, ss)

    def span(a, b, rgb):
        _render_scene(prov, jq, tab, a, b, bones, palette, radii, width, height, ss, background, rgb, ('rgb',))
    yield from _pipeline(Fv, chunk, (height, width), x.device, span)
