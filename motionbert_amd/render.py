"""Mesh video frames on the device (csrc/render.hip): the last line of infer_wild_mesh.py, `render_and_save` -> `vismo.motion2video_mesh`,
as compute.  An Instinct has no graphics pipeline; the frames are drawn by an exact fixed-point tile rasteriser instead (include/mbx.h has
the definition: orthographic along +z, image x right with mesh x, image y down with mesh y, inside the bounding cube of the whole motion,
z-buffered and flat-shaded, white background).

    frame_cube(verts, seq_lens=None)        [n_tracks,4] = (cx, cy, cz, 1 / (2 R)) per track over ALL its frames, torch operations on the device
    render_mesh(verts, faces, ...)          verts [F,V,3] + faces [Nf,3] -> {'rgb': uint8 [F,size,size,3]} (+ the test hooks 'face_id', 'depth',
                                            'vq') as device tensors
    render_chunks(verts, faces, ...)        generator of host uint8 [n,size,size,3] arrays, `chunk` frames at a time through two pinned
                                            buffers: 4,960 frames at 1024 x 1024 are 15.6 GB and cannot be one tensor

Not here: video encoding, the skeleton videos of `motion2video_3d`, smooth shading, other cameras, several persons in one frame.

There is no CPU path: without an injected kernel provider (`ops=`), tensors that are not on a ROCm device raise."""
from __future__ import annotations

import numpy as np
import torch

from . import hip_ops

MAX_SIZE, SUB, ZQ = 2048, 16, 1 << 20
WANT_KEYS = ('rgb', 'face_id', 'depth', 'vq')
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


def render_chunks(verts, faces, cube=None, seq_lens=None, size: int = 1024, ss: int = 1, color=MESH_COLOR, alpha: float = MESH_ALPHA,
                  chunk: int = 32, ops=None):
    """A generator of host uint8 arrays [n,size,size,3], n <= `chunk` frames at a time, in frame order: the frames of `render_mesh` without
    ever holding them all.  The cube is that of the whole motion (per track), whatever the chunking.  On the device two frame buffers and two
    pinned host buffers alternate: the copy of one chunk runs on a side stream under the render of the next, and the host waits once per
    chunk, for that chunk's copy.  An array is valid until the generator is advanced again (its buffer is then reused)."""
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
    spans = [(a, min(a + chunk, F)) for a in range(0, F, chunk)]
    n_buf = min(2, len(spans))
    piped = verts.is_cuda
    dbuf = [torch.empty(min(chunk, F), size, size, 3, dtype=torch.uint8, device=dev) for _ in range(n_buf)]
    hbuf = [torch.empty(min(chunk, F), size, size, 3, dtype=torch.uint8, pin_memory=True) for _ in range(n_buf)] if piped else dbuf
    side = torch.cuda.Stream(device=dev) if piped else None
    copied = [None] * n_buf

    def launch(i):
        a, b = spans[i]
        k = i % n_buf
        rgb = dbuf[k][:b - a]
        if copied[k] is not None:
            torch.cuda.current_stream(dev).wait_event(copied[k])      # the copy that last read this device buffer
        _render(prov, verts[a:b], faces, cube, (ptr - a).clamp_(0, b - a), size, ss, color, alpha, rgb, ('rgb',))
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
