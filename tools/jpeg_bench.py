"""What the device JPEG encoder costs per frame on one MI355X, and what a video file costs end to end against frames brought to the host raw.

    python tools/jpeg_bench.py [--out profiles/jpeg_bench.txt] [--frames 243] [--reps 5] [--pillow-frames 12] [--build-host-pillow-ms MS]

In one process, after one warm-up pass of everything, alternating repetitions, the median of each, wall clock around the call and a
synchronize (wrapper included).  243 frames at 1024 x 1024 of three contents: mesh frames (render_mesh of the synthetic 13,776-face body of
tools/render_bench.py), skeleton frames (render_skeleton of tests/skelerr.walking) and uniform noise; quality 90, 4:2:0, one MCU row per restart
interval (the defaults of motionbert_amd.video).
  (a) per content and stage: mbx_jpeg_blocks, mbx_jpeg_entropy_sizes, mbx_jpeg_entropy, each on its own, and encode_jpeg as a whole (with its
      one host read); compressed bytes per frame against the 3,145,728 of a raw frame;
  (b) mesh_video / skeleton_video (chunk 32) into a file, against render_chunks / skeleton_chunks (chunk 32) drained into host memory -- the code
      of the parent commit, the same process; the ratio is recorded, not a condition;
  (c) the host route to the same file: raw frames through render_chunks / skeleton_chunks, each encoded by Pillow (libjpeg-turbo) at the same
      settings, timed on `--pillow-frames` frames on the host of this GPU where Pillow imports; otherwise the figure measured on the build
      machine's CPU is passed in and labelled so.
Conditions fixed in advance: the device path (render, encode, copy of the compressed bytes, file) takes no more time per frame than (c), and
the bytes that cross the host link per frame are fewer than raw."""
from __future__ import annotations

import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import hip_ops          # noqa: E402
from motionbert_amd import render as R      # noqa: E402
from motionbert_amd import video as V       # noqa: E402
from tests import rendererr as RE           # noqa: E402
from tests import skelerr as SE             # noqa: E402
from tools.render_bench import once         # noqa: E402

SIZE, QUALITY, SUB, CHUNK = 1024, 90, '420', 32
RAW = SIZE * SIZE * 3


def pillow_ms(frames):
    """milliseconds per frame of PIL.Image.save(..., 'JPEG') at the bench's settings over host frames [n,size,size,3], or None without Pillow"""
    try:
        from PIL import Image
    except ImportError:
        return None
    restart = V.geometry(SIZE, SIZE, SUB)[0]
    secs = []
    for f in frames:
        t0 = time.perf_counter()
        Image.fromarray(f).save(io.BytesIO(), 'JPEG', quality=QUALITY, subsampling=2, optimize=False, restart_marker_blocks=restart)
        secs.append(time.perf_counter() - t0)
    return statistics.median(secs) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, default=243)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--pillow-frames', type=int, default=12)
    ap.add_argument('--build-host-pillow-ms', type=float, nargs=2, default=None, metavar=('MESH', 'SKELETON'),
                    help='Pillow ms/frame (mesh, skeleton content) measured on the build machine, used where Pillow does not import here')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'jpeg_bench needs the GPU: there is no CPU timing'
    dev, F, ops = torch.device('cuda'), args.frames, hip_ops.get()
    x3d = torch.from_numpy(SE.walking(F, seed=2)).to(dev)
    verts_h, faces_h = RE.body_like(F, seed=2)
    verts, faces = torch.from_numpy(verts_h).to(dev), torch.from_numpy(faces_h).to(dev)
    cube = R.frame_cube(verts)
    rgb = torch.empty(F, SIZE, SIZE, 3, dtype=torch.uint8, device=dev)
    mx, my, bpm = V.geometry(SIZE, SIZE, SUB)
    restart, sub = mx, V.SUBSAMPLINGS.index(SUB)
    coef = torch.empty(F, mx * my, bpm, 64, dtype=torch.int16, device=dev)
    offsets = torch.empty(F + 1, dtype=torch.int64, device=dev)
    ws = ops.jpeg_ws(F, SIZE, SIZE, sub, restart, dev)
    lines = [f'device JPEG encoder on {torch.cuda.get_device_name(0)}: wall clock around call + synchronize, median (min .. max) of {args.reps} alternating '
             f'repetitions after one warm-up pass; {F} frames at {SIZE} x {SIZE}, quality {QUALITY}, 4:2:0, restart interval {restart} MCUs '
             f'({my} intervals per frame); a raw frame is {RAW} bytes']
    contents = {'mesh': lambda: R.render_mesh(verts, faces, cube=cube, size=SIZE, out=rgb),
                'skeleton': lambda: R.render_skeleton(x3d, size=SIZE, out=rgb),
                'noise': lambda: rgb.random_(0, 256)}
    tmp = tempfile.mkdtemp()
    ok, per_frame, host_sample = True, {}, {}
    # ---------------------------------------------------------------------------------------- (a) the stages
    for name, fill in contents.items():
        fill()
        torch.cuda.synchronize()
        host_sample[name] = rgb[::max(F // args.pillow_frames, 1)][:args.pillow_frames].cpu().numpy()
        data = [None]

        def emit():
            ops.jpeg_emit(coef, SIZE, SIZE, sub, QUALITY, restart, offsets, data[0], ws)
        runs = [('blocks', lambda: ops.jpeg_blocks(rgb, QUALITY, sub, coef)),
                ('sizes', lambda: ops.jpeg_sizes(coef, SIZE, SIZE, sub, QUALITY, restart, offsets, ws)),
                ('emit', emit),
                ('encode_jpeg', lambda: V.encode_jpeg(rgb, QUALITY, SUB))]
        runs[0][1](), runs[1][1]()
        total = int(offsets[F])
        data[0] = torch.empty(total, dtype=torch.uint8, device=dev)
        for _, fn in runs:
            fn()
        ms = {k: [] for k, _ in runs}
        for r in range(args.reps):
            for k, fn in runs:
                ms[k].append(once(fn))
        per_frame[name] = total / F
        ok = ok and total / F < RAW
        lines.append(f'(a) {name} frames: {total / F:11.0f} bytes/frame compressed = 1 / {RAW * F / total:.1f} of raw')
        for k, _ in runs:
            m = statistics.median(ms[k])
            lines.append(f'    {k:12s} {m:9.2f} ms ({min(ms[k]):.2f} .. {max(ms[k]):.2f})   {m / F * 1e3:8.2f} us/frame  {F / m * 1e3:9.0f} frames/s')
    # ---------------------------------------------------------------------------------------- (b) files against raw frames on the host
    def drain(gen):
        n = 0
        for part in gen:
            n += part.shape[0]
        assert n == F
    runs = [('mesh_video', lambda: V.mesh_video(os.path.join(tmp, 'mesh.avi'), verts, faces, 30, cube=cube, size=SIZE, chunk=CHUNK)),
            ('render_chunks', lambda: drain(R.render_chunks(verts, faces, cube=cube, size=SIZE, chunk=CHUNK))),
            ('skeleton_video', lambda: V.skeleton_video(os.path.join(tmp, 'x3d.avi'), x3d, 30, size=SIZE, chunk=CHUNK)),
            ('skeleton_chunks', lambda: drain(R.skeleton_chunks(x3d, size=SIZE, chunk=CHUNK)))]
    for _, fn in runs:
        fn()
    ms = {k: [] for k, _ in runs}
    for r in range(args.reps):
        for k, fn in runs:
            ms[k].append(once(fn))
        print(f'repetition {r}: ' + '  '.join(f'{k} {ms[k][-1]:.1f} ms' for k, _ in runs), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    sizes = {k: os.path.getsize(os.path.join(tmp, f)) for k, f in (('mesh_video', 'mesh.avi'), ('skeleton_video', 'x3d.avi'))}
    lines.append(f'(b) into a file (chunk {CHUNK}, a temporary directory) against raw frames into host memory (the parent commit\'s path), the same process:')
    for k, _ in runs:
        extra = f'   file {sizes[k]} bytes = {sizes[k] / F:.0f} bytes/frame over the host link against {RAW}' if k in sizes else f'   {RAW} bytes/frame over the host link'
        lines.append(f'    {k:16s} {med[k]:9.2f} ms ({min(ms[k]):.2f} .. {max(ms[k]):.2f})   {F / med[k] * 1e3:9.0f} frames/s{extra}')
    for v, c in (('mesh_video', 'render_chunks'), ('skeleton_video', 'skeleton_chunks')):
        lines.append(f'    {v} / {c} = {med[v] / med[c]:.3f} in time (recorded, not a condition)')
        ok = ok and sizes[v] / F < RAW
    # ---------------------------------------------------------------------------------------- (c) the host route
    for k, (v, c) in (('mesh', ('mesh_video', 'render_chunks')), ('skeleton', ('skeleton_video', 'skeleton_chunks'))):
        p = pillow_ms(host_sample[k])
        label = f'Pillow on the host of this GPU, median of {len(host_sample[k])} frames'
        if p is None and args.build_host_pillow_ms is not None:
            p = args.build_host_pillow_ms[0 if k == 'mesh' else 1]
            label = 'Pillow does not import on the GPU machine: timed on the BUILD machine\'s CPU and passed in'
        if p is None:
            lines.append(f'(c) {k}: Pillow does not import here and no build-machine figure was given: not measured')
            ok = False
            continue
        host = med[c] / F + p
        lines.append(f'(c) {k}: host route = {c} {med[c] / F:.3f} ms/frame + Pillow {p:.3f} ms/frame ({label}) = {host:.3f} ms/frame; device path '
                     f'{med[v] / F:.3f} ms/frame: {host / (med[v] / F):.1f}x')
        ok = ok and med[v] / F <= host
    lines.append('acceptance (device path not slower than raw copy + host encoder; fewer bytes over the host link than raw): ' + ('met' if ok else 'NOT met'))
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
