"""What the mesh rasteriser costs per frame on one MI355X, next to the reference's route (matplotlib `plot_trisurf` on the host).

    python tools/render_bench.py [--out profiles/render_bench.txt] [--frames 243] [--reps 5] [--mpl-frames 3]

The synthetic closed surface of tests/rendererr.body_like (6,890 vertices / 13,776 faces, a standing body's proportions, swaying) over 243
frames, one cube for the whole motion.  Configurations: 1024 x 1024 at ss = 1 and ss = 2, 512 x 512 at ss = 1.  After one warm-up pass of
every configuration, alternating repetitions, the median of each:
  (a) render_mesh(verts, faces, cube=, out=) + synchronize: wrapper, projection and the three raster launches, output allocated before;
  (b) render_chunks(chunk=32) drained: the same frames brought to the host through the two pinned buffers, end to end.
Per configuration also: the share of the output-write floor, F size^2 3 bytes over 6.29 TB/s -- the float4 copy rate MI355X_MICROARCH.md
gives for HBM, NOT measured here -- and the share of tiles that took the background exit, computed from the projected vertices with the
kernel's box rule.  The reference's route is timed on THIS host: a figure of 8 x 8 inches, orthographic 3-D axes at elev -90 / azim -90,
`plot_trisurf` of the same faces with the reference's colour, rendered to PNG at 128 dpi (1024 x 1024), per frame.
The only condition fixed in advance: the device render's median time per frame is not above the reference route's."""
from __future__ import annotations

import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import render as R      # noqa: E402
from tests import rendererr as RE           # noqa: E402

HBM_WRITE = 6.29e12
CONFIGS = ((1024, 1), (1024, 2), (512, 1))


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def background_share(vq, S):
    """the share of the tiles of all frames that lie outside the frame's box of vertices inside the guard (the kernel's early exit)"""
    x, y = vq[..., 0].long(), vq[..., 1].long()
    ok = (x.abs() <= RE.GUARD) & (y.abs() <= RE.GUARD)
    big = 1 << 40
    hit = torch.zeros(vq.shape[0], dtype=torch.long, device=vq.device) + 1
    for c in (x, y):
        lo = torch.where(ok, c, big).amin(1)
        hi = torch.where(ok, c, -big).amax(1)
        j0 = ((lo + RE.SUB // 2 - 1) >> 4).clamp(min=0)
        j1 = ((hi - RE.SUB // 2) >> 4).clamp(max=S - 1)
        hit = hit * torch.where(j1 >= j0, j1 // RE.TILE - j0 // RE.TILE + 1, 0)
    tiles = ((S + RE.TILE - 1) // RE.TILE) ** 2
    return 1.0 - hit.sum().item() / (vq.shape[0] * tiles)


def matplotlib_route(verts, faces, frames):
    """seconds per frame of the reference's route on this host, or None without matplotlib"""
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    lo, hi = verts.reshape(-1, 3).min(0), verts.reshape(-1, 3).max(0)
    mid, half = (hi + lo) / 2, (hi - lo).max() / 2
    secs = []
    for f in np.linspace(0, verts.shape[0] - 1, frames).astype(int):
        t0 = time.perf_counter()
        fig = plt.figure(figsize=(8, 8))
        ax = fig.add_subplot(projection='3d', proj_type='ortho')
        ax.set_xlim(mid[0] - half, mid[0] + half)
        ax.set_ylim(mid[1] - half, mid[1] + half)
        ax.set_zlim(mid[2] - half, mid[2] + half)
        ax.view_init(elev=-90, azim=-90)
        ax.set_axis_off()
        ax.plot_trisurf(verts[f, :, 0], verts[f, :, 1], triangles=faces, Z=verts[f, :, 2], color=tuple(c / 255.0 for c in RE.COLOR) + (RE.ALPHA,))
        buf = io.BytesIO()
        fig.savefig(buf, format='png', dpi=128)
        plt.close(fig)
        secs.append(time.perf_counter() - t0)
    return statistics.median(secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, default=243)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--mpl-frames', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'render_bench needs the GPU: there is no CPU timing'
    dev = torch.device('cuda')
    F = args.frames
    verts_h, faces_h = RE.body_like(F, seed=2)
    verts, faces = torch.from_numpy(verts_h).to(dev), torch.from_numpy(faces_h).to(dev)
    cube = R.frame_cube(verts)
    lines = [f'mesh rasteriser on {torch.cuda.get_device_name(0)}: wall clock around call + synchronize, median (min .. max) of {args.reps} alternating '
             f'repetitions after one warm-up pass; {F} frames of {verts.shape[1]} vertices / {faces.shape[0]} faces, one cube for the motion']
    outs = {c: torch.empty(F, c[0], c[0], 3, dtype=torch.uint8, device=dev) for c in CONFIGS}

    def mesh(c):
        return lambda: R.render_mesh(verts, faces, cube=cube, size=c[0], ss=c[1], out=outs[c])

    def chunks(c):
        def run():
            n = 0
            for part in R.render_chunks(verts, faces, cube=cube, size=c[0], ss=c[1], chunk=32):
                n += part.shape[0]
            assert n == F
        return run
    runs = [(('mesh', c), mesh(c)) for c in CONFIGS] + [(('chunks', c), chunks(c)) for c in CONFIGS]
    for _, fn in runs:
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in runs}
    for r in range(args.reps):
        for k, fn in runs:
            ms[k].append(once(fn))
        print(f'repetition {r}: ' + '  '.join(f'{k[0]} {k[1][0]}/ss{k[1][1]} {ms[k][-1]:.1f} ms' for k, _ in runs), flush=True)
    per_frame = {}
    for c in CONFIGS:
        size, ss = c
        m = statistics.median(ms[('mesh', c)])
        e = statistics.median(ms[('chunks', c)])
        per_frame[c] = m / F
        floor_ms = F * size * size * 3 / HBM_WRITE * 1e3
        vq = R.render_mesh(verts, faces, cube=cube, size=size, ss=ss, out=outs[c], want=('vq',))['vq']
        lines.append(f'{size} x {size}, ss = {ss}:')
        lines.append(f'  (a) render_mesh      {m:9.2f} ms ({min(ms[("mesh", c)]):.2f} .. {max(ms[("mesh", c)]):.2f})   {m / F:7.3f} ms/frame  {F / m * 1e3:9.0f} frames/s'
                     f'   output-write floor {floor_ms:.3f} ms = {100 * floor_ms / m:.1f} % of the time (6.29 TB/s: the guide\'s figure, not a run)')
        lines.append(f'  (b) render_chunks    {e:9.2f} ms ({min(ms[("chunks", c)]):.2f} .. {max(ms[("chunks", c)]):.2f})   {e / F:7.3f} ms/frame  {F / e * 1e3:9.0f} frames/s'
                     f'   to the host, {F * size * size * 3 / e / 1e6:.2f} GB/s of frames')
        lines.append(f'      tiles that took the background exit: {100 * background_share(vq, size * ss):.1f} %')
    mpl = matplotlib_route(verts_h, faces_h, args.mpl_frames)
    worst = max(per_frame.values())
    if mpl is None:
        lines.append('the reference\'s route: matplotlib is not installed on this host: not measured')
        ok = False
    else:
        import matplotlib
        lines.append(f'the reference\'s route (matplotlib {matplotlib.__version__} plot_trisurf + savefig at 1024 x 1024, on the host of this GPU, median of '
                     f'{args.mpl_frames} frames): {mpl:.2f} s/frame = {1 / mpl:.2f} frames/s; the device render at 1024 x 1024, ss = 1 is '
                     f'{mpl * 1e3 / per_frame[(1024, 1)]:.0f}x faster per frame')
        ok = worst <= mpl * 1e3
    lines.append(f'acceptance (device median per frame, slowest configuration {worst:.3f} ms, not above the reference route\'s): ' + ('met' if ok else 'NOT met'))
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
