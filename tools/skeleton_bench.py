"""What the skeleton rasteriser costs per frame on one MI355X, next to the mesh rasteriser and to the reference's route (16 matplotlib
`ax.plot` calls in a 3D figure per frame, on the host).

    python tools/skeleton_bench.py [--out profiles/skeleton_bench.txt] [--frames 243] [--reps 5] [--mpl-frames 3]

In one process, after one warm-up pass of every configuration, alternating repetitions, the median of each, wall clock around the call and a
synchronize (wrapper included), 243 frames at 1024 x 1024, ss = 1 and ss = 2:
  (a) render_skeleton(x3d, out=) of tests/skelerr.walking: 17 joints, 16 bones, 48 primitives per frame;
  (b) render_mesh(verts, faces, cube=, out=) of the synthetic 13,776-face body of tools/render_bench.py;
  (c) skeleton_chunks(chunk=32) drained: the skeleton frames brought to the host through the two pinned buffers.
Next to (a): the output-write floor, F size^2 3 bytes over 6.29 TB/s -- the float4 copy rate MI355X_MICROARCH.md gives for HBM, NOT
measured here.  The reference's route is timed on THIS host where matplotlib imports: a plain restatement of the figure of vismo.py:259-284
(10 x 10 inches, the limits, view_init(12, 80), the 16 plots, savefig at 120 dpi with a tight box); a recorded comparison, not a condition.
The condition fixed in advance: at both ss the skeleton median is not above the mesh median (at most 48 primitives per frame against 13,776
faces)."""
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
from tests import skelerr as SE             # noqa: E402
from tools.render_bench import HBM_WRITE, once      # noqa: E402

SIZE = 1024
CONFIGS = (1, 2)


def matplotlib_route(x3d, frames):
    """seconds per frame of the reference's route on this host, or None without matplotlib"""
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    world = (x3d + np.array([1, 1, 0], np.float32)) * 512 / 2
    secs = []
    for f in np.linspace(0, x3d.shape[0] - 1, frames).astype(int):
        t0 = time.perf_counter()
        fig = plt.figure(0, figsize=(10, 10))
        ax = plt.axes(projection='3d')
        ax.set_xlim(-512, 0)
        ax.set_ylim(-256, 256)
        ax.set_zlim(-512, 0)
        ax.view_init(elev=12., azim=80)
        plt.tick_params(left=False, right=False, labelleft=False, labelbottom=False, bottom=False)
        for (a, b), colour in zip(R.SKELETON_BONES, R.SKELETON_COLORS):
            xs, ys, zs = world[f, [a, b]].T
            ax.plot(-xs, -zs, -ys, color=tuple(c / 255.0 for c in colour), lw=3, marker='o', markerfacecolor='w', markersize=3, markeredgewidth=2)
        buf = io.BytesIO()
        fig.savefig(buf, format='png', dpi=120, bbox_inches='tight', pad_inches=0)
        plt.close()
        secs.append(time.perf_counter() - t0)
    return statistics.median(secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, default=243)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--mpl-frames', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'skeleton_bench needs the GPU: there is no CPU timing'
    dev = torch.device('cuda')
    F = args.frames
    x_h = SE.walking(F, seed=2)
    x3d = torch.from_numpy(x_h).to(dev)
    verts_h, faces_h = RE.body_like(F, seed=2)
    verts, faces = torch.from_numpy(verts_h).to(dev), torch.from_numpy(faces_h).to(dev)
    cube = R.frame_cube(verts)
    out = torch.empty(F, SIZE, SIZE, 3, dtype=torch.uint8, device=dev)
    lines = [f'skeleton rasteriser on {torch.cuda.get_device_name(0)}: wall clock around call + synchronize, median (min .. max) of {args.reps} alternating '
             f'repetitions after one warm-up pass; {F} frames at {SIZE} x {SIZE}; skeleton: 17 joints / 16 bones; mesh: {verts.shape[1]} vertices / '
             f'{faces.shape[0]} faces']

    def chunks(ss):
        def run():
            n = 0
            for part in R.skeleton_chunks(x3d, size=SIZE, ss=ss, chunk=32):
                n += part.shape[0]
            assert n == F
        return run
    runs = []
    for ss in CONFIGS:
        runs += [(('skeleton', ss), lambda ss=ss: R.render_skeleton(x3d, size=SIZE, ss=ss, out=out)),
                 (('mesh', ss), lambda ss=ss: R.render_mesh(verts, faces, cube=cube, size=SIZE, ss=ss, out=out)),
                 (('chunks', ss), chunks(ss))]
    for _, fn in runs:
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in runs}
    for r in range(args.reps):
        for k, fn in runs:
            ms[k].append(once(fn))
        print(f'repetition {r}: ' + '  '.join(f'{k[0]} ss{k[1]} {ms[k][-1]:.2f} ms' for k, _ in runs), flush=True)
    floor_ms = F * SIZE * SIZE * 3 / HBM_WRITE * 1e3
    ok = True
    med = {k: statistics.median(v) for k, v in ms.items()}
    for ss in CONFIGS:
        s, m, e = med[('skeleton', ss)], med[('mesh', ss)], med[('chunks', ss)]
        ok = ok and s <= m
        rng = lambda k: f'({min(ms[k]):.2f} .. {max(ms[k]):.2f})'      # noqa: E731
        lines.append(f'{SIZE} x {SIZE}, ss = {ss}:')
        lines.append(f'  (a) render_skeleton  {s:9.2f} ms {rng(("skeleton", ss))}   {s / F:7.4f} ms/frame  {F / s * 1e3:9.0f} frames/s'
                     f'   output-write floor {floor_ms:.3f} ms = {100 * floor_ms / s:.1f} % of the time (6.29 TB/s: the guide\'s figure, not a run)')
        lines.append(f'  (b) render_mesh      {m:9.2f} ms {rng(("mesh", ss))}   {m / F:7.4f} ms/frame  {F / m * 1e3:9.0f} frames/s'
                     f'   skeleton / mesh = {s / m:.3f}')
        lines.append(f'  (c) skeleton_chunks  {e:9.2f} ms {rng(("chunks", ss))}   {e / F:7.4f} ms/frame  {F / e * 1e3:9.0f} frames/s'
                     f'   to the host, {F * SIZE * SIZE * 3 / e / 1e6:.2f} GB/s of frames')
    mpl = matplotlib_route(x_h, args.mpl_frames)
    if mpl is None:
        lines.append('the reference\'s route: matplotlib is not installed on this host: not measured')
    else:
        import matplotlib
        lines.append(f'the reference\'s route (matplotlib {matplotlib.__version__}, 16 ax.plot calls in a 3D figure + savefig at 120 dpi, on the host of this GPU, '
                     f'median of {args.mpl_frames} frames): {mpl:.3f} s/frame = {1 / mpl:.2f} frames/s; the device render at ss = 1 is '
                     f'{mpl * 1e3 / (med[("skeleton", 1)] / F):.0f}x faster per frame (recorded, not a condition)')
    lines.append('acceptance (skeleton median not above the mesh median, ss = 1 and ss = 2): ' + ('met' if ok else 'NOT met'))
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
