"""What drawing a crowd into one video costs on one MI355X: `render.render_scene` next to what the package offered before it for the same picture.

    python tools/scene_bench.py [--out profiles/scene_bench.txt] [--reps 5]

The crowd of the README: 30 tracks with the seeded lengths of tools/ragged_bench.py (uniform in [20, 400]) and seeded, staggered start frames; a
walking H36M skeleton per track (tests/skelerr.walking) placed in video pixels.  In one process, after one warm-up pass of every configuration,
alternating repetitions, the median of each, wall clock around the call and a synchronize (wrappers included):
  (a) 1024 x 1024: render_scene(x, table, out=) -- one projection and one raster launch for all video frames;
  (b) 1024 x 1024: the composed loop: one render_skeleton(want=('rgb', 'prim_id'), out=) per track, under a view that maps the track's pixel
      coordinates onto the image, then per track canvas[frames] = where(prim_id >= 0, rgb, canvas[frames]) with torch operations.  The same
      persons at the same places in the same colours, later tracks over earlier ones;
  (c) 1920 x 1080: render_scene over white, and (d) over per-frame background frames (a uint8 tensor already on the device);
  (e) 1920 x 1080: scene_video end to end into a Motion-JPEG file (chunk 32, quality 90, 4:2:0), over the background frames.
The condition fixed in advance: the median of (a) is not above the median of (b)."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import render as R      # noqa: E402
from motionbert_amd import video as V       # noqa: E402
from tests import skelerr as SE             # noqa: E402
from tools.render_bench import once         # noqa: E402


def crowd(W, H):
    """-> (x3d dict idx -> [F_idx,17,3] f32 in pixels, frame ids dict): the lengths of tools/ragged_bench.py, start frames uniform in [0, 200]"""
    lens = [int(v) for v in np.random.RandomState(2024).randint(20, 401, 30)]
    starts = [int(v) for v in np.random.RandomState(2025).randint(0, 201, 30)]
    g = np.random.default_rng(7)
    x3d, ids = {}, {}
    for k, (n, s) in enumerate(zip(lens, starts)):
        at = np.array([g.uniform(0.1 * W, 0.9 * W), g.uniform(0.35 * H, 0.65 * H), 0.0])
        x3d[k] = (at + 0.3 * H * SE.walking(n, seed=k)).astype(np.float32)
        ids[k] = np.arange(s, s + n, dtype=np.int64)
    return x3d, ids


def pixel_view(size):
    """the 15 values under which render_skeleton draws x_in = x_pix / (size / 2) - 1 at x_pix: W = 1, u = x_pix / size, v = -y_pix / size"""
    return (-1 / 512, 0, 0, 0, 0, 0, 1 / 512, 0, 0, 0, 0, 1, 0.0, 0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'scene_bench needs the GPU: there is no CPU timing'
    dev = torch.device('cuda')
    lines = []

    # ---- 1024 x 1024: the scene against the composed loop
    S = 1024
    x3d, ids = crowd(S, S)
    table = tuple(torch.from_numpy(t).to(dev) for t in R.scene_table(ids))
    Fv, rows = table[0].numel() - 1, table[1].numel()
    x = torch.from_numpy(np.concatenate(list(x3d.values()))).to(dev)
    palette = torch.from_numpy(R.track_palette(len(x3d))).to(dev)
    radii = R.skeleton_radii(S)
    out = torch.empty(Fv, S, S, 3, dtype=torch.uint8, device=dev)
    most = max(len(v) for v in ids.values())
    per_frame = np.diff(R.scene_table(ids)[0])
    lines.append(f'crowd rasteriser on {torch.cuda.get_device_name(0)}: wall clock around call + synchronize, median (min .. max) of {args.reps} alternating '
                 f'repetitions after one warm-up pass; {len(x3d)} tracks of {min(len(v) for v in ids.values())} to {most} frames, {rows} rows in {Fv} video '
                 f'frames, {per_frame.min()} to {per_frame.max()} persons per frame (mean {per_frame.mean():.1f})')

    def scene():
        R.render_scene(x, table, S, S, palette=palette, radii=radii, out=out)

    tracks_in = [(torch.from_numpy(v / np.float32(S / 2) - np.float32(1)).to(dev), torch.from_numpy(ids[k]).to(dev)) for k, v in x3d.items()]
    canvas = torch.empty(Fv, S, S, 3, dtype=torch.uint8, device=dev)
    one_rgb = torch.empty(most, S, S, 3, dtype=torch.uint8, device=dev)
    bones = torch.tensor(R.SKELETON_BONES, dtype=torch.int32, device=dev)
    view = pixel_view(S)

    def composed():
        canvas.fill_(255)
        for k, (xin, frames) in enumerate(tracks_in):
            got = R.render_skeleton(xin, size=S, view=view, bones=bones, colors=palette[k], radii=radii, out=one_rgb[:xin.shape[0]], want=('rgb', 'prim_id'))
            a, b = int(ids[k][0]), int(ids[k][-1]) + 1                       # a track's frames are consecutive here: a slice, no gather
            canvas[a:b] = torch.where((got['prim_id'] >= 0).unsqueeze(-1), got['rgb'], canvas[a:b])

    runs = [('scene', scene), ('composed', composed)]
    for _, fn in runs:
        fn()
    torch.cuda.synchronize()
    differ = int((out != canvas).any(-1).sum())
    ms = {k: [] for k, _ in runs}
    for r in range(args.reps):
        for k, fn in runs:
            ms[k].append(once(fn))
        print(f'repetition {r}: ' + '  '.join(f'{k} {ms[k][-1]:.2f} ms' for k, _ in runs), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    rng = lambda k: f'({min(ms[k]):.2f} .. {max(ms[k]):.2f})'      # noqa: E731
    ok = med['scene'] <= med['composed']
    lines.append(f'{S} x {S}, ss = 1, white background:')
    lines.append(f'  (a) render_scene       {med["scene"]:9.2f} ms {rng("scene")}   {med["scene"] / Fv:7.4f} ms/video frame  {Fv / med["scene"] * 1e3:9.0f} frames/s')
    lines.append(f'  (b) composed loop      {med["composed"]:9.2f} ms {rng("composed")}   {len(x3d)} render_skeleton calls over {rows} frames + torch.where per track'
                 f'   scene / composed = {med["scene"] / med["composed"]:.3f}')
    lines.append(f'      pixels that differ between the two pictures: {differ} of {Fv * S * S} (the view of (b) rounds the coordinates once more)')
    del canvas, one_rgb, out, tracks_in
    torch.cuda.empty_cache()

    # ---- 1920 x 1080
    W, H = 1920, 1080
    x3d, ids = crowd(W, H)
    table = tuple(torch.from_numpy(t).to(dev) for t in R.scene_table(ids))
    x = torch.from_numpy(np.concatenate(list(x3d.values()))).to(dev)
    out = torch.empty(Fv, H, W, 3, dtype=torch.uint8, device=dev)
    i, j = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
    bg = torch.stack([((i + 2 * f) % 200).to(torch.uint8) for f in range(Fv)]).unsqueeze(-1) + torch.stack([j % 50, (i + j) % 40, (i * 3) % 30], -1).to(torch.uint8)
    path = os.path.join(tempfile.mkdtemp(), 'crowd.avi')
    size = {}

    def video():
        size['frames'], size['bytes'] = V.scene_video(path, x, table, W, H, 25, background=bg, palette=palette, chunk=32)

    runs = [('white', lambda: R.render_scene(x, table, W, H, palette=palette, out=out)),
            ('frames', lambda: R.render_scene(x, table, W, H, palette=palette, background=bg, out=out)), ('video', video)]
    for _, fn in runs:
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in runs}
    for r in range(args.reps):
        for k, fn in runs:
            ms[k].append(once(fn))
        print(f'repetition {r}: ' + '  '.join(f'{k} {ms[k][-1]:.2f} ms' for k, _ in runs), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append(f'{W} x {H}, ss = 1, {Fv} video frames:')
    lines.append(f'  (c) render_scene, white        {med["white"]:9.2f} ms {rng("white")}   {med["white"] / Fv:7.4f} ms/video frame  {Fv / med["white"] * 1e3:9.0f} frames/s')
    lines.append(f'  (d) render_scene, over frames  {med["frames"]:9.2f} ms {rng("frames")}   {med["frames"] / Fv:7.4f} ms/video frame  {Fv / med["frames"] * 1e3:9.0f} frames/s'
                 f'   reads {Fv * H * W * 3 / 1e9:.2f} GB of background')
    lines.append(f'  (e) scene_video, over frames   {med["video"]:9.2f} ms {rng("video")}   {med["video"] / Fv:7.4f} ms/video frame  {Fv / med["video"] * 1e3:9.0f} frames/s'
                 f'   {size["frames"]} frames, {size["bytes"] / 1e6:.1f} MB of Motion-JPEG')
    os.remove(path)
    lines.append('acceptance (render_scene median not above the composed loop\'s median at 1024 x 1024): ' + ('met' if ok else 'NOT met'))
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
