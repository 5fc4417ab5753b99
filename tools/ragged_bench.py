"""What `wild.infer(batching='ragged')` costs next to `batching='equal'` (the default, the path before ragged batches existed), on one
MI355X, in the same build and the same process.

    python tools/ragged_bench.py [--out profiles/ragged_bench.txt] [--reps 7]

  workload A, crowd   30 tracks with seeded lengths uniform in [20, 400]: up to 30 distinct tail lengths, each a batch-1 forward of its
                      own on the equal-length path; whole clips packed into ceil(frames / (64 x 243)) forwards on the ragged path
  workload B          four persons x 4,960 frames (20 clips x 243 + a tail of 100 each): 80 full clips and four equal tails -- the case the
                      equal-length path was built for
Full model and MotionBERT-Lite, bf16, flip on, crop mode.  Host clock around whole `wild.infer` calls (wrapper, input stage, uploads
and the final device-to-host copy included); every shape of both paths is run once before the timed window; the two paths alternate
inside one process; median (min .. max) of --reps passes.  Also mbx_attn_fwd_ragged alone against the per-clip mbx_attn_fwd launches for
workload A's table (full model's shape, HIP events around `--inner` back-to-back repetitions).  Recorded; the acceptance condition on A
is only that the ragged median is not above the equal-length median.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                  # noqa: E402  (the model configurations)
from tests import wilderr as WE              # noqa: E402

CLIP = 243


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/ragged_bench.py measures on the ROCm device; none found')
    from motionbert_amd import DSTformer, hip_ops, wild
    from motionbert_amd.engine import MODE_TEMPORAL
    from motionbert_amd.model import ragged_tables
    dev = torch.device('cuda', 0)
    lines = [f'ragged batches on {torch.cuda.get_device_name(0)}: wild.infer(batching=...) end to end, clip_len {CLIP}, max_batch 64, flip on, crop mode, '
             f'bf16; host clock, median (min .. max) of {args.reps} alternating passes after one warm-up pass per path']

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def fmt(t):
        return f'{t[0] * 1e3:9.2f} ms ({t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f})'

    crowd_lens = [int(v) for v in np.random.RandomState(2024).randint(20, 401, 30)]
    loads = (('A crowd', {k: WE.detections(n, 9100 + k) for k, n in enumerate(crowd_lens)}),
             ('B four persons', {k: WE.detections(4960, 9000 + k) for k in range(4)}))
    for name, tracks in loads:
        lens = [len(v) for v in tracks.values()]
        eq = sum(math_ceil(len(offs), 64) for _, offs in wild.clip_plan(lens, CLIP))
        rg = len(wild.ragged_plan(lens, CLIP, 64 * CLIP))
        say(f'workload {name}: {len(lens)} tracks, {sum(lens)} frames, {sum(math_ceil(n, CLIP) for n in lens)} clips; network calls: equal {eq}, ragged {rg}')
    for label, cfg in (('full model (dim_feat 512, depth 5)', bench.FULL), ('MotionBERT-Lite (dim_feat 256, depth 5)', bench.LITE)):
        torch.manual_seed(0)
        model = DSTformer(norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **cfg).to(dev).eval()
        say(f'{label}, precision {model.precision}:')
        for name, tracks in loads:
            frames = sum(len(v) for v in tracks.values())
            paths = {b: (lambda b=b: wild.infer(model, tracks, clip_len=CLIP, batching=b)) for b in ('equal', 'ragged')}
            first = {b: f() for b, f in paths.items()}                   # warm every shape of both paths
            worst = max(float(np.abs(first['equal'][k].astype(np.float64) - first['ragged'][k]).max()) for k in tracks)
            ts = {b: [] for b in paths}
            for _ in range(args.reps):
                for b, f in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    ts[b].append(time.perf_counter() - t0)
            se, sr = stats(ts['equal']), stats(ts['ragged'])
            say(f'  {name:15s} equal  {fmt(se)}   {frames / se[0]:9.0f} frames/s')
            say(f'  {name:15s} ragged {fmt(sr)}   {frames / sr[0]:9.0f} frames/s   ragged / equal {sr[0] / se[0]:.3f}   worst |ragged - equal| {worst:.3e}')
    # ---- the temporal attention kernel alone, workload A's clips, the full model's shape
    ops = hip_ops.get()
    J, H, hd = 17, 8, 64
    clips = [c for _, cl in wild.ragged_plan(crowd_lens, CLIP, 1 << 30) for c in cl]
    tab_h, _, max_len = ragged_tables(clips)
    F = int(tab_h[:, 1].sum())
    qkv = torch.randn(F * J, 3 * H * hd, device=dev).to(torch.bfloat16)
    o, lse = torch.empty(F * J, H * hd, device=dev, dtype=torch.bfloat16), torch.empty(F * J, H, device=dev)
    tab = torch.from_numpy(tab_h).to(dev)
    rows = [(int(a) * J, int(a + n) * J, int(n)) for a, n in tab_h]

    def ragged():
        ops.attn_fwd_ragged(qkv, o, lse, tab, len(clips), F, max_len, J, H, hd ** -0.5)

    def per_clip():
        for r0, r1, L in rows:
            ops.attn_fwd(qkv[r0:r1], o[r0:r1], lse[r0:r1], 1, L, J, H, hd ** -0.5, MODE_TEMPORAL)

    res = {}
    for fn in (ragged, per_clip):
        fn()
    for _ in range(args.reps):
        for fn in (ragged, per_clip):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(fn.__name__, []).append(e0.elapsed_time(e1) * 1e-3 / args.inner)
    sr, sp = stats(res['ragged']), stats(res['per_clip'])
    say(f'temporal attention alone, workload A ({len(clips)} clips, {F} frames, H {H}, hd {hd}, bf16; HIP events, {args.inner} back-to-back repetitions):')
    say(f'  mbx_attn_fwd_ragged, one launch              {fmt(sr)}')
    say(f'  mbx_attn_fwd per clip, {len(clips)} launches            {fmt(sp)}   ragged / per clip {sr[0] / sp[0]:.3f}')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def math_ceil(a, b):
    return -(-a // b)


if __name__ == '__main__':
    main()
