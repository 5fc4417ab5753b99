"""What in-the-wild inference costs through `motionbert_amd.wild.infer` next to the reference's loop, on one MI355X.

    python tools/wild_bench.py [--out profiles/wild_bench.txt] [--reps 5]

A video of 20 clips x 243 frames + a tail of 100 (4960 frames) per person, for one person and for four, through the full model and
MotionBERT-Lite (bf16, the models' default precision).  Recorded, no threshold, no ratio promised:
  path A  `wild.infer`: one upload, mbx_wild_input, pooled batches through flip_tta, mbx_wild_output, one device-to-host copy;
  path B  the reference's loop (infer_wild.py:63-96 as tests/wilderr.reference_loop restates it) through the SAME model, person after
          person: batch 1, two forwards per clip, flip_data deep copies, a .cpu() per clip -- from the input stage's output, which is
          timed separately for both paths.
Host clock around calls that end in a device-to-host copy (path A's last step, path B's per-clip .cpu()) or an explicit synchronise
(the device input stage).  Every shape is run once before the timed window; A and B alternate inside one process; median (min .. max)
of --reps passes.  The host input stage (numpy, one thread) is timed on the CPU of the GPU machine this tool runs on.
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

CLIP, CLIPS, TAIL = 243, 20, 100


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/wild_bench.py measures on the ROCm device; none found')
    from motionbert_amd import DSTformer, wild
    dev = torch.device('cuda', 0)
    F = CLIPS * CLIP + TAIL
    lines = [f'in-the-wild inference on {torch.cuda.get_device_name(0)}: {F} frames per person ({CLIPS} clips x {CLIP} + a tail of {TAIL}), flip on, '
             f'crop mode; host clock, median (min .. max) of {args.reps} alternating passes after one warm-up pass per shape']

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def fmt(t):
        return f'{t[0] * 1e3:10.2f} ms ({t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f})'

    people = {n: {k: WE.detections(F, 9000 + k) for k in range(n)} for n in (1, 4)}
    # ---- the two input stages, on their own
    say('input stage (halpe2h36m + crop_scale), per run of all persons:')
    for n, tracks in people.items():
        kp, lens = np.concatenate(list(tracks.values())), [F] * n
        host, devt = [], []
        wild.wild_input(kp, scale_range=[1, 1], seq_lens=lens)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ref = WE.input_ref(kp, None, [1, 1], lens)[0]
            host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            y = wild.wild_input(kp, scale_range=[1, 1], seq_lens=lens)
            torch.cuda.synchronize()
            devt.append(time.perf_counter() - t0)
        same = WE.differing(y.cpu().numpy(), ref) == 0
        say(f'  {n} person(s): numpy on this host (the CPU of the GPU machine), one thread {fmt(stats(host))}')
        say(f'  {n} person(s): upload of [{n * F},26,3] float64 + mbx_wild_input (3 launches) + synchronise {fmt(stats(devt))}   equal bits: {same}')
    # ---- the two loops
    for label, cfg in (('full model (dim_feat 512, depth 5)', bench.FULL), ('MotionBERT-Lite (dim_feat 256, depth 5)', bench.LITE)):
        torch.manual_seed(0)
        model = DSTformer(norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **cfg).to(dev).eval()
        say(f'{label}, precision {model.precision}:')
        for n, tracks in people.items():
            motions = {k: WE.input_ref(v, None, [1, 1])[0] for k, v in tracks.items()}

            def path_a():
                return wild.infer(model, tracks, clip_len=CLIP)

            def path_b():
                return {k: WE.reference_loop(model, m, CLIP, True, False, False, False, device=dev) for k, m in motions.items()}

            a, b = path_a(), path_b()                                    # warm every shape of both paths
            worst = max(float(np.abs(a[k].astype(np.float64) - b[k]).max()) for k in tracks)
            ta, tb = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                path_a()
                ta.append(time.perf_counter() - t0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                path_b()
                tb.append(time.perf_counter() - t0)
            clips = n * (CLIPS + 1)
            sa, sb = stats(ta), stats(tb)
            say(f'  {n} person(s), {clips} clips: A wild.infer (input stage included)        {fmt(sa)}   {n * F / sa[0]:10.0f} frames/s')
            say(f'  {n} person(s), {clips} clips: B reference loop (input stage NOT included) {fmt(sb)}   {n * F / sb[0]:10.0f} frames/s')
            say(f'  {n} person(s): worst |A - B| {worst:.3e} (normalised coordinates; the two paths run the network at different batch sizes)')
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
