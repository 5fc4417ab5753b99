"""What the one-launch 2D front end of pre-training costs next to the same result composed from the entry points that existed before it, on
one MI355X.

    python tools/motion2d_bench.py [--out profiles/motion2d_bench.txt] [--reps 200]

Shapes [64, 81, 17, 3] (InstaVariety) and [64, 30, 17, 3] (PoseTrack's clip length), everything resident on the device, the draws given.
  fused     augment.motion2d_input(x, want=data, gt, conf, x_aug; noise and mask on; rootrel): one launch of mbx_motion2d_input
  composed  a crop-only augment.action_input on x[:, None], torch.where (zeroing), data.flip_batch, the root subtraction,
            Augmenter2D.augment2D (mbx_augment2d) -- the parent commit's entry points; the [N,9] parameter rows are built outside the timing
Both go through their Python wrappers (output allocation included): that is what a training loop pays.  Before anything is timed the two
results are compared bit for bit.  Method: 20 warm-up passes of both, then `reps` (>= 200) timed repetitions of each, ALTERNATING fused and
composed so that drift of the host hits both alike; every repetition sits between two HIP events and ends in an event synchronise; medians
and the 10th / 90th percentiles are reported.  A second figure per side: the host clock around `reps` back-to-back calls ended by one device
synchronise, per call -- the rate at which a loop that does not wait can issue them.  The acceptance condition is that the fused median is
not above the composed median (exit status 1 otherwise)."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import motion2derr as ME      # noqa: E402

SHAPES = ((64, 81, 17), (64, 30, 17))


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stream_rate(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    reps = max(200, args.reps)
    assert torch.cuda.is_available(), 'motion2d_bench needs an MI355X'
    from motionbert_amd.augment import action_input, motion2d_input
    from motionbert_amd.data import flip_batch
    dev = 'cuda'
    aug = ME.AugConfig(np.load(os.path.join(ROOT, 'tests/golden/augment2d.npz'))).augmenter()
    lines = [f'2D pre-training front end on {torch.cuda.get_device_name(0)} (one device): microseconds per call, median (p10 .. p90) of {reps} '
             'repetitions between HIP events, fused and composed alternating, after 20 warm-up passes; "issue" = host clock around '
             f'{reps} back-to-back calls and one synchronise, per call']
    ok = True
    for shape in SHAPES:
        N, T, J = shape
        x = ME.motion_inputs(N, T, J, 9000 + T).to(dev)
        p = ME.draw_params(N, 9100 + T).to(dev)
        p9 = torch.zeros(N, 9, device=dev)
        p9[:, 8] = p[:, 0]
        which = p[:, 1] < 0.5
        seed = 9200 + T

        def fused():
            return motion2d_input(x, aug=aug, noise=True, mask=True, rootrel=True, want=ME.OUTPUTS, seed=seed, params=p)

        def composed():
            d = action_input(x[:, None], random_move=False, scale_range=ME.SCALE_RANGE, params=p9)[:, 0]
            d = torch.where(d[..., 2:] == 0, torch.zeros_like(d), d)
            d = flip_batch(d, which)
            return dict(data=d, gt=d - d[:, :, 0:1, :], conf=d[..., 2:], x_aug=aug.augment2D(d, noise=True, mask=True, seed=seed))
        a, b = fused(), composed()
        same = all(torch.equal(a[k], b[k]) for k in ME.OUTPUTS)
        for _ in range(20):
            fused()
            composed()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(reps):
            tf.append(one(fused))
            tc.append(one(composed))
        sf, sc = stream_rate(fused, reps), stream_rate(composed, reps)
        q = lambda v: (float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90)))          # noqa: E731
        (mf, lf, hf), (mc, lc, hc) = q(tf), q(tc)
        kb = N * T * J * 3 * 4 / 1024
        lines.append(f'[{N}, {T}, {J}, 3] ({kb:.0f} KB in; data, gt, x_aug of that size and conf a third of it out); results bit-equal: {same}')
        lines.append(f'  fused     1 launch (mbx_motion2d_input)                                  {mf:8.1f} us ({lf:.1f} .. {hf:.1f})   issue {sf:8.1f} us')
        lines.append(f'  composed  action_input + where + flip_batch + subtraction + augment2D    {mc:8.1f} us ({lc:.1f} .. {hc:.1f})   issue {sc:8.1f} us')
        lines.append(f'  composed / fused: {mc / mf:.2f} x between events, {sc / sf:.2f} x issue rate')
        print('\n'.join(lines[-4:]), flush=True)
        ok = ok and same and mf <= mc
    lines.append('acceptance (fused median <= composed median, results bit-equal): ' + ('met' if ok else 'NOT met'))
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
