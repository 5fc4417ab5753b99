"""What the action-recognition kernels cost next to the torch operations they replace, on one MI355X.

    python tools/action_bench.py [--out profiles/action_bench.txt]

HIP events around 20 timed passes after 5 warm-up passes (median, and the spread); recorded, no threshold:
  (i)   mbx_action_input at [32, 2, 243, 17, 3] (random_move + crop_scale of a training batch, one launch): microseconds and GB/s of the
        tensor read once and written once -- against the same transformation as batched torch operations on the same device (the fp32
        evaluation of tests/actionerr.action_input_eq, the draws given);
  (ii)  mbx_xent_topk at (N, C) = (32, 60) and (32, 120): loss, gradient and top-1 / top-5 hits in one launch -- against torch's
        cross_entropy forward + backward and the reference's accuracy() (topk, eq, two sums).
The reference's own input stage runs on the HOST, per sample, in numpy: 4.2 ms per [2, 243, 17, 3] sample, one thread.  That figure was
taken on the build machine's CPU, NOT on the GPU host this tool runs on; it is quoted in the output as such and not measured here.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import actionerr as AE      # noqa: E402


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from motionbert_amd import hip_ops
    ops = hip_ops.get()
    dev = 'cuda'
    lines = [f'action-recognition kernels on {torch.cuda.get_device_name(0)}: HIP events, median (min .. max) of 20 passes after 5 warm-up passes']

    def say(name, t, extra=''):
        lines.append(f'  {name:84s} {t[0] * 1e3:9.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f}){extra}')
        print(lines[-1], flush=True)

    # (i) the input stage of one training batch
    shape = (32, 2, 243, 17, 3)
    x = AE.motion_inputs(*shape[:4], 1).to(dev)
    p = AE.draw_params(32, 5).to(dev)
    y, pout = torch.empty_like(x), torch.empty(32, 9, device=dev)
    ranges = AE.RANGES + (AE.CROP_DEFAULT,)
    nbytes = 2 * x.numel() * 4
    lines.append(f'(i) random_move + crop_scale at {list(shape)}: {x.numel() * 4 / 2 ** 20:.2f} MiB in, as much out')
    t = timed(lambda: ops.action_input(x, y, None, pout, ranges, 3, 1234))
    say('mbx_action_input (draws from the seed, params_out): 1 launch', t, f'  {nbytes / t[0] / 1e6:.1f} GB/s of one read + one write')
    t = timed(lambda: ops.action_input(x, y, p, None, ranges, 3, 0))
    say('mbx_action_input (params_in)', t, f'  {nbytes / t[0] / 1e6:.1f} GB/s')
    t = timed(lambda: ops.action_input(x, y, p, None, ranges, 2, 0))
    say('mbx_action_input (crop only: the validation loader)', t, f'  {nbytes / t[0] / 1e6:.1f} GB/s')
    with torch.no_grad():
        say('torch: the same equations as batched fp32 operations on the device (draws given)', timed(lambda: AE.action_input_eq(x, p, 3, torch.float32)))
    lines.append('  reference, for scale: NTURGBD.__getitem__ in numpy on the host, one thread: 4.2 ms per sample = 134 ms per batch of 32 '
                 '(measured on the BUILD machine\'s CPU, not on this host; not measured by this tool)')

    # (ii) loss, gradient and accuracy of one step
    for N, C in ((32, 60), (32, 120)):
        zh, labh = AE.logit_inputs(N, C, 3)
        z, lab = zh.to(dev), labh.to(dev)
        lab32 = lab.to(torch.int32)
        values, d, acc = torch.empty(3, device=dev), torch.empty_like(z), torch.zeros(4, dtype=torch.float64, device=dev)
        lines.append(f'(ii) cross-entropy, gradient and top-1 / top-5 hits at (N, C) = ({N}, {C})')
        say('mbx_xent_topk (values + dlogits + fp64 meter): 1 launch', timed(lambda: ops.xent_topk(z, lab32, values, d, acc)))
        say('mbx_xent_topk (values + meter: validation)', timed(lambda: ops.xent_topk(z, lab32, values, None, acc)))
        zt = z.clone().requires_grad_(True)

        def torch_step():
            zt.grad = None
            loss = torch.nn.functional.cross_entropy(zt, lab)
            loss.backward()
            with torch.no_grad():
                _, pred = zt.topk(5, 1, True, True)
                correct = pred.t().eq(lab.view(1, -1).expand(5, -1))
                return loss, correct[:1].reshape(-1).float().sum(0), correct[:5].reshape(-1).float().sum(0)
        say('torch: cross_entropy forward + backward + topk / eq / sums (no .item())', timed(torch_step))
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
