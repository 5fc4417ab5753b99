#!/usr/bin/env python
"""HIP-event times of `pose_loss_full`, of `pose_loss`, and of the same eight quantities (with the gradient) through torch ops on the device,
at the training step's size (64, 243, 17): the record in profiles/pose_loss_full.txt.  Nothing is gated on these numbers.

    python tools/time_pose_loss_full.py [OUT.txt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import hip_ops                      # noqa: E402
from tests import limberr as LM                         # noqa: E402


def timed(fn, warmup=10, iters=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    B, T = 64, 243
    ops = hip_ops.get()
    pred, gt = LM.limb_inputs(B, T, LM.SEEDS[(B, T)], 'cuda')
    l8, l4, dpred = torch.empty(8, device='cuda'), torch.empty(4, device='cuda'), torch.empty_like(pred)
    w7 = LM.weights7(LM.LAMBDAS)

    def torch_ops():
        p = pred.detach().requires_grad_(True)
        t = LM.terms64(p, gt)                 # the reference's formulas with torch ops, here in fp32
        sum(w * v for w, v in zip(w7, t)).backward()

    rows = [('pose_loss_full, all six lambdas nonzero, with dpred', lambda: ops.pose_loss_full(pred, gt, LM.LAMBDAS, l8, dpred)),
            ('pose_loss_full, the four new lambdas 0, with dpred', lambda: ops.pose_loss_full(pred, gt, LM.LAMBDAS_BASE, l8, dpred)),
            ('pose_loss_full, scalars only (dpred = NULL)', lambda: ops.pose_loss_full(pred, gt, LM.LAMBDAS, l8, None)),
            ('pose_loss (three terms), with dpred', lambda: ops.pose_loss(pred, gt, 0.5, 20.0, l4, dpred)),
            ('torch ops on the device: seven losses + autograd, fp32', torch_ops)]
    lines = [f'{torch.cuda.get_device_name(0)}; pred, gt [{B},{T},17,3] fp32; HIP events around one call, median (min .. max) of 50 after 10 warm-up calls, microseconds',
             '(host launch cost included: the torch-ops row is about a hundred launches issued from Python)']
    for name, fn in rows:
        med, lo, hi = timed(fn)
        lines.append(f'{name:60s} {med:9.1f}  ({lo:.1f} .. {hi:.1f})')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
