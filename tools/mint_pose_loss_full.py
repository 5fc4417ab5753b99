#!/usr/bin/env python
"""Mint tests/golden/pose_loss_full.npz with the REFERENCE's own lib/model/loss.py (imported read-only at run time from the checkout
oracle/make_golden.py names: MOTIONBERT_REFERENCE): the seven losses of train.py:177-184, the weighted total of :185-191 with all six
lambdas nonzero, the autograd gradient of the total and of each term with respect to the prediction, in float64.

    python tools/mint_pose_loss_full.py

Inputs come from tests/limberr.limb_inputs (values exact in fp32, stored as float64; gt root-relative).  Per tag (B, T):
    a (3, 7), t1 (2, 1), t2 (2, 2), b (2, 243):   {tag}.pred, {tag}.gt, {tag}.losses [8], {tag}.dpred, {tag}.dterms [7, ...]
For `b` the seven per-term gradients are kept for the frames {tag}.dterm_frames only (the first and last eight of each clip): all of
them would take the file past the size a committed fixture may have.  The total gradient is kept whole for every tag."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import import_reference_loss      # noqa: E402
from tests import limberr as LM                            # noqa: E402

LAMBDAS = (0.5, 20.0, 0.25, 0.5, 0.125, 2.0)      # scale, 3d_velocity, lv, lg, a, av: all exact in fp32
CASES = (('a', 3, 7, 11), ('t1', 2, 1, 12), ('t2', 2, 2, 13), ('b', 2, 243, 15))      # tag, B, T, seed


def main():
    L = import_reference_loss()
    fns = (lambda p, g: L.loss_mpjpe(p, g), lambda p, g: L.n_mpjpe(p, g), lambda p, g: L.loss_velocity(p, g), lambda p, g: L.loss_limb_var(p),
           lambda p, g: L.loss_limb_gt(p, g), lambda p, g: L.loss_angle(p, g), lambda p, g: L.loss_angle_velocity(p, g))
    save = {'lambdas': np.asarray(LAMBDAS, dtype=np.float64)}
    for tag, B, T, seed in CASES:
        pred32, gt32 = LM.limb_inputs(B, T, seed, 'cpu')
        gt = gt32.double()
        assert float(gt[:, :, 0].abs().max()) == 0.0
        terms, dterms = [], []
        for fn in fns:
            p = pred32.double().requires_grad_(True)
            v = fn(p, gt).double()
            if v.requires_grad:
                v.backward()
            terms.append(float(v.detach()))
            dterms.append(p.grad.numpy().copy() if p.grad is not None else np.zeros((B, T, 17, 3)))
        p = pred32.double().requires_grad_(True)
        total = sum(w * fn(p, gt).double() for w, fn in zip((1.0,) + LAMBDAS, fns))
        total.backward()
        dterms = np.stack(dterms)
        save.update({f'{tag}.pred': pred32.double().numpy(), f'{tag}.gt': gt.numpy(), f'{tag}.losses': np.asarray(terms + [float(total.detach())]),
                     f'{tag}.dpred': p.grad.numpy()})
        if B * T > 64:
            frames = np.asarray([b * T + t for b in range(B) for t in list(range(8)) + list(range(T - 8, T))])
            save[f'{tag}.dterm_frames'] = frames
            save[f'{tag}.dterms'] = dterms.reshape(7, B * T, 17, 3)[:, frames]
        else:
            save[f'{tag}.dterms'] = dterms
        print(f'[pose_loss_full {tag}] ' + ' '.join(f'{n} {v:.6f}' for n, v in zip(LM.NAMES, terms + [float(total.detach())])))
    out = os.path.join(ROOT, 'tests/golden', 'pose_loss_full.npz')
    np.savez_compressed(out, **save)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
