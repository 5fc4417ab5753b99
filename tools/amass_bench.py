"""What the AMASS joints kernel costs next to the plain torch formulation, on one MI355X.

    python tools/amass_bench.py [--out profiles/amass_bench.txt] [--frames 2916] [--verts 6890] [--reps 15]

F = 2,916 frames (the slice of the reference's tools/preprocess_amass.py), a synthetic SMPL-H + DMPL model of the real size (V = 6,890, weight
rows with at most 4 non-zeros), K = 17, camera step included.  Two regressors span the pair list: one vertex per regressed joint (Np small)
and full support (Np = 17 x 52 = 884, the dense maximum).  Per Np, alternating repetitions after warm-up passes, the median of each:
  (a) amass_joints(camera=True): wrapper and launch, the exact-fp32 MFMA product (the default);
  (b) the same with the product on the vector unit (flags bit 1: the measured alternative);
  (c) PlainSMPLH of tests/amasserr.py in float32 torch operations on the same device: what a user without the kernel runs (the regressor on
      the shaped vertices, chained 4x4 transforms, the [F,V,4,4] tensor, Q @ vertices, the camera step), with its peak allocation.
Wall clock around call + synchronize (the wrapper is part of what is measured); the two launches also alone, between HIP events.  The
product's FLOPs are 2 x 3 Np x 484 x F; its share of the fp32 rate is taken against 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz = 157.3 TFLOP/s,
over the time of the WHOLE call or launch (rotations, chain and transforms included), so it understates the product loop.  The acceptance condition is only (a) <= (c) at both Np."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import amass as AM      # noqa: E402
from motionbert_amd import hip_ops          # noqa: E402
from tests import amasserr as AE            # noqa: E402

PEAK_F32 = 256 * 4 * 64 * 2.4e9


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, reps):
    """median HIP-event time of `fn` issued back to back (ms): the launch without the wait of the host"""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, default=2916)
    ap.add_argument('--verts', type=int, default=6890)
    ap.add_argument('--reps', type=int, default=15)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'amass_bench needs the GPU: there is no CPU timing'
    dev = torch.device('cuda')
    F, V = args.frames, args.verts
    inp = {k: v.to(dev) for k, v in AE.inputs(F, 3, max_angle=2.0).items()}
    lines = [f'AMASS joints on {torch.cuda.get_device_name(0)}: wall clock around call + synchronize, median (min .. max) of {args.reps} alternating '
             f'repetitions after 3 warm-up passes; F = {F} frames, V = {V} vertices, K = 17, camera step included']
    ok = True
    for label, support in (('one vertex per regressed joint', 1), ('full regressor support', None)):
        model = AM.SMPLHModel.synthetic(V, 1, regressor_support=support)
        md, ops = model.tensors(dev), hip_ops.get()
        plain = AE.PlainSMPLH(model)
        kp = torch.empty(F, 17, 3, dtype=torch.float32, device=dev)

        def run_mfma():
            AM.amass_joints(model, inp['poses'], inp['betas'], inp['dmpls'], inp['trans'], camera=True)

        def run_fma():
            ops.amass_joints(md, inp['poses'], inp['betas'], inp['dmpls'], inp['trans'], kp, camera=True, fma=True)

        def run_plain():
            with torch.no_grad():
                plain(inp['poses'], inp['betas'], inp['dmpls'], inp['trans'], camera=True)

        runs = (('(a) kernel, MFMA product', run_mfma), ('(b) kernel, vector-unit product', run_fma), ('(c) plain torch operations, fp32', run_plain))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(3):
            run_plain()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        for _ in range(3):
            run_mfma()
            run_fma()
        ms = {name: [] for name, _ in runs}
        for _ in range(args.reps):
            for name, fn in runs:
                ms[name].append(once(fn))
        flops = 2.0 * 3 * model.Np * AM.FEAT * F
        lines.append(f'{label}: Np = {model.Np} pairs, P {model.Np * 3 * AM.FEAT * 4 / 1e6:.2f} MB, product {flops / 1e9:.2f} GFLOP')
        med = {}
        for name, _ in runs:
            med[name] = statistics.median(ms[name])
            extra = ''
            if name[1] in 'ab':
                extra = f'   product {flops / (med[name] * 1e-3) / 1e12:6.2f} TFLOP/s = {100 * flops / (med[name] * 1e-3) / PEAK_F32:5.1f} % of the fp32 rate'
            lines.append(f'  {name:36s} {med[name] * 1e3:10.1f} us ({min(ms[name]) * 1e3:.1f} .. {max(ms[name]) * 1e3:.1f})   {F / (med[name] * 1e-3):12.0f} frames/s{extra}')
            print(lines[-1], flush=True)
        a, b, c = (med[name] for name, _ in runs)

        def launch_mfma():
            ops.amass_joints(md, inp['poses'], inp['betas'], inp['dmpls'], inp['trans'], kp, camera=True)
        ea, eb = events(launch_mfma, 4 * args.reps), events(run_fma, 4 * args.reps)
        lines.append(f'      the launch alone (HIP events around the binding, output allocated before): MFMA {ea * 1e3:.1f} us = '
                     f'{100 * flops / (ea * 1e-3) / PEAK_F32:.1f} % of the fp32 rate for the product, vector unit {eb * 1e3:.1f} us = '
                     f'{100 * flops / (eb * 1e-3) / PEAK_F32:.1f} %')
        lines.append(f'      plain / kernel {c / a:.1f}x; vector-unit / MFMA {b / a:.2f}x; plain path peak allocation above the inputs {peak / 1e6:.0f} MB '
                     f'(the kernel: the {F * 17 * 12 / 1e3:.0f} KB of its output)')
        ok = ok and a <= c
    lines.append('acceptance (kernel median <= plain median at both Np): ' + ('met' if ok else 'NOT met'))
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
