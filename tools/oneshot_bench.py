"""What the one-shot kernels cost next to the torch operations they replace, on one MI355X.

    python tools/oneshot_bench.py [--out profiles/oneshot_bench.txt]

HIP events around 20 timed passes after 5 warm-up passes (median, and the spread); recorded, no threshold:
  (i)   mbx_supcon_loss at (bsz, n_views, D) = (32, 1, 2048), the shape of configs/action/MB_*_NTU120_oneshot.yaml: loss and gradient
        through the normalisation in one call -- against the same torch operations on the same device: F.normalize, then the project's
        own statement of the loss (tests/supconerr.supcon_terms64: logits, row maximum, masked exp-sum, log-probabilities, mean over the
        positives) in fp32, then autograd's backward;
  (ii)  mbx_nn_cosine at (M, N, D) = (20, N, 2048), N = 4,096 and 32,768 -- against the torch operations a validation over a test split
        runs (train_action_1shot.py:61-66): the [M, N, D] broadcast of F.cosine_similarity and argmax, with torch.cuda.max_memory_allocated
        around it.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import supconerr as SC      # noqa: E402


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
    g = torch.Generator().manual_seed(0)
    lines = [f'one-shot kernels on {torch.cuda.get_device_name(0)}: HIP events, median (min .. max) of 20 passes after 5 warm-up passes']

    def say(name, t):
        lines.append(f'  {name:72s} {t[0] * 1e3:9.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f})')
        print(lines[-1], flush=True)

    # (i) the loss of one training step
    z = torch.randn(32, 1, 2048, generator=g).to(dev)
    lab = (torch.arange(32) // 2)[torch.randperm(32, generator=g)].to(dev)
    lab32 = lab.to(torch.int32)
    loss, dz = torch.empty(1, device=dev), torch.empty_like(z)
    lines.append('(i) SupCon loss and gradient at (bsz, n_views, D) = (32, 1, 2048), temperature 0.1, through the L2 normalisation')
    say('mbx_supcon_loss (loss + dfeat, normalize=1): 3 launches', timed(lambda: ops.supcon_loss(z, lab32, 0.1, 0.07, True, loss, dz)))
    say('mbx_supcon_loss (loss only)', timed(lambda: ops.supcon_loss(z, lab32, 0.1, 0.07, True, loss, None)))
    zt = z.clone().requires_grad_(True)

    t, tb = SC.f32(0.1), SC.f32(0.07)

    def torch_loss():
        return SC.supcon_terms64(torch.nn.functional.normalize(zt.reshape(32, 2048), dim=-1), lab, t, tb)

    def torch_step():
        zt.grad = None
        torch_loss().backward()
    say('torch: F.normalize + the same loss in torch operations (fp32) + backward', timed(torch_step))
    with torch.no_grad():
        say('torch: F.normalize + the same loss in torch operations, forward only', timed(torch_loss))

    # (ii) the evaluation
    for N in (4096, 32768):
        a = torch.nn.functional.normalize(torch.randn(20, 2048, generator=g), dim=-1).to(dev)
        t = torch.nn.functional.normalize(torch.randn(N, 2048, generator=g), dim=-1).to(dev)
        al = torch.arange(20, dtype=torch.int32, device=dev)
        tl = (torch.arange(N, dtype=torch.int32) % 20).to(dev)
        pred, hits = torch.empty(N, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        lines.append(f'(ii) 1-NN by cosine similarity at (M, N, D) = (20, {N}, 2048): {N * 2048 * 4 / 2 ** 20:.0f} MiB of test embeddings')
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        say('mbx_nn_cosine (labels, hit count)', timed(lambda: ops.nn_cosine(a, al, t, tl, pred, None, hits)))
        lines.append(f'      peak memory above the inputs: {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.1f} MiB')

        def ref():
            dis = torch.nn.functional.cosine_similarity(a.unsqueeze(1), t.unsqueeze(0), dim=-1)
            p = al[torch.argmax(dis, dim=0)]
            return (p == tl).sum()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        say('torch: F.cosine_similarity over the [M, N, D] broadcast + argmax', timed(ref))
        lines.append(f'      peak memory above the inputs: {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.1f} MiB')
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
