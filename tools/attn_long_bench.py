"""Temporal attention at long sequence lengths: forward and backward of the resident (T <= 256) and streamed (T > 256, csrc/
attention_stream.hip) kernels at B = 64 clips, H = 8, J = 17, head dim 64 and 32, bf16.  TFLOP/s by the SURVEY 8(d) convention:
4 L^2 hd per problem forward, twice that backward.  Times here are CUDA-event averages over back-to-back launches; per-kernel times
come from a separate run under `rocprofv3 --kernel-trace --stats`.  `--e2e` adds one end-to-end number (report only):
MotionBERT-Lite forward + backward at B = 8, T = 486, bf16, clips/s.

    python tools/attn_long_bench.py [--iters N] [--e2e]
"""
import argparse
import json
import os
import sys
from functools import partial

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motionbert_amd import hip_ops                  # noqa: E402
from motionbert_amd.engine import MODE_TEMPORAL    # noqa: E402

B, H, J = 64, 8, 17
LENGTHS = (243, 256, 257, 486, 972)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def attention(iters):
    ops, rows = hip_ops.get(), []
    for hd in (64, 32):
        for T in LENGTHS:
            C, M = H * hd, B * T * J
            g = torch.Generator(device='cuda').manual_seed(T)
            qkv = torch.randn(M, 3 * C, device='cuda', generator=g).to(torch.bfloat16)
            do = torch.randn(M, C, device='cuda', generator=g).to(torch.bfloat16)
            o, lse = torch.empty(M, C, device='cuda', dtype=torch.bfloat16), torch.empty(M, H, device='cuda')
            dqkv = torch.empty(M, 3 * C, device='cuda', dtype=torch.bfloat16)
            scale = hd ** -0.5
            tf = timed(lambda: ops.attn_fwd(qkv, o, lse, B, T, J, H, scale, MODE_TEMPORAL), iters)
            tb = timed(lambda: ops.attn_bwd(qkv, o, do, lse, dqkv, B, T, J, H, scale, MODE_TEMPORAL), iters)
            flop = 4.0 * T * T * hd * B * J * H
            rows.append(dict(hd=hd, T=T, path='resident' if T <= 256 else 'streamed', fwd_ms=round(tf, 4),
                             fwd_tflops=round(flop / tf / 1e9, 1), bwd_ms=round(tb, 4), bwd_tflops=round(2 * flop / tb / 1e9, 1)))
            print(json.dumps(rows[-1]), flush=True)
            del qkv, do, o, lse, dqkv
    return rows


def floors(rows):
    """The speed floors at hd = 64: streamed T = 486 against resident T = 243, measured in the same call."""
    r = {(x['hd'], x['T']): x for x in rows}
    ref, new = r[(64, 243)], r[(64, 486)]
    f = dict(fwd_ratio=round(new['fwd_tflops'] / ref['fwd_tflops'], 3), fwd_floor=0.5,
             bwd_ratio=round(new['bwd_tflops'] / ref['bwd_tflops'], 3), bwd_floor=0.4)
    f['met'] = f['fwd_ratio'] >= 0.5 and f['bwd_ratio'] >= 0.4
    return f


def end_to_end(iters):
    from motionbert_amd import DSTformer
    torch.manual_seed(0)
    model = DSTformer(dim_in=3, dim_out=3, dim_feat=256, dim_rep=512, depth=5, num_heads=8, mlp_ratio=4, num_joints=17, maxlen=486,
                      norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)).cuda()
    model.precision = 'bf16'
    x = torch.rand(8, 486, 17, 3, device='cuda') * 2 - 1

    def step():
        model.zero_grad(set_to_none=True)
        model(x).square().mean().backward()
    ms = timed(step, iters)
    return dict(model='MotionBERT-Lite', B=8, T=486, precision='bf16', step_ms=round(ms, 3), clips_per_s=round(8 / ms * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--e2e', action='store_true')
    a = ap.parse_args()
    rows = attention(a.iters)
    print(json.dumps(dict(floors=floors(rows))), flush=True)
    if a.e2e:
        print(json.dumps(dict(end_to_end=end_to_end(max(3, a.iters // 4)))), flush=True)


if __name__ == '__main__':
    main()
