"""Diagnostics (-DMBX_TN_TRACE build): where a chunk of the weight-gradient GEMM (gemm_tn_pipe256_kernel) spends its cycles -- per workgroup,
for the first wave of the leading and of the trailing group: transposed reads + waits | first barrier | LDS-DMA issue + 16 MFMAs | second barrier.
    python tools/build_variants.py tntrace -DMBX_TN_TRACE
    MBX_LIB=tools/variants/libmbx_tntrace.so python tools/tn_trace.py [clips] [N] [K]"""
import sys

import numpy as np
import torch

import trace_common as tc            # (first: it puts the repository root on sys.path)
from motionbert_amd import hip_ops
clips = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
K = int(sys.argv[3]) if len(sys.argv) > 3 else 512
M, dev, BF = clips * 243 * 17, 'cuda', torch.bfloat16
ops = hip_ops.get()
SLOTS, WGS = 5, 4096                 # TN_TRACE_SLOTS (gemm_pipe.hip) for each of the two wave groups of a workgroup; the largest grid this tool takes
buf = tc.arm(ops, 2 * SLOTS * WGS)
g = torch.Generator(device=dev).manual_seed(0)
dy = (torch.randn(M, N, device=dev, generator=g) * 0.5).to(BF)
a = (torch.randn(M, K, device=dev, generator=g) * 0.5).to(BF)
dw, db = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
fn = lambda: ops.gemm_tn(dy, a, dw, db)
ms = tc.timed_launch(fn, buf)
wgs, rest = divmod(int(ops.lib.mbx_diag_last_need()), 2 * SLOTS * 8)      # the split plan is the library's: the grid is read back, the record is this tool's
assert rest == 0 and wgs % 8 == 0, f'the traced launch writes {wgs * 2 * SLOTS * 8 + rest} bytes: not whole records of 2 x {SLOTS} int64 for a grid of 8 n workgroups'
tc.check_need(ops, buf, 2 * SLOTS * wgs)
raw = buf.cpu().numpy()[:2 * SLOTS * wgs].reshape(-1, 2, SLOTS)
raw = raw[raw[:, 0, 4] > 0]
print(f'# gemm_tn_pipe256_kernel dW [{N}, {K}] over M = {M}: {len(raw)} workgroups, launch {ms:.3f} ms (trace build), '
      f'{int(np.median(raw[:, 0, 4]))} chunks of 32 tokens per workgroup; shader cycles per chunk (median over workgroups)')
names = ['transposed reads + waits (+ bias dots)', 'first barrier', 'LDS-DMA issue + 16 MFMAs', 'second barrier']
for w, tag in ((0, 'leading group (wave 0)'), (1, 'trailing group (wave 4)')):
    per = raw[:, w, :4] / raw[:, w, 4:5]
    print(f'{tag}: ' + '   '.join(f'{nm} {np.median(per[:, k]):6.0f}' for k, nm in enumerate(names)) + f'   | chunk {np.median(per.sum(1)):6.0f}')
