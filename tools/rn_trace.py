"""Diagnostics (-DMBX_RN_TRACE build): where a 128-row tile of the row-owner LayerNorm-backward GEMM (mbx_rows_lnbwd_t) spends its time in
situ -- eleven time stamps per workgroup, all workgroups of one launch.
    python tools/build_variants.py rntrace -DMBX_RN_TRACE
    MBX_LIB=tools/variants/libmbx_rntrace.so python tools/rn_trace.py [clips] [K]"""
import sys

import numpy as np
import torch

import trace_common as tc            # (first: it puts the repository root on sys.path)
from motionbert_amd import hip_ops
clips = int(sys.argv[1]) if len(sys.argv) > 1 else 64
K = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
N, M, dev, BF = 512, clips * 243 * 17, 'cuda', torch.bfloat16
tiles = (M + 127) // 128
ops = hip_ops.get()
SLOTS = 12                           # RN_TRACE_SLOTS (gemm_rows_n.hip): eleven stamps and the hardware id per workgroup
buf = tc.arm(ops, SLOTS * tiles)
g = torch.Generator(device=dev).manual_seed(0)
dy = (torch.randn(M, K, device=dev, generator=g) * 0.5).to(BF)
w = (torch.randn(N, K, device=dev, generator=g) * 0.05).to(BF)
xhat = torch.randn(M, N, device=dev, generator=g).to(BF)
rstd = torch.rand(M, device=dev, generator=g) + 0.5
dres = torch.randn(M, N, device=dev, generator=g).to(BF)
out = torch.empty(M, N, device=dev, dtype=BF)
packed = ops.rows_n_pack(w)
fn = lambda: ops.rows_lnbwd_t(dy, packed, xhat, rstd, dres, out)
ms = tc.timed_launch(fn, buf)
tc.check_need(ops, buf, SLOTS * tiles)
raw = tc.records(buf, tiles, SLOTS)
us = tc.to_us(raw[:, :11])
CUT = 256                            # not the first and not the last round
names = ['prologue (first stage and tokens landed)', 'loop', 'drain + barrier', 'xhat registers -> LDS', 'pass 1 (row means) + row constants',
         'pass 2 quarter 0 (dx, stores issued)', 'pass 2 quarter 1', 'pass 2 quarter 2', 'pass 2 quarter 3', 'stores acknowledged']
print(f'# rows_n_lnbwd_kernel at {clips} clips, K = {K}: {tiles} tiles ({len(raw)} workgroups), launch {ms:.3f} ms (trace build); steady-state tiles: {len(tc.steady(us, CUT))}')
print('\n'.join(tc.phase_table(us, names, CUT, 52)))
# gaps between consecutive workgroups on the same CU (hardware id in column 11)
hw = raw[:, 11]
gaps = tc.same_cu_gaps(us, hw, 10)
if len(gaps):
    print(f'# gap between a workgroup\'s last store acknowledged and the next workgroup\'s entry on the same CU: median {np.median(gaps):.2f} us '
          f'(10th / 90th percentile {np.percentile(gaps, 10):.2f} / {np.percentile(gaps, 90):.2f}); workgroups per CU: {len(raw) / len(np.unique(hw)):.2f}')
