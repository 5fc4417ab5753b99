"""Diagnostics (-DMBX_ROWS_TRACE build): where a 128-row tile of the row-owner qkv kernel (mbx_rows_gemm_nk_ln: LayerNorm + qkv from the
fp32 rows, N = 1536, K = 512) spends its time in situ -- six time stamps per workgroup, all workgroups of one launch.
    python tools/build_variants.py rowstrace -DMBX_ROWS_TRACE
    MBX_LIB=tools/variants/libmbx_rowstrace.so python tools/rows_trace.py [clips]"""
import sys

import numpy as np
import torch

import trace_common as tc            # (first: it puts the repository root on sys.path)
from motionbert_amd import hip_ops
clips = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N, K, M, dev, BF = 1536, 512, clips * 243 * 17, 'cuda', torch.bfloat16
tiles = (M + 127) // 128
ops = hip_ops.get()
SLOTS = 8                            # ROWS_TRACE_SLOTS (gemm_rows.hip): six stamps, the hardware id, the shader cycles per workgroup
# the launcher's grid: whole rounds of the chip (two workgroups per CU) as whole tiles, the tiles of the last round in `parts` column ranges
slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
nfull = tiles // slots * slots
parts = next((p for p in range(8, 1, -1) if (N // 64) % p == 0 and (tiles - nfull) * p <= slots), 1)
wgs = tiles if parts == 1 else nfull + (tiles - nfull) * parts
buf = tc.arm(ops, SLOTS * wgs)
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(M, K, device=dev, generator=g)
w = (torch.randn(N, K, device=dev, generator=g) * 0.05).to(BF)
bias = torch.randn(N, device=dev, generator=g)
rsum = w.float().sum(1)
packed = ops.rows_pack_nk(w)
out = torch.empty(M, N, device=dev, dtype=BF)
fn = lambda: ops.rows_gemm_nk_ln(x, packed, bias, rsum, 1e-6, out)
ms = tc.timed_launch(fn, buf)
tc.check_need(ops, buf, SLOTS * wgs)
raw = tc.records(buf, wgs, SLOTS)
full = raw[:(tiles // 512) * 512] if tiles >= 512 else raw
us = tc.to_us(full[:, :6])
names = ['prologue (fp32 rows -> operand + statistics, first stages landed)', 'chunk 0 (two 32-column tiles)', 'chunks 1 .. n/2', 'chunks n/2 .. n', 'last epilogue + stores acknowledged']
dur = np.diff(us, axis=1)
total = us[:, 5] - us[:, 0]
print(f'# rows_nk_kernel<512, LN, from fp32 rows> at {clips} clips: {tiles} tiles ({len(raw)} workgroups), launch {ms:.3f} ms (trace build) = '
      f'{2.0 * M * N * K / ms / 1e9:.0f} TFLOP/s; two workgroups per CU')
print(f'# effective shader clock: {np.median(full[:, 7] / (total * 1e-6)) / 1e9:.3f} GHz')
print('\n'.join(tc.phase_table(us, names, 0, 72)))
nch = N // 64
per_chunk = np.median(dur[:, 2] + dur[:, 3]) / (nch - 1)
print(f'# steady state: {per_chunk:.2f} us per chunk of 64 MFMA slots = {per_chunk / 64 * 1e3:.1f} ns per slot; one v_mfma_f32_32x32x16_bf16 = 32 cycles')
