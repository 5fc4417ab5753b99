"""Diagnostics (-DMBX_ATTN_TRACE build): where a problem of the temporal attention backward (attn_bwd_fused_kernel: one (clip, joint, head)
sequence of 243 frames per workgroup of sixteen waves) spends its time in situ -- eight time stamps per workgroup, all of one launch.
    python tools/build_variants.py attntrace -DMBX_ATTN_TRACE
    MBX_LIB=tools/variants/libmbx_attntrace.so python tools/attn_trace.py [clips]"""
import sys

import numpy as np
import torch

import trace_common as tc            # (first: it puts the repository root on sys.path)
from motionbert_amd import hip_ops
from motionbert_amd.engine import MODE_TEMPORAL
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T, J, H, hd, dev = 243, 17, 8, 64, 'cuda'
C, M, nprob = H * hd, B * T * J, B * J * H
ops = hip_ops.get()
SLOTS, WAVES = 9, 16                 # ATTN_TRACE_SLOTS, ATTN_TRACE_WAVES (attention.hip): eight stamps + hardware id per problem; one stamp per wave
buf = tc.arm(ops, (SLOTS + WAVES) * nprob)
g = torch.Generator(device=dev).manual_seed(0)
qkv = torch.randn(M, 3 * C, device=dev, generator=g).to(torch.bfloat16)
d_o = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16)
o, lse = torch.empty(M, C, device=dev, dtype=torch.bfloat16), torch.empty(M, H, device=dev)
dqkv = torch.empty_like(qkv)
ops.attn_fwd(qkv, o, lse, B, T, J, H, hd ** -0.5, MODE_TEMPORAL)
fn = lambda: ops.attn_bwd(qkv, o, d_o, lse, dqkv, B, T, J, H, hd ** -0.5, MODE_TEMPORAL)
ms = tc.timed_launch(fn, buf)
tc.check_need(ops, buf, (SLOTS + WAVES) * nprob)
raw = tc.records(buf, nprob, SLOTS)
us = tc.to_us(raw[:, :8])
CUT = 512                            # not the first and not the last two rounds
names = ['fill: loads issued, landed, written to the LDS tiles', 'statistics + first barrier', 'compute (dQ | dK, dV)', 'second barrier (slowest wave)',
         'gradients staged over the tiles + third barrier', 'copy-out: LDS reads + stores issued', 'stores acknowledged']
print(f'# attn_bwd_fused_kernel<64> at {B} clips: {nprob} problems, launch {ms:.3f} ms (trace build); steady-state problems: {len(tc.steady(us, CUT))}')
print('\n'.join(tc.phase_table(us, names, CUT, 58, whole='whole problem', num_width=7)))
t = buf.cpu().numpy()
ok = t[:SLOTS * nprob].reshape(-1, SLOTS)[:, 0] > 0
pw = t[SLOTS * nprob:(SLOTS + WAVES) * nprob].reshape(-1, WAVES).astype(np.float64)
rel = (pw[ok] - raw[:, 2].astype(np.float64)[:, None]) / tc.TICKS_PER_US
print('# end of the compute phase per wave, us after the first barrier (median over all problems): ' + ' '.join(f'{np.median(rel[:, w]):.1f}' for w in range(16)))
print(f'# launch / (problems / 256 CUs) = {ms * 1e3 / (nprob / 256):.2f} us per problem and CU')
