"""Diagnostics (MBX_DIAG build): per-phase cycle stamps of the leading and the trailing wave of one workgroup of
gemm_nt_pp256.   MBX_LIB=tools/variants/libmbx_diag.so python tools/pp_trace.py [N K]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
buf = torch.zeros(4096, dtype=torch.int64, device='cuda')
os.environ['MBX_TRACE_BUF'] = hex(buf.data_ptr())
from motionbert_amd import hip_ops
from motionbert_amd.engine import EPI_STORE
ops = hip_ops.get()
M, N, K = 64 * 243 * 17, int(sys.argv[1]) if len(sys.argv) > 1 else 1536, int(sys.argv[2]) if len(sys.argv) > 2 else 512
a = torch.randn(M, K, device='cuda').bfloat16(); w = torch.randn(N, K, device='cuda').bfloat16()
out = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
for it in range(3):
    ops.gemm_nt(a, w, None, EPI_STORE, out_t=out)
torch.cuda.synchronize()
t = buf.cpu().tolist()
nk = K // 32
for name, off in (('leading (wave 0)', 0), ('trailing (wave 4)', 2048)):
    u = t[off:off + 2 + 4 * nk]
    print(f'{name}: start {u[0] - t[0]}')
    print(' kt:   R(reads+wait)  barrier1  M(mfma+dma+wait)  barrier2   [cycles]')
    for kt in range(nk):
        b = 1 + 4 * kt
        prev = u[b - 1]
        print(f'{kt:3d}: {u[b]-prev:10d} {u[b+1]-u[b]:10d} {u[b+2]-u[b+1]:12d} {u[b+3]-u[b+2]:12d}')
    print(f' loop total {u[4 * nk] - u[0]} cycles; entry -> loop start {u[0] - t[off + 1000]}; loop end -> epilogue issued {t[off + 1001] - u[4 * nk]}; '
          f'stores drained after {t[off + 1002] - t[off + 1001]} more; whole tile {t[off + 1002] - t[off + 1000]} cycles')
