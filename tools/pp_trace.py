"""Diagnostics (MBX_DIAG build): per-phase cycle stamps of the leading and the trailing wave of one workgroup (number 3000) of
gemm_nt_pp256.
    python tools/build_variants.py diag
    MBX_LIB=tools/variants/libmbx_diag.so python tools/pp_trace.py [N K]"""
import sys
import torch
import trace_common as tc      # (puts the repository root on sys.path)
from motionbert_amd import hip_ops
from motionbert_amd.engine import EPI_STORE
ops = hip_ops.get()
GROUP, EDGE = 2048, 1000      # PP_TRACE_GROUP, PP_TRACE_EDGE (gemm_pipe.hip): the trailing group's record; entry / epilogue issued / acknowledged
M, N, K = 64 * 243 * 17, int(sys.argv[1]) if len(sys.argv) > 1 else 1536, int(sys.argv[2]) if len(sys.argv) > 2 else 512
a = torch.randn(M, K, device='cuda').bfloat16(); w = torch.randn(N, K, device='cuda').bfloat16()
out = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
nk = K // 32
buf = tc.arm(ops, GROUP + max(4 * nk + 1, EDGE + 3))
tc.timed_launch(lambda: ops.gemm_nt(a, w, None, EPI_STORE, out_t=out), buf, warm=2)
tc.check_need(ops, buf, GROUP + max(4 * nk + 1, EDGE + 3))
t = buf.cpu().tolist()
for name, off in (('leading (wave 0)', 0), ('trailing (wave 4)', GROUP)):
    u = t[off:off + 2 + 4 * nk]
    print(f'{name}: start {u[0] - t[0]}')
    print(' kt:   R(reads+wait)  barrier1  M(mfma+dma+wait)  barrier2   [cycles]')
    for kt in range(nk):
        b = 1 + 4 * kt
        prev = u[b - 1]
        print(f'{kt:3d}: {u[b]-prev:10d} {u[b+1]-u[b]:10d} {u[b+2]-u[b+1]:12d} {u[b+3]-u[b+2]:12d}')
    print(f' loop total {u[4 * nk] - u[0]} cycles; entry -> loop start {u[0] - t[off + EDGE]}; loop end -> epilogue issued {t[off + EDGE + 1] - u[4 * nk]}; '
          f'stores drained after {t[off + EDGE + 2] - t[off + EDGE + 1]} more; whole tile {t[off + EDGE + 2] - t[off + EDGE]} cycles')
