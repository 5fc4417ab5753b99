"""Diagnostics (MBX_DIAG + MBX_TRACE build): per-k-tile cycle stamps of one wave of one workgroup (number 4000) of gemm_nt_pipe, the 256 x 128
kernel.  It runs the resid and lnbwd epilogues, and store only for N < 256 (wider ones run gemm_nt_pp256: tools/pp_trace.py).
    python tools/build_variants.py diagtrace -DMBX_DIAG -DMBX_TRACE
    MBX_LIB=tools/variants/libmbx_diagtrace.so python tools/nt_trace.py [N K [store|resid|lnbwd]]"""
import sys
import torch
import trace_common as tc      # (puts the repository root on sys.path)
from motionbert_amd import hip_ops
from motionbert_amd.engine import EPI_STORE, EPI_RESID
ops = hip_ops.get()
M, N, K = 64 * 243 * 17, int(sys.argv[1]) if len(sys.argv) > 1 else 1536, int(sys.argv[2]) if len(sys.argv) > 2 else 512
mode = sys.argv[3] if len(sys.argv) > 3 else 'store'      # store | resid | lnbwd (the 256x128 kernel's epilogues)
a = torch.randn(M, K, device='cuda').bfloat16(); w = torch.randn(N, K, device='cuda').bfloat16()
out = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
outf, resid = torch.empty(M, N, device='cuda'), torch.randn(M, N, device='cuda')
rowc = torch.rand(M, 4, device='cuda')
nk = K // 32
buf = tc.arm(ops, 3 + 4 * nk)      # ntp_trace_slots (gemm_pipe.hip): entry, four per k-tile, epilogue issued / acknowledged
dx_t = torch.empty_like(out)
fn = {'resid': lambda: ops.gemm_nt(a, w, None, EPI_RESID, out_f=outf, resid=resid),
      'lnbwd': lambda: ops.gemm_nt_lnbwd(a, w, out, rowc, resid, None, outf, dx_t),
      'store': lambda: ops.gemm_nt(a, w, None, EPI_STORE, out_t=out)}[mode]
tc.timed_launch(fn, buf, warm=2)
tc.check_need(ops, buf, 3 + 4 * nk)
t = buf.cpu().tolist()
t0 = t[0]
print(f'N={N} K={K} {mode}'); print('k-tile: wait(vmcnt)  barrier  issue  compute   [cycles]')
for kt in range(nk):
    b = 1 + kt * 4
    prev = t[b - 1] if kt else t0
    print(f'{kt:3d}: {t[b]-prev:8d} {t[b+1]-t[b]:8d} {t[b+2]-t[b+1]:6d} {t[b+3]-t[b+2]:8d}')
e = 1 + nk * 4
print(f'epilogue issue {t[e]-t[e-1]} cycles, store drain {t[e+1]-t[e]} cycles, total tile {t[e+1]-t0} cycles')
