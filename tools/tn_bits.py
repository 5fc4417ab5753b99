"""SHA-256 digests of what the weight-gradient GEMMs (bf16, fp32, bf16x3; with and without db) and every A.W^T epilogue of every launcher write
for fixed inputs (generated on the CPU from a fixed seed).  Two libraries whose listings are equal compute the same bits: run it once per
library and diff -- the way a host-side change of the launchers (split plan, epilogue dispatch) is pinned.

    MBX_LIB=<library> python tools/tn_bits.py [out.txt]"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motionbert_amd import hip_ops
from motionbert_amd.engine import EPI_DGELU, EPI_GELU, EPI_RESID, EPI_STORE, EPI_TANH

DEV, BF = 'cuda', torch.bfloat16
M_STEP = 64 * 243 * 17
TN_SHAPES = [(17, 256, 256), (4131, 1280, 256), (4131, 512, 2048), (33, 128, 512), (17, 128, 128), (64, 128, 128),
             (M_STEP, 1536, 512), (M_STEP, 512, 2048), (M_STEP, 768, 256)]
NT_SHAPES = [(4131, 512, 512), (4131, 128, 512)]
LINES = []


def sha(t):
    torch.cuda.synchronize()
    t = t.contiguous()
    return hashlib.sha256(t.view(torch.int16 if t.dtype == BF else torch.int32).cpu().numpy().tobytes()).hexdigest()


def say(name, *tensors):
    LINES.append(f'{name:44s} ' + ' '.join(sha(t) for t in tensors))
    print(LINES[-1], flush=True)


def rnd(gen, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV).to(dtype)


def fresh(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), device=DEV, dtype=dtype)


def tn(ops, M, N, K):
    gen = torch.Generator().manual_seed(1000 + N + K)
    dy32, a32 = rnd(gen, M, N), rnd(gen, M, K)
    for tag, dy, a in (('bf16', dy32.to(BF), a32.to(BF)), ('f32', dy32, a32), ('x3', ops.split(dy32), ops.split(a32))):
        dw, db, dw2 = fresh(N, K), fresh(N), fresh(N, K)
        ops.gemm_tn(dy, a, dw, db)
        ops.gemm_tn(dy, a, dw2, None)
        say(f'gemm_tn.{tag}.{M}x{N}x{K} dw db dw_nodb', dw, db, dw2)


def nt(ops, M, N, K):
    gen = torch.Generator().manual_seed(2000 + N + K)
    a32, w32, bias = rnd(gen, M, K), rnd(gen, N, K, scale=0.05), rnd(gen, N)
    resid, aux32 = rnd(gen, M, N), rnd(gen, M, N)
    for tag, a, w, aux, T in (('bf16', a32.to(BF), w32.to(BF), aux32.to(BF), BF), ('f32', a32, w32, aux32, torch.float32),
                              ('x3', ops.split(a32), ops.split(w32), aux32, torch.float32)):
        u, g, r, t, d = fresh(M, N, dtype=T), fresh(M, N, dtype=T), fresh(M, N), fresh(M, N), fresh(M, N, dtype=T)
        ops.gemm_nt(a, w, bias, EPI_STORE, out_t=u)
        say(f'gemm_nt.{tag}.store.{M}x{N}x{K}', u)
        u.fill_(float('nan'))
        ops.gemm_nt(a, w, bias, EPI_GELU, out_t=u, out2_t=g)
        say(f'gemm_nt.{tag}.gelu.{M}x{N}x{K} u g', u, g)
        ops.gemm_nt(a, w, bias, EPI_RESID, out_f=r, resid=resid)
        say(f'gemm_nt.{tag}.resid.{M}x{N}x{K}', r)
        ops.gemm_nt(a, w, bias, EPI_TANH, out_f=t)
        say(f'gemm_nt.{tag}.tanh.{M}x{N}x{K}', t)
        ops.gemm_nt(a, w, None, EPI_DGELU, out_t=d, aux_t=aux)
        say(f'gemm_nt.{tag}.dgelu.{M}x{N}x{K}', d)
    a, w, aux = a32.to(BF), w32.to(BF), aux32.to(BF)
    if N >= 256:                               # the entries that only the 256 x 256 kernel serves
        od, og, om = fresh(M, N, dtype=BF), fresh(M, N, dtype=BF), fresh(M, N, dtype=BF)
        ops.gemm_nt_gelu_d(a, w, bias, od, og)
        say(f'gemm_nt_gelu_d.{M}x{N}x{K} d g', od, og)
        ops.gemm_nt_mul(a, w, aux, om)
        say(f'gemm_nt_mul.{M}x{N}x{K}', om)
        ds, part = fresh(M, N, dtype=BF), fresh(N // 64, M, 2)
        ops.gemm_nt_dgelu_stats(a, w, ds, aux, bias, rnd(gen, N), part)
        say(f'gemm_nt_dgelu_stats.{M}x{N}x{K} du part', ds, part)
    rowc, extra = rnd(gen, M, 4), rnd(gen, M, N)
    for tag, dres in (('lnbwd', resid), ('lnbwd_t', resid.to(BF))):
        dx, dx_t = fresh(M, N), fresh(M, N, dtype=BF)
        ops.gemm_nt_lnbwd(a, w, aux, rowc, dres, extra, dx, dx_t)
        say(f'gemm_nt_{tag}.{M}x{N}x{K} dx dx_t', dx, dx_t)


def main():
    ops = hip_ops.get()
    print(f'# library: {os.path.basename(hip_ops.LIB_PATH)}', flush=True)
    for shape in TN_SHAPES:
        tn(ops, *shape)
    for shape in NT_SHAPES:
        nt(ops, *shape)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
