"""Build diagnostic / A-B variants of the kernel library next to the product one.

    python tools/build_variants.py diag                      # -DMBX_DIAG: the MBX_DBG / MBX_NTP_LDS_PAD environment switches are live
    python tools/build_variants.py name -DFOO=1 -DBAR=2      # any extra compile flags

The diagnostic flags (csrc/mbx_diag.h): -DMBX_DIAG (with -DMBX_TRACE: the cycle stamps of nt_trace.py), -DMBX_TN_TRACE, -DMBX_ROWS_TRACE,
-DMBX_RN_TRACE, -DMBX_MLP_TRACE (=2: five more stamps), -DMBX_ATTN_TRACE, and the ablation bits -DMBX_{ROWS,RN,MLP,ATTN}_DBG=bits.  A build
with any of the first seven exports mbx_diag_set_trace(buf, bytes): tools/trace_common.py arms it with a sized stamp buffer, and a traced
launch stamps only if the buffer holds what its grid writes.  No build reads a buffer address from the environment.

Output: tools/variants/libmbx_<name>.so (git-ignored).  The measurement scripts pick a variant with
MBX_LIB=tools/variants/libmbx_<name>.so; the product library (motionbert_amd/libmbx.so) has no switches."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motionbert_amd import build as B


def main():
    name, extra = sys.argv[1], sys.argv[2:]
    if name == 'diag' and '-DMBX_DIAG' not in extra:
        extra = ['-DMBX_DIAG'] + extra
    out = os.path.join(ROOT, 'tools', 'variants')
    obj = os.path.join(out, '_obj_' + name)
    os.makedirs(obj, exist_ok=True)
    hipcc = B._hipcc()

    def cc(src):
        o = os.path.join(obj, src.replace('.hip', '.o'))
        subprocess.run([hipcc] + B.FLAGS + extra + ['-c', os.path.join(B.CSRC, src), '-o', o], check=True)
        return o
    with ThreadPoolExecutor(max_workers=len(B.SOURCES)) as ex:
        objs = list(ex.map(cc, B.SOURCES))
    lib = os.path.join(out, f'libmbx_{name}.so')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib] + objs, check=True)
    print(lib)


if __name__ == '__main__':
    main()
