"""Record the weight-gradient workspace sizes of a library over the sweep of tests/test_tn_plan.py (no GPU needed: the size functions are
host arithmetic).  The table in tests/golden/tn_ws_parent.json was recorded from the library of the commit BEFORE the launch plan
(TnPlan, csrc/mbx_common.h) replaced the launchers' own derivations; the test holds every later library to it.

    MBX_LIB=<library to record> python tools/tn_plan_table.py [out.json [what the library was built from, e.g. a commit hash]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = (1, 17, 31, 32, 33, 257, 4131, 4168, 264384)
NKS = (8, 64, 128, 136, 256, 264, 512, 768, 1024, 1280, 1536, 2048)


def table(lib):
    """{'M,N,K': [mbx_gemm_tn_ws, mbx_gemm_tn_x3_workspace]} over the sweep"""
    return {f'{M},{N},{K}': [int(lib.mbx_gemm_tn_ws(M, N, K)), int(lib.mbx_gemm_tn_x3_workspace(M, N, K))]
            for M in MS for N in NKS for K in NKS}


def main():
    from motionbert_amd import hip_ops
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'tn_ws_parent.json')
    t = table(hip_ops.load_library())
    with open(out, 'w') as f:
        json.dump({'recorded_from': sys.argv[2] if len(sys.argv) > 2 else os.path.basename(hip_ops.LIB_PATH), 'columns': ['mbx_gemm_tn_ws', 'mbx_gemm_tn_x3_workspace'], 'bytes': t}, f,
                  separators=(',', ':'))
        f.write('\n')
    print(f'{out}: {len(t)} shapes from {hip_ops.LIB_PATH}')


if __name__ == '__main__':
    main()
