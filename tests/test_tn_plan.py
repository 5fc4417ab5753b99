"""The weight-gradient launch plan (TnPlan, csrc/mbx_common.h) through the two workspace-size entries, which return the plan's ws_bytes:
host arithmetic, no GPU.  A launcher takes the offsets of its partials from the same plan, so a size that moves here is a kernel that would
write somewhere else.

* mbx_gemm_tn_x3_workspace against the independent restatement of the split rule, localerr.tn_splits;
* both entries against tests/golden/tn_ws_parent.json, recorded by tools/tn_plan_table.py from the library of the commit before the plan
  replaced the five launchers' own derivations."""
import json
import os

import pytest

from tests import localerr as LE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 17, 31, 32, 33, 257, 4131, 4168, 264384)
NKS = (8, 64, 128, 136, 256, 264, 512, 768, 1024, 1280, 1536, 2048)
SWEEP = [(M, N, K) for M in MS for N in NKS for K in NKS]


@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


@pytest.fixture(scope='module')
def parent():
    with open(os.path.join(ROOT, 'tests', 'golden', 'tn_ws_parent.json')) as f:
        return json.load(f)['bytes']


def test_sweep_reaches_every_branch_of_the_plan():
    """What the sweep is there for, stated with the restated rule: clamped and unclamped split counts, a split count of 1, the tile counts
    of the round-6 search (1, 3) and of the whole-round rule (5 -> fallback, 12), every bias-slot case of the 256-tile kernel, ragged
    columns, both tile families."""
    big = [(M, N, K) for M, N, K in SWEEP if N >= 256 and K >= 256]
    small = [s for s in SWEEP if s not in set(big)]
    assert big and small
    assert {-(-N // 256) * -(-K // 256) for _, N, K in big} >= {1, 3, 5, 12}
    assert {-(-K // 256) for _, _, K in big} >= {1, 2, 3, 4, 8}
    assert any(N % 128 or K % 128 for _, N, K in SWEEP)
    for x3 in (False, True):
        for fam, bms in ((big, 32), (small, 64)):
            s = {(LE.tn_splits(M, N, K, x3), (3 if x3 else 1) * -(-M // bms)) for M, N, K in fam}
            assert x3 or any(sp == 1 for sp, _ in s)              # X3 walks at least three chunks: its split count is never 1
            assert any(sp == nch and sp > 1 for sp, nch in s), 'no split count clamped by the chunks'
            assert any(sp < nch for sp, nch in s), 'no unclamped split count'
    assert max(LE.tn_splits(M, N, K) for M, N, K in big) > 128     # the round-6 search goes past the 128 of the other rules


def test_x3_workspace_is_the_restated_split_rule(lib):
    bad = [(M, N, K, int(lib.mbx_gemm_tn_x3_workspace(M, N, K)), LE.tn_splits(M, N, K, True) * (N * K + 4 * N) * 4 + 256) for M, N, K in SWEEP]
    bad = [b for b in bad if b[3] != b[4]]
    assert not bad, f'{len(bad)} of {len(SWEEP)} shapes, first (M, N, K, library, restated): {bad[:5]}'


def test_workspace_sizes_are_the_parent_commits(lib, parent):
    assert sorted(parent) == sorted(f'{M},{N},{K}' for M, N, K in SWEEP)
    bad = []
    for M, N, K in SWEEP:
        got = [int(lib.mbx_gemm_tn_ws(M, N, K)), int(lib.mbx_gemm_tn_x3_workspace(M, N, K))]
        if got != parent[f'{M},{N},{K}']:
            bad.append((M, N, K, got, parent[f'{M},{N},{K}']))
    assert not bad, f'{len(bad)} of {len(SWEEP)} shapes, first (M, N, K, library, parent): {bad[:5]}'
