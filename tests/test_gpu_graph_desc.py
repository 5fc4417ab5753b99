"""A captured hipGraph and the weight-descriptor cache of the kernel provider (hip_ops.HipOps._desc_cache).

The packers (prep_weights, fold_norm_weights, rows_n_pack_many) keep small device tables per set of weight addresses.  A graph
under capture bakes the ADDRESSES of those tables into its copy nodes and reads them at every replay; the cache drops all entries
of a kind when the 16th arrives (_desc_room), which any other model's forward can cause.  The entries a capture used must outlive
that: HipOps._desc_held.  Found when a longer GPU suite moved the 16th entry between the capture and the second replay of
test_gpu_train.test_graphed_train_step_matches_eager_steps."""
import pytest
import torch

from tests.helpers import build_model, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CFG = dict(dim_in=3, dim_out=3, dim_feat=256, dim_rep=512, depth=1, num_heads=8, mlp_ratio=4, num_joints=17, maxlen=243)


def test_captured_train_step_survives_descriptor_eviction():
    from motionbert_amd import hip_ops
    from motionbert_amd.train import FlatAdamW, GraphedTrainStep, pose_loss
    ops = hip_ops.get()
    a, b = build_model(CFG, seed=1).to(DEV), build_model(CFG, seed=1).to(DEV)
    oa, ob = FlatAdamW(a, lr=2e-4, weight_decay=0.01), FlatAdamW(b, lr=2e-4, weight_decay=0.01)
    batches = [(make_input(2, 27, 17, 30 + i).to(DEV), (torch.randn(2, 27, 17, 3, generator=torch.Generator().manual_seed(40 + i)) * 0.3).to(DEV))
               for i in range(2)]
    before = set(ops._desc_held)
    step = GraphedTrainStep(a, oa, *batches[0])
    held = [e for k, e in ops._desc_held.items() if k not in before]
    assert held, 'the capture read descriptor tables: their entries must be held'
    assert all(any(e is c for c in ops._desc_cache.values()) for e in held)
    tables = [(e['desc'], e['desc'].clone()) for e in held]
    # what the 16th entry of a kind does, for every kind; then allocations that would take over freed tables
    for kind in ('prep', 'fold', 'rnpack'):
        ops._desc_room(kind, keep=0)
    assert not ops._desc_cache
    junk = [torch.full((n,), -1, dtype=torch.int64, device=DEV) for n in (8, 16, 32, 64, 128) for _ in range(16)]
    torch.cuda.synchronize()
    assert all(torch.equal(t, c) for t, c in tables), 'a table the graph reads was overwritten'
    for x, gt in batches:
        la = step(x, gt)
        ob.zero_grad(set_to_none=True)
        total, lb = pose_loss(b(x), gt)
        total.backward()
        ob.step()
        assert torch.allclose(la, lb, rtol=1e-6, atol=0), (la, lb)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters())), 'graph replay and eager steps must be bit-identical'
    del junk
