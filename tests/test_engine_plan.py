"""Invariants of the engine's sequencing plan (engine.plan_pass: a pure function, no tensors, no provider): what forward saves, what
backward runs and what the packer prepares cannot disagree, over the configurations of the trace matrix (tools/engine_trace.py), the
full and the Lite model, and row counts on both sides of both row limits."""
import itertools

import pytest

from motionbert_amd import engine
from motionbert_amd.engine import LINEARS, ORDER, STREAMS, Caps, ModelCfg, plan_pass


def _cfg(C, hidden, depth, att_fuse=True):
    return ModelCfg(dim_in=3, dim_out=3, C=C, R=C, depth=depth, H=8, hidden=hidden, J=17, maxlen=243, eps=1e-6, scale=(C // 8) ** -0.5,
                    att_fuse=att_fuse, qkv_bias=True)


CFGS = {'tiny': _cfg(64, 128, 2), 'tiny-average': _cfg(64, 128, 2, att_fuse=False), 'full': _cfg(512, 1024, 5), 'lite': _cfg(256, 512, 5)}
ALL_ON = dict(fold=True, gelu_d=True, grad_stream=True, rows_lnbwd=True, rows_resid_ln=True, block_grad_t=True, proj_mlp=True, fuse_ln=True)


def _caps():
    """Everything on, each switch off alone (as the engine derives them: no row-owner backward, no operand-typed Block boundary and no
    saved derivative without rows_lnbwd), recompute, and the plain sequencings (fp32 and dropout: no fold; bf16x3)."""
    yield 'all', Caps(**ALL_ON)
    for off in ('fold', 'gelu_d', 'grad_stream', 'rows_resid_ln', 'block_grad_t', 'proj_mlp', 'fuse_ln'):
        yield off + '=0', Caps(**dict(ALL_ON, **{off: False}))
    yield 'rows_lnbwd=0', Caps(**dict(ALL_ON, rows_lnbwd=False, block_grad_t=False, gelu_d=False))
    yield 'recompute', Caps(**dict(ALL_ON, recompute=True))
    yield 'fp32', Caps(**dict(ALL_ON, fold=False))      # (training with dropout comes to the same: Engine.__init__ grants no `fold`)
    yield 'bf16x3', Caps(**dict(ALL_ON, fold=False, x3=True))


def _row_counts(cfg):
    """One clip, and the last row count inside / the first beyond each of the two row limits."""
    lnbwd = (engine.ROW_OFFSET_LIMIT - 1) // (2 * max(3 * cfg.C, cfg.hidden))
    resid = (engine.ROW_OFFSET_LIMIT - 1) // max(4 * cfg.C, 2 * max(cfg.C, cfg.hidden))
    return (9 * 17, lnbwd, lnbwd + 1, resid, resid + 1)


def _subs(cfg):      # (block prefix, level, sub, typ, module) in execution order
    return [(pre, i, sub, typ, mod) for pre, i, sub, typ, _, mod, _ in engine.sublayers(cfg)]


@pytest.mark.parametrize('cfg_name', list(CFGS))
def test_plan_invariants(cfg_name):
    cfg = CFGS[cfg_name]
    for (cname, caps), M, need_grad, rawln in itertools.product(_caps(), _row_counts(cfg), (True, False), (True, False)):
        if rawln and need_grad:
            continue      # the no-grad sequencing is never asked for with a backward
        plan = plan_pass(cfg, caps, M, need_grad, rawln)
        tag = (cfg_name, cname, M, need_grad, rawln)
        assert set(plan.sub) == {(pre, sub) for pre, _, sub, _, _ in _subs(cfg)}, tag
        lin_in = {(pre, sub): f'{pre}.{mod}.{LINEARS[typ][0]}' for pre, _, sub, typ, mod in _subs(cfg)}
        lin_out = {(pre, sub): f'{pre}.{mod}.{LINEARS[typ][1]}' for pre, _, sub, typ, mod in _subs(cfg)}
        # every sub-layer that saves the derivative has the row-owner tail, and not the conditional one of a Block's first sub-layer
        for key, sp in plan.sub.items():
            assert sp.save != 'd' or (sp.tail == 'rows' and key[1] > 0), (tag, key)
            assert (sp.save is None) == (not need_grad or lin_in[key].endswith('.qkv')), (tag, key)
            assert (sp.tail is None) == (not need_grad), (tag, key)
        # the pack lists are exactly the row-owner entries
        assert sorted(plan.pack_n) == sorted(lin_in[k] for k, sp in plan.sub.items() if sp.tail == 'rows'), tag
        assert sorted(plan.pack_f) == sorted(lin_out[k] for k, sp in plan.sub.items() if sp.lin_out == 'rows'), tag
        assert all(k[1] < 3 for k, sp in plan.sub.items() if sp.lin_out == 'rows'), tag      # the fourth sub-layer feeds no LayerNorm
        # a level hands its gradients down operand-typed only if both Blocks' first sub-layers are eligible for the row-owner tail
        assert len(plan.out_t) == cfg.depth, tag
        for i, out_t in enumerate(plan.out_t):
            assert out_t == all(plan.sub[f'{st}.{i}', 0].tail == 'rows' for st, _ in STREAMS), (tag, i)
            assert not out_t or (plan.gstream and cfg.att_fuse), (tag, i)
        # a deferred proj is followed by an MLP packed with that proj in front, and nothing else has one in front
        packed = {name: front for what, name, front in plan.pack_k if what == 'mlp'}
        for (stream, kind), i in itertools.product(STREAMS, range(cfg.depth)):
            pre = f'{stream}.{i}'
            for sub, (typ, _, mod, _) in enumerate(ORDER[kind]):
                sp = plan.sub[pre, sub]
                if sp.lin_out == 'deferred':
                    nxt = ORDER[kind][sub + 1]
                    assert nxt[0] == 'mlp' and plan.sub[pre, sub + 1].lin_out == 'fused', (tag, pre, sub)
                    assert plan.sub[pre, sub + 1].front == packed[f'{pre}.{nxt[2]}'] == f'{pre}.{mod}.proj', (tag, pre, sub)
                elif sp.lin_out == 'fused':
                    assert packed[f'{pre}.{mod}'] == sp.front, (tag, pre, sub)
                    assert sp.front is None or plan.sub[pre, sub - 1].lin_out == 'deferred', (tag, pre, sub)
                else:
                    assert sp.front is None and f'{pre}.{mod}' not in packed, (tag, pre, sub)
        raw = {sp.lin_in for sp in plan.sub.values()}
        assert raw == ({'raw'} if rawln and plan.fold else {'ln'}), tag
        assert (len(plan.pack_k) == 8 * cfg.depth) == (raw == {'raw'}) and (not plan.pack_k) == (raw == {'ln'}), tag
        # the plain sequencing has no folded or row-owner entry anywhere
        if not plan.fold:
            assert not caps.fold, tag
            assert not (plan.gstream or plan.embed_norm or any(plan.out_t) or plan.pack_f or plan.pack_n or plan.pack_k), tag
            assert all(sp == ('ln', 'tile', None, sp.save, 'plain' if need_grad else None) and sp.save != 'd' for sp in plan.sub.values()), tag
            assert set(plan.fuse_norm) <= {None, 'pair', 'norm'}, tag
        else:
            assert set(plan.fuse_norm) <= {None, 'xhat', 'norm'}, tag
        assert plan.fuse_norm[-1] == ('norm' if cfg.att_fuse and caps.fuse_ln else None), tag


def test_the_row_limits_move_the_plan_and_nothing_else():
    """Beyond a row limit the plan is the one of the A/B switch at 0."""
    for cfg in (CFGS['full'], CFGS['lite']):
        caps = Caps(**ALL_ON)
        _, lnbwd, lnbwd1, resid, resid1 = _row_counts(cfg)
        assert lnbwd < resid
        off = Caps(**dict(ALL_ON, rows_lnbwd=False, block_grad_t=False, gelu_d=False))
        assert plan_pass(cfg, caps, lnbwd1, True, False) == plan_pass(cfg, off, lnbwd1, True, False) != plan_pass(cfg, caps, lnbwd, True, False)
        off2 = Caps(**dict(ALL_ON, rows_lnbwd=False, block_grad_t=False, gelu_d=False, rows_resid_ln=False))
        assert plan_pass(cfg, caps, resid1, True, False) == plan_pass(cfg, off2, resid1, True, False) != plan_pass(cfg, caps, resid, True, False)
