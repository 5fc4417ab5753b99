"""Record what motionbert_amd/engine.py asks of its kernel provider, call by call, over every sequencing it has (no GPU needed: the
provider is the torch restatement oracle.torch_ops.MockOps behind a forwarding proxy).  tests/golden/engine_trace.json was recorded at
the commit BEFORE the sub-layer helpers of engine.py replaced the per-sub-layer copies; tests/test_engine_trace.py holds every later
engine to it: the same `ops` calls in the same order on the same tensors.

A call is recorded as its method name and its arguments bound to the provider's signature (defaults filled in, so an omitted `drop` and
`drop=None` are one thing): a tensor as (buffer number, shape, dtype), a tuple or list element by element, a dict as its sorted keys, a
scalar as its value.  A buffer is storage address + offset + shape, numbered by first appearance; every tensor seen is held until the
case ends so that no address comes back.  Aliasing (`dropout(g, g)`, views of the returned tensor) and swapped arguments therefore show.

The device provider (`hip_ops.get()`, an MI355X) has a case list of its own, `gpu_cases()`, for what the mock cannot reach: the second
stream, ragged batches and flip TTA.  There every call records one more field, `stream`: 0 when it was issued on the stream that was
current when the case began (the pass's launch stream), 1 on any other.  tests/golden/engine_trace_gpu.json was recorded at the commit
BEFORE the engine's decisions moved into one plan per pass; tests/test_gpu_engine_trace.py compares against it.

    python tools/engine_trace.py --record [out.json [what it was recorded from, e.g. a commit hash]]
    python tools/engine_trace.py --record-gpu [out.json [what it was recorded from]]
    python tools/engine_trace.py --bits       one SHA-256 per case over output, input gradient and parameter gradients (host-dependent)"""
import functools
import hashlib
import inspect
import json
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SWITCH_VARS = ('MBX_X3_PLANES', 'MBX_DUAL_STREAM', 'MBX_FOLD_LN', 'MBX_GRAD_STREAM', 'MBX_ROWS_LNBWD', 'MBX_ROWS_RESID_LN',
               'MBX_BLOCK_GRAD_T', 'MBX_GELU_D', 'MBX_RAWLN', 'MBX_PROJ_MLP')
DROP_SEED = 20240607


@functools.lru_cache(maxsize=None)
def _signature(cls, name):
    """Signature of provider method `name` as a caller sees it (no `self`)."""
    raw, sig = inspect.getattr_static(cls, name), inspect.signature(getattr(cls, name))
    if isinstance(raw, (staticmethod, classmethod)):
        return sig
    return sig.replace(parameters=list(sig.parameters.values())[1:])


class Recorder:
    """Forwards everything to `ops`; every method call leaves one record in `calls`."""

    def __init__(self, ops, launch_stream=None):
        self.__dict__.update(_ops=ops, calls=[], _held=[], _bufs={}, _launch=launch_stream)

    def __getattr__(self, name):
        attr = getattr(self._ops, name)      # AttributeError where the provider has no such kernel: hasattr() probes see the provider
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            bound = _signature(type(self._ops), name).bind(*args, **kwargs)
            bound.apply_defaults()
            self.calls.append([name] + [[k, self._describe(v)] for k, v in bound.arguments.items()])
            if self._launch is not None:      # device cases: issued on the pass's launch stream (0) or on another one (1)
                self.calls[-1].append(['stream', int(torch.cuda.current_stream() != self._launch)])
            return attr(*args, **kwargs)
        return call

    def __setattr__(self, name, value):
        setattr(self._ops, name, value)

    def _describe(self, v):
        if isinstance(v, torch.Tensor):
            self._held.append(v)
            key = (v.untyped_storage().data_ptr(), v.storage_offset(), tuple(v.shape))
            return ['T', self._bufs.setdefault(key, len(self._bufs)), list(v.shape), str(v.dtype)]
        if isinstance(v, (tuple, list)):
            return [self._describe(e) for e in v]
        if isinstance(v, dict):
            return ['D'] + sorted(str(k) for k in v)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return str(v)


def call_digest(call) -> str:
    return hashlib.sha256(json.dumps(call, separators=(',', ':')).encode()).hexdigest()


def cases():
    """[(name, spec)]: the fixed matrix.  spec: fixture, precision, fold, recompute, grad, drop, off (one MBX_* switch at 0), att_fuse,
    out ('pose', 'rep' or 'pool')."""
    base = dict(fixture='tiny_trained', precision='bf16', fold=True, recompute=False, grad=True, drop=False, off=None, att_fuse=True, out='pose')
    out = []

    def add(**kw):
        spec = dict(base, **kw)
        name = '-'.join([spec['fixture'], spec['precision'], 'fold' if spec['fold'] else 'plain'] + (['recompute'] if spec['recompute'] else []) +
                        ['grad' if spec['grad'] else 'nograd'] + (['drop'] if spec['drop'] else []) + ([spec['off'] + '=0'] if spec['off'] else []) +
                        ([] if spec['att_fuse'] else ['average']) + ([] if spec['out'] == 'pose' else [spec['out']]))
        out.append((name, spec))
    for precision in ('fp32', 'bf16', 'bf16x3'):
        for fold in (True, False):
            for recompute in (False, True):
                add(precision=precision, fold=fold, recompute=recompute)
                add(precision=precision, fold=fold, recompute=recompute, drop=True)
            add(precision=precision, fold=fold, grad=False)      # (without a backward there is nothing to rebuild)
        # the other fixture: other weights, the same sequencing
        add(fixture='tiny_default', precision=precision)
        add(fixture='tiny_default', precision=precision, grad=False)
    for off in SWITCH_VARS:
        for precision in ('bf16', 'bf16x3'):
            add(precision=precision, off=off)
            add(precision=precision, off=off, grad=False)
    for precision in ('bf16', 'bf16x3'):
        add(precision=precision, att_fuse=False)
        add(precision=precision, att_fuse=False, grad=False)
        add(precision=precision, out='rep')
        add(precision=precision, out='rep', grad=False)
        add(precision=precision, out='pool')
        add(precision=precision, out='pool', drop=True)
    return out


_fixtures = {}


def _fixture(name):
    if name not in _fixtures:
        z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
        _fixtures[name] = ({k: z[k] for k in z.files}, {k[4:]: z[k].item() for k in z.files if k.startswith('cfg.')})
    return _fixtures[name]


@functools.lru_cache(maxsize=None)
def _model(fixture, att_fuse, drop):
    """The fixture's arrays and a model that holds its weights (dropout on: every rate 0.1), shared by the cases."""
    import torch.nn as nn
    from motionbert_amd import DSTformer
    z, cfg = _fixture(fixture)
    cfg = dict(cfg, att_fuse=att_fuse)
    if drop:
        cfg.update(drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1)
    model = DSTformer(norm_layer=partial(nn.LayerNorm, eps=1e-6), **cfg)
    model.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('w.') and (att_fuse or 'ts_attn' not in k)},
                          strict=True)
    return z, model


def run_case(spec, bits=False):
    """The recorded calls of one case (and, `bits`, the SHA-256 over the bytes of output, input gradient and parameter gradients)."""
    from motionbert_amd import engine, model as M
    from oracle.torch_ops import MockOps
    z, model = _model(spec['fixture'], spec['att_fuse'], spec['drop'])
    model.precision, model.fold_ln, model.recompute = spec['precision'], spec['fold'], spec['recompute']
    model.train()
    model._drop_seed = DROP_SEED
    for p in model.parameters():
        p.grad = None
    env = {spec['off']: '0'} if spec['off'] else {}
    engine.reload_switches(env)
    try:
        ops = Recorder(MockOps())
        x = torch.from_numpy(z['x']).clone().requires_grad_(spec['grad'])
        # (pooling: the dropout of the action heads sits on the representation, with its own seed)
        what = {'pose': False, 'rep': True, 'pool': ('pool', 1, 0.1 if spec['drop'] else 0.0, DROP_SEED + 1)}[spec['out']]
        with torch.set_grad_enabled(spec['grad']):
            out = M.run(ops, model, x, what)
        if spec['grad']:
            cot = {'pose': 'cot', 'rep': 'cot_rep'}.get(spec['out'])
            (out * torch.from_numpy(z[cot])).sum().backward() if cot else out.sum().backward()
    finally:
        engine.reload_switches()
    digest = None
    if bits:
        h = hashlib.sha256(out.detach().numpy().tobytes())
        if spec['grad']:
            h.update(x.grad.numpy().tobytes())
            for n, p in model.named_parameters():
                h.update(n.encode() + (b'-' if p.grad is None else p.grad.numpy().tobytes()))
        digest = h.hexdigest()
    return ops.calls, digest


GPU_CFG = dict(dim_in=3, dim_out=3, dim_feat=256, dim_rep=256, depth=2, num_heads=8, mlp_ratio=2, num_joints=17, maxlen=16)
GPU_B, GPU_T, GPU_CLIPS = 2, 9, (9, 5)


def gpu_cases():
    """[(name, spec)] for the device provider, at the smallest shape at which every capability of HipOps holds (dim_feat 256, head
    dim 32, hidden 512; 2 clips of 9 frames).  spec: precision, grad, off (one MBX_* switch at 0), ragged (two clips of 9 and 5 frames
    in one forward, with flip TTA)."""
    base = dict(precision='bf16', grad=True, off=None, ragged=False)
    return [('bf16-grad', base), ('bf16-grad-MBX_BLOCK_GRAD_T=0', dict(base, off='MBX_BLOCK_GRAD_T')),
            ('bf16-grad-MBX_DUAL_STREAM=0', dict(base, off='MBX_DUAL_STREAM')), ('bf16-nograd', dict(base, grad=False)),
            ('bf16-nograd-ragged-tta', dict(base, grad=False, ragged=True)), ('bf16x3-grad', dict(base, precision='bf16x3'))]


@functools.lru_cache(maxsize=None)
def _gpu_model():
    import torch.nn as nn
    from motionbert_amd import DSTformer
    torch.manual_seed(0)
    return DSTformer(norm_layer=partial(nn.LayerNorm, eps=1e-6), **GPU_CFG).to('cuda:0')


def run_gpu_case(spec):
    """The recorded calls of one device case (seeded random weights; the prepared-weight cache is emptied first)."""
    from motionbert_amd import engine, hip_ops, model as M
    from motionbert_amd.augment import FLIP_PERM
    dev = torch.device('cuda:0')
    model = _gpu_model()
    model.precision = spec['precision']
    model.train(spec['grad'])
    for p in model.parameters():
        p.grad = None
    g = torch.Generator().manual_seed(1)
    engine.reload_switches({spec['off']: '0'} if spec['off'] else {})
    try:
        with torch.cuda.device(dev):
            hip_ops.get().weight_cache.clear()
            ops = Recorder(hip_ops.get(), launch_stream=torch.cuda.current_stream())
            with torch.set_grad_enabled(spec['grad']):
                if spec['ragged']:
                    clip_tab, frame_t, max_len = M.ragged_tables(GPU_CLIPS, GPU_CFG['maxlen'])
                    x = (torch.rand(1, sum(GPU_CLIPS), 17, 3, generator=g) * 2 - 1).to(dev)
                    ragged = (torch.from_numpy(clip_tab).to(dev), torch.from_numpy(frame_t).to(dev), len(GPU_CLIPS), max_len)
                    M.run(ops, model, x, ('tta', torch.tensor(FLIP_PERM, dtype=torch.int32, device=dev)), ragged=ragged)
                else:
                    x = (torch.rand(GPU_B, GPU_T, 17, 3, generator=g) * 2 - 1).to(dev).requires_grad_(spec['grad'])
                    out = M.run(ops, model, x, False)
                    if spec['grad']:
                        out.sum().backward()
            torch.cuda.synchronize()
    finally:
        engine.reload_switches()
    return ops.calls


def layouts():
    """linear_names / folded_pairs at depth 1 and 5: the flat gradient layout and the descriptor tables follow their order."""
    from motionbert_amd.engine import ModelCfg, folded_pairs, linear_names
    out = {}
    for depth in (1, 5):
        cfg = ModelCfg(dim_in=3, dim_out=3, C=512, R=512, depth=depth, H=8, hidden=1024, J=17, maxlen=243, eps=1e-6, scale=0.125,
                       att_fuse=True, qkv_bias=True)
        out[str(depth)] = dict(linear_names=linear_names(cfg), folded_pairs=[list(p) for p in folded_pairs(cfg)])
    return out


def trace_table(gpu=False):
    """{case: {'sha256': of all its calls, 'calls': 4 hex digits per call (to find the first one that differs)}}"""
    table = {}
    for name, spec in (gpu_cases() if gpu else cases()):
        calls = run_gpu_case(spec) if gpu else run_case(spec)[0]
        digests = [call_digest(c) for c in calls]
        table[name] = dict(sha256=hashlib.sha256(''.join(digests).encode()).hexdigest(), calls=''.join(d[:4] for d in digests))
    return table


def main():
    args = sys.argv[1:]
    if args[:1] == ['--bits']:
        for name, spec in cases():
            print(run_case(spec, bits=True)[1], name)
    elif args[:1] == ['--record']:
        out = args[1] if len(args) > 1 else os.path.join(GOLDEN, 'engine_trace.json')
        t = trace_table()
        with open(out, 'w') as f:
            json.dump({'recorded_from': args[2] if len(args) > 2 else 'working tree', 'cases': t, 'layouts': layouts()}, f, separators=(',', ':'))
            f.write('\n')
        print(f'{out}: {len(t)} cases, {sum(len(c["calls"]) // 4 for c in t.values())} calls')
    elif args[:1] == ['--record-gpu']:
        out = args[1] if len(args) > 1 else os.path.join(GOLDEN, 'engine_trace_gpu.json')
        t = trace_table(gpu=True)
        with open(out, 'w') as f:
            json.dump({'recorded_from': args[2] if len(args) > 2 else 'working tree', 'cases': t}, f, separators=(',', ':'))
            f.write('\n')
        print(f'{out}: {len(t)} cases, {sum(len(c["calls"]) // 4 for c in t.values())} calls')
    else:
        sys.exit(__doc__)


if __name__ == '__main__':
    main()
