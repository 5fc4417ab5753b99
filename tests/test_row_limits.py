"""The row counts the N-resident row-owner kernels serve (mbx_rows_lnbwd_t, mbx_rows_resid_ln: 32-bit byte offsets per tensor) are stated
once on the Python side, engine.rows_lnbwd_fits / rows_resid_ln_fits over engine.ROW_OFFSET_LIMIT, because the engine has to choose its
sequencing per forward, before anything runs.  Here: the predicates at their boundary values, the same boundary read off the library's
own argument checks (no launch: see _refusal), and the engine's call sequence on either side of a limit patched down to the fixture's
size -- beyond it, call for call, the sequence of the A/B switches at 0."""
import ctypes
import importlib.util
import os

import pytest

from motionbert_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predicates_at_their_boundaries():
    # bf16 [M, 1536] (dX of qkv at dim_feat 512): 3072-byte rows, the last row count below 2^32 bytes is 1,398,101
    assert 1398101 * 3072 < 2 ** 32 <= 1398102 * 3072
    assert engine.rows_lnbwd_fits(1398101, 512, 1536) and not engine.rows_lnbwd_fits(1398102, 512, 1536)
    # K = 1024 (dX of fc1): 2^21 rows of 2048 bytes are 2^32 bytes exactly: refused; N alone (K = N = 512): 2^22 rows
    assert engine.rows_lnbwd_fits(2 ** 21 - 1, 512, 1024) and not engine.rows_lnbwd_fits(2 ** 21, 512, 1024)
    assert engine.rows_lnbwd_fits(2 ** 22 - 1, 512, 512) and not engine.rows_lnbwd_fits(2 ** 22, 512, 512)
    # rows_resid_ln: fp32 [M, N] and bf16 [M, K]
    assert engine.rows_resid_ln_fits(2 ** 21 - 1, 512, 512) and not engine.rows_resid_ln_fits(2 ** 21, 512, 512)          # N 4 = 2048
    assert engine.rows_resid_ln_fits(1398101, 256, 1536) and not engine.rows_resid_ln_fits(1398102, 256, 1536)            # K 2 = 3072
    assert engine.rows_resid_ln_fits(2 ** 22 - 1, 256, 256) and not engine.rows_resid_ln_fits(2 ** 22, 256, 256)          # N 4 = 1024
    # the benchmark's 256 clips lie inside both, 339 clips of 243 frames are the first batch outside mbx_rows_lnbwd_t's
    M256 = 256 * 243 * 17
    assert engine.rows_lnbwd_fits(M256, 512, 1536) and engine.rows_resid_ln_fits(M256, 512, 1024)
    assert engine.rows_lnbwd_fits(338 * 4131, 512, 1536) and not engine.rows_lnbwd_fits(339 * 4131, 512, 1536)


@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def _refusal(lib, entry, M, N, K):
    """Why the entry refuses M x N x K when its output ALIASES an input.  Its checks run in the order null pointers, shape, the 32-bit
    offset limits, aliasing, and every one of them returns before anything is launched or dereferenced: the message says on which side
    of the limits M lies, with made-up addresses and without a GPU."""
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]
    f = ctypes.cast(p[3], ctypes.POINTER(ctypes.c_float))
    if entry == 'lnbwd':      # dx_t == dres_t
        rc = lib.mbx_rows_lnbwd_t(p[0], p[1], p[2], f, p[4], p[4], M, N, K, None)
    else:                     # y == resid
        rc = lib.mbx_rows_resid_ln(p[0], p[1], f, f, f, p[5], f, f, 1e-6, M, N, K, None)
    assert rc != 0
    return lib.mbx_last_error().decode()


@pytest.mark.parametrize('entry,N,K', [('lnbwd', 512, 1536), ('lnbwd', 512, 1024), ('lnbwd', 512, 512), ('lnbwd', 256, 1024), ('lnbwd', 256, 256),
                                       ('resid', 512, 512), ('resid', 512, 1024), ('resid', 512, 1536), ('resid', 256, 256), ('resid', 256, 1024)])
def test_python_limits_are_the_librarys(lib, entry, N, K):
    fits = engine.rows_lnbwd_fits if entry == 'lnbwd' else engine.rows_resid_ln_fits
    row_bytes = max(N * (2 if entry == 'lnbwd' else 4), K * 2)
    last = (engine.ROW_OFFSET_LIMIT - 1) // row_bytes      # the largest row count inside
    assert fits(last, N, K) and not fits(last + 1, N, K)
    inside, beyond = _refusal(lib, entry, last, N, K), _refusal(lib, entry, last + 1, N, K)
    assert 'aliases' in inside and '32-bit' not in inside, inside
    assert '32-bit' in beyond and f'M={last + 1}' in beyond, beyond


# ------------------------------------------------------------------------------------------------------------- the engine's sequencing
def _tool():
    spec = importlib.util.spec_from_file_location('engine_trace', os.path.join(ROOT, 'tools', 'engine_trace.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = dict(fixture='tiny_trained', precision='bf16', fold=True, recompute=False, grad=True, drop=False, off=None, att_fuse=True, out='pose')
# tiny_trained: M = 2 x 9 x 17 = 306 rows, C = 64, 3 C = 192, hidden = 128
M_FIX = 306
LNBWD_BYTES = M_FIX * 192 * 2      # dy of qkv's dX: the largest tensor mbx_rows_lnbwd_t meets
RESID_BYTES = M_FIX * 64 * 4       # y of mbx_rows_resid_ln (a of fc2: 306 x 128 x 2, the same)


def _digests(tool, monkeypatch, limit=None, mock_off=(), probes=False, **kw):
    from oracle.torch_ops import MockOps
    with monkeypatch.context() as mp:
        if limit is not None:
            mp.setattr(engine, 'ROW_OFFSET_LIMIT', limit)
        for attr in mock_off:
            mp.setattr(MockOps, attr, False)
        calls, _ = tool.run_case(dict(BASE, **kw))
    if probes:
        return [c[0] for c in calls], [tool.call_digest(c) for c in calls]
    # the capability probes (can_*: no tensors, asked once per Engine) are left out: a switch at 0 is not even asked about
    calls = [c for c in calls if not c[0].startswith('can_')]
    return [c[0] for c in calls], [tool.call_digest(c) for c in calls]


@pytest.mark.parametrize('grad,recompute', [(True, False), (True, True), (False, False)])      # (without a backward there is nothing to rebuild)
def test_engine_falls_back_past_the_limit(monkeypatch, grad, recompute):
    tool = _tool()
    kw = dict(grad=grad, recompute=recompute)
    # rawln (the no-grad sequencing) uses neither kernel: switch it off there so that the forward has something to choose
    if not grad:
        kw['off'] = 'MBX_RAWLN'
    default = _digests(tool, monkeypatch, **kw)
    # one byte of room: still the row-owner sequence, call for call
    assert _digests(tool, monkeypatch, limit=LNBWD_BYTES + 1, **kw) == default
    assert 'rows_resid_ln' in default[0] and ('rows_lnbwd_t' in default[0]) == grad
    # the backward kernel's largest tensor reaches the limit: it gives way to the tile kernels, the forward kernel (smaller tensors) stays
    names, dig = _digests(tool, monkeypatch, limit=LNBWD_BYTES, **kw)
    assert 'rows_lnbwd_t' not in names and 'gemm_nt_gelu_d' not in names and 'gemm_nt_mul' not in names and 'rows_resid_ln' in names
    assert (names, dig) == _digests(tool, monkeypatch, mock_off=('fuse_rows_lnbwd',), **kw)      # exactly the provider without that kernel
    if grad:
        assert names.count('gemm_nt_lnbwd') == 16 and names.count('lnbwd_rowc') == 16 and 'attn_bwd_stats' in names
    # ... and the forward kernel's: both give way
    assert 'rows_resid_ln' in _digests(tool, monkeypatch, limit=RESID_BYTES + 1, **kw)[0]
    names, dig = _digests(tool, monkeypatch, limit=RESID_BYTES, **kw)
    assert 'rows_resid_ln' not in names and 'rows_lnbwd_t' not in names and 'rows_n_pack_many' not in names
    assert (names, dig) == _digests(tool, monkeypatch, mock_off=('fuse_rows_lnbwd', 'fuse_rows_resid_ln'), **kw)


def test_fallback_equals_the_recorded_switch_off_sequence(monkeypatch):
    """Past mbx_rows_lnbwd_t's limit the engine issues the calls tests/golden/engine_trace.json holds for MBX_ROWS_LNBWD=0"""
    import hashlib
    import json
    tool = _tool()
    with open(os.path.join(ROOT, 'tests', 'golden', 'engine_trace.json')) as f:
        golden = json.load(f)['cases']
    _, dig = _digests(tool, monkeypatch, probes=True, off='MBX_ROWS_LNBWD')
    assert hashlib.sha256(''.join(dig).encode()).hexdigest() == golden['tiny_trained-bf16-fold-grad-MBX_ROWS_LNBWD=0']['sha256']
    assert _digests(tool, monkeypatch, limit=LNBWD_BYTES) == _digests(tool, monkeypatch, off='MBX_ROWS_LNBWD')
    _, dig = _digests(tool, monkeypatch, probes=True)
    assert hashlib.sha256(''.join(dig).encode()).hexdigest() == golden['tiny_trained-bf16-fold-grad']['sha256']


def test_a_step_of_339_clips_takes_the_tile_tail():
    """What the decision is about: 339 clips x 243 frames in bf16 at dim_feat 512 used to run the forward for the row-owner tail (the saved
    GELU derivative) and meet the refusal of mbx_rows_lnbwd_t in backward"""
    cfg = engine.ModelCfg(dim_in=3, dim_out=3, C=512, R=512, depth=5, H=8, hidden=1024, J=17, maxlen=243, eps=1e-6, scale=0.125,
                          att_fuse=True, qkv_bias=True)
    caps = engine.Caps(fold=True, gelu_d=True, grad_stream=True, rows_lnbwd=True, rows_resid_ln=True, block_grad_t=True, proj_mlp=True,
                       fuse_ln=True)
    for clips, want in ((256, (True, True)), (338, (True, True)), (339, (False, True)), (507, (False, True)), (508, (False, False))):
        plan = engine.plan_pass(cfg, caps, clips * 243 * 17, need_grad=True, rawln=False)
        lnbwd_rows = any(sp.tail == 'rows' for sp in plan.sub.values())
        resid_rows = any(sp.lin_out == 'rows' for sp in plan.sub.values())
        assert (lnbwd_rows, resid_rows) == (bool(plan.pack_n), bool(plan.pack_f)) == want, clips
        saves = {sp.save for sp in plan.sub.values()}
        assert saves == ({'d', None} if want[0] else {'u', None}), clips
    # at 339 clips no MLP saves the derivative
    plan = engine.plan_pass(cfg, caps, 339 * 243 * 17, need_grad=True, rawln=False)
    assert not any(sp.save == 'd' for sp in plan.sub.values()) and all(sp.tail == 'fold' for sp in plan.sub.values())
