"""The numpy model of the self-synchronising entropy decode (tests/jpegsyncerr.py) against the reference of the one-lane decode
(tests/jpegdecerr.py), on the CPU: the model equals it on every input, every seeded corruption fails, every chosen input has the property
it is chosen for, video.decode_jpeg takes the new route end to end, and the library's two symbols refuse bad arguments before any launch.
The kernels themselves are held to this model in tests/test_gpu_jpeg_sync.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from motionbert_amd import video as V
from tests import jpegdecerr as D
from tests import jpegerr as J
from tests import jpegsyncerr as Y
from tests.helpers import GOLDEN

CASES, _ = D.load_fixture(os.path.join(GOLDEN, 'jpeg_dec_pil.npz'))
PROBES = ('white.2048', 'white.256', 'noise', 'cut', 'malformed.cut', 'malformed.run_past_63', 'malformed.unused_code', 'malformed.trailing_byte',
          'sweep.48')
SMALL_WS = 300                                                           # the max_interval_bytes of the long-interval probes


@pytest.mark.parametrize('i', range(len(CASES)), ids=[D.case_name(c) for c in CASES])
def test_model_equals_the_reference_on_the_fixture(i):
    ref_coef, ref_status, _ = D.entropy(CASES[i]['file'])
    coef, status, route = Y.entropy_sync(CASES[i]['file'])
    assert not J.gate_equal('coef', coef, ref_coef) and not J.gate_equal('status', status, ref_status)
    assert not route.any(), 'a well-formed file of a few chunks is decoded in parallel'


@pytest.mark.parametrize('name', sorted(Y.inputs()))
def test_model_equals_the_reference_on_the_inputs(name):
    (ref_coef, ref_status), (coef, status, route) = Y.reference(name)
    assert not J.gate_equal('coef', coef, ref_coef) and not J.gate_equal('status', status, ref_status)
    if name != 'white.2048':                                              # the fallback is taken where the one-lane body finds an error, only there
        assert ((route != 0) == ((ref_status != D.OK) & (ref_status != D.MARKERS))).all()


@pytest.mark.parametrize('corrupt', Y.CORRUPTIONS)
def test_every_corruption_fails_a_gate(corrupt):
    failed = []
    for name in PROBES:
        kw = dict(max_interval_bytes=SMALL_WS) if corrupt == 'long_interval_unflagged' else {}
        (ref_coef, ref_status), (_, _, ref_route) = Y.reference(name)
        if kw:
            ref_route = Y.entropy_sync(Y.inputs()[name], **kw)[2]
        coef, status, route = Y.entropy_sync(Y.inputs()[name], corrupt=(corrupt,), **kw)
        failed += J.gate_equal(f'{name}.coef', coef, ref_coef) + J.gate_equal(f'{name}.status', status, ref_status)
        failed += J.gate_equal(f'{name}.route', route, ref_route)
    assert failed, f'the corruption {corrupt} passes every gate'


def _interval(name):
    f = Y.inputs()[name]
    p = D.parse(f)
    return f[p['scan'][0]:p['scan'][1]], p, D.geometry(p['H'], p['W'], p['sub'])[2]


def test_inputs_have_the_properties_they_are_chosen_for():
    raw, p, bpm = _interval('noise')
    r = np.frombuffer(raw, np.uint8)
    pair = np.nonzero((r[:-1] == 0xff) & (r[1:] == 0))[0]                # the FF of every FF 00
    on_00 = [b for b in range(Y.S, len(raw), Y.S) if raw[b - 1] == 0xff and raw[b] == 0]
    assert on_00 and ((pair + 1) % Y.S == 0).any(), 'no FF 00 pair straddles a subsequence boundary, so no subsequence begins on the 00'
    assert all(Y.Stream(raw, p['dht'], bpm).first(b // Y.S) == (8 * (b + 1), 0, 0) for b in on_00)
    plan = Y.plan(raw, p['dht'], bpm)
    assert plan['n_chunk'] >= 2 and plan['route'] == 0 and Y.reference('noise')[1][2].tolist() == [0]
    raw, p, bpm = _interval('noise.512')
    plan = Y.plan(raw, p['dht'], bpm)
    assert plan['n_chunk'] >= 3 and plan['route'] == 0 and Y.reference('noise.512')[1][2].tolist() == [0]
    raw, p, bpm = _interval('white.2048')
    plan = Y.plan(raw, p['dht'], bpm)
    assert plan['n_chunk'] >= 2 and plan['route'] == 1 and not all(plan['chunk_ok'])
    for name in ('white.64', 'white.256'):                                # one chunk: the induction from lane 0, a lane per round
        raw, p, bpm = _interval(name)
        plan = Y.plan(raw, p['dht'], bpm)
        assert plan['n_chunk'] == 1 and plan['route'] == 0 and Y.rounds(raw, p['dht'], bpm) == plan['n_sub']
        assert name == 'white.64' or plan['n_sub'] > 4, 'the induction has nothing to walk'
    lengths = sorted(len(_interval(f'sweep.{n:02d}')[0]) for n in range(1, 49))
    assert len({-(-n // Y.S) for n in lengths}) >= 20, 'the sweep crosses few multiples of S'
    assert len(_interval('white.64')[0]) < Y.S < lengths[0], 'the scan shorter than S is white.64 (the smallest noise frame of the sweep is not)'
    raw, p, bpm = _interval('longest')
    plan = Y.plan(raw, p['dht'], bpm)
    # The issue names a block that spans THREE subsequences, i.e. a lane in the middle of an interval that completes no block.  That exists
    # at S = 128 only: the longest baseline block is 22 + 63 * 26 = 1,660 bits, less than one subsequence of 8 * 256 bits, so at the S that
    # is kept every subsequence but the last sees a block end.  What is left to demand is that the blocks span TWO: lanes entered mid-block
    inside = [j for j in range(1, plan['n_sub']) if plan['entry'][j][2] != 0]
    assert len(inside) >= 3, 'the blocks of 1,660 bits do not span subsequences'
    assert 1660 < 8 * Y.S or any(c[0] == 0 for c in plan['cnt'][:-1]), 'no subsequence lies inside one block although one could'
    assert Y.reference('cut')[0][1].tolist() == [D.TRUNCATED] and Y.reference('cut')[0][0].any()


def test_long_interval_is_flagged_and_exact():
    for name in ('noise', 'sweep.48'):
        (ref_coef, ref_status), _ = Y.reference(name)
        coef, status, route = Y.entropy_sync(Y.inputs()[name], max_interval_bytes=SMALL_WS)
        assert route.tolist() == [3] and not J.gate_equal('coef', coef, ref_coef) and not J.gate_equal('status', status, ref_status)


def test_decode_jpeg_through_the_new_route():
    files = [Y.inputs()[k] for k in ('sweep.20', 'sweep.20', 'sweep.48')]
    ops = Y.SyncRefOps()
    res = V.decode_jpeg(files[:2], device='cpu', ops=ops, entropy='sync', want=('rgb', 'coef', 'status', 'route'))
    assert ('dec_entropy_sync', 2) in ops.calls and not any(c[0] == 'dec_entropy' for c in ops.calls)
    assert res['route'].shape == (2, 1) and res['route'].dtype == torch.int32 and not res['route'].any() and not res['status'].any()
    for f in range(2):
        assert not J.gate_equal('rgb', res['rgb'][f].numpy(), D.decode(files[f])) and not J.gate_equal('coef', res['coef'][f].numpy(), D.entropy(files[f])[0])
    ops = Y.SyncRefOps()                                                  # 'auto': one interval per frame takes 'sync', more take 'interval'
    V.decode_jpeg([files[0]], device='cpu', ops=ops)
    many = [c['file'] for c in CASES if c['restart'] == 1 and (c['H'], c['W']) == (31, 7)][0]
    got = V.decode_jpeg([many], device='cpu', ops=ops)
    assert [c[0] for c in ops.calls if c[0].startswith('dec_entropy')] == ['dec_entropy_sync', 'dec_entropy']
    assert not J.gate_equal('rgb', got[0].numpy(), D.decode(many))
    ops = Y.SyncRefOps()                                                  # 'sync' works for any number of intervals
    res = V.decode_jpeg([many], device='cpu', ops=ops, entropy='sync', want=('rgb', 'route'))
    assert ('dec_entropy_sync', 1) in ops.calls and res['route'].shape[1] > 1 and not J.gate_equal('rgb', res['rgb'][0].numpy(), D.decode(many))
    with pytest.raises(ValueError, match='status 1'):                     # a malformed interval raises on this route as on the other
        V.decode_jpeg([Y.inputs()['cut']], device='cpu', ops=Y.SyncRefOps(), entropy='sync')
    res = V.decode_jpeg([Y.inputs()['cut']], device='cpu', ops=Y.SyncRefOps(), entropy='sync', want=('status', 'route'))
    assert res['status'].tolist() == [[D.TRUNCATED]] and res['route'].tolist() == [[2]]
    with pytest.raises(ValueError, match='entropy must be one of'):
        V.decode_jpeg(files[:1], device='cpu', ops=Y.SyncRefOps(), entropy='parallel')


def test_a_provider_without_the_new_method():
    files = [Y.inputs()['sweep.20']]
    ops = D.RefOps()
    auto = V.decode_jpeg(files, device='cpu', ops=ops, want=('rgb', 'route'))
    assert [c[0] for c in ops.calls] == ['dec_index', 'dec_entropy', 'dec_pixels'] and not auto['route'].any()
    assert torch.equal(auto['rgb'], V.decode_jpeg(files, device='cpu', ops=D.RefOps(), entropy='interval'))
    with pytest.raises(RuntimeError, match='jpeg_dec_entropy_sync'):
        V.decode_jpeg(files, device='cpu', ops=D.RefOps(), entropy='sync')
    with pytest.raises(ValueError, match='entropy must be one of'):
        V.MJPEGReader(os.devnull, entropy='parallel')


# ------------------------------------------------------------------------------------------------ the library without a GPU
@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_symbols_and_version(lib):
    assert lib.mbx_version() >= 260
    assert hasattr(lib, 'mbx_jpeg_dec_entropy_sync') and hasattr(lib, 'mbx_jpeg_dec_sync_ws')
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'mbx.h')).read()
    assert Y.S == 256 and Y.CH == 256 and 'mbx_jpeg_dec_entropy_sync' in header


def test_workspace_grows_with_its_arguments(lib):
    ws = lib.mbx_jpeg_dec_sync_ws
    base = ws(1, 1, 100000)
    assert base > 0 and ws(2, 1, 100000) > base and ws(1, 2, 100000) > base and ws(1, 1, 400000) > base
    assert ws(1, 1, 0) > 0 and ws(1, 1, 1) == ws(1, 1, Y.S * Y.CH) < ws(1, 1, Y.S * Y.CH + 1)
    assert ws(0, 1, 100) == 0 and ws(1, 0, 100) == 0 and ws(1, 1, -1) == 0 and ws(1, 1, Y.MAX_BYTES + 1) == 0 and ws(70000, 1, 100) == 0


def test_argument_errors_are_reported_not_launched(lib):
    fn = lib.mbx_jpeg_dec_entropy_sync
    buf = (ctypes.c_char * 4096)()                                        # host memory that passes for a pointer: no call here gets to a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.mbx_jpeg_dec_sync_ws(1, 1, 1000)

    def call(data=p, data_bytes=64, pos=p, tables=p, F=1, H=16, W=16, sub=0, restart=0, longest=1000, coef=p, status=p, route=p, ws=p, ws_bytes=need):
        return fn(data, data_bytes, pos, tables, F, H, W, sub, restart, longest, coef, status, route, ws, ws_bytes, None)
    for name in ('data', 'pos', 'tables', 'coef', 'status', 'route', 'ws'):
        assert call(**{name: None}) != 0 and b'null' in lib.mbx_last_error(), name
    assert call(ws_bytes=need - 1) != 0 and b'workspace' in lib.mbx_last_error()
    assert call(ws_bytes=0) != 0 and b'workspace' in lib.mbx_last_error()
    assert call(longest=-1) != 0 and b'max_interval_bytes' in lib.mbx_last_error()
    assert call(data_bytes=-1) != 0 and b'data_bytes' in lib.mbx_last_error()
    assert call(F=-1) != 0 and b'bad sizes' in lib.mbx_last_error()
    assert call(F=65536) != 0 and b'bad sizes' in lib.mbx_last_error()
    assert call(H=0) != 0 and call(W=4096) != 0 and call(sub=3) != 0 and call(restart=-1) != 0
    assert call(F=0, data=None, pos=None, tables=None, coef=None, status=None, route=None, ws=None, ws_bytes=0) == 0, 'F = 0 is a no-op'
