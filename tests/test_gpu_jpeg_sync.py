"""The self-synchronising entropy decode on a real MI355X (csrc/jpeg_sync.hip) against the kernel it must equal and against its numpy model
(tests/jpegsyncerr.py; the model's own checks on the CPU: tests/test_jpegsyncerr.py, the kernels' decode on the host: tests/test_jpeg_sync_host.py).

Gates, for every call: coef and status equal those of ops.jpeg_dec_entropy on the same input and those of the model; route equals the
model's (it is a property of the bytes, the tables, S and CH); there is no tolerance.  coef, status, route and ws are sentinel-filled
beforehand; guard elements behind each of them must be untouched; two runs with different sentinels in ws (and coef) give the same bits.
What was measured goes to jpeg_sync_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd import video as V
from tests import jpegdecerr as D
from tests import jpegerr as J
from tests import jpegsyncerr as Y
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096
REPORT = {}
CASES, VERSIONS = D.load_fixture(os.path.join(GOLDEN, 'jpeg_dec_pil.npz'))
NAMED = [k for k in sorted(Y.inputs()) if not k.startswith('sweep')]


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'jpeg_sync_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, fixture=VERSIONS, S=Y.S, CH=Y.CH, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'jpeg_sync_parity.txt'), 'w') as f:
        f.write(f'mbx_jpeg_dec_entropy_sync (S = {Y.S} bytes, CH = {Y.CH} subsequences) against mbx_jpeg_dec_entropy on the same input and against the\n'
                'numpy model.  `failed`: gate messages (0 passes); every gate is equality.  `coef_diff` / `status_diff`: elements that differ from the\n'
                "one-lane kernel's; `route`: per value, the intervals that took it (0 parallel, 1 a chunk not self-contained, 2 a strict check, 3 longer\n"
                'than the host said); `bytes`: the longest interval; `chunks`: of that interval.\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + '  '.join(f'{n} {v}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return whole[:n].view(shape), whole


def _both(ops, files, fill=-21846, max_bytes=None):
    """index, then the one-lane kernel and the new one on the same F files (one header), every output sentinel-filled and guarded ->
    numpy (status, coef) of the one-lane kernel, (status, coef, route) of the new one, the longest interval"""
    p = D.parse(files[0])
    H, W, sub, F = p['H'], p['W'], D.SUB_CODE[p['sub']], len(files)
    mx, my, bpm = D.geometry(H, W, p['sub'])
    n_int = D.n_intervals(H, W, p['sub'], p['restart'])
    off = np.concatenate([[0], np.cumsum([len(f) for f in files])])
    data, data_all = _guarded((int(off[-1]),), torch.uint8, 0)
    data.copy_(torch.from_numpy(np.frombuffer(b''.join(files), np.uint8).copy()))
    data_all[int(off[-1]):] = 0xFF
    facts = [D.parse(x) for x in files]
    scans = torch.tensor([[off[f] + q['scan'][0], off[f] + q['scan'][1]] for f, q in enumerate(facts)], dtype=torch.int64, device=DEV)
    longest = max(q['scan'][1] - q['scan'][0] for q in facts) if max_bytes is None else max_bytes
    pos = torch.empty(F, n_int + 1, dtype=torch.int64, device=DEV)
    st0 = torch.empty(F, n_int, dtype=torch.int32, device=DEV)
    ops.jpeg_dec_index(data, scans, n_int, pos, st0)
    tables = ops.jpeg_dec_tables(p['dht']).to(DEV)
    ref_status, ref_coef = st0.clone(), torch.full((F, mx * my, bpm, 64), fill, dtype=torch.int16, device=DEV)
    ops.jpeg_dec_entropy(data, pos, tables, H, W, sub, p['restart'], ref_coef, ref_status)
    status, status_all = _guarded((F, n_int), torch.int32, -9)
    status.copy_(st0)
    route, route_all = _guarded((F, n_int), torch.int32, -13)
    coef, coef_all = _guarded((F, mx * my, bpm, 64), torch.int16, fill)
    n_ws = ops.jpeg_dec_sync_ws(F, n_int, longest, DEV).numel()
    ws, ws_all = _guarded((n_ws,), torch.uint8, fill & 0xFF)
    ops.jpeg_dec_entropy_sync(data, pos, tables, H, W, sub, p['restart'], longest, coef, status, route, ws)
    torch.cuda.synchronize()
    assert (status_all[status.numel():] == -9).all() and (route_all[route.numel():] == -13).all(), 'guard elements behind status / route were written'
    assert (coef_all[coef.numel():] == fill).all(), 'guard elements behind coef were written'
    assert (ws_all[n_ws:] == (fill & 0xFF)).all(), 'guard bytes behind ws were written'
    real = int((pos[:, 1:] - 2 - pos[:, :-1]).max())
    return (ref_status.cpu().numpy(), ref_coef.cpu().numpy()), (status.cpu().numpy(), coef.cpu().numpy(), route.cpu().numpy()), real


def _gates(ops, name, files, models, max_bytes=None):
    """every gate of the module's docstring for one call; models: per file (coef, status, route) of the numpy model"""
    (ref_status, ref_coef), (status, coef, route), real = _both(ops, files, max_bytes=max_bytes)
    failed = J.gate_equal(f'{name}.coef', coef, ref_coef) + J.gate_equal(f'{name}.status', status, ref_status)
    for f, (m_coef, m_status, m_route) in enumerate(models):
        failed += J.gate_equal(f'{name}.{f}.model.coef', coef[f], m_coef) + J.gate_equal(f'{name}.{f}.model.status', status[f], m_status)
        failed += J.gate_equal(f'{name}.{f}.route', route[f], m_route)
    _, again, _ = _both(ops, files, fill=23130, max_bytes=max_bytes)
    if not all(np.array_equal(a, b) for a, b in zip(again, (status, coef, route))):
        failed.append(f'{name}: two runs with different sentinels differ (or an element is not written)')
    REPORT[name] = dict(failed=len(failed), coef_diff=int((coef != ref_coef).sum()), status_diff=int((status != ref_status).sum()), bytes=real,
                        chunks=int(np.ceil(np.ceil(real / Y.S) / Y.CH)), route={int(v): int((route == v).sum()) for v in np.unique(route)})
    return failed, status, coef, route


@pytest.mark.parametrize('i', range(len(CASES)), ids=[D.case_name(c) for c in CASES])
def test_fixture_case(ops, i):
    """the files Pillow wrote (restart 0, 1, 3, one row, more than the frame; 4:2:2; optimised tables) through 'sync', and the pixels"""
    c = CASES[i]
    failed, status, _, route = _gates(ops, D.case_name(c), [c['file']], [Y.entropy_sync(c['file'])])
    assert not status.any() and not route.any()
    res = V.decode_jpeg([c['file']], device=DEV, entropy='sync', want=('rgb', 'route'))
    failed += J.gate_equal('decode_jpeg', res['rgb'][0].cpu().numpy(), c['rgb'])
    assert not res['route'].any()
    assert not failed, failed


def test_sweep_of_scan_lengths(ops):
    """4:4:4 noise frames 8 x 8 n at quality 100: the scan's end falls everywhere inside a subsequence, and on both sides of many multiples of S"""
    failed = []
    for n in range(1, 49):
        name = f'sweep.{n:02d}'
        f, _, _, route = _gates(ops, name, [Y.inputs()[name]], [Y.reference(name)[1]])
        failed += f
        assert not route.any()
    assert not failed, failed


@pytest.mark.parametrize('name', NAMED)
def test_named_input(ops, name):
    """noise over several chunks (route 0), the white frames (one chunk by induction; two chunks: route 1 and exact through the fallback), the
    blocks of 1,660 bits, the file cut inside its scan, and the malformed scans: status, zeros and kept blocks as the one-lane kernel's"""
    ref, model = Y.reference(name)
    failed, status, coef, route = _gates(ops, name, [Y.inputs()[name]], [model])
    failed += J.gate_equal('reference.coef', coef[0], ref[0]) + J.gate_equal('reference.status', status[0], ref[1])
    expect = {'noise': [0], 'noise.512': [0], 'white.64': [0], 'white.256': [0], 'white.2048': [1], 'longest': [0], 'cut': [2]}
    if name in expect:
        assert route[0].tolist() == expect[name]
    if name == 'cut':
        assert status[0].tolist() == [D.TRUNCATED] and coef[0].any() and not coef[0][-1].any()
    if name.startswith('malformed.'):
        _, k, st = D.malformed()[name[10:]]
        assert status[0, k] == st
        with pytest.raises(ValueError, match=f'restart interval {0 if st == D.MARKERS else k} of 3: status {st}'):
            V.decode_jpeg([Y.inputs()[name]], device=DEV, entropy='sync')
    assert not failed, failed


def test_frames_together_equal_frames_alone(ops):
    """three frames with different scan lengths in one call against three calls; a cut frame twice beside a whole one; three headers"""
    lengths = [Y.one_interval(J.content('noise', 24, 80, seed=s), 90, '420') for s in (1, 2, 3)]      # one header, three scan lengths
    assert len({len(f) for f in lengths}) == 3
    failed = []
    for n, group in enumerate((lengths, [Y.inputs()['cut']] * 2 + [Y.one_interval(J.content('render', 64, 64), 90, '444')])):
        f, status, coef, route = _gates(ops, f'together.{n}', group, [Y.entropy_sync(x) for x in group])
        failed += f
        for k, x in enumerate(group):
            _, (s1, c1, r1), _ = _both(ops, [x])
            failed += J.gate_equal(f'alone.{n}.{k}.coef', coef[k], c1[0]) + J.gate_equal(f'alone.{n}.{k}.status', status[k], s1[0])
            failed += J.gate_equal(f'alone.{n}.{k}.route', route[k], r1[0])
    assert route[:, 0].tolist() == [2, 2, 0]
    files = [Y.one_interval(J.content('noise', 24, 80, seed=s), q, '420') for s, q in ((1, 100), (2, 60), (3, 90))]
    got = V.decode_jpeg(files, device=DEV, entropy='sync')                # three quantisation tables: three groups
    for k, x in enumerate(files):
        failed += J.gate_equal(f'mixed.{k}', got[k].cpu().numpy(), D.decode(x))
    assert not failed, failed


def test_interval_longer_than_the_host_said(ops):
    """max_interval_bytes below the real interval: route 3, the exact result, and nothing outside the smaller ws"""
    for name, small in (('noise', 300), ('sweep.48', 1), ('white.256', 0), ('noise', Y.S * Y.CH)):
        _, (coef, status, _) = Y.reference(name)
        failed, _, _, route = _gates(ops, f'long.{name}.{small}', [Y.inputs()[name]], [(coef, status, np.array([3], np.int32))], max_bytes=small)
        assert route.tolist() == [[3]] and not failed, failed


def test_reader_auto_equals_interval(tmp_path):
    """an AVI of frames without restart markers inside the frame: 'auto' takes the new route and gives the pixels of 'interval'"""
    H, W, F = 48, 64, 5
    files = [Y.one_interval(J.content(k, H, W, seed=s), 90, '420') for s, k in enumerate(('noise', 'render', 'ramp', 'white', 'noise'))]
    path = str(tmp_path / 'plain.avi')
    with V.MJPEGWriter(path, W, H, 25) as w:
        w.write(b''.join(files), np.concatenate([[0], np.cumsum([len(f) for f in files])]))
    with V.MJPEGReader(path) as auto, V.MJPEGReader(path, entropy='interval') as interval, V.MJPEGReader(path, entropy='sync') as sync:
        assert auto.entropy == 'auto' and auto.frames == F
        a, b, c = auto.read(), interval.read(), sync.read()
        failed = J.gate_equal('auto', a.cpu().numpy(), b.cpu().numpy()) + J.gate_equal('sync', c.cpu().numpy(), b.cpu().numpy())
        failed += J.gate_equal('reference', a.cpu().numpy(), np.stack([D.decode(f) for f in files]))
        failed += J.gate_equal('chunks', torch.cat([x.clone() for x in auto.chunks(2)]).cpu().numpy(), b.cpu().numpy())
    res = V.decode_jpeg(files, device=DEV, want=('coef', 'route', 'status'))
    assert res['route'].shape == (F, 1) and not res['route'].any() and not res['status'].any()
    assert torch.equal(res['coef'], V.decode_jpeg(files, device=DEV, entropy='interval', want=('coef',))['coef'])
    REPORT['reader.auto.48x64'] = dict(failed=len(failed))
    assert not failed, failed
