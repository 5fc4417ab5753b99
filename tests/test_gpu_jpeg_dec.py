"""The JPEG decoding kernels on a real MI355X (csrc/jpeg_dec.hip, the reading half of motionbert_amd.video): the gates of tests/jpegdecerr.py
(its own checks on the CPU: tests/test_jpegdecerr.py, tests/test_video_read.py) applied to the kernels.

Gates.  Restart positions, coefficients and pixels: equal with the numpy reference and with what libjpeg-turbo decodes
(tests/golden/jpeg_dec_pil.npz); there is no tolerance.  Every output is sentinel-filled beforehand; guard elements behind each buffer must be
untouched; F = 3 frames in one call give the pixels of three calls, and two runs give the same bits.  Malformed scans are ordinary inputs with
a defined output: their status code, zeros, untouched guards.  What was measured goes to jpeg_dec_parity.json / .txt in the directory
MBX_REPORT_DIR names (default reports/)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from motionbert_amd import video as V
from tests import jpegdecerr as D
from tests import jpegerr as J
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096
REPORT = {}
CASES, VERSIONS = D.load_fixture(os.path.join(GOLDEN, 'jpeg_dec_pil.npz'))


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'jpeg_dec_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, fixture=VERSIONS, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'jpeg_dec_parity.txt'), 'w') as f:
        f.write('JPEG decoding kernels against the pixels libjpeg-turbo decodes (' + ', '.join(VERSIONS) + ') and the numpy reference.  `failed`: gate\n'
                'messages (0 passes); every gate is equality.  `pos_diff` / `coef_diff` / `pixel_diff`: differing restart positions, coefficients and\n'
                'pixel values of the three kernels; `e2e_diff`: of decode_jpeg; `bytes`: size of the file; `intervals`: restart intervals.\n')
        for k in sorted(REPORT):
            f.write(f'{k:44s} ' + '  '.join(f'{n} {v:.4g}' if isinstance(v, float) else f'{n} {v}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def _guarded(shape, dtype, fill):
    """a sentinel-filled tensor with GUARD more elements behind it: (view, whole)"""
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return whole[:n].view(shape), whole


def _stages(ops, files, fill=-21846):
    """the three kernels one by one on F files that share a header, every output sentinel-filled and guarded -> numpy pos, status, coef, rgb
    (rgb from the REFERENCE's coefficients when every status is 0, so that each kernel answers for itself)"""
    p = D.parse(files[0])
    H, W, sub, F = p['H'], p['W'], D.SUB_CODE[p['sub']], len(files)
    mx, my, bpm = D.geometry(H, W, p['sub'])
    n_int = D.n_intervals(H, W, p['sub'], p['restart'])
    off = np.concatenate([[0], np.cumsum([len(f) for f in files])])
    data, data_all = _guarded((int(off[-1]),), torch.uint8, 0)
    data.copy_(torch.from_numpy(np.frombuffer(b''.join(files), np.uint8).copy()))
    data_all[int(off[-1]):] = 0xFF                                        # behind the files: bytes a reader must never take for a marker's partner
    scans = torch.tensor([[off[f] + D.parse(x)['scan'][0], off[f] + D.parse(x)['scan'][1]] for f, x in enumerate(files)], dtype=torch.int64, device=DEV)
    pos, pos_all = _guarded((F, n_int + 1), torch.int64, -7)
    status, status_all = _guarded((F, n_int), torch.int32, -9)
    coef, coef_all = _guarded((F, mx * my, bpm, 64), torch.int16, fill)
    rgb, rgb_all = _guarded((F, H, W, 3), torch.uint8, fill & 0xFF)
    ops.jpeg_dec_index(data, scans, n_int, pos, status)
    tables = ops.jpeg_dec_tables(p['dht']).to(DEV)
    ops.jpeg_dec_entropy(data, pos, tables, H, W, sub, p['restart'], coef, status)
    st = status.cpu().numpy()
    src = coef if st.any() else torch.from_numpy(np.stack([D.entropy(x)[0] for x in files])).to(DEV)
    ops.jpeg_dec_pixels(src, p['q'], H, W, sub, rgb, ops.jpeg_dec_ws(F, H, W, sub, DEV))
    torch.cuda.synchronize()
    assert (pos_all[pos.numel():] == -7).all() and (status_all[status.numel():] == -9).all(), 'guard elements behind pos / status were written'
    assert (coef_all[coef.numel():] == fill).all(), 'guard elements behind coef were written'
    assert (rgb_all[rgb.numel():] == (fill & 0xFF)).all(), 'guard bytes behind rgb were written'
    return pos.cpu().numpy(), st, coef.cpu().numpy(), rgb.cpu().numpy(), off


@pytest.mark.parametrize('i', range(len(CASES)), ids=[D.case_name(c) for c in CASES])
def test_fixture_case(ops, i):
    """every stage against the reference and libjpeg-turbo: positions, coefficients, pixels from ITS coefficients, decode_jpeg end to end"""
    c = CASES[i]
    ref_coef, ref_status, ref_pos = D.entropy(c['file'])
    assert not ref_status.any()
    pos, status, coef, rgb, _ = _stages(ops, [c['file']])
    failed = J.gate_equal('pos', pos[0], ref_pos) + J.gate_equal('status', status[0], ref_status) + J.gate_equal('coef', coef[0], ref_coef)
    failed += J.gate_equal('pixels', rgb[0], c['rgb'])
    e2e = V.decode_jpeg([c['file']], device=DEV)
    failed += J.gate_equal('decode_jpeg', e2e[0].cpu().numpy(), c['rgb'])
    again = _stages(ops, [c['file']], fill=23130)                         # an unwritten element keeps another sentinel
    if not (np.array_equal(again[2], coef) and np.array_equal(again[3], rgb) and np.array_equal(again[0], pos)):
        failed.append('two runs differ (or an element is not written)')
    REPORT[D.case_name(c)] = dict(failed=len(failed), pos_diff=int((pos[0] != ref_pos).sum()), coef_diff=int((coef[0] != ref_coef).sum()),
                                  pixel_diff=int((rgb[0] != c['rgb']).sum()), e2e_diff=int((e2e[0].cpu().numpy() != c['rgb']).sum()),
                                  bytes=len(c['file']), intervals=len(ref_status))
    assert not failed, failed


def test_range_table_beyond_the_clamp(ops):
    """the crafted scan whose samples leave the part of the range-limit table a clamp would give (jpegdecerr.crafted_range)"""
    data = D.crafted_range()
    _, status, _, rgb, _ = _stages(ops, [data])
    failed = J.gate_equal('pixels', rgb[0], D.decode(data))
    assert not status.any() and J.gate_equal('clamp', rgb[0], D.decode(data, corrupt=('clamp_not_table',)))
    REPORT['crafted.range_table'] = dict(failed=len(failed))
    assert not failed, failed


def test_frames_together_equal_frames_alone(ops):
    """F = 3 different frames in one call against three calls of one frame, for the three subsamplings; a call of mixed headers; F = 0"""
    failed = []
    for sub in ('420', '422', '444'):
        files = [J.encode(J.content(k, 40, 56, seed=9), 75, sub, 5) for k in ('noise', 'render', 'ramp')] if sub != '422' else \
            [c['file'] for c in CASES if (c['H'], c['W'], c['sub'], c['quality'], c['optimize']) == (17, 33, '422', 100, False)]
        assert len(files) == 3 and len(set(files)) == 3
        pos, status, coef, rgb, off = _stages(ops, files)
        assert not status.any()
        for f, x in enumerate(files):
            p1, s1, c1, r1, _ = _stages(ops, [x])
            failed += J.gate_equal(f'together.{sub}.{f}.coef', coef[f], c1[0]) + J.gate_equal(f'together.{sub}.{f}.rgb', rgb[f], r1[0])
            failed += J.gate_equal(f'together.{sub}.{f}.pos', pos[f] - off[f], p1[0]) + J.gate_equal(f'reference.{sub}.{f}', rgb[f], D.decode(x))
    mixed = [c['file'] for c in CASES if (c['H'], c['W']) == (17, 33)]
    got = V.decode_jpeg(mixed, device=DEV)
    assert torch.equal(got, V.decode_jpeg(mixed, device=DEV)), 'two runs differ'
    for f, x in enumerate(mixed):
        failed += J.gate_equal(f'mixed.{f}', got[f].cpu().numpy(), D.decode(x))
    dev_data = torch.from_numpy(np.frombuffer(b''.join(mixed), np.uint8).copy()).to(DEV)
    assert torch.equal(V.decode_jpeg(dev_data, np.cumsum([0] + [len(x) for x in mixed])), got)
    out = torch.full_like(got, 0x5A)
    assert V.decode_jpeg(mixed, device=DEV, out=out) is out and torch.equal(out, got)      # 'cuda' names the current device
    e = V.decode_jpeg([], device=DEV)
    assert e.shape == (0, 0, 0, 3) and e.is_cuda
    REPORT['frames_together'] = dict(failed=len(failed))
    assert not failed, failed


@pytest.mark.parametrize('name', sorted(J.crafted_blocks()))
def test_crafted_blocks_through_the_coder_and_back(ops, name):
    """the corners of the entropy coder (4:4:4 MCUs) through mbx_jpeg_entropy and back through mbx_jpeg_dec_entropy"""
    coef, rs = J.crafted_blocks()[name]
    n = coef.shape[0]
    my = 1 if n <= 256 else 2
    H, W = 8 * my, 8 * (n // my)
    dev = torch.from_numpy(coef[None]).to(DEV)
    off = torch.empty(2, dtype=torch.int64, device=DEV)
    ws = ops.jpeg_ws(1, H, W, 0, rs, DEV)
    ops.jpeg_sizes(dev, H, W, 0, 90, rs, off, ws)
    data = torch.empty(int(off[1]), dtype=torch.uint8, device=DEV)
    ops.jpeg_emit(dev, H, W, 0, 90, rs, off, data, ws)
    back = V.decode_jpeg(data, off, want=('coef', 'status'))
    failed = J.gate_equal(name, back['coef'][0].cpu().numpy(), coef)
    assert not back['status'].any()
    REPORT['crafted.' + name] = dict(failed=len(failed), bytes=int(off[1]))
    assert not failed, failed


def test_skeleton_render_round_trip():
    """decode_jpeg(encode_jpeg(x)) against the reference decode of the same bytes, for a 72 x 72 skeleton render"""
    from tests import skelerr as SE
    rgb = R.render_skeleton(SE.walking(3, seed=7), size=72, radii=R.skeleton_radii(256))['rgb']
    assert (rgb != 255).any()
    data, off = V.encode_jpeg(rgb, 90, '420')
    got = V.decode_jpeg(data, off).cpu().numpy()
    failed = []
    for f, x in enumerate(V.frames_to_host(data, off)):
        failed += J.gate_equal(f'frame {f}', got[f], D.decode(x))
    REPORT['skeleton_round_trip.72'] = dict(failed=len(failed), psnr_db=float(10 * np.log10(255 ** 2 / max(np.mean((got.astype(float) - rgb.cpu().numpy()) ** 2), 1e-9))))
    assert not failed, failed


@pytest.mark.parametrize('name', sorted(D.malformed()))
def test_malformed_scans_have_a_defined_result(ops, name):
    """ordinary inputs with a defined output: the status code, zeros from the block the error lies in, untouched guards, and decode_jpeg raises"""
    data, k, st = D.malformed()[name]
    ref_coef, ref_status, ref_pos = D.entropy(data)
    pos, status, coef, _, _ = _stages(ops, [data, data])                  # twice in one call: the second frame's offsets are not the first's
    failed = []
    for f in range(2):
        failed += J.gate_equal(f'status.{f}', status[f], ref_status) + J.gate_equal(f'coef.{f}', coef[f], ref_coef)
        failed += J.gate_equal(f'pos.{f}', pos[f] - f * len(data), ref_pos)
    assert status[0, k] == st
    with pytest.raises(ValueError, match=f'restart interval {0 if st == D.MARKERS else k} of 3: status {st}'):
        V.decode_jpeg([data], device=DEV)
    REPORT['malformed.' + name] = dict(failed=len(failed), status=int(st))
    assert not failed, failed


def test_scene_video_over_a_reader(tmp_path):
    """one scene_video at 96 x 72 over an MJPEGReader against the tensor route, byte for byte; the reader's chunks against its read"""
    from tests import sceneerr as SC
    from tests import skelerr as SE
    W, H, Fv = 96, 72, 5
    g = np.random.default_rng(5)
    ids = {3: np.arange(5), 8: np.array([1, 2, 4])}
    x3d = {k: np.stack([np.array([30 + 30 * n + 2 * t, 36, 0.0]) + 30 * SE.POSE + g.normal(0, 0.2, SE.POSE.shape) for t in v]).astype(np.float32)
           for n, (k, v) in enumerate(ids.items())}
    table = R.scene_table(ids)
    bg = torch.from_numpy(SC.backdrop(Fv, W, H, seed=4)).to(DEV)
    src, a, b = str(tmp_path / 'in.avi'), str(tmp_path / 'a.avi'), str(tmp_path / 'b.avi')
    data, off = V.encode_jpeg(bg, 90, '420')
    with V.MJPEGWriter(src, W, H, 25) as w:
        w.write(data.cpu().numpy(), off.cpu().numpy())
    with V.MJPEGReader(src) as r:
        assert (r.frames, r.width, r.height, r.fps) == (Fv, W, H, 25.0)
        decoded = r.read()
        failed = J.gate_equal('read', decoded.cpu().numpy(), np.stack([D.decode(r.frame_bytes(f)) for f in range(Fv)]))
        parts = torch.cat([p.clone() for p in r.chunks(2)])
        failed += J.gate_equal('chunks', parts.cpu().numpy(), decoded.cpu().numpy())
        res = V.scene_video(a, x3d, table, W, H, 25, background=r, chunk=2)
        assert res == (Fv, os.path.getsize(a))
        V.scene_video(b, x3d, table, W, H, 25, background=decoded, chunk=2)
    if open(a, 'rb').read() != open(b, 'rb').read():
        failed.append('scene_video over the reader and over the decoded tensor write different files')
    REPORT['scene_video.reader.96x72'] = dict(failed=len(failed), bytes=res[1])
    assert not failed, failed
