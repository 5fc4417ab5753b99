"""The JPEG kernels on a real MI355X (csrc/jpeg.hip, motionbert_amd.video): the gates of tests/jpegerr.py (its own checks on the CPU:
tests/test_jpegerr.py, tests/test_video.py) applied to the kernels.

Gates.  Coefficients, scan bytes and whole files: equal bytes with libjpeg-turbo's own output (tests/golden/jpeg_pil.npz) and with the numpy
reference; there is no tolerance.  Every output is sentinel-filled beforehand; guard bytes behind each buffer must be untouched; F = 3 frames
in one call give the bytes of three calls, and two runs give the same bits.  What was measured goes to jpeg_parity.json / .txt in the directory
MBX_REPORT_DIR names (default reports/)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from motionbert_amd import video as V
from tests import jpegerr as J
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096
REPORT = {}
CASES, VERSIONS = J.load_fixture(os.path.join(GOLDEN, 'jpeg_pil.npz'))


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'jpeg_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, fixture=VERSIONS, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'jpeg_parity.txt'), 'w') as f:
        f.write('JPEG kernels against libjpeg-turbo\'s files (' + ', '.join(VERSIONS) + ') and the numpy reference.  `failed`: gate messages (0 passes);\n'
                'every gate is byte equality.  `coef_diff`: differing coefficients of mbx_jpeg_blocks; `file_diff`: differing files; `bytes`: size of\n'
                'the compared files; `ratio`: raw RGB bytes over file bytes.\n')
        for k in sorted(REPORT):
            f.write(f'{k:40s} ' + '  '.join(f'{n} {v:.4g}' if isinstance(v, float) else f'{n} {v}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def _guarded(n, dtype, fill):
    """a sentinel-filled 1-D tensor of n elements with GUARD more behind it: (view, whole)"""
    whole = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return whole[:n], whole


def _blocks(ops, rgb, quality, sub, fill=-21846):
    F, H, W = rgb.shape[:3]
    mx, my, bpm = J.geometry(H, W, sub)
    coef, whole = _guarded(F * mx * my * bpm * 64, torch.int16, fill)
    coef = coef.view(F, mx * my, bpm, 64)
    ops.jpeg_blocks(rgb, quality, int(sub == '420'), coef)
    torch.cuda.synchronize()
    assert (whole[coef.numel():] == fill).all(), 'guard elements behind coef were written'
    return coef


def _entropy(ops, coef, H, W, sub, quality, restart, fill=0xA5):
    """mbx_jpeg_entropy_sizes + mbx_jpeg_entropy into sentinel-filled, guarded buffers -> (data, offsets) as numpy; asserts the guards"""
    F, s = coef.shape[0], int(sub == '420')
    off, off_all = _guarded(F + 1, torch.int64, -7)
    ws = ops.jpeg_ws(F, H, W, s, restart, coef.device)
    ops.jpeg_sizes(coef, H, W, s, quality, restart, off, ws)
    total = int(off[F])
    assert (off_all[F + 1:] == -7).all(), 'guard elements behind offsets were written'
    data, data_all = _guarded(total, torch.uint8, fill)
    ops.jpeg_emit(coef, H, W, s, quality, restart, off, data, ws)
    torch.cuda.synchronize()
    assert (data_all[total:] == fill).all(), 'guard bytes behind data were written'
    return data.cpu().numpy(), off.cpu().numpy()


@pytest.mark.parametrize('i', range(len(CASES)), ids=[J.case_name(c) for c in CASES])
def test_fixture_case(ops, i):
    """every stage against libjpeg-turbo: coefficients, the scan from ITS coefficients, the whole file from the pixels"""
    c = CASES[i]
    H, W, q, sub, rs = c['H'], c['W'], c['quality'], c['sub'], c['restart']
    rgb = torch.from_numpy(c['rgb'][None]).to(DEV)
    coef = _blocks(ops, rgb, q, sub)
    failed = J.gate_equal('coef', coef[0].cpu().numpy(), c['coef'])
    coef_diff = int((coef[0].cpu().numpy() != c['coef']).sum())
    data, off = _entropy(ops, torch.from_numpy(c['coef'][None]).to(DEV), H, W, sub, q, rs)
    parsed = J.parse(c['file'], decode=False)
    failed += J.gate_files('entropy', data, off, [c['file']])
    if len(data) == len(c['file']):
        failed += J.gate_equal('scan', data[parsed['header_len']:-2], np.frombuffer(parsed['scan'], np.uint8))
    whole, woff = V.encode_jpeg(rgb, q, sub, rs)
    failed += J.gate_files('file', whole.cpu().numpy(), woff.cpu().numpy(), [c['file']])
    again, _ = _entropy(ops, torch.from_numpy(c['coef'][None]).to(DEV), H, W, sub, q, rs, fill=0x5A)      # an unwritten byte keeps another sentinel
    if not np.array_equal(again, data):
        failed.append('entropy: two runs differ (or a byte is not written)')
    REPORT[J.case_name(c)] = dict(failed=len(failed), coef_diff=coef_diff, file_diff=int(whole.cpu().numpy().tobytes() != c['file']),
                                  bytes=len(c['file']), ratio=3.0 * H * W / len(c['file']))
    assert not failed, failed


@pytest.mark.parametrize('name', sorted(J.crafted_blocks()))
def test_crafted_blocks(ops, name):
    """the corners of the entropy coder, as 4:4:4 MCUs, against the numpy coder"""
    coef, rs = J.crafted_blocks()[name]
    n = coef.shape[0]
    my = 1 if n <= 256 else 2
    H, W = 8 * my, 8 * (n // my)
    assert (W // 8) * my == n
    data, off = _entropy(ops, torch.from_numpy(coef[None]).to(DEV), H, W, '444', 90, rs)
    ref = J.header(H, W, 90, '444', rs) + J.scan(coef, rs) + b'\xff\xd9'
    failed = J.gate_files(name, data, off, [ref])
    REPORT['crafted.' + name] = dict(failed=len(failed), bytes=len(ref))
    assert not failed, failed


def test_frames_together_equal_frames_alone(ops):
    """F = 3 different frames in one call against three calls of one frame (the offsets too), for both subsamplings"""
    frames = np.stack([J.content(k, 40, 56, seed=9) for k in ('noise', 'render', 'ramp')])
    rgb = torch.from_numpy(frames).to(DEV)
    failed = []
    for sub, rs in (('420', None), ('444', 5)):
        data, off = V.encode_jpeg(rgb, 75, sub, rs)
        data2, off2 = V.encode_jpeg(rgb, 75, sub, rs)
        assert torch.equal(data, data2) and torch.equal(off, off2), 'two runs differ'
        alone = [V.frames_to_host(*V.encode_jpeg(rgb[f:f + 1].contiguous(), 75, sub, rs))[0] for f in range(3)]
        failed += J.gate_files(f'together.{sub}', data.cpu().numpy(), off.cpu().numpy(), alone)
        failed += J.gate_files(f'reference.{sub}', data.cpu().numpy(), off.cpu().numpy(), [J.encode(f, 75, sub, rs) for f in frames])
        assert V.frames_to_host(data, off) == alone
    e, o = V.encode_jpeg(rgb[:0], 75)
    assert e.shape == (0,) and o.tolist() == [0] and e.is_cuda
    REPORT['frames_together'] = dict(failed=len(failed))
    assert not failed, failed


def _check_video(name, path, frames_bytes, rgb, quality, sub):
    got = J.avi_frames(open(path, 'rb').read())
    refs = [J.encode(f, quality, sub) for f in rgb]
    failed = [f'{name}: {len(got)} chunks for {len(refs)} frames'] if len(got) != len(refs) else []
    for f, (g, r) in enumerate(zip(got, refs)):
        failed += J.gate_file(f'{name} frame {f}', g[:len(r)] if len(g) == len(r) + 1 and len(r) & 1 else g, r)      # a chunk is padded to even length
    REPORT[name] = dict(failed=len(failed), bytes=frames_bytes[1], ratio=float(rgb.size) / frames_bytes[1])
    assert frames_bytes == (len(refs), os.path.getsize(path))
    assert not failed, failed


def test_skeleton_video(tmp_path):
    from tests import skelerr as SE
    x = SE.walking(5, seed=7)
    radii = R.skeleton_radii(256)
    path = str(tmp_path / 'x3d.avi')
    res = V.skeleton_video(path, x, 25, quality=90, size=72, radii=radii, chunk=2)
    rgb = R.render_skeleton(x, size=72, radii=radii)['rgb'].cpu().numpy()
    assert (rgb != 255).any()
    _check_video('skeleton_video.72', path, res, rgb, 90, '420')


def test_mesh_video(tmp_path):
    from motionbert_amd.smpl import SMPLLayer, SMPLModel
    from tests import smplerr as SM
    model = SMPLModel.synthetic(257, 55)
    layer = SMPLLayer(model).to(DEV)
    inp = SM.inputs(5, 257, 17, 77, model)
    with torch.no_grad():
        verts, _ = layer.forward_kp(inp['betas'].to(DEV), inp['rot'].to(DEV))
    faces = torch.from_numpy(np.random.default_rng(4).integers(0, 257, (400, 3)).astype(np.int32)).to(DEV)
    path = str(tmp_path / 'mesh.avi')
    res = V.mesh_video(path, verts.contiguous(), faces, 30, quality=75, subsampling='444', size=72, chunk=2)
    rgb = R.render_mesh(verts.contiguous(), faces, size=72)['rgb'].cpu().numpy()
    assert (rgb != 255).any()
    _check_video('mesh_video.72', path, res, rgb, 75, '444')
