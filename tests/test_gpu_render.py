"""The mesh rasteriser on a real MI355X (mbx_render_project and mbx_render_raster in csrc/render.hip, motionbert_amd.render): the gates of
tests/rendererr.py (its own checks on the CPU: tests/test_rendererr.py, tests/test_render.py) applied to the kernels.

Gates.  Projected integers, face_id and depth: equal bits with the host reference.  rgb: the float64 value rounded half up, one level of
freedom only within the derived fp32 bound of a half (at ss = 2 through the exact average); background exactly 255.  Every output is
sentinel-filled beforehand and must be written everywhere; guard rows behind each buffer must be untouched; two runs and a frame-by-frame
render give the bits of the whole.  What was measured goes to render_parity.json / .txt in the directory MBX_REPORT_DIR names (default
reports/)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from tests import rendererr as RE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZE = 72            # no multiple of the 32-sample tile: 3 tiles per side at ss = 1 (the last 8 samples wide), 5 at ss = 2
GUARD_ROWS = 4
REPORT = {}


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'render_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'render_parity.txt'), 'w') as f:
        f.write('mesh rasteriser against the host reference.  `failed`: gate messages (0 passes).  vq / face_id / depth are gated on equal bits.\n'
                '`rgb_off_by_one`: channels that differ from the float64 rounding (each inside its derived interval when failed = 0), of\n'
                '`rgb_channels`; `rgb_free`: channels whose interval holds two values; `bound_max`: the widest fp32 bound, in levels;\n'
                '`covered`: share of samples inside the mesh.\n')
        for k in sorted(REPORT):
            f.write(f'{k:30s} ' + '  '.join(f'{n} {v:.4g}' if isinstance(v, float) else f'{n} {v}' for n, v in sorted(REPORT[k].items())) + '\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def ops():
    from motionbert_amd import hip_ops
    return hip_ops.get()


def _guarded(shape, dtype, fill):
    """a sentinel-filled tensor of `shape` with GUARD_ROWS more leading rows behind it: (view, whole)"""
    whole = torch.full((shape[0] + GUARD_ROWS,) + tuple(shape[1:]), fill, dtype=dtype, device=DEV)
    return whole[:shape[0]], whole


def _raster(ops, vq, verts, faces, size, ss, fills=(7, -77, -77)):
    """mbx_render_raster into sentinel-filled, guarded buffers -> dict of numpy arrays; asserts the guards"""
    F, S = vq.shape[0], size * ss
    rgb, rgb_all = _guarded((F, size, size, 3), torch.uint8, fills[0])
    fid, fid_all = _guarded((F, S, S), torch.int32, fills[1])
    dep, dep_all = _guarded((F, S, S), torch.int32, fills[2])
    ops.render_raster(vq, verts, faces, size, ss, RE.COLOR, RE.ALPHA, rgb, fid, dep)
    torch.cuda.synchronize()
    assert (rgb_all[F:] == fills[0]).all() and (fid_all[F:] == fills[1]).all() and (dep_all[F:] == fills[2]).all(), 'guard rows were written'
    return dict(rgb=rgb.cpu().numpy(), face_id=fid.cpu().numpy(), depth=dep.cpu().numpy())


def _check_raster(ops, name, vq, verts, faces, size, ss, ref=None):
    """gates, every element written (two sentinel values), run-to-run and frame-by-frame bits"""
    tv, tf, tq = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV), torch.from_numpy(vq).to(DEV)
    ref = ref or RE.raster(vq, verts, faces, size, ss)
    got = _raster(ops, tq, tv, tf, size, ss)
    rep = {}
    failed = RE.gate_all(got, ref, ss, rep)
    again = _raster(ops, tq, tv, tf, size, ss, fills=(9, -99, -99))      # an element left unwritten keeps a different sentinel each time
    for k in got:
        if not np.array_equal(got[k], again[k]):
            failed.append(f'{k}: two runs differ (or an element is not written)')
    if vq.shape[0] > 1:
        for f in range(vq.shape[0]):
            one = _raster(ops, tq[f:f + 1].contiguous(), tv[f:f + 1].contiguous(), tf, size, ss)
            for k in got:
                if not np.array_equal(got[k][f:f + 1], one[k]):
                    failed.append(f'{k}: frame {f} on its own differs from the whole')
    REPORT[name] = dict(rep, failed=len(failed))
    assert not failed, failed
    return got


# ------------------------------------------------------------------------------------------------ the float-level scene through the API
@pytest.mark.parametrize('ss', [1, 2])
def test_icosphere_two_tracks(ops, ss):
    """42 vertices / 80 faces deformed over 3 frames, two tracks with different cubes (2 + 1 frames), a NaN vertex in frame 1"""
    verts, faces = RE.deformed_icosphere(3, seed=1)
    verts[1, 5, 0] = np.nan
    tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    clean = tv.clone()
    clean[1, 5] = clean[1, 6]                                          # the cube is taken of finite vertices
    cube = R.frame_cube(clean, [2, 1])
    assert not torch.equal(cube[0], cube[1])
    got = R.render_mesh(tv, tf, cube=cube, seq_lens=[2, 1], size=SIZE, ss=ss, want=('rgb', 'face_id', 'depth', 'vq'))
    torch.cuda.synchronize()
    ref_q = RE.project(verts, cube.cpu().numpy(), [0, 2, 3], SIZE * ss)
    assert ref_q[1, 5, 0] == RE.OUTSIDE
    failed = RE.gate_equal('vq', got['vq'].cpu().numpy(), ref_q)
    ref = RE.raster(ref_q, verts, faces, SIZE, ss)
    rep = {}
    failed += RE.gate_all({k: got[k].cpu().numpy() for k in ('rgb', 'face_id', 'depth')}, ref, ss, rep)
    REPORT[f'icosphere.ss{ss}'] = dict(rep, failed=len(failed))
    assert not failed, failed
    assert 0.1 < rep['covered'] < 0.9
    _check_raster(ops, f'icosphere.raster.ss{ss}', ref_q, verts, faces, SIZE, ss, ref=ref)
    # the chunked generator gives the frames of the whole
    chunks = [c.copy() for c in R.render_chunks(tv, tf, cube=cube, seq_lens=[2, 1], size=SIZE, ss=ss, chunk=2)]
    assert [c.shape[0] for c in chunks] == [2, 1] and np.array_equal(np.concatenate(chunks), got['rgb'].cpu().numpy())


def test_projection_bits(ops):
    """a cloud large enough for a contracted multiply-add to show, more than one vertex chunk, non-finite and far-away values, a frame
    outside every track"""
    g = np.random.default_rng(3)
    v = g.standard_normal((3, 2500, 3)).astype(np.float32)
    v[0, 0] = [np.nan, np.inf, -np.inf]
    v[1, 1] = [1e30, -1e30, 3e9]
    v[1, 2499] = [9.0, -9.0, 9.0]
    cube = torch.tensor([[0.01, -0.02, 0.03, 0.11], [0.5, 0.5, 0.5, 0.2]], dtype=torch.float32, device=DEV)
    ptr = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    for size, ss in ((72, 1), (72, 2), (2048, 2)):
        out, whole = _guarded((3, 2500, 3), torch.int32, -5)
        ops.render_project(torch.from_numpy(v).to(DEV), cube, ptr, size, ss, out)
        torch.cuda.synchronize()
        assert (whole[3:] == -5).all()
        ref = RE.project(v, cube.cpu().numpy(), [0, 1, 2], size * ss)
        assert (ref[2] == RE.OUTSIDE).all() and (ref[0, 0] == RE.OUTSIDE).all()
        failed = RE.gate_equal('vq', out.cpu().numpy(), ref)
        REPORT[f'project.{size}.ss{ss}'] = dict(failed=len(failed), values=int(ref.size))
        assert not failed, failed


# ------------------------------------------------------------------------------------------------ the integer-level cases
@pytest.mark.parametrize('ss', [1, 2])
@pytest.mark.parametrize('name', ['quads', 'whole', 'stack', 'corners', 'dropped'])
def test_crafted(ops, name, ss):
    vq, faces = RE.crafted_cases(SIZE, ss)[name]
    if name == 'stack':
        assert faces.shape[0] % 256 != 0 and faces.shape[0] > 512
    got = _check_raster(ops, f'{name}.ss{ss}', vq, RE.verts_from_vq(vq, SIZE * ss), faces, SIZE, ss)
    if name == 'whole':
        assert (got['face_id'] == 0).all()
    if name == 'dropped':
        assert (got['face_id'][1] == -1).all() and (got['rgb'][1] == 255).all()


def test_property_quads_on_the_device(ops):
    """the exactly-once property on the kernel itself: every sample of a split quad belongs to one face"""
    for n, (vq, faces, _) in enumerate(RE.property_quads()):
        v = RE.verts_from_vq(vq, 32)
        tq, tv = torch.from_numpy(vq).to(DEV), torch.from_numpy(v).to(DEV)
        count = np.zeros((32, 32), np.int64)
        for k in range(len(faces)):
            count += _raster(ops, tq, tv, torch.from_numpy(faces[k:k + 1].copy()).to(DEV), 32, 1)['face_id'][0] >= 0
        both = _raster(ops, tq, tv, torch.from_numpy(faces).to(DEV), 32, 1)['face_id'][0] >= 0
        assert count.max() == 1 and np.array_equal(both, count == 1), n


def test_odd_size_takes_the_byte_stores(ops):
    """size 37: rows of 111 bytes are not dword aligned, the last quad of every row is half outside the image"""
    vq, faces = RE.crafted_cases(SIZE)['corners']
    _check_raster(ops, 'corners.37', vq, RE.verts_from_vq(vq, 37), faces, 37, 1)


def test_full_size(ops):
    """6,890 vertices / 13,776 faces, one frame at 1024 x 1024, through the API"""
    verts, faces = RE.body_like(1, seed=2)
    assert verts.shape == (1, 6890, 3) and faces.shape == (13776, 3)
    tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    cube = R.frame_cube(tv)
    got = R.render_mesh(tv, tf, cube=cube, size=1024, ss=1, want=('rgb', 'face_id', 'depth', 'vq'))
    torch.cuda.synchronize()
    ref_q = RE.project(verts, cube.cpu().numpy(), [0, 1], 1024)
    failed = RE.gate_equal('vq', got['vq'].cpu().numpy(), ref_q)
    rep = {}
    failed += RE.gate_all({k: got[k].cpu().numpy() for k in ('rgb', 'face_id', 'depth')}, RE.raster(ref_q, verts, faces, 1024, 1), 1, rep)
    REPORT['body.1024.ss1'] = dict(rep, failed=len(failed))
    assert not failed, failed
    assert rep['covered'] > 0.1
