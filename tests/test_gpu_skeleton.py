"""The skeleton rasteriser on a real MI355X (mbx_skeleton_project and mbx_skeleton_raster in csrc/skeleton.hip, motionbert_amd.render): the
gates of tests/skelerr.py (its own checks on the CPU: tests/test_skelerr.py, tests/test_skeleton.py) applied to the kernels.

Gates.  Projected integers, prim_id and rgb: equal bits with the host reference; there is no tolerance.  Every output is sentinel-filled
beforehand and must be written everywhere; guard rows behind each buffer must be untouched; two runs and a frame-by-frame render give the bits
of the whole.  What was measured goes to skeleton_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from tests import skelerr as SE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZE = 72            # no multiple of the 32-sample tile: 3 tiles per side at ss = 1 (the last 8 samples wide), 5 at ss = 2
GUARD_ROWS = 4
REPORT = {}
BONES, COLORS = np.array(R.SKELETON_BONES, np.int32), np.array(R.SKELETON_COLORS, np.uint8)


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'skeleton_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'skeleton_parity.txt'), 'w') as f:
        f.write('skeleton rasteriser against the host reference.  `failed`: gate messages (0 passes).  jq / prim_id / rgb are gated on equal bits.\n'
                '`covered`: share of samples inside a primitive; `prims_seen`: primitives that win a sample; `values`: projected integers;\n'
                '`dropped`: joints that project to the sentinel.\n')
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


def _raster(ops, jq, bones, colors, radii, size, ss, fills=(7, -77)):
    """mbx_skeleton_raster into sentinel-filled, guarded buffers -> dict of numpy arrays; asserts the guards"""
    F, S = jq.shape[0], size * ss
    rgb, rgb_all = _guarded((F, size, size, 3), torch.uint8, fills[0])
    pid, pid_all = _guarded((F, S, S), torch.int32, fills[1])
    ops.skeleton_raster(jq, bones, colors, radii, size, ss, rgb, pid)
    torch.cuda.synchronize()
    assert (rgb_all[F:] == fills[0]).all() and (pid_all[F:] == fills[1]).all(), 'guard rows were written'
    return dict(rgb=rgb.cpu().numpy(), prim_id=pid.cpu().numpy())


def _check_raster(ops, name, jq, bones, colors, radii, size, ss, ref=None):
    """gates, every element written (two sentinel values), run-to-run and frame-by-frame bits"""
    tq, tb, tc = torch.from_numpy(jq).to(DEV), torch.from_numpy(bones).to(DEV), torch.from_numpy(colors).to(DEV)
    ref = ref or SE.raster(jq, bones, colors, radii, size, ss)
    got = _raster(ops, tq, tb, tc, radii, size, ss)
    rep = {}
    failed = SE.gate_all(got, ref, rep)
    again = _raster(ops, tq, tb, tc, radii, size, ss, fills=(9, -99))      # an element left unwritten keeps a different sentinel each time
    for k in got:
        if not np.array_equal(got[k], again[k]):
            failed.append(f'{k}: two runs differ (or an element is not written)')
    if jq.shape[0] > 1:
        for f in range(jq.shape[0]):
            one = _raster(ops, tq[f:f + 1].contiguous(), tb, tc, radii, size, ss)
            for k in got:
                if not np.array_equal(got[k][f:f + 1], one[k]):
                    failed.append(f'{k}: frame {f} on its own differs from the whole')
    REPORT[name] = dict(rep, failed=len(failed))
    assert not failed, failed
    return got


# ------------------------------------------------------------------------------------------------ the projection
def test_projection_bits(ops):
    """a few hundred joints in and around the box, with NaN, infinities, W <= 0 and joints beyond the guard; then the view under which a
    contracted multiply-add would show in the integers"""
    x = SE.joint_cloud(400, seed=5)
    tx = torch.from_numpy(x).to(DEV)
    F, J = x.shape[:2]
    for size, ss in ((72, 1), (72, 2), (37, 1), (2048, 2)):
        ref = SE.project(x, R.SKELETON_VIEW, size * ss)
        assert (ref[0, [0, 1, 2, 4, 7]] == SE.OUTSIDE).all() and (ref[0, 3] != SE.OUTSIDE).all() and (ref[1:] != SE.OUTSIDE).all()
        assert (ref[0, 5:7] == SE.OUTSIDE).all() == (size == 2048)
        outs = []
        for fill in (-5, -6):
            out, whole = _guarded((F, J, 2), torch.int32, fill)
            ops.skeleton_project(tx, R.SKELETON_VIEW, size, ss, out)
            torch.cuda.synchronize()
            assert (whole[F:] == fill).all(), 'guard rows were written'
            outs.append(out.cpu().numpy())
        failed = SE.gate_equal('jq', outs[0], ref) + SE.gate_equal('jq (second run)', outs[1], ref)
        for f in (0, F - 1):
            one, _ = _guarded((1, J, 2), torch.int32, -7)
            ops.skeleton_project(tx[f:f + 1].contiguous(), R.SKELETON_VIEW, size, ss, one)
            failed += SE.gate_equal(f'jq of frame {f} alone', one.cpu().numpy(), ref[f:f + 1])
        REPORT[f'project.{size}.ss{ss}'] = dict(failed=len(failed), values=int(ref.size), dropped=int((ref[..., 0] == SE.OUTSIDE).sum()))
        assert not failed, failed
    out = torch.full((1, 1, 2), -5, dtype=torch.int32, device=DEV)
    ops.skeleton_project(torch.from_numpy(SE.FMA_JOINT).to(DEV), SE.FMA_VIEW, SIZE, 1, out)
    ref = SE.project(SE.FMA_JOINT, SE.FMA_VIEW, SIZE)
    assert ref.tolist() == [[[-1, -1]]] and SE.project(SE.FMA_JOINT, SE.FMA_VIEW, SIZE, ('fma',)).tolist() == [[[0, -1]]]
    REPORT['project.contraction'] = dict(failed=int(not np.array_equal(out.cpu().numpy(), ref)), values=2)
    assert np.array_equal(out.cpu().numpy(), ref), out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the default skeleton through the API
@pytest.mark.parametrize('size,ss', [(SIZE, 1), (SIZE, 2), (37, 1)])
def test_default_skeleton(ops, size, ss):
    """F = 5 at 72 x 72 (three tiles per side, the last 8 wide) and at 37 x 37 (rows of 111 bytes: the byte stores), with the widths of a
    256-px frame so that lines, rings and centres all hold samples"""
    x = SE.walking(5, seed=7)
    x[3, 13] = np.nan                                                  # the left wrist of frame 3: its bone is not drawn
    radii = tuple(ss * r for r in R.skeleton_radii(256))
    got = R.render_skeleton(torch.from_numpy(x).to(DEV), size=size, ss=ss, radii=radii, want=('rgb', 'prim_id', 'jq'))
    torch.cuda.synchronize()
    ref_q = SE.project(x, R.SKELETON_VIEW, size * ss)
    assert (ref_q[3, 13] == SE.OUTSIDE).all()
    failed = SE.gate_equal('jq', got['jq'].cpu().numpy(), ref_q)
    ref = SE.raster(ref_q, BONES, COLORS, radii, size, ss)
    rep = {}
    failed += SE.gate_all({k: got[k].cpu().numpy() for k in ('rgb', 'prim_id')}, ref, rep)
    REPORT[f'default.{size}.ss{ss}'] = dict(rep, failed=len(failed))
    assert not failed, failed
    assert rep['prims_seen'] >= (30 if size == SIZE else 16) and not (ref['prim_id'][3] // 3 == 13).any() and (ref['prim_id'][2] // 3 == 13).any()
    _check_raster(ops, f'default.raster.{size}.ss{ss}', ref_q, BONES, COLORS, radii, size, ss, ref=ref)
    # the reference's own widths, and the chunked generator against the whole
    thin = R.render_skeleton(x, size=size, ss=ss, want=('rgb', 'prim_id'))
    ref_thin = SE.raster(ref_q, BONES, COLORS, R.skeleton_radii(size, ss), size, ss)
    assert not SE.gate_all({k: thin[k].cpu().numpy() for k in ('rgb', 'prim_id')}, ref_thin)
    chunks = [p.copy() for p in R.skeleton_chunks(x, size=size, ss=ss, radii=radii, chunk=2)]
    assert [p.shape[0] for p in chunks] == [2, 2, 1] and np.array_equal(np.concatenate(chunks), got['rgb'].cpu().numpy())


# ------------------------------------------------------------------------------------------------ the integer-level cases
@pytest.mark.parametrize('ss', [1, 2])
@pytest.mark.parametrize('name', ['degenerate', 'exact_r', 'tile_corner', 'radius_40', 'r_zero', 'outside', 'guard', 'sentinel', 'stack', 'order'])
def test_crafted(ops, name, ss):
    jq, bones, colors, radii = SE.crafted_cases(SIZE, ss)[name]
    got = _check_raster(ops, f'{name}.ss{ss}', jq, bones, colors, radii, SIZE, ss)
    pid = got['prim_id']
    if name == 'degenerate':
        assert set(np.unique(pid)) == {-1, 0, 2}                       # the marker at b covers the marker at a
    if name == 'r_zero':
        assert (pid >= 0).sum() == 36 + 58 and not (pid // 3 == 2).any()
    if name == 'guard':
        assert set(np.unique(pid)) == {0, 3}                           # every cross product of the last bone is beyond 2^31: rejected
    if name == 'sentinel':
        assert set(np.unique(pid[0] // 3)) == {-1, 0, 3, 6} and (pid[1] == -1).all() and (got['rgb'][1] == 255).all()
    if name == 'stack':
        assert pid.max() // 3 == 63
    if name == 'order':
        assert pid[0, 35, 36] == 3 and pid[0, 35, 20] == 8              # the later line over the earlier marker; the later marker over the line
    if name == 'radius_40':
        assert len({(i // 32, j // 32) for i, j in zip(*np.nonzero(pid[0] >= 0))}) >= 4


def test_full_size(ops):
    """two frames of the default skeleton at 1024 x 1024, through the API, with the reference's own widths"""
    x = SE.walking(2, seed=11)
    got = R.render_skeleton(torch.from_numpy(x).to(DEV), size=1024, want=('rgb', 'prim_id', 'jq'))
    torch.cuda.synchronize()
    ref_q = SE.project(x, R.SKELETON_VIEW, 1024)
    failed = SE.gate_equal('jq', got['jq'].cpu().numpy(), ref_q)
    rep = {}
    failed += SE.gate_all({k: got[k].cpu().numpy() for k in ('rgb', 'prim_id')}, SE.raster(ref_q, BONES, COLORS, R.skeleton_radii(1024), 1024, 1), rep)
    REPORT['default.1024.ss1'] = dict(rep, failed=len(failed))
    assert not failed, failed
    assert rep['prims_seen'] >= 30 and 0.001 < rep['covered'] < 0.1
