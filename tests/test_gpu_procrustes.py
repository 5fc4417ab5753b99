"""The Procrustes solver on a real MI355X outside the region the fixtures guarantee (csrc/pose_solve.h behind mbx_pose_errors and
mbx_mesh_errors): every family of tests/procerr.py -- conditioned, planar, mirrored, equal singular values, other units, J = 2 .. 64,
poses exactly on a line (H of rank one), needles down to s1 / s0 = 1e-12 -- against the reference's LAPACK route in float64
(eval_fixture.NumpyOps.pose_errors, mesherr.rigid_align64).  The gate is procerr.gate: 1e-10 relative where s1 / s0 >= 1e-3, plus the
transverse extent of the thinner pose below that; it is derived there from the inputs alone, and tests/test_procerr.py shows on the CPU
that it rejects the routine without its rank-one guard (NaN on an axis-aligned line and on J = 2, several per cent on an oblique line).

What was measured goes to procrustes_parity.json / .txt in the directory MBX_REPORT_DIR names (default reports/): per family the worst
|d| / allowed with its frame and the s1 / s0 range.  Nothing in the report feeds a gate.

Measured on the MI355X (profiles/procrustes_parity.txt): see that file; every ratio below 1, the worst 0.54 on a needle, 4e-3 of the gate
where s1 / s0 >= 1e-3.  The library before the guard, same tests, same device: e2 NaN on all 203 frames of `line.pred.axis`,
`line.gt.axis` and `J2.axis` (pose and mesh form) and NaN action means and summary in the evaluator test; `line.gt.oblique` finite but
off by up to 8.7 % (pose form), 5.1 % / 8.9 % (mesh form, 17 / 14 joints); `J2.random`, `line.pred.oblique` and `line.both`, on which the
CPU model of that code has NaN frames, passed on the device (fma contraction leaves another rounding residue in H v1)."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from tests import eval_fixture as FX
from tests import mesherr as ME
from tests import procerr as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F64 = torch.float64
REPORT = {}
NAMES = list(P.families())
MESH_NAMES = P.mesh_names()


def _report_dir():
    return os.environ.get('MBX_REPORT_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reports')


@pytest.fixture(scope='module', autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'procrustes_parity.json'), 'w') as f:
        json.dump(dict(seconds=time.time() - t0, cases=REPORT), f, indent=1, sort_keys=True)
    with open(os.path.join(out, 'procrustes_parity.txt'), 'w') as f:
        f.write('Procrustes-aligned errors against float64 LAPACK: worst |d| / allowed per family (<= 1 passes; inf: a frame that is not finite)\n')
        groups = {}
        for k in sorted(REPORT):
            r = REPORT[k]
            if 'worst' not in r:
                f.write(f'{k:34s} ' + '  '.join(f'{n} {v:.4g}' for n, v in sorted(r.items())) + '\n')
                continue
            f.write(f'{k:34s} worst {r["worst"]:.4g} at frame {r["frame"]}  not finite {r["not_finite"]}  s1/s0 {r["cond_min"]:.3g} .. {r["cond_max"]:.3g}'
                    f'  worst relative error {r["rel"]:.3g}\n')
            g = groups.setdefault(f'{k.split(":")[0]}: {P.group(k.split(":")[1])}', [0.0, math.inf, 0.0])
            g[0], g[1], g[2] = max(g[0], r['worst']), min(g[1], r['cond_min']), max(g[2], r['cond_max'])
        f.write('per family group\n')
        for k in sorted(groups):
            f.write(f'{k:34s} worst {groups[k][0]:.4g}  s1/s0 {groups[k][1]:.3g} .. {groups[k][2]:.3g}\n')
        f.write(f'module wall time {time.time() - t0:.1f} s\n')


@pytest.fixture(scope='module')
def cases():
    return P.cases()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared cases are read-only)


def guarded(n, pad=64):
    """a NaN-filled fp64 output of n elements inside a larger NaN-filled buffer: (the output, a check that nothing around it was written)"""
    buf = torch.full((n + 2 * pad,), math.nan, dtype=F64, device=DEV)

    def untouched():
        return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all())
    return buf[pad:pad + n], untouched


def record(tag, got, ref, allowed, s):
    r = P.ratios(got, ref, allowed)
    cond = s[:, 1] / s[:, 0]
    fin = np.isfinite(r)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(fin & (ref > 0), np.abs(np.where(fin, got, 0.0) - ref) / ref, 0.0)
    REPORT[tag] = dict(worst=float(r.max()), frame=int(r.argmax()), not_finite=int((~fin).sum()), cond_min=float(cond.min()), cond_max=float(cond.max()),
                       rel=float(rel.max()))
    print(f'{tag}: worst |d| / allowed {r.max():.3g} at frame {int(r.argmax())}, {int((~fin).sum())} frames not finite, s1/s0 {cond.min():.3g} .. {cond.max():.3g}')
    return r


@pytest.fixture(scope='module')
def device_errors(cases):
    """{family: (e1, e2, nothing written around them)} of mbx_pose_errors, one call per family: run once, shared, never written to"""
    from motionbert_amd import pose_errors
    out = {}
    for name, c in cases.items():
        n = len(c.pred)
        (e1, ok1), (e2, ok2) = guarded(n), guarded(n)
        pose_errors(dev(c.pred[:, None]), dev(c.gt[:, None]), out=(e1.view(n, 1), e2.view(n, 1)))
        torch.cuda.synchronize()
        out[name] = (e1.cpu().numpy(), e2.cpu().numpy(), ok1() and ok2())
    return out


@pytest.mark.parametrize('name', NAMES)
def test_pose_errors_on_every_family(cases, device_errors, name):
    """e1 to the project's gate, e2 inside procerr.gate and finite on every frame, nothing written outside the outputs.  J = 2 and J = 64
    are the two ends of the LDS row stride 3J | 1 (7 and 193 words), J = 3 and 4 the next ones."""
    c = cases[name]
    e1, e2, untouched = device_errors[name]
    assert untouched, 'the kernel wrote outside its outputs'
    d1 = np.abs(e1 - c.e1_ref)
    print(f'{name}: e1 worst |d| {np.nanmax(d1):.3e} (an e1 of exactly 0, pred == gt, is matched exactly)')
    r = record(f'pose:{name}', e2, c.e2_ref, c.allowed, c.s)
    assert np.isfinite(e1).all() and bool((d1 <= FX.GATE * c.e1_ref).all())
    assert np.isfinite(e2).all(), f'e2 is not finite on {int((~np.isfinite(e2)).sum())} frames, the first one {int(np.argmin(np.isfinite(e2)))}'
    assert r.max() <= 1.0


def test_a_degenerate_lane_does_not_disturb_its_neighbours(cases, device_errors):
    """every J = 17 family interleaved frame by frame in one [1,F,17,3] call, so that every wave holds rank-one, needle and ordinary frames side
    by side: the bits of the per-family calls"""
    from motionbert_amd import pose_errors
    names = [n for n in NAMES if cases[n].pred.shape[1] == 17]
    pred = np.stack([cases[n].pred for n in names], 1).reshape(1, -1, 17, 3)          # frame f of family k at f * len(names) + k
    gt = np.stack([cases[n].gt for n in names], 1).reshape(1, -1, 17, 3)
    e1, e2 = pose_errors(dev(pred), dev(gt))
    assert e1.shape == (1, P.FRAMES * len(names))
    e1, e2 = e1.cpu().numpy().reshape(P.FRAMES, len(names)), e2.cpu().numpy().reshape(P.FRAMES, len(names))
    for k, n in enumerate(names):
        assert np.array_equal(e1[:, k].view(np.int64), device_errors[n][0].view(np.int64)), n
        assert np.array_equal(e2[:, k].view(np.int64), device_errors[n][1].view(np.int64)), n
    # and the families one after the other (whole waves of degenerate frames next to whole waves of ordinary ones)
    pred, gt = np.concatenate([cases[n].pred for n in names])[None], np.concatenate([cases[n].gt for n in names])[None]
    q1, q2 = pose_errors(dev(pred), dev(gt))
    assert np.array_equal(q1.cpu().numpy().reshape(-1).view(np.int64), np.concatenate([device_errors[n][0] for n in names]).view(np.int64))
    assert np.array_equal(q2.cpu().numpy().reshape(-1).view(np.int64), np.concatenate([device_errors[n][1] for n in names]).view(np.int64))


@pytest.mark.parametrize('name', MESH_NAMES)
def test_mesh_errors_on_the_degenerate_families(cases, name):
    """the J = 17 families as kp_p / kp_g of mbx_mesh_errors, with 7 vertices or none: the plain rows as tests/test_gpu_mesh.py gates them,
    PA-MPJPE over 17 joints and over the 14-joint subset inside the mesh form of the gate"""
    from motionbert_amd import hip_ops
    c = cases[name]
    n = len(c.pred)
    with_verts = MESH_NAMES.index(name) % 2 == 0
    vp = vg = None
    if with_verts:
        g = torch.Generator().manual_seed(9100 + MESH_NAMES.index(name))
        vp, vg = 300.0 * torch.randn(n, 7, 3, generator=g), 300.0 * torch.randn(n, 7, 3, generator=g)
    ref = ME.mesh_errors64(None if vp is None else vp.numpy(), None if vg is None else vg.numpy(), c.pred, c.gt)
    err, untouched = guarded(5 * n)
    err = err.view(5, n)
    hip_ops.get().mesh_errors(None if vp is None else vp.to(DEV), None if vg is None else vg.to(DEV), dev(c.pred), dev(c.gt), err)
    torch.cuda.synchronize()
    assert untouched(), 'the kernel wrote outside its output'
    got = err.cpu().numpy()
    plain = ME.err_ratio(got[:3], ref[:3])
    REPORT[f'mesh:{name}:plain rows'] = dict(ratio=plain)
    idx = list(ME.H36M_17_TO_14)
    r17 = record(f'mesh17:{name}', got[3], ref[3], P.gate(c.pred, c.gt, ref[3]), c.s)
    r14 = record(f'mesh14:{name}', got[4], ref[4], P.gate(c.pred[:, idx], c.gt[:, idx], ref[4]), P.spectrum(c.pred[:, idx], c.gt[:, idx])[0])
    assert with_verts or bool(np.isnan(got[0]).all())
    assert np.isfinite(got[1:]).all(), 'a joint row is not finite'
    assert plain <= 1.0 and r17.max() <= 1.0 and r14.max() <= 1.0


def test_one_collinear_clip_leaves_the_evaluation_finite(cases):
    """The synthetic split of the evaluation fixture with the predictions of one clip replaced by poses on a coordinate axis: per action
    and summary equal the fp64 aggregation of the reference's errors.  One NaN frame would turn its action and the summary into NaN."""
    b = FX.part_b(FX.load())
    case = (0, 1, 0)
    ev = FX.make_evaluator(b, case)
    clip = int(np.nonzero(ev.keep_clip)[0][0])
    T = ev.T
    line = cases['line.pred.axis'].pred
    assert T <= len(line) and b['outputs'].shape[2] == 17
    b = dict(b, outputs=b['outputs'].copy())
    b['outputs'][clip] = line[:T] / 512.0                       # normalised image coordinates; still exactly on an axis
    e1, e2, per = FX.run_split(ev, b, DEV)
    ops = FX.NumpyOps()
    split = b['split']
    r1, r2 = torch.empty(len(split), T, dtype=F64), torch.empty(len(split), T, dtype=F64)
    ops.pose_errors(torch.from_numpy(b['outputs']), torch.from_numpy(b['gts'][split]), torch.from_numpy(b['hw_clips'].astype(np.float32)),
                    torch.from_numpy(b['factors'][split].astype(np.float32)), None, False, r1, r2)
    assert bool(torch.isfinite(r2).all())
    A = len(ev.action_names)
    ref_per, ref_sum, ref_count = torch.empty(2, A, dtype=F64), torch.empty(2, dtype=F64), torch.empty(A, dtype=torch.int32)
    ops.eval_reduce(r1, r2, torch.from_numpy(ev.row_ptr_host), torch.from_numpy(ev.slots_host), ev.action_id.cpu(), A, ref_per, ref_sum, ref_count)
    got = np.array([[per[a][0] for a in ev.action_names], [per[a][1] for a in ev.action_names]])
    print(f'clip {clip} on a line: summary {e1!r} {e2!r}, reference {ref_sum.tolist()}')
    clip_e2 = ev.e2[clip].cpu().numpy()
    assert np.isfinite(clip_e2).all(), 'e2 of the collinear clip'
    assert np.isfinite(got).all() and np.isfinite([e1, e2]).all() and ev.count.cpu().tolist() == ref_count.tolist()
    r_per, r_sum = FX.rel_err(got, ref_per.numpy()), FX.rel_err([e1, e2], ref_sum.numpy())
    REPORT['evaluator:line.pred.axis'] = dict(per_action=r_per / FX.GATE, summary=r_sum / FX.GATE)
    assert r_per < FX.GATE and r_sum < FX.GATE
