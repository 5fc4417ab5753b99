#!/usr/bin/env python
"""Mint tests/golden/mesh.npz with the REFERENCE's own lib/utils/utils_mesh.py and lib/model/loss_mesh.py (imported read-only at run time
from the checkout oracle/make_golden.py names: MOTIONBERT_REFERENCE).  loss_mesh.py imports `ipdb`, which need not be installed: an
empty stand-in module is registered first.  lib/model/model_mesh.py needs `smplx` and cannot be imported; its head arithmetic is the two
utils_mesh calls rot6d_to_rotmat and rotation_matrix_to_angle_axis.

    python tools/mint_mesh.py             # write the fixture
    python tools/mint_mesh.py --check     # mint again and compare every array with the committed file, bit for bit

Inputs come from the seeded makers of tests/mesherr.py and are not stored.  Every result is the reference's code in float64 on the fp32 bits
of the inputs; `.ref32` is the yardstick of the fp32 gates: max |error| / max |float64 value| of the SAME code run in float32.
  rot.{M}.rows                       the joints whose rows are kept (all, or the first and last 32)
  rot.{M}.rotmat / .aa / .dx6        [rows, 9 / 3 / 6]; dx6 = autograd of sum(rotmat drot) + sum(aa daa) for the maker's cotangents
  rot.{M}.{rotmat,aa,dx6}.ref32      the yardsticks, over ALL rows
  loss.{F}.rows                      the frames whose dtheta rows are kept
  loss.{F}.t{0,1}.losses             [3] = loss_pose, loss_shape, loss_norm of MeshLoss(loss_type MSE / L1)
  loss.{F}.t{0,1}.dtheta             d (sum mesherr.LAMBDAS3 * losses) / d pred_theta, [rows, 82]
  loss.{F}.t{0,1}.{losses,dtheta}.ref32    yardsticks ([3] per loss; one number for dtheta)
  err.{F}.{V}.rows                   [5, F] per frame (mesherr.ERR_ROWS), V = 6890 only: compute_error_frames (MPVE, MPJPE-17), the 14-joint MPJPE
                                     and rigid_align per frame as evaluate_mesh applies them
  err.{F}.{V}.dict                   evaluate_mesh's five means in the order of mesherr.ERR_ROWS
(the reference's evaluation hard-codes 6890 vertices; the V = 7 case of the GPU test has the restatement alone, which the V = 6890 cases pin)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden                             # noqa: E402
from tests import mesherr as ME                            # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'mesh.npz')


def import_reference_mesh():
    """(utils_mesh, loss_mesh) of the reference, without shadowing by this repository's own lib/ shim"""
    REF = make_golden.REF
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'lib' or k.startswith('lib.')}
    had_ipdb = 'ipdb' in sys.modules
    try:
        for name, sub in (('lib', 'lib'), ('lib.model', 'lib/model'), ('lib.utils', 'lib/utils')):
            pkg = types.ModuleType(name)
            pkg.__path__ = [os.path.join(REF, sub)]
            sys.modules[name] = pkg
        if not had_ipdb:
            sys.modules['ipdb'] = types.ModuleType('ipdb')
        mods = []
        for name, path in (('lib.utils.utils_mesh', 'lib/utils/utils_mesh.py'), ('lib.model.loss', 'lib/model/loss.py'),
                           ('lib.model.loss_mesh', 'lib/model/loss_mesh.py')):
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            mods.append(mod)
        return mods[0], mods[2]
    finally:
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            sys.modules.pop(k)
        if not had_ipdb:
            sys.modules.pop('ipdb', None)
        sys.modules.update(saved)


def ref_rot(U, x6, drot, daa, dtype):
    x = x6.detach().clone().to(dtype).requires_grad_(True)
    R = U.rot6d_to_rotmat(x)
    aa = U.rotation_matrix_to_angle_axis(R.reshape(-1, 3, 3))
    ((R.reshape(-1, 9) * drot.to(dtype)).sum() + (aa * daa.to(dtype)).sum()).backward()
    return R.detach().reshape(-1, 9), aa.detach(), x.grad


def ref_losses(L, pred, gt, loss_type, dtype):
    crit = L.MeshLoss(loss_type=('MSE', 'L1')[loss_type], device='cpu')
    p = pred.detach().clone().to(dtype).requires_grad_(True)
    F = p.shape[0]
    kp = torch.zeros(1, F, 17, 3, dtype=dtype)
    kp[..., 1:, :] = torch.arange(16 * 3, dtype=dtype).reshape(16, 3)       # the joint terms are not kept; any pose with distinct joints will do
    d = crit([{'theta': p.reshape(1, F, 82), 'kp_3d': kp + 0.5}], {'theta': gt.to(dtype).reshape(1, F, 82), 'kp_3d': kp})
    ls = (d['loss_pose'], d['loss_shape'], d['loss_norm'])
    sum(float(np.float32(l)) * v for l, v in zip(ME.LAMBDAS3, ls)).backward()
    return torch.stack([v.detach() for v in ls]), p.grad


def mint():
    U, L = import_reference_mesh()
    save = {}
    for M in ME.ROT_M:
        x6, drot, daa = ME.rot_inputs(M, ME.rot_seed(M))
        r64, r32 = ref_rot(U, x6, drot, daa, torch.float64), ref_rot(U, x6, drot, daa, torch.float32)
        mine = ME.rot_chain_grad(x6, drot, daa, torch.float64)
        rows = ME.fixture_rows(M, 9)
        save[f'rot.{M}.rows'] = rows.astype(np.int64)
        for name, a64, a32, b in zip(('rotmat', 'aa', 'dx6'), r64, r32, mine):
            assert ME.stat(b, a64) <= 1e-12, (M, name, ME.stat(b, a64))
            save[f'rot.{M}.{name}'] = a64.numpy()[rows]
            save[f'rot.{M}.{name}.ref32'] = np.asarray(ME.stat(a32, a64), dtype=np.float64)
        print(f'[rot {M}] ref32 ' + ' '.join('%s %.3g' % (n, float(save[f'rot.{M}.{n}.ref32'])) for n in ('rotmat', 'aa', 'dx6')))
    for F in ME.LOSS_F:
        pred, gt = ME.theta_inputs(F, ME.loss_seed(F))
        rows = ME.fixture_rows(F, 82)
        save[f'loss.{F}.rows'] = rows.astype(np.int64)
        for t in (0, 1):
            l64, d64 = ref_losses(L, pred, gt, t, torch.float64)
            l32, d32 = ref_losses(L, pred, gt, t, torch.float32)
            ml, md = ME.param_loss_grad(pred, gt, t, ME.LAMBDAS3, torch.float64)
            assert float(((ml - l64).abs() / l64.abs()).max()) <= 1e-12 and ME.stat(md, d64) <= 1e-12, (F, t)
            save[f'loss.{F}.t{t}.losses'] = l64.numpy()
            save[f'loss.{F}.t{t}.dtheta'] = d64.numpy()[rows]
            save[f'loss.{F}.t{t}.losses.ref32'] = ((l32.double() - l64).abs() / l64.abs()).numpy()
            save[f'loss.{F}.t{t}.dtheta.ref32'] = np.asarray(ME.stat(d32, d64), dtype=np.float64)
            print(f'[loss {F} type {t}] ' + ' '.join('%.9f' % float(v) for v in l64) + ' ref32 ' +
                  ' '.join('%.3g' % v for v in save[f'loss.{F}.t{t}.losses.ref32']) + ' dtheta %.3g' % float(save[f'loss.{F}.t{t}.dtheta.ref32']))
    for case in ME.ERR_CASES:
        F, V = case
        if V != 6890:
            continue
        vp, vg, kp, kg = [a.double() for a in ME.err_inputs(F, V, ME.err_seed(case))]
        out, tgt = [{'verts': vp, 'kp_3d': kp}], {'verts': vg, 'kp_3d': kg}
        mpjpes, mpves = U.compute_error_frames(out, tgt)
        p17, g17 = (kp - kp[:, :1]).numpy(), (kg - kg[:, :1]).numpy()
        idx = list(ME.H36M_17_TO_14)
        rows = np.empty((5, F))
        rows[0], rows[1] = mpves.numpy(), mpjpes.numpy()
        rows[2] = np.sqrt(np.square(p17[:, idx] - g17[:, idx]).sum(-1)).mean(-1)
        with np.errstate(divide='ignore', invalid='ignore'):
            for f in range(F):
                rows[3, f] = np.sqrt(np.square(U.rigid_align(p17[f], g17[f]) - g17[f]).sum(-1)).mean()
                rows[4, f] = np.sqrt(np.square(U.rigid_align(p17[f][idx], g17[f][idx]) - g17[f][idx]).sum(-1)).mean()
            d = U.evaluate_mesh({'verts': vp.numpy(), 'verts_gt': vg.numpy(), 'kp_3d': kp.numpy(), 'kp_3d_gt': kg.numpy()})
        mine = ME.mesh_errors64(vp.numpy(), vg.numpy(), kp.numpy(), kg.numpy())
        assert ME.err_ratio(mine, rows) <= 1e-12 / ME.GATE64, (case, ME.err_ratio(mine, rows) * ME.GATE64)
        dict_rows = np.asarray([d[k] for k in ME.ERR_ROWS], dtype=np.float64)
        assert ME.err_ratio(np.asarray([ME.aggregate(rows)[k] for k in ME.ERR_ROWS]), dict_rows) <= 1e-12 / ME.GATE64, case
        save['err.%d.%d.rows' % case] = rows
        save['err.%d.%d.dict' % case] = dict_rows
        print(f'[err {case}] ' + ' '.join('%s %.6f' % (k, v) for k, v in zip(ME.ERR_ROWS, dict_rows)))
    return save


def main():
    save = mint()
    if '--check' in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(save), (sorted(old.files), sorted(save))
        for k, v in save.items():
            assert old[k].dtype == np.asarray(v).dtype and old[k].tobytes() == np.asarray(v).tobytes(), k
        print('re-minted bit-identically:', OUT)
        return
    np.savez_compressed(OUT, **save)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
