#!/usr/bin/env python
"""Mint tests/golden/supcon.npz with the REFERENCE's own lib/model/loss_supcon.py (imported read-only at run time from the checkout
oracle/make_golden.py names: MOTIONBERT_REFERENCE) and, for the evaluation, with plain torch (train_action_1shot.py itself needs
tensorboardX and pytorch_metric_learning and cannot be imported).  Everything in float64.

    python tools/mint_supcon.py             # write the fixture
    python tools/mint_supcon.py --check     # mint again and compare every array with the committed file, bit for bit

Inputs come from the seeded makers of tests/supconerr.py and are not stored.  Per case (bsz, n_views, D) of supconerr.GPU_SHAPES and
normalize n in (0, 1), at temperature f32(0.1) and the class's default base temperature f32(0.07):
    sc.{bsz}.{n_views}.{D}.labels, sc.{...}.n{n}.loss, sc.{...}.n{n}.dfeat (autograd, with respect to the rows before F.normalize when n = 1)
A case of more than 16384 elements -- (32, 1, 2048) and (128, 1, 4096) -- keeps the gradient of its first and last four anchor rows only
(sc.{...}.rows names them), for both n: all rows of both would take the file past the size a committed fixture may have.
Per case (M, N, D) of supconerr.NN_SHAPES: nn.{M}.{N}.{D}.argmax = argmax(F.cosine_similarity(anchors[:, None], test[None], dim=-1), dim=0) and
nn.{...}.acc = mean(anchor_labels[argmax] == test_labels)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden                             # noqa: E402
from tests import supconerr as SC                          # noqa: E402

TAU, TAU_B = SC.FIXTURE_TAUS
OUT = os.path.join(ROOT, 'tests/golden', 'supcon.npz')


def import_reference_supcon():
    spec = importlib.util.spec_from_file_location('ref_lib_model_loss_supcon', os.path.join(make_golden.REF, 'lib/model/loss_supcon.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mint():
    L = import_reference_supcon()
    crit = L.SupConLoss(temperature=SC.f32(TAU), base_temperature=SC.f32(TAU_B))
    save = {'tau': np.asarray([SC.f32(TAU), SC.f32(TAU_B)], dtype=np.float64)}
    for shape in SC.GPU_SHAPES:
        bsz, nv, D = shape
        feat, lab = SC.supcon_inputs(bsz, nv, D, SC.case_seed(shape))
        tag = 'sc.%d.%d.%d' % shape
        rows = SC.fixture_rows(bsz * nv, D).numpy()
        save[tag + '.labels'] = lab.numpy().astype(np.int64)
        save[tag + '.rows'] = rows.astype(np.int64)
        for n in (0, 1):
            z = feat.double().requires_grad_(True)
            x = torch.nn.functional.normalize(z, dim=-1) if n else z
            loss = crit(x, lab)
            loss.backward()
            save[f'{tag}.n{n}.loss'] = np.asarray(float(loss.detach()), dtype=np.float64)
            save[f'{tag}.n{n}.dfeat'] = z.grad.reshape(bsz * nv, D).numpy()[rows]
            print(f'[supcon {shape} normalize={n}] loss {float(loss):.9f}')
    for shape in SC.NN_SHAPES:
        M, N, D = shape
        a, al, t, tl = SC.nn_inputs(M, N, D, SC.case_seed(shape), SC.NN_NOISE[shape])
        idx = torch.cat([torch.argmax(torch.nn.functional.cosine_similarity(a.double().unsqueeze(1), t[n:n + 256].double().unsqueeze(0), dim=-1), dim=0)
                         for n in range(0, N, 256)])
        acc = float((al[idx] == tl).double().mean())
        save['nn.%d.%d.%d.argmax' % shape] = idx.numpy().astype(np.int32)
        save['nn.%d.%d.%d.acc' % shape] = np.asarray(acc, dtype=np.float64)
        print(f'[nn {shape}] accuracy {acc:.6f}')
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
