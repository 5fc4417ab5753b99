#!/usr/bin/env python
"""Mint tests/golden/smpl_flip.npz with the REFERENCE's own `flip_thetas_batch` (lib/utils/utils_mesh.py:486-513, imported read-only at run
time as tools/mint_mesh.py imports it).

    python tools/mint_smpl_flip.py             # write the fixture
    python tools/mint_smpl_flip.py --check     # mint again and compare every array with the committed file, bit for bit

  in.{i} / out.{i}     thetas [N,F,72] fp32 (fp64 for the last case) and the reference's flipped thetas, for the shapes CASES; seeded inputs with
                       planted zeros (the sign of a negated zero is part of the bits)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mint_mesh import import_reference_mesh          # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'smpl_flip.npz')
CASES = ((1, 1, torch.float32), (2, 3, torch.float32), (3, 5, torch.float64))


def mint():
    U, _ = import_reference_mesh()
    save = {}
    for i, (N, F, dtype) in enumerate(CASES):
        g = torch.Generator().manual_seed(900 + i)
        x = (0.8 * torch.randn(N, F, 72, generator=g)).to(dtype)
        x[torch.rand(N, F, 72, generator=g) < 0.1] = 0.0
        y = U.flip_thetas_batch(x.clone())
        assert y.shape == x.shape and y.dtype == x.dtype
        save[f'in.{i}'], save[f'out.{i}'] = x.numpy(), y.numpy()
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
