#!/usr/bin/env python
"""Mint tests/golden/wild_mesh.npz with the REFERENCE's own `solve_scale` (infer_wild_mesh.py:42-56), read at run time from the checkout
oracle/make_golden.py names (MOTIONBERT_REFERENCE).

    python tools/mint_wild_mesh.py             # write the fixture (about a minute per problem: 400 least_squares starts each)
    python tools/mint_wild_mesh.py --check     # mint again and compare every array with the committed file, bit for bit

infer_wild_mesh.py cannot be imported: it parses arguments, loads a checkpoint and opens a video at import, and needs `imageio`.  The file
is therefore parsed with `ast`, and only the function definitions `err` and `solve_scale` are compiled, into a namespace that holds
`numpy`, scipy's `least_squares` and a `tqdm` stand-in.  Nothing of the reference's text is stored.  `solve_scale` returns only its best
scale and prints its best `fun`; the `least_squares` it calls is wrapped to record the lowest `fun` it returned.  Per problem of
wildmesherr.FIXTURE_PROBLEMS (seeded by tests/wildmesherr.fit_problem; the points as infer_wild_mesh.py:150-151 forms them):
    {name}.scale   float64: the reference's best_scale
    {name}.fun     float64: the fun of that start, the reference's ranking criterion
    {name}.points  int64: the number of points
Needs scipy; the tests do not."""
import ast
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden                             # noqa: E402
from tests import wildmesherr as WM                        # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'wild_mesh.npz')


def reference_solve_scale():
    """(solve_scale, record): the reference's function and the list its least_squares calls append (fun, x) to"""
    from scipy.optimize import least_squares
    with open(os.path.join(make_golden.REF, 'infer_wild_mesh.py')) as f:
        tree = ast.parse(f.read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ('err', 'solve_scale')]
    assert sorted(d.name for d in defs) == ['err', 'solve_scale']
    record = []

    def recording(*a, **k):
        est = least_squares(*a, **k)
        record.append((float(np.ravel(est['fun'])[0]), np.array(est['x'], dtype=np.float64)))
        return est
    ns = {'np': np, 'least_squares': recording, 'tqdm': lambda it, *a, **k: it}
    exec(compile(ast.Module(body=defs, type_ignores=[]), 'infer_wild_mesh.py', 'exec'), ns)
    return ns['solve_scale'], record


def mint():
    solve_scale, record = reference_solve_scale()
    save = {}
    for name in WM.FIXTURE_PROBLEMS:
        ref, kp = WM.fit_problem(name)
        x = ref - ref[:, :1]                               # infer_wild_mesh.py:150-151
        y = kp - kp[:, :1]
        del record[:]
        t0 = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            best_scale = solve_scale(x, y)
        funs = np.array([f for f, _ in record])
        assert len(record) == 400
        best = int(np.argmin(funs))                        # the first strict minimum, as the `<` of the loop keeps it
        assert record[best][1][0] == best_scale
        save[f'{name}.scale'] = np.float64(best_scale)
        save[f'{name}.fun'] = np.float64(funs[best])
        save[f'{name}.points'] = np.int64(x.shape[0] * x.shape[1])
        s, t, obj, it = WM.fit_ref(name)
        print(f'[{name}] {x.shape[0] * 17} points, {time.time() - t0:.0f} s: best scale {best_scale!r}, fun {funs[best]!r}, spread of the starts '
              f'{(funs.max() - funs.min()) / funs.min():.2e}; fit_ref scale {s!r}, objective {obj!r} ({(funs[best] - obj) / obj:.2e} below), '
              f'{it} iterations', flush=True)
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
