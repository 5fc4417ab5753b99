"""tests/wildmesherr.py on the CPU: the gates of in-the-wild mesh recovery pass on the clean CPU provider and fail on every seeded
corruption; the fixture conditions hold for fit_ref itself; the three library entries refuse bad arguments before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import wildmesherr as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def fixture():
    return WM.load_fixture()


@pytest.fixture(scope='module')
def case():
    return WM.mesh_case(65, 3, 3, 8500)


def test_constants_are_the_headers():
    src = open(os.path.join(ROOT, 'include', 'mbx.h')).read()
    got = {k: float(v) for k, v in re.findall(r'#define MBX_SCALE_FIT_(DELTA|TOL|CAP) (\S+)', src)}
    assert got == {'DELTA': WM.DELTA, 'TOL': WM.TOL, 'CAP': float(WM.CAP)}
    assert WM.CORRUPTIONS == WM.MESH_CORRUPTIONS + WM.FIT_CORRUPTIONS + WM.PLACE_CORRUPTIONS and len(WM.CORRUPTIONS) == 10


def test_problems_are_what_their_names_say():
    for name, on in WM.ON_KINK.items():
        x, y = WM.points(*WM.fit_problem(name))
        s, t, obj, it = WM.fit_ref(name)
        assert len(x) == int(name[1:])
        assert (np.abs(t).max() <= 1e-9 * np.abs(y).max()) == on, (name, t)
    x, y = WM.points(*WM.fit_problem('exact'))
    assert np.array_equal(y, 2.0 * x) and WM.fit_ref('exact')[:1] == (2.0,) and WM.fit_ref('exact')[2] == 0.0
    assert [0 if n is None else len(WM.fit_problem(n)[0]) for n in WM.POOL] == [1, 0, 20, 70] and len(WM.fit_problem(WM.LARGE)[0]) == 1025


def test_fit_ref_meets_the_fixture_conditions(fixture):
    """(a) and (b) for the float64 reference fit itself: below the reference's own best on every minted problem, and the production
    stopping rule (1e-13, in numpy) within the 1e-10 gate of it"""
    assert sorted(fixture.files) == sorted(f'{n}.{k}' for n in WM.FIXTURE_PROBLEMS for k in ('scale', 'fun', 'points'))
    for name in WM.FIXTURE_PROBLEMS:
        s, t, obj, it = WM.fit_ref(name)
        res = WM.fit_check(np.array([s, *t, obj, it], dtype=np.float64), name, fixture)
        assert res['b'] == 0.0 and res['a'] <= 1.0, (name, res)
        assert int(fixture[f'{name}.points']) == 17 * len(WM.fit_problem(name)[0])
    for name in WM.PROBLEMS:
        res = WM.fit_check(WM.fit_row(*WM.fit_problem(name)), name, fixture)
        assert WM.fit_passes(res) and res['b'] <= 0.1 and 1 <= res['iterations'] <= 500, (name, res)
    # two summation orders of the same iteration: far inside the gate
    ref, kp = WM.fit_problem('p1020')
    a, b = WM.fit_row(ref, kp), WM.fit_row(ref[::-1].copy(), kp[::-1].copy())
    assert abs(a[0] - b[0]) / a[0] <= 1e-13


def test_clean_provider_passes_every_gate(fixture, case):
    ops = WM.WildMeshOps()
    report = {}
    assert WM.mesh_gate_run(ops, CPU, case, report) == []
    assert set(report) == {'pair.verts', 'pair.kp', 'pair.verts.verts'}      # the single-pass and theta gates are bit equality
    assert all(0 < v <= 1.0 for v in report.values()), report
    assert WM.fit_gate_run(ops, CPU, fixture, WM.PROBLEMS + (WM.LARGE,)) == []
    assert WM.place_gate_run(ops, CPU) == 0


@pytest.mark.parametrize('corrupt', WM.CORRUPTIONS)
def test_every_corruption_fails_a_gate(corrupt, fixture, case):
    ops = WM.WildMeshOps(corrupt)
    if corrupt in WM.MESH_CORRUPTIONS:
        failed = WM.mesh_gate_run(ops, CPU, case)
        assert failed and any(f.startswith('pair') for f in failed), failed
        if corrupt == 'kp_before_scale':
            assert 'pair.kp' in failed and 'pair.verts' not in failed
        assert WM.place_gate_run(ops, CPU) == 0
    elif corrupt in WM.FIT_CORRUPTIONS:
        failed = WM.fit_gate_run(ops, CPU, fixture)
        assert failed, corrupt
        if corrupt == 'irls_no_floor':
            assert 'fit.exact' in failed
        assert WM.mesh_gate_run(ops, CPU, case) == []
    else:
        assert WM.place_gate_run(ops, CPU) > 0
        assert WM.fit_gate_run(ops, CPU, fixture, ('p17',)) == []


def test_gate_inputs_come_from_the_reference_alone(case):
    """the pair gate is computed from the plain path in two precisions: the same numbers whatever provider is under test"""
    a, b = WM.pair_gates(case['model'], case)[1], WM.pair_gates(case['model'], case)[1]
    assert a == b and all(v >= WM.SE.FLOOR for v in a.values())


# ------------------------------------------------------------------------------------------------ the library's refusals (no launch)
@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_library_refusals_are_reported_not_crashed(lib):
    assert lib.mbx_version() >= 160
    p = C.c_void_p(4096)            # never dereferenced: every check below fails before a launch
    parents = (C.c_int * 24)(-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
    ws = C.c_void_p(4096)

    def mesh(K=17, n=2, T=3, F=6, dst_max=3, V=65, Q=p, theta_a=p, theta_b=p, verts=p, kp=p, theta=p, par=parents, ws_bytes=1 << 40, rot=p):
        return lib.mbx_wild_mesh(p, p, p, p, p, par, p, Q, K, rot, p, theta_a, theta_b, 1000.0, p, dst_max, n, T, F, verts, kp, theta, V, ws, ws_bytes, None)

    def err():
        return lib.mbx_last_error().decode()
    assert mesh(n=0) == 0                                                     # nT = 0: a no-op
    assert mesh(dst_max=4) != 0 and 'does not fit' in err()
    assert mesh(dst_max=-1) != 0 and 'does not fit' in err()
    assert mesh(V=0) != 0 and 'bad sizes' in err()
    assert mesh(K=33) != 0 and 'bad sizes' in err()
    assert mesh(T=0) != 0 and 'bad sizes' in err()
    assert mesh(n=1 << 18, T=3, F=1 << 20, dst_max=0) != 0 and 'bad sizes' in err()        # 2 n T > 2^20 with pass B
    bad = (C.c_int * 24)(*([-1] + [23] * 23))
    assert mesh(par=bad) != 0 and 'forward-ordered' in err()
    assert mesh(ws_bytes=64) != 0 and 'workspace' in err()
    assert mesh(verts=None, kp=None, theta=None) != 0 and 'no output' in err()
    assert mesh(theta_a=None) != 0 and 'theta_a' in err()
    assert mesh(Q=None) != 0 and 'regressor' in err()
    assert mesh(rot=None) != 0 and 'null' in err()
    need1, need2 = lib.mbx_wild_mesh_ws(6, 65, 17, 0), lib.mbx_wild_mesh_ws(6, 65, 17, 1)
    assert need1 == lib.mbx_smpl_fwd_ws(6, 65, 17) and need2 > lib.mbx_smpl_fwd_ws(12, 65, 17) and lib.mbx_wild_mesh_ws(0, 65, 17, 1) == 0
    assert lib.mbx_scale_fit(p, p, p, 0, 5, p, None) == 0                     # no tracks: a no-op
    assert lib.mbx_scale_fit(p, p, p, -1, 5, p, None) != 0 and 'bad sizes' in err()
    assert lib.mbx_scale_fit(p, p, None, 1, 5, p, None) != 0 and 'null' in err()
    assert lib.mbx_scale_fit(C.c_void_p(4100), p, p, 1, 5, p, None) != 0 and 'aligned' in err()
    assert lib.mbx_wild_mesh_place(p, p, 17, p, p, 1, p, 0, 65, None) == 0    # no frames: a no-op
    assert lib.mbx_wild_mesh_place(p, p, 0, p, p, 1, p, 5, 65, None) != 0 and 'bad sizes' in err()
    assert lib.mbx_wild_mesh_place(None, p, 17, p, p, 1, p, 5, 65, None) != 0 and 'null' in err()


def test_binding_refuses_wrong_layouts_before_the_library_is_called():
    from motionbert_amd import hip_ops

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f'the library was called ({name})')
    ops = hip_ops.HipOps(lib=NoLib())
    case = WM.mesh_case(7, 2, 3, 8501)
    model = case['model'].tensors()
    Q = case['model'].J_regressor_h36m
    dst = torch.from_numpy(case['dst'])
    rot, betas, th = case['rot_a'].reshape(-1, 24, 9), case['betas_a'], case['theta_a']
    verts, kp = torch.empty(case['F'], 7, 3), torch.empty(case['F'], 17, 3)
    with pytest.raises(RuntimeError, match='clips of'):
        ops.wild_mesh(model, Q, rot, betas, None, None, 1000.0, dst, int(dst.max()), 2, verts, kp, None)
    with pytest.raises(RuntimeError, match='does not fit'):
        ops.wild_mesh(model, Q, rot, betas, None, None, 1000.0, dst, case['F'] - 2, 3, verts, kp, None)
    with pytest.raises(RuntimeError, match='theta_a'):
        ops.wild_mesh(model, Q, rot, betas, None, th, 1000.0, dst, int(dst.max()), 3, verts, kp, torch.empty(case['F'], 82))
    with pytest.raises(RuntimeError, match='dst_frames must be a contiguous torch.int32'):
        ops.wild_mesh(model, Q, rot, betas, None, None, 1000.0, dst.long(), int(dst.max()), 3, verts, kp, None)
    with pytest.raises(RuntimeError, match='verts must be a contiguous'):
        ops.wild_mesh(model, Q, rot, betas, None, None, 1000.0, dst, int(dst.max()), 3, verts.double(), kp, None)
    ref, k32 = torch.zeros(5, 17, 3, dtype=torch.float64), torch.zeros(5, 17, 3)
    ptr, fit = torch.tensor([0, 5], dtype=torch.int32), torch.zeros(1, 6, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='ref must be a contiguous torch.float64'):
        ops.scale_fit(ref.float(), k32, ptr, fit)
    with pytest.raises(RuntimeError, match=r'fit \[S,6\]'):
        ops.scale_fit(ref, k32, ptr, torch.zeros(2, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='needs verts'):
        ops.wild_mesh_place(torch.zeros(5, 7, 3), k32, ref[:4], ptr, fit)
    with pytest.raises(RuntimeError, match='fit must be a contiguous torch.float64'):
        ops.wild_mesh_place(torch.zeros(5, 7, 3), k32, ref, ptr, fit.float())
