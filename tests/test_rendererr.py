"""The host reference of the mesh rasteriser (tests/rendererr.py) checked on its own, on the CPU: properties that hold whatever edge
convention was chosen, and seeded corruptions that each fail a gate."""
import numpy as np
import pytest

from tests import rendererr as RE

SIZE = 72


def _raster(vq, faces, size=SIZE, ss=1, **kw):
    return RE.raster(vq, RE.verts_from_vq(vq, size * ss), faces, size, ss, **kw)


# ------------------------------------------------------------------------------------------------ properties
def test_split_quads_cover_every_sample_once():
    for vq, faces, rect in RE.property_quads():
        count = np.zeros((32, 32), np.int64)
        for n in range(len(faces)):
            count += _raster(vq, faces[n:n + 1], size=32)['face_id'][0] >= 0
        assert count.max() == 1, 'a sample belongs to two faces'
        both = _raster(vq, faces, size=32)['face_id'][0] >= 0
        assert np.array_equal(both, count == 1)
        if rect is not None:              # corners on sample centres: the quad covers its samples up to the edges the rule does not own
            x0, y0, x1, y1 = rect
            assert both[y0 + 1:y1, x0 + 1:x1].all() and not both[:y0].any() and not both[y1 + 1:].any()
            assert both.sum() in ((x1 - x0) * (y1 - y0), (x1 - x0 + 1) * (y1 - y0 + 1), (x1 - x0) * (y1 - y0 + 1), (x1 - x0 + 1) * (y1 - y0))


def test_an_axis_aligned_quad_owns_two_of_its_four_sides():
    vq, faces, rect = RE.property_quads()[0]
    x0, y0, x1, y1 = rect
    cov = _raster(vq, faces, size=32)['face_id'][0] >= 0
    assert cov.sum() == (x1 - x0) * (y1 - y0)              # each side is owned by the quad or by its neighbour, never both


def test_winding_changes_nothing():
    cases = RE.crafted_cases(SIZE)
    for name in ('quads', 'corners', 'stack'):
        vq, faces = cases[name]
        faces = faces[:200]
        ref = _raster(vq, faces)
        for perm in ([0, 2, 1], [1, 0, 2], [2, 1, 0], [1, 2, 0]):
            alt = _raster(vq, np.ascontiguousarray(faces[:, perm]))
            for k in ('face_id', 'depth', 'rgb'):
                assert np.array_equal(ref[k], alt[k]), (name, perm, k)


def test_whole_sample_shifts_shift_the_buffers():
    vq, faces = RE.crafted_cases(SIZE)['corners']
    ref = _raster(vq, faces)
    for dj, di in ((3, 0), (0, 5), (7, 2)):
        moved = vq.copy()
        moved[..., 0] += RE.SUB * dj
        moved[..., 1] += RE.SUB * di
        alt = RE.raster(moved, RE.verts_from_vq(vq, SIZE), faces, SIZE, 1)
        for k, empty in (('face_id', -1), ('depth', 0x7fffffff)):
            want = np.full_like(ref[k], empty)
            want[:, di:, dj:] = ref[k][:, :SIZE - di, :SIZE - dj]
            assert np.array_equal(alt[k], want), (dj, di, k)


def test_coplanar_copies_resolve_to_the_lower_index():
    vq, faces = RE.crafted_cases(SIZE)['quads']
    one = _raster(vq, faces[:1])
    for twice in (np.stack([faces[0], faces[0]]), np.stack([faces[0], faces[0][[2, 1, 0]]])):
        two = _raster(vq, twice)
        assert np.array_equal(two['face_id'], one['face_id']) and np.array_equal(two['depth'], one['depth'])
        assert (two['face_id'] == 0).any() and not (two['face_id'] == 1).any()


def test_depth_is_the_floor_of_the_plane_and_nearer_wins():
    vq, faces = RE.crafted_cases(SIZE)['corners']
    r = _raster(vq, faces)
    near = _raster(vq, faces[-2:])
    a, b = _raster(vq, faces[-2:-1]), _raster(vq, faces[-1:])
    both = (a['face_id'] >= 0) & (b['face_id'] >= 0)
    assert both.any() and np.array_equal(near['depth'][both], np.minimum(a['depth'], b['depth'])[both])
    assert (near['face_id'][both] == 0).any() and (near['face_id'][both] == 1).any()           # the two faces interpenetrate
    assert r['depth'][r['face_id'] >= 0].min() >= 0 and r['depth'][r['face_id'] >= 0].max() <= RE.ZQ


def test_dropped_faces():
    vq, faces = RE.crafted_cases(SIZE)['dropped']
    r = _raster(vq, faces)
    assert sorted(np.unique(r['face_id'][0])) == [-1, 0, 11]        # the drawn face, its reversed copy (12) loses the tie; face 11
    assert (r['face_id'][1] == -1).all() and (r['depth'][1] == 0x7fffffff).all() and (r['rgb'][1] == 255).all()


def test_projection_reference():
    g = np.random.default_rng(0)
    v = g.standard_normal((3, 50, 3)).astype(np.float32)
    v[1, 7, 0] = np.nan
    v[1, 8, 2] = np.inf
    v[2, 9, 1] = 1e30
    cube = np.array([[0, 0, 0, 0.1], [1, 1, 1, 0.05]], np.float32)
    q = RE.project(v, cube, [0, 2, 3], 144)
    assert q.dtype == np.int32 and (q[1, 7, 0], q[1, 8, 2], q[2, 9, 1]) == (RE.OUTSIDE,) * 3
    x = np.float64(v[0, 0, 0])
    assert q[0, 0, 0] == int(np.floor(np.float32(np.float32(np.float32(x * np.float32(0.1)) + np.float32(0.5)) * np.float32(144 * 16))))
    assert q[2, 0, 2] == int(np.floor(((np.float32(v[2, 0, 2]) - np.float32(1)) * np.float32(0.05) + np.float32(0.5)) * np.float32(RE.ZQ)))
    assert (RE.project(v, cube[:1], [0, 2], 144)[2] == RE.OUTSIDE).all()              # a frame outside every track


# ------------------------------------------------------------------------------------------------ seeded corruptions
@pytest.fixture(scope='module')
def scene():
    """one float-level scene (the deformed icosphere, two tracks) and the integer-level cases, with their references"""
    verts, faces = RE.deformed_icosphere(3, seed=1)
    lo, hi = verts[:2].reshape(-1, 3).min(0), verts[:2].reshape(-1, 3).max(0)
    lo2, hi2 = verts[2].min(0), verts[2].max(0)
    cube = np.array([np.append((hi + lo) / 2, 1 / (hi - lo).max()), np.append((hi2 + lo2) / 2, 1 / (hi2 - lo2).max())], np.float32)
    cloud = np.random.default_rng(3).standard_normal((1, 4096, 3)).astype(np.float32)      # enough vertices for the last bit of a product to matter
    return dict(verts=verts, faces=faces, cube=cube, ptr=[0, 2, 3], cases=RE.crafted_cases(SIZE), cloud=cloud,
                cloud_cube=np.array([[0.01, -0.02, 0.03, 0.11]], np.float32))


def _run(scene, ss, corrupt):
    """every gate over the scene and the crafted cases with the corruption in the producer: the list of failures"""
    S = SIZE * ss
    ref_q = RE.project(scene['verts'], scene['cube'], scene['ptr'], S)
    got_q = RE.project(scene['verts'], scene['cube'], scene['ptr'], S, corrupt)
    failed = RE.gate_equal('vq', got_q, ref_q)
    failed += RE.gate_equal('vq (cloud)', RE.project(scene['cloud'], scene['cloud_cube'], [0, 1], S, corrupt), RE.project(scene['cloud'], scene['cloud_cube'], [0, 1], S))
    ref = RE.raster(ref_q, scene['verts'], scene['faces'], SIZE, ss)
    failed += RE.gate_all(RE.raster(got_q, scene['verts'], scene['faces'], SIZE, ss, corrupt=corrupt), ref, ss)
    for name, (vq, faces) in scene['cases'].items():
        v = RE.verts_from_vq(vq, S)
        failed += [f'{name}: {m}' for m in RE.gate_all(RE.raster(vq, v, faces, SIZE, ss, corrupt=corrupt), RE.raster(vq, v, faces, SIZE, ss), ss)]
    return failed


def test_the_reference_passes_its_own_gates(scene):
    assert _run(scene, 1, ()) == [] and _run(scene, 2, ()) == []


@pytest.mark.parametrize('corrupt', RE.CORRUPTIONS)
def test_seeded_corruption_fails_a_gate(scene, corrupt):
    assert len(RE.CORRUPTIONS) >= 10
    failed = _run(scene, 2 if corrupt == 'ss_no_round' else 1, (corrupt,))
    assert failed, f'{corrupt} passes every gate'


def test_rgb_gate_allows_one_level_only_next_to_a_half(scene):
    vq, faces = scene['cases']['corners']
    v = RE.verts_from_vq(vq, SIZE)
    ref = RE.raster(vq, v, faces, SIZE, 1)
    lo, hi = RE.sample_interval(ref)
    assert (hi - lo).max() <= 1 and ((lo == hi).mean() > 0.99)
    off = ref['rgb'].copy()
    i = np.argwhere(ref['face_id'] >= 0)[0]
    off[i[0], i[1], i[2], 0] += 1 if lo[i[0], i[1], i[2], 0] == hi[i[0], i[1], i[2], 0] else 2
    assert RE.gate_rgb(off, ref, 1)
    bg = ref['rgb'].copy()
    j = np.argwhere(ref['face_id'] < 0)[0]
    bg[j[0], j[1], j[2], 1] = 254
    assert any('background' in m for m in RE.gate_rgb(bg, ref, 1))
