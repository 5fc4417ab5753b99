"""The reference of the crowd rasteriser and its gates on the CPU (tests/sceneerr.py): every seeded corruption of a convention fails a gate, the
two reductions to the single-skeleton reference hold, and the crafted scene holds what its description says."""
import numpy as np
import pytest

from motionbert_amd import render as R
from tests import sceneerr as SC
from tests import skelerr as SE

W, H, SS = 72, 40, 2
RASTER_CORRUPTIONS = SC.CORRUPTIONS[:10]


@pytest.fixture(scope='module')
def scene():
    case = SC.crafted_case(W, H, SS, counts=(0, 1, 13, SC.CHUNK + 1))
    case['background'] = SC.backdrop(4, W, H, seed=3)
    case['ref'] = SC.raster(case['jq'], case['table'], case['bones'], case['palette'], case['radii'], W, H, SS, case['background'])
    return case


def _raster(case, **kw):
    args = dict(jq=case['jq'], table=case['table'], bones=case['bones'], palette=case['palette'], radii=case['radii'], W=W, H=H, ss=SS,
                background=case['background'])
    args.update(kw)
    return SC.raster(**args)


def test_the_crafted_scene_holds_its_cases(scene):
    ref, (ptr, rows, person), n0, np_ = scene['ref'], scene['table'], scene['R'] - 6, 3 * len(SC.BONES5)
    assert ptr.tolist() == [0, 0, 1, 14, SC.CHUNK + 15] and (ref['prim_id'][0] == -1).all()
    assert np.array_equal(ref['rgb'][0], scene['background'][0]) and not np.array_equal(ref['rgb'][1], scene['background'][1])
    seen = [set((np.unique(ref['prim_id'][f][ref['prim_id'][f] >= 0]) // np_).tolist()) for f in range(4)]
    lists = [rows[ptr[f]:ptr[f + 1]].tolist() for f in range(4)]
    for f in (2, 3):
        rank = {r: lists[f].index(r) for r in (n0, n0 + 1, n0 + 2, n0 + 3, n0 + 4, n0 + 5)}
        assert rank[n0] not in seen[f]                                        # wholly outside
        assert {rank[n0 + 1], rank[n0 + 2], rank[n0 + 5]} <= seen[f]         # the corner, the one with sentinel joints, the touching marker
        assert rank[n0 + 4] in seen[f] and rank[n0 + 3] not in seen[f]       # twins: the later rank wins everywhere
        assert not {k for k, r in enumerate(lists[f]) if not 0 <= r < scene['R']} & seen[f]
        bad_person = [k for k, q in enumerate(person[ptr[f]:ptr[f + 1]].tolist()) if not 0 <= q < scene['P']]
        assert len(bad_person) == 2 and not set(bad_person) & seen[f]        # a drawn row with a palette row that does not exist
    # the corner person lies in four tiles; the person with sentinel joints has lost the bones at joints 1 and 8
    i, j = np.nonzero(ref['prim_id'][2] // np_ == lists[2].index(n0 + 1))
    assert len({(a // 32, b // 32) for a, b in zip(i, j)}) == 4
    prims = np.unique(ref['prim_id'][2][ref['prim_id'][2] // np_ == lists[2].index(n0 + 2)] % np_ // 3)
    assert prims.tolist() == [0]                                             # BONES5: only (0, 7) touches neither joint 1 nor joint 8
    # the touching marker: its leftmost covered sample is the last one of tile column 0
    i, j = np.nonzero(ref['prim_id'][2] // np_ == lists[2].index(n0 + 5))
    assert j.min() == 31 and (j == 31).sum() == 1


@pytest.mark.parametrize('name', RASTER_CORRUPTIONS)
def test_every_raster_corruption_fails_a_gate(scene, name):
    assert len(RASTER_CORRUPTIONS) >= 10
    assert SC.gate_all(_raster(scene, corrupt=(name,)), scene['ref'])


def test_the_gates_pass_the_reference_and_see_one_element(scene):
    again = _raster(scene)
    assert SC.gate_all(again, scene['ref']) == []
    again['rgb'][3, H - 1, W - 1, 2] ^= 1
    assert SC.gate_all(again, scene['ref']) == ['rgb: 1 of %d elements differ' % again['rgb'].size]


def test_projection_and_its_corruptions():
    x = np.array([[[0, 0, 9], [1.25, -1.25, 0], [17.03125, 39.96875, 0], [-0.015625, 3.046875, 0], [np.nan, 1, 0], [1, np.inf, 0], [3, 4, np.nan],
                   [8192.0, 0, 0], [8192.0625, 0, 0], [-8192.0, 5, 0], [1e30, 0, 0]]], np.float32)
    assert SC.project(x, 1)[0].tolist() == [[0, 0], [20, -20], [273, 640], [0, 49]] + [[SC.OUTSIDE] * 2] * 2 + [[48, 64], [1 << 17, 0]] + \
        [[(1 << 17) + 1, 0], [-(1 << 17), 80], [SC.OUTSIDE] * 2]
    q2 = SC.project(x, 2)
    assert q2[0, 7].tolist() == [1 << 18, 0] and q2[0, 8].tolist() == [SC.OUTSIDE] * 2 and q2[0, 3].tolist() == [0, 98]
    assert np.array_equal(SC.project(x[..., :2], 2), q2)                      # z is not used
    for name in ('no_half', 'truncated'):
        assert SC.gate_equal('jq', SC.project(x, 1, (name,)), SC.project(x, 1)), name
    # numpy float64 in this order is what the header states: the product is exact, so a fused multiply-add gives the same bits
    g = np.random.default_rng(0)
    y = g.uniform(-100, 2100, (50, 17, 2)).astype(np.float32)
    assert np.array_equal(SC.project(y, 2)[..., 0], np.floor(np.array([[float(v) * 32 + 0.5 for v in r] for r in y[..., 0]])).astype(np.int32))


@pytest.mark.parametrize('ss', [1, 2])
def test_reduction_a_one_person_per_frame_is_the_skeleton_raster(ss):
    size = 72
    jq = SE.project(SE.walking(3, seed=4), R.SKELETON_VIEW, size * ss)
    radii = tuple(ss * r for r in R.skeleton_radii(256))
    assert SC.reduction_a(SC.raster, jq, np.array(R.SKELETON_BONES, np.int32), np.array(R.SKELETON_COLORS, np.uint8), radii, size, ss) == []
    for name in ('tile_corner', 'sentinel', 'guard', 'order', 'stack'):
        jq, bones, colors, radii = SE.crafted_cases(size, ss)[name]
        assert SC.reduction_a(SC.raster, jq, bones, colors, radii, size, ss) == [], name
    # and the gate of the reduction sees a wrong convention
    assert SC.reduction_a(lambda *a: SC.raster(*a[:8], (254, 255, 255)), jq, bones, colors, radii, size, ss)
    assert SC.reduction_a(lambda *a: SC.raster(*a, corrupt=('first_wins',)), jq, bones, colors, radii, size, ss) == []      # one person: no order


@pytest.mark.parametrize('ss', [1, 2])
def test_reduction_b_a_crowd_is_its_persons_painted_in_order(ss):
    case = SC.crafted_case(40, 72, ss, counts=(2, 0, SC.CHUNK + 1))
    args = (case['jq'], case['table'], case['bones'], case['palette'], case['radii'], 40, 72, ss)
    for bg in ((10, 200, 30), SC.backdrop(1, 40, 72), SC.backdrop(3, 40, 72, seed=1)):
        whole = SC.raster(*args, bg)
        assert (whole['prim_id'] >= 0).mean() > 0.1
        assert SC.reduction_b(whole, *args, bg) == []
    for name in ('rank_ignored', 'first_wins', 'ss_mean_white', 'palette_wrong_person', 'chunk_second_dropped'):
        bad = SC.raster(*args, bg, corrupt=(name,))
        assert SC.reduction_b(bad, *args, bg) or (name == 'ss_mean_white' and ss == 1), name


def test_one_palette_row_is_everybody(scene):
    one = _raster(scene, palette=scene['palette'][:1])
    # prim_id changes only where an entry named a palette row that does not exist: with one row the person is not looked at
    assert (one['prim_id'] >= 0).sum() >= (scene['ref']['prim_id'] >= 0).sum()
    colours = {tuple(v) for v in scene['palette'][0].tolist()} | {(255, 255, 255)}
    flat = SC.raster(scene['jq'], scene['table'], scene['bones'], scene['palette'][:1], scene['radii'], 2 * W, 2 * H, 1, (0, 0, 0))
    assert np.array_equal(flat['prim_id'], one['prim_id']) and {tuple(v) for v in flat['rgb'][flat['prim_id'] >= 0].tolist()} <= colours
