"""The host reference of the skeleton rasteriser (tests/skelerr.py) checked on its own, on the CPU: properties that hold under any convention,
counted in Python integers, and the seeded corruptions, each of which must fail a gate."""
import numpy as np
import pytest

from motionbert_amd import render as R
from tests import skelerr as SE

SIZE = 72
ONE = np.array([[0, 1]], np.int32)
BLUE = np.array([[10, 20, 200]], np.uint8)
c = SE.c


def cover(jq, radii, bones=ONE, size=SIZE, ss=1):
    colors = np.tile(BLUE, (len(bones), 1))
    return SE.raster(np.asarray(jq, np.int32), bones, colors, radii, size, ss)['prim_id'] >= 0


def samples(S=SIZE):
    return [(SE.SUB * j + 8, SE.SUB * i + 8, i, j) for i in range(S) for j in range(S)]


# ------------------------------------------------------------------------------------------------ properties
def test_swapping_the_ends_changes_no_coverage():
    g = np.random.default_rng(0)
    for _ in range(5):
        jq = g.integers(-200, SIZE * 16 + 200, (1, 2, 2))
        radii = (int(g.integers(0, 80)), int(g.integers(40, 90)), int(g.integers(0, 40)))
        assert np.array_equal(cover(jq, radii), cover(jq[:, ::-1], radii))


def test_a_whole_sample_shift_shifts_the_buffers():
    jq = np.array([[[c(20) + 3, c(25) - 5], [c(40) - 7, c(33) + 2]]], np.int32)
    radii = (37, 55, 21)
    base = SE.raster(jq, ONE, BLUE, radii, SIZE, 1)
    for dx, dy in ((5, 0), (0, -7), (-11, 13)):
        moved = SE.raster(jq + np.array([16 * dx, 16 * dy], np.int32), ONE, BLUE, radii, SIZE, 1)
        for k in ('prim_id', 'rgb'):
            assert np.array_equal(np.roll(base[k], (dy, dx), axis=(1, 2)), moved[k]), (dx, dy, k)      # nothing is near the border: the roll wraps background


def test_coverage_grows_with_the_radius():
    jq = np.array([[[c(15) + 5, c(50) - 3], [c(55) + 1, c(20) + 7]]], np.int32)
    last = cover(jq, (0, 0, 0))
    for r in (1, 7, 16, 33, 90, 200):
        now = cover(jq, (r, r, 0))
        assert (now | ~last).all() and now.sum() > last.sum()
        last = now


def test_a_disc_holds_the_samples_counted_one_by_one():
    for cx, cy, r in ((c(30), c(30), 5 * 16), (c(30) + 5, c(41) - 3, 77), (c(2), c(70), 100), (c(36), c(36), 0), (c(36) + 1, c(36), 0)):
        count = sum(1 for x, y, _, _ in samples() if (x - cx) ** 2 + (y - cy) ** 2 <= r * r)
        assert cover([[[cx, cy], [cx, cy]]], (r, 0, 0)).sum() == count, (cx, cy, r)
    assert cover([[[c(30), c(30)], [c(30), c(30)]]], (5 * 16, 0, 0)).sum() > 60 and cover([[[c(36) + 1, c(36)], [c(36) + 1, c(36)]]], (0, 0, 0)).sum() == 0


def test_a_capsule_is_its_two_discs_and_its_rectangle():
    g = np.random.default_rng(1)
    for n in range(6):
        (ax, ay), (bx, by) = g.integers(-100, SIZE * 16 + 100, (2, 2)).tolist()
        r = int(g.integers(0, 120))
        dx, dy = bx - ax, by - ay
        dd = dx * dx + dy * dy
        want = np.zeros((SIZE, SIZE), bool)
        for x, y, i, j in samples():
            t = (x - ax) * dx + (y - ay) * dy
            cross = (x - ax) * dy - (y - ay) * dx
            rect = 0 <= t <= dd and cross * cross <= r * r * dd
            want[i, j] = rect or (x - ax) ** 2 + (y - ay) ** 2 <= r * r or (x - bx) ** 2 + (y - by) ** 2 <= r * r
        assert np.array_equal(cover([[[ax, ay], [bx, by]]], (r, 0, 0))[0], want), n


def test_radius_zero_covers_only_samples_on_the_segment():
    for a, b in (((c(5), c(5)), (c(40), c(40))), ((c(3), c(50)), (c(60), c(50))), ((c(10), c(10)), (c(40), c(25))), ((c(10), c(60) + 1), (c(30), c(60) + 1))):
        want = np.zeros((SIZE, SIZE), bool)
        for x, y, i, j in samples():
            on_line = (x - a[0]) * (b[1] - a[1]) == (y - a[1]) * (b[0] - a[0])
            want[i, j] = on_line and min(a[0], b[0]) <= x <= max(a[0], b[0]) and min(a[1], b[1]) <= y <= max(a[1], b[1])
        assert np.array_equal(cover([[a, b]], (0, 0, 0))[0], want), (a, b)
    assert cover([[(c(5), c(5)), (c(40), c(40))]], (0, 0, 0)).sum() == 36 and cover([[(c(10), c(60) + 1), (c(30), c(60) + 1)]], (0, 0, 0)).sum() == 0


def test_the_wide_compare_agrees_with_python_integers():
    """ends at the guard: cross products beyond 2^31, whose squares do not fit int64"""
    jq, bones, colors, radii = SE.crafted_cases(SIZE)['guard']
    got = SE.raster(jq, bones, colors, radii, SIZE, 1)['prim_id'][0]
    want = np.full((SIZE, SIZE), -1)
    big = 0
    for k, (ia, ib) in enumerate(bones.tolist()):
        (ax, ay), (bx, by) = jq[0, ia].tolist(), jq[0, ib].tolist()
        dx, dy = bx - ax, by - ay
        dd = dx * dx + dy * dy
        for x, y, i, j in samples():
            t, cross = (x - ax) * dx + (y - ay) * dy, (x - ax) * dy - (y - ay) * dx
            big += abs(cross) >= 1 << 31
            assert 0 < t < dd
            if cross * cross <= radii[0] ** 2 * dd:
                want[i, j] = 3 * k
    assert big >= SIZE * SIZE and (want == 0).sum() > 1000 and (want == 3).sum() > 1000 and not (want == 6).any() and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the seeded corruptions
def scenes():
    """(x [F,J,3] or None, view, jq or None, bones, colors, radii, size, ss): what the corruptions are shown on"""
    bones, colors = np.array(R.SKELETON_BONES, np.int32), np.array(R.SKELETON_COLORS, np.uint8)
    out = [(SE.walking(2, seed=3), R.SKELETON_VIEW, None, bones, colors, R.skeleton_radii(256), SIZE, ss) for ss in (1, 2)]
    out.append((SE.joint_cloud(20000, seed=1), R.SKELETON_VIEW, None, None, None, None, 2048, 2))            # the projection alone
    out.append((SE.FMA_JOINT, SE.FMA_VIEW, None, None, None, None, SIZE, 1))
    for name in ('exact_r', 'sentinel'):
        jq, b, col, radii = SE.crafted_cases(SIZE)[name]
        out.append((None, None, jq, b, col, radii, SIZE, 1))
    return out


def run(scene, corrupt=()):
    x, view, jq, bones, colors, radii, size, ss = scene
    res = {}
    if x is not None:
        jq = res['jq'] = SE.project(x, view, size * ss, corrupt)
    if bones is not None:
        res.update(SE.raster(jq, bones, colors, radii, size, ss, corrupt))
    return res


@pytest.fixture(scope='module')
def clean():
    return [(s, run(s)) for s in scenes()]


def gates(got, ref):
    return [m for k in ('jq', 'prim_id', 'rgb') if k in ref for m in SE.gate_equal(k, got[k], ref[k])]


def test_the_scenes_show_what_they_are_for(clean):
    assert not any(gates(run(s), ref) for s, ref in clean)
    jq = clean[2][1]['jq']
    assert (jq[0, :3] == SE.OUTSIDE).all() and (jq[0, 4:8] == SE.OUTSIDE).all() and 0.5 < (jq != SE.OUTSIDE).mean() < 1
    assert clean[3][1]['jq'].tolist() == [[[-1, -1]]]                          # the uncontracted rounding of both rows (skelerr.FMA_VIEW)
    assert len(np.unique(clean[0][1]['prim_id'])) > 30


@pytest.mark.parametrize('name', SE.CORRUPTIONS)
def test_every_corruption_fails_a_gate(clean, name):
    failed = [m for s, ref in clean for m in gates(run(s, (name,)), ref)]
    assert failed, f'{name}: no gate notices'
