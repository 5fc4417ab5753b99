"""motionbert_amd.render's skeleton frames end to end on the CPU through the reference provider (tests/skelerr.RefOps): the view against the
reference's own drawing code (tests/golden/skeleton_view.npz, minted by tools/mint_skeleton.py), validation, F = 0, chunks against the whole,
host arrays, and the C ABI's refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from tests import skelerr as SE
from tests.helpers import GOLDEN

SIZE = 40
CLASSES = (R.COLOR_LEFT, R.COLOR_RIGHT, R.COLOR_MID)


@pytest.fixture(scope='module')
def motion():
    return torch.from_numpy(SE.walking(5, seed=2))


# ------------------------------------------------------------------------------------------------ the view
def test_the_view_is_the_matrix_of_the_reference_axes():
    z = np.load(os.path.join(GOLDEN, 'skeleton_view.npz'))
    M = z['M']
    ours = np.array(R.SKELETON_VIEW[:12]).reshape(3, 4)
    assert np.allclose(ours, M[[0, 1, 3]], rtol=1e-12, atol=0)
    assert M[0, 0] == -2.2898245799383393e-03 and M[0, 1] == 4.0375785453255678e-04 and M[0, 2] == 0 and M[0, 3] == -5.8619509246421508e-01
    assert R.SKELETON_VIEW[12:] == (-0.095, 0.09, 1 / 0.185)
    # w over the box of the axes: the perspective row never comes near zero
    corners = np.array([[x, y, zz, 1.0] for x in (-512, 0) for y in (-256, 256) for zz in (-512, 0)])
    w = corners @ M[3]
    assert 9.1 < w.min() < 9.3 and 10.7 < w.max() < 10.9


def test_the_tables_are_the_reference_lists():
    assert len(R.SKELETON_BONES) == 16 == len(R.SKELETON_COLORS)
    assert [R.SKELETON_COLORS[R.SKELETON_BONES.index(b)] for b in ((0, 4), (12, 13), (0, 1), (15, 16), (0, 7), (9, 10))] == \
        [R.COLOR_LEFT, R.COLOR_LEFT, R.COLOR_RIGHT, R.COLOR_RIGHT, R.COLOR_MID, R.COLOR_MID]
    assert sum(c == R.COLOR_LEFT for c in R.SKELETON_COLORS) == 6 == sum(c == R.COLOR_RIGHT for c in R.SKELETON_COLORS)
    assert (R.COLOR_LEFT, R.COLOR_RIGHT, R.COLOR_MID) == ((0x02, 0x31, 0x5E), (0x2F, 0x70, 0xAF), (0x00, 0x45, 0x7E))
    # widths at the reference's own frame: 5 px, 8.33 px and 1.67 px across -> radii of 40, 66.7 and 13.3 sixteenths
    assert R.skeleton_radii(924) == (40, 67, 13) and R.skeleton_radii(924, 2) == (80, 133, 27)
    assert all(0 <= r <= R.MAX_RADIUS for r in R.skeleton_radii(2048, 2))


def test_placement_agrees_with_the_reference_drawing():
    """the reference's motion2video_3d drew the scene; per frame and colour class the centroid of our render lies inside the box of the
    reference's pixels of that colour, grown by one block for the rounding of its tight crop, and moves the way the reference's does.  Drawn
    with the widths of a 256-px frame: at 64 px the reference's widths are a third of a sample and a line may pass between all centres."""
    z = np.load(os.path.join(GOLDEN, 'skeleton_view.npz'))
    x = SE.view_scene()
    assert np.array_equal(z['motion'], x)
    rgb = R.render_skeleton(x, size=64, radii=R.skeleton_radii(256), ops=SE.RefOps())['rgb'].numpy()
    ours, theirs = np.zeros((len(x), 3, 2)), np.zeros((len(x), 3, 2))
    for t in range(len(x)):
        for k, colour in enumerate(CLASSES):
            i, j = np.nonzero((rgb[t] == np.array(colour, np.uint8)).all(-1))
            ri, rj = np.nonzero(z['mask'][t, k])
            assert len(i) > 3 and len(ri) > 3
            ours[t, k], theirs[t, k] = (j.mean(), i.mean()), (rj.mean(), ri.mean())
            assert rj.min() - 1 <= j.mean() <= rj.max() + 1 and ri.min() - 1 <= i.mean() <= ri.max() + 1, (t, k)
    step_o, step_t = np.diff(ours, axis=0), np.diff(theirs, axis=0)
    moved = np.abs(step_t) > 2
    assert moved.sum() >= 20 and np.array_equal(np.sign(step_o)[moved], np.sign(step_t)[moved])
    # the left limbs are drawn right of the right limbs: image x right with x
    assert (ours[:, 0, 0] > ours[:, 1, 0] + 3).all() and (theirs[:, 0, 0] > theirs[:, 1, 0] + 3).all()


# ------------------------------------------------------------------------------------------------ the API
def test_render_skeleton_matches_the_reference(motion):
    ops = SE.RefOps()
    got = R.render_skeleton(motion, size=SIZE, ss=2, want=('rgb', 'prim_id', 'jq'), ops=ops)
    assert ops.calls == [('project', 5), ('raster', 5)]
    assert got['rgb'].shape == (5, SIZE, SIZE, 3) and got['rgb'].dtype == torch.uint8 and got['prim_id'].shape == (5, 2 * SIZE, 2 * SIZE)
    jq = SE.project(motion.numpy(), R.SKELETON_VIEW, 2 * SIZE)
    ref = SE.raster(jq, R.SKELETON_BONES, R.SKELETON_COLORS, R.skeleton_radii(SIZE, 2), SIZE, 2)
    assert np.array_equal(got['jq'].numpy(), jq) and np.array_equal(got['rgb'].numpy(), ref['rgb']) and np.array_equal(got['prim_id'].numpy(), ref['prim_id'])
    assert jq.min() >= 0 and jq.max() <= 2 * SIZE * SE.SUB and all((ref['prim_id'][f] >= 0).any() for f in range(5))
    # a host array goes straight in; `out`; other bones, colours and radii; a view
    out = torch.zeros(5, SIZE, SIZE, 3, dtype=torch.uint8)
    res = R.render_skeleton(motion.numpy(), size=SIZE, ss=2, out=out, ops=SE.RefOps())
    assert set(res) == {'rgb'} and res['rgb'] is out and np.array_equal(out.numpy(), ref['rgb'])
    bones, colors = [(0, 7), (7, 8)], torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.uint8)
    two = R.render_skeleton(motion, size=SIZE, bones=bones, colors=colors, radii=(20, 30, 10), want=('prim_id',), ops=SE.RefOps())['prim_id'].numpy()
    assert np.array_equal(two, SE.raster(SE.project(motion.numpy(), R.SKELETON_VIEW, SIZE), bones, colors.numpy(), (20, 30, 10), SIZE, 1)['prim_id'])
    assert set(np.unique(two)) <= set(range(-1, 6))
    view = np.array(R.SKELETON_VIEW)
    view[12] = -0.2
    assert not np.array_equal(R.render_skeleton(motion, size=SIZE, view=view, want=('jq',), ops=SE.RefOps())['jq'].numpy()[..., 0],
                              SE.project(motion.numpy(), R.SKELETON_VIEW, SIZE)[..., 0])


def test_chunks_equal_the_whole(motion):
    whole = R.render_skeleton(motion, size=SIZE, ops=SE.RefOps())['rgb'].numpy()
    for chunk in (1, 2, 5, 32):
        ops = SE.RefOps()
        parts = [p.copy() for p in R.skeleton_chunks(motion, size=SIZE, chunk=chunk, ops=ops)]
        assert [p.shape[0] for p in parts] == [min(chunk, 5 - a) for a in range(0, 5, chunk)]
        assert all(p.dtype == np.uint8 for p in parts) and np.array_equal(np.concatenate(parts), whole), chunk
        assert [c for c in ops.calls if c[0] == 'raster'] == [('raster', p.shape[0]) for p in parts]
    assert np.array_equal(np.concatenate([p.copy() for p in R.skeleton_chunks(motion.numpy(), size=SIZE, chunk=3, ops=SE.RefOps())]), whole)
    assert list(R.skeleton_chunks(motion[:0], size=SIZE, ops=SE.RefOps())) == []


def test_no_frames_no_launch(motion):
    ops = SE.RefOps()
    got = R.render_skeleton(motion[:0], size=SIZE, ss=2, want=('rgb', 'prim_id', 'jq'), ops=ops)
    assert ops.calls == []
    assert got['rgb'].shape == (0, SIZE, SIZE, 3) and got['prim_id'].shape == (0, 2 * SIZE, 2 * SIZE) and got['jq'].shape == (0, 17, 2)


def test_validation(motion):
    ops = SE.RefOps()
    for bad, match in ((dict(x3d=motion.double()), 'float32'), (dict(x3d=motion[0]), 'x3d'), (dict(x3d=motion.numpy().astype(np.float64)), 'float32'),
                       (dict(x3d=motion[..., :2]), 'x3d'), (dict(x3d=torch.zeros(2, 33, 3)), 'x3d'), (dict(x3d=[[1, 2, 3]]), 'x3d'),
                       (dict(size=0), 'size'), (dict(size=2049), 'size'), (dict(size=64.0), 'size'), (dict(ss=3), 'ss'), (dict(ss=0), 'ss'),
                       (dict(view=R.SKELETON_VIEW[:14]), 'view'), (dict(view=(float('nan'),) * 15), 'view'),
                       (dict(bones=[(0, 1)]), 'colors'), (dict(bones=[(0, 1)], colors=[(1, 2, 3), (4, 5, 6)]), 'colors'),
                       (dict(bones=[(0, 1, 2)], colors=[(1, 2, 3)]), 'bones'), (dict(bones=[(0, 1)] * 65, colors=[(1, 2, 3)] * 65), 'bones'),
                       (dict(bones=torch.zeros(1, 2, dtype=torch.int64), colors=[(1, 2, 3)]), 'bones'), (dict(colors=[(1, 2, 300)] * 16), 'colors'),
                       (dict(radii=(1, 2)), 'radii'), (dict(radii=(1.0, 2, 1)), 'radii'), (dict(radii=(1, 2, 3)), 'radii'), (dict(radii=(-1, 2, 1)), 'radii'),
                       (dict(radii=(1, 2049, 1)), 'radii'), (dict(want=('frames',)), 'want'), (dict(want=()), 'want'),
                       (dict(out=torch.zeros(5, SIZE, SIZE, 3)), 'out'), (dict(out=torch.zeros(4, SIZE, SIZE, 3, dtype=torch.uint8)), 'out')):
        kw = dict(x3d=motion, size=SIZE, ops=ops)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            R.render_skeleton(kw.pop('x3d'), **kw)
    with pytest.raises(ValueError, match='chunk'):
        list(R.skeleton_chunks(motion, size=SIZE, chunk=0, ops=ops))
    assert ops.calls == []
    # host tensors without a provider: no CPU path
    with pytest.raises(RuntimeError, match='ROCm device'):
        R.render_skeleton(motion, size=SIZE)
    with pytest.raises(RuntimeError, match='ROCm device'):
        list(R.skeleton_chunks(motion, size=SIZE))


def test_library_refuses_bad_arguments():
    """no launch is made: the checks come first"""
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 210
    view = (ctypes.c_double * 15)(*R.SKELETON_VIEW)
    assert lib.mbx_skeleton_project(None, view, 1, 17, 64, 3, None, None) != 0 and b'ss' in lib.mbx_last_error()
    assert lib.mbx_skeleton_project(None, view, 1, 17, 4096, 1, None, None) != 0 and b'size' in lib.mbx_last_error()
    assert lib.mbx_skeleton_project(None, view, 1, 33, 64, 1, None, None) != 0 and b'J=33' in lib.mbx_last_error()
    assert lib.mbx_skeleton_project(None, view, -1, 17, 64, 1, None, None) != 0 and b'F=-1' in lib.mbx_last_error()
    assert lib.mbx_skeleton_project(None, view, 1, 17, 64, 1, None, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_skeleton_project(None, None, 0, 17, 64, 1, None, None) == 0
    r = lambda *a: lib.mbx_skeleton_raster(None, None, None, *a, None, None, None)      # noqa: E731  (F, J, Nb, r_line, r_out, r_in, size, ss)
    assert r(1, 17, 0, 1, 2, 1, 64, 1) != 0 and b'Nb=0' in lib.mbx_last_error()
    assert r(1, 17, 65, 1, 2, 1, 64, 1) != 0 and b'Nb=65' in lib.mbx_last_error()
    assert r(1, 0, 16, 1, 2, 1, 64, 1) != 0 and b'J=0' in lib.mbx_last_error()
    assert r(1, 17, 16, 2049, 2, 1, 64, 1) != 0 and b'radius' in lib.mbx_last_error()
    assert r(1, 17, 16, 1, 2, 3, 64, 1) != 0 and b'radius' in lib.mbx_last_error()
    assert r(1, 17, 16, 1, 2, -1, 64, 1) != 0 and b'radius' in lib.mbx_last_error()
    assert r(1, 17, 16, 1, 2, 1, 0, 1) != 0 and b'size' in lib.mbx_last_error()
    assert r(1, 17, 16, 1, 2, 1, 64, 4) != 0 and b'ss' in lib.mbx_last_error()
    assert r(1, 17, 16, 1, 2, 1, 64, 1) != 0 and b'null' in lib.mbx_last_error()
    assert r(0, 17, 16, 1, 2, 1, 64, 1) == 0
