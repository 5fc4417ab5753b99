"""motionbert_amd.render end to end on the CPU through the reference provider (tests/rendererr.RefOps): validation, F = 0, chunks against
the whole, per-track cubes, the faces of SMPLModel, the C ABI's refusals, and the orientation of the view against the reference's own
drawing code (tests/golden/render_view.npz, minted by tools/mint_render.py)."""
import os

import numpy as np
import pytest
import torch

from motionbert_amd import render as R
from motionbert_amd.smpl import SMPLModel
from tests import rendererr as RE
from tests.helpers import GOLDEN

SIZE = 40


@pytest.fixture(scope='module')
def scene():
    verts, faces = RE.deformed_icosphere(5, seed=4)
    verts[3:] += np.float32(500.0)                       # the second track lives elsewhere
    return torch.from_numpy(verts), torch.from_numpy(faces)


def test_frame_cube(scene):
    verts, _ = scene
    cube = R.frame_cube(verts, [3, 2])
    assert cube.shape == (2, 4) and cube.dtype == torch.float32
    v = verts[:3].reshape(-1, 3).numpy()
    assert np.allclose(cube[0, :3].numpy(), (v.max(0) + v.min(0)) / 2, rtol=1e-6)
    assert np.isclose(cube[0, 3].item(), 1 / ((v.max(0) - v.min(0)).max() * (1 + 2.0 ** -16)), rtol=1e-6)
    assert torch.equal(R.frame_cube(verts[3:]), cube[1:])
    one = R.frame_cube(verts)                             # the whole motion: the box of all five frames
    assert one[0, 3] < cube[0, 3] and one[0, 3] < cube[1, 3]
    with pytest.raises(ValueError, match='seq_lens'):
        R.frame_cube(verts, [3, 3])


def test_render_mesh_matches_the_reference_and_frames_the_whole_motion(scene):
    verts, faces = scene
    ops = RE.RefOps()
    got = R.render_mesh(verts, faces, seq_lens=[3, 2], size=SIZE, ss=2, want=('rgb', 'face_id', 'depth', 'vq'), ops=ops)
    assert ops.calls == [('project', 5), ('raster', 5)]
    assert got['rgb'].shape == (5, SIZE, SIZE, 3) and got['rgb'].dtype == torch.uint8 and got['face_id'].shape == (5, 2 * SIZE, 2 * SIZE)
    cube = R.frame_cube(verts, [3, 2]).numpy()
    vq = RE.project(verts.numpy(), cube, [0, 3, 5], 2 * SIZE)
    ref = RE.raster(vq, verts.numpy(), faces.numpy(), SIZE, 2)
    assert np.array_equal(got['vq'].numpy(), vq) and np.array_equal(got['rgb'].numpy(), ref['rgb'])
    assert np.array_equal(got['face_id'].numpy(), ref['face_id']) and np.array_equal(got['depth'].numpy(), ref['depth'])
    # every vertex of a track lies inside the image and the depth range: the cube is that of all the track's frames
    assert vq.min() >= 0 and vq[..., :2].max() <= 2 * SIZE * RE.SUB and vq[..., 2].max() <= RE.ZQ
    assert all(((ref['face_id'][f] >= 0).mean() > 0.05) for f in range(5))
    # per-track cubes: one cube over both tracks would shrink each body to a corner
    single = R.render_mesh(verts, faces, size=SIZE, ss=1, want=('face_id',), ops=RE.RefOps())['face_id'].numpy()
    assert (single >= 0).mean() < 0.25 * (ref['face_id'] >= 0).mean()
    # an explicit cube and `out`
    out = torch.zeros(5, SIZE, SIZE, 3, dtype=torch.uint8)
    res = R.render_mesh(verts, faces, cube=torch.from_numpy(cube), seq_lens=[3, 2], size=SIZE, ss=2, out=out, ops=RE.RefOps())
    assert set(res) == {'rgb'} and res['rgb'] is out and np.array_equal(out.numpy(), ref['rgb'])


def test_chunks_equal_the_whole(scene):
    verts, faces = scene
    whole = R.render_mesh(verts, faces, seq_lens=[3, 2], size=SIZE, ops=RE.RefOps())['rgb'].numpy()
    for chunk in (1, 2, 5, 32):
        ops = RE.RefOps()
        parts = [c.copy() for c in R.render_chunks(verts, faces, seq_lens=[3, 2], size=SIZE, chunk=chunk, ops=ops)]
        assert [p.shape[0] for p in parts] == [min(chunk, 5 - a) for a in range(0, 5, chunk)]
        assert all(p.dtype == np.uint8 for p in parts) and np.array_equal(np.concatenate(parts), whole), chunk
        assert [c for c in ops.calls if c[0] == 'raster'] == [('raster', p.shape[0]) for p in parts]
    assert list(R.render_chunks(verts[:0], faces, size=SIZE, ops=RE.RefOps())) == []


def test_no_frames_no_launch(scene):
    verts, faces = scene
    ops = RE.RefOps()
    got = R.render_mesh(verts[:0], faces, size=SIZE, ss=2, want=('rgb', 'face_id', 'depth', 'vq'), ops=ops)
    assert ops.calls == []
    assert got['rgb'].shape == (0, SIZE, SIZE, 3) and got['face_id'].shape == (0, 2 * SIZE, 2 * SIZE) and got['vq'].shape == (0, 42, 3)


def test_validation(scene):
    verts, faces = scene
    ops = RE.RefOps()
    for bad, match in ((dict(verts=verts.double()), 'float32'), (dict(verts=verts[0]), 'verts'), (dict(verts=verts.numpy()), 'verts'),
                       (dict(faces=faces.long()), 'int32'), (dict(faces=faces[:, :2]), 'faces'), (dict(faces=faces[:0]), 'empty'),
                       (dict(size=0), 'size'), (dict(size=2049), 'size'), (dict(size=64.0), 'size'), (dict(ss=3), 'ss'), (dict(ss=0), 'ss'),
                       (dict(seq_lens=[2, 2]), 'seq_lens'), (dict(cube=torch.zeros(2, 4)), 'cube'), (dict(cube=torch.zeros(1, 4).double()), 'cube'),
                       (dict(want=('frames',)), 'want'), (dict(want=()), 'want'), (dict(color=(1, 2)), 'color'), (dict(alpha=1.5), 'alpha'),
                       (dict(out=torch.zeros(5, SIZE, SIZE, 3)), 'out'), (dict(out=torch.zeros(4, SIZE, SIZE, 3, dtype=torch.uint8)), 'out')):
        kw = dict(verts=verts, faces=faces, size=SIZE, ops=ops)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            R.render_mesh(kw.pop('verts'), kw.pop('faces'), **kw)
    with pytest.raises(ValueError, match='chunk'):
        list(R.render_chunks(verts, faces, size=SIZE, chunk=0, ops=ops))
    assert ops.calls == []
    # host tensors without a provider: no CPU path
    with pytest.raises(RuntimeError, match='ROCm device'):
        R.render_mesh(verts, faces, size=SIZE)
    with pytest.raises(RuntimeError, match='ROCm device'):
        list(R.render_chunks(verts, faces, size=SIZE))


def test_library_refuses_bad_arguments():
    """no launch is made: the checks come first"""
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 200
    assert lib.mbx_render_raster_ws(3, 100) >= 3 * 4 + 3 * 100 * 8
    assert lib.mbx_render_project(None, None, None, 1, 1, 10, 64, 3, None, None) != 0 and b'ss' in lib.mbx_last_error()
    assert lib.mbx_render_project(None, None, None, 1, 1, 10, 4096, 1, None, None) != 0 and b'size' in lib.mbx_last_error()
    assert lib.mbx_render_project(None, None, None, 1, 1, 10, 64, 1, None, None) != 0 and b'null' in lib.mbx_last_error()
    assert lib.mbx_render_project(None, None, None, 1, 0, 10, 64, 1, None, None) == 0
    assert lib.mbx_render_raster(None, None, None, 1, 10, 0, 64, 1, 1.0, 1.0, 1.0, 0.9, None, None, None, None, 0, None) != 0
    assert b'Nf' in lib.mbx_last_error()
    assert lib.mbx_render_raster(None, None, None, 1, 10, 5, 64, 1, 256.0, 1.0, 1.0, 0.9, None, None, None, None, 0, None) != 0
    assert b'colour' in lib.mbx_last_error()
    assert lib.mbx_render_raster(None, None, None, 1, 10, 5, 64, 1, 1.0, 1.0, 1.0, 0.9, None, None, None, None, 0, None) != 0
    assert b'null' in lib.mbx_last_error()
    assert lib.mbx_render_raster(None, None, None, 0, 10, 5, 64, 1, 1.0, 1.0, 1.0, 0.9, None, None, None, None, 0, None) == 0


def test_smpl_model_keeps_its_faces(tmp_path):
    m = SMPLModel.synthetic(30, 0)
    assert m.faces is None
    m.to_npz(tmp_path / 'plain.npz')
    assert 'faces' not in np.load(tmp_path / 'plain.npz').files and SMPLModel.from_npz(tmp_path / 'plain.npz').faces is None
    faces = np.random.default_rng(0).integers(0, 30, (50, 3)).astype(np.uint32)         # the model files store `f` as uint32
    m.faces = SMPLModel(m.v_template, m.shapedirs, m.posedirs.numpy(), m.J_regressor, m.parents, m.lbs_weights, faces=faces).faces
    assert m.faces.dtype == torch.int32 and np.array_equal(m.faces.numpy(), faces.astype(np.int32))
    m.to_npz(tmp_path / 'with.npz')
    back = SMPLModel.from_npz(tmp_path / 'with.npz')
    assert torch.equal(back.faces, m.faces) and torch.equal(back.v_template, m.v_template)
    z = dict(np.load(tmp_path / 'with.npz'))
    z['f'] = z.pop('faces')                                                             # the name in the model files
    np.savez(tmp_path / 'f.npz', **z)
    assert torch.equal(SMPLModel.from_npz(tmp_path / 'f.npz').faces, m.faces)

    class Module:
        pass
    mod = Module()
    for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'parents', 'lbs_weights'):
        setattr(mod, k, getattr(m, k))
    assert SMPLModel.from_module(mod).faces is None
    mod.faces = faces
    assert torch.equal(SMPLModel.from_module(mod).faces, m.faces)
    for bad in (faces[:, :2], faces.astype(np.float32), np.full((2, 3), 30), np.full((2, 3), -1)):
        with pytest.raises(ValueError, match='faces'):
            SMPLModel(m.v_template, m.shapedirs, m.posedirs.numpy(), m.J_regressor, m.parents, m.lbs_weights, faces=bad)


def test_orientation_agrees_with_the_reference_drawing():
    """the reference's motion2video_mesh drew the scene; both renders put the blob in the same quadrant of the image, frame by frame, and
    move it the same way between frames: x right, y down, one cube for the whole motion"""
    z = np.load(os.path.join(GOLDEN, 'render_view.npz'))
    verts, faces = RE.view_scene()
    assert np.array_equal(z['verts'], verts) and np.array_equal(z['faces'], faces)
    fid = R.render_mesh(torch.from_numpy(verts), torch.from_numpy(faces), size=64, want=('face_id',), ops=RE.RefOps())['face_id'].numpy()

    def centroids(mask):
        return np.array([[np.nonzero(m)[1].mean(), np.nonzero(m)[0].mean()] for m in mask])
    ours, theirs = centroids(fid >= 0), centroids(z['mask'])
    assert np.array_equal(np.sign(ours - 31.5), np.sign(theirs - 31.5))                          # the quadrant, every frame
    assert np.array_equal(np.sign(ours[:4] - 31.5), np.sign(np.array(RE.VIEW_XY[:4])))            # +x right of centre, +y below it
    step_o, step_t = np.diff(ours, axis=0), np.diff(theirs, axis=0)
    moved = np.abs(np.diff(np.array(RE.VIEW_XY), axis=0)) > 0
    assert np.array_equal(np.sign(step_o)[moved], np.sign(step_t)[moved])                        # the direction of every move
    assert np.array_equal(np.sign(step_o)[moved], np.sign(np.diff(np.array(RE.VIEW_XY), axis=0))[moved])
