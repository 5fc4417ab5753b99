#!/usr/bin/env python
"""Mint tests/golden/render_view.npz with the REFERENCE's own `motion2video_mesh` (lib/utils/vismo.py:287-338), run unmodified from the
checkout oracle/make_golden.py names (MOTIONBERT_REFERENCE).

    python tools/mint_render.py             # write the fixture
    python tools/mint_render.py --check     # mint again and compare with the committed file

vismo.py imports modules that need not be installed (`cv2`, `imageio`, `ipdb`, and `smplx` / `easydict` through utils_smpl and tools).  Each
missing one is replaced in `sys.modules` by a stand-in that holds only the names the import statements ask for; `cv2` additionally decodes
the PNG that `get_img_from_fig` hands it (through PIL) and converts BGR to RGBA, as the two calls of that function expect.  The video writer
`imageio.get_writer` returns collects the frames; `get_smpl_faces` returns the faces of the test mesh.  matplotlib draws with the Agg backend.

The scene (tests/rendererr.view_scene): a small icosahedron that visits the four quadrants of the bounding cube and then moves across it.
Stored, and nothing else: the vertices [T,V,3] float32, the faces, and per frame the 64 x 64 foreground mask of the reference's image
(a block holds a pixel that is not white).  Needs matplotlib and PIL; the tests do not."""
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden                             # noqa: E402
from tests import rendererr as RE                          # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'render_view.npz')
MASK = 64


def _stand_in(name, **names):
    try:
        __import__(name)
        return False
    except ImportError:
        m = types.ModuleType(name)
        m.__dict__.update(names)
        sys.modules[name] = m
        return True


def reference_vismo(faces, frames):
    """the reference's vismo module, with its writer appending to `frames` and its faces replaced by `faces`"""
    import matplotlib
    matplotlib.use('Agg')
    from PIL import Image

    def imdecode(buf, flags):
        return np.asarray(Image.open(io.BytesIO(np.asarray(buf).tobytes())).convert('RGB'))[:, :, ::-1].copy()      # BGR, as cv2 decodes

    def cvtColor(img, code):
        assert code == 'BGR2RGBA'
        return np.concatenate([img[:, :, ::-1], np.full(img.shape[:2] + (1,), 255, np.uint8)], 2)

    class Writer:
        def append_data(self, frame):
            frames.append(np.asarray(frame).copy())

        def close(self):
            pass
    _stand_in('cv2', imdecode=imdecode, cvtColor=cvtColor, COLOR_BGR2RGBA='BGR2RGBA')
    if _stand_in('imageio'):
        sys.modules['imageio'].get_writer = lambda *a, **k: Writer()
    _stand_in('ipdb')
    _stand_in('easydict', EasyDict=dict)
    if _stand_in('smplx', SMPL=object):
        _stand_in('smplx.utils', ModelOutput=object, SMPLOutput=object)
        _stand_in('smplx.lbs', vertices2joints=None)
    sys.path.insert(0, make_golden.REF)
    from lib.utils import vismo
    vismo.imageio.get_writer = lambda *a, **k: Writer()
    vismo.get_smpl_faces = lambda: faces
    return vismo


def mint():
    verts, faces = RE.view_scene()
    frames = []
    vismo = reference_vismo(faces, frames)
    vismo.motion2video_mesh(np.transpose(verts.astype(np.float64), (1, 2, 0)), 'render_view.mp4', draw_face=True)      # [V,3,T], as render_and_save passes it
    assert len(frames) == verts.shape[0]
    masks = []
    for img in frames:
        fg = (img[:, :, :3] != 255).any(-1)
        H, W = fg.shape
        m = np.zeros((MASK, MASK), bool)
        ii, jj = np.nonzero(fg)
        m[ii * MASK // H, jj * MASK // W] = True
        masks.append(m)
        print(f'frame {len(masks) - 1}: image {H} x {W}, {int(fg.sum())} foreground pixels, centroid of the mask (x, y) = '
              f'({np.nonzero(m)[1].mean():.1f}, {np.nonzero(m)[0].mean():.1f})', flush=True)
    return dict(verts=verts, faces=faces, mask=np.stack(masks))


def main():
    save = mint()
    if '--check' in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(save)
        for k, v in save.items():
            assert np.array_equal(old[k], v), k
        print('re-minted identically:', OUT)
        return
    np.savez_compressed(OUT, **save)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
