#!/usr/bin/env python
"""Mint tests/golden/skeleton_view.npz with the REFERENCE's own `motion2video_3d` (lib/utils/vismo.py:246-285), run unmodified from the
checkout oracle/make_golden.py names (MOTIONBERT_REFERENCE), with the stand-ins of tools/mint_render.py for the modules vismo.py imports.

    python tools/mint_skeleton.py             # write the fixture
    python tools/mint_skeleton.py --check     # mint again and compare with the committed file

The collecting writer also reads `plt.gcf().axes[0].get_proj()` for each frame: the reference appends a frame before it closes the figure.

The scene (tests/skelerr.view_scene): a 17-joint pose whose left, right and middle bones are apart, placed in the four quadrants of the box,
near and far, and then moved.  It goes through `pixel2world_vis_motion(motion, dim=3)` as render_and_save passes it on.  Stored, and nothing
else: the motion [T,17,3] float32, the projection matrix M [4,4] float64 (one for all frames: asserted), matplotlib's version string, and
per frame and per colour class (left, right, mid) the 64 x 64 mask of the reference's image: a block holds a pixel that equals the class's
colour exactly.  Needs matplotlib and PIL; the tests do not."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import render as R                     # noqa: E402
from tests import skelerr as SE                            # noqa: E402
from tools.mint_render import MASK, reference_vismo        # noqa: E402

OUT = os.path.join(ROOT, 'tests/golden', 'skeleton_view.npz')
CLASSES = (R.COLOR_LEFT, R.COLOR_RIGHT, R.COLOR_MID)


class Frames(list):
    """the list the stand-in writer appends to: every frame brings the projection of the figure that is still open"""

    def __init__(self):
        super().__init__()
        self.proj = []

    def append(self, frame):
        import matplotlib.pyplot as plt
        self.proj.append(np.array(plt.gcf().axes[0].get_proj(), np.float64))
        super().append(frame)


def mint():
    import matplotlib
    motion = SE.view_scene()
    frames = Frames()
    vismo = reference_vismo(None, frames)
    world = vismo.pixel2world_vis_motion(np.transpose(motion, (1, 2, 0)), dim=3)      # [17,3,T], as render_and_save forms it
    assert world.dtype == np.float32
    vismo.motion2video_3d(world, 'skeleton_view.mp4')
    assert len(frames) == motion.shape[0] == len(frames.proj)
    M = frames.proj[0]
    assert all(np.array_equal(M, p) for p in frames.proj), 'the projection changed between frames'
    masks = np.zeros((len(frames), len(CLASSES), MASK, MASK), bool)
    for t, img in enumerate(frames):
        H, W = img.shape[:2]
        for k, colour in enumerate(CLASSES):
            ii, jj = np.nonzero((img[:, :, :3] == np.array(colour, np.uint8)).all(-1))
            masks[t, k, ii * MASK // H, jj * MASK // W] = True
            print(f'frame {t} class {k}: image {H} x {W}, {len(ii)} pixels of the colour, centroid of the mask (x, y) = '
                  f'({np.nonzero(masks[t, k])[1].mean():.1f}, {np.nonzero(masks[t, k])[0].mean():.1f})', flush=True)
    return dict(motion=motion, M=M, matplotlib=np.array(matplotlib.__version__), mask=masks)


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
