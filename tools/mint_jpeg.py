"""Mint tests/golden/jpeg_pil.npz: libjpeg-turbo's own files (through Pillow, optimize=False) for the cases the JPEG gates run on.

    python tools/mint_jpeg.py            # needs Pillow; run where it is installed

Per case i the fixture holds the input frame (`rgb_i`), Pillow's complete file (`file_i`) and the quantised coefficients parsed from it
(`coef_i`, [n_mcu, blocks per MCU, 64] in zigzag order); `params` [n,5] = (H, W, quality, sub (1: 4:2:0), restart interval in MCUs), `kinds` the
content names and `versions` Pillow's and libjpeg-turbo's.  The mint refuses to write if the numpy reference (tests/jpegerr.py) differs from
Pillow in any byte or coefficient: the fixture then proves the reference, and the reference can stand in for libjpeg wherever Pillow is absent."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpegerr as J      # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'jpeg_pil.npz')
# (H, W, content, quality, subsampling, restart): 'row' = one MCU row, 'all' = more MCUs than the frame has.  Every size, content, quality,
# subsampling and restart value appears; noise at quality 100 appears at every size.
CASES = [
    (1, 1, 'noise', 100, '444', 1), (16, 16, 'noise', 100, '420', 'row'), (33, 17, 'noise', 100, '420', 3), (40, 56, 'noise', 100, '444', 'all'),
    (72, 72, 'noise', 100, '420', 1), (250, 250, 'noise', 100, '420', 'row'), (16, 2048, 'noise', 100, '420', 3),
    (33, 17, 'ramp', 75, '444', 1), (33, 17, 'render', 90, '420', 'row'), (33, 17, 'noise', 25, '420', 1),
    (40, 56, 'ramp', 25, '420', 3), (40, 56, 'render', 75, '420', 'all'), (40, 56, 'noise', 75, '444', 3),
    (72, 72, 'render', 90, '444', 'row'), (72, 72, 'white', 75, '420', 3), (72, 72, 'noise', 90, '420', 'all'),
    (16, 16, 'black', 25, '444', 'all'), (1, 1, 'white', 90, '420', 'row'),
    (250, 250, 'render', 90, '420', 'row'), (250, 250, 'render', 75, '444', 'all'), (16, 2048, 'ramp', 75, '444', 1), (16, 2048, 'render', 90, '420', 'row'),
]


def restart_of(H, W, sub, r):
    mx, my, _ = J.geometry(H, W, sub)
    return mx if r == 'row' else mx * my + 7 if r == 'all' else r


def pil_file(rgb, quality, sub, restart):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, 'JPEG', quality=quality, subsampling={'420': 2, '444': 0}[sub], optimize=False, restart_marker_blocks=restart)
    return b.getvalue()


def main():
    import PIL
    from PIL import features
    out, params, kinds = {}, [], []
    for i, (H, W, kind, quality, sub, r) in enumerate(CASES):
        restart = restart_of(H, W, sub, r)
        rgb = J.content(kind, H, W, seed=100 + i)
        ref = pil_file(rgb, quality, sub, restart)
        ours = J.encode(rgb, quality, sub, restart)
        bad = J.gate_file(f'case {i} {H}x{W} {kind} q{quality} {sub} restart {restart}', ours, ref)
        parsed = J.parse(ref)
        bad += J.gate_equal(f'case {i} coefficients', J.front(rgb, quality, sub), parsed['coef'])
        if bad or (parsed['H'], parsed['W'], parsed['sub'], parsed['restart']) != (H, W, sub, restart):
            sys.exit(f'the numpy reference differs from Pillow, nothing written: {bad}')
        out[f'rgb_{i}'], out[f'file_{i}'], out[f'coef_{i}'] = rgb, np.frombuffer(ref, np.uint8), parsed['coef']
        params.append((H, W, quality, int(sub == '420'), restart))
        kinds.append(kind)
    out['params'], out['kinds'] = np.array(params, np.int32), np.array(kinds)
    out['versions'] = np.array([f'Pillow {PIL.__version__}', f'libjpeg-turbo {features.version("libjpeg_turbo")}', f'jpeglib {features.version("jpg")}'])
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {len(CASES)} cases, {os.path.getsize(OUT)} bytes, {" / ".join(out["versions"])}')


if __name__ == '__main__':
    main()
