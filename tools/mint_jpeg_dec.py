"""Mint tests/golden/jpeg_dec_pil.npz: files written by libjpeg-turbo (through Pillow) and the pixels libjpeg-turbo decodes from them, for the cases
the JPEG decoding gates run on.

    python tools/mint_jpeg_dec.py            # needs Pillow; run where it is installed

Per case i the fixture holds Pillow's file (`file_i`) and `Image.open(file).convert('RGB')` (`rgb_i`); `params` [n,6] = (H, W, quality, sub (0:
4:4:4, 1: 4:2:0, 2: 4:2:2), restart interval in MCUs (0: none), optimize), `kinds` the content names and `versions` Pillow's and libjpeg-turbo's.
The mint refuses to write if the numpy reference (tests/jpegdecerr.py) differs from Pillow in any pixel: the fixture then proves the reference,
and the reference can stand in for libjpeg wherever Pillow is absent."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpegdecerr as D      # noqa: E402
from tests import jpegerr as J         # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'jpeg_dec_pil.npz')
# (H, W, content, quality, subsampling, restart, optimize): 'row' = one MCU row, 'all' = more MCUs than the frame has, 0 = no DRI.  The smallest
# shapes that reach every branch: partial MCUs both ways (3x5, 17x33), dw <= 2 (2x6 and 5x3 for 4:2:0, 9x4 and 5x3 for 4:2:2: the replicate
# rule), dw = 4 (31x7: both edge cases adjacent), the widest strip (16x2048).  Quality 100 gives the largest IDCT overshoot a picture can; it stays inside the part of the range-limit table that
# equals a clamp in every case here (tests/jpegdecerr.crafted_range has a scan that leaves it).
CASES = [
    (1, 1, 'noise', 100, '444', 0, False), (1, 1, 'noise', 90, '420', 1, False), (1, 1, 'noise', 100, '422', 0, True),
    (8, 8, 'noise', 100, '420', 0, False), (8, 8, 'smooth', 25, '422', 1, True), (8, 8, 'render', 90, '444', 'all', False),
    (3, 5, 'noise', 100, '420', 1, True), (3, 5, 'noise', 90, '422', 0, False), (3, 5, 'smooth', 25, '444', 3, False),
    (17, 33, 'noise', 100, '420', 'row', False), (17, 33, 'noise', 100, '422', 3, True), (17, 33, 'render', 90, '444', 1, True),
    (17, 33, 'smooth', 25, '420', 0, True),
    (17, 33, 'noise', 100, '422', 3, False), (17, 33, 'render', 100, '422', 3, False), (17, 33, 'smooth', 100, '422', 3, False),      # one header: a call of three
    (2, 6, 'noise', 100, '420', 0, False), (2, 6, 'noise', 90, '422', 1, False), (9, 4, 'noise', 100, '422', 0, True), (9, 4, 'noise', 25, '420', 1, False),
    (5, 3, 'noise', 100, '420', 0, False), (5, 3, 'noise', 100, '422', 'all', False), (5, 3, 'smooth', 90, '444', 0, True),
    (31, 7, 'noise', 100, '420', 1, False), (31, 7, 'noise', 100, '422', 'row', True), (31, 7, 'render', 25, '420', 0, True),
    (64, 48, 'noise', 100, '422', 'row', False), (64, 48, 'render', 90, '420', 3, True), (64, 48, 'smooth', 25, '444', 0, False),
    (64, 48, 'noise', 90, '420', 'all', True),
    (250, 250, 'noise', 100, '420', 'row', False), (250, 250, 'render', 90, '422', 0, True), (250, 250, 'smooth', 25, '444', 3, False),
    (16, 2048, 'noise', 100, '420', 'row', False), (16, 2048, 'render', 90, '422', 3, True), (16, 2048, 'smooth', 90, '444', 0, False),
]


def content(kind, H, W, seed):
    if kind == 'smooth':
        return J.content('ramp', H, W, seed)
    return J.content(kind, H, W, seed)


def restart_of(H, W, sub, r):
    mx, my, _ = D.geometry(H, W, sub)
    return mx if r == 'row' else mx * my + 7 if r == 'all' else r


def pil_file(rgb, quality, sub, restart, optimize):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, 'JPEG', quality=quality, subsampling={'444': 0, '422': 1, '420': 2}[sub], optimize=optimize,
                              restart_marker_blocks=restart)
    return b.getvalue()


def pil_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def main():
    import PIL
    from PIL import features
    out, params, kinds = {}, [], []
    for i, (H, W, kind, quality, sub, r, optimize) in enumerate(CASES):
        restart = restart_of(H, W, sub, r)
        data = pil_file(content(kind, H, W, 200 + i), quality, sub, restart, optimize)
        ref, p = pil_pixels(data), D.parse(data)
        bad = J.gate_equal(f'case {i} {H}x{W} {kind} q{quality} {sub} restart {restart} optimize {optimize}', D.decode(data), ref)
        if bad or (p['H'], p['W'], p['sub'], p['restart']) != (H, W, sub, restart):
            sys.exit(f'the numpy reference differs from Pillow, nothing written: {bad}')
        out[f'file_{i}'], out[f'rgb_{i}'] = np.frombuffer(data, np.uint8), ref
        params.append((H, W, quality, D.SUB_CODE[sub], restart, int(optimize)))
        kinds.append(kind)
    out['params'], out['kinds'] = np.array(params, np.int32), np.array(kinds)
    out['versions'] = np.array([f'Pillow {PIL.__version__}', f'libjpeg-turbo {features.version("libjpeg_turbo")}', f'jpeglib {features.version("jpg")}'])
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {len(params)} cases, {os.path.getsize(OUT)} bytes, {" / ".join(out["versions"])}')


if __name__ == '__main__':
    main()
