"""What reading Motion-JPEG on the device costs per frame on one MI355X, against decoding on the host and uploading raw frames.

    python tools/jpeg_dec_bench.py [--out profiles/jpeg_dec_bench.txt] [--frames 32] [--reps 5]

In one process, after one warm-up pass of everything, alternating repetitions, the median of each, wall clock around the call and a
synchronize (wrapper, host parser and upload included).  Material: files this package's own writer produces (encode_jpeg + MJPEGWriter, read
back through MJPEGReader) at 1920 x 1080 and at 1024 x 1024, 4:2:0, quality 90, one MCU row per restart interval; content: a ramp per channel
that moves from frame to frame plus noise of a few levels (tests/sceneerr.backdrop's formula, on the device).
  (a) decode_jpeg from the host's compressed bytes to rgb on the device, against Pillow (libjpeg-turbo) decoding the same files on this
      machine's host plus the upload of the raw frames;
  (b) the three kernels on their own (mbx_jpeg_dec_index, mbx_jpeg_dec_entropy, mbx_jpeg_dec_pixels) and the bytes per second of the pixel
      stage (coefficients read, planes written and read, rgb written) against the 6.29 TB/s of a float4 copy;
  (c) the same frames without restart markers: one interval, so one lane, per frame -- what a file written by ffmpeg presents;
  (d) scene_video over a reader against scene_video over a resident tensor of the same decoded frames.
Condition fixed in advance, (a): the device median per frame is not above the Pillow-plus-upload median.  (b) to (d) are recorded."""
from __future__ import annotations

import argparse
import io
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import hip_ops          # noqa: E402
from motionbert_amd import render as R      # noqa: E402
from motionbert_amd import video as V       # noqa: E402
from tests import skelerr as SE             # noqa: E402
from tools.render_bench import once         # noqa: E402

QUALITY, SUB, COPY_RATE = 90, '420', 6.29e12


def material(F, H, W, dev):
    i, j = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
    t = torch.arange(F, device=dev)[:, None, None]
    rgb = torch.stack([(3 * i + 5 * j + 40 * t) % 200, (7 * i + 2 * j + 90 * t) % 230, (i * j + 17 * t) % 250], -1)
    return (rgb + torch.randint(0, 5, rgb.shape, device=dev)).to(torch.uint8).contiguous()


def write_and_read(path, rgb, fps, restart=None):
    H, W = rgb.shape[1:3]
    data, off = V.encode_jpeg(rgb, QUALITY, SUB, restart)
    with V.MJPEGWriter(path, W, H, fps) as w:
        w.write(data.cpu().numpy(), off.cpu().numpy())
    with V.MJPEGReader(path) as r:
        return [r.frame_bytes(f) for f in range(r.frames)]


def pillow_route(files, dev):
    from PIL import Image
    host = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert('RGB')) for f in files])
    return torch.from_numpy(host).to(dev)


def stats(ms, F):
    m = statistics.median(ms)
    return f'{m:9.2f} ms ({min(ms):.2f} .. {max(ms):.2f})   {m / F:8.3f} ms/frame  {F / m * 1e3:8.0f} frames/s'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'jpeg_dec_bench needs the GPU: there is no CPU timing'
    try:
        import PIL
        from PIL import features
        pil = f'Pillow {PIL.__version__}, libjpeg-turbo {features.version("libjpeg_turbo")}'
    except ImportError:
        pil = None
    dev, F, ops, tmp = torch.device('cuda'), args.frames, hip_ops.get(), tempfile.mkdtemp()
    lines = [f'device JPEG decoder on {torch.cuda.get_device_name(0)}: wall clock around call + synchronize, median (min .. max) of {args.reps} '
             f'alternating repetitions after one warm-up pass; {F} frames per call, quality {QUALITY}, 4:2:0; host decoder: {pil or "Pillow does not import"}']
    ok = pil is not None
    for H, W in ((1080, 1920), (1024, 1024)):
        rgb = material(F, H, W, dev)
        files = write_and_read(os.path.join(tmp, 'in.avi'), rgb, 25)
        whole = write_and_read(os.path.join(tmp, 'whole.avi'), rgb, 25, restart=65535)
        mx, my, bpm = V.dec_geometry(H, W, SUB)
        total = sum(len(f) for f in files)
        lines.append(f'{H} x {W}: {total / F:.0f} bytes/frame compressed = 1 / {3 * H * W * F / total:.1f} of raw; {my} restart intervals of {mx} MCUs per frame')
        # ------------------------------------------------------------------------------------ (a), (c)
        runs = [('decode_jpeg', lambda: V.decode_jpeg(files, device=dev)), ('decode_jpeg, no restart markers', lambda: V.decode_jpeg(whole, device=dev))]
        if pil:
            runs.append(('Pillow + upload', lambda: pillow_route(files, dev)))
            assert torch.equal(runs[0][1](), runs[2][1]()), 'the device decoder and Pillow disagree'
        for _, fn in runs:
            fn()
        ms = {k: [] for k, _ in runs}
        for r in range(args.reps):
            for k, fn in runs:
                ms[k].append(once(fn))
            print(f'{H} x {W} repetition {r}: ' + '  '.join(f'{k} {ms[k][-1]:.1f} ms' for k, _ in runs), flush=True)
        for k, _ in runs:
            lines.append(f'(a) {k:32s} {stats(ms[k], F)}' if 'no restart' not in k else f'(c) {k:32s} {stats(ms[k], F)}')
        if pil:
            d, p = statistics.median(ms['decode_jpeg']), statistics.median(ms['Pillow + upload'])
            lines.append(f'    device / host = {d / p:.3f}: {"met" if d <= p else "NOT met"}')
            ok = ok and d <= p
        # ------------------------------------------------------------------------------------ (b)
        for label, fs in (('row intervals', files), ('one interval', whole)):
            facts = V.parse_jpeg(fs[0])
            n_int = -(-mx * my // facts['restart']) if facts['restart'] else 1
            off = np.concatenate([[0], np.cumsum([len(f) for f in fs])])
            data = torch.from_numpy(np.frombuffer(b''.join(fs), np.uint8).copy()).to(dev)
            scans = torch.tensor([[off[f] + V.parse_jpeg(x)['scan'][0], off[f] + V.parse_jpeg(x)['scan'][1]] for f, x in enumerate(fs)], device=dev)
            pos = torch.empty(F, n_int + 1, dtype=torch.int64, device=dev)
            status = torch.empty(F, n_int, dtype=torch.int32, device=dev)
            coef = torch.empty(F, mx * my, bpm, 64, dtype=torch.int16, device=dev)
            out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
            tables, ws = ops.jpeg_dec_tables(facts['dht']).to(dev), ops.jpeg_dec_ws(F, H, W, 1, dev)
            kern = [('index', lambda: ops.jpeg_dec_index(data, scans, n_int, pos, status)),
                    ('entropy', lambda: ops.jpeg_dec_entropy(data, pos, tables, H, W, 1, facts['restart'], coef, status)),
                    ('pixels', lambda: ops.jpeg_dec_pixels(coef, facts['q'], H, W, 1, out, ws))]
            for _, fn in kern:
                fn()
            assert not status.any() and torch.equal(out, runs[0][1]())
            km = {k: [] for k, _ in kern}
            for r in range(args.reps):
                for k, fn in kern:
                    km[k].append(once(fn))
            for k, _ in kern:
                lines.append(f'(b) {label:14s} {k:8s} {stats(km[k], F)}')
            moved = coef.numel() * 2 + 2 * ws.numel() + out.numel()
            rate = moved / (statistics.median(km['pixels']) * 1e-3)
            lines.append(f'    pixel stage: {moved / F:.0f} bytes/frame moved, {rate / 1e12:.3f} TB/s = {rate / COPY_RATE:.1%} of a float4 copy')
        # ------------------------------------------------------------------------------------ (d)
        ids = {k: np.arange(F) for k in range(4)}
        x3d = {k: (np.array([W * (k + 1) / 5, H / 2, 0.0]) + H / 4 * SE.POSE[None] + np.arange(F)[:, None, None] * [2.0, 0, 0]).astype(np.float32) for k in ids}
        table = R.scene_table(ids)
        resident = V.decode_jpeg(files, device=dev)
        with V.MJPEGReader(os.path.join(tmp, 'in.avi')) as reader:
            sv = [('scene_video over a reader', lambda: V.scene_video(os.path.join(tmp, 'a.avi'), x3d, table, W, H, 25, background=reader, chunk=16)),
                  ('scene_video over a tensor', lambda: V.scene_video(os.path.join(tmp, 'b.avi'), x3d, table, W, H, 25, background=resident, chunk=16))]
            for _, fn in sv:
                fn()
            assert open(os.path.join(tmp, 'a.avi'), 'rb').read() == open(os.path.join(tmp, 'b.avi'), 'rb').read()
            sm = {k: [] for k, _ in sv}
            for r in range(args.reps):
                for k, fn in sv:
                    sm[k].append(once(fn))
        for k, _ in sv:
            lines.append(f'(d) {k:32s} {stats(sm[k], F)}')
        lines.append(f'    reader / tensor = {statistics.median(sm[sv[0][0]]) / statistics.median(sm[sv[1][0]]):.3f} in time; the tensor route holds '
                     f'{resident.numel()} bytes of background on the device, the reader route {min(16, F) * H * W * 3}')
    lines.append('acceptance (decode_jpeg with its upload not slower per frame than Pillow on this host plus the upload of raw frames, both sizes): '
                 + ('met' if ok else 'NOT met'))
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
