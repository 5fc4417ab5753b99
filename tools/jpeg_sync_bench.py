"""What the self-synchronising entropy decode (csrc/jpeg_sync.hip) costs per frame on one MI355X for Motion-JPEG WITHOUT restart markers, the
files ffmpeg, cameras and capture cards write, against the one-lane-per-interval route on the same files and against the host.

    python tools/jpeg_sync_bench.py [--out profiles/jpeg_sync_bench.txt] [--frames 32] [--reps 5] [--stage-only] [--sync-bytes S]

In one process, after one warm-up pass of everything, alternating repetitions, the median of each, wall clock around the call and a
synchronize (wrapper, host parser and upload included).  Material: tools/jpeg_dec_bench.py's (a ramp per channel that moves from frame to
frame plus noise of a few levels, quality 90, 4:2:0) at 1920 x 1080 and 1024 x 1024, every frame ONE interval.
  (a) decode_jpeg(entropy='sync'), decode_jpeg(entropy='interval') and Pillow (libjpeg-turbo) on this machine's host plus the upload of the
      raw frames, all on the same files;
  (b) the entropy stage alone, both routes; the kernels of the new one (a torch.profiler trace of one call); the rounds per chunk of the
      speculation and of the verification, and the route counts, read from the workspace and from `route`;
  (c) a uniform white 1080p frame: every MCU is the same 32 bits, a wrong block index never heals, and its scan is one chunk, which walks
      its whole induction lane by lane -- the worst case of the rounds; beside it the one-lane route on the same frame, which 'auto' gives up;
  (d) both routes on the files with one MCU row per interval (where 'auto' takes 'interval'): the crossover for a later change of that rule.
Conditions fixed in advance, (a): the 'sync' median is not above the 'interval' median, and not above the Pillow-plus-upload median.
--stage-only measures (b) alone: for builds of the library with another MBX_JPEG_SYNC_BYTES (MBX_LIB names the library, --sync-bytes its S; without the flag S is include/mbx.h's)."""
from __future__ import annotations

import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd import hip_ops                                      # noqa: E402
from motionbert_amd import video as V                                   # noqa: E402
from tools.jpeg_dec_bench import QUALITY, SUB, material, pillow_route, stats, write_and_read      # noqa: E402
from tools.render_bench import once                                     # noqa: E402

_HEADER = open(os.path.join(ROOT, 'include', 'mbx.h')).read()
SYNC_BYTES = int(re.search(r'#define MBX_JPEG_SYNC_BYTES (\d+)', _HEADER).group(1))      # what the library is built with, unless -D said otherwise
CH = int(re.search(r'#define MBX_JPEG_SYNC_CHUNK (\d+)', _HEADER).group(1))


class Stage:
    """the entropy stage of F files of one header, both routes, on buffers made once"""

    def __init__(self, ops, files, H, W, dev, S):
        self.ops, self.F, self.S = ops, len(files), S
        mx, my, bpm = V.dec_geometry(H, W, SUB)
        facts = [V.parse_jpeg(f) for f in files]
        p = facts[0]
        self.n_int = n_int = -(-mx * my // p['restart']) if p['restart'] else 1
        off = np.concatenate([[0], np.cumsum([len(f) for f in files])])
        data = torch.from_numpy(np.frombuffer(b''.join(files), np.uint8).copy()).to(dev)
        scans = torch.tensor([[off[f] + q['scan'][0], off[f] + q['scan'][1]] for f, q in enumerate(facts)], device=dev)
        self.longest = longest = max(q['scan'][1] - q['scan'][0] for q in facts)
        pos = torch.empty(self.F, n_int + 1, dtype=torch.int64, device=dev)
        self.status0 = torch.empty(self.F, n_int, dtype=torch.int32, device=dev)
        ops.jpeg_dec_index(data, scans, n_int, pos, self.status0)
        self.status, self.route = self.status0.clone(), torch.zeros_like(self.status0)
        self.coef = torch.empty(self.F, mx * my, bpm, 64, dtype=torch.int16, device=dev)
        tables = ops.jpeg_dec_tables(p['dht']).to(dev)
        self.ws = ops.jpeg_dec_sync_ws(self.F, n_int, longest, dev)
        self.sync = lambda: ops.jpeg_dec_entropy_sync(data, pos, tables, H, W, 1, p['restart'], longest, self.coef, self.status, self.route, self.ws)
        self.interval = lambda: ops.jpeg_dec_entropy(data, pos, tables, H, W, 1, p['restart'], self.coef, self.status)
        self.lengths = (pos[:, 1:] - 2 - pos[:, :-1]).cpu().numpy()

    def rounds(self):
        """(rounds of A, rounds of B) of every chunk that exists, from the workspace's last array (csrc/jpeg_sync.hip, SyncWs)"""
        max_chunks = max(1, -(-(-(-self.longest // self.S)) // CH))
        M = self.F * self.n_int * max_chunks
        r = self.ws[M * CH * 32 + M * 44:M * CH * 32 + M * 52].view(torch.int32).view(self.F * self.n_int, max_chunks, 2).cpu().numpy()
        n_chunk = -(-(-(-self.lengths.reshape(-1) // self.S)) // CH)
        live = np.arange(max_chunks)[None] < n_chunk[:, None]
        return r[..., 0][live], r[..., 1][live]

    def kernels(self):
        """name -> device microseconds of one call of the new route, from torch.profiler; None where it records no kernels"""
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                self.sync()
                torch.cuda.synchronize()
            out = {}
            for e in prof.key_averages():
                t = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0)
                if 'jpeg_sync' in e.key and t:
                    out[e.key.split('jpeg_sync_')[1].split('_kernel')[0]] = t / max(e.count, 1)
            return out or None
        except Exception as e:                                            # a measurement aid: the medians do not depend on it
            print(f'torch.profiler: {type(e).__name__}: {e}', flush=True)
            return None


def describe(stage, F, lines, reps, label):
    runs = [('sync', stage.sync), ('interval', stage.interval)]
    stage.sync()
    sync_coef, route = stage.coef.clone(), stage.route.cpu().numpy()
    stage.status.copy_(stage.status0)
    stage.interval()
    assert torch.equal(sync_coef, stage.coef) and not stage.status.any(), 'the two routes disagree'
    ms = {k: [] for k, _ in runs}
    for _ in range(reps):
        for k, fn in runs:
            ms[k].append(once(fn))
    for k, _ in runs:
        lines.append(f'(b) {label:14s} entropy {k:9s} {stats(ms[k], F)}')
    stage.sync()
    torch.cuda.synchronize()
    ra, rb = stage.rounds()
    lines.append(f'    {label}: {len(ra)} chunks of {CH} x {stage.S} bytes; rounds per chunk: speculation mean {ra.mean():.1f} max {ra.max()}, verification mean '
                 f'{rb.mean():.1f} max {rb.max()}; route counts {({int(v): int((route == v).sum()) for v in np.unique(route)})}')
    kern = stage.kernels()
    lines.append('    kernels of one call (us): ' + ('  '.join(f'{k} {v:.0f}' for k, v in kern.items()) if kern else 'not recorded (no kernel trace in this process)'))
    return statistics.median(ms['sync'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stage-only', action='store_true')
    ap.add_argument('--sync-bytes', type=int, default=SYNC_BYTES, help='only for a library built with -DMBX_JPEG_SYNC_BYTES=...')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'jpeg_sync_bench needs the GPU: there is no CPU timing'
    try:
        import PIL
        from PIL import features
        pil = f'Pillow {PIL.__version__}, libjpeg-turbo {features.version("libjpeg_turbo")}'
    except ImportError:
        pil = None
    dev, F, ops, tmp = torch.device('cuda'), args.frames, hip_ops.get(), tempfile.mkdtemp()
    lines = [f'self-synchronising JPEG entropy decode on {torch.cuda.get_device_name(0)}, S = {args.sync_bytes} bytes, library {os.path.basename(hip_ops.LIB_PATH)}: '
             f'wall clock around call + synchronize, median (min .. max) of {args.reps} alternating repetitions after one warm-up pass; {F} frames per '
             f'call, quality {QUALITY}, 4:2:0, ONE interval per frame; host decoder: {pil or "Pillow does not import"}']
    ok = pil is not None or args.stage_only
    for H, W in ((1080, 1920), (1024, 1024)):
        rgb = material(F, H, W, dev)
        whole = write_and_read(os.path.join(tmp, 'whole.avi'), rgb, 25, restart=65535)
        lines.append(f'{H} x {W}: {sum(len(f) for f in whole) / F:.0f} bytes/frame compressed, no restart markers inside the frame')
        if not args.stage_only:
            runs = [("decode_jpeg(entropy='sync')", lambda: V.decode_jpeg(whole, device=dev, entropy='sync')),
                    ("decode_jpeg(entropy='interval')", lambda: V.decode_jpeg(whole, device=dev, entropy='interval'))]
            if pil:
                runs.append(('Pillow + upload', lambda: pillow_route(whole, dev)))
            first = [fn() for _, fn in runs]                              # the warm-up pass
            assert all(torch.equal(first[0], x) for x in first[1:]), 'the routes disagree'
            del first
            ms = {k: [] for k, _ in runs}
            for r in range(args.reps):
                for k, fn in runs:
                    ms[k].append(once(fn))
                print(f'{H} x {W} repetition {r}: ' + '  '.join(f'{k} {ms[k][-1]:.1f} ms' for k, _ in runs), flush=True)
            for k, _ in runs:
                lines.append(f'(a) {k:32s} {stats(ms[k], F)}')
            med = {k: statistics.median(v) for k, v in ms.items()}
            s, i = med[runs[0][0]], med[runs[1][0]]
            lines.append(f'    sync / interval = {s / i:.3f}: {"met" if s <= i else "NOT met"}')
            ok = ok and s <= i
            if pil:
                lines.append(f'    sync / host = {s / med["Pillow + upload"]:.3f}: {"met" if s <= med["Pillow + upload"] else "NOT met"}')
                ok = ok and s <= med['Pillow + upload']
        describe(Stage(ops, whole, H, W, dev, args.sync_bytes), F, lines, args.reps, 'one interval')
        if not args.stage_only:
            rows = write_and_read(os.path.join(tmp, 'rows.avi'), rgb, 25)
            describe(Stage(ops, rows, H, W, dev, args.sync_bytes), F, lines, args.reps, 'row intervals')
            if H == 1080:
                white = write_and_read(os.path.join(tmp, 'white.avi'), torch.full((1, H, W, 3), 255, dtype=torch.uint8, device=dev), 25, restart=65535)
                st = Stage(ops, white, H, W, dev, args.sync_bytes)
                wm, wi = [], []
                st.sync()
                st.interval()
                for _ in range(args.reps):
                    wm.append(once(st.sync))
                    wi.append(once(st.interval))
                ra, rb = st.rounds()
                lines.append(f'(c) white 1080p, one frame, entropy sync     {stats(wm, 1)}; scan {int(st.lengths.max())} bytes, rounds {ra.tolist()} / {rb.tolist()}, '
                             f'route {st.route.cpu().numpy().reshape(-1).tolist()}')
                lines.append(f'(c) white 1080p, one frame, entropy interval {stats(wi, 1)}')
    if not args.stage_only:
        lines.append("acceptance ('sync' not slower than 'interval' on the same files, and not slower than Pillow on this host plus the upload of raw frames, "
                     'both sizes): ' + ('met' if ok else 'NOT met'))
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
