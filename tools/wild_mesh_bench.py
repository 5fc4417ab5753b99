"""What in-the-wild mesh recovery costs on one MI355X, next to the same results composed from what the package had before.

    python tools/wild_mesh_bench.py [--out profiles/wild_mesh_bench.txt] [--reps 3]

Recorded, no threshold, no ratio promised.  V = 6,890 vertices (a synthetic model of SMPL's size), the full backbone in its default
precision (bf16), a seeded head, 4,960 frames per person (20 clips x 243 + a tail of 100), flip on:
  (1) `wild.infer_mesh` for one and for four persons (input stage and the copy of the results to the host included) against the
      reference's loop through the same model: `mesh.flip_average` per clip at batch 1 with a `.cpu()` of vertices and joints per clip
      (infer_wild_mesh.py:108-146; its input stage NOT included).  Host clock around work that ends in a synchronise, median (min .. max) of
      alternating passes after one warm-up pass of each.
  (2) `mbx_wild_mesh` alone at 64 clips x 243 frames against two `SMPLLayer.forward_kp` calls + the torch mean + the copy into the stitched
      rows, on the same parameters: HIP events, median (min .. max) of 20 passes after 5 warm-up passes, and the peak device memory of each.
  (3) `mbx_scale_fit` on 84,320 points (one person of 4,960 frames), with its iteration count; next to it the same iteration in numpy on
      this host, and the host times of the reference's 400-start `solve_scale` from the run of tools/mint_wild_mesh.py -- those were taken
      on the BUILD machine's CPU (scipy 1.15.3), not on this one, on problems of 17 to 1,020 points."""
from __future__ import annotations

import argparse
import os
import sys
import time
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                  # noqa: E402  (the model configurations)
from tests import mesherr as ME              # noqa: E402
from tests import wilderr as WE              # noqa: E402
from tests import wildmesherr as WM          # noqa: E402
from tools.smpl_bench import timed           # noqa: E402

CLIP, CLIPS, TAIL, V = 243, 20, 100, 6890
MINT_HOST = 'reference solve_scale (400 least_squares starts), BUILD machine CPU, scipy 1.15.3: 340 points 7 s, 1,020 points 16 s, 17 points 19 s'


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/wild_mesh_bench.py measures on the ROCm device; none found')
    from motionbert_amd import DSTformer, wild
    from motionbert_amd.mesh import MeshRegressor, flip_average
    from motionbert_amd.smpl import SMPLLayer, SMPLModel, rodrigues
    dev = torch.device('cuda', 0)
    F = CLIPS * CLIP + TAIL
    lines = [f'in-the-wild mesh recovery on {torch.cuda.get_device_name(0)}: V = {V}, {F} frames per person ({CLIPS} clips x {CLIP} + a tail of {TAIL}), flip on']

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def fmt(t, unit=1e3, name='ms'):
        return f'{t[0] * unit:10.2f} {name} ({t[1] * unit:.2f} .. {t[2] * unit:.2f})'

    torch.manual_seed(0)
    layer = SMPLLayer(SMPLModel.synthetic(V, 1))
    pose, shape = ME.mean_params()
    net = MeshRegressor(DSTformer(norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **bench.FULL), smpl=layer, init_pose=pose, init_shape=shape,
                        J_regressor=layer.J_regressor_h36m, dim_rep=512, hidden_dim=2048, dropout_ratio=0.).to(dev).eval()
    with torch.no_grad():
        net.head.head_pose.weight.mul_(40.0)
        net.head.head_shape.weight.mul_(40.0)
    # ---- (1) the two loops
    say(f'(1) detections to meshes, full backbone, precision {net.backbone.precision}; host clock, median (min .. max) of {args.reps} alternating passes:')
    for n in (1, 4):
        tracks = {k: WE.detections(F, 9000 + k) for k in range(n)}
        motions = {k: WE.input_ref(v, None, [1, 1])[0] for k, v in tracks.items()}

        def path_a():
            return wild.infer_mesh(net, layer, tracks, clip_len=CLIP)

        def path_b():
            res = {}
            with torch.no_grad():
                for k, m in motions.items():
                    vs, ks = [], []
                    for i in range(0, len(m), CLIP):
                        out = flip_average(net, layer, torch.from_numpy(m[i:i + CLIP])[None].to(dev))[0]
                        vs.append(out['verts'][0].float().cpu().numpy())
                        ks.append(out['kp_3d'][0].float().cpu().numpy())
                    res[k] = dict(verts=np.concatenate(vs), kp_3d=np.concatenate(ks))
            return res

        a, b = path_a(), path_b()                                        # warm every shape of both paths
        top = max(float(np.abs(b[k]['verts']).max()) for k in tracks)
        worst = max(float(np.abs(a[k]['verts'].astype(np.float64) - b[k]['verts']).max()) for k in tracks)
        del a, b
        ta, tb = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            path_a()
            ta.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            path_b()
            tb.append(time.perf_counter() - t0)
        sa, sb = stats(ta), stats(tb)
        mb = n * F * V * 12 / 1e6
        say(f'  {n} person(s), {n * (CLIPS + 1)} clips, vertices {mb:.0f} MB: A wild.infer_mesh (input stage, copy to the host included) {fmt(sa)}   {n * F / sa[0]:9.0f} frames/s')
        say(f'  {n} person(s), {n * (CLIPS + 1)} clips, vertices {mb:.0f} MB: B flip_average per clip at batch 1 + .cpu() per clip      {fmt(sb)}   {n * F / sb[0]:9.0f} frames/s')
        say(f'  {n} person(s): B / A {sb[0] / sa[0]:.2f}x; worst |A - B| of the vertices {worst:.3e} mm of {top:.0f} mm (the network runs at different batch sizes, bf16)')
    # the device part of A without the final copy
    tracks = {k: WE.detections(F, 9000 + k) for k in range(4)}
    wild.infer_mesh(net, layer, tracks, clip_len=CLIP, to_host=False)
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wild.infer_mesh(net, layer, tracks, clip_len=CLIP, to_host=False)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    say(f'  4 persons: A with to_host=False (results stay on the device)                        {fmt(stats(ts))}')
    torch.cuda.empty_cache()
    # ---- (2) the paired kernel alone
    n, T = 64, CLIP
    nT = n * T
    g = torch.Generator().manual_seed(2)
    ops = wild.hip_ops.get()
    with torch.no_grad():
        aa = (0.4 * torch.randn(nT, 72, generator=g)).to(dev)
        betas = torch.randn(nT, 10, generator=g).to(dev)
        rot_a = rodrigues(aa.reshape(-1, 3)).view(nT, 24, 9).contiguous()
        theta_b = torch.cat([(0.4 * torch.randn(nT, 72, generator=g)).to(dev), torch.randn(nT, 10, generator=g).to(dev)], 1).contiguous()
        dst = (torch.arange(n, dtype=torch.int32) * T).to(dev)
        Q = layer.J_regressor_h36m.to(dev)
        tensors = layer.to(dev).model_tensors()
        from motionbert_amd.mesh import flip_thetas_batch

        def paired():
            verts = torch.empty(nT, V, 3, device=dev)
            kp = torch.empty(nT, 17, 3, device=dev)
            ops.wild_mesh(tensors, Q, rot_a, betas, None, theta_b, 1000.0, dst, int((n - 1) * T), T, verts, kp, None)
            return verts, kp

        def composed():
            verts = torch.empty(nT, V, 3, device=dev)
            kp = torch.empty(nT, 17, 3, device=dev)
            va, ka = layer.forward_kp(betas, rot_a.view(nT, 24, 3, 3), Q, 1000.0)
            pb = flip_thetas_batch(theta_b[None, :, :72])[0]
            vb, kb = layer.forward_kp(theta_b[:, 72:].contiguous(), rodrigues(pb.reshape(-1, 3)).view(nT, 24, 3, 3), Q, 1000.0)
            verts.copy_((va + vb) * 0.5)
            kp.copy_((ka + kb) * 0.5)
            return verts, kp

        res = {}
        for name, fn in (('mbx_wild_mesh (prepare, chain, paired vertex kernel, keypoint finish)', paired),
                         ('2 x forward_kp + rodrigues + torch mean + copy into the stitched rows', composed)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t = timed(fn)
            peak = (torch.cuda.max_memory_allocated() - base) / 1e6
            res[name] = (t, peak, fn())
        say(f'(2) the paired SMPL stage alone, {n} clips x {T} = {nT} frames, verts {nT * V * 12 / 1e6:.0f} MB + kp; HIP events, median (min .. max) of 20 passes:')
        for name, (t, peak, _) in res.items():
            say(f'  {name:76s} {fmt(t, 1.0)}   peak device memory above the inputs {peak:8.0f} MB')
        (ta, pa, oa), (tb, pb_, ob) = res.values()
        diff = float((oa[0] - ob[0]).abs().max())
        say(f'  composed / paired: time {tb[0] / ta[0]:.2f}x, peak memory {pb_ / pa:.2f}x; worst |difference| of the vertices {diff:.3e} mm; '
            f'the paired kernel writes {nT * V * 12 / 1e6:.0f} MB of vertices once: {nT * V * 12 / (ta[0] * 1e-3) / 1e12:.2f} TB/s, far from the memory bound -- '
            f'it is bound by the {2 * nT * V * 217 * 6 / 1e9:.0f} GFLOP of the two pose and shape blends ({2 * nT * V * 217 * 6 / (ta[0] * 1e-3) / 1e12:.1f} TFLOP/s fp32 on the vector unit)')
        del res, oa, ob
    torch.cuda.empty_cache()
    # ---- (3) the scale fit
    ref, kp = WM.fit_problem('p84320')
    ref_d, kp_d = torch.from_numpy(ref).to(dev), torch.from_numpy(kp).to(dev)
    ptr = torch.tensor([0, len(ref)], dtype=torch.int32).to(dev)
    fit = torch.empty(1, 6, dtype=torch.float64, device=dev)
    t = timed(lambda: ops.scale_fit(ref_d, kp_d, ptr, fit))
    row = fit.cpu().numpy()[0]
    t0 = time.perf_counter()
    host = WM.fit_row(ref, kp)
    th = time.perf_counter() - t0
    say(f'(3) mbx_scale_fit, one track of {len(ref)} frames = {17 * len(ref)} points: {fmt(t, 1.0)}, {int(row[5])} iterations, scale {row[0]!r}, '
        f'objective {row[4]!r}')
    say(f'  the same iteration in numpy on this host (the CPU of the GPU machine): {th * 1e3:.0f} ms, {int(host[5])} iterations, scale {host[0]!r}; '
        f'|device - numpy| / scale {abs(row[0] - host[0]) / abs(host[0]):.2e}')
    say(f'  {MINT_HOST}')
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
