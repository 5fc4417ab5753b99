"""What the mesh targets cost on one MI355X, next to what the reference's loop pays for them.

    python tools/mesh_gt_bench.py [--out profiles/mesh_gt_bench.txt] [--verts 6890]

HIP events around 20 timed passes after 5 warm-up passes (median, and the spread: the method of tools/smpl_bench.py); recorded, no
threshold.  At 128 clips x 16 frames (the batch of configs/mesh/*.yaml) and 512 clips x 1 frame (the COCO loader), V = 6,890 vertices (a
synthetic model of SMPL's size, weight rows with at most 4 non-zeros as SMPL's), K = 17, millimetres:
  (a) `mesh.mesh_targets`: 2D input, theta, kp_3d and verts from one mbx_mesh_gt, flips drawn on the device; and its parts: the prepare
      kernel alone (`want=('theta',)`), mbx_smpl_fwd on ready rotation matrices (chain + vertex kernel + keypoint finish).  The centring pass
      is reported as the difference  (a) - prepare - mbx_smpl_fwd : an upper bound (it includes the launch and whatever the three other
      kernels lose by running in one call), next to the bytes it must move, 2 x F x V x 12.
  (b) the same result composed from what the package had before: `flip_thetas_batch` / `flip_input` / `torch.where` / `clamp` for the flips,
      `smpl.rodrigues`, `SMPLLayer.forward_kp`, and torch operations for both root subtractions and the theta join.
  (c) a pinned-host-to-device copy of a `verts` batch of that size: what train_mesh.py:172-176 pays per step after its workers ran SMPL.
  (d) the plain smplx-style path (tools/smpl_bench.plain_lbs in fp32, Rodrigues, `* 1000`, the regressor, the subtractions) for ONE clip on
      the host CPU with torch's default thread count: a host measurement of whatever machine this ran on, not of a DataLoader worker of a
      training box."""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd.mesh import flip_input, flip_thetas_batch, mesh_targets      # noqa: E402
from motionbert_amd.smpl import SMPLLayer, SMPLModel, rodrigues                   # noqa: E402
from tools.smpl_bench import plain_lbs, timed                                     # noqa: E402


def composed(layer, pose, shape, m2d, flags):
    """(b): the targets from the operations the package had before mbx_mesh_gt"""
    N, T = pose.shape[:2]
    which = flags.bool().view(N, 1, 1)
    x = m2d.clone()
    x[..., 2] = x[..., 2].clamp(0, 1)
    x = torch.where(which.unsqueeze(-1), flip_input(x), x)
    p = torch.where(which, flip_thetas_batch(pose), pose)
    rot = rodrigues(p.reshape(-1, 3)).view(N * T, 24, 3, 3)
    verts, kp = layer.forward_kp(shape.reshape(N * T, 10), rot, scale=1000.0)
    root = kp[:, :1]
    return x, {'theta': torch.cat([p, shape], -1), 'kp_3d': (kp - root).view(N, T, -1, 3), 'verts': (verts - root).view(N, T, -1, 3)}


def host_clip(model, pose, shape):
    """(d): one clip on the host"""
    m = {k: getattr(model, k) for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'lbs_weights')}
    T = pose.shape[0]
    rot = rodrigues(pose.reshape(-1, 3)).view(T, 24, 3, 3)
    verts = plain_lbs(m, model.parents, shape, rot)[0] * 1000.0
    kp = torch.matmul(model.J_regressor_h36m[None].expand(T, -1, -1), verts)
    return verts - kp[:, :1], kp - kp[:, :1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--verts', type=int, default=6890)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'mesh_gt_bench needs the GPU'
    dev, V = 'cuda', args.verts
    model = SMPLModel.synthetic(V, 1)
    layer = SMPLLayer(model).to(dev)
    lines = [f'mesh targets on {torch.cuda.get_device_name(0)}: HIP events, median (min .. max) of 20 passes after 5 warm-up passes; V = {V}, K = 17']

    def say(name, t):
        lines.append(f'  {name:92s} {t[0] * 1e3:10.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f})')
        print(lines[-1], flush=True)
        return t[0]

    for N, T in ((128, 16), (512, 1)):
        F = N * T
        g = torch.Generator().manual_seed(2)
        pose = (0.5 * torch.randn(N, T, 72, generator=g)).to(dev)
        shape = torch.randn(N, T, 10, generator=g).to(dev)
        m2d = torch.rand(N, T, 17, 3, generator=g).to(dev)
        lines.append(f'{N} clips x {T} frames = {F} frames: verts {F * V * 12 / 1e6:.0f} MB, the inputs {F * (72 + 10 + 51) * 4 / 1e6:.2f} MB')
        with torch.no_grad():
            flags = mesh_targets(layer, pose, shape, flip=True, seed=7, want=(), return_flips=True)[2]
            rot = rodrigues(pose.reshape(-1, 3)).view(F, 24, 3, 3).contiguous()
            betas = shape.reshape(F, 10)
            a = say('(a) mesh_targets: x2d, theta, kp_3d, verts (mbx_mesh_gt, flips drawn)', timed(lambda: mesh_targets(layer, pose, shape, m2d, flip=True, seed=7)))
            prep = say('    prepare kernel alone (x2d, theta)', timed(lambda: mesh_targets(layer, pose, shape, m2d, flip=True, seed=7, want=('theta',))))
            fwd = say('    mbx_smpl_fwd on ready rotations (chain, vertices, keypoint finish): verts + kp', timed(lambda: layer.forward_kp(betas, rot, scale=1000.0)))
            say('    mesh_targets without verts (x2d, theta, kp_3d)', timed(lambda: mesh_targets(layer, pose, shape, m2d, flip=True, seed=7, want=('theta', 'kp_3d'))))
            b = say('(b) composed: torch flips + rodrigues + SMPLLayer.forward_kp + torch subtractions', timed(lambda: composed(layer, pose, shape, m2d, flags)))
            host = torch.empty(F, V, 3).pin_memory()
            dst = torch.empty(F, V, 3, device=dev)
            c = say('(c) pinned host -> device copy of one verts batch', timed(lambda: dst.copy_(host, non_blocking=True)))
        centre = a - prep - fwd
        lines.append(f'      centring pass by difference (a) - prepare - mbx_smpl_fwd: {centre * 1e3:.1f} us for {2 * F * V * 12 / 1e6:.0f} MB read + written '
                     f'({2 * F * V * 12 / max(centre, 1e-9) / 1e9:.2f} TB/s if that were all of it); the estimate was 100 us at 2,048 frames')
        lines.append(f'      (b) / (a) {b / a:.2f}x;  (c) / (a) {c / a:.2f}x;  host link {F * V * 12 / (c * 1e-3) / 1e9:.1f} GB/s')
        del host, dst
    T = 16
    g = torch.Generator().manual_seed(3)
    pose1, shape1 = 0.5 * torch.randn(T, 72, generator=g), torch.randn(T, 10, generator=g)
    with torch.no_grad():
        for _ in range(2):
            host_clip(model, pose1, shape1)
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            host_clip(model, pose1, shape1)
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    lines.append(f'(d) HOST measurement (this machine\'s CPU, {torch.get_num_threads()} torch threads): the plain path for one clip of {T} frames '
                 f'{ts[len(ts) // 2]:.1f} ms (min {ts[0]:.1f}, max {ts[-1]:.1f}) of 7 passes; a batch of 128 clips is 128 of these on the DataLoader workers')
    print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
