"""What the mesh-recovery kernels cost next to the torch operations they replace, on one MI355X.

    python tools/mesh_bench.py [--out profiles/mesh_bench.txt]

HIP events around 20 timed passes after 5 warm-up passes (median, and the spread); recorded, no threshold.  All at 128 clips x 16 frames,
the batch of configs/mesh/*.yaml: F = 2,048 frames, M = 49,152 joints, V = 6,890 vertices.
  (i)   the head's rotation chain, forward + backward (mbx_rot6d_theta_fwd + _bwd) -- against the same operations in torch on the same
        device (tests/mesherr.rot_chain: 6D -> rotation matrix -> quaternion cases -> axis-angle, from the formulas) and autograd;
  (ii)  the three parameter losses and their gradient (mbx_mesh_param_loss, L1) -- against tests/mesherr.param_losses + autograd;
  (iii) mbx_mesh_errors -- against the torch operations of compute_error (MPVE and the 17-joint MPJPE on the device; the reference also
        copies every vertex to the host for evaluate_mesh and aligns per frame in numpy, which is not timed here), and the bytes per
        second it achieves against the 2 x F x V x 12 bytes of vertices it must read.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import mesherr as ME      # noqa: E402


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from motionbert_amd import hip_ops
    ops = hip_ops.get()
    dev = 'cuda'
    N, T, V = 128, 16, 6890
    F, M = N * T, N * T * 24
    lines = [f'mesh kernels on {torch.cuda.get_device_name(0)}: HIP events, median (min .. max) of 20 passes after 5 warm-up passes; '
             f'{N} x {T} frames']

    def say(name, t):
        lines.append(f'  {name:84s} {t[0] * 1e3:9.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f})')
        print(lines[-1], flush=True)
        return t[0]

    # (i) rotation chain
    x6, drot, daa = [a.to(dev) for a in ME.rot_inputs(M, 1)]
    R, aa, dx = torch.empty(M, 9, device=dev), torch.empty(M, 3, device=dev), torch.empty(M, 6, device=dev)
    lines.append(f'(i) rotation chain 6D -> rotation matrix -> quaternion -> axis-angle, M = {M} joints')

    def chain():
        ops.rot6d_theta_fwd(x6, R, aa)
        ops.rot6d_theta_bwd(x6, drot, daa, dx)
    a = say('mbx_rot6d_theta_fwd + mbx_rot6d_theta_bwd: 2 launches', timed(chain))
    say('mbx_rot6d_theta_fwd alone', timed(lambda: ops.rot6d_theta_fwd(x6, R, aa)))
    xt = x6.clone().requires_grad_(True)

    def torch_chain():
        xt.grad = None
        r, t = ME.rot_chain(xt)
        ((r.reshape(-1, 9) * drot).sum() + (t * daa).sum()).backward()
    b = say('torch: the same chain in torch operations (fp32) + autograd backward', timed(torch_chain))
    lines.append(f'      ratio {b / a:.1f}x')

    # (ii) parameter losses
    pred, gt = [a.to(dev) for a in ME.theta_inputs(F, 2)]
    losses, dth = torch.empty(4, device=dev), torch.empty(F, 82, device=dev)
    lines.append(f'(ii) loss_pose (batch_rodrigues on both sides), loss_shape, loss_norm and d(weighted sum)/d theta, L1, F = {F} frames')
    a = say('mbx_mesh_param_loss (losses + dtheta): 2 launches', timed(lambda: ops.mesh_param_loss(pred, gt, 1, ME.LAMBDAS3, losses, dth)))
    say('mbx_mesh_param_loss (losses only)', timed(lambda: ops.mesh_param_loss(pred, gt, 1, ME.LAMBDAS3, losses, None)))
    pt = pred.clone().requires_grad_(True)

    def torch_losses():
        pt.grad = None
        ls = ME.param_losses(pt, gt, 1)
        sum(w * v for w, v in zip(ME.LAMBDAS3, ls)).backward()
    b = say('torch: the same losses in torch operations (fp32) + autograd backward', timed(torch_losses))
    lines.append(f'      ratio {b / a:.1f}x')

    # (iii) errors
    g = torch.Generator(device=dev).manual_seed(3)
    vg = 300.0 * torch.randn(F, V, 3, device=dev, generator=g)
    vp = vg + 20.0 * torch.randn(F, V, 3, device=dev, generator=g)
    kg = 300.0 * torch.randn(F, 17, 3, device=dev, generator=g)
    kp = kg + 20.0 * torch.randn(F, 17, 3, device=dev, generator=g)
    err = torch.empty(5, F, dtype=torch.float64, device=dev)
    nbytes = 2 * F * V * 12
    lines.append(f'(iii) per-frame errors at V = {V}: {nbytes / 1e6:.0f} MB of vertices to read')
    a = say('mbx_mesh_errors (MPVE, MPJPE 17 / 14, PA-MPJPE 17 / 14; fp64)', timed(lambda: ops.mesh_errors(vp, vg, kp, kg, err)))
    lines.append(f'      {nbytes / (a * 1e-3) / 1e12:.2f} TB/s of vertex reads')
    say('mbx_mesh_errors without vertices (the four joint rows)', timed(lambda: ops.mesh_errors(None, None, kp, kg, err)))

    def torch_errors():
        a_, b_ = vp - kp[:, :1], vg - kg[:, :1]
        mpve = torch.sqrt(((a_ - b_) ** 2).sum(-1)).mean(-1)
        p, q = kp - kp[:, :1], kg - kg[:, :1]
        return torch.sqrt(((p - q) ** 2).sum(-1)).mean(-1).mean(), mpve.mean()
    b = say('torch: compute_error (MPVE + 17-joint MPJPE only, fp32, on the device)', timed(torch_errors))
    lines.append(f'      ratio {b / a:.1f}x (for two of the five rows, in fp32)')
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
