"""What the fused SMPL layer costs next to the plain torch formulation, on one MI355X.

    python tools/smpl_bench.py [--out profiles/smpl_bench.txt] [--frames 2048] [--verts 6890]

HIP events around 20 timed passes after 5 warm-up passes (median, and the spread); recorded, no threshold.  At 128 clips x 16 frames, the
batch of configs/mesh/*.yaml: F = 2,048 frames, V = 6,890 vertices (a synthetic model of SMPL's size: motionbert_amd.smpl.SMPLModel.synthetic,
weight rows with at most 4 non-zeros as SMPL's), K = 17 regressed joints, scale 1000.
  (i)   mbx_smpl_fwd alone (verts + kp);
  (ii)  forward + backward with dkp only: the training case (the loss reads the 17 joints);
  (iii) forward + backward with dverts too.
The comparison point, same device and process: linear blend skinning the way smplx writes it (plain_lbs below, the restatement of
tests/smplerr.py in fp32: J_regressor on the shaped vertices, chained 4x4 transforms, the [F,V,4,4] tensor, homogeneous vertices), `* 1000`,
the batched [17,V] matmul, and autograd's backward; with its peak allocated memory.
Bytes and FLOPs below are computed from the shapes: what the algorithm needs, not what a kernel moved."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motionbert_amd.smpl import SMPLLayer, SMPLModel      # noqa: E402


def plain_lbs(m, parents, betas, rot):
    """(vertices [F,V,3], posed joints [F,24,3]) as smplx.lbs.lbs(pose2rot=False) forms them"""
    B, V = betas.shape[0], m['v_template'].shape[0]
    v_shaped = m['v_template'][None] + torch.einsum('bl,mkl->bmk', betas, m['shapedirs'])
    J = torch.einsum('bik,ji->bjk', v_shaped, m['J_regressor'])
    ident = torch.eye(3, dtype=rot.dtype, device=rot.device)
    pose_feature = (rot[:, 1:] - ident).reshape(B, -1)
    v_posed = torch.matmul(pose_feature, m['posedirs']).view(B, -1, 3) + v_shaped
    joints = J[..., None]
    rel = joints.clone()
    rel[:, 1:] = rel[:, 1:] - joints[:, list(parents[1:])]
    tm = torch.cat([torch.nn.functional.pad(rot.reshape(-1, 3, 3), [0, 0, 0, 1]),
                    torch.nn.functional.pad(rel.reshape(-1, 3, 1), [0, 0, 0, 1], value=1.0)], dim=2).reshape(B, 24, 4, 4)
    chain = [tm[:, 0]]
    for i in range(1, 24):
        chain.append(torch.matmul(chain[parents[i]], tm[:, i]))
    transforms = torch.stack(chain, dim=1)
    joints_h = torch.nn.functional.pad(joints, [0, 0, 0, 1])
    A = transforms - torch.nn.functional.pad(torch.matmul(transforms, joints_h), [3, 0, 0, 0, 0, 0, 0, 0])
    W = m['lbs_weights'][None].expand(B, -1, -1)
    T = torch.matmul(W, A.view(B, 24, 16)).view(B, -1, 4, 4)
    v_homo = torch.matmul(T, torch.cat([v_posed, torch.ones(B, V, 1, dtype=rot.dtype, device=rot.device)], dim=2)[..., None])
    return v_homo[:, :, :3, 0], transforms[:, :, :3, 3]


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
    ap.add_argument('--frames', type=int, default=2048)
    ap.add_argument('--verts', type=int, default=6890)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'smpl_bench needs the GPU: there is no CPU timing'
    dev = 'cuda'
    F, V, K, scale = args.frames, args.verts, 17, 1000.0
    model = SMPLModel.synthetic(V, 1)
    layer = SMPLLayer(model).to(dev)
    g = torch.Generator().manual_seed(2)
    betas = torch.randn(F, 10, generator=g).to(dev)
    axis = torch.randn(F * 24, 3, generator=g, dtype=torch.float64)
    from motionbert_amd.smpl import rodrigues
    rot = rodrigues((axis / axis.norm(dim=1, keepdim=True) * 2.0 * torch.rand(F * 24, 1, generator=g, dtype=torch.float64))).float()
    rot = rot.reshape(F, 24, 3, 3).to(dev).contiguous()
    dverts, dkp = torch.randn(F, V, 3, generator=g).to(dev), torch.randn(F, K, 3, generator=g).to(dev)
    lines = [f'SMPL layer on {torch.cuda.get_device_name(0)}: HIP events, median (min .. max) of 20 passes after 5 warm-up passes; '
             f'F = {F} frames, V = {V} vertices, K = {K}']
    flop_f = 2.0 * F * V * (3 * 207 + 30 + 24 * 12 + 12 + 3 * K)
    lines.append(f'  from the shapes: model data {(V * (3 + 30 + 621 + 24 + K)) * 4 / 1e6:.1f} MB, vertices written {F * V * 12 / 1e6:.0f} MB, '
                 f'forward {flop_f / 1e9:.1f} GFLOP with dense weights (pose blend {2.0 * F * V * 621 / 1e9:.1f})')

    def say(name, t):
        lines.append(f'  {name:86s} {t[0] * 1e3:10.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f})')
        print(lines[-1], flush=True)
        return t[0]

    b_, r_ = betas.clone().requires_grad_(True), rot.clone().requires_grad_(True)

    def fused(mode):
        def run():
            if mode == 'fwd':
                with torch.no_grad():
                    layer.forward_kp(betas, rot, scale=scale)
                return
            b_.grad = r_.grad = None
            verts, kp = layer.forward_kp(b_, r_, scale=scale)
            loss = (kp * dkp).sum()
            if mode == 'both':
                loss = loss + (verts * dverts).sum()
            loss.backward()
        return run

    m = {k: getattr(model, k).to(dev) for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'lbs_weights')}
    Q = model.J_regressor_h36m.to(dev)

    def plain(mode):
        def run():
            if mode == 'fwd':
                with torch.no_grad():
                    v = plain_lbs(m, model.parents, betas, rot)[0] * scale
                    torch.matmul(Q[None].expand(F, -1, -1), v)
                return
            b_.grad = r_.grad = None
            verts = plain_lbs(m, model.parents, b_, r_)[0] * scale
            kp = torch.matmul(Q[None].expand(F, -1, -1), verts)
            loss = (kp * dkp).sum()
            if mode == 'both':
                loss = loss + (verts * dverts).sum()
            loss.backward()
        return run

    names = {'fwd': '(i) forward alone (verts + kp)', 'kp': '(ii) forward + backward, dkp only (training)', 'both': '(iii) forward + backward, dverts + dkp'}
    for mode in ('fwd', 'kp', 'both'):
        lines.append(names[mode])
        res = {}
        for label, make in (('fused: mbx_smpl_fwd' + ('' if mode == 'fwd' else ' + mbx_smpl_bwd') + ' through SMPLLayer.forward_kp', fused),
                            ('plain torch operations (fp32)' + ('' if mode == 'fwd' else ' + autograd backward'), plain)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            res[label] = say(label, timed(make(mode)))
            lines.append(f'      peak allocated above the inputs {(torch.cuda.max_memory_allocated() - base) / 1e6:.0f} MB')
        a, b = list(res.values())
        lines.append(f'      plain / fused {b / a:.2f}x')
        if mode == 'fwd':
            lines.append(f'      fused forward: {flop_f / (a * 1e-3) / 1e12:.1f} TFLOP/s of the dense-weight count, {F * V * 12 / (a * 1e-3) / 1e12:.2f} TB/s of vertex writes')
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
