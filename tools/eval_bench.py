"""How long does an H36M evaluation epoch take, and where?  Synthetic clips of H36M-test size (2,333 clips x 243 frames x 17 joints).

    python tools/eval_bench.py [--out profiles/eval_bench.txt] [--clips 2333] [--batch 32]

Three numbers, no threshold:
  (i)   the flip-TTA forward of the full model (DSTformer, dim_feat 512, depth 5) over all clips, bf16, batches of --batch clips:
        a host clock around work that ends in a device synchronise, after one warm-up batch;
  (ii)  the device metrics: mbx_pose_errors over all clips + mbx_eval_reduce, device events over 20 warmed repetitions (median);
  (iii) the host path the reference runs instead (train.py:82-153), restated below in numpy on this box's CPU: the device-to-host
        copy of the predictions, the denormalisation, the per-clip loop with the batched LAPACK SVD (lib/model/loss.py:16-51) and
        the per-frame aggregation loop.  Timed once (it takes seconds).
"""
from __future__ import annotations

import argparse
import os
import platform
import sys
import time
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FULL = dict(dim_in=3, dim_out=3, dim_feat=512, dim_rep=512, depth=5, num_heads=8, mlp_ratio=2, num_joints=17, maxlen=243)
ACTIONS = ['Directions', 'Discussion', 'Eating', 'Greeting', 'Phoning', 'Photo', 'Posing', 'Purchases', 'Sitting', 'SittingDown', 'Smoking', 'Waiting',
           'WalkDog', 'WalkTogether', 'Walking']


def mpjpe(predicted, target):
    return np.mean(np.linalg.norm(predicted - target, axis=len(target.shape) - 1), axis=1)


def p_mpjpe(predicted, target):
    """lib/model/loss.py:16-51, restated."""
    muX, muY = np.mean(target, axis=1, keepdims=True), np.mean(predicted, axis=1, keepdims=True)
    X0, Y0 = target - muX, predicted - muY
    normX, normY = np.sqrt(np.sum(X0 ** 2, axis=(1, 2), keepdims=True)), np.sqrt(np.sum(Y0 ** 2, axis=(1, 2), keepdims=True))
    X0 /= normX
    Y0 /= normY
    U, s, Vt = np.linalg.svd(np.matmul(X0.transpose(0, 2, 1), Y0))
    V = Vt.transpose(0, 2, 1)
    sign = np.sign(np.expand_dims(np.linalg.det(np.matmul(V, U.transpose(0, 2, 1))), axis=1))
    V[:, :, -1] *= sign
    s[:, -1] *= sign.flatten()
    R = np.matmul(V, U.transpose(0, 2, 1))
    a = np.expand_dims(np.sum(s, axis=1, keepdims=True), axis=2) * normX / normY
    t = muX - a * np.matmul(muY, R)
    return np.mean(np.linalg.norm(a * np.matmul(predicted, R) + t - target, axis=len(target.shape) - 1), axis=1)


def host_path(pred_dev, hw, factor_clips, frame_clips, gt_clips, actions):
    """train.py:82-149 without the block list (synthetic sources).  Returns (e1, e2, seconds of the copy, seconds of the rest)."""
    t0 = time.perf_counter()
    results_all = pred_dev.cpu().numpy()
    t1 = time.perf_counter()
    for idx in range(len(results_all)):                                   # datareader_h36m.py:132-135
        w, h = hw[idx]
        results_all[idx, :, :, :2] = (results_all[idx, :, :, :2] + np.array([1, h / w])) * w / 2
        results_all[idx, :, :, 2:] = results_all[idx, :, :, 2:] * w / 2
    F = len(actions)
    e1_all, e2_all, oc = np.zeros(F), np.zeros(F), np.zeros(F)
    names = sorted(set(actions.tolist()))
    res1, res2 = {a: [] for a in names}, {a: [] for a in names}
    for idx in range(len(results_all)):                                   # train.py:112-130
        pred = results_all[idx]
        pred *= factor_clips[idx][:, None, None]
        pred = pred - pred[:, 0:1, :]
        gt = gt_clips[idx] - gt_clips[idx][:, 0:1, :]
        e1_all[frame_clips[idx]] += mpjpe(pred, gt)
        e2_all[frame_clips[idx]] += p_mpjpe(pred, gt)
        oc[frame_clips[idx]] += 1
    for idx in range(F):                                                  # train.py:131-137
        if e1_all[idx] > 0:
            res1[actions[idx]].append(e1_all[idx] / oc[idx])
            res2[actions[idx]].append(e2_all[idx] / oc[idx])
    e1 = np.mean([np.mean(res1[a]) for a in names])
    e2 = np.mean([np.mean(res2[a]) for a in names])
    return e1, e2, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--clips', type=int, default=2333)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    from motionbert_amd import DSTformer
    from motionbert_amd.augment import flip_tta
    from motionbert_amd.evaluate import H36MEvaluator
    dev = torch.device('cuda', 0)
    Nc, T, J = a.clips, 243, 17
    rng = np.random.default_rng(0)
    F = Nc * T
    frame_clips = np.arange(F).reshape(Nc, T)                             # test stride 243: every frame in one clip
    actions = np.array(ACTIONS)[(np.arange(F) // T) % len(ACTIONS)]
    sources = np.array(['s_00_act_%02d_subact_01_ca_01' % (c % 15) for c in range(Nc)])[np.arange(F) // T]
    gts = (rng.standard_normal((F, J, 3)) * 200).astype(np.float32)
    factors = rng.uniform(3, 5, size=F).astype(np.float32)
    hw = np.tile(np.array([[1000.0, 1002.0], [1000.0, 1000.0]]), (Nc // 2 + 1, 1))[:Nc]
    x = torch.cat([torch.rand(Nc, T, J, 2) * 2 - 1, torch.rand(Nc, T, J, 1)], -1).to(dev)
    lines = [f'eval_bench: {Nc} clips x {T} frames x {J} joints = {F} frames', f'box: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}; '
             f'host {platform.processor() or platform.machine()}, {len(os.sched_getaffinity(0))} CPUs available to this process']

    # (i) flip-TTA forward
    torch.manual_seed(0)
    model = DSTformer(norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **FULL).to(dev).eval()
    model.precision = 'bf16'
    flip_tta(model, x[:a.batch])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    preds = [flip_tta(model, x[i:i + a.batch]) for i in range(0, Nc, a.batch)]
    torch.cuda.synchronize()
    t_fwd = time.perf_counter() - t0
    pred = torch.cat(preds)
    del preds
    lines.append(f'(i)   flip-TTA forward, full model, bf16, batch {a.batch}: {t_fwd * 1e3:9.1f} ms  ({Nc / t_fwd:.0f} clips/s)')

    # (ii) device metrics
    ev = H36MEvaluator(gts[frame_clips], factors[frame_clips], frame_clips, hw, actions, sources, rootrel=False, flip=False, device=dev)
    ops = ev.ops

    def metrics():
        ops.pose_errors(pred, ev.gt, ev.hw, ev.factor, None, False, ev.e1, ev.e2)
        ops.eval_reduce(ev.e1, ev.e2, ev.row_ptr, ev.slots, ev.action_id, len(ev.action_names), ev.per_action, ev.summary, ev.count)
    for _ in range(3):
        metrics()
    torch.cuda.synchronize()
    ms, ms_err = [], []
    for _ in range(20):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        ops.pose_errors(pred, ev.gt, ev.hw, ev.factor, None, False, ev.e1, ev.e2)
        e[1].record()
        ops.eval_reduce(ev.e1, ev.e2, ev.row_ptr, ev.slots, ev.action_id, len(ev.action_names), ev.per_action, ev.summary, ev.count)
        e[2].record()
        e[2].synchronize()
        ms.append(e[0].elapsed_time(e[2]))
        ms_err.append(e[0].elapsed_time(e[1]))
    ev.cursor = Nc
    d1, d2, _ = ev.finish()
    lines.append(f'(ii)  device metrics (mbx_pose_errors + mbx_eval_reduce), median of 20: {np.median(ms):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}; '
                 f'mbx_pose_errors alone {np.median(ms_err):.3f} ms)')

    # (iii) the host path
    h1, h2, t_copy, t_host = host_path(pred, hw, factors[frame_clips].astype(np.float64), frame_clips, gts[frame_clips].astype(np.float64), actions)
    lines.append(f'(iii) host path in numpy (train.py:82-153 restated): {(t_copy + t_host) * 1e3:9.1f} ms  (device-to-host copy {t_copy * 1e3:.1f} ms, '
                 f'denormalise + SVD + loops {t_host * 1e3:.1f} ms)')
    lines.append(f'P1 / P2 of the synthetic data: device {d1:.6f} / {d2:.6f}, host {h1:.6f} / {h2:.6f} (the host path rounds the denormalised and the '
                 f'factor-scaled predictions to fp32 in place, the device path keeps fp64)')
    lines.append(f'host path / forward = {(t_copy + t_host) / t_fwd:.2f}; host path / device metrics = {(t_copy + t_host) * 1e3 / np.median(ms):.0f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
