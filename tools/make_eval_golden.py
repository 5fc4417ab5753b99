"""Mint tests/golden/eval_h36m.npz: the fixture of the device-side H36M evaluation (motionbert_amd/evaluate.py, csrc/pose_eval.hip).

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout (MOTIONBERT_REFERENCE, as oracle/make_golden.py):

    python tools/make_eval_golden.py            # writes the file; the same bytes on every run on one machine
    python tools/make_eval_golden.py --check    # regenerates in memory and compares with the committed file

The per-frame errors are the reference's own `lib.model.loss.mpjpe` / `p_mpjpe` (numpy, LAPACK SVD) on fp64 copies of the stored
inputs, and the clips come from its `lib.utils.utils_data.split_clips`.  Its train.py and DataReaderH36M cannot be imported without
prettytable / easydict / the dataset pickle, so the two steps around the errors are restated here in fp64 with their line numbers:
the denormalisation (datareader_h36m.py:125-136) and the aggregation loop (train.py:100-149).

Contents (data only; every stored input is exactly representable in fp32, most as scaled int16 to keep the file small):
  (a) a.*   4,096 single frames, J = 17: gt = anisotropic Gaussians in whole millimetres; pred = a random similarity transform of gt
            (every fifth frame with a reflection) plus 40 mm noise, on a 1/16 mm grid; a.e1 / a.e2 fp64 = mpjpe / p_mpjpe of the
            root-relative poses, as train.py:124-127 calls them.
  (b) b.*   a synthetic test split: 6 sources over 4 actions and two camera resolutions, one source named like a blocked one, one
            shorter than a clip (split_clips resamples it: repeated frames inside a clip), clip length 27, test stride 9 (frames
            covered 0, 1, 2 or 3 times); per-frame factors, fixed "network outputs" and model inputs per clip; expected per-action /
            summary / count for rootrel x (hw and factor | neither) x gt_2d.

Conditioning is a condition of the fixture, not a tolerance of the tests: every frame of every case has both extents > 0 and the
second singular value of the normalised H >= 0.01 (asserted below), so no frame is excluded from any comparison.
"""
from __future__ import annotations

import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'eval_h36m.npz')
BLOCK_LIST = ['s_09_act_05_subact_02', 's_09_act_10_subact_02', 's_09_act_13_subact_01']      # train.py:109-111
N_FRAMES, STRIDE, J = 27, 9, 17


def reference_dir():
    ref = os.environ.get('MOTIONBERT_REFERENCE')
    if not ref:
        sys.path.insert(0, ROOT)
        from oracle.make_golden import REF as ref      # the default the other fixture scripts use
    return ref


def load_reference(rel, name):
    """One module of the reference by file path (this repository has a lib/ package of its own)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(reference_dir(), rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def second_singular_value(pred, gt):
    """Of the normalised H of loss.py:23-35, per frame, with both extents."""
    X0 = gt - gt.mean(1, keepdims=True)
    Y0 = pred - pred.mean(1, keepdims=True)
    nx, ny = np.sqrt((X0 ** 2).sum((1, 2))), np.sqrt((Y0 ** 2).sum((1, 2)))
    H = np.matmul((X0 / nx[:, None, None]).transpose(0, 2, 1), Y0 / ny[:, None, None])
    return np.linalg.svd(H, compute_uv=False)[:, 1], nx, ny


def check_conditioning(pred, gt, what):
    s1, nx, ny = second_singular_value(pred, gt)
    assert nx.min() > 0 and ny.min() > 0 and s1.min() >= 0.01, (what, nx.min(), ny.min(), s1.min())
    return float(s1.min())


def quantise(a, step, dtype=np.int16):
    info = np.iinfo(dtype)
    return np.clip(np.rint(a / step), info.min, info.max).astype(dtype)


def random_rotations(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]           # proper
    return q


def part_a(rng, loss):
    n = 4096
    sigma = rng.uniform(50.0, 300.0, size=(n, 1, 3))
    gt_q = quantise(rng.standard_normal((n, J, 3)) * sigma, 1.0)
    gt = gt_q.astype(np.float64)
    R = random_rotations(rng, n)
    R[::5, :, 2] *= -1                                # every fifth frame: a reflection
    pred = rng.uniform(0.7, 1.3, size=(n, 1, 1)) * np.matmul(gt, R) + rng.standard_normal((n, 1, 3)) * 100.0
    pred_q = quantise(pred + rng.standard_normal((n, J, 3)) * 40.0, 1.0 / 16)
    pred = pred_q.astype(np.float64) / 16
    assert np.array_equal(pred.astype(np.float32).astype(np.float64), pred)
    s1 = check_conditioning(pred, gt, 'a')
    print(f'(a) {n} frames, smallest second singular value {s1:.4f}')
    rp, rg = pred - pred[:, 0:1, :], gt - gt[:, 0:1, :]      # train.py:124-125: the errors are taken on root-relative poses
    return {'a.gt_q': gt_q, 'a.gt_step': np.float64(1.0), 'a.pred_q': pred_q, 'a.pred_step': np.float64(1.0 / 16),
            'a.e1': loss.mpjpe(rp.copy(), rg.copy()), 'a.e2': loss.p_mpjpe(rp.copy(), rg.copy())}


def denormalize(data, hw):
    """datareader_h36m.py:125-136 in fp64: data [Nc,T,J,3], hw [Nc,2] = (res_w, res_h)."""
    data = data.copy()
    for idx in range(len(data)):
        res_w, res_h = hw[idx]
        data[idx, :, :, :2] = (data[idx, :, :, :2] + np.array([1, res_h / res_w])) * res_w / 2      # :134
        data[idx, :, :, 2:] = data[idx, :, :, 2:] * res_w / 2                                       # :135
    return data


def aggregate(loss, results_all, actions, factor_clips, source_clips, frame_clips, gt_clips, what):
    """train.py:100-149 in fp64 (results_all is not modified).  Returns (per_action [2,A], summary [2], count [A], worst conditioning)."""
    num_test_frames = len(actions)
    e1_all, e2_all, oc = np.zeros(num_test_frames), np.zeros(num_test_frames), np.zeros(num_test_frames)          # :100-102
    action_names = sorted(set(actions.tolist()))                                                                 # :105
    results = {a: [] for a in action_names}
    results_procrustes = {a: [] for a in action_names}
    worst = np.inf
    for idx in range(len(frame_clips)):                                                                          # :112
        source = source_clips[idx][0][:-6]                                                                       # :113
        if source in BLOCK_LIST:
            continue
        frame_list = frame_clips[idx]
        pred = results_all[idx] * factor_clips[idx][:, None, None]                                               # :118-121
        pred = pred - pred[:, 0:1, :]                                                                            # :124
        gt = gt_clips[idx] - gt_clips[idx][:, 0:1, :]                                                            # :125
        worst = min(worst, check_conditioning(pred, gt, (what, idx)))
        err1, err2 = loss.mpjpe(pred.copy(), gt.copy()), loss.p_mpjpe(pred.copy(), gt.copy())                    # :126-127
        e1_all[frame_list] += err1                                                                               # :128-130
        e2_all[frame_list] += err2
        oc[frame_list] += 1
    for idx in range(num_test_frames):                                                                           # :131-137
        if e1_all[idx] > 0:
            results[actions[idx]].append(e1_all[idx] / oc[idx])
            results_procrustes[actions[idx]].append(e2_all[idx] / oc[idx])
    per = np.array([[np.mean(results[a]) for a in action_names], [np.mean(results_procrustes[a]) for a in action_names]])      # :142-144
    count = np.array([len(results[a]) for a in action_names], dtype=np.int32)
    return per, per.mean(1), count, worst                                                                        # :148-149


def part_b(rng, loss, udata):
    names = ['s_09_act_02_subact_01_ca_01', 's_09_act_02_subact_02_ca_02', 's_09_act_05_subact_02_ca_01', 's_09_act_05_subact_01_ca_03',
             's_11_act_12_subact_01_ca_04', 's_11_act_15_subact_02_ca_02']
    acts = ['Directions', 'Directions', 'Eating', 'Eating', 'Sitting', 'Walking']
    lens = [45, 50, 36, 54, 20, 47]
    cams = [(1000, 1002), (1000, 1000), (1000, 1002), (1000, 1000), (1000, 1000), (1000, 1002)]      # datareader_h36m.py:89-96
    sources = np.array(sum([[n] * l for n, l in zip(names, lens)], []))
    actions = np.array(sum([[a] * l for a, l in zip(acts, lens)], []))
    hw_frames = np.array(sum([[c] * l for c, l in zip(cams, lens)], []), dtype=np.float64)
    F = len(sources)
    np.random.seed(20240917)                          # split_clips -> resample draws from numpy's global generator for the short source
    split = np.stack([np.asarray(s, dtype=np.int64) for s in udata.split_clips(list(sources), N_FRAMES, data_stride=STRIDE)])
    cover = np.bincount(split.reshape(-1), minlength=F)
    assert {0, 1, 2, 3} <= set(cover.tolist()), sorted(set(cover.tolist()))
    assert any(len(set(c.tolist())) < N_FRAMES for c in split), 'no clip with a repeated frame'
    # per test frame: a pose in millimetres (joints_2.5d_image), a 2.5D factor, and where the person stands in the image
    sigma = rng.uniform(80.0, 300.0, size=(F, 1, 3))
    gt_q = quantise(rng.standard_normal((F, J, 3)) * sigma + rng.standard_normal((F, 1, 3)) * 200.0, 1.0 / 8)
    gts = gt_q.astype(np.float64) / 8
    factors = rng.uniform(3.0, 5.0, size=F).astype(np.float32)
    centre = rng.uniform(350.0, 650.0, size=(F, 1, 3)) * np.array([1.0, 1.0, 0.0])
    img = (gts - gts[:, :1]) / factors.astype(np.float64)[:, None, None] + centre                  # pixels
    w, h = hw_frames[:, 0][:, None, None], hw_frames[:, 1][:, None, None]
    norm = np.concatenate([img[..., :2] / w * 2 - np.concatenate([np.ones_like(w), h / w], -1), img[..., 2:] / w * 2], -1)      # :71-72
    Nc = len(split)
    small =0.15 * rng.standard_normal((Nc, 3, 3))
    R = np.linalg.qr(np.eye(3) + small - small.transpose(0, 2, 1))[0]
    R = R * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]                                   # near the identity, proper
    clip_norm = norm[split]                                                                         # [Nc,T,J,3]
    mid = clip_norm.mean(2, keepdims=True)
    out_q = quantise(np.matmul(clip_norm - mid, R[:, None]) * rng.uniform(0.9, 1.1, size=(Nc, 1, 1, 1)) + mid
                     + rng.standard_normal(clip_norm.shape) * 0.01, 2.0 ** -14)
    outputs = out_q.astype(np.float64) * 2.0 ** -14                                                 # the fixed "network outputs"
    x_q = quantise(np.concatenate([clip_norm[..., :2] + rng.standard_normal(clip_norm[..., :2].shape) * 0.005,
                                   rng.uniform(0.0, 1.0, size=clip_norm[..., :1].shape)], -1), 2.0 ** -14)
    x = x_q.astype(np.float64) * 2.0 ** -14                                                         # model input: x, y, confidence
    hw_clips = hw_frames[split][:, 0, :]                                                            # get_hw(), :109-114
    fx = {'b.sources': sources, 'b.actions': actions, 'b.split': split.astype(np.int32), 'b.gt_q': gt_q, 'b.gt_step': np.float64(1.0 / 8),
          'b.factor': factors, 'b.hw_frames': hw_frames.astype(np.float32), 'b.out_q': out_q, 'b.out_step': np.float64(2.0 ** -14), 'b.x_q': x_q,
          'b.x_step': np.float64(2.0 ** -14), 'b.cover': cover.astype(np.int32), 'b.action_names': np.array(sorted(set(acts)))}
    frames = np.arange(F)
    worst = np.inf
    for rootrel in (0, 1):
        for denorm in (0, 1):
            for gt_2d in (0, 1):
                pred = outputs.copy()
                if rootrel:
                    pred[:, :, 0, :] = 0                                                            # train.py:75-76
                if gt_2d:
                    pred[..., :2] = x[..., :2]                                                      # train.py:80-81
                fac = factors.astype(np.float64)[split] if denorm else np.ones(split.shape)
                if denorm:
                    pred = denormalize(pred, hw_clips)                                              # train.py:84
                tag = f'rootrel{rootrel}.denorm{denorm}.gt2d{gt_2d}'
                per, summary, count, s1 = aggregate(loss, pred, actions, fac, sources[split], frames[split], gts[split], tag)
                worst = min(worst, s1)
                assert np.isfinite(per).all() and count.sum() == (cover[~np.isin([s[:-6] for s in sources], BLOCK_LIST)] > 0).sum()
                fx[f'b.{tag}.per_action'], fx[f'b.{tag}.summary'], fx[f'b.{tag}.count'] = per, summary, count
                print(f'(b) {tag}: P1 {summary[0]:.6f}  P2 {summary[1]:.6f}  frames {count.tolist()}')
    print(f'(b) {F} test frames, {Nc} clips, coverage {sorted(set(cover.tolist()))}, smallest second singular value {worst:.4f}')
    return fx


def npz_bytes(arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, a.getvalue(), compresslevel=9)
    return buf.getvalue()


def main():
    loss = load_reference('lib/model/loss.py', 'ref_lib_model_loss')
    udata = load_reference('lib/utils/utils_data.py', 'ref_lib_utils_utils_data')
    fx = part_a(np.random.default_rng(1701), loss)
    fx.update(part_b(np.random.default_rng(1702), loss, udata))
    blob = npz_bytes(fx)
    assert len(blob) < 1_000_000, len(blob)
    if '--check' in sys.argv:
        same = open(OUT, 'rb').read() == blob
        print('identical to the committed file' if same else 'DIFFERS from the committed file')
        sys.exit(0 if same else 1)
    with open(OUT, 'wb') as f:
        f.write(blob)
    print(f'wrote {OUT}: {len(blob)} bytes')


if __name__ == '__main__':
    main()
