"""Decoding of tests/golden/eval_h36m.npz (tools/make_eval_golden.py) for the evaluation tests, and the small fakes they share."""
import os

import numpy as np
import torch

from tests.helpers import GOLDEN

GATE = 1e-10      # relative; see tests/test_gpu_evaluate.py for where it comes from
CASES = [(r, d, g) for r in (0, 1) for d in (0, 1) for g in (0, 1)]      # rootrel, hw and factor present, gt_2d


def load():
    return np.load(os.path.join(GOLDEN, 'eval_h36m.npz'), allow_pickle=False)


def part_a(z):
    """(pred, gt) [4096,17,3] fp32 (exact: the stored grids are fp32-representable), (e1, e2) fp64."""
    pred = (z['a.pred_q'].astype(np.float64) * z['a.pred_step']).astype(np.float32)
    gt = (z['a.gt_q'].astype(np.float64) * z['a.gt_step']).astype(np.float32)
    return pred, gt, z['a.e1'], z['a.e2']


def part_b(z):
    split = z['b.split'].astype(np.int64)
    gts = (z['b.gt_q'].astype(np.float64) * z['b.gt_step']).astype(np.float32)
    return dict(sources=z['b.sources'], actions=z['b.actions'], split=split, gts=gts, factors=z['b.factor'], hw_clips=z['b.hw_frames'][split][:, 0, :],
                outputs=(z['b.out_q'].astype(np.float64) * z['b.out_step']).astype(np.float32),
                x=(z['b.x_q'].astype(np.float64) * z['b.x_step']).astype(np.float32), cover=z['b.cover'], action_names=[str(a) for a in z['b.action_names']])


def expected(z, case):
    tag = 'b.rootrel%d.denorm%d.gt2d%d' % case
    return z[tag + '.per_action'], z[tag + '.summary'], z[tag + '.count']


def make_evaluator(b, case, **kw):
    from motionbert_amd.evaluate import H36MEvaluator
    rootrel, denorm, gt_2d = case
    split = b['split']
    return H36MEvaluator(b['gts'][split], b['factors'][split] if denorm else None, split, b['hw_clips'] if denorm else None, b['actions'], b['sources'],
                         rootrel=bool(rootrel), flip=False, gt_2d=bool(gt_2d), **kw)


class FixedOutputs:
    """Stands in for the model: hands out stored network outputs clip by clip, in the order update() asks for them."""

    def __init__(self, outputs: torch.Tensor):
        self.outputs, self.at = outputs, 0

    def __call__(self, x):
        n = x.shape[0]
        out = self.outputs[self.at:self.at + n].clone()
        self.at += n
        return out


def run_split(ev, b, device, batches=(5, 1, 7, 3)):
    """Feed fixture (b) through update() in uneven batches; returns finish()."""
    assert sum(batches) == len(b['split'])
    model = FixedOutputs(torch.from_numpy(b['outputs']).to(device))
    x = torch.from_numpy(b['x']).to(device)
    at = 0
    for n in batches:
        ev.update(model, x[at:at + n])
        at += n
    return ev.finish()


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


class NumpyOps:
    """The two evaluation entries of the kernel provider in numpy fp64, on CPU tensors (same argument lists as HipOps)."""

    def pose_errors(self, pred, gt, hw, factor, x, rootrel, e1, e2):
        p, g = pred.double().numpy().copy(), gt.double().numpy()
        if rootrel:
            p[:, :, 0, :] = 0
        if x is not None:
            p[..., :2] = x.double().numpy()[..., :2]
        if hw is not None:
            w, h = hw.double().numpy()[:, 0].reshape(-1, 1, 1, 1), hw.double().numpy()[:, 1].reshape(-1, 1, 1, 1)
            p[..., :2] = (p[..., :2] + np.concatenate([np.ones_like(w), h / w], -1)) * w / 2
            p[..., 2:] = p[..., 2:] * w / 2
        if factor is not None:
            p = p * factor.double().numpy()[:, :, None, None]
        p, g = p - p[:, :, :1], g - g[:, :, :1]
        e1.copy_(torch.from_numpy(np.linalg.norm(p - g, axis=-1).mean(-1)))
        X0, Y0 = g - g.mean(2, keepdims=True), p - p.mean(2, keepdims=True)
        nx, ny = np.sqrt((X0 ** 2).sum((2, 3), keepdims=True)), np.sqrt((Y0 ** 2).sum((2, 3), keepdims=True))
        U, s, Vt = np.linalg.svd(np.matmul((X0 / nx).swapaxes(2, 3), Y0 / ny))
        V = Vt.swapaxes(2, 3).copy()
        d = np.sign(np.linalg.det(np.matmul(V, U.swapaxes(2, 3))))
        V[..., -1] *= d[..., None]
        s[..., -1] *= d
        a = s.sum(-1)[..., None, None] * nx / ny
        e2.copy_(torch.from_numpy(np.linalg.norm(a * np.matmul(Y0, np.matmul(V, U.swapaxes(2, 3))) - X0, axis=-1).mean(-1)))

    def eval_reduce(self, e1, e2, row_ptr, slots, action, A, per_action, summary, count):
        e1, e2, rp, sl, act = e1.numpy().reshape(-1), e2.numpy().reshape(-1), row_ptr.numpy(), slots.numpy(), action.numpy()
        assert len(rp) == len(act) + 1 and rp[-1] == len(sl)
        s, n = np.zeros((2, A)), np.zeros(A, np.int64)
        for f in range(len(act)):
            k = sl[rp[f]:rp[f + 1]]
            if len(k) and e1[k].sum() / len(k) > 0:
                s[0, act[f]] += e1[k].sum() / len(k)
                s[1, act[f]] += e2[k].sum() / len(k)
                n[act[f]] += 1
        per_action.copy_(torch.from_numpy(s / n))
        summary.copy_(torch.from_numpy((s / n).mean(1)))
        count.copy_(torch.from_numpy(n.astype(np.int32)))
