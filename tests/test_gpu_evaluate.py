"""Device-side H36M evaluation on a real MI355X: mbx_pose_errors / mbx_eval_reduce and motionbert_amd.evaluate against
tests/golden/eval_h36m.npz (per-frame errors from the reference's lib.model.loss on its LAPACK route, aggregation restated from
train.py:100-149 in fp64; tools/make_eval_golden.py).

The gate, 1e-10 relative on every frame and every aggregate (tests/eval_fixture.py GATE): a CPU prototype of the kernel's algorithm
(fp64, 8 Jacobi sweeps on H^T H, cross-product third vectors) agreed with the reference to 1.3e-14 worst case over 20,000 frames of
the fixture's kind; the same code in fp32 was off by 1e-7 at the median and 5.5e-6 worst case.  1e-10 is four orders away from both:
a correct fp64 kernel passes, any fp32 slip fails.  The fixture guarantees conditioning (second singular value of the normalised
H >= 0.01, both extents > 0, asserted when it is minted), so no frame is excluded from any comparison."""
import numpy as np
import pytest
import torch

from tests import eval_fixture as FX
from tests.helpers import build_model, load_golden, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def fx():
    z = FX.load()
    return z, FX.part_b(z)


def test_pose_errors_match_the_reference_on_every_frame(fx):
    from motionbert_amd import pose_errors
    z, _ = fx
    pred, gt, ref1, ref2 = FX.part_a(z)
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    e1, e2 = pose_errors(p, g)
    assert e1.dtype == torch.float64 and e1.shape == (4096,) and e1.is_cuda
    r1, r2 = FX.rel_err(e1.cpu().numpy(), ref1), FX.rel_err(e2.cpu().numpy(), ref2)
    print(f'fixture (a): worst relative error e1 {r1:.3e}, e2 {r2:.3e}')
    assert r1 < FX.GATE and r2 < FX.GATE
    # the same frames as a [N,T,J,3] batch whose rows start off a 16-byte boundary, and a tail workgroup: the same bits
    q1, q2 = pose_errors(p[1:4092].view(1, 4091, 17, 3), g[1:4092].view(1, 4091, 17, 3))
    assert torch.equal(q1.view(-1), e1[1:4092]) and torch.equal(q2.view(-1), e2[1:4092])


def _numpy_errors(pred, gt):
    """lib/model/loss.py:8-51 on root-relative fp64 poses, restated (the reference is not on the GPU box) for joint counts the fixture lacks."""
    ops_np = FX.NumpyOps()
    e1, e2 = torch.empty(len(pred), 1, dtype=torch.float64), torch.empty(len(pred), 1, dtype=torch.float64)
    ops_np.pose_errors(torch.from_numpy(pred)[:, None], torch.from_numpy(gt)[:, None], None, None, None, False, e1, e2)
    return e1.numpy().reshape(-1), e2.numpy().reshape(-1)


@pytest.mark.parametrize('J', [8, 64])
def test_other_joint_counts(J):
    """J is a runtime argument: an even LDS row (J = 8), the largest one (J = 64, more than 64 KiB of LDS) and a frame count that is
    no multiple of 64.  Same generator and the same conditioning condition as fixture (a), same gate."""
    from motionbert_amd import pose_errors
    rng = np.random.default_rng(J)
    n = 203
    gt = np.rint(rng.standard_normal((n, J, 3)) * rng.uniform(50.0, 300.0, size=(n, 1, 3)))
    R = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    pred = np.rint((rng.uniform(0.7, 1.3, size=(n, 1, 1)) * np.matmul(gt, R) + rng.standard_normal((n, 1, 3)) * 100 + rng.standard_normal((n, J, 3)) * 40) * 16) / 16
    X0, Y0 = gt - gt.mean(1, keepdims=True), pred - pred.mean(1, keepdims=True)
    H = np.matmul(X0.transpose(0, 2, 1), Y0) / (np.linalg.norm(X0, axis=(1, 2)) * np.linalg.norm(Y0, axis=(1, 2)))[:, None, None]
    assert np.linalg.svd(H, compute_uv=False)[:, 1].min() >= 0.01
    ref1, ref2 = _numpy_errors(pred, gt)
    e1, e2 = pose_errors(torch.from_numpy(pred.astype(np.float32)).to(DEV), torch.from_numpy(gt.astype(np.float32)).to(DEV))
    r1, r2 = FX.rel_err(e1.cpu().numpy(), ref1), FX.rel_err(e2.cpu().numpy(), ref2)
    print(f'J = {J}: worst relative error e1 {r1:.3e}, e2 {r2:.3e}')
    assert r1 < FX.GATE and r2 < FX.GATE


@pytest.mark.parametrize('case', FX.CASES)
def test_full_path_on_the_synthetic_split(fx, case):
    """rootrel on / off, hw and factor present / NULL, gt_2d, clips fed in uneven update() calls."""
    z, b = fx
    ev = FX.make_evaluator(b, case)
    e1, e2, per = FX.run_split(ev, b, DEV)
    ref_per, ref_sum, ref_count = FX.expected(z, case)
    got = np.array([[per[a][0] for a in ev.action_names], [per[a][1] for a in ev.action_names]])
    r_per, r_sum = FX.rel_err(got, ref_per), FX.rel_err([e1, e2], ref_sum)
    print(f'{case}: worst relative error per action {r_per:.3e}, summary {r_sum:.3e}')
    assert ev.action_names == b['action_names'] and ev.count.cpu().tolist() == ref_count.tolist()
    assert r_per < FX.GATE and r_sum < FX.GATE
    # one batch instead of four: the same bits (slots, not call order, decide where an error lands)
    ev2 = FX.make_evaluator(b, case)
    assert FX.run_split(ev2, b, DEV, batches=(16,)) == (e1, e2, per)


def test_finish_is_deterministic(fx):
    _, b = fx
    ev = FX.make_evaluator(b, (0, 1, 0))
    first = FX.run_split(ev, b, DEV)
    raw = (ev.per_action.clone(), ev.summary.clone(), ev.count.clone())
    ev.per_action.fill_(-1.0)
    second = ev.finish()
    assert first == second
    assert torch.equal(raw[0], ev.per_action) and torch.equal(raw[1], ev.summary) and torch.equal(raw[2], ev.count)
    # a larger problem (several chunks per action): two reductions of the same errors, bit for bit
    from motionbert_amd import hip_ops
    ops = hip_ops.get()
    g = torch.Generator().manual_seed(3)
    F, A = 40000, 7
    e1 = (torch.rand(F * 2, generator=g, dtype=torch.float64) * 80 + 1).to(DEV)
    e2 = (torch.rand(F * 2, generator=g, dtype=torch.float64) * 60 + 1).to(DEV)
    row_ptr = (torch.arange(F + 1, dtype=torch.int32) * 2).to(DEV)
    slots = torch.randperm(F * 2, generator=g).to(torch.int32).to(DEV)
    action = torch.randint(0, A, (F,), generator=g).to(torch.int32).to(DEV)
    outs = []
    for _ in range(2):
        per, summ, cnt = torch.empty(2, A, dtype=torch.float64, device=DEV), torch.empty(2, dtype=torch.float64, device=DEV), torch.empty(A, dtype=torch.int32, device=DEV)
        ops.eval_reduce(e1, e2, row_ptr, slots, action, A, per, summ, cnt)
        outs.append((per.cpu(), summ.cpu(), cnt.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    m1 = (e1[slots.long()].view(F, 2).sum(1) / 2).cpu()
    want = torch.stack([m1[action.cpu() == a].mean() for a in range(A)])
    assert torch.allclose(outs[0][0][0], want, rtol=1e-12, atol=0) and outs[0][2].sum().item() == F


class _Reader:
    """Duck-typed DataReaderH36M: the public side evaluate() reads (dt_dataset, get_split_id, get_hw)."""

    def __init__(self, b, T, stride):
        self.dt_dataset = {'test': {'action': b['actions'].tolist(), 'source': b['sources'].tolist(), '2.5d_factor': b['factors'].astype(np.float64),
                                    'joints_2.5d_image': b['gts'].astype(np.float64)}}
        src = b['sources']
        starts = [i for i in range(0, len(src) - T + 1, stride) if src[i] == src[i + T - 1]]
        self.split = [range(i, i + T) for i in starts]
        self.hw = np.array([[1000, 1002] if 'ca_01' in src[i] or 'ca_02' in src[i] else [1000, 1000] for i in starts], dtype=np.float64)

    def get_split_id(self):
        return None, self.split

    def get_hw(self):
        return self.hw


class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(no_conf=False, flip=True, rootrel=False, gt_2d=False), **kw)


@pytest.mark.parametrize('kw', [dict(), dict(rootrel=True, gt_2d=True), dict(flip=False, rootrel=True)])
def test_evaluate_end_to_end(fx, kw):
    """The drop-in: a tiny trained model, a duck-typed reader, the reference's signature and return triple."""
    from motionbert_amd.augment import flip_tta
    from motionbert_amd.evaluate import H36MEvaluator, evaluate
    _, b = fx
    zt, cfg = load_golden('tiny_trained')
    model = build_model(cfg)
    model.load_state_dict({k[2:]: torch.from_numpy(zt[k]) for k in zt.files if k.startswith('w.')}, strict=True)
    model.precision = 'fp32'
    model = model.to(DEV)
    reader, args = _Reader(b, T=9, stride=4), _Args(**kw)
    Nc = len(reader.split)
    x_all = make_input(Nc, 9, 17, 11)
    sizes = [7, 1] + [8] * ((Nc - 8) // 8) + ([(Nc - 8) % 8] if (Nc - 8) % 8 else [])
    loader, at = [], 0
    for n in sizes:
        loader.append((x_all[at:at + n], torch.zeros(n, 9, 17, 3)))      # CPU batches, as a DataLoader yields them
        at += n
    assert at == Nc
    model.train()                                                         # evaluate() switches to eval, as the reference does
    e1, e2, results_all = evaluate(args, model, loader, reader)
    assert not model.training and isinstance(results_all, np.ndarray) and results_all.shape == (Nc, 9, 17, 3) and results_all.dtype == np.float32
    # the same model's outputs through H36MEvaluator, and the host denormalisation of those outputs
    with torch.no_grad():
        outs = torch.cat([flip_tta(model, x.to(DEV)) if args.flip else model(x.to(DEV)) for x, _ in loader])
    split = np.stack([np.asarray(s) for s in reader.split])
    ev = H36MEvaluator(b['gts'][split], b['factors'][split], split, reader.hw, b['actions'], b['sources'], rootrel=args.rootrel, flip=False,
                       gt_2d=args.gt_2d)
    model_out = FX.FixedOutputs(outs)
    for x, _ in loader:
        ev.update(model_out, x.to(DEV))
    r1, r2, _ = ev.finish()
    print(f'{kw}: evaluate {e1!r} {e2!r}; evaluator {r1!r} {r2!r}')
    assert np.isfinite([e1, e2]).all() and e1 > 0 and e2 > 0
    assert e1 == pytest.approx(r1, rel=1e-12) and e2 == pytest.approx(r2, rel=1e-12)
    want = outs.cpu().numpy().astype(np.float64)
    if args.rootrel:
        want[:, :, 0, :] = 0
    if args.gt_2d:
        want[..., :2] = x_all.numpy()[..., :2]
    w, h = reader.hw[:, 0].reshape(-1, 1, 1, 1), reader.hw[:, 1].reshape(-1, 1, 1, 1)
    want[..., :2] = (want[..., :2] + np.concatenate([np.ones_like(w), h / w], -1)) * w / 2
    want[..., 2:] = want[..., 2:] * w / 2
    assert np.allclose(results_all, want, rtol=1e-6, atol=1e-4)           # fp32 rounding of pixel coordinates up to about 1000


def test_arguments_are_refused_before_any_launch():
    from motionbert_amd import hip_ops
    lib = hip_ops.get().lib
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
    ibuf = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, ip = buf.data_ptr(), ibuf.data_ptr()

    def errors(pred=p, gt=p, x=None, xc=0, gt_2d=0, e1=p, e2=p, N=1, T=4, J=17):
        return lib.mbx_pose_errors(pred, gt, None, None, x, xc, 0, gt_2d, e1, e2, N, T, J, None)

    def reduce(e1=p, row_ptr=ip, n_row_ptr=9, slots=ip, nnz=8, action=ip, F=8, A=2, per=p, ws=p):
        return lib.mbx_eval_reduce(e1, p, 16, row_ptr, n_row_ptr, slots, nnz, action, F, A, per, p, ip, ws, None)

    torch.cuda.synchronize()
    for what, call, word in [('J = 1', lambda: errors(J=1), b'joint count'), ('J = 65', lambda: errors(J=65), b'joint count'),
                             ('null pred', lambda: errors(pred=None), b'null'), ('null e2', lambda: errors(e2=None), b'null'),
                             ('gt_2d without x', lambda: errors(gt_2d=1), b'gt_2d'), ('x with one channel', lambda: errors(gt_2d=1, x=p, xc=1), b'gt_2d'),
                             ('no frames', lambda: errors(T=0), b'bad shape'), ('null row table', lambda: reduce(row_ptr=None), b'null'),
                             ('null workspace', lambda: reduce(ws=None), b'null'), ('row table of F entries', lambda: reduce(n_row_ptr=8), b'CSR'),
                             ('row table of F + 2 entries', lambda: reduce(n_row_ptr=10), b'CSR'),
                             ('null slots with nnz > 0', lambda: reduce(slots=None), b'slot'), ('no actions', lambda: reduce(A=0), b'bad sizes')]:
        rc = call()
        assert rc != 0 and word in lib.mbx_last_error(), (what, rc, lib.mbx_last_error())
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and int(ibuf.abs().sum()) == 0      # nothing ran: the output buffers are untouched
    assert lib.mbx_eval_reduce_ws(8, 2) >= 8 * 3 * 8 and lib.mbx_eval_reduce_ws(0, 2) == 0
