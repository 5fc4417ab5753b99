"""The host logic of the 2D pre-training data path on the CPU, with the kernel provider of tests/motion2derr.py injected: the two packers
against the reference's own arrays (tests/golden/motion2d.npz), the PackedMotion2D stream and its one-launch front end, run_pretrain_epoch
against pretrain_epoch_plan, PretrainStep.step_prepared against __call__, and the argument errors of the C entry on the library loaded
without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

from motionbert_amd import augment, data, hip_ops, train
from tests import motion2derr as ME
from tests.helpers import GOLDEN


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'motion2d.npz'))


@pytest.fixture(scope='module')
def packed(tmp_path_factory):
    d = tmp_path_factory.mktemp('motion2d')
    ann = d / 'posetrack'
    ann.mkdir()
    for name, content in ME.posetrack_files().items():
        with open(ann / name, 'w') as f:
            json.dump(content, f)
    motion_all, id_all = ME.instav_arrays()
    np.save(d / 'motion_all.npy', motion_all)
    np.save(d / 'id_all.npy', id_all)
    pt = data.pack_posetrack(str(ann), str(d / 'pt'))
    iv = data.pack_instav(str(d / 'motion_all.npy'), str(d / 'id_all.npy'), str(d / 'iv'))
    return str(d / 'pt'), pt, str(d / 'iv'), iv


def test_packers_are_bit_equal_to_the_reference_arrays(packed, fixture):
    pt_prefix, pt, iv_prefix, iv = packed
    got = np.load(pt_prefix + '.motion2d.npy')
    assert got.dtype == np.float32 and pt['n'] == 3 and pt['clip_shape'] == [30, 17, 3]
    assert got.tobytes() == fixture['pt.motions_2d'].astype(np.float32).tobytes()
    got = np.load(iv_prefix + '.motion2d.npy')
    assert got.dtype == np.float32 and iv['n'] == 3 and iv['clip_shape'] == [81, 17, 3]
    assert got.tobytes() == fixture['iv.motions_2d'].tobytes()
    assert json.load(open(iv_prefix + '.json'))['kind'] == 'instav' and json.load(open(pt_prefix + '.json'))['kind'] == 'posetrack'


def test_packed_motion2d_stream_shapes_seeds_and_sharding(packed):
    _, _, iv_prefix, _ = packed
    ops = ME.TorchMotion2DOps()
    ds = data.PackedMotion2D(iv_prefix, device='cpu', kind='instav', ops=ops)
    assert len(ds) == 3
    got = list(ds.batches(2, shuffle=True, epoch=3, seed=11))
    assert [tuple(a.shape) for a, _ in got] == [(2, 81, 17, 3), (1, 81, 17, 3)] and all(a is b and a.dtype == torch.float32 for a, b in got)
    assert [c[1] for c in ops.calls] == [ME.CROP | ME.ZERO | ME.FLIP | ME.ROOTREL] * 2 and all(c[4] == ('data',) and not c[3] for c in ops.calls)
    seeds = [c[2] for c in ops.calls]
    assert seeds == [data.PackedAction.batch_seed(11, 3, 0, 0), data.PackedAction.batch_seed(11, 3, 0, 1)] and seeds[0] != seeds[1]
    idx = data.shard_indices(3, True, 3, 11, 0, 1)
    clips = np.load(iv_prefix + '.motion2d.npy')
    for k, (a, _) in enumerate(got):
        rows = np.sort(idx[2 * k:2 * k + 2])
        want = augment.motion2d_input(torch.from_numpy(clips[rows]), seed=seeds[k], ops=ME.TorchMotion2DOps())['data']
        assert torch.equal(a, want) and float(a.abs().max()) <= 1.0
    again = list(ds.batches(2, shuffle=True, epoch=3, seed=11))
    assert all(torch.equal(a, b) for (a, _), (b, _) in zip(got, again))                                 # reproducible from the seed
    other = list(ds.batches(2, shuffle=True, epoch=4, seed=11))
    assert not all(torch.equal(a, b) for (a, _), (b, _) in zip(got, other))
    assert len(list(ds.batches(2, drop_last=True))) == 1
    shards = [list(ds.batches(1, shuffle=True, epoch=0, seed=5, rank=r, world=2)) for r in range(2)]
    assert [len(s) for s in shards] == [2, 2]                                                          # equal shares, the tail wrapped


def test_posetrack_kind_only_flips(packed, fixture):
    pt_prefix = packed[0]
    ops = ME.TorchMotion2DOps()
    ds = data.PackedMotion2D(pt_prefix, device='cpu', kind='posetrack', scale_range=(0.25, 1), ops=ops)
    (a, _), = list(ds.batches(3, shuffle=False))
    assert ops.calls[0][1] == ME.FLIP | ME.ROOTREL
    stored = torch.from_numpy(fixture['pt.motions_2d'].astype(np.float32))
    flipped = stored[:, :, ME.FLIP_PERM] * torch.tensor([-1.0, 1.0, 1.0])
    assert all(torch.equal(a[i], stored[i]) or torch.equal(a[i], flipped[i]) for i in range(3))
    ds = data.PackedMotion2D(pt_prefix, device='cpu', kind='posetrack', flip=False, ops=ops)
    (a, _), = list(ds.batches(3, shuffle=False))
    assert torch.equal(a, stored) and ops.calls[-1][1] == ME.ROOTREL
    with pytest.raises(ValueError, match='kind'):
        data.PackedMotion2D(pt_prefix, device='cpu', kind='coco')


@pytest.mark.parametrize('rootrel', [True, False])
def test_front_triple_equals_the_steps_own_no_grad_block(packed, rootrel):
    _, _, iv_prefix, _ = packed
    ds = data.PackedMotion2D(iv_prefix, device='cpu', kind='instav', ops=ME.TorchMotion2DOps())
    step = train.PretrainStep(None, None, aug=None, rootrel=rootrel, mask=False, noise=False)
    plain = list(ds.batches(2, shuffle=True, epoch=1, seed=2))
    front = list(ds.batches(2, shuffle=True, epoch=1, seed=2, front=step, has_gt=False))
    assert len(front) == len(plain) == 2
    seen = {}
    step.step_prepared = lambda x, gt, conf, has_3d=False: seen.update(x=x, gt=gt, conf=conf)           # what __call__ hands on
    for (d, _), (x_aug, gt, conf) in zip(plain, front):
        step(d, d, has_3d=False, has_gt=False)
        assert torch.equal(x_aug, seen['x']) and torch.equal(gt, seen['gt']) and torch.equal(conf, seen['conf'])
        assert conf.shape == d.shape[:3] + (1,)


def test_front_flags_follow_the_step_and_no_conf_is_refused(packed):
    _, _, iv_prefix, _ = packed
    ops = ME.TorchMotion2DOps()
    ds = data.PackedMotion2D(iv_prefix, device='cpu', kind='instav', ops=ops)
    aug = ME.AugConfig(np.load(os.path.join(GOLDEN, 'augment2d.npz'))).augmenter()
    step = train.PretrainStep(None, None, aug=aug, rootrel=False, mask=True, noise=True)
    base = ME.CROP | ME.ZERO | ME.FLIP
    for has_gt, want in ((True, base | ME.MASK | ME.NOISE), (False, base | ME.MASK)):
        x_aug, gt, conf = next(iter(ds.batches(3, shuffle=False, front=step, has_gt=has_gt)))
        assert ops.calls[-1][1] == want and ops.calls[-1][4] == ('gt', 'conf', 'x_aug')
        assert bool((x_aug == 0).all(-1).any()) and x_aug.shape == gt.shape                             # the masks removed points
    with pytest.raises(ValueError, match='no_conf'):
        next(iter(ds.batches(3, front=train.PretrainStep(None, None, mask=False, noise=False, no_conf=True))))


def test_motion2d_input_argument_errors():
    x = ME.motion_inputs(2, 5, 17, 1)
    ops = ME.TorchMotion2DOps()
    with pytest.raises(ValueError, match=r'\[N,T,J,3\]'):
        augment.motion2d_input(x[..., :2], ops=ops)
    with pytest.raises(ValueError, match='want'):
        augment.motion2d_input(x, want=('data', 'velocity'), ops=ops)
    with pytest.raises(ValueError, match='Augmenter2D'):
        augment.motion2d_input(x, mask=True, ops=ops)
    with pytest.raises(ValueError, match='lo > hi'):
        augment.motion2d_input(x, scale_range=(1, 0.25), ops=ops)
    with pytest.raises(ValueError, match='17-joint'):
        augment.motion2d_input(ME.motion_inputs(2, 5, 32, 1), ops=ops)
    with pytest.raises(ValueError, match='params'):
        augment.motion2d_input(x, params=torch.zeros(2, 9), ops=ops)
    with pytest.raises(RuntimeError, match='ROCm device'):
        augment.motion2d_input(x)
    out, used = augment.motion2d_input(x, want=('conf', 'gt'), seed=9, return_params=True, ops=ops)
    assert set(out) == {'conf', 'gt'} and torch.equal(used, ME.draw_params(2, 9))


class _RecordingStep:
    """what run_pretrain_epoch needs of a PretrainStep: the front-end attributes, __call__ for 3D batches, step_prepared for 2D ones"""
    aug, rootrel, mask, noise, no_conf = None, True, False, False, False

    def __init__(self):
        self.log = []

    def __call__(self, batch_input, batch_gt, has_3d, has_gt=True):
        self.log.append(('3d', has_3d, has_gt, tuple(batch_input.shape)))
        return torch.tensor([1.0, 2.0, 3.0, float(len(batch_input))])

    def step_prepared(self, x_aug, gt, conf, has_3d=False):
        self.log.append(('2d', has_3d, tuple(x_aug.shape), tuple(conf.shape)))
        return torch.tensor([0.0, 0.0, 0.0, float(len(x_aug))])


class _Fake3D:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def batches(self, batch_size, shuffle=True, epoch=0, seed=0, rank=0, world=1):
        idx = data.shard_indices(self.n, shuffle, epoch, seed, rank, world)
        for i in range(0, len(idx), batch_size):
            b = len(idx[i:i + batch_size])
            yield torch.zeros(b, 9, 17, 3), torch.zeros(b, 9, 17, 3)


def test_run_pretrain_epoch_follows_the_plan(packed):
    pt_prefix, _, iv_prefix, _ = packed
    ops = ME.TorchMotion2DOps()
    pt = data.PackedMotion2D(pt_prefix, device='cpu', kind='posetrack', ops=ops)
    iv = data.PackedMotion2D(iv_prefix, device='cpu', kind='instav', ops=ops)
    m3 = _Fake3D(5)
    step = _RecordingStep()
    out = train.run_pretrain_epoch(step, pt, iv, m3, batch_size=2, epoch=30, seed=1)
    plan = train.pretrain_epoch_plan(2, 2, 3, epoch=30)
    assert list(out) == [p[0] for p in plan] and [out[p[0]]['batches'] for p in plan] == [p[3] for p in plan]
    assert [e[0] for e in step.log] == ['2d'] * 4 + ['3d'] * 3
    assert [e[2][1] for e in step.log[:4]] == [30, 30, 81, 81]                                          # PoseTrack first, then InstaVariety
    assert all(e[1] is True and e[2] is True for e in step.log[4:])
    assert out['3d']['losses'] == pytest.approx([1.0, 2.0, 3.0, 5 / 3]) and out['instav']['losses'] == pytest.approx([0, 0, 0, 1.5])
    # the flags of the 2D launches: PoseTrack flips only, InstaVariety crops, zeroes and flips; no noise without has_gt (none asked here)
    assert [c[1] & ~ME.ROOTREL for c in ops.calls] == [ME.FLIP] * 2 + [ME.CROP | ME.ZERO | ME.FLIP] * 2
    step = _RecordingStep()
    out = train.run_pretrain_epoch(step, pt, iv, m3, batch_size=2, epoch=3, seed=1)                     # before the curriculum epoch: 3D only
    assert list(out) == ['3d'] and [e[0] for e in step.log] == ['3d'] * 3
    out = train.run_pretrain_epoch(_RecordingStep(), None, None, m3, batch_size=2, epoch=40, seed=1, train_2d=False)
    assert list(out) == ['3d']
    shares = [train.run_pretrain_epoch(_RecordingStep(), pt, iv, m3, batch_size=1, epoch=30, rank=r, world=2) for r in range(2)]
    assert [[v['batches'] for v in s.values()] for s in shares] == [[2, 2, 3]] * 2                      # equal steps on every rank


def test_step_prepared_moves_the_model_as_call_does(monkeypatch):
    def loss_2d(pred, target, conf, ops=None):
        return torch.mean(torch.norm((pred[..., :2] - target[..., :2]) * conf, dim=-1))
    monkeypatch.setattr(train, 'loss_2d_weighted', loss_2d)

    class Step(train.PretrainStep):
        def loss_3d(self, pred, batch_gt):
            total = torch.mean(torch.norm(pred - batch_gt, dim=-1))
            return total, torch.stack([total.detach()] * 4)

    def make():
        torch.manual_seed(3)
        net = torch.nn.Sequential(torch.nn.Linear(3, 8), torch.nn.Tanh(), torch.nn.Linear(8, 3))
        return net, torch.optim.SGD(net.parameters(), lr=0.1)
    x = ME.motion_inputs(2, 5, 17, 4)
    gt3 = torch.randn(2, 5, 17, 3, generator=torch.Generator().manual_seed(5))
    for rootrel in (True, False):
        (a, oa), (b, ob) = make(), make()
        sa, sb = Step(a, oa, mask=False, noise=False, rootrel=rootrel), Step(b, ob, mask=False, noise=False, rootrel=rootrel)
        la = [sa(x, x, has_3d=False), sa(x, gt3, has_3d=True)]
        target = x - x[:, :, 0:1] if rootrel else torch.cat([x[..., :2], x[..., 2:] - x[:, 0:1, 0:1, 2:]], -1)
        target3 = gt3 - gt3[:, :, 0:1] if rootrel else torch.cat([gt3[..., :2], gt3[..., 2:] - gt3[:, 0:1, 0:1, 2:]], -1)
        lb = [sb.step_prepared(x, target, x[..., 2:], has_3d=False), sb.step_prepared(x, target3, None, has_3d=True)]
        assert all(torch.equal(u, v) for u, v in zip(la, lb)) and la[0].shape == (4,)
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
        with pytest.raises(ValueError, match='conf'):
            sb.step_prepared(x, target, None, has_3d=False)


def test_abi_argument_errors_without_a_gpu():
    """validation happens before any launch, so this is safe without a GPU"""
    lib = hip_ops.load_library()
    assert lib.mbx_version() >= 170
    err = lambda: lib.mbx_last_error().decode()                                           # noqa: E731
    tail = (None, None, None, 0.06, 0.002, 0.0, 0.0, 0.0, 0.0, 0.05, 0.1)

    def call(x=4096, outs=(1 << 20, None, None, None), shape=(1, 30, 17), r=(0.25, 1.0), p=0.5, flags=7, noise=tail):
        return lib.mbx_motion2d_input(x, *outs, *shape, None, None, *r, p, *noise, flags, 0, None)
    assert call(x=None) != 0 and 'null' in err()
    assert call(outs=(None,) * 4) != 0 and 'no output' in err()
    for shape in ((0, 30, 17), (1, 0, 17), (1, 30, 0), (1, 30, 33)):
        assert call(shape=shape, flags=3) != 0 and 'bad shape' in err(), shape
    assert call(r=(1.0, 0.25)) != 0 and 'lo > hi' in err()
    for p in (-0.1, 1.5):
        assert call(p=p) != 0 and 'flip_prob' in err()
    assert call(flags=64) != 0 and 'flags' in err()
    assert call(shape=(1, 30, 16), flags=4) != 0 and '17-joint' in err()
    assert call(flags=8) != 0 and 'noise needs' in err()
    assert call(shape=(1 << 20, 1 << 8, 16), flags=3, outs=(1 << 50, None, None, None)) != 0 and '32-bit' in err()
    nbytes = 30 * 17 * 3 * 4
    for k in range(4):                                                                   # every output against x: overlapping from either side
        for off in (0, nbytes - 4, -(nbytes // 3 if k == 2 else nbytes) + 4):
            outs = [None] * 4
            outs[k] = (1 << 20) + off
            assert call(x=1 << 20, outs=tuple(outs)) != 0 and 'overlaps' in err(), (k, off)
