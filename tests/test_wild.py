"""`motionbert_amd.wild.infer` end to end on the CPU: the numpy stand-in provider (tests/wilderr.NumpyWildOps) and a fixed element-wise
network (wilderr.FixedNet) against the restated loop of infer_wild.py:63-96 (wilderr.reference_loop: batch 1, two forwards, flip_data
copies), bit for bit, for every combination of flip, rootrel, gt_2d, no_conf and pixel; the batching, the dict form and the argument
errors.  The input of the reference loop is the restated read_input, which tests/test_wilderr.py pins to the reference's own output."""
import itertools

import numpy as np
import pytest
import torch

from motionbert_amd import wild
from tests import wilderr as WE

L = WE.CLIP_LEN
VID = (1920, 1080)
LENGTHS = (L - 1, L, L + 1, 2 * L + 3)
BATCHES = (1, 2, 64)


@pytest.fixture(scope='module')
def kps():
    return {F: WE.detections(F, 8400 + F) for F in LENGTHS}


def _motion(kp, pixel, seq_lens=None):
    return WE.input_ref(kp, VID if pixel else None, None if pixel else [1, 1], seq_lens)[0]


@pytest.mark.parametrize('flip,rootrel,gt_2d,no_conf,pixel', list(itertools.product((False, True), repeat=5)))
def test_infer_equals_the_reference_loop(kps, flip, rootrel, gt_2d, no_conf, pixel):
    for F in LENGTHS:
        want = WE.reference_loop(WE.FixedNet(), _motion(kps[F], pixel), L, flip, rootrel, gt_2d, no_conf, VID if pixel else None)
        assert want.shape == (F, 17, 3) and want.dtype == np.float32
        for mb in BATCHES:
            net, ops = WE.FixedNet(), WE.NumpyWildOps()
            got = wild.infer(net, kps[F], clip_len=L, vid_size=VID if pixel else None, pixel=pixel, flip=flip, rootrel=rootrel, gt_2d=gt_2d, no_conf=no_conf,
                             max_batch=mb, ops=ops)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32
            assert WE.differing(got, want) == 0, (F, mb)
            assert net.evals == 1 and ops.calls[0] == ('wild_input', (F, 26, 3), WE.PIXEL if pixel else WE.CROP, 2 if no_conf else 3)
            # full clips in batches of at most max_batch, the tail in a batch of its own
            full, tail = divmod(F, L)
            shapes = [(min(mb, full - b), L, 17, 2 if no_conf else 3) for b in range(0, full, mb)] + ([(1, tail, 17, 2 if no_conf else 3)] if tail else [])
            assert net.calls == [(('tta',) + s if flip else s) for s in shapes]
            assert [c[1] for c in ops.calls[1:]] == [s[:2] + (17, 3) for s in shapes]


def test_dict_form_pools_the_tracks(kps):
    """three persons of different lengths in one pass: per person the reference loop's bits; the full clips of ALL tracks share batches"""
    tracks = {5: WE.detections(L - 4, 8501), 'b': WE.detections(2 * L, 8502), 2: WE.detections(L + 1, 8503)}
    for pixel, gt_2d in ((False, False), (True, True)):
        net, ops = WE.FixedNet(), WE.NumpyWildOps()
        got = wild.infer(net, tracks, clip_len=L, vid_size=VID, pixel=pixel, gt_2d=gt_2d, max_batch=64, ops=ops)
        assert list(got) == [5, 'b', 2]
        for k, kp in tracks.items():
            want = WE.reference_loop(WE.FixedNet(), _motion(kp, pixel), L, True, False, gt_2d, False, VID if pixel else None)
            assert WE.differing(got[k], want) == 0, k
            single = wild.infer(WE.FixedNet(), kp, clip_len=L, vid_size=VID, pixel=pixel, gt_2d=gt_2d, ops=WE.NumpyWildOps())
            assert WE.differing(got[k], single) == 0, k
        assert net.calls == [('tta', 3, L, 17, 3), ('tta', 1, L - 4, 17, 3), ('tta', 1, 1, 17, 3)]
        assert len([c for c in ops.calls if c[0] == 'wild_input']) == 1
    # tensors in, tails of equal length share a batch
    same = {0: torch.from_numpy(WE.detections(L + 2, 8504)), 1: torch.from_numpy(WE.detections(2, 8505))}
    net = WE.FixedNet()
    out = wild.infer(net, same, clip_len=L, flip=False, ops=WE.NumpyWildOps())
    assert net.calls == [(1, L, 17, 3), (2, 2, 17, 3)] and out[1].shape == (2, 17, 3)


def test_wrapped_model_and_views(kps):
    class Wrapped:                      # nn.DataParallel's public side
        def __init__(self, module):
            self.module = module

        def eval(self):
            self.module.eval()
            return self

        def __call__(self, x):
            return self.module(x)

    F = 2 * L + 3
    for flip in (False, True):
        got = wild.infer(Wrapped(WE.FixedNet()), kps[F], clip_len=L, flip=flip, ops=WE.NumpyWildOps())
        assert WE.differing(got, wild.infer(WE.FixedNet(), kps[F], clip_len=L, flip=flip, ops=WE.NumpyWildOps())) == 0
    # consecutive clips reach the network as a view of the input stage's output: no copy
    seen = []

    class Net(WE.FixedNet):
        def __call__(self, x):
            seen.append(x)
            return super().__call__(x)

    wild.infer(Net(), kps[F], clip_len=L, flip=False, ops=WE.NumpyWildOps())
    assert [tuple(x.shape[:2]) for x in seen] == [(2, L), (1, 3)]
    assert seen[1].data_ptr() == seen[0].data_ptr() + 2 * L * 17 * 3 * 4 and seen[0].is_contiguous()


def test_wild_input_interface(kps):
    kp, ops = kps[L + 1], WE.NumpyWildOps()
    y = wild.wild_input(kp, scale_range=[1, 1], ops=ops)
    assert y.dtype == torch.float32 and tuple(y.shape) == (L + 1, 17, 3)
    y2, box = wild.wild_input(torch.from_numpy(kp), scale_range=(1, 1), channels=2, return_box=True, ops=ops)
    assert tuple(y2.shape) == (L + 1, 17, 2) and WE.differing(y2.numpy(), np.ascontiguousarray(y.numpy()[..., :2])) == 0
    assert box.dtype == torch.float64 and tuple(box.shape) == (1, 4) and box[0, 3] == (L + 1) * 17
    # the box maps crop-mode coordinates back to pixels
    xs, ys, scale, _ = box[0].tolist()
    back = (y.numpy()[..., :2].astype(np.float64) / 2 + 0.5) * scale + [xs, ys]
    assert np.allclose(back, WE.halpe2h36m(kp)[..., :2], rtol=0, atol=1e-3)
    both = wild.wild_input(kp, vid_size=VID, scale_range=[1, 1], ops=ops)
    assert WE.differing(both.numpy(), WE.input_ref(kp, VID, [1, 1])[0]) == 0
    ratio = wild.wild_input(kp, scale_range=[1.25, 1.25], ops=ops)
    assert WE.differing(ratio.numpy(), WE.input_ref(kp, None, [1.25, 1.25])[0]) == 0
    empty = wild.wild_input(np.zeros((0, 26, 3)), scale_range=[1, 1], ops=ops)
    assert tuple(empty.shape) == (0, 17, 3)
    with pytest.raises(ValueError, match='pixel mode'):
        wild.wild_input(kp, ops=ops)
    with pytest.raises(ValueError, match='training'):
        wild.wild_input(kp, scale_range=[0.8, 1.0], ops=ops)
    with pytest.raises(ValueError, match='channels'):
        wild.wild_input(kp, scale_range=[1, 1], channels=1, ops=ops)
    with pytest.raises(ValueError, match='Halpe-26'):
        wild.wild_input(kp[:, :17], scale_range=[1, 1], ops=ops)
    with pytest.raises(ValueError, match='sum to'):
        wild.wild_input(kp, scale_range=[1, 1], seq_lens=[3, 3], ops=ops)
    with pytest.raises(ValueError, match='vid_size'):
        wild.wild_input(kp, vid_size=(0, 1080), ops=ops)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='ROCm device'):
            wild.wild_input(kp, scale_range=[1, 1])


def test_wild_output_interface():
    ops = WE.NumpyWildOps()
    case = WE.output_cases()['pixel.gt2d']
    dst = torch.full((case['F'], 17, 3), float('nan'))
    pred = torch.from_numpy(case['pred'])
    got = wild.wild_output(pred, dst, case['dst'].tolist(), x=torch.from_numpy(case['x']), gt_2d=True, vid_size=case['vid_size'], ops=ops)
    assert got is dst and WE.differing(dst.numpy(), WE.output_ref(case)) == 0 and WE.differing(pred.numpy(), case['pred']) == 0
    with pytest.raises(ValueError, match='does not fit'):
        wild.wild_output(pred, dst, [case['F']] * len(pred), ops=ops)
    with pytest.raises(ValueError, match='does not fit'):
        wild.wild_output(pred, dst, [-1] * len(pred), ops=ops)
    with pytest.raises(ValueError, match='offsets'):
        wild.wild_output(pred, dst, [0], ops=ops)
    with pytest.raises(ValueError, match='pass x'):
        wild.wild_output(pred, dst, case['dst'].tolist(), gt_2d=True, ops=ops)
    with pytest.raises(ValueError, match='pred'):
        wild.wild_output(pred[..., :2], dst, case['dst'].tolist(), ops=ops)
    with pytest.raises(ValueError, match='dst'):
        wild.wild_output(pred, dst.double(), case['dst'].tolist(), ops=ops)


def test_infer_argument_errors(kps):
    ops, kp = WE.NumpyWildOps(), kps[L]
    with pytest.raises(ValueError, match='maxlen'):
        wild.infer(WE.FixedNet(maxlen=L), kp, clip_len=L + 1, ops=ops)
    with pytest.raises(ValueError, match='vid_size'):
        wild.infer(WE.FixedNet(), kp, clip_len=L, pixel=True, ops=ops)
    with pytest.raises(ValueError, match='max_batch'):
        wild.infer(WE.FixedNet(), kp, clip_len=L, max_batch=0, ops=ops)
    with pytest.raises(ValueError, match='no tracks'):
        wild.infer(WE.FixedNet(), {}, clip_len=L, ops=ops)
    with pytest.raises(ValueError, match="track 'a'"):
        wild.infer(WE.FixedNet(), {'a': kp[:, :17]}, clip_len=L, ops=ops)
    with pytest.raises(RuntimeError, match='ROCm device'):
        wild.infer(WE.FixedNet(), kp, clip_len=L)                 # no provider, a model without parameters on the device
