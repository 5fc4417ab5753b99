"""Restatements, inputs and gates for the action-recognition kernels (csrc/action.hip): mbx_action_input (lib/data/dataset_action.py:76-112,
173-182 + lib/utils/utils_data.py:7-29) and mbx_xent_topk (train_action.py:55-61,180-184 + lib/utils/learning.py:25-37).  Plain module, no
fixtures: tests/test_gpu_action.py applies it to the kernels on the GPU, tests/test_actionerr.py to seeded corruptions on the CPU,
tools/mint_action.py pins it to the reference's own code at 1e-12 (tests/golden/action.npz).

  action_input_eq / action_input_ref64   random_move + crop_scale for a batch in torch, in a chosen dtype (float64: the restatement;
                                         float32: the same equations, the yardstick of the gates)
  xent_topk_eq / xent_topk_ref64         row losses, mean, gradient, ranks and top-1 / top-5 hits, likewise
  motion_inputs / planted_motion / logit_inputs / planted_logits / annotations   seeded inputs (not stored in the fixture, but for the
                                         annotation arrays)
  input_gate / xent_gates                the gates
  TorchActionOps                         the two entries of the kernel provider on CPU tensors, for the host-logic tests

Gates.  The yardstick is the SAME equations evaluated in float32 by torch on the CPU against float64, per sample (input stage) and per row
(loss, gradient), as a max-norm.  The device gets 4 x that: a factor 2 for device sin / cos / exp / log documented at 2 ulp where the CPU's
are 1 and for fused multiply-adds that round in other places, a factor 2 for comparing maxima over different rounding patterns (the
factors of tests/mesherr.py).  Floors, so that a sample or row which float32 happens to get exactly does not yield a zero gate -- 8 fp32
ulps (mesherr.FLOOR) of
  * input stage: the largest magnitude the output went through.  The written value is x'' = 2 (x' - xs) / scale - 1: a rounding of x'
    (half an ulp of |x'|) comes out multiplied by 2 / scale, so the magnitude is max(|output|, 2 max(|x'|, |y'|) / scale), and
    max(|x'|, |y'|, |c|) without the crop;
  * row loss: max(1, |loss|).  The loss is log(s) - (z_y - m) with s >= 1 (the maximum contributes exp(0)): half an ulp of s is an
    absolute error of up to 2^-24 in log(s) however small the loss itself is;
  * gradient row: max_j softmax_j * |grad_scale| / N, the magnitude before the one-hot is subtracted (p_y - 1 cancels when p_y is near 1).
The mean loss: the kernel adds the row losses in fp64 and rounds once, so its gate is the mean of the row gates plus one ulp of the mean.
The discrete outcomes -- which samples are zeroed, the hit counts, params_out against params_in -- must match exactly."""
import numpy as np
import torch

from oracle import augment_oracle

EPS32 = 2.0 ** -23
FLOOR = 8 * EPS32
FACTOR = 4.0
RANGES = ((-10.0, 10.0), (0.9, 1.1), (-0.1, 0.1))         # random_move's defaults: angle (degrees), scale, translation
CROP_DEFAULT = (1.0, 1.0)
CROP_CLIP = (0.5, 0.7)                                    # a box smaller than the skeleton: the clip is active
MOVE, CROP = 1, 2

INPUT_CORRUPTIONS = ('second_person_still', 'no_end_point', 'box_over_all', 'div_ratio', 'conf_unclipped', 'threshold_3')
XENT_CORRUPTIONS = ('no_div_n', 'ge_rank')
CORRUPTIONS = INPUT_CORRUPTIONS + XENT_CORRUPTIONS


# ------------------------------------------------------------------------------------------------ input stage
def action_input_eq(x, params, flags, dtype, corrupt=None, clip=True):
    """(y [N,M,T,J,3], zeroed [N] bool, mag [N]) of x [N,M,T,J,3] and params [N,9] = A0 A1 S0 S1 Tx0 Tx1 Ty0 Ty1 ratio, evaluated in `dtype`.
    mag: the magnitude the gate's floor refers to (module docstring).  clip=False leaves the normalised values unclipped (for
    clipped_fraction).  corrupt: one of INPUT_CORRUPTIONS."""
    assert corrupt is None or corrupt in INPUT_CORRUPTIONS
    x, p = x.to(dtype), params.to(dtype)
    N, M, T, J, _ = x.shape
    px, py, c = x[..., 0], x[..., 1], x[..., 2]
    if flags & MOVE:
        t = torch.arange(T, dtype=dtype, device=x.device)
        f = t / (T if corrupt == 'no_end_point' else T - 1) if T > 1 else torch.zeros(T, dtype=dtype, device=x.device)
        lerp = lambda k: (p[:, k, None] + (p[:, k + 1, None] - p[:, k, None]) * f[None]).reshape(N, 1, T, 1)       # noqa: E731
        a = lerp(0) * (np.pi / 180)
        s, tx, ty = lerp(2), lerp(4), lerp(6)
        cs, sn = torch.cos(a) * s, torch.sin(a) * s
        mx, my = cs * px - sn * py + tx, sn * px + cs * py + ty
        if corrupt == 'second_person_still' and M > 1:
            mx, my = torch.cat([mx[:, :1], px[:, 1:]], 1), torch.cat([my[:, :1], py[:, 1:]], 1)
    else:
        mx, my = px, py
    amax = torch.maximum(mx.abs().amax(dim=(1, 2, 3)), my.abs().amax(dim=(1, 2, 3)))
    if not flags & CROP:
        return torch.stack([mx, my, c], -1), torch.zeros(N, dtype=torch.bool, device=x.device), torch.maximum(amax, c.abs().amax(dim=(1, 2, 3)))
    valid = torch.ones_like(c, dtype=torch.bool) if corrupt == 'box_over_all' else c != 0
    inf = torch.full_like(mx, float('inf'))
    xmin, xmax = torch.where(valid, mx, inf).amin(dim=(1, 2, 3)), torch.where(valid, mx, -inf).amax(dim=(1, 2, 3))
    ymin, ymax = torch.where(valid, my, inf).amin(dim=(1, 2, 3)), torch.where(valid, my, -inf).amax(dim=(1, 2, 3))
    count = (c != 0).sum(dim=(1, 2, 3))
    ext = torch.maximum(xmax - xmin, ymax - ymin)
    scale = ext / p[:, 8] if corrupt == 'div_ratio' else ext * p[:, 8]
    zeroed = (count < (3 if corrupt == 'threshold_3' else 4)) | (scale == 0)
    scale = torch.where(zeroed, torch.ones_like(scale), scale)
    xs, ys = (xmin + xmax - scale) / 2, (ymin + ymax - scale) / 2
    v = lambda q: q.reshape(N, 1, 1, 1)                                                                       # noqa: E731
    ox, oy, oc = ((mx - v(xs)) / v(scale) - 0.5) * 2, ((my - v(ys)) / v(scale) - 0.5) * 2, c
    if clip:
        ox, oy = ox.clamp(-1, 1), oy.clamp(-1, 1)
        oc = c if corrupt == 'conf_unclipped' else c.clamp(-1, 1)
    y = torch.stack([ox, oy, oc], -1)
    y = torch.where(v(zeroed).unsqueeze(-1), torch.zeros_like(y), y)
    mag = torch.maximum(y.abs().amax(dim=(1, 2, 3, 4)), 2 * amax / scale)
    return y, zeroed, torch.where(zeroed, torch.ones_like(mag), mag)


def action_input_ref64(x, params, flags, corrupt=None):
    return action_input_eq(x, params, flags, torch.float64, corrupt)


def clipped_fraction(x, params, flags):
    """the share of the x, y coordinates of the batch that the clip changes, on the float64 restatement alone"""
    y, _, _ = action_input_eq(x, params, flags, torch.float64, clip=False)
    return float((y[..., :2].abs() > 1 + 1e-9).double().mean())


def input_gate(got, x, params, flags):
    """(worst share of a sample's gate, zeroed as the float64 restatement has it, per-sample shares) for a kernel output `got` of the
    fp32 inputs x, params"""
    ref, gate, zero = input_gates(x, params, flags)
    got = got.detach().cpu()
    err = (got.double() - ref).abs().amax(dim=(1, 2, 3, 4))
    share = torch.nan_to_num(err / gate, nan=float('inf'))
    return float(share.max()), bool(torch.equal((got == 0).reshape(len(got), -1).all(1), zero)), share


def input_gates(x, params, flags):
    """(float64 output, per-sample gate [N], all-zero samples [N]) for the fp32 inputs x, params"""
    ref, zeroed, mag = action_input_eq(x, params, flags, torch.float64)
    y32, _, _ = action_input_eq(x, params, flags, torch.float32)
    yard = (y32.double() - ref).abs().amax(dim=(1, 2, 3, 4))
    return ref, torch.maximum(FACTOR * yard, FLOOR * mag), zeroed | (ref == 0).reshape(len(ref), -1).all(1)


def draw_params(N, seed, crop_range=CROP_DEFAULT, ranges=RANGES):
    """params [N,9] fp32 exactly as mbx_action_input forms them from `seed`: min(fma(hi - lo, u(stream k, index n), lo), hi) with the
    counter-based uniform numbers of oracle/augment_oracle.py.  The fused multiply-add is restated in float64, where the product of two
    fp32 numbers is exact and the sum is rounded once more only at a distance from an fp32 tie that no draw of the tests comes near."""
    idx = torch.arange(N, dtype=torch.int64)
    cols = []
    for k in range(9):
        lo, hi = ranges[k // 2] if k < 4 else ranges[2] if k < 8 else crop_range
        lo, hi = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
        v = ((hi - lo).double() * augment_oracle.uniform(seed, k, idx).double() + lo.double()).float()
        cols.append(torch.minimum(v, hi))
    return torch.stack(cols, 1)


def host_params(N, seed, crop_range=CROP_DEFAULT):
    """params [N,9] fp32 from numpy's generator in the order random_move and crop_scale draw them (for the params_in tests)"""
    r = np.random.RandomState(seed)
    rows = []
    for _ in range(N):
        rows.append(np.concatenate([r.uniform(lo, hi, 2) for lo, hi in (RANGES[0], RANGES[1], RANGES[2], RANGES[2])] + [r.uniform(*crop_range, size=1)]))
    return torch.from_numpy(np.asarray(rows, dtype=np.float32))


def motion_inputs(N, M, T, J, seed):
    """x [N,M,T,J,3] fp32, NTU-like after pack_action: each person a cloud of joints around a centre that drifts over the clip, confidences
    in [0.3, 1).  A sample of 500 joints or more has about 0.3 % of them undetected: confidence 0 and parked near the image corner
    (-1, -1), outside the box of the rest."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand(N, M, 1, 1, 2, generator=g) - 0.5
    drift = 0.2 * (torch.rand(N, M, 1, 1, 2, generator=g) - 0.5) * torch.linspace(0, 1, T).reshape(1, 1, T, 1, 1)
    pose = 0.15 * torch.randn(N, M, 1, J, 2, generator=g) + 0.02 * torch.randn(N, M, T, J, 2, generator=g)
    conf = 0.3 + 0.7 * torch.rand(N, M, T, J, 1, generator=g)
    x = torch.cat([centre + drift + pose, conf], -1)
    if M * T * J >= 500:
        lost = torch.rand(N, M, T, J, generator=g) < 0.003
        x[lost] = torch.tensor([-1.0, -1.0, 0.0]) + torch.cat([0.01 * torch.rand(int(lost.sum()), 2, generator=g), torch.zeros(int(lost.sum()), 1)], 1)
    return x.float().contiguous()


PLANTED = ('all_conf_0', 'three_valid', 'four_valid', 'coincident', 'fake_second', 'conf_1p5', 'plain')


def planted_motion(seed=7300, T=9, J=17):
    """x [7,2,T,J,3]: the samples of PLANTED.  In the few-valid samples every undetected joint lies well inside the box of the valid ones
    (which sit at (+-0.5, +-0.5) in frame 0), and the fake second person inside the box of the first, so that nothing is clipped there."""
    g = torch.Generator().manual_seed(seed)
    x = motion_inputs(len(PLANTED), 2, T, J, seed + 1)
    corners = torch.tensor([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]])
    x[0, ..., 2] = 0.0
    for n, k in ((1, 3), (2, 4)):
        x[n, ..., :2] = 0.3 * (torch.rand(2, T, J, 2, generator=g) - 0.5)
        x[n, ..., 2] = 0.0
        x[n, 0, 0, :k, :2] = corners[:k]
        x[n, 0, 0, :k, 2] = 0.9
    x[3, ..., 2] = 0.0                       # five valid joints of one frame at one point: scale == 0 exactly, in any precision
    x[3, 1, T // 2, 3:8, :2] = torch.tensor([0.25, -0.125])
    x[3, 1, T // 2, 3:8, 2] = 0.8
    x[4, 1] = 0.0                            # the all-zero second person pack_action adds: moved to (tx_t, ty_t), confidence 0
    x[4, 0, ..., :2] -= x[4, 0, ..., :2].mean(dim=(0, 1))       # the first person around the origin: the second lands inside its box
    x[5, 0, :, ::3, 2] = 1.5
    x[5, 1, :, 1::4, 2] = -1.5
    return x.contiguous()


# (N, M, T) at J = 17: the issue's list, then a clip longer than the kernel's frame table (AI_FRAMES = 512 in csrc/action.hip) and the table's
# exact size, so that one, two and a partial second chunk occur
INPUT_SHAPES = ((1, 1, 1), (2, 2, 2), (3, 2, 27), (5, 1, 64), (2, 2, 243), (1, 2, 486), (1, 1, 512), (1, 1, 600))
CLIP_SHAPE = (3, 2, 27)
FLAG_SHAPE = (2, 2, 9)


def input_seed(shape):
    return 7100 + sum(int(v) * w for v, w in zip(shape, (1, 17, 289))) % 9973


def input_cases():
    """name -> (x, flags, crop_range): every case of the fixture and of the GPU parity test; the nine draws per sample are the fixture's
    `{name}.params` (case_params)"""
    cases = {}
    for shape in INPUT_SHAPES:
        cases['in.%d.%d.%d' % shape] = (motion_inputs(*shape, 17, input_seed(shape)), MOVE | CROP, CROP_DEFAULT)
    cases['in.planted'] = (planted_motion(), MOVE | CROP, CROP_DEFAULT)
    cases['in.clip'] = (motion_inputs(*CLIP_SHAPE, 17, 7400), MOVE | CROP, CROP_CLIP)
    for flags in (0, MOVE, CROP):
        cases['in.flags%d' % flags] = (motion_inputs(*FLAG_SHAPE, 17, 7500), flags, CROP_DEFAULT)
    return cases


def case_params(fixture, name):
    """params [N,9] fp32 of a case: numpy's draws as the reference made them, float32 values (tools/mint_action.py)"""
    p = torch.from_numpy(fixture[name + '.params'])
    assert torch.equal(p.float().double(), p), name
    return p.float()


def fixture_frames(T):
    """frames of a case the fixture keeps: all, or the first and last 8 and every 8th of a clip of more than 64 frames"""
    return np.arange(T) if T <= 64 else np.unique(np.concatenate([np.arange(8), np.arange(T - 8, T), np.arange(0, T, 8)]))


# ------------------------------------------------------------------------------------------------ cross-entropy and top-k
def xent_topk_eq(logits, labels, dtype, gscale=1.0, corrupt=None):
    """dict(row_loss [N], loss, d [N,C], rank [N], hit1, hit5, pmax [N]) of logits [N,C] (fp32 bits) and labels [N], evaluated in `dtype`.  A
    label outside [0, C): NaN in the row's loss and gradient, no hit."""
    assert corrupt is None or corrupt in XENT_CORRUPTIONS
    z = logits.to(dtype)
    N, C = z.shape
    lab = labels.long()
    ok = (lab >= 0) & (lab < C)
    safe = torch.where(ok, lab, torch.zeros_like(lab))
    m = z.amax(dim=1, keepdim=True)
    e = torch.exp(z - m)
    s = e.sum(dim=1, keepdim=True)
    zy = z.gather(1, safe[:, None])
    nan = torch.full((N,), float('nan'), dtype=dtype)
    row_loss = torch.where(ok, (torch.log(s) - (zy - m))[:, 0], nan)
    onehot = torch.zeros_like(z).scatter_(1, safe[:, None], 1.0)
    scale = torch.tensor(gscale, dtype=dtype) / (1 if corrupt == 'no_div_n' else N)
    d = torch.where(ok[:, None], (e / s - onehot) * scale, nan[:, None])
    col = torch.arange(C)[None]
    if corrupt == 'ge_rank':
        rank = ((z >= zy) & (col != safe[:, None])).sum(1)
    else:
        rank = ((z > zy) | ((z == zy) & (col < safe[:, None]))).sum(1)
    return dict(row_loss=row_loss, loss=row_loss.mean(), d=d, rank=rank, hit1=int(((rank < 1) & ok).sum()), hit5=int(((rank < 5) & ok).sum()),
                pmax=(e / s).amax(dim=1))


def xent_topk_ref64(logits, labels, gscale=1.0, corrupt=None):
    return xent_topk_eq(logits, labels, torch.float64, gscale, corrupt)


def xent_gates(logits, labels, gscale=1.0):
    """(float64 results, row-loss gates [N], mean-loss gate, gradient row gates [N])"""
    r64, r32 = xent_topk_eq(logits, labels, torch.float64, gscale), xent_topk_eq(logits, labels, torch.float32, gscale)
    N = logits.shape[0]
    ok = ~torch.isnan(r64['row_loss'])
    l64 = torch.where(ok, r64['row_loss'], torch.zeros_like(r64['row_loss']))
    yard = torch.where(ok, (r32['row_loss'].double() - r64['row_loss']).abs(), torch.zeros_like(l64))
    g_row = torch.maximum(FACTOR * yard, FLOOR * l64.abs().clamp_min(1.0))
    g_mean = g_row.mean() + EPS32 * l64.mean().abs()
    dy = torch.where(ok[:, None], (r32['d'].double() - r64['d']).abs(), torch.zeros_like(r64['d'])).amax(dim=1)
    g_d = torch.maximum(FACTOR * dy, FLOOR * r64['pmax'] * abs(gscale) / N)
    return r64, g_row, float(g_mean), g_d


def same_nan(a, b):
    return bool(torch.equal(torch.isnan(a), torch.isnan(b)))


def xent_check(values, dlogits, logits, labels, gscale=1.0):
    """shares of the gates for one kernel call: dict(loss, grad, exact) with exact = hit counts and NaN pattern as float64 has them"""
    r64, _, g_mean, g_d = xent_gates(logits, labels, gscale)
    values = values.detach().cpu().double()
    exact = int(values[1]) == r64['hit1'] and int(values[2]) == r64['hit5'] and bool(torch.isnan(values[0])) == bool(torch.isnan(r64['loss']))
    loss_share = 0.0 if torch.isnan(r64['loss']) else float((values[0] - r64['loss']).abs() / g_mean)
    grad_share = 0.0
    if dlogits is not None:
        d = dlogits.detach().cpu().double()
        exact = exact and same_nan(d, r64['d'])
        err = torch.where(torch.isnan(r64['d']), torch.zeros_like(d), (d - r64['d']).abs()).amax(dim=1)
        grad_share = float(torch.nan_to_num(err / g_d, nan=float('inf')).max())
    return dict(loss=loss_share, grad=grad_share, exact=bool(exact))


def logit_inputs(N, C, seed):
    """logits [N,C] fp32 (scores of spread 3 with the target's raised, so that top-1, top-5 and misses all occur), labels [N] int64;
    tie-free (asserted)"""
    g = torch.Generator().manual_seed(seed)
    z = (2.0 * torch.randn(N, C, generator=g)).float()
    lab = torch.randint(0, C, (N,), generator=g)
    z[torch.arange(N), lab] += 6.0 * torch.rand(N, generator=g)
    for _ in range(64):
        tied = torch.tensor([len(torch.unique(r)) < C for r in z])
        if not bool(tied.any()):
            break
        z[tied] = (2.0 * torch.randn(int(tied.sum()), C, generator=g)).float()      # a row with two equal scores is drawn again
    else:
        raise AssertionError('logit_inputs: could not remove every tie')
    z = z.contiguous()
    return z, lab


def planted_logits(C=61, seed=7700):
    """logits [9,C], labels [9]: the target at +80 among -80; at -80 among +80; one foreign score of 1e4; the target exactly 5th; exactly
    6th; tied for the maximum with a LATER column (a hit: rank 0); tied with an EARLIER column (rank 1); a six-way tie for the maximum
    with the target last (rank 5: no top-5 hit); an ordinary row."""
    z, lab = logit_inputs(9, C, seed)
    z = z.clamp(-8, 8)
    lab = torch.full((9,), 20, dtype=torch.int64)
    z[0], z[1] = -80.0, 80.0
    z[0, 20], z[1, 20] = 80.0, -80.0
    z[2, 33] = 1e4
    for r, k in ((3, 4), (4, 5)):
        z[r, 20] = 20.0
        z[r, 40:40 + k] = 21.0 + torch.arange(k, dtype=torch.float32)
    z[5, 20] = z[5, 50] = 30.0
    z[6, 20] = z[6, 3] = 30.0
    z[7, 20] = 30.0
    z[7, 5:10] = 30.0
    return z.contiguous(), lab


def bad_label_logits(C=61, seed=7701):
    """logits [4,C] with labels [C, 5, -1, 7]: rows 0 and 2 have no class"""
    z, lab = logit_inputs(4, C, seed)
    return z, torch.tensor([C, 5, -1, 7])


XENT_SHAPES = ((1, 5), (2, 60), (32, 60), (33, 120), (257, 61), (64, 1000))


def xent_seed(shape):
    return 7600 + (shape[0] * 31 + shape[1]) % 997


def fixture_rows(n, width, limit=16384):
    """rows of an [n, width] gradient the fixture keeps: all, or the first and last 4 of an array of more than `limit` elements"""
    return np.arange(n) if n * width <= limit else np.concatenate([np.arange(4), np.arange(n - 4, n)])


# ------------------------------------------------------------------------------------------------ a synthetic annotation file
ANN_FRAMES = (7, 20, 27, 60, 243, 500)       # total_frames per sample: shorter than, equal to and longer than n_frames = 27
ANN_PERSONS = (1, 2, 1, 2, 2, 1)
ANN_N_FRAMES = 27
ANN_SPLITS = {'xsub_train': (0, 1, 4, 5), 'xsub_val': (2, 3, 5)}


def annotations(seed=7800):
    """the arrays of a six-sample NTU annotation file as float16 (the dtype of the published pickles): keypoint [M,T0,17,2] in pixels of a
    1080 x 1920 image, keypoint_score [M,T0,17]; two-person samples cross paths, so that the tracking swaps names"""
    r = np.random.RandomState(seed)
    out = []
    for i, (T0, M) in enumerate(zip(ANN_FRAMES, ANN_PERSONS)):
        start = r.uniform(300, 1600, (M, 1, 1, 2)) * np.array([1.0, 0.5])
        walk = np.cumsum(r.normal(0, 6, (M, T0, 1, 2)), axis=1)
        if M == 2:
            walk[1] += (start[0] - start[1]) * np.linspace(0, 1.2, T0).reshape(T0, 1, 1)
        kp = start + walk + r.normal(0, 40, (M, 1, 17, 2)) + r.normal(0, 2, (M, T0, 17, 2))
        out.append(dict(frame_dir='S%03d' % i, label=int(r.randint(60)), total_frames=T0, img_shape=(1080, 1920),
                        keypoint=kp.astype(np.float16), keypoint_score=r.uniform(0.2, 1.0, (M, T0, 17)).astype(np.float16)))
    return out


def annotation_file(anns):
    return dict(split={k: [anns[i]['frame_dir'] for i in v] for k, v in ANN_SPLITS.items()}, annotations=anns)


# ------------------------------------------------------------------------------------------------ a kernel provider in torch (CPU tests)
class TorchActionOps:
    """The action entries of the kernel provider on CPU tensors, from the float64 restatements: same argument lists as HipOps, results
    rounded to the outputs' dtype.  `calls` lists the entries used."""

    def __init__(self):
        self.calls = []

    def action_input(self, x, y, params_in, params_out, ranges, flags, seed):
        assert x.dtype == torch.float32 and x.is_contiguous() and y.shape == x.shape
        self.calls.append(('action_input', tuple(x.shape), int(flags), int(seed), params_in is not None))
        p = params_in if params_in is not None else draw_params(x.shape[0], int(seed), crop_range=ranges[3], ranges=ranges[:3])
        if params_out is not None:
            params_out.copy_(p)
        y.copy_(action_input_ref64(x, p, flags)[0])

    def xent_topk(self, logits, labels, values, dlogits, acc, grad_scale=1.0):
        assert logits.dtype == torch.float32 and logits.is_contiguous() and labels.dtype == torch.int32
        self.calls.append(('xent_topk', tuple(logits.shape), dlogits is not None, acc is not None))
        r = xent_topk_ref64(logits, labels, grad_scale)
        values.copy_(torch.stack([r['loss'], torch.tensor(float(r['hit1'])), torch.tensor(float(r['hit5']))]))
        if dlogits is not None:
            dlogits.copy_(r['d'])
        if acc is not None:
            acc += torch.tensor([float(r['row_loss'].sum()), r['hit1'], r['hit5'], logits.shape[0]], dtype=torch.float64)
