"""Restatements, inputs, gates and a CPU provider for the mesh targets (mbx_mesh_gt in csrc/smpl.hip, motionbert_amd.mesh.mesh_targets,
motionbert_amd.data.pack_mesh / PackedMesh).  Plain module, no fixtures: tests/test_gpu_mesh_gt.py applies it to the kernels on the GPU,
tests/test_meshgterr.py to seeded corruptions on the CPU, tests/test_mesh_data.py to the data path; tools/mint_mesh_gt.py pins the exact
parts to the reference's own functions (tests/golden/mesh_gt.npz).  It imports tests/smplerr.py and tests/mesherr.py and changes neither.

  exact_targets             `theta`, `x2d` and the flags in numpy: copies, negations and one clip, restated from flip_thetas
                            (utils_mesh.py:458-484), flip_data (utils_data.py:54-66) and np.clip (dataset_mesh.py:67).  Compared bit for bit,
                            the sign of a negated zero included.
  body_targets              `kp_3d`, `verts`: no SMPL implementation exists next to this project, so the definition is the plain path of
                            tests/smplerr.py (plain_lbs on rodrigues_plain) in float64, followed by the data set's `* 1000`, the regressor and
                            the two root subtractions in the order of dataset_mesh.py:85-90.
  gates                     per output array  max |error| / max |float64 value|  at most 4 x what body_targets shows in float32 against itself
                            in float64 on the same inputs on the CPU, never less than 8 fp32 ulps (the standing rule of tests/mesherr.py).
                            Computed from the reference alone when the test runs; nothing read off a kernel enters it.
  inputs / flip_pattern     seeded clips with the planted rows, and the flip patterns
  MockOps                   smplerr.MockOps + `mesh_gt`: the fp32 model of the kernels on CPU tensors; `gt_corrupt` plants one of CORRUPTIONS
  make_pickle               small synthetic detection pickles for pack_mesh (h36m: four cameras, two sources, 40 frames)

One corruption of the issue's list needs a reading.  'root subtracted before the scale' as a pure reordering, (x - root) * 1000 against
x * 1000 - root * 1000, is the same number in exact arithmetic and differs by one rounding in float32: no gate that a float32 kernel can pass
can see it.  What the order of dataset_mesh.py:85-90 does protect against is a root TAKEN before the scale, metres subtracted from
millimetres; 'root_before_scale' plants that."""
import math

import numpy as np
import torch

from oracle import augment_oracle
from tests import mesherr as ME
from tests import smplerr as SE

F32, F64 = torch.float32, torch.float64
FLOOR = ME.FLOOR          # 8 fp32 ulps, the floor of every gate
SCALE = 1000.0
THETA_PAIRS = ((1, 2), (4, 5), (7, 8), (10, 11), (13, 14), (16, 17), (18, 19), (20, 21), (22, 23))       # utils_mesh.py:475
LEFT, RIGHT = (4, 5, 6, 11, 12, 13), (1, 2, 3, 14, 15, 16)                                                # utils_data.py:61-62

CORRUPTIONS = ('pairs_without_sign', 'sign_on_component_0', 'root_before_scale', 'root_from_joint_1', 'verts_uncentred', 'conf_unclipped',
               'x_not_negated', 'flag_by_frame', 'rodrigues_without_eps')


# ------------------------------------------------------------------------------------------------ the exact part
def flip_thetas(thetas, corrupt=None):
    """flip_thetas (utils_mesh.py:458-484) of [...,24,3] numpy: components 1 and 2 negated, the nine pairs swapped"""
    out = thetas.copy()
    neg = (0, 2) if corrupt == 'sign_on_component_0' else (1, 2)
    if corrupt != 'pairs_without_sign':
        for c in neg:
            out[..., c] = -1 * out[..., c]
    for a, b in THETA_PAIRS:
        out[..., a, :], out[..., b, :] = out[..., b, :].copy(), out[..., a, :].copy()
    return out


def flip_data(data, corrupt=None):
    """flip_data (utils_data.py:54-66) of [...,17,D] numpy"""
    out = data.copy()
    if corrupt != 'x_not_negated':
        out[..., 0] *= -1
    out[..., list(LEFT + RIGHT), :] = out[..., list(RIGHT + LEFT), :]
    return out


def frame_flags(flags, N, T, corrupt=None):
    """[N,T] bool: the flag every frame is treated with.  'flag_by_frame': frame f of the batch reads flags[f] where the clip's is
    flags[f // T] (past the end of the flags: no flip)"""
    flags = np.asarray(flags).astype(bool).reshape(N)
    if corrupt == 'flag_by_frame':
        padded = np.concatenate([flags, np.zeros(N * T - N, dtype=bool)])
        return padded.reshape(N, T)
    return np.repeat(flags[:, None], T, axis=1)


def exact_targets(pose, shape, motion_2d, flags, corrupt=None):
    """(x2d [N,T,17,3] or None, theta [N,T,82]) float32 numpy of pose [N,T,72], shape [N,T,10], motion_2d [N,T,17,3] (numpy float32) and the
    clip flags [N]: dataset_mesh.py:66-77,91 for every clip"""
    assert corrupt is None or corrupt in CORRUPTIONS
    N, T = pose.shape[:2]
    ff = frame_flags(flags, N, T, corrupt)
    p = pose.reshape(N, T, 24, 3)
    theta = np.concatenate([np.where(ff[:, :, None, None], flip_thetas(p, corrupt), p).reshape(N, T, 72), shape], axis=-1).astype(np.float32)
    x2d = None
    if motion_2d is not None:
        m = motion_2d.copy()
        if corrupt != 'conf_unclipped':
            m[..., 2] = np.clip(m[..., 2], 0, 1)
        x2d = np.where(ff[:, :, None, None], flip_data(m, corrupt), m).astype(np.float32)
    return x2d, theta


# ------------------------------------------------------------------------------------------------ the float64 definition of kp_3d and verts
def body_targets(model, theta, dtype, Q=None, scale=SCALE):
    """(kp_3d [N,T,K,3], verts [N,T,V,3]) in `dtype` from the fp32 bits of theta [N,T,82] (the pose AFTER the flip, and the shape): the
    plain path of tests/smplerr.py (rodrigues_plain, plain_lbs), `* scale`, the regressor, both root subtractions (dataset_mesh.py:79-90)"""
    theta = torch.as_tensor(theta)
    N, T = theta.shape[:2]
    th = theta.reshape(N * T, 82).to(dtype)
    m = SE.model_dict(model, dtype)
    Q = (model.J_regressor_h36m if Q is None else Q).to(dtype)
    rot = SE.rodrigues_plain(th[:, :72].reshape(-1, 3)).reshape(N * T, 24, 3, 3)
    verts = SE.plain_lbs(m, th[:, 72:], rot)[0] * scale
    kp = torch.matmul(Q[None].expand(N * T, -1, -1), verts)
    verts = verts - kp[:, :1, :]
    kp = kp - kp[:, :1, :]
    return kp.reshape(N, T, -1, 3), verts.reshape(N, T, -1, 3)


def gates(model, theta, Q=None, scale=SCALE):
    """(ref64, gate): the float64 kp_3d / verts and, per array, 4 x the stat of the float32 plain path against them (floor 8 ulps)"""
    k64, v64 = body_targets(model, theta, F64, Q, scale)
    k32, v32 = body_targets(model, theta, F32, Q, scale)
    return dict(kp_3d=k64, verts=v64), dict(kp_3d=SE.gate32(SE.stat(k32, k64)), verts=SE.gate32(SE.stat(v32, v64)))


def check(got, want_x2d, want_theta, want_flags, ref64, gate, report=None):
    """the list of failed gates of one mesh_gt result (`got`: dict x2d / theta / kp_3d / verts / flips_used, entries may be missing): the
    exact arrays bit for bit, the body arrays by stat / gate (recorded in `report`)"""
    failed = []
    for name, want in (('x2d', want_x2d), ('theta', want_theta)):
        if got.get(name) is not None and want is not None:
            g = np.ascontiguousarray(got[name].detach().cpu().numpy())
            if g.shape != want.shape or g.dtype != np.float32 or g.view(np.uint32).tolist() != np.ascontiguousarray(want).view(np.uint32).tolist():
                failed.append(name)
    if got.get('flips_used') is not None and got['flips_used'].cpu().numpy().astype(bool).tolist() != np.asarray(want_flags).astype(bool).tolist():
        failed.append('flips_used')
    for name in ('kp_3d', 'verts'):
        if got.get(name) is not None:
            r = SE.stat(got[name].reshape(ref64[name].shape), ref64[name]) / gate[name]
            if report is not None:
                report[name] = r
            if not r <= 1.0:
                failed.append(name)
    return failed


# ------------------------------------------------------------------------------------------------ inputs
TINY, NEAR_PI = 1e-9, 1e-3


def inputs(N, T, seed):
    """pose [N,T,72], shape [N,T,10], motion_2d [N,T,17,3] float32 tensors.  Joints are axis-angle vectors of length about 0.9.  Planted in
    EVERY frame: joints 22 and 23 (the hands of real fits) all-zero; joint 20 a vector of magnitude 1e-9; joint 21 (and, in frame 0, the
    global orientation) a rotation by an angle within 1e-3 of pi; one exactly zero component with its sign bit to be flipped (joint 19,
    component 1).  With more than one frame the last frame of the batch is all-zero (the rest pose).  The confidences run from below 0 to
    above 1 (about a fifth on either side), one of them exactly 0 and one exactly 1."""
    g = torch.Generator().manual_seed(seed)
    F = N * T
    pose = 0.5 * torch.randn(F, 24, 3, generator=g)
    pose[:, 22:] = 0.0
    d = torch.randn(F, 3, generator=g)
    pose[:, 20] = TINY * d / d.norm(dim=1, keepdim=True)
    d = torch.randn(F, 3, generator=g, dtype=F64)
    pose[:, 21] = ((math.pi - NEAR_PI * torch.rand(F, 1, generator=g, dtype=F64)) * d / d.norm(dim=1, keepdim=True)).float()
    pose[0, 0] = pose[0, 21][[1, 2, 0]]
    pose[:, 19, 1] = 0.0
    if F > 1:
        pose[F - 1] = 0.0
    shape = torch.randn(F, 10, generator=g)
    m2d = torch.cat([torch.rand(F, 17, 2, generator=g) * 2 - 1, torch.rand(F, 17, 1, generator=g) * 1.6 - 0.3], dim=-1)
    m2d[0, 0, 2], m2d[0, 1, 2] = 0.0, 1.0
    return pose.reshape(N, T, 72).float().contiguous(), shape.reshape(N, T, 10).float().contiguous(), m2d.reshape(N, T, 17, 3).float().contiguous()


PATTERNS = ('none', 'all', 'alternating')
EXACT_CASES = ((3, 2, 'alternating'), (2, 3, 'all'), (2, 1, 'none'), (5, 7, 'alternating'))       # (N, T, pattern) of the fixture


def exact_seed(N, T):
    return 7400 + 13 * N + T


def flip_pattern(N, kind):
    """[N] uint8 flags"""
    assert kind in PATTERNS
    return {'none': torch.zeros(N, dtype=torch.uint8), 'all': torch.ones(N, dtype=torch.uint8),
            'alternating': (torch.arange(N) % 2 == 0).to(torch.uint8)}[kind]


def drawn_flags(seed, N, flip_prob):
    """the flags mbx_mesh_gt draws: u(seed, stream 0, index n) < flip_prob with the counter-based hash of csrc/aug_rng.h"""
    return (augment_oracle.uniform(int(seed), 0, torch.arange(N, dtype=torch.int64)) < np.float32(flip_prob)).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ a kernel provider on the CPU
def _rodrigues32(aa, eps=True):
    """the prepare kernel's Rodrigues in float32 torch operations: angle = |r + 1e-8|, R = I + sin K + (1 - cos) K^2"""
    angle = (aa + (1e-8 if eps else 0.0)).norm(dim=1, keepdim=True)
    d = aa / angle
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    s, c = torch.sin(angle[:, 0]), 1.0 - torch.cos(angle[:, 0])
    return torch.stack([1.0 - c * (y * y + z * z), c * (x * y) - s * z, s * y + c * (x * z),
                        s * z + c * (x * y), 1.0 - c * (x * x + z * z), c * (y * z) - s * x,
                        c * (x * z) - s * y, s * x + c * (y * z), 1.0 - c * (x * x + y * y)], dim=1)


class MockOps(SE.MockOps):
    """smplerr.MockOps plus the mesh-target entries on CPU tensors, same argument lists as HipOps: the exact part from exact_targets, the
    body from forward_eq in float32 (the model of the chain and vertex kernels) on _rodrigues32.  `gt_corrupt` plants one of CORRUPTIONS."""

    def __init__(self, gt_corrupt=None):
        super().__init__()
        assert gt_corrupt is None or gt_corrupt in CORRUPTIONS
        self.gt_corrupt = gt_corrupt

    def mesh_gt_ws(self, F, V, K, device):
        return torch.empty(16, dtype=torch.uint8)

    def mesh_gt(self, model, Q, pose, shape, motion_2d, flips, seed, flip_prob, scale, x2d, theta, kp_3d, verts, flips_used, ws=None):
        self._count('mesh_gt')
        c = self.gt_corrupt
        N, T = pose.shape[:2]
        assert pose.dtype == F32 and shape.dtype == F32 and (flips is None or flips.dtype == torch.uint8)
        flags = flips if flips is not None else drawn_flags(seed, N, flip_prob)
        x, th = exact_targets(pose.numpy(), shape.numpy(), None if motion_2d is None else motion_2d.numpy(), flags.numpy(), c)
        if x2d is not None:
            x2d.copy_(torch.from_numpy(x))
        if theta is not None:
            theta.copy_(torch.from_numpy(th))
        if flips_used is not None:
            flips_used.copy_(flags)
        if kp_3d is None and verts is None:
            return
        th = torch.from_numpy(th).reshape(N * T, 82)
        rot = _rodrigues32(th[:, :72].reshape(-1, 3), eps=c != 'rodrigues_without_eps').reshape(N * T, 24, 3, 3)
        s = float(np.float32(scale))
        v, k, _ = SE.forward_eq(self._m(model), th[:, 72:].contiguous(), rot, Q.float(), s)
        root = k[:, 1:2] if c == 'root_from_joint_1' else (k[:, :1] / s if c == 'root_before_scale' else k[:, :1])
        if kp_3d is not None:
            kp_3d.copy_((k - root).reshape(kp_3d.shape))
        if verts is not None:
            verts.copy_((v if c == 'verts_uncentred' else v - root).reshape(verts.shape))


def run_mock(layer, pose, shape, motion_2d, flags, gt_corrupt=None, want=('theta', 'kp_3d', 'verts')):
    """mesh_targets driven through MockOps: the dict check() takes"""
    from motionbert_amd.mesh import mesh_targets
    x2d, out, used = mesh_targets(layer, pose, shape, motion_2d, flip=flags, want=want, return_flips=True, ops=MockOps(gt_corrupt))
    return dict(out, x2d=x2d, flips_used=used)


# ------------------------------------------------------------------------------------------------ detection pickles for pack_mesh
CAMERAS = ('54138969', '55011271', '58860488', '60457274')
PACK_CASES = (('h36m', 8, 4), ('pw3d', 8, 4), ('coco', 8, 4))        # (dataset, clip_len, data_stride)
PACK_SEED = {'h36m': 8101, 'pw3d': 8102, 'coco': 8103}


def _part(rng, sources, cameras=None, conf_dims=3):
    n = len(sources)
    d = {'joint_2d': rng.uniform(0, 1000, size=(n, 17, 3)), 'source': list(sources),
         'confidence': rng.uniform(-0.2, 1.2, size=(n, 17, 1) if conf_dims == 3 else (n, 17)),
         'smpl_pose': rng.normal(0, 0.5, size=(n, 72)), 'smpl_shape': rng.normal(0, 1, size=(n, 10))}
    if cameras is not None:
        d['camera_name'] = [cameras[s] for s in sources]
    return d


def make_pickle(dataset, seed):
    """{'train', 'test'}: what read_pkl returns for the detection file of `dataset`.  h36m: 40 frames per split from two sources and four
    cameras (the source names carry the camera; a source of 23 frames and one of 17: with clips of 8 frames the first leaves a window
    unfinished at its end, and a third, short source of 5 frames in the middle of the train split is resampled with random rounding);
    pw3d: three sources, one of them shorter than a clip; coco: single frames, two-dimensional confidences."""
    rng = np.random.RandomState(seed)
    if dataset == 'h36m':
        cams = {f's{k}.{c}': c for k in range(4) for c in CAMERAS}
        train = [f's0.{CAMERAS[0]}'] * 18 + [f's2.{CAMERAS[2]}'] * 5 + [f's1.{CAMERAS[1]}'] * 17
        test = [f's0.{CAMERAS[3]}'] * 23 + [f's1.{CAMERAS[2]}'] * 17
        return {'train': _part(rng, train, cams), 'test': _part(rng, test, cams)}
    if dataset == 'pw3d':
        train = ['a'] * 13 + ['b'] * 6 + ['c'] * 11
        test = ['d'] * 5 + ['e'] * 19
        return {'train': _part(rng, train), 'test': _part(rng, test)}
    assert dataset == 'coco'
    return {'train': _part(rng, [f'img{i}' for i in range(12)], conf_dims=2), 'test': _part(rng, [f'val{i}' for i in range(7)], conf_dims=2)}
