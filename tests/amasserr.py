"""Restatements, inputs, gates and a CPU provider for the AMASS kernel (csrc/amass.hip, motionbert_amd/amass.py).  Plain module, no fixtures:
tests/test_gpu_amass.py applies it to the kernel on the GPU, tests/test_amasserr.py to the identity, analytic cases and seeded corruptions on
the CPU, tests/test_amass.py drives the Python layer through `MockOps`.

`human_body_prior` is not a dependency of this project and its BodyModel cannot be run next to it, so the body model is pinned as SMPL was
(tests/smplerr.py), twice and independently:

  plain_lbs_h      SMPL-H + DMPL the way `smplx.lbs.lbs` writes it for BodyModel(num_betas=16, num_dmpls=8): 52 joints, 24 coefficients
                   c = [betas, dmpls] on [shapedirs | dmpldirs], J_regressor applied to the shaped vertices, 4x4 homogeneous transforms chained
                   by batched matmuls, the [F,V,4,4] per-vertex transform tensor, + trans, then Q @ vertices.  Float64 is the definition,
                   float32 the yardstick (and, on the device, what a user without the kernel would run: `PlainSMPLH`).
  folded_eq        the equations of include/mbx.h (mbx_amass_joints) term by term on the folded model, in the dtype of their inputs; float32
                   on the model's stored fold is what `MockOps` runs.  `corrupt=` plants one of CORRUPTIONS.

Gate (the standing rule of tests/mesherr.py): per output array  stat = max |error| / max |float64 value|  may be at most 4 x the stat of
plain_lbs_h in float32 against plain_lbs_h in float64 on the same inputs, computed on the CPU when the test runs; never less than 8 fp32 ulps.
Nothing is read off the kernel."""
import numpy as np
import torch

from motionbert_amd import amass as AM
from tests import mesherr as ME

F32, F64 = torch.float32, torch.float64
FLOOR = ME.FLOOR
stat = ME.stat
gate32 = ME.gate32
CAM_SCALE = float(np.float32(0.298))

CORRUPTIONS = ('wrong_parent', 'pf_with_identity', 'hand_pose_dropped', 'dmpl_not_in_Jd', 'A_without_offset', 'weights_transposed',
               'last_pair_dropped', 'trans_dropped', 'camera_axes_unswapped', 'camera_scale_missing')
RAW = ('v_template', 'shapedirs', 'dmpldirs', 'posedirs', 'J_regressor', 'weights', 'J_regressor_h36m')


# ------------------------------------------------------------------------------------------------ the model in a dtype
def fold(raw, pairs):
    """Jt, Jd, P [Np,3,484], s, qs of include/mbx.h from the raw arrays, in their dtype, by dense sums over the vertices"""
    S = torch.cat([raw['shapedirs'], raw['dmpldirs']], dim=2)
    D = torch.cat([raw['v_template'][:, :, None], S, raw['posedirs']], dim=2)                 # [V,3,484]
    Q, w = raw['J_regressor_h36m'], raw['weights']
    j, k = pairs[:, 0].long(), pairs[:, 1].long()
    coef = Q[j] * w[:, k].t()                                                                  # [Np,V]
    return dict(Jt=raw['J_regressor'] @ raw['v_template'], Jd=torch.einsum('jv,vck->jck', raw['J_regressor'], S),
                P=torch.einsum('pv,vcn->pcn', coef, D), s=coef.sum(1), qs=Q.sum(1))


def model_dict(model, dtype=F64, exact_fold=False, corrupt=None, device=None):
    """the raw arrays of an SMPLHModel in `dtype` (the fp32 bits, widened) and the fold: the model's stored fp32 arrays (what the kernel
    reads), or with exact_fold the sums formed in `dtype`"""
    d = {k: getattr(model, k).to(device=device, dtype=dtype) for k in RAW}
    d['pairs'] = model.pairs.to(device=device)
    d['parents'] = tuple(model.parents)
    if corrupt == 'weights_transposed':
        d['weights'] = d['weights'].reshape(-1).reshape(52, -1).t().contiguous()               # the flat array read as [k,v]
        exact_fold = True
        live = torch.einsum('jv,vk->jk', (d['J_regressor_h36m'] != 0).to(dtype), (d['weights'] != 0).to(dtype)) > 0
        d['pairs'] = live.nonzero().to(torch.int32)
    if exact_fold:
        d.update(fold(d, d['pairs']))
    else:
        d.update({k: getattr(model, k).to(device=device, dtype=dtype) for k in ('Jt', 'Jd', 'P', 's', 'qs')})
    return d


def rodrigues_plain(aa):
    """smplx's batch_rodrigues of [M,3] in the dtype of aa: angle = |r + 1e-8|, R = I + sin K + (1 - cos) K K"""
    angle = (aa + 1e-8).norm(dim=1, keepdim=True)
    d = aa / angle
    K = torch.zeros(aa.shape[0], 3, 3, dtype=aa.dtype, device=aa.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    return torch.eye(3, dtype=aa.dtype, device=aa.device) + torch.sin(angle)[:, :, None] * K + (1 - torch.cos(angle))[:, :, None] * (K @ K)


def _coef(betas, dmpls, F):
    b = betas[None].expand(F, -1) if betas.dim() == 1 else betas
    d = torch.zeros(F, 8, dtype=b.dtype, device=b.device) if dmpls is None else dmpls
    return torch.cat([b, d], dim=1)


def camera_step(kp, corrupt=None):
    """convert_amass.py:26-31 in the dtype of kp: (x, y, z) -> (x, -z, y), then x float32(0.298)"""
    if corrupt != 'camera_axes_unswapped':
        kp = torch.stack([kp[..., 0], -kp[..., 2], kp[..., 1]], dim=-1)
    return kp if corrupt == 'camera_scale_missing' else kp * CAM_SCALE


# ------------------------------------------------------------------------------------------------ the way smplx / BodyModel write it
def plain_lbs_h(m, poses, betas, dmpls=None, trans=None, camera=False):
    """kp [F,K,3] = Q @ (lbs vertices + trans) in the dtype of the inputs"""
    B, V = poses.shape[0], m['v_template'].shape[0]
    parents = m['parents']
    rot = rodrigues_plain(poses.reshape(-1, 3)).reshape(B, 52, 3, 3)
    c = _coef(betas, dmpls, B)
    v_shaped = m['v_template'][None] + torch.einsum('bl,mkl->bmk', c, torch.cat([m['shapedirs'], m['dmpldirs']], dim=2))
    J = torch.einsum('bik,ji->bjk', v_shaped, m['J_regressor'])
    ident = torch.eye(3, dtype=rot.dtype, device=rot.device)
    pose_feature = (rot[:, 1:] - ident).reshape(B, -1)
    v_posed = torch.matmul(pose_feature, m['posedirs'].reshape(-1, 459).t()).view(B, -1, 3) + v_shaped
    joints = J[..., None]
    rel = joints.clone()
    rel[:, 1:] = rel[:, 1:] - joints[:, list(parents[1:])]
    tm = torch.cat([torch.nn.functional.pad(rot.reshape(-1, 3, 3), [0, 0, 0, 1]),
                    torch.nn.functional.pad(rel.reshape(-1, 3, 1), [0, 0, 0, 1], value=1.0)], dim=2).reshape(B, 52, 4, 4)
    chain = [tm[:, 0]]
    for i in range(1, 52):
        chain.append(torch.matmul(chain[parents[i]], tm[:, i]))
    transforms = torch.stack(chain, dim=1)
    joints_h = torch.nn.functional.pad(joints, [0, 0, 0, 1])
    A = transforms - torch.nn.functional.pad(torch.matmul(transforms, joints_h), [3, 0, 0, 0, 0, 0, 0, 0])
    W = m['weights'][None].expand(B, -1, -1)
    T = torch.matmul(W, A.view(B, 52, 16)).view(B, -1, 4, 4)                                  # the [F,V,4,4] tensor
    v_homo = torch.matmul(T, torch.cat([v_posed, torch.ones(B, V, 1, dtype=rot.dtype, device=rot.device)], dim=2)[..., None])
    verts = v_homo[:, :, :3, 0]
    if trans is not None:
        verts = verts + trans[:, None, :]
    kp = torch.matmul(m['J_regressor_h36m'][None].expand(B, -1, -1), verts)
    return camera_step(kp) if camera else kp


# ------------------------------------------------------------------------------------------------ the equations of include/mbx.h
def folded_eq(m, poses, betas, dmpls=None, trans=None, camera=False, corrupt=None):
    """kp [F,K,3] from the folded model, in the dtype of the inputs"""
    assert corrupt is None or corrupt in CORRUPTIONS
    F, K = poses.shape[0], m['qs'].shape[0]
    parents = list(m['parents'])
    if corrupt == 'wrong_parent':
        parents[38] = 21                        # the second joint of a right-hand finger hangs off the wrist instead of the first (37)
    if corrupt == 'hand_pose_dropped':
        poses = torch.cat([poses[:, :66], torch.zeros_like(poses[:, 66:])], dim=1)
    R = rodrigues_plain(poses.reshape(-1, 3)).reshape(F, 52, 3, 3)
    c = _coef(betas, dmpls, F)
    ident = torch.eye(3, dtype=R.dtype)
    pf = (R[:, 1:] if corrupt == 'pf_with_identity' else R[:, 1:] - ident).reshape(F, 459)
    feat = torch.cat([torch.ones(F, 1, dtype=R.dtype), c, pf], dim=1)                          # [F,484]
    cj = torch.cat([c[:, :16], torch.zeros_like(c[:, 16:])], dim=1) if corrupt == 'dmpl_not_in_Jd' else c
    J = m['Jt'][None] + torch.einsum('jck,fk->fjc', m['Jd'], cj)
    Grot, Gt = [R[:, 0]], [J[:, 0]]
    for k in range(1, 52):
        p = parents[k]
        Grot.append(Grot[p] @ R[:, k])
        Gt.append((Grot[p] @ (J[:, k] - J[:, p])[..., None])[..., 0] + Gt[p])
    Grot, Gt = torch.stack(Grot, 1), torch.stack(Gt, 1)
    At = Gt if corrupt == 'A_without_offset' else Gt - (Grot @ J[..., None])[..., 0]
    pairs, P, s = m['pairs'].long(), m['P'], m['s']
    if corrupt == 'last_pair_dropped':
        pairs, P, s = pairs[:-1], P[:-1], s[:-1]
    y = torch.einsum('pcn,fn->fpc', P, feat)
    j, k = pairs[:, 0], pairs[:, 1]
    contrib = torch.einsum('fpcd,fpd->fpc', Grot[:, k], y) + At[:, k] * s[None, :, None]
    kp = torch.zeros(F, K, 3, dtype=R.dtype).index_add_(1, j, contrib)
    if trans is not None and corrupt != 'trans_dropped':
        kp = kp + m['qs'][None, :, None] * trans[:, None, :]
    return camera_step(kp, corrupt) if camera else kp


# ------------------------------------------------------------------------------------------------ inputs and gates
def inputs(F, seed, max_angle=2.0, per_frame_betas=False, dmpls=True, trans=True, trans_scale=1.0):
    """fp32 inputs: 52 axis-angle vectors per frame with angles uniform in [0, max_angle] (frame 0, where F > 2: the zero pose; frame 1:
    every angle = max_angle), betas ~ N(0,1) ([16], or [F,16]), dmpls ~ N(0,1), trans ~ trans_scale N(0,1) metres"""
    g = torch.Generator().manual_seed(seed)
    axis = torch.randn(F, 52, 3, generator=g, dtype=F64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    angle = max_angle * torch.rand(F, 52, 1, generator=g, dtype=F64)
    if F > 2:
        angle[0] = 0.0
        angle[1] = max_angle
    inp = dict(poses=(axis * angle).reshape(F, 156).float(), betas=torch.randn((F, 16) if per_frame_betas else (16,), generator=g).float())
    d, t = torch.randn(F, 8, generator=g).float(), (trans_scale * torch.randn(F, 3, generator=g)).float()
    inp['dmpls'], inp['trans'] = (d if dmpls else None), (t if trans else None)
    return inp


def _cast(inp, dtype, device=None):
    return {k: (None if v is None else v.to(device=device, dtype=dtype)) for k, v in inp.items()}


def plain(model, inp, dtype, camera=False):
    return plain_lbs_h(model_dict(model, dtype), **_cast(inp, dtype), camera=camera)


def eq(model, inp, dtype, camera=False, corrupt=None, exact_fold=False):
    return folded_eq(model_dict(model, dtype, exact_fold, corrupt), **_cast(inp, dtype), camera=camera, corrupt=corrupt)


def gates(model, inp, camera=False):
    """(ref64, gate): the float64 plain joints and 4 x the stat of the float32 plain path against them (floor 8 ulps)"""
    r64 = plain(model, inp, F64, camera)
    return r64, gate32(stat(plain(model, inp, F32, camera), r64))


# ------------------------------------------------------------------------------------------------ a kernel provider on the CPU
class MockOps:
    """The AMASS entry of the kernel provider on CPU tensors: folded_eq in float32 on the arrays the binding receives, same argument list as
    HipOps.  `corrupt` plants one of CORRUPTIONS (those of the folded model's arrays excepted: the model arrives folded)."""

    def __init__(self, corrupt=None):
        self.calls, self.corrupt = {}, corrupt

    def amass_joints(self, model, poses, betas, dmpls, trans, kp, camera=False, fma=False):
        self.calls['amass_joints'] = self.calls.get('amass_joints', 0) + 1
        assert poses.dtype == F32 and betas.dtype == F32 and kp.dtype == F32 and tuple(kp.shape) == (poses.shape[0], model['qs'].numel(), 3)
        m = {k: model[k].float() for k in ('Jt', 'Jd', 'P', 's', 'qs')}
        m['pairs'], m['parents'] = model['pairs'], tuple(int(p) for p in model['parents'])
        kp.copy_(folded_eq(m, poses, betas, dmpls, trans, camera=bool(camera), corrupt=self.corrupt))


# ------------------------------------------------------------------------------------------------ the plain path as a module
class PlainSMPLH(torch.nn.Module):
    """plain_lbs_h on the device and in the dtype of `poses`: what a user's BodyModel + regressor + camera step compute"""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self._m = {}

    def forward(self, poses, betas, dmpls=None, trans=None, camera=False):
        key = (str(poses.device), poses.dtype)
        if key not in self._m:
            self._m[key] = model_dict(self.model, poses.dtype, device=poses.device)
        return plain_lbs_h(self._m[key], poses, betas, dmpls, trans, camera=camera)


# ------------------------------------------------------------------------------------------------ a tiny AMASS tree
TREE = (  # (path below the root, fps, frames, gender, keep dmpls, pose columns)
    ('ACCAD/s1/walk_poses.npz', 120.0, 50, 'male', True, 156),
    ('ACCAD/s1/run_poses.npz', 90.0, 31, 'female', True, 156),           # round(1.5) = 2: half to even
    ('BMLmovi/s2/a_poses.npz', 150.0, 41, b'male', True, 156),            # round(2.5) = 2; a bytes-typed gender
    ('BMLmovi/s2/b_poses.npz', 100.0, 24, 'neutral', True, 156),          # round(1.67) = 2; neither female nor male
    ('CMU/01/01_01_poses.npz', 60.0, 36, 'female', True, 156),            # 36 = 3 slices of 12: a multiple of the tests' max_len
    ('CMU/01/no_dmpls_poses.npz', 60.0, 20, 'male', False, 156),          # skipped: missing key
    ('CMU/01/slow_poses.npz', 20.0, 20, 'male', True, 156),               # skipped: stride 0
    ('CMU/01/smplx_poses.npz', 60.0, 20, 'male', True, 150),              # skipped: 150 pose columns
)
SKIPPED = ('CMU/01/no_dmpls_poses.npz', 'CMU/01/slow_poses.npz', 'CMU/01/smplx_poses.npz')
STRIDES = {'ACCAD/s1/walk_poses.npz': 2, 'ACCAD/s1/run_poses.npz': 2, 'BMLmovi/s2/a_poses.npz': 2, 'BMLmovi/s2/b_poses.npz': 2,
           'CMU/01/01_01_poses.npz': 1}


def tree_models(V=65):
    """the two body models the tree's tests and tools/mint_amass.py use"""
    return dict(female=AM.SMPLHModel.synthetic(V, 8740), male=AM.SMPLHModel.synthetic(V, 8741))


def write_tree(root, seed=8700):
    """the files of TREE under `root`, as AMASS stores them (float64 arrays; 16 betas; 8 dmpls); returns the paths"""
    import os
    rng = np.random.RandomState(seed)
    paths = []
    for rel, fps, n, gender, keep_dmpls, cols in TREE:
        path = os.path.join(root, *rel.split('/'))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        axis = rng.randn(n, cols // 3, 3)
        poses = (axis / np.linalg.norm(axis, axis=-1, keepdims=True) * rng.uniform(0, 1.5, (n, cols // 3, 1))).reshape(n, cols)
        x = dict(mocap_framerate=np.float64(fps), gender=np.array(gender), betas=rng.randn(16), poses=poses, trans=rng.randn(n, 3),
                 dmpls=rng.randn(n, 8))
        if not keep_dmpls:
            del x['dmpls']
        np.savez(path, **x)
        paths.append(path)
    return paths
