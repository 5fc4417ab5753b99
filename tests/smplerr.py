"""Restatements, inputs, gates and a CPU provider for the SMPL kernels (csrc/smpl.hip, motionbert_amd/smpl.py).  Plain module, no fixtures:
tests/test_gpu_smpl.py applies it to the kernels on the GPU, tests/test_smplerr.py to analytic identities and seeded corruptions on the CPU.

No SMPL implementation exists next to this project (the reference only imports `smplx`), so the definition is pinned twice, independently:

  forward_eq / backward_eq   the equations of include/mbx.h term by term (folded Jt / Jd, the 3x4 transforms A_j, the hand-written backward with
                             its chain walk from joint 23 down to 0), in the dtype of their inputs: float64 is the restatement, float32 the
                             model of the kernels that `MockOps` runs.  `corrupt=` plants one of CORRUPTIONS.
  plain_lbs                  linear blend skinning the way `smplx.lbs.lbs` writes it: J_regressor applied to the shaped vertices, 4x4
                             homogeneous transforms chained by batched matmuls, the [F,V,4,4] per-vertex transform tensor, homogeneous
                             vertices; gradient by autograd.  It is the user's alternative, and the yardstick of the gates.

Gate (the standing rule of tests/mesherr.py): per fp32 output array  stat = max |error| / max |float64 value|  may be at most 4 x the stat of
plain_lbs in float32 against plain_lbs in float64 on the same inputs, computed on the CPU when the test runs; never less than 8 fp32 ulps.
Nothing is read off the kernels."""
import math

import numpy as np
import torch

from tests import mesherr as ME

F32, F64 = torch.float32, torch.float64
FLOOR = ME.FLOOR
stat = ME.stat
gate32 = ME.gate32

CORRUPTIONS = ('wrong_parent', 'pf_with_identity', 'A_without_offset', 'weights_transposed', 'kp_without_scale', 'dbeta_without_Jd',
               'dpf_not_added', 'last_tile_dropped')
TILE = 64          # the kernels' vertex tile ('last_tile_dropped')


# ------------------------------------------------------------------------------------------------ the equations of include/mbx.h
def model_dict(model, dtype=F64, exact_fold=False, device=None):
    """the arrays of an SMPLModel in `dtype` (the fp32 bits, widened); Jt / Jd are the model's folded fp32 arrays (what the kernels read),
    or with exact_fold the products J_regressor . v_template / shapedirs formed in `dtype` (what the plain path computes per call)"""
    d = {k: getattr(model, k).to(device=device, dtype=dtype) for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'lbs_weights', 'Jt', 'Jd')}
    if exact_fold:
        d['Jt'] = d['J_regressor'] @ d['v_template']
        d['Jd'] = torch.einsum('jv,vck->jck', d['J_regressor'], d['shapedirs'])
    d['parents'] = tuple(model.parents)
    return d


def _parents(m, corrupt):
    p = list(m['parents'])
    if corrupt == 'wrong_parent':
        p[10] = 1                      # the left foot hangs off the left hip instead of the left ankle (7)
    return p


def _chain(m, betas, rot, corrupt=None):
    """J [F,24,3], Grot [F,24,3,3], Gt [F,24,3], A [F,24,3,4]"""
    parents = _parents(m, corrupt)
    J = m['Jt'][None] + torch.einsum('jck,fk->fjc', m['Jd'], betas)
    Grot, Gt = [rot[:, 0]], [J[:, 0]]
    for j in range(1, 24):
        p = parents[j]
        Grot.append(Grot[p] @ rot[:, j])
        Gt.append((Grot[p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p])
    Grot, Gt = torch.stack(Grot, 1), torch.stack(Gt, 1)
    At = Gt if corrupt == 'A_without_offset' else Gt - (Grot @ J[..., None])[..., 0]
    return J, Grot, Gt, torch.cat([Grot, At[..., None]], dim=-1)


def _weights(m, corrupt):
    w = m['lbs_weights']
    return w.reshape(-1).reshape(24, -1).t() if corrupt == 'weights_transposed' else w        # the flat array read as [j,v]


def _live(V, corrupt, like):
    keep = torch.ones(V, dtype=like.dtype)
    if corrupt == 'last_tile_dropped' and V % TILE:
        keep[V - V % TILE:] = 0
    return keep


def _vposed(m, betas, rot, corrupt):
    F, V = betas.shape[0], m['v_template'].shape[0]
    ident = torch.eye(3, dtype=rot.dtype)
    pf = (rot[:, 1:] if corrupt == 'pf_with_identity' else rot[:, 1:] - ident).reshape(F, 207)
    return m['v_template'][None] + torch.einsum('vck,fk->fvc', m['shapedirs'], betas) + (pf @ m['posedirs']).reshape(F, V, 3)


def forward_eq(m, betas, rot, Q=None, scale=1.0, corrupt=None):
    """(verts [F,V,3], kp [F,K,3] or None, joints [F,24,3]) in the dtype of betas / rot / m"""
    assert corrupt is None or corrupt in CORRUPTIONS
    V = m['v_template'].shape[0]
    J, Grot, Gt, A = _chain(m, betas, rot, corrupt)
    vp = _vposed(m, betas, rot, corrupt)
    T = torch.einsum('vj,fjce->fvce', _weights(m, corrupt), A)
    x = (torch.einsum('fvcd,fvd->fvc', T[..., :3], vp) + T[..., 3]) * _live(V, corrupt, vp)[None, :, None]
    kp = None if Q is None else (1.0 if corrupt == 'kp_without_scale' else scale) * torch.einsum('kv,fvc->fkc', Q, x)
    return scale * x, kp, scale * Gt


def backward_eq(m, betas, rot, Q, scale, dverts=None, dkp=None, djoints=None, corrupt=None):
    """(drot [F,24,3,3], dbetas [F,10]): the hand-written backward of include/mbx.h"""
    assert corrupt is None or corrupt in CORRUPTIONS
    F, V = betas.shape[0], m['v_template'].shape[0]
    parents = _parents(m, corrupt)
    J, Grot, Gt, A = _chain(m, betas, rot, corrupt)
    vp = _vposed(m, betas, rot, corrupt)
    w = _weights(m, corrupt)
    T = torch.einsum('vj,fjce->fvce', w, A)
    g = torch.zeros(F, V, 3, dtype=betas.dtype)
    if dverts is not None:
        g = g + dverts
    if dkp is not None:
        g = g + torch.einsum('kv,fkc->fvc', Q, dkp)
    g = scale * g * _live(V, corrupt, g)[None, :, None]
    dT = torch.cat([g[..., :, None] * vp[..., None, :], g[..., None]], dim=-1)               # [F,V,3,4]
    dA = torch.einsum('vj,fvce->fjce', w, dT)
    dvp = torch.einsum('fvcd,fvc->fvd', T[..., :3], g)
    dbeta = torch.einsum('vck,fvc->fk', m['shapedirs'], dvp)
    dpf = dvp.reshape(F, 3 * V) @ m['posedirs'].t()                                           # [F,207]
    # A_j = [Grot_j | Gt_j - Grot_j J_j]
    dAt = dA[..., 3]
    dGrot = [dA[:, j, :, :3] - (0 if corrupt == 'A_without_offset' else dAt[:, j, :, None] * J[:, j, None, :]) for j in range(24)]
    dGt = [dAt[:, j] + (scale * djoints[:, j] if djoints is not None else 0) for j in range(24)]
    dJ = [torch.zeros(F, 3, dtype=betas.dtype) if corrupt == 'A_without_offset' else -(Grot[:, j].transpose(1, 2) @ dAt[:, j, :, None])[..., 0]
          for j in range(24)]
    dR = [None] * 24
    for j in range(23, 0, -1):
        p = parents[j]
        rel = J[:, j] - J[:, p]
        dGrot[p] = dGrot[p] + dGrot[j] @ rot[:, j].transpose(1, 2) + dGt[j][:, :, None] * rel[:, None, :]
        dR[j] = Grot[:, p].transpose(1, 2) @ dGrot[j]
        drel = (Grot[:, p].transpose(1, 2) @ dGt[j][..., None])[..., 0]
        dGt[p] = dGt[p] + dGt[j]
        dJ[j] = dJ[j] + drel
        dJ[p] = dJ[p] - drel
    dR[0] = dGrot[0]
    dJ[0] = dJ[0] + dGt[0]
    if corrupt != 'dbeta_without_Jd':
        dbeta = dbeta + torch.einsum('jck,fjc->fk', m['Jd'], torch.stack(dJ, 1))
    dR = torch.stack(dR, 1)
    if corrupt != 'dpf_not_added':
        dR = torch.cat([dR[:, :1], dR[:, 1:] + dpf.reshape(F, 23, 3, 3)], dim=1)
    return dR, dbeta


# ------------------------------------------------------------------------------------------------ the way smplx writes it
def plain_lbs(m, betas, rot):
    """(vertices [F,V,3], posed joints [F,24,3]) of `smplx.lbs.lbs(betas, rot, ..., pose2rot=False)`, in the dtype of its inputs"""
    B, V = betas.shape[0], m['v_template'].shape[0]
    parents = m['parents']
    v_shaped = m['v_template'][None] + torch.einsum('bl,mkl->bmk', betas, m['shapedirs'])
    J = torch.einsum('bik,ji->bjk', v_shaped, m['J_regressor'])
    ident = torch.eye(3, dtype=rot.dtype, device=rot.device)
    pose_feature = (rot[:, 1:] - ident).reshape(B, -1)
    v_posed = torch.matmul(pose_feature, m['posedirs']).view(B, -1, 3) + v_shaped
    # batch_rigid_transform
    joints = J[..., None]
    rel = joints.clone()
    rel[:, 1:] = rel[:, 1:] - joints[:, list(parents[1:])]
    tm = torch.cat([torch.nn.functional.pad(rot.reshape(-1, 3, 3), [0, 0, 0, 1]),
                    torch.nn.functional.pad(rel.reshape(-1, 3, 1), [0, 0, 0, 1], value=1.0)], dim=2).reshape(B, 24, 4, 4)
    chain = [tm[:, 0]]
    for i in range(1, 24):
        chain.append(torch.matmul(chain[parents[i]], tm[:, i]))
    transforms = torch.stack(chain, dim=1)
    posed_joints = transforms[:, :, :3, 3]
    joints_h = torch.nn.functional.pad(joints, [0, 0, 0, 1])
    A = transforms - torch.nn.functional.pad(torch.matmul(transforms, joints_h), [3, 0, 0, 0, 0, 0, 0, 0])
    W = m['lbs_weights'][None].expand(B, -1, -1)
    T = torch.matmul(W, A.view(B, 24, 16)).view(B, -1, 4, 4)                                  # the [F,V,4,4] tensor
    v_homo = torch.matmul(T, torch.cat([v_posed, torch.ones(B, V, 1, dtype=rot.dtype, device=rot.device)], dim=2)[..., None])
    return v_homo[:, :, :3, 0], posed_joints


def plain_outputs(m, betas, rot, Q, scale):
    """verts, kp (None without Q), joints as the head forms them around the plain layer: `vertices * scale`, `matmul(Q, verts)`"""
    v, j = plain_lbs(m, betas, rot)
    verts = v * scale
    kp = None if Q is None else torch.matmul(Q[None].expand(betas.shape[0], -1, -1), verts)
    return verts, kp, j * scale


def plain_all(model, inp, dtype, scale=1.0, use=('dverts', 'dkp', 'djoints')):
    """every output and gradient of the plain path in `dtype` from the fp32 bits of the inputs: dict verts, kp, joints, drot, dbetas;
    the cotangents named in `use` (and present in inp) are applied"""
    m = model_dict(model, dtype)
    b = inp['betas'].detach().clone().to(dtype).requires_grad_(True)
    r = inp['rot'].detach().clone().to(dtype).requires_grad_(True)
    Q = None if inp.get('Q') is None else inp['Q'].to(dtype)
    verts, kp, joints = plain_outputs(m, b, r, Q, scale)
    loss = 0
    for name, out in (('dverts', verts), ('dkp', kp), ('djoints', joints)):
        if name in use and inp.get(name) is not None and out is not None:
            loss = loss + (out * inp[name].to(dtype)).sum()
    out = dict(verts=verts.detach(), kp=None if kp is None else kp.detach(), joints=joints.detach())
    if torch.is_tensor(loss):
        loss.backward()
        out['drot'], out['dbetas'] = r.grad, b.grad
    return out


def eq_all(model, inp, dtype, scale=1.0, use=('dverts', 'dkp', 'djoints'), corrupt=None, exact_fold=False):
    """the same dict from forward_eq / backward_eq"""
    m = model_dict(model, dtype, exact_fold)
    b, r = inp['betas'].to(dtype), inp['rot'].to(dtype)
    Q = None if inp.get('Q') is None else inp['Q'].to(dtype)
    verts, kp, joints = forward_eq(m, b, r, Q, scale, corrupt)
    cot = {n: (inp[n].to(dtype) if n in use and inp.get(n) is not None else None) for n in ('dverts', 'dkp', 'djoints')}
    if Q is None:
        cot['dkp'] = None
    out = dict(verts=verts, kp=kp, joints=joints)
    if any(v is not None for v in cot.values()):
        out['drot'], out['dbetas'] = backward_eq(m, b, r, Q, scale, cot['dverts'], cot['dkp'], cot['djoints'], corrupt)
    return out


def gates(model, inp, scale=1.0, use=('dverts', 'dkp', 'djoints')):
    """(ref64, gate): the float64 plain outputs and, per array, 4 x the stat of the float32 plain path against them (floor 8 ulps)"""
    r64, r32 = plain_all(model, inp, F64, scale, use), plain_all(model, inp, F32, scale, use)
    return r64, {k: gate32(stat(r32[k], r64[k])) for k in r64 if r64[k] is not None}


# ------------------------------------------------------------------------------------------------ inputs
def rotations(n, seed, max_angle=2.0):
    """[n,3,3] float64 rotation matrices from axis-angle vectors with angles uniform in [0, max_angle]"""
    g = torch.Generator().manual_seed(seed)
    axis = torch.randn(n, 3, generator=g, dtype=F64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    return ME.axis_angle_matrix64(axis, max_angle * torch.rand(n, generator=g, dtype=F64))


def inputs(F, V, K, seed, model=None):
    """fp32 inputs and cotangents: betas ~ N(0,1), rotations of up to 2 rad, Q (K > 0: the first K rows of a softmax regressor, or the
    model's J_regressor_h36m for K = 17) and random dverts / dkp / djoints"""
    g = torch.Generator().manual_seed(seed)
    inp = dict(betas=torch.randn(F, 10, generator=g).float(), rot=rotations(F * 24, seed + 1).reshape(F, 24, 3, 3).float().contiguous())
    inp['Q'] = None
    if K:
        if model is not None and K == 17 and model.J_regressor_h36m is not None:
            inp['Q'] = model.J_regressor_h36m.clone()
        else:
            inp['Q'] = torch.softmax(2.0 * torch.randn(K, V, generator=g), dim=1).float().contiguous()
    inp['dverts'] = torch.randn(F, V, 3, generator=g).float()
    inp['dkp'] = torch.randn(F, K, 3, generator=g).float() if K else None
    inp['djoints'] = torch.randn(F, 24, 3, generator=g).float()
    return inp


# ------------------------------------------------------------------------------------------------ a kernel provider on the CPU
class MockOps(ME.TorchOps):
    """The SMPL entries of the kernel provider on CPU tensors: the fp32 model of the kernels (forward_eq / backward_eq in float32 on the
    arrays the binding receives), same argument lists as HipOps.  `corrupt` plants one of CORRUPTIONS."""

    def __init__(self, corrupt=None):
        super().__init__()
        self.corrupt = corrupt

    @staticmethod
    def _m(model):
        d = {k: model[k].float() for k in ('v_template', 'shapedirs', 'posedirs', 'Jt', 'Jd', 'lbs_weights')}
        d['parents'] = tuple(int(p) for p in model['parents'])
        return d

    def smpl_fwd_ws(self, F, V, K, device):
        return torch.empty(16, dtype=torch.uint8)

    smpl_bwd_ws = smpl_fwd_ws

    def smpl_pack(self, shapedirs, posedirs, packed_t):
        self._count('smpl_pack')
        V = shapedirs.shape[0]
        packed_t.zero_()
        packed_t[:, :207] = posedirs.t()
        packed_t[:, 207:217] = shapedirs.reshape(3 * V, 10)

    def smpl_fwd(self, model, Q, betas, rotmat, scale, verts, kp, joints, ws=None):
        self._count('smpl_fwd')
        F = betas.shape[0]
        v, k, j = forward_eq(self._m(model), betas.float(), rotmat.reshape(F, 24, 3, 3).float(), Q, float(np.float32(scale)), self.corrupt)
        if verts is not None:
            verts.copy_(v)
        if kp is not None:
            kp.copy_(k)
        if joints is not None:
            joints.copy_(j)

    def smpl_bwd(self, model, Q, betas, rotmat, scale, dverts, dkp, djoints, drotmat, dbetas, ws=None):
        self._count('smpl_bwd')
        F = betas.shape[0]
        assert model.get('packed_t') is not None and tuple(model['packed_t'].shape) == (3 * model['v_template'].shape[0], 224)
        dr, db = backward_eq(self._m(model), betas.float(), rotmat.reshape(F, 24, 3, 3).float(), Q, float(np.float32(scale)), dverts, dkp, djoints,
                             self.corrupt)
        drotmat.copy_(dr.reshape(drotmat.shape))
        dbetas.copy_(db)


def mock_all(model, inp, scale=1.0, use=('dverts', 'dkp', 'djoints'), corrupt=None):
    """the dict of eq_all, produced by driving MockOps through the provider's argument lists"""
    ops = MockOps(corrupt)
    F, V = inp['betas'].shape[0], model.V
    md = model.tensors()
    md['packed_t'] = torch.empty(3 * V, 224)
    ops.smpl_pack(md['shapedirs'], md['posedirs'], md['packed_t'])
    Q = inp.get('Q')
    K = 0 if Q is None else Q.shape[0]
    out = dict(verts=torch.full((F, V, 3), math.nan), kp=None if Q is None else torch.full((F, K, 3), math.nan), joints=torch.full((F, 24, 3), math.nan))
    rot = inp['rot'].reshape(F, 24, 9)
    ops.smpl_fwd(md, Q, inp['betas'], rot, scale, out['verts'], out['kp'], out['joints'])
    cot = {n: (inp[n] if n in use and inp.get(n) is not None else None) for n in ('dverts', 'dkp', 'djoints')}
    if Q is None:
        cot['dkp'] = None
    if any(v is not None for v in cot.values()):
        out['drot'], out['dbetas'] = torch.full((F, 24, 9), math.nan), torch.full((F, 10), math.nan)
        ops.smpl_bwd(md, Q, inp['betas'], rot, scale, cot['dverts'], cot['dkp'], cot['djoints'], out['drot'], out['dbetas'])
        out['drot'] = out['drot'].reshape(F, 24, 3, 3)
    return out


def worst_ratio(got, ref64, gate, report=None):
    """max over the arrays of stat / gate; every ratio goes into `report` (a dict) where given"""
    worst = 0.0
    for k, g in gate.items():
        if got.get(k) is None:
            continue
        r = stat(got[k].reshape(ref64[k].shape), ref64[k]) / g
        if report is not None:
            report[k] = r
        worst = max(worst, r)
    return worst


# ------------------------------------------------------------------------------------------------ the plain layer as a module
def rodrigues_plain(aa):
    """smplx's batch_rodrigues of [M,3] in the dtype of aa: angle = |r + 1e-8|, R = I + sin K + (1 - cos) K K"""
    angle = (aa + 1e-8).norm(dim=1, keepdim=True)
    d = aa / angle
    K = torch.zeros(aa.shape[0], 3, 3, dtype=aa.dtype, device=aa.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    return torch.eye(3, dtype=aa.dtype, device=aa.device) + torch.sin(angle)[:, :, None] * K + (1 - torch.cos(angle))[:, :, None] * (K @ K)


class PlainSMPL(torch.nn.Module):
    """plain_lbs behind the reference's call signature, in the dtype of `betas`: what a user's smplx layer computes"""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.J_regressor_h36m = model.J_regressor_h36m

    def forward(self, betas, body_pose, global_orient, pose2rot=False):
        import types
        F = betas.shape[0]
        if pose2rot:
            rot = rodrigues_plain(torch.cat([global_orient.reshape(F, 1, 3), body_pose.reshape(F, 23, 3)], 1).reshape(-1, 3)).reshape(F, 24, 3, 3)
        else:
            rot = torch.cat([global_orient.reshape(F, 1, 3, 3), body_pose.reshape(F, 23, 3, 3)], dim=1)
        v, j = plain_lbs(model_dict(self.model, betas.dtype, device=betas.device), betas, rot.to(betas.dtype))
        return types.SimpleNamespace(vertices=v, joints=j)
