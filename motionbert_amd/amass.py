"""AMASS on the device (csrc/amass.hip): the reference's `tools/compress_amass.py` -> `tools/preprocess_amass.py` -> `tools/convert_amass.py`
without `human_body_prior`, without vertices and without per-clip pickles.

    SMPLHModel                  the arrays of one SMPL-H + DMPL body model as `BodyModel(num_betas=16, num_dmpls=8)` uses them: v_template [V,3],
                                shapedirs [V,3,>=16], dmpldirs [V,3,>=8] (`eigvec` of the DMPL file), posedirs [V,3,459], J_regressor [52,V],
                                weights [V,52], parents [52] and the regressor Q = J_regressor_h36m [K<=32,V].  Only Q . vertices is wanted, so
                                the vertex sum is folded away once, in float64 (`Jt, Jd, pairs, P, s, qs`: include/mbx.h, mbx_amass_joints).
                                `from_npz(smplh_npz, dmpl_npz, j_regressor_h36m)`, `from_arrays(...)`, `synthetic(V, seed)` for tests.
    amass_joints(model, ...)    [F,K,3] fp32 joints of poses [F,156], betas [16] or [F,16], dmpls [F,8], trans [F,3]; `camera=True` applies
                                convert_amass.py's axis swap and 0.298 in the launch.
    read_amass(root)            compress_amass.py: the sequences at 60 fps, and the files the reference's bare `except` drops, by name.
    pack_amass(root, models, out_prefix)     the three scripts end to end into `pack_motion3d`'s format (`PackedMotion3D(prefix, synthetic=True)`).

There is no CPU path: without an injected kernel provider (`ops=`) the work runs on the ROCm device."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import hip_ops
from .data import _split_clips

NUM_JOINTS, NUM_BETAS, NUM_DMPLS, NUM_COEF, POSE_FEATS, FEAT, MAX_K, MAX_PAIRS = 52, 16, 8, 24, 459, 484, 32, 17 * 52
TARGET_FPS = 60
#: the SMPL-H kinematic tree: the 22 body joints of SMPL (without its two hand joints), then 15 joints per hand off the wrists (20, 21)
SMPLH_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19,
                 20, 22, 23, 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35,
                 21, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50)
assert len(SMPLH_PARENTS) == NUM_JOINTS


def _dense64(a):
    if hasattr(a, 'todense'):                      # scipy sparse J_regressor of the original model files
        a = a.todense()
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class SMPLHModel:
    """The arrays of one SMPL-H + DMPL model, validated, as float32 CPU tensors (`parents`: a tuple of ints), and their fold, formed in
    float64 from the stored fp32 bits and stored in float32:
        Jt [52,3] = J_regressor . v_template          Jd [52,3,24] = J_regressor . [shapedirs | dmpldirs]
        pairs [Np,2] (j,k), sorted by j then k: those with Q[j,v] w[v,k] != 0 for some vertex (for a non-negative Q and w: s != 0)
        P [Np,3,484] = sum_v Q[j,v] w[v,k] [T_v | S_v | posedirs_v]       s [Np] = sum_v Q[j,v] w[v,k]       qs [K] = sum_v Q[j,v]"""

    def __init__(self, v_template, shapedirs, dmpldirs, posedirs, J_regressor, parents, weights, J_regressor_h36m):
        vt, sd, dd, pd = _dense64(v_template), _dense64(shapedirs), _dense64(dmpldirs), _dense64(posedirs)
        jr, w, q = _dense64(J_regressor), _dense64(weights), _dense64(J_regressor_h36m)
        if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
            raise ValueError(f'v_template needs to be [V >= 1, 3], got {vt.shape}')
        V = vt.shape[0]
        if sd.ndim != 3 or sd.shape[:2] != (V, 3) or sd.shape[2] < NUM_BETAS:
            raise ValueError(f'shapedirs needs to be [{V}, 3, >= {NUM_BETAS}], got {sd.shape}')
        if dd.ndim != 3 or dd.shape[:2] != (V, 3) or dd.shape[2] < NUM_DMPLS:
            raise ValueError(f'dmpldirs needs to be [{V}, 3, >= {NUM_DMPLS}], got {dd.shape}')
        sd = np.ascontiguousarray(sd[:, :, :NUM_BETAS])                      # BodyModel: shapedirs[:, :, :num_betas], eigvec[:, :, :num_dmpls]
        dd = np.ascontiguousarray(dd[:, :, :NUM_DMPLS])
        if pd.shape != (V, 3, POSE_FEATS):
            raise ValueError(f'posedirs needs to be [{V}, 3, {POSE_FEATS}], got {pd.shape}')
        if jr.shape != (NUM_JOINTS, V):
            raise ValueError(f'J_regressor needs to be [{NUM_JOINTS}, {V}], got {jr.shape}')
        if w.shape != (V, NUM_JOINTS):
            raise ValueError(f'weights needs to be [{V}, {NUM_JOINTS}], got {w.shape}')
        if q.ndim != 2 or q.shape[1] != V or not 1 <= q.shape[0] <= MAX_K:
            raise ValueError(f'J_regressor_h36m needs to be [1 <= K <= {MAX_K}, {V}], got {q.shape}')
        parents = tuple(int(p) for p in np.asarray(parents.detach().cpu() if torch.is_tensor(parents) else parents).reshape(-1))
        if len(parents) != NUM_JOINTS:
            raise ValueError(f'parents needs {NUM_JOINTS} entries, got {len(parents)}')
        parents = (-1,) + parents[1:]                                        # the files store 2^32 - 1 for the root
        for j in range(1, NUM_JOINTS):
            if not 0 <= parents[j] < j:
                raise ValueError(f'parents[{j}] = {parents[j]} is not a forward-ordered tree (0 <= parents[j] < j)')
        for name, a in (('v_template', vt), ('shapedirs', sd), ('dmpldirs', dd), ('posedirs', pd), ('J_regressor', jr), ('weights', w),
                        ('J_regressor_h36m', q)):
            if not np.isfinite(a).all():
                raise ValueError(f'{name} has non-finite entries')
        vt, sd, dd, pd, jr, w, q = (a.astype(np.float32).astype(np.float64) for a in (vt, sd, dd, pd, jr, w, q))   # fold from the fp32 bits
        self.V, self.K, self.parents = V, q.shape[0], parents
        self.v_template, self.shapedirs, self.dmpldirs, self.posedirs = (torch.from_numpy(a).float() for a in (vt, sd, dd, pd))
        self.J_regressor, self.weights, self.J_regressor_h36m = (torch.from_numpy(a).float() for a in (jr, w, q))
        S = np.concatenate([sd, dd], axis=2)                                 # [V,3,24]
        self.Jt = torch.from_numpy(jr @ vt).float()
        self.Jd = torch.from_numpy(np.einsum('jv,vck->jck', jr, S)).float().contiguous()
        D = np.concatenate([vt[:, :, None], S, pd], axis=2).reshape(V, 3 * FEAT)      # [T_v | S_v | posedirs_v]
        live = np.einsum('jv,vk->jk', (q != 0).astype(np.float64), (w != 0).astype(np.float64)) > 0
        pairs = np.argwhere(live)                                            # row-major: sorted by j, then k
        coef = q[pairs[:, 0]] * w[:, pairs[:, 1]].T                          # [Np,V]
        self.pairs = torch.from_numpy(pairs.astype(np.int32)).contiguous()
        self.P = torch.from_numpy((coef @ D).reshape(-1, 3, FEAT)).float().contiguous()
        self.s = torch.from_numpy(coef.sum(1)).float()
        self.qs = torch.from_numpy(q.sum(1)).float()
        self._dev = {}

    @property
    def Np(self):
        return int(self.pairs.shape[0])

    @classmethod
    def from_arrays(cls, v_template, shapedirs, dmpldirs, posedirs, J_regressor, parents, weights, J_regressor_h36m):
        return cls(v_template, shapedirs, dmpldirs, posedirs, J_regressor, parents, weights, J_regressor_h36m)

    @classmethod
    def from_npz(cls, smplh_npz, dmpl_npz, j_regressor_h36m):
        """the files preprocess_amass.py names: `body_models/smplh/<gender>/model.npz` (v_template, shapedirs, posedirs [V,3,459],
        J_regressor, weights, kintree_table), `body_models/dmpls/<gender>/model.npz` (eigvec) and `J_regressor_h36m_correct.npy`"""
        with np.load(smplh_npz, allow_pickle=False) as z:
            keys = set(z.files)
            missing = [k for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights', 'kintree_table') if k not in keys]
            if missing:
                raise ValueError(f'{smplh_npz}: missing arrays {missing} (have {sorted(keys)})')
            body = {k: z[k] for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights')}
            parents = np.asarray(z['kintree_table'])[0].astype(np.int64)
        with np.load(dmpl_npz, allow_pickle=False) as z:
            if 'eigvec' not in z.files:
                raise ValueError(f'{dmpl_npz}: missing array eigvec (have {sorted(z.files)})')
            eigvec = z['eigvec']
        q = np.load(j_regressor_h36m, allow_pickle=False)
        return cls(body['v_template'], body['shapedirs'], eigvec, body['posedirs'], body['J_regressor'], parents, body['weights'], q)

    @classmethod
    def synthetic(cls, V, seed, dense_weights=False, regressor_support=None):
        """a model for tests: the SMPL-H tree, a random template of about body size, shape and DMPL directions of 2 cm and pose directions
        of 1 cm per unit, weight rows with at most 4 non-zeros (dense_weights: all 52) summing to 1, regressor rows non-negative summing
        to 1 with `regressor_support` non-zeros each (default: all V)"""
        g = torch.Generator().manual_seed(int(seed))
        vt = 0.3 * torch.randn(V, 3, generator=g, dtype=torch.float64)
        sd = 0.02 * torch.randn(V, 3, NUM_BETAS, generator=g, dtype=torch.float64)
        dd = 0.02 * torch.randn(V, 3, NUM_DMPLS, generator=g, dtype=torch.float64)
        pd = 0.01 * torch.randn(V, 3, POSE_FEATS, generator=g, dtype=torch.float64)

        def sparse_softmax(rows, cols, keep):
            logits = 2.0 * torch.randn(rows, cols, generator=g, dtype=torch.float64)
            if keep is not None and keep < cols:
                idx = torch.rand(rows, cols, generator=g).argsort(dim=1)[:, :max(1, int(keep))]
                mask = torch.zeros(rows, cols, dtype=torch.bool).scatter_(1, idx, True)
                logits = logits.masked_fill(~mask, -float('inf'))
            return torch.softmax(logits, dim=1)
        w = sparse_softmax(V, NUM_JOINTS, None if dense_weights else 4)
        jr = sparse_softmax(NUM_JOINTS, V, None)
        q = sparse_softmax(17, V, regressor_support)
        return cls(vt, sd, dd, pd, jr, SMPLH_PARENTS, w, q)

    def tensors(self, device=None):
        """the dict the kernel provider takes, on `device` (kept per device: P is the large one)"""
        key = str(device)
        d = self._dev.get(key)
        if d is None:
            d = {k: (getattr(self, k).to(device) if device is not None else getattr(self, k)).contiguous() for k in ('Jt', 'Jd', 'pairs', 'P', 's', 'qs')}
            d['parents'] = self.parents
            self._dev[key] = d
        return d


def amass_joints(model: SMPLHModel, poses, betas, dmpls=None, trans=None, camera: bool = False, ops=None, device=None) -> torch.Tensor:
    """[F,K,3] fp32 (K = 17 for J_regressor_h36m): Q . vertices of the body model for poses [F,156], betas [16] (one per sequence) or
    [F,16], dmpls [F,8] or None (zeros), trans [F,3] or None (zeros); arrays or tensors, rounded to fp32 first as the reference's
    `torch.Tensor(...)` does.  camera: convert_amass.py's (x, y, z) -> (x, -z, y), then x float32(0.298).  The result stays on the device
    (`device`: default the tensors' own, or the current ROCm device for host input; with an injected `ops`, where ops computes)."""
    if not isinstance(model, SMPLHModel):
        raise TypeError('amass_joints needs an SMPLHModel (SMPLHModel.from_npz / from_arrays / synthetic)')

    def f32(a):
        if a is None:
            return None
        t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        return t.to(torch.float32)
    poses, betas, dmpls, trans = f32(poses), f32(betas), f32(dmpls), f32(trans)
    if poses.dim() != 2 or poses.shape[1] != 3 * NUM_JOINTS:
        raise ValueError(f'poses [F,{3 * NUM_JOINTS}] expected, got {tuple(poses.shape)}')
    F = poses.shape[0]
    if betas.dim() == 1 and betas.shape[0] >= NUM_BETAS:
        betas = betas[:NUM_BETAS]                                          # preprocess_amass.py:54
    if tuple(betas.shape) not in ((NUM_BETAS,), (F, NUM_BETAS)):
        raise ValueError(f'betas [{NUM_BETAS}] or [{F},{NUM_BETAS}] expected, got {tuple(betas.shape)}')
    if dmpls is not None:
        if dmpls.dim() != 2 or dmpls.shape[0] != F or dmpls.shape[1] < NUM_DMPLS:
            raise ValueError(f'dmpls [{F}, >= {NUM_DMPLS}] expected, got {tuple(dmpls.shape)}')
        dmpls = dmpls[:, :NUM_DMPLS]                                       # preprocess_amass.py:55
    if trans is not None and tuple(trans.shape) != (F, 3):
        raise ValueError(f'trans [{F},3] expected, got {tuple(trans.shape)}')
    if ops is None:
        if device is None:
            device = poses.device if poses.is_cuda else (torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None)
        if device is None:
            raise RuntimeError('motionbert_amd.amass.amass_joints runs on the ROCm device; there is no CPU path')
        ops = hip_ops.get()
    elif device is None:
        device = poses.device
    poses, betas, dmpls, trans = (None if t is None else t.to(device).contiguous() for t in (poses, betas, dmpls, trans))
    kp = torch.empty(F, model.K, 3, dtype=torch.float32, device=device)
    if F:
        ops.amass_joints(model.tensors(device), poses, betas, dmpls, trans, kp, camera=bool(camera))
    return kp


# ---------------------------------------------------------------------------------------------------------------
# compress_amass.py
# ---------------------------------------------------------------------------------------------------------------
def _walk(root):
    files = []
    for d, _dirs, names in os.walk(root):
        files += [os.path.join(d, n) for n in names]
    return sorted(files)


def read_amass(root: str):
    """compress_amass.py: every file under `root` in sorted path order, taken at 60 fps: `stride = round(mocap_framerate / 60)` (python's
    round: half to even, so 90 and 150 fps give 2), `trans / dmpls / poses` `[::stride]`.  Returns `(sequences, skipped)`: sequences = dicts
    `name` (the path below root, joined with '_'), `fps`, `len_ori`, `gender`, `betas`, `poses [n,156]`, `dmpls`, `trans`; skipped =
    `(path, reason)` of every file the reference's bare `except` drops without a word: not a readable .npz, a missing key, a stride of 0
    (below 30 fps), pose rows that are not 156 wide (preprocess_amass.py would stop there), arrays of unequal length."""
    seqs, skipped = [], []
    root = os.path.normpath(root)
    for path in _walk(root):
        try:
            with np.load(path, allow_pickle=False) as z:
                x = {k: z[k] for k in z.files}
        except Exception as e:                                            # noqa: BLE001 (a readme, a licence file, a broken archive)
            skipped.append((path, f'not a readable npz: {type(e).__name__}'))
            continue
        missing = [k for k in ('mocap_framerate', 'trans', 'dmpls', 'poses', 'gender', 'betas') if k not in x]
        if missing:
            skipped.append((path, f'missing {missing}'))
            continue
        fps = float(np.asarray(x['mocap_framerate']).reshape(-1)[0])
        stride = round(fps / TARGET_FPS) if np.isfinite(fps) else 0
        if stride < 1:
            skipped.append((path, f'stride round({fps:g} / {TARGET_FPS}) = {stride}'))
            continue
        poses, dmpls, trans = (np.asarray(x[k]) for k in ('poses', 'dmpls', 'trans'))
        if poses.ndim != 2 or poses.shape[1] != 3 * NUM_JOINTS:
            skipped.append((path, f'poses {poses.shape}, [n,{3 * NUM_JOINTS}] expected'))
            continue
        if dmpls.ndim != 2 or dmpls.shape[1] < NUM_DMPLS or trans.shape != (poses.shape[0], 3) or dmpls.shape[0] != poses.shape[0]:
            skipped.append((path, f'trans {trans.shape} / dmpls {dmpls.shape} do not match poses {poses.shape}'))
            continue
        seqs.append(dict(name='_'.join(os.path.relpath(path, root).split(os.sep)), path=path, fps=fps, len_ori=int(trans.shape[0]),
                         gender=x['gender'], betas=np.asarray(x['betas']), poses=poses[::stride], dmpls=dmpls[::stride], trans=trans[::stride]))
    return seqs, skipped


def pick_gender(gender, rule: str = 'reference') -> str:
    """preprocess_amass.py:30-32.  'reference': `str(gender)` must be 'female' or 'male', else female -- so the bytes-typed gender of some
    AMASS files (str -> "b'male'") is female, as in the reference; 'decode': bytes are decoded first."""
    if rule not in ('reference', 'decode'):
        raise ValueError(f"gender_rule 'reference' or 'decode' expected, got {rule!r}")
    g = gender.item() if isinstance(gender, np.ndarray) and gender.ndim == 0 else gender
    if rule == 'decode' and isinstance(g, (bytes, np.bytes_)):
        g = g.decode()
    g = str(g)
    return g if g in ('female', 'male') else 'female'


def slice_table(n: int, max_len: int):
    """preprocess_amass.py:44-48: `n // max_len + 1` slices [start, end); the last one is empty when n is a multiple of max_len"""
    return [(i * max_len, min((i + 1) * max_len, n)) for i in range(n // max_len + 1)]


def pack_amass(root: str, models: dict, out_prefix: str, n_frames: int = 243, data_stride: int = 81, max_len: int = 2916, scale: float = 0.298,
               seed: int = 0, gender_rule: str = 'reference', ops=None, device=None, chunk: int = 256) -> dict:
    """The reference's three AMASS scripts end to end: `read_amass(root)`; per sequence the body model `models['female' / 'male']` by
    `pick_gender`, its joints from one `amass_joints(camera=True)` launch (they stay on the device); the slices of `max_len` frames of a
    sequence are the "videos" of `split_clips` (convert_amass.py:20-36), windows of `n_frames` every `data_stride`, a shorter video resampled
    with `np.random.RandomState(seed)` (the reference: the global numpy state).  A sequence whose length is a multiple of `max_len` has an
    empty last slice: the reference stores a [17,0,3] array for it, which contributes no frame and no clip; it is dropped here.  The clips
    are gathered on the device `chunk` at a time and written straight into `<out_prefix>.label.npy` [N,n_frames,K,3] / `.json` in
    pack_motion3d's format with `has_input: false`: it opens with `PackedMotion3D(out_prefix, synthetic=True)`.  Returns the metadata, with
    the skipped files.  `scale`: the camera step's factor; the launch carries convert_amass.py's 0.298, another value is applied to the
    unflagged joints with the same two fp32 operations in torch."""
    in_launch = np.float32(scale) == np.float32(0.298)
    for g in ('female', 'male'):
        if not isinstance(models.get(g), SMPLHModel):
            raise ValueError(f"models needs an SMPLHModel for '{g}'")
    if models['female'].K != models['male'].K:
        raise ValueError('the two body models regress different numbers of joints')
    K = models['female'].K
    seqs, skipped = read_amass(root)
    joints, vid_list, videos = [], [], []
    for sq in seqs:
        model = models[pick_gender(sq['gender'], gender_rule)]
        kp = amass_joints(model, sq['poses'], np.asarray(sq['betas'])[:NUM_BETAS], sq['dmpls'], sq['trans'], camera=in_launch, ops=ops,
                          device=device)
        if not in_launch:
            kp = torch.stack([kp[..., 0], -kp[..., 2], kp[..., 1]], dim=-1) * float(np.float32(scale))
        joints.append(kp)
        for a, b in slice_table(kp.shape[0], max_len):
            if b > a:
                vid_list += [len(videos)] * (b - a)
                videos.append(dict(name=sq['name'], start=a, len=b - a))
    if not vid_list:
        raise ValueError(f'no AMASS frames under {root} ({len(skipped)} files skipped)')
    joints = torch.cat(joints, dim=0)                                      # [frames,K,3], on the device
    split_id = _split_clips(vid_list, n_frames, data_stride, np.random.RandomState(seed))
    n = len(split_id)
    if n == 0:
        raise ValueError(f'{len(vid_list)} frames give no clip of {n_frames} frames')
    idx = torch.from_numpy(np.stack(split_id).astype(np.int64))
    lab = np.lib.format.open_memmap(out_prefix + '.label.npy', mode='w+', dtype=np.float32, shape=(n, n_frames, K, 3))
    for i in range(0, n, chunk):
        rows = idx[i:i + chunk].to(joints.device)
        lab[i:i + chunk] = joints[rows.reshape(-1)].reshape(rows.shape[0], n_frames, K, 3).cpu().numpy()
    lab.flush()
    del lab
    meta = dict(n=n, clip_shape=[n_frames, K, 3], has_input=False, split='train', subsets=['AMASS'], source='amass', n_frames=n_frames,
                data_stride=data_stride, max_len=max_len, scale=float(np.float32(scale)), seed=seed, gender_rule=gender_rule, frames=len(vid_list),
                videos=videos, skipped=[[os.path.relpath(p, root), why] for p, why in skipped])
    with open(out_prefix + '.json', 'w') as f:
        json.dump(meta, f)
    return meta
