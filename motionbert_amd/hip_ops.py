"""ctypes binding of libmbx.so: the kernel provider (`ops`) used by motionbert_amd.engine.

Thin by design: every method checks nothing but dtypes/contiguity, takes raw device pointers from
the torch tensors (PyTorch owns all memory), passes the current HIP stream and raises
RuntimeError(mbx_last_error()) on a non-zero return.  There is no CPU implementation and no
fallback: if libmbx.so cannot be loaded the import of this module's `get()` fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from itertools import accumulate
from typing import Dict, List, Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MBX_LIB', os.path.join(_HERE, 'libmbx.so'))   # MBX_LIB: A/B builds of the kernel library

MBX_F32, MBX_BF16, MBX_BF16_LO = 0, 1, 2
_DT = {torch.float32: MBX_F32, torch.bfloat16: MBX_BF16}

_vp, _i, _f, _sz, _i64p = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_void_p

# name -> (restype, argtypes); mirrors include/mbx.h one to one
SIGNATURES = {
    'mbx_last_error': (C.c_char_p, []),
    'mbx_version': (_i, []),
    'mbx_prep_weights': (_i, [_i64p, _i, _i, _i, _i, _vp]),
    'mbx_embed_fwd': (_i, [_vp] * 6 + [_i] * 5 + [_vp]),
    'mbx_embed_ln_fwd': (_i, [_vp] * 5 + [_f] + [_vp] * 4 + [_i] * 5 + [_vp]),
    'mbx_embed_bwd_ws': (_sz, [_i] * 4),
    'mbx_embed_bwd': (_i, [_vp] * 8 + [_i] * 5 + [_vp, _vp]),
    'mbx_embed_bwd_pair': (_i, [_vp] * 9 + [_i] * 5 + [_vp, _vp]),
    'mbx_layernorm_fwd': (_i, [_vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'mbx_layernorm_bwd_ws': (_sz, [_i]),
    'mbx_layernorm_bwd': (_i, [_vp] * 11 + [_i, _i, _i, _vp, _vp]),
    'mbx_gemm_nt': (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'mbx_gemm_tn_ws': (_sz, [_i, _i, _i]),
    'mbx_gemm_tn': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'mbx_fold_norm_weights': (_i, [_i64p, _i, _i, _i, _vp]),
    'mbx_gemm_nt_dgelu_stats': (_i, [_vp] * 7 + [_i, _i, _i, _vp]),
    'mbx_gemm_nt_gelu_d': (_i, [_vp] * 5 + [_i, _i, _i, _vp]),
    'mbx_gemm_nt_mul': (_i, [_vp] * 4 + [_i, _i, _i, _vp]),
    'mbx_lnbwd_rowc': (_i, [_vp, _i, _vp, _vp, _i, _i, _vp]),
    'mbx_gemm_nt_lnbwd': (_i, [_vp] * 8 + [_i, _i, _i, _vp]),
    'mbx_gemm_nt_lnbwd_t': (_i, [_vp] * 8 + [_i, _i, _i, _vp]),
    'mbx_unfold_norm_grads_ws': (_sz, [_i, _i]),
    'mbx_unfold_norm_grads': (_i, [_vp] * 7 + [_i, _i, _vp, _vp]),
    'mbx_mlp_pack_bytes': (_sz, [_i, _i]),
    'mbx_mlp_pack_weights': (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    'mbx_proj_mlp_pack_bytes': (_sz, [_i, _i]),
    'mbx_proj_mlp_pack_weights': (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    'mbx_proj_mlp_fused_fwd': (_i, [_vp] * 8 + [_f, _i, _i, _i, _vp]),
    'mbx_mlp_fused_fwd': (_i, [_vp, _i] + [_vp] * 7 + [_f, _vp, _vp, _i, _i, _i, _vp]),
    'mbx_rows_pack_bytes': (_sz, [_i, _i]),
    'mbx_rows_pack_nk': (_i, [_vp, _vp, _i, _i, _vp]),
    'mbx_rows_gemm_nk': (_i, [_vp] * 7 + [_i, _i, _i, _vp]),
    'mbx_rows_gemm_nk_ln': (_i, [_vp] * 4 + [_f, _vp, _i, _i, _i, _vp]),
    'mbx_gelu_fwd': (_i, [_vp, _vp, _sz, _i, _vp]),
    'mbx_split_bf16': (_i, [_vp, _vp, _vp, _sz, _vp]),
    'mbx_gemm_nt_x3p': (_i, [_vp] * 5 + [_i] + [_vp] * 4 + [_i, _i, _i, _vp]),
    'mbx_layernorm_bwd_planes': (_i, [_vp] * 12 + [_i, _i, _vp, _vp]),
    'mbx_layernorm_fwd_planes': (_i, [_vp] * 3 + [_f] + [_vp] * 4 + [_i, _i, _vp]),
    'mbx_gemm_nt_x3': (_i, [_vp] * 5 + [_i] + [_vp] * 5 + [_i, _i, _i, _vp]),
    'mbx_gemm_tn_x3_workspace': (_sz, [_i, _i, _i]),
    'mbx_gemm_tn_x3': (_i, [_vp] * 6 + [_i, _i, _i, _vp, _vp]),
    'mbx_attn_fwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _i, _vp]),
    'mbx_attn_bwd_planes': (_i, [_vp] * 6 + [_i, _i, _i, _i, _i, _f, _i, _f, C.c_uint64, _vp]),
    'mbx_attn_bwd': (_i, [_vp] * 5 + [_i, _i, _i, _i, _i, _f, _i, _i, _vp]),
    'mbx_attn_fwd_drop': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _i, _f, C.c_uint64, _vp]),
    'mbx_attn_bwd_drop': (_i, [_vp] * 5 + [_i, _i, _i, _i, _i, _f, _i, _i, _f, C.c_uint64, _vp]),
    'mbx_attn_bwd_stats': (_i, [_vp] * 8 + [_i, _i, _i, _i, _i, _f, _i, _vp]),
    'mbx_fuse_fwd': (_i, [_vp] * 6 + [_i, _i, _vp]),
    'mbx_fuse_ln_fwd': (_i, [_vp] * 12 + [_f] + [_vp] * 2 + [_i] * 3 + [_vp]),
    'mbx_fuse_bwd_ws': (_sz, [_i]),
    'mbx_fuse_bwd': (_i, [_vp] * 11 + [_i, _i, _i, _vp, _vp]),
    'mbx_fuse_bwd_pair': (_i, [_vp] * 10 + [_i, _i, _vp, _vp]),
    'mbx_average': (_i, [_vp, _vp, _vp, _sz, _vp]),
    'mbx_average_bwd': (_i, [_vp] * 5 + [_sz, _i, _vp]),
    'mbx_head_fwd': (_i, [_vp] * 4 + [_i, _i, _i, _vp]),
    'mbx_head_bwd_ws': (_sz, [_i, _i]),
    'mbx_head_bwd': (_i, [_vp] * 6 + [_i, _i, _i, _i, _vp, _vp]),
    'mbx_tanh_bwd': (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    'mbx_pose_loss_ws': (_sz, [_i, _i]),
    'mbx_pose_loss': (_i, [_vp, _vp, _f, _f, _vp, _vp, _f, _i, _i, _i, _vp, _vp]),
    'mbx_pose_loss_full_ws': (_sz, [_i, _i]),
    'mbx_pose_loss_full': (_i, [_vp, _vp] + [_f] * 6 + [_vp, _vp, _f, _i, _i, _i, _vp, _vp]),
    'mbx_loss_2d_weighted_ws': (_sz, [_i, _i]),
    'mbx_loss_2d_weighted': (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _f, _i, _i, _i, _vp, _vp]),
    'mbx_pool_rep_fwd': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, C.c_uint64, _vp]),
    'mbx_tanh_pool_bwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, C.c_uint64, _i, _vp]),
    'mbx_dropout': (_i, [_vp, _vp, _sz, _f, C.c_uint64, _i, _vp]),
    'mbx_residual_drop': (_i, [_vp, _vp, _sz, _i, _i, _f, C.c_uint64, _f, C.c_uint64, _vp]),
    'mbx_grad_drop': (_i, [_vp, _vp, _sz, _i, _i, _f, C.c_uint64, _f, C.c_uint64, _i, _vp]),
    'mbx_augment2d': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp] + [_f] * 8 + [_i, C.c_uint64, _vp]),
    'mbx_embed_fwd_tta': (_i, [_vp] * 7 + [_i] * 5 + [_vp]),
    'mbx_flip_average': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'mbx_pose_errors': (_i, [_vp] * 5 + [_i] * 3 + [_vp] * 2 + [_i] * 3 + [_vp]),
    'mbx_eval_reduce_ws': (_sz, [_i, _i]),
    'mbx_eval_reduce': (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i] + [_vp] * 5),
    'mbx_supcon_loss_ws': (_sz, [_i, _i]),
    'mbx_supcon_loss': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _i, _f, _vp, _vp, _vp, _vp]),
    'mbx_nn_cosine': (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    'mbx_rot6d_theta_fwd': (_i, [_vp, _vp, _vp, _i, _vp]),
    'mbx_rot6d_theta_bwd': (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    'mbx_mesh_param_loss_ws': (_sz, [_i]),
    'mbx_mesh_param_loss': (_i, [_vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _i, _vp, _vp]),
    'mbx_mesh_errors': (_i, [_vp] * 5 + [_i, _i, _vp]),
    'mbx_smpl_pack': (_i, [_vp, _vp, _vp, _i, _vp]),
    'mbx_smpl_fwd_ws': (_sz, [_i, _i, _i]),
    'mbx_smpl_bwd_ws': (_sz, [_i, _i, _i]),
    'mbx_smpl_fwd': (_i, [_vp] * 5 + [C.POINTER(C.c_int)] + [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    'mbx_smpl_bwd': (_i, [_vp] * 6 + [C.POINTER(C.c_int)] + [_vp, _vp, _i, _vp, _vp, _f] + [_vp] * 5 + [_i, _i, _vp, _sz, _vp]),
    'mbx_mesh_gt_ws': (_sz, [_i, _i, _i]),
    'mbx_mesh_gt': (_i, [_vp, _vp, _vp, _vp, C.c_uint64, _f] + [_vp] * 5 + [C.POINTER(C.c_int)] + [_vp, _vp, _i, _f] + [_vp] * 5 + [_i, _i, _i, _vp, _sz, _vp]),
    'mbx_action_input': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp] + [_f] * 8 + [_i, C.c_uint64, _vp]),
    'mbx_motion2d_input': (_i, [_vp] * 5 + [_i, _i, _i, _vp, _vp] + [_f] * 3 + [_vp] * 3 + [_f] * 8 + [_i, C.c_uint64, _vp]),
    'mbx_amass_joints': (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, C.POINTER(C.c_int)] + [_vp] * 4 + [_i, _i, _i, _vp, _i, _vp]),
    'mbx_xent_topk': (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp]),
    'mbx_wild_input_ws': (_sz, [_i, _i]),
    'mbx_wild_input': (_i, [_vp, _vp, _i, _vp, _i, _i] + [C.c_double] * 4 + [_i, _i, _vp, _vp, _vp, _sz, _vp]),
    'mbx_wild_output': (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _f, C.c_double, C.c_double, _vp, _vp]),
    'mbx_wild_output_ragged': (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _f, C.c_double, C.c_double, _vp, _vp]),
    'mbx_attn_fwd_ragged': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    'mbx_embed_fwd_ragged': (_i, [_vp] * 7 + [_i] * 5 + [_vp]),
    'mbx_embed_fwd_tta_ragged': (_i, [_vp] * 8 + [_i] * 5 + [_vp]),
    'mbx_wild_mesh_ws': (_sz, [_i, _i, _i, _i]),
    'mbx_wild_mesh': (_i, [_vp] * 5 + [C.POINTER(C.c_int)] + [_vp, _vp, _i] + [_vp] * 4 + [_f, _vp] + [_i] * 4 + [_vp] * 3 + [_i, _vp, _sz, _vp]),
    'mbx_scale_fit': (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    'mbx_wild_mesh_place': (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp]),
    'mbx_render_project': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'mbx_render_raster_ws': (_sz, [_i, _i]),
    'mbx_render_raster': (_i, [_vp, _vp, _vp] + [_i] * 5 + [_f] * 4 + [_vp, _vp, _vp, _vp, _sz, _vp]),
    'mbx_skeleton_project': (_i, [_vp, C.POINTER(C.c_double), _i, _i, _i, _i, _vp, _vp]),
    'mbx_skeleton_raster': (_i, [_vp, _vp, _vp] + [_i] * 8 + [_vp, _vp, _vp]),
    'mbx_scene_project': (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    'mbx_scene_raster': (_i, [_vp] * 4 + [_i] + [_vp, _vp] + [_i] * 11 + [_vp, _i, _i, _vp, _vp, _vp]),
    'mbx_jpeg_header': (_i, [_i] * 5 + [_vp]),
    'mbx_jpeg_blocks': (_i, [_vp] + [_i] * 5 + [_vp, _vp]),
    'mbx_jpeg_entropy_ws': (_sz, [_i] * 5),
    'mbx_jpeg_entropy_sizes': (_i, [_vp] + [_i] * 6 + [_vp, _vp, _sz, _vp]),
    'mbx_jpeg_entropy': (_i, [_vp] + [_i] * 6 + [_vp, _vp, C.c_longlong, _vp, _sz, _vp]),
    'mbx_jpeg_dec_tables': (_i, [_vp, _vp]),
    'mbx_jpeg_dec_index': (_i, [_vp, C.c_longlong, _vp, _i, _i, _vp, _vp, _vp]),
    'mbx_jpeg_dec_entropy': (_i, [_vp, C.c_longlong, _vp, _vp] + [_i] * 5 + [_vp, _vp, _vp]),
    'mbx_jpeg_dec_ws': (_sz, [_i] * 4),
    'mbx_jpeg_dec_sync_ws': (_sz, [_i, _i, C.c_longlong]),
    'mbx_jpeg_dec_entropy_sync': (_i, [_vp, C.c_longlong, _vp, _vp] + [_i] * 5 + [C.c_longlong, _vp, _vp, _vp, _vp, _sz, _vp]),
    'mbx_jpeg_dec_pixels': (_i, [_vp, _vp] + [_i] * 4 + [_vp, _vp, _sz, _vp]),
    'mbx_rows_n_pack_bytes': (_sz, [_i, _i]),
    'mbx_rows_lnbwd_t': (_i, [_vp] * 6 + [_i, _i, _i, _vp]),
    'mbx_rows_n_pack_many': (_i, [_i64p, _i, _i, _i, _vp]),
    'mbx_rows_resid_ln': (_i, [_vp] * 8 + [_f, _i, _i, _i, _vp]),
    'mbx_mfma_probe_ws': (_sz, [_i]),
    'mbx_mfma_probe': (_i, [_vp, _i, _i, C.c_uint, _vp, _vp]),
    'mbx_adamw_step': (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _f, _f, _f, _f, _i, _vp]),
}


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """dlopen libmbx.so and attach the prototypes.  Works without a GPU (symbols only)."""
    if not os.path.exists(path):
        raise RuntimeError(f'{path} not found: build it with `python -m motionbert_amd.build` '
                           '(hipcc --offload-arch=gfx950); there is no fallback implementation')
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    return lib


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class HipOps:
    """Kernel provider backed by libmbx.so.  Stateless apart from size caches."""

    multi_stream = True   # every call takes the current stream: safe to drive from several HIP streams
    grad_stream_t = True  # mbx_gemm_nt_lnbwd_t exists: the gradient residual stream may travel as bf16 inside a Block

    def __init__(self, lib: Optional[C.CDLL] = None):
        self.lib = lib or load_library()
        self._ws_cache: Dict[tuple, int] = {}
        self._desc_cache: Dict[tuple, dict] = {}
        self._desc_held: Dict[int, dict] = {}         # descriptor-table entries a captured hipGraph reads at replay (_hold_if_capturing)
        self.weight_cache: Dict[int, tuple] = {}      # device index -> (key, prepared weights) of the last no-grad forward (engine.prepare_weights)
        self._lock = threading.Lock()

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc: int):
        if rc != 0:
            raise RuntimeError('libmbx: ' + self.lib.mbx_last_error().decode())

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def _ws(self, key: tuple, fn, *args, device=None) -> torch.Tensor:
        n = self._ws_cache.get(key)
        if n is None:
            n = int(fn(*args))
            self._ws_cache[key] = n
        return torch.empty(max(n, 16), dtype=torch.uint8, device=device)

    def _hold_if_capturing(self, ent: dict):
        """Called under the lock with the descriptor-table entry a packer is about to read.  A hipGraph under capture records the
        ADDRESSES of the entry's device tables in its copy nodes and reads them again at every replay, while the tables live in the
        ordinary allocator pool and belong to `_desc_cache` alone: once `_desc_room` dropped the entry (another model's forward
        adding the 16th of its kind) the allocator handed the memory on and the replay packed weights from whatever lay there.
        Entries used during a capture are therefore kept for the life of the provider (a few hundred bytes each)."""
        if torch.cuda.is_current_stream_capturing():
            self._desc_held[id(ent)] = ent

    # ------------------------------------------------------------------ weights
    def prep_weights(self, P: Dict[str, torch.Tensor], names: List[str], tdtype, need_t: bool, x3: bool = False):
        """T-typed copies of every Linear weight: Wn[name] [N,K] and (for backward) Wt[name] [K,N].
        x3 (precision 'bf16x3'): every entry is a (hi, lo) pair of bf16 planes, w = hi + lo up to 2^-16 relative."""
        if x3:
            hi_n, hi_t = self._prep_weights(P, names, torch.bfloat16, need_t, False)
            lo_n, lo_t = self._prep_weights(P, names, torch.bfloat16, need_t, True)
            return ({n: (hi_n[n], lo_n[n]) for n in names}, {n: (hi_t[n], lo_t[n]) for n in names} if need_t else {})
        return self._prep_weights(P, names, tdtype, need_t, False)

    def _desc_room(self, kind: str, keep: int = 16):
        """Called under the lock before a descriptor-table entry of `kind` is added: once `keep` of that kind exist (models come and
        go, operands move) they are dropped -- only that kind, the dict is shared by the three packers."""
        stale = [k for k in self._desc_cache if k[0] == kind]
        if len(stale) >= keep:
            for k in stale:
                del self._desc_cache[k]

    def _desc_entry(self, kind: str, key: tuple, build) -> dict:
        """The descriptor-cache protocol of the three packers: the entry of `(kind,) + key`; where it is missing, room is made and
        `build()` makes it (`desc`: the device table without the addresses that change from call to call, filled into a clone)."""
        with self._lock:
            ent = self._desc_cache.get((kind,) + key)
            if ent is None:
                self._desc_room(kind)
                ent = self._desc_cache[(kind,) + key] = build()
            self._hold_if_capturing(ent)
        return ent

    def _prep_weights(self, P, names, tdtype, need_t, lo):
        ws = [P[n + '.weight'] for n in names]
        dev = ws[0].device
        dt = _DT[tdtype]

        def build():
            offs = list(accumulate((w.numel() for w in ws), initial=0))      # element offsets into the flat buffers, the total last
            return dict(desc=torch.tensor([[w.data_ptr(), 0, 0, *w.shape] for w in ws], dtype=torch.int64).to(dev),
                        offs=(torch.tensor(offs[:-1], dtype=torch.int64) * torch.empty(0, dtype=tdtype).element_size()).to(dev),
                        offs_host=offs[:-1], total=offs[-1], max_n=max(w.shape[0] for w in ws), max_k=max(w.shape[1] for w in ws))
        key = (tuple((w.data_ptr(), tuple(w.shape)) for w in ws), dt, dev.index)
        ent = self._desc_entry('prep', key, build)
        for w in ws:
            if w.dtype != torch.float32 or not w.is_contiguous():
                raise RuntimeError('libmbx: parameters must be contiguous fp32')
        desc = ent['desc'].clone()
        make_n = tdtype != torch.float32          # fp32 mode reads the parameters in place
        flat_n = torch.empty(ent['total'], dtype=tdtype, device=dev) if make_n else None
        flat_t = torch.empty(ent['total'], dtype=tdtype, device=dev) if need_t else None
        if make_n:
            desc[:, 1] = ent['offs'] + flat_n.data_ptr()
        if need_t:
            desc[:, 2] = ent['offs'] + flat_t.data_ptr()
        if make_n or need_t:
            self._ck(self.lib.mbx_prep_weights(desc.data_ptr(), len(ws), ent['max_n'], ent['max_k'], MBX_BF16_LO if lo else dt, self._stream()))
        Wn, Wt = {}, {}
        for n, w, off in zip(names, ws, ent['offs_host']):
            N, K = w.shape
            Wn[n] = flat_n[off:off + N * K].view(N, K) if make_n else w.detach()
            if need_t:
                Wt[n] = flat_t[off:off + N * K].view(K, N)
        return Wn, Wt

    # ------------------------------------------------------------------ LayerNorm folding (bf16 path)
    @staticmethod
    def can_fold(tdtype, cfg) -> bool:
        """The folded-LayerNorm kernels exist for bf16 operands; every kernel-side shape constraint of the set is mirrored HERE, because
        the decision is taken before the forward (which then drops the fp32 sub-layer inputs) and a refusal in backward would come too
        late: GELU' row dots per 64-column block and the 64-wide k tiles of the LayerNorm-backward GEMM (hidden % 64, C % 64: K of the dX
        GEMMs is 3 C / hidden, N is C), attention row dots in the bf16 kernels with head dim 32 / 64 (every sequence length: the streamed kernels beyond 256
        frames have the row-dot form too)."""
        return tdtype == torch.bfloat16 and cfg.hidden % 64 == 0 and cfg.C % 64 == 0 and cfg.hd in (32, 64)

    def fold_norm_weights(self, P: Dict[str, torch.Tensor], pairs, need_t: bool, tdtype=torch.bfloat16):
        """For every (linear, norm) pair: Wn[linear] = bf16(W diag(gamma)) [N,K], Wt[linear] = its transpose [K,N] (need_t),
        Bf[linear] = b + W beta (fp32 [N]), Rs[linear] = row sums of the rounded folded weights (fp32 [N]).  One call, two launches."""
        if tdtype != torch.bfloat16:
            raise RuntimeError('libmbx: fold_norm_weights is a bf16 path')
        ps = [(P[l + '.weight'], P.get(l + '.bias'), P[n + '.weight'], P[n + '.bias']) for l, n in pairs]      # W, b, gamma, beta
        ws = [p[0] for p in ps]
        dev = ws[0].device

        def build():
            for t in (t for p in ps for t in p if t is not None):
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError('libmbx: parameters must be contiguous fp32')
            offs = list(accumulate((w.numel() for w in ws), initial=0))      # element offsets of the weights, the total last
            voffs = list(accumulate((w.shape[0] for w in ws), initial=0))      # ... of the [N] vectors
            rows = [[w.data_ptr(), _p(b) or 0, g.data_ptr(), bt.data_ptr(), 0, 0, 0, 0, *w.shape] for w, b, g, bt in ps]
            return dict(desc=torch.tensor(rows, dtype=torch.int64).to(dev), offs=(torch.tensor(offs[:-1], dtype=torch.int64) * 2).to(dev),
                        voffs=(torch.tensor(voffs[:-1], dtype=torch.int64) * 4).to(dev), offs_host=offs[:-1], voffs_host=voffs[:-1],
                        total=offs[-1], vtotal=voffs[-1], max_n=max(w.shape[0] for w in ws), max_k=max(w.shape[1] for w in ws))
        key = (tuple((w.data_ptr(), tuple(w.shape), g.data_ptr(), bt.data_ptr(), _p(b) or 0) for w, b, g, bt in ps), dev.index)
        ent = self._desc_entry('fold', key, build)
        desc = ent['desc'].clone()
        flat_n = torch.empty(ent['total'], dtype=torch.bfloat16, device=dev)
        flat_t = torch.empty(ent['total'], dtype=torch.bfloat16, device=dev) if need_t else None
        flat_b = torch.empty(ent['vtotal'], dtype=torch.float32, device=dev)
        flat_r = torch.empty(ent['vtotal'], dtype=torch.float32, device=dev)
        desc[:, 4] = ent['offs'] + flat_n.data_ptr()
        if need_t:
            desc[:, 5] = ent['offs'] + flat_t.data_ptr()
        desc[:, 6] = ent['voffs'] + flat_b.data_ptr()
        desc[:, 7] = ent['voffs'] + flat_r.data_ptr()
        self._ck(self.lib.mbx_fold_norm_weights(desc.data_ptr(), len(ws), ent['max_n'], ent['max_k'], self._stream()))
        Wn, Wt, Bf, Rs = {}, {}, {}, {}
        for (l, _), w, off, voff in zip(pairs, ws, ent['offs_host'], ent['voffs_host']):
            N, K = w.shape
            Wn[l] = flat_n[off:off + N * K].view(N, K)
            if need_t:
                Wt[l] = flat_t[off:off + N * K].view(K, N)
            Bf[l], Rs[l] = flat_b[voff:voff + N], flat_r[voff:voff + N]
        return Wn, Wt, Bf, Rs

    def gemm_nt_dgelu_stats(self, a_t, w_t, out_t, aux_t, bias_f, rsum, part):
        M, K = a_t.shape
        N = w_t.shape[0]
        self._ck(self.lib.mbx_gemm_nt_dgelu_stats(_p(a_t), _p(w_t), _p(out_t), _p(aux_t), _p(bias_f), _p(rsum), _p(part), M, N, K, self._stream()))

    # round 5: fc1 + GELU with the derivative saved for backward instead of the pre-activation, and the one-multiply backward epilogue
    @staticmethod
    def can_gelu_d(tdtype, cfg) -> bool:
        return tdtype == torch.bfloat16 and cfg.hidden >= 256 and cfg.hidden % 8 == 0 and cfg.C % 64 == 0

    def gemm_nt_gelu_d(self, a_t, w_t, bias, out_d, out_g):
        M, K = a_t.shape
        N = w_t.shape[0]
        self._ck(self.lib.mbx_gemm_nt_gelu_d(_p(a_t), _p(w_t), _p(bias), _p(out_d), _p(out_g), M, N, K, self._stream()))

    def gemm_nt_mul(self, a_t, w_t, aux_t, out_t):
        M, K = a_t.shape
        N = w_t.shape[0]
        self._ck(self.lib.mbx_gemm_nt_mul(_p(a_t), _p(w_t), _p(aux_t), _p(out_t), M, N, K, self._stream()))

    def attn_bwd_stats(self, qkv, o, do, lse, dqkv, bias_f, rsum, part, B, T, J, H, scale, mode):
        hd = o.shape[-1] // H
        self._ck(self.lib.mbx_attn_bwd_stats(_p(qkv), _p(o), _p(do), _p(lse), _p(dqkv), _p(bias_f), _p(rsum), _p(part), B, T, J, H, hd,
                                             float(scale), int(mode), self._stream()))

    def lnbwd_rowc(self, part, rstd, rowc, C):
        nb, M = part.shape[0], part.shape[1]          # block-major partial row dots [nb, M, 2]
        self._ck(self.lib.mbx_lnbwd_rowc(_p(part), nb, _p(rstd), _p(rowc), M, int(C), self._stream()))

    def gemm_nt_lnbwd(self, a_t, w_t, xhat, rowc, dres, extra, dx, dx_t):
        """dres fp32: dx fp32 (+ optional bf16 copy dx_t).  dres bf16 (the gradient stream inside a Block): dx and dx_t both optional."""
        M, K = a_t.shape
        N = w_t.shape[0]
        fn = self.lib.mbx_gemm_nt_lnbwd_t if dres.dtype == torch.bfloat16 else self.lib.mbx_gemm_nt_lnbwd
        self._ck(fn(_p(a_t), _p(w_t), _p(xhat), _p(rowc), _p(dres), _p(extra), _p(dx), _p(dx_t), M, N, K, self._stream()))

    # ------------------------------------------------------------------ raw-operand LayerNorm + fused MLP (bf16 no-grad path)
    @staticmethod
    def can_fuse_mlp(tdtype, cfg) -> bool:
        """The fused MLP forward (mbx_mlp_fused_fwd) and the raw-operand GEMMs exist for bf16, C in {256, 512}."""
        return tdtype == torch.bfloat16 and cfg.C in (256, 512) and cfg.hidden % 64 == 0 and cfg.hidden <= 1536

    def mlp_pack_weights(self, w1_t, w2_t):
        """fc1 [hidden, C] and fc2 [C, hidden] (bf16) -> the MFMA-fragment stream mbx_mlp_fused_fwd consumes."""
        hidden, Cc = w1_t.shape
        packed = torch.empty(int(self.lib.mbx_mlp_pack_bytes(Cc, hidden)), dtype=torch.uint8, device=w1_t.device)
        self._ck(self.lib.mbx_mlp_pack_weights(_p(w1_t), _p(w2_t), _p(packed), Cc, hidden, self._stream()))
        return packed

    def proj_mlp_pack_weights(self, wp_t, w1_t, w2_t):
        """attn.proj [C, C], fc1 [hidden, C] (folded) and fc2 [C, hidden] (bf16) -> the fragment stream of mbx_proj_mlp_fused_fwd."""
        hidden, Cc = w1_t.shape
        packed = torch.empty(int(self.lib.mbx_proj_mlp_pack_bytes(Cc, hidden)), dtype=torch.uint8, device=w1_t.device)
        self._ck(self.lib.mbx_proj_mlp_pack_weights(_p(wp_t), _p(w1_t), _p(w2_t), _p(packed), Cc, hidden, self._stream()))
        return packed

    def proj_mlp_fused_fwd(self, o_t, packed, bp, b1, b2, rsum, resid, y, eps):
        """y = y1 + fc2(gelu(fc1(LayerNorm(y1)))), y1 = resid + o . Wp^T + bp: attention proj + residual + the whole MLP sub-layer, one kernel."""
        M, Cc = resid.shape
        self._ck(self.lib.mbx_proj_mlp_fused_fwd(_p(o_t), _p(packed), _p(bp), _p(b1), _p(b2), _p(rsum), _p(resid), _p(y), float(eps), M, Cc,
                                                 b1.shape[0], self._stream()))

    def mlp_fused_fwd(self, a_t, raw_in, packed, b1, b2, rsum, resid, y, y_t, eps, mean, rstd):
        """a_t = None: the raw operand is made in the kernel from the fp32 rows of `resid`."""
        M, Cc = resid.shape
        self._ck(self.lib.mbx_mlp_fused_fwd(_p(a_t), int(bool(raw_in)), _p(packed), _p(b1), _p(b2), _p(rsum), _p(resid), _p(y), _p(y_t),
                                            float(eps), _p(mean), _p(rstd), M, Cc, b1.shape[0], self._stream()))

    # ------------------------------------------------------------------ row-owner GEMMs (gemm_rows.hip)
    def rows_pack_nk(self, w_t):
        """w [N, K] bf16 (K in {256, 512}) -> the MFMA-fragment stream of the K-resident row-owner GEMM."""
        N, K = w_t.shape
        packed = torch.empty(int(self.lib.mbx_rows_pack_bytes(N, K)), dtype=torch.uint8, device=w_t.device)
        self._ck(self.lib.mbx_rows_pack_nk(_p(w_t), _p(packed), N, K, self._stream()))
        return packed

    def rows_gemm_nk(self, a_t, packed, bias, out_t, rsum=None, mean=None, rstd=None):
        """out_t bf16 [M,N] = a . w^T + bias, or with (rsum, mean, rstd) the raw-operand LayerNorm form out = rstd (a . w^T - mean rsum) + bias."""
        M, K = a_t.shape
        self._ck(self.lib.mbx_rows_gemm_nk(_p(a_t), _p(packed), _p(bias), _p(rsum), _p(mean), _p(rstd), _p(out_t), M, out_t.shape[1], K,
                                           self._stream()))

    def rows_gemm_nk_ln(self, x, packed, bias, rsum, eps, out_t):
        """out_t bf16 [M,N] = Linear'(LayerNorm(x)) straight from the fp32 rows x [M,K]: operand bf16(x) and the row statistics are made
        in the kernel (no LayerNorm pass, no bf16 copy of the residual stream)."""
        M, K = x.shape
        self._ck(self.lib.mbx_rows_gemm_nk_ln(_p(x), _p(packed), _p(bias), _p(rsum), float(eps), _p(out_t), M, out_t.shape[1], K, self._stream()))

    # ------------------------------------------------------------------ N-resident row-owner GEMM + LayerNorm backward (round 5)
    @staticmethod
    def can_rows_lnbwd(tdtype, cfg) -> bool:
        """mbx_rows_lnbwd_t / mbx_rows_resid_ln exist for bf16, dim_feat 512 (contraction lengths C, 3 C, hidden: multiples of 256, >= 512) and
        -- round 6 -- dim_feat 256 (MotionBERT-Lite: multiples of 256, >= 256); anything else falls back to the tile kernels."""
        return (tdtype == torch.bfloat16 and cfg.C in (256, 512) and cfg.hidden % 256 == 0 and cfg.hidden >= (512 if cfg.C == 512 else 256))

    def rows_n_pack(self, w_t):
        """w bf16 [N, K], N = 512 or 256 (the operand of the dX GEMM) in the fragment order of mbx_rows_lnbwd_t / mbx_rows_resid_ln."""
        return self.rows_n_pack_many([w_t])[0]

    def rows_n_pack_many(self, ws):
        """rows_n_pack of every operand of the list in one launch; the results are views into one buffer.  The descriptor table lives on the
        device and is cached by the operands' offsets from the first one: no host-to-device copy in the steady state (nor inside a graph
        capture after a warm-up step); source and destination addresses are filled in on the device."""
        if not ws:
            return []
        dev = ws[0].device
        N = ws[0].shape[0]
        for w in ws:
            if w.shape[0] != N or N not in (256, 512) or w.shape[1] < N or w.shape[1] % 256 or w.dtype != torch.bfloat16 or not w.is_contiguous():
                raise RuntimeError(f'rows_n_pack_many: operand {tuple(w.shape)} {w.dtype} (bf16 [N, K], one N = 256 or 512 for all, K % 256 == 0, '
                                   f'K >= N, contiguous)')
        # The descriptor table is cached by the operands' offsets from the first one -- stable from step to step when they are views into
        # ONE flat buffer (prep_weights / fold_norm_weights make them so).  Operands of separate allocations get absolute addresses in
        # the key instead: still correct, just a cache entry per set of addresses.
        base = ws[0].data_ptr()
        store = ws[0].untyped_storage().data_ptr()
        if any(w.untyped_storage().data_ptr() != store for w in ws):
            base = 0

        def build():
            offs = list(accumulate((N * w.shape[1] * 2 for w in ws), initial=0))      # byte offsets into the flat buffer, the total last
            rows = [[w.data_ptr() - base, o, w.shape[1]] for w, o in zip(ws, offs)]
            return dict(desc=torch.tensor(rows, dtype=torch.int64).to(dev), offs=offs[:-1], total=offs[-1], max_k=max(w.shape[1] for w in ws))
        key = (base == 0, N, tuple((w.data_ptr() - base, w.shape[1]) for w in ws), dev.index)
        ent = self._desc_entry('rnpack', key, build)
        flat = torch.empty(ent['total'], dtype=torch.uint8, device=dev)
        desc = ent['desc'].clone()
        desc[:, 0] += base
        desc[:, 1] += flat.data_ptr()
        self._ck(self.lib.mbx_rows_n_pack_many(desc.data_ptr(), len(ws), N, ent['max_k'], self._stream()))
        return [flat[o:o + N * w.shape[1] * 2] for w, o in zip(ws, ent['offs'])]

    def rows_lnbwd_t(self, dy_t, packed, xhat, rstd, dres_t, dx_t):
        """dx_t = T(dres_t + LayerNorm'(dy . w^T)) with both row means taken in the kernel (no row dots from the producers of dy)."""
        M, K = dy_t.shape
        self._ck(self.lib.mbx_rows_lnbwd_t(_p(dy_t), _p(packed), _p(xhat), _p(rstd), _p(dres_t), _p(dx_t), M, dx_t.shape[1], K, self._stream()))

    can_rows_resid_ln = can_rows_lnbwd      # same shape constraints (dim_feat 512 or 256; contraction lengths C and hidden)

    def rows_resid_ln(self, a_t, packed, bias, resid, y, xhat, mean, rstd, eps):
        """y = resid + a . w^T + bias (fp32) and the plain LayerNorm of its rows (xhat in the operand type, mean, rstd) in one kernel."""
        M, K = a_t.shape
        self._ck(self.lib.mbx_rows_resid_ln(_p(a_t), _p(packed), _p(bias), _p(resid), _p(y), _p(xhat), _p(mean), _p(rstd), float(eps), M, y.shape[1], K,
                                            self._stream()))

    # ------------------------------------------------------------------ measurement aid (bench.py, tools/clock_power.py)
    def mfma_probe(self, seconds: float = 0.25, wgs_per_cu: int = 1, device=None):
        """The bf16 MFMA rate the part sustains with nothing but MFMAs in the loop (random operands), run for about `seconds` so
        that the power management has settled: dict(tflops, clock_ghz, ms).  `clock_ghz` = shader cycles / real time inside the
        kernel (median over workgroups)."""
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        n_wg = cus * wgs_per_cu
        ws = torch.zeros(int(self.lib.mbx_mfma_probe_ws(n_wg)), dtype=torch.uint8, device=dev)
        flops = C.c_double(0.0)

        def run(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._ck(self.lib.mbx_mfma_probe(_p(ws), n_wg, iters, 1234, C.byref(flops), self._stream()))
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        ms = run(20000)                                            # calibrate, then one long launch
        iters = max(20000, int(20000 * seconds * 1e3 / max(ms, 1e-3)))
        ms = run(iters)
        st = ws[n_wg * 1024:].view(torch.int64).view(n_wg, 2).cpu().double()
        clock = float((st[:, 0] / (st[:, 1] * 1e-8)).median()) / 1e9
        return dict(tflops=flops.value / ms / 1e9, clock_ghz=clock, ms=ms, iters=iters, wgs_per_cu=wgs_per_cu)

    def unfold_norm_grads(self, dw, db, w, gamma, beta, dgamma, dbeta):
        N, K = dw.shape
        ws = self._ws(('unf', N, K), self.lib.mbx_unfold_norm_grads_ws, N, K, device=dw.device)
        self._ck(self.lib.mbx_unfold_norm_grads(_p(dw), _p(db), _p(w), _p(gamma), _p(beta), _p(dgamma), _p(dbeta), N, K, _p(ws), self._stream()))

    # ------------------------------------------------------------------ embedding
    def embed_fwd(self, x, w, b, pos, temp, h, B, T, J):
        self._ck(self.lib.mbx_embed_fwd(_p(x), _p(w), _p(b), _p(pos), _p(temp), _p(h), B, T, J, x.shape[-1], h.shape[-1],
                                        self._stream()))

    @staticmethod
    def can_embed_ln(tdtype, cfg) -> bool:
        """mbx_embed_ln_fwd writes a bf16 xhat and keeps the embedding weights in registers: bf16, dim_in <= 4, dim_feat <= 1024."""
        return tdtype == torch.bfloat16 and cfg.dim_in <= 4 and cfg.C <= 1024 and cfg.C % 4 == 0

    def embed_ln_fwd(self, x, w, b, pos, temp, eps, h, xhat, mean, rstd, B, T, J):
        """embed_fwd and the plain normalisation of its rows (layernorm_fwd(h, None, None)) in one launch; xhat bf16"""
        if xhat.dtype != torch.bfloat16:
            raise RuntimeError('libmbx: embed_ln_fwd writes a bf16 xhat')
        self._ck(self.lib.mbx_embed_ln_fwd(_p(x), _p(w), _p(b), _p(pos), _p(temp), float(eps), _p(h), _p(xhat), _p(mean), _p(rstd), B, T, J,
                                           x.shape[-1], h.shape[-1], self._stream()))

    def embed_bwd(self, dh, x, w, dw, db, dpos, dtemp, dx, B, T, J):
        Din, Cc = x.shape[-1], dh.shape[-1]
        ws = self._ws(('emb', T, J, Din, Cc), self.lib.mbx_embed_bwd_ws, T, J, Din, Cc, device=dh.device)
        dtemp.zero_()
        self._ck(self.lib.mbx_embed_bwd(_p(dh), _p(x), _p(w), _p(dw), _p(db), _p(dpos), _p(dtemp), _p(dx), B, T, J, Din, Cc,
                                        _p(ws), self._stream()))

    def embed_bwd_pair(self, dh_a, dh_b, x, w, dw, db, dpos, dtemp, dx, B, T, J):
        """embed_bwd with the incoming gradient as the sum of two bf16 tensors (the two Blocks' input gradients of level 0)."""
        Din, Cc = x.shape[-1], dh_a.shape[-1]
        ws = self._ws(('emb', T, J, Din, Cc), self.lib.mbx_embed_bwd_ws, T, J, Din, Cc, device=dh_a.device)
        dtemp.zero_()
        self._ck(self.lib.mbx_embed_bwd_pair(_p(dh_a), _p(dh_b), _p(x), _p(w), _p(dw), _p(db), _p(dpos), _p(dtemp), _p(dx), B, T, J, Din, Cc,
                                             _p(ws), self._stream()))

    # ------------------------------------------------------------------ layernorm
    layernorm_fwd_planes_ok = True      # the producers below accept a (hi, lo) pair of bf16 planes where a bf16x3 GEMM operand is due

    def layernorm_fwd(self, x, g, b, eps, y_t, mean, rstd):
        M, Cc = x.shape
        if isinstance(y_t, tuple):      # bf16x3: the operand planes straight from the kernel
            self._ck(self.lib.mbx_layernorm_fwd_planes(_p(x), _p(g), _p(b), float(eps), _p(y_t[0]), _p(y_t[1]), _p(mean), _p(rstd), M, Cc,
                                                       self._stream()))
            return
        self._ck(self.lib.mbx_layernorm_fwd(_p(x), _p(g), _p(b), float(eps), _p(y_t), _p(mean), _p(rstd), M, Cc,
                                            _DT[y_t.dtype], self._stream()))

    def layernorm_bwd(self, dy_t, x, mean, rstd, g, dres, extra, dx, dx_t, dg, db):
        M, Cc = x.shape
        ws = self._ws(('lnb', Cc), self.lib.mbx_layernorm_bwd_ws, Cc, device=x.device)
        if isinstance(dx_t, tuple):      # bf16x3: the T copy of dx as operand planes
            self._ck(self.lib.mbx_layernorm_bwd_planes(_p(dy_t), _p(x), _p(mean), _p(rstd), _p(g), _p(dres), _p(extra), _p(dx), _p(dx_t[0]),
                                                       _p(dx_t[1]), _p(dg), _p(db), M, Cc, _p(ws), self._stream()))
            return
        self._ck(self.lib.mbx_layernorm_bwd(_p(dy_t), _p(x), _p(mean), _p(rstd), _p(g), _p(dres), _p(extra), _p(dx), _p(dx_t),
                                            _p(dg), _p(db), M, Cc, _DT[dy_t.dtype], _p(ws), self._stream()))

    # ------------------------------------------------------------------ GEMMs
    def gelu_fwd(self, u, g):
        self._ck(self.lib.mbx_gelu_fwd(_p(u), _p(g), u.numel(), _DT[u.dtype], self._stream()))

    def split(self, t):
        """fp32 tensor -> (hi, lo) bf16 planes of the bf16x3 split (t = hi + lo up to 2^-16 relative)."""
        hi, lo = torch.empty_like(t, dtype=torch.bfloat16), torch.empty_like(t, dtype=torch.bfloat16)
        self._ck(self.lib.mbx_split_bf16(_p(t), _p(hi), _p(lo), t.numel(), self._stream()))
        return hi, lo

    def gemm_nt(self, a_t, w_t, bias, epi, out_t=None, out2_t=None, out_f=None, resid=None, aux_t=None):
        if isinstance(a_t, tuple):       # bf16x3: (hi, lo) operand planes, fp32 T-typed outputs
            (ah, al), (wh, wl) = a_t, w_t
            M, K = ah.shape
            N = wh.shape[0]
            if wh.shape[1] != K:
                raise RuntimeError(f'libmbx: gemm_nt_x3 operand mismatch {tuple(ah.shape)} x {tuple(wh.shape)}')
            planes = out2_t if isinstance(out2_t, tuple) else (out_t if isinstance(out_t, tuple) else None)
            if planes is not None:       # the last output leaves as the (hi, lo) planes of the operand split
                self._ck(self.lib.mbx_gemm_nt_x3p(_p(ah), _p(al), _p(wh), _p(wl), _p(bias), int(epi), _p(None if planes is out_t else out_t),
                                                  _p(planes[0]), _p(planes[1]), _p(aux_t), M, N, K, self._stream()))
                return
            self._ck(self.lib.mbx_gemm_nt_x3(_p(ah), _p(al), _p(wh), _p(wl), _p(bias), int(epi), _p(out_t), _p(out2_t), _p(out_f),
                                             _p(resid), _p(aux_t), M, N, K, self._stream()))
            return
        M, K = a_t.shape
        N = w_t.shape[0]
        if w_t.shape[1] != K or a_t.dtype != w_t.dtype:
            raise RuntimeError(f'libmbx: gemm_nt operand mismatch {tuple(a_t.shape)} {a_t.dtype} x {tuple(w_t.shape)} {w_t.dtype}')
        self._ck(self.lib.mbx_gemm_nt(_p(a_t), _p(w_t), _p(bias), int(epi), _p(out_t), _p(out2_t), _p(out_f), _p(resid),
                                      _p(aux_t), M, N, K, _DT[a_t.dtype], self._stream()))

    def gemm_tn(self, dy_t, a_t, dw, db):
        if isinstance(dy_t, tuple):      # bf16x3
            (yh, yl), (ah, al) = dy_t, a_t
            M, N = yh.shape
            K = ah.shape[1]
            ws = self._ws(('tnx3', M, N, K), self.lib.mbx_gemm_tn_x3_workspace, M, N, K, device=yh.device)
            self._ck(self.lib.mbx_gemm_tn_x3(_p(yh), _p(yl), _p(ah), _p(al), _p(dw), _p(db), M, N, K, _p(ws), self._stream()))
            return
        M, N = dy_t.shape
        K = a_t.shape[1]
        ws = self._ws(('tn', M, N, K), self.lib.mbx_gemm_tn_ws, M, N, K, device=dy_t.device)
        self._ck(self.lib.mbx_gemm_tn(_p(dy_t), _p(a_t), _p(dw), _p(db), M, N, K, _DT[dy_t.dtype], _p(ws), self._stream()))

    # ------------------------------------------------------------------ attention
    def attn_fwd(self, qkv, o, lse, B, T, J, H, scale, mode, drop=None):
        """drop = (p, seed): nn.Dropout(p) on the probabilities inside the kernel (counter-based mask, dropmask.py)."""
        hd = o.shape[-1] // H
        if drop is not None and drop[0] > 0:
            self._ck(self.lib.mbx_attn_fwd_drop(_p(qkv), _p(o), _p(lse), B, T, J, H, hd, float(scale), int(mode), _DT[qkv.dtype],
                                                float(drop[0]), int(drop[1]), self._stream()))
            return
        self._ck(self.lib.mbx_attn_fwd(_p(qkv), _p(o), _p(lse), B, T, J, H, hd, float(scale), int(mode), _DT[qkv.dtype],
                                       self._stream()))

    def attn_fwd_ragged(self, qkv, o, lse, clip_tab, n_clips, F, max_len, J, H, scale):
        """temporal attention of a ragged batch: qkv [F J,3C], o [F J,C], lse [F J,H]; clip_tab [>= n_clips,2] i32 on the device =
        (first frame, frames), every clip of at most max_len <= 256 frames."""
        if qkv.shape[0] != F * J or o.shape[0] != F * J or lse.numel() != F * J * H or qkv.shape[-1] != 3 * o.shape[-1]:
            raise RuntimeError(f'libmbx: attn_fwd_ragged needs qkv [{F * J},3C], o [{F * J},C] and lse [{F * J},{H}], got {tuple(qkv.shape)}, '
                               f'{tuple(o.shape)}, {tuple(lse.shape)}')
        if not all(t.is_contiguous() and t.device == qkv.device for t in (qkv, o, lse, clip_tab)) or o.dtype != qkv.dtype:
            raise RuntimeError('libmbx: attn_fwd_ragged needs contiguous tensors of one dtype on one device')
        self._dense('attn_fwd_ragged', torch.float32, F * J * H, qkv.device, lse=lse)
        self._dense('attn_fwd_ragged', torch.int32, None, qkv.device, clip_tab=clip_tab)
        if clip_tab.numel() < 2 * n_clips:
            raise RuntimeError(f'libmbx: attn_fwd_ragged: a table of {clip_tab.numel() // 2} rows for {n_clips} clips')
        self._ck(self.lib.mbx_attn_fwd_ragged(_p(qkv), _p(o), _p(lse), _p(clip_tab), int(n_clips), int(F), int(max_len), J, H, o.shape[-1] // H,
                                              float(scale), _DT[qkv.dtype], self._stream()))

    def attn_bwd(self, qkv, o, do, lse, dqkv, B, T, J, H, scale, mode, drop=None):
        hd = o.shape[-1] // H
        if isinstance(dqkv, tuple):      # bf16x3 (fp32 kernels): dq / dk / dv as operand planes
            p, seed = (float(drop[0]), int(drop[1])) if drop is not None and drop[0] > 0 else (0.0, 0)
            self._ck(self.lib.mbx_attn_bwd_planes(_p(qkv), _p(o), _p(do), _p(lse), _p(dqkv[0]), _p(dqkv[1]), B, T, J, H, hd, float(scale),
                                                  int(mode), p, seed, self._stream()))
            return
        if drop is not None and drop[0] > 0:
            self._ck(self.lib.mbx_attn_bwd_drop(_p(qkv), _p(o), _p(do), _p(lse), _p(dqkv), B, T, J, H, hd, float(scale), int(mode),
                                                _DT[qkv.dtype], float(drop[0]), int(drop[1]), self._stream()))
            return
        self._ck(self.lib.mbx_attn_bwd(_p(qkv), _p(o), _p(do), _p(lse), _p(dqkv), B, T, J, H, hd, float(scale), int(mode),
                                       _DT[qkv.dtype], self._stream()))

    # ------------------------------------------------------------------ fusion
    def fuse_fwd(self, x_st, x_ts, w, b, out, alpha):
        M, Cc = x_st.shape
        self._ck(self.lib.mbx_fuse_fwd(_p(x_st), _p(x_ts), _p(w), _p(b), _p(out), _p(alpha), M, Cc, self._stream()))

    def fuse_ln_fwd(self, x_st, x_ts, w, b, out, alpha, g1, b1, xn1, g2, b2, xn2, eps, mean, rstd):
        M, Cc = x_st.shape
        self._ck(self.lib.mbx_fuse_ln_fwd(_p(x_st), _p(x_ts), _p(w), _p(b), _p(out), _p(alpha), _p(g1), _p(b1), _p(xn1), _p(g2), _p(b2),
                                          _p(xn2), float(eps), _p(mean), _p(rstd), M, Cc, _DT[xn1.dtype], self._stream()))

    def fuse_bwd(self, dh, x_st, x_ts, alpha, w, d_st, d_ts, d_st_t, d_ts_t, dw, db):
        M, Cc = x_st.shape
        ws = self._ws(('fub', Cc), self.lib.mbx_fuse_bwd_ws, Cc, device=dh.device)
        self._ck(self.lib.mbx_fuse_bwd(_p(dh), _p(x_st), _p(x_ts), _p(alpha), _p(w), _p(d_st), _p(d_ts), _p(d_st_t), _p(d_ts_t),
                                       _p(dw), _p(db), M, Cc, _DT[d_st_t.dtype], _p(ws), self._stream()))

    def fuse_bwd_pair(self, dh_a, dh_b, x_st, x_ts, alpha, w, d_st_t, d_ts_t, dw, db):
        """fuse_bwd with the incoming gradient as the sum of two bf16 tensors (the two Blocks' input gradients of the level above)."""
        M, Cc = x_st.shape
        ws = self._ws(('fub', Cc), self.lib.mbx_fuse_bwd_ws, Cc, device=x_st.device)
        self._ck(self.lib.mbx_fuse_bwd_pair(_p(dh_a), _p(dh_b), _p(x_st), _p(x_ts), _p(alpha), _p(w), _p(d_st_t), _p(d_ts_t), _p(dw), _p(db), M, Cc,
                                            _p(ws), self._stream()))

    def average(self, x_st, x_ts, out):
        self._ck(self.lib.mbx_average(_p(x_st), _p(x_ts), _p(out), x_st.numel(), self._stream()))

    def average_bwd(self, dh, d_st, d_ts, d_st_t, d_ts_t):
        self._ck(self.lib.mbx_average_bwd(_p(dh), _p(d_st), _p(d_ts), _p(d_st_t), _p(d_ts_t), dh.numel(), _DT[d_st_t.dtype],
                                          self._stream()))

    # ------------------------------------------------------------------ tail
    def head_fwd(self, rep, w, b, out):
        M, R = rep.shape
        self._ck(self.lib.mbx_head_fwd(_p(rep), _p(w), _p(b), _p(out), M, R, w.shape[0], self._stream()))

    def head_bwd(self, dout, rep, w, dpre_t, dw, db):
        M, R = rep.shape
        D = w.shape[0]
        ws = self._ws(('hdb', R, D), self.lib.mbx_head_bwd_ws, R, D, device=rep.device)
        self._ck(self.lib.mbx_head_bwd(_p(dout), _p(rep), _p(w), _p(dpre_t), _p(dw), _p(db), M, R, D, _DT[dpre_t.dtype], _p(ws),
                                       self._stream()))

    def tanh_bwd(self, drep, rep, dpre_t):
        self._ck(self.lib.mbx_tanh_bwd(_p(drep), _p(rep), _p(dpre_t), rep.numel(), _DT[dpre_t.dtype], self._stream()))


    # ------------------------------------------------------------------ input stage
    def augment2d(self, x, y, noise, uniform_range, jitter_std, d2c, mask_ratio, mask_T_ratio, flags, seed):
        B, T, J, Cin = x.shape
        mean, std, weight = noise if noise is not None else (None, None, None)
        a, b, m, s = d2c
        self._ck(self.lib.mbx_augment2d(_p(x), _p(y), B, T, J, Cin, _p(mean), _p(std), _p(weight), float(uniform_range), float(jitter_std),
                                        float(a), float(b), float(m), float(s), float(mask_ratio), float(mask_T_ratio), int(flags),
                                        int(seed), self._stream()))

    def embed_fwd_tta(self, x, perm, w, b, pos, temp, h, B, T, J):
        self._ck(self.lib.mbx_embed_fwd_tta(_p(x), _p(perm), _p(w), _p(b), _p(pos), _p(temp), _p(h), B, T, J, x.shape[-1], h.shape[-1],
                                            self._stream()))

    def embed_fwd_ragged(self, x, w, b, pos, temp, frame_t, h, F, J):
        """embed_fwd for a ragged batch x [F,J,Din]: frame f takes the temporal row temp[frame_t[f]] (frame_t [F] i32 on the device)"""
        self._embed_ragged('embed_fwd_ragged', x, None, w, b, pos, temp, frame_t, h, F, J)

    def embed_fwd_tta_ragged(self, x, perm, w, b, pos, temp, frame_t, h, F, J):
        """embed_fwd_tta for a ragged batch: h [2 F J,C], rows F J .. are the flipped view with the same frame_t"""
        self._embed_ragged('embed_fwd_tta_ragged', x, perm, w, b, pos, temp, frame_t, h, F, J)

    def _embed_ragged(self, what, x, perm, w, b, pos, temp, frame_t, h, F, J):
        rows, C, dev = (1 if perm is None else 2) * F * J, h.shape[-1], x.device
        n_temp = temp.numel() // C
        self._dense(what, torch.float32, None, dev, w=w, b=b, pos=pos, temp=temp)
        self._dense(what, torch.float32, F * J * x.shape[-1], dev, x=x)
        self._dense(what, torch.float32, rows * C, dev, h=h)
        self._dense(what, torch.int32, F, dev, frame_t=frame_t)
        if perm is None:
            self._ck(self.lib.mbx_embed_fwd_ragged(_p(x), _p(w), _p(b), _p(pos), _p(temp), _p(frame_t), _p(h), F, J, x.shape[-1], C, n_temp,
                                                   self._stream()))
        else:
            self._dense(what, torch.int32, J, dev, perm=perm)
            self._ck(self.lib.mbx_embed_fwd_tta_ragged(_p(x), _p(perm), _p(w), _p(b), _p(pos), _p(temp), _p(frame_t), _p(h), F, J, x.shape[-1], C,
                                                       n_temp, self._stream()))

    def flip_average(self, out2, perm, out):
        B, T, J, D = out.shape
        self._ck(self.lib.mbx_flip_average(_p(out2), _p(perm), _p(out), B, T, J, D, self._stream()))

    # ------------------------------------------------------------------ evaluation (train.py:56-153)
    def pose_errors(self, pred, gt, hw, factor, x, rootrel, e1, e2):
        """pred, gt [N,T,J,3] f32; hw [N,2] / factor [N,T] f32 or None; x = the model input [N,T,J,>=2] (gt_2d) or None; e1, e2 [N,T] f64."""
        N, T, J, _ = pred.shape
        self._ck(self.lib.mbx_pose_errors(_p(pred), _p(gt), _p(hw), _p(factor), _p(x), 0 if x is None else x.shape[-1], int(bool(rootrel)),
                                          int(x is not None), _p(e1), _p(e2), N, T, J, self._stream()))

    def eval_reduce(self, e1, e2, row_ptr, slots, action, A, per_action, summary, count):
        F = action.numel()
        ws = self._ws(('evr', F, A), self.lib.mbx_eval_reduce_ws, F, A, device=e1.device)
        self._ck(self.lib.mbx_eval_reduce(_p(e1), _p(e2), e1.numel(), _p(row_ptr), row_ptr.numel(), _p(slots), slots.numel(), _p(action), F, int(A),
                                          _p(per_action), _p(summary), _p(count), _p(ws), self._stream()))

    # ------------------------------------------------------------------ one-shot recognition (train_action_1shot.py)
    @staticmethod
    def _dense(what, dtype, numel, dev, **tensors):
        """every named tensor (None allowed) is contiguous, of `dtype`, of `numel` elements (None: any) and on device `dev`: the kernels
        take raw pointers, so a strided view or a tensor of another size would be read or written with the wrong layout"""
        for name, t in tensors.items():
            if t is not None and (t.dtype != dtype or not t.is_contiguous() or t.device != dev or (numel is not None and t.numel() != numel)):
                raise RuntimeError(f'libmbx: {what}: {name} must be a contiguous {dtype} tensor' + (f' of {numel} elements' if numel is not None else '') +
                                   f' on {dev}, got {tuple(t.shape)} {t.dtype} strides {t.stride()} on {t.device}')

    def supcon_loss(self, feat, labels, temperature, base_temperature, normalize, loss, dfeat, grad_scale=1.0):
        """feat [bsz,n_views,D] f32, labels [bsz] i32, loss [1] f32, dfeat like feat or None; all contiguous, on the device of feat."""
        if feat.dim() != 3:
            raise RuntimeError(f'libmbx: supcon_loss needs feat [bsz,n_views,D], got {tuple(feat.shape)}')
        bsz, n_views, D = feat.shape
        self._dense('supcon_loss', torch.float32, bsz * n_views * D, feat.device, feat=feat, dfeat=dfeat)
        self._dense('supcon_loss', torch.float32, 1, feat.device, loss=loss)
        self._dense('supcon_loss', torch.int32, bsz, feat.device, labels=labels)
        A = bsz * n_views
        ws = self._ws(('supcon', A, D), self.lib.mbx_supcon_loss_ws, A, D, device=feat.device)
        self._ck(self.lib.mbx_supcon_loss(_p(feat), _p(labels), bsz, n_views, D, float(temperature), float(base_temperature),
                                          int(bool(normalize)), float(grad_scale), _p(loss), _p(dfeat), _p(ws), self._stream()))

    def nn_cosine(self, anchors, anchor_labels, test, test_labels, pred_label, best_sim, hits):
        """anchors [M,D] / test [N,D] f32, labels i32, pred_label [N] i32, best_sim [N] f32 or None, hits [1] i64 (accumulated); all
        contiguous, on the device of anchors."""
        if anchors.dim() != 2 or test.dim() != 2 or test.shape[1] != anchors.shape[1]:
            raise RuntimeError(f'libmbx: nn_cosine needs anchors [M,D] and test [N,D], got {tuple(anchors.shape)} / {tuple(test.shape)}')
        M, D = anchors.shape
        N = test.shape[0]
        dev = anchors.device
        self._dense('nn_cosine', torch.float32, None, dev, anchors=anchors, test=test)
        self._dense('nn_cosine', torch.float32, N, dev, best_sim=best_sim)
        self._dense('nn_cosine', torch.int32, M, dev, anchor_labels=anchor_labels)
        self._dense('nn_cosine', torch.int32, N, dev, pred_label=pred_label, test_labels=test_labels)
        self._dense('nn_cosine', torch.int64, 1, dev, hits=hits)
        if test_labels is not None and hits is None:
            raise RuntimeError('libmbx: nn_cosine: test labels without a hit counter')
        self._ck(self.lib.mbx_nn_cosine(_p(anchors), _p(anchor_labels), M, _p(test), _p(test_labels), N, D, _p(pred_label), _p(best_sim),
                                        _p(hits), self._stream()))

    # ------------------------------------------------------------------ action recognition (train_action.py, lib/data/dataset_action.py)
    def action_input(self, x, y, params_in, params_out, ranges, flags, seed):
        """x, y [N,M,T,J,3] f32; params_in / params_out [N,9] f32 or None; ranges = ((angle lo, hi), (scale ..), (translation ..), (crop ..));
        flags bit 0 move, bit 1 crop; all contiguous, on the device of x."""
        if x.dim() != 5 or x.shape[-1] != 3:
            raise RuntimeError(f'libmbx: action_input needs x [N,M,T,J,3], got {tuple(x.shape)}')
        N, M, T, J, _ = x.shape
        self._dense('action_input', torch.float32, x.numel(), x.device, x=x, y=y)
        self._dense('action_input', torch.float32, N * 9, x.device, params_in=params_in, params_out=params_out)
        (a0, a1), (s0, s1), (t0, t1), (c0, c1) = ranges
        self._ck(self.lib.mbx_action_input(_p(x), _p(y), N, M, T, J, _p(params_in), _p(params_out), float(a0), float(a1), float(s0), float(s1),
                                           float(t0), float(t1), float(c0), float(c1), int(flags), int(seed), self._stream()))

    def motion2d_input(self, x, data, gt, conf, x_aug, params_in, params_out, ratio_range, flip_prob, noise, uniform_range, jitter_std, d2c,
                       mask_ratio, mask_T_ratio, flags, seed):
        """x [N,T,J,3] f32; data / gt / x_aug like x, conf [N,T,J,1], each or None; params_in / params_out [N,2] f32 or None; noise = (mean,
        std, weight) or None; flags bit 0 crop, 1 zero unseen, 2 flip, 3 noise, 4 mask, 5 rootrel; all contiguous, on the device of x."""
        if x.dim() != 4 or x.shape[-1] != 3:
            raise RuntimeError(f'libmbx: motion2d_input needs x [N,T,J,3], got {tuple(x.shape)}')
        N, T, J, _ = x.shape
        self._dense('motion2d_input', torch.float32, x.numel(), x.device, x=x, data=data, gt=gt, x_aug=x_aug)
        self._dense('motion2d_input', torch.float32, N * T * J, x.device, conf=conf)
        self._dense('motion2d_input', torch.float32, N * 2, x.device, params_in=params_in, params_out=params_out)
        mean, std, weight = noise if noise is not None else (None, None, None)
        self._dense('motion2d_input', torch.float32, 2 * J, x.device, noise_mean=mean, noise_std=std)      # the kernel reads entry j of each
        self._dense('motion2d_input', torch.float32, J, x.device, noise_weight=weight)
        a, b, m, s = d2c
        self._ck(self.lib.mbx_motion2d_input(_p(x), _p(data), _p(gt), _p(conf), _p(x_aug), N, T, J, _p(params_in), _p(params_out),
                                             float(ratio_range[0]), float(ratio_range[1]), float(flip_prob), _p(mean), _p(std), _p(weight),
                                             float(uniform_range), float(jitter_std), float(a), float(b), float(m), float(s),
                                             float(mask_ratio), float(mask_T_ratio), int(flags), int(seed), self._stream()))

    # ------------------------------------------------------------------ AMASS joints (csrc/amass.hip; motionbert_amd/amass.py)
    def amass_joints(self, model, poses, betas, dmpls, trans, kp, camera=False, fma=False):
        """model: the folded SMPL-H dict of amass.SMPLHModel.tensors(): Jt [52,3], Jd [52,3,24], pairs [Np,2] i32, P [Np,3,484], s [Np],
        qs [K] f32 on the device of poses, parents (52 host ints); poses [F,156], betas [16] or [F,16], dmpls [F,8] or None, trans [F,3] or
        None, kp [F,K,3] f32; camera: the step of convert_amass.py in the launch; fma: the vector-unit product (measurement only)."""
        if poses.dim() != 2 or poses.shape[1] != 156:
            raise RuntimeError(f'libmbx: amass_joints needs poses [F,156], got {tuple(poses.shape)}')
        F, dev = poses.shape[0], poses.device
        pairs, P, qs = model['pairs'], model['P'], model['qs']
        Np, K = pairs.shape[0], qs.numel()
        if not 1 <= K <= 32 or Np > 17 * 52 or pairs.dim() != 2 or pairs.shape[1] != 2:
            raise RuntimeError(f'libmbx: amass_joints needs 1 <= K <= 32 joints and pairs [Np <= 884, 2], got K = {K}, pairs {tuple(pairs.shape)}')
        if betas.shape not in ((16,), (F, 16)):
            raise RuntimeError(f'libmbx: amass_joints needs betas [16] or [{F},16], got {tuple(betas.shape)}')
        self._dense('amass_joints', torch.float32, F * 156, dev, poses=poses)
        self._dense('amass_joints', torch.float32, None, dev, betas=betas)
        self._dense('amass_joints', torch.float32, F * 8, dev, dmpls=dmpls)
        self._dense('amass_joints', torch.float32, F * 3, dev, trans=trans)
        self._dense('amass_joints', torch.float32, F * K * 3, dev, kp=kp)
        self._dense('amass_joints', torch.float32, 156, dev, Jt=model['Jt'])
        self._dense('amass_joints', torch.float32, 156 * 24, dev, Jd=model['Jd'])
        self._dense('amass_joints', torch.int32, Np * 2, dev, pairs=pairs)
        self._dense('amass_joints', torch.float32, Np * 3 * 484, dev, P=P)
        self._dense('amass_joints', torch.float32, Np, dev, s=model['s'])
        self._dense('amass_joints', torch.float32, K, dev, qs=qs)
        parents = [int(p) for p in model['parents']]
        if len(parents) != 52:
            raise RuntimeError(f'libmbx: amass_joints needs 52 parents, got {len(parents)}')
        self._ck(self.lib.mbx_amass_joints(_p(poses), _p(betas), int(betas.dim() == 2), _p(dmpls), _p(trans), _p(model['Jt']), _p(model['Jd']),
                                           (C.c_int * 52)(*parents), _p(pairs), _p(P), _p(model['s']), _p(qs), Np, K,
                                           int(bool(camera)) | (2 if fma else 0), _p(kp), F, self._stream()))

    def xent_topk(self, logits, labels, values, dlogits, acc, grad_scale=1.0):
        """logits [N,C] f32, labels [N] i32, values [3] f32, dlogits like logits or None, acc [4] f64 (accumulated) or None; all contiguous, on
        the device of logits."""
        if logits.dim() != 2:
            raise RuntimeError(f'libmbx: xent_topk needs logits [N,C], got {tuple(logits.shape)}')
        N, Cc = logits.shape
        dev = logits.device
        self._dense('xent_topk', torch.float32, N * Cc, dev, logits=logits, dlogits=dlogits)
        self._dense('xent_topk', torch.float32, 3, dev, values=values)
        self._dense('xent_topk', torch.int32, N, dev, labels=labels)
        self._dense('xent_topk', torch.float64, 4, dev, acc=acc)
        self._ck(self.lib.mbx_xent_topk(_p(logits), _p(labels), N, Cc, float(grad_scale), _p(values), _p(dlogits), _p(acc), self._stream()))

    # ------------------------------------------------------------------ in-the-wild inference (infer_wild.py, lib/data/dataset_wild.py)
    def wild_input(self, kp, chunk_tab, seq_chunk_ptr, half_w, half_h, pix_scale, ratio, flags, y, box):
        """kp [F,26,3] f64; chunk_tab [n_chunks,3] / seq_chunk_ptr [S+1] i32 (motionbert_amd.wild.chunk_table); flags bit 0 pixel mode,
        bit 1 crop mode; y [F,17,2|3] f32; box [S,4] f64 or None; all contiguous, on the device of kp."""
        if kp.dim() != 3 or tuple(kp.shape[1:]) != (26, 3):
            raise RuntimeError(f'libmbx: wild_input needs kp [F,26,3], got {tuple(kp.shape)}')
        F, dev = kp.shape[0], kp.device
        if y.dim() != 3 or y.shape[0] != F or y.shape[1] != 17 or y.shape[2] not in (2, 3):
            raise RuntimeError(f'libmbx: wild_input needs y [{F},17,2|3], got {tuple(y.shape)}')
        if chunk_tab.dim() != 2 or chunk_tab.shape[1] != 3 or seq_chunk_ptr.dim() != 1 or seq_chunk_ptr.numel() < 2:
            raise RuntimeError(f'libmbx: wild_input needs chunk_tab [n_chunks,3] and seq_chunk_ptr [S+1], got {tuple(chunk_tab.shape)} / {tuple(seq_chunk_ptr.shape)}')
        S, n_chunks = seq_chunk_ptr.numel() - 1, chunk_tab.shape[0]
        self._dense('wild_input', torch.float64, F * 78, dev, kp=kp)
        self._dense('wild_input', torch.float32, F * 17 * y.shape[2], dev, y=y)
        self._dense('wild_input', torch.int32, None, dev, chunk_tab=chunk_tab, seq_chunk_ptr=seq_chunk_ptr)
        self._dense('wild_input', torch.float64, S * 4, dev, box=box)
        ws = self._ws(('wildin', F, S), self.lib.mbx_wild_input_ws, F, S, device=dev)
        self._ck(self.lib.mbx_wild_input(_p(kp), _p(chunk_tab), n_chunks, _p(seq_chunk_ptr), S, F, float(half_w), float(half_h), float(pix_scale),
                                         float(ratio), int(flags), y.shape[2], _p(y), _p(box), _p(ws), ws.numel(), self._stream()))

    def wild_output(self, pred, x, dst_frames, dst_max, flags, pix_scale, half_w, half_h, out):
        """pred [n,T,17,3] f32 (not modified); x [n,T,17,2|3] f32 or None (read with flags bit 1, gt_2d); dst_frames [n] i32 on the device
        with `dst_max` its largest entry (host int: the rows dst_max .. dst_max + T - 1 of out must exist, checked here); flags bit 0
        rootrel, bit 1 gt_2d, bit 2 pixel mode; out [F,17,3] f32."""
        if pred.dim() != 4 or tuple(pred.shape[2:]) != (17, 3) or pred.shape[1] < 1:
            raise RuntimeError(f'libmbx: wild_output needs pred [n,T >= 1,17,3], got {tuple(pred.shape)}')
        n, T = pred.shape[:2]
        dev = pred.device
        if out.dim() != 3 or tuple(out.shape[1:]) != (17, 3):
            raise RuntimeError(f'libmbx: wild_output needs out [F,17,3], got {tuple(out.shape)}')
        if n and not 0 <= int(dst_max) <= out.shape[0] - T:
            raise RuntimeError(f'libmbx: wild_output: a clip of {T} frames at row {int(dst_max)} does not fit out [{out.shape[0]},17,3]')
        xc = 0
        if x is not None:
            if x.dim() != 4 or tuple(x.shape[:3]) != (n, T, 17) or x.shape[3] not in (2, 3):
                raise RuntimeError(f'libmbx: wild_output needs x [{n},{T},17,2|3], got {tuple(x.shape)}')
            xc = x.shape[3]
        elif int(flags) & 2:
            raise RuntimeError('libmbx: wild_output: gt_2d needs the network input x')
        self._dense('wild_output', torch.float32, None, dev, pred=pred, x=x, out=out)
        self._dense('wild_output', torch.int32, n, dev, dst_frames=dst_frames)
        self._ck(self.lib.mbx_wild_output(_p(pred), _p(x), xc, _p(dst_frames), n, T, int(flags), float(pix_scale), float(half_w), float(half_h),
                                          _p(out), self._stream()))

    def wild_output_ragged(self, pred, x, frame_t, dst0, flags, pix_scale, half_w, half_h, out):
        """wild_output for one ragged batch: pred [Fb,17,3] f32 (not modified) goes to rows dst0 .. dst0 + Fb - 1 of out [F,17,3]; x
        [Fb,17,2|3] f32 or None (gt_2d); frame_t [Fb] i32 on the device = the index of each frame inside its clip (z of joint 0 is
        zeroed where it is 0, unless rootrel)."""
        if pred.dim() != 3 or tuple(pred.shape[1:]) != (17, 3):
            raise RuntimeError(f'libmbx: wild_output_ragged needs pred [Fb,17,3], got {tuple(pred.shape)}')
        Fb, dev = pred.shape[0], pred.device
        if out.dim() != 3 or tuple(out.shape[1:]) != (17, 3):
            raise RuntimeError(f'libmbx: wild_output_ragged needs out [F,17,3], got {tuple(out.shape)}')
        if not 0 <= int(dst0) <= out.shape[0] - Fb:
            raise RuntimeError(f'libmbx: wild_output_ragged: a batch of {Fb} frames at row {int(dst0)} does not fit out [{out.shape[0]},17,3]')
        xc = 0
        if x is not None:
            if x.dim() != 3 or tuple(x.shape[:2]) != (Fb, 17) or x.shape[2] not in (2, 3):
                raise RuntimeError(f'libmbx: wild_output_ragged needs x [{Fb},17,2|3], got {tuple(x.shape)}')
            xc = x.shape[2]
        elif int(flags) & 2:
            raise RuntimeError('libmbx: wild_output_ragged: gt_2d needs the network input x')
        self._dense('wild_output_ragged', torch.float32, None, dev, pred=pred, x=x, out=out)
        self._dense('wild_output_ragged', torch.int32, Fb, dev, frame_t=frame_t)
        self._ck(self.lib.mbx_wild_output_ragged(_p(pred), _p(x), xc, _p(frame_t), Fb, int(dst0), out.shape[0], int(flags), float(pix_scale),
                                                 float(half_w), float(half_h), _p(out), self._stream()))

    # ------------------------------------------------------------------ mesh recovery (train_mesh.py, lib/model/model_mesh.py, loss_mesh.py)
    def rot6d_theta_fwd(self, x6, rotmat, aa):
        """x6 [M,6] f32 -> rotmat [M,9] (or [M,3,3]) and aa [M,3] f32, either None; all contiguous, on the device of x6."""
        if x6.dim() != 2 or x6.shape[1] != 6 or (rotmat is None and aa is None):
            raise RuntimeError(f'libmbx: rot6d_theta_fwd needs x6 [M,6] and at least one output, got {tuple(x6.shape)}')
        M = x6.shape[0]
        self._dense('rot6d_theta_fwd', torch.float32, M * 6, x6.device, x6=x6)
        self._dense('rot6d_theta_fwd', torch.float32, M * 9, x6.device, rotmat=rotmat)
        self._dense('rot6d_theta_fwd', torch.float32, M * 3, x6.device, aa=aa)
        self._ck(self.lib.mbx_rot6d_theta_fwd(_p(x6), _p(rotmat), _p(aa), M, self._stream()))

    def rot6d_theta_bwd(self, x6, drotmat, daa, dx6):
        """dx6 [M,6] = the cotangents drotmat [M,9] / daa [M,3] (either None: zero) pulled back to x6 [M,6]."""
        if x6.dim() != 2 or x6.shape[1] != 6:
            raise RuntimeError(f'libmbx: rot6d_theta_bwd needs x6 [M,6], got {tuple(x6.shape)}')
        M = x6.shape[0]
        if dx6 is None or dx6.data_ptr() == x6.data_ptr() and M:
            raise RuntimeError('libmbx: rot6d_theta_bwd needs dx6, which must not alias x6')
        self._dense('rot6d_theta_bwd', torch.float32, M * 6, x6.device, x6=x6, dx6=dx6)
        self._dense('rot6d_theta_bwd', torch.float32, M * 9, x6.device, drotmat=drotmat)
        self._dense('rot6d_theta_bwd', torch.float32, M * 3, x6.device, daa=daa)
        self._ck(self.lib.mbx_rot6d_theta_bwd(_p(x6), _p(drotmat), _p(daa), _p(dx6), M, self._stream()))

    def mesh_param_loss(self, pred_theta, gt_theta, loss_type, lambdas3, losses, dtheta, grad_scale=1.0):
        """pred_theta, gt_theta [F,82] f32; loss_type 0 (MSE) / 1 (L1); lambdas3 = (lambda_pose, lambda_shape, lambda_norm);
        losses [4] f32 = [loss_pose, loss_shape, loss_norm, weighted sum]; dtheta like pred_theta or None."""
        if pred_theta.dim() != 2 or pred_theta.shape[1] != 82 or pred_theta.shape[0] < 1 or gt_theta.shape != pred_theta.shape or len(lambdas3) != 3:
            raise RuntimeError(f'libmbx: mesh_param_loss needs pred_theta, gt_theta [F >= 1, 82] and three lambdas, got {tuple(pred_theta.shape)} / '
                               f'{tuple(gt_theta.shape)} / {len(lambdas3)} lambdas')
        if int(loss_type) not in (0, 1):
            raise RuntimeError(f'libmbx: mesh_param_loss: loss_type {loss_type} (0 = MSE, 1 = L1)')
        F = pred_theta.shape[0]
        dev = pred_theta.device
        self._dense('mesh_param_loss', torch.float32, F * 82, dev, pred_theta=pred_theta, gt_theta=gt_theta, dtheta=dtheta)
        self._dense('mesh_param_loss', torch.float32, 4, dev, losses=losses)
        if losses is None:
            raise RuntimeError('libmbx: mesh_param_loss: losses [4] is required')
        ws = self._ws(('mpl', F), self.lib.mbx_mesh_param_loss_ws, F, device=dev)
        self._ck(self.lib.mbx_mesh_param_loss(_p(pred_theta), _p(gt_theta), int(loss_type), *[float(v) for v in lambdas3], float(grad_scale),
                                              _p(losses), _p(dtheta), F, _p(ws), self._stream()))

    def mesh_errors(self, verts_p, verts_g, kp_p, kp_g, err):
        """verts_p, verts_g [F,V,3] f32 (both None: the MPVE row is NaN), kp_p, kp_g [F,17,3] f32, err [5,F] f64 =
        [mpve, mpjpe_17j, mpjpe (14 joints), pa_mpjpe_17j, pa_mpjpe (14 joints)] per frame."""
        if kp_p.dim() != 3 or tuple(kp_p.shape[1:]) != (17, 3) or kp_g.shape != kp_p.shape:
            raise RuntimeError(f'libmbx: mesh_errors needs kp_p, kp_g [F,17,3], got {tuple(kp_p.shape)} / {tuple(kp_g.shape)}')
        F = kp_p.shape[0]
        dev = kp_p.device
        if (verts_p is None) != (verts_g is None):
            raise RuntimeError('libmbx: mesh_errors: verts_p and verts_g must both be given or both be None')
        V = 1
        if verts_p is not None:
            if verts_p.dim() != 3 or verts_p.shape[0] != F or verts_p.shape[2] != 3 or verts_p.shape[1] < 1 or verts_g.shape != verts_p.shape:
                raise RuntimeError(f'libmbx: mesh_errors needs verts_p, verts_g [{F},V >= 1,3], got {tuple(verts_p.shape)} / {tuple(verts_g.shape)}')
            V = verts_p.shape[1]
        self._dense('mesh_errors', torch.float32, F * 51, dev, kp_p=kp_p, kp_g=kp_g)
        self._dense('mesh_errors', torch.float32, F * V * 3, dev, verts_p=verts_p, verts_g=verts_g)
        self._dense('mesh_errors', torch.float64, 5 * F, dev, err=err)
        if err is None:
            raise RuntimeError('libmbx: mesh_errors: err [5,F] is required')
        self._ck(self.lib.mbx_mesh_errors(_p(verts_p), _p(verts_g), _p(kp_p), _p(kp_g), _p(err), F, V, self._stream()))

    # ------------------------------------------------------------------ SMPL body model (csrc/smpl.hip; motionbert_amd/smpl.py)
    def _smpl_model(self, what, m, need_packed):
        """m: dict of the model tensors (smpl.SMPLModel.tensors()): checked dense f32 on one device; returns (V, device, args) with args
        the model's arguments in ABI order: v_template, shapedirs, posedirs[, packed_t], Jt, Jd, parents (host), lbs_weights; Q, K follow"""
        vt = m['v_template']
        if vt.dim() != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
            raise RuntimeError(f'libmbx: {what} needs v_template [V >= 1, 3], got {tuple(vt.shape)}')
        V, dev = vt.shape[0], vt.device
        self._dense(what, torch.float32, V * 3, dev, v_template=vt)
        self._dense(what, torch.float32, V * 30, dev, shapedirs=m['shapedirs'])
        self._dense(what, torch.float32, 207 * 3 * V, dev, posedirs=m['posedirs'])
        self._dense(what, torch.float32, 72, dev, Jt=m['Jt'])
        self._dense(what, torch.float32, 720, dev, Jd=m['Jd'])
        self._dense(what, torch.float32, V * 24, dev, lbs_weights=m['lbs_weights'])
        if need_packed:
            if m.get('packed_t') is None:
                raise RuntimeError(f'libmbx: {what} needs packed_t [3V,224] (smpl_pack)')
            self._dense(what, torch.float32, 3 * V * 224, dev, packed_t=m['packed_t'])
        parents = [int(p) for p in m['parents']]
        if len(parents) != 24:
            raise RuntimeError(f'libmbx: {what} needs 24 parents, got {len(parents)}')
        packed = (_p(m['packed_t']),) if need_packed else ()
        return V, dev, (_p(vt), _p(m['shapedirs']), _p(m['posedirs']), *packed, _p(m['Jt']), _p(m['Jd']), (C.c_int * 24)(*parents),
                        _p(m['lbs_weights']))

    @staticmethod
    def _smpl_q(what, Q, V, need):
        """the regressor Q [1 <= K <= 32, V] checked; returns K (0 without Q).  need: True where the entry cannot do without Q, else the name of
        the argument that reads Q where that argument is given (false where it is not)"""
        if need is True and Q is None or Q is not None and (Q.dim() != 2 or Q.shape[1] != V or not 1 <= Q.shape[0] <= 32):
            raise RuntimeError(f'libmbx: {what} needs Q [1 <= K <= 32, {V}], got {None if Q is None else tuple(Q.shape)}')
        if need and Q is None:
            raise RuntimeError(f'libmbx: {what}: {need} needs the regressor Q')
        return 0 if Q is None else Q.shape[0]

    @staticmethod
    def _smpl_frames(what, betas, rotmat):
        if betas.dim() != 2 or betas.shape[1] != 10 or rotmat.dim() not in (3, 4) or rotmat.shape[0] != betas.shape[0] or rotmat.numel() != betas.shape[0] * 216:
            raise RuntimeError(f'libmbx: {what} needs betas [F,10] and rotmat [F,24,9] (or [F,24,3,3]), got {tuple(betas.shape)} / {tuple(rotmat.shape)}')
        return betas.shape[0]

    def smpl_pack(self, shapedirs, posedirs, packed_t):
        """packed_t [3V,224] f32 = [posedirs^T | shapedirs | 0] of shapedirs [V,3,10] and posedirs [207,3V]"""
        if shapedirs.dim() != 3 or tuple(shapedirs.shape[1:]) != (3, 10) or shapedirs.shape[0] < 1:
            raise RuntimeError(f'libmbx: smpl_pack needs shapedirs [V >= 1,3,10], got {tuple(shapedirs.shape)}')
        V, dev = shapedirs.shape[0], shapedirs.device
        self._dense('smpl_pack', torch.float32, V * 30, dev, shapedirs=shapedirs)
        self._dense('smpl_pack', torch.float32, 207 * 3 * V, dev, posedirs=posedirs)
        self._dense('smpl_pack', torch.float32, 3 * V * 224, dev, packed_t=packed_t)
        if posedirs is None or packed_t is None:
            raise RuntimeError('libmbx: smpl_pack: posedirs and packed_t are required')
        self._ck(self.lib.mbx_smpl_pack(_p(shapedirs), _p(posedirs), _p(packed_t), V, self._stream()))

    def smpl_fwd_ws(self, F, V, K, device):
        return self._ws(('smplf', F, V, K), self.lib.mbx_smpl_fwd_ws, F, V, K, device=device)

    def smpl_bwd_ws(self, F, V, K, device):
        return self._ws(('smplb', F, V, K), self.lib.mbx_smpl_bwd_ws, F, V, K, device=device)

    def smpl_fwd(self, model, Q, betas, rotmat, scale, verts, kp, joints, ws=None):
        """model: dict v_template [V,3], shapedirs [V,3,10], posedirs [207,3V], Jt [24,3], Jd [24,3,10], lbs_weights [V,24] f32 on the device
        and parents (24 host ints); Q [K,V] f32 or None; betas [F,10], rotmat [F,24,9] f32; outputs verts [F,V,3] / kp [F,K,3] /
        joints [F,24,3] f32, each may be None; ws: a uint8 workspace of smpl_fwd_ws(F, V, K with kp else 0) (allocated when None)."""
        V, dev, margs = self._smpl_model('smpl_fwd', model, False)
        F = self._smpl_frames('smpl_fwd', betas, rotmat)
        if verts is None and kp is None and joints is None:
            raise RuntimeError('libmbx: smpl_fwd: no output')
        K = self._smpl_q('smpl_fwd', Q, V, kp is not None and 'kp')
        self._dense('smpl_fwd', torch.float32, K * V, dev, Q=Q)
        self._dense('smpl_fwd', torch.float32, F * 10, dev, betas=betas)
        self._dense('smpl_fwd', torch.float32, F * 216, dev, rotmat=rotmat)
        self._dense('smpl_fwd', torch.float32, F * V * 3, dev, verts=verts)
        self._dense('smpl_fwd', torch.float32, F * K * 3, dev, kp=kp)
        self._dense('smpl_fwd', torch.float32, F * 72, dev, joints=joints)
        if ws is None:
            ws = self.smpl_fwd_ws(F, V, K if kp is not None else 0, dev)
        self._dense('smpl_fwd', torch.uint8, None, dev, ws=ws)
        self._ck(self.lib.mbx_smpl_fwd(*margs, _p(Q), K, _p(betas), _p(rotmat), float(scale), _p(verts), _p(kp), _p(joints), F, V, _p(ws),
                                       ws.numel(), self._stream()))

    def smpl_bwd(self, model, Q, betas, rotmat, scale, dverts, dkp, djoints, drotmat, dbetas, ws=None):
        """the cotangents dverts [F,V,3] / dkp [F,K,3] / djoints [F,24,3] (each may be None: zero) pulled back to drotmat [F,24,9] and
        dbetas [F,10]; model as smpl_fwd plus packed_t [3V,224]."""
        V, dev, margs = self._smpl_model('smpl_bwd', model, True)
        F = self._smpl_frames('smpl_bwd', betas, rotmat)
        K = self._smpl_q('smpl_bwd', Q, V, dkp is not None and 'dkp')
        if drotmat is None or dbetas is None:
            raise RuntimeError('libmbx: smpl_bwd: drotmat and dbetas are required')
        self._dense('smpl_bwd', torch.float32, K * V, dev, Q=Q)
        self._dense('smpl_bwd', torch.float32, F * 10, dev, betas=betas, dbetas=dbetas)
        self._dense('smpl_bwd', torch.float32, F * 216, dev, rotmat=rotmat, drotmat=drotmat)
        self._dense('smpl_bwd', torch.float32, F * V * 3, dev, dverts=dverts)
        self._dense('smpl_bwd', torch.float32, F * K * 3, dev, dkp=dkp)
        self._dense('smpl_bwd', torch.float32, F * 72, dev, djoints=djoints)
        if ws is None:
            ws = self.smpl_bwd_ws(F, V, K, dev)
        self._dense('smpl_bwd', torch.uint8, None, dev, ws=ws)
        self._ck(self.lib.mbx_smpl_bwd(*margs, _p(Q), K, _p(betas), _p(rotmat), float(scale), _p(dverts), _p(dkp), _p(djoints), _p(drotmat),
                                       _p(dbetas), F, V, _p(ws), ws.numel(), self._stream()))

    # ------------------------------------------------------------------ mesh targets (csrc/smpl.hip; motionbert_amd/mesh.py: mesh_targets)
    def mesh_gt_ws(self, F, V, K, device):
        return self._ws(('meshgt', F, V, K), self.lib.mbx_mesh_gt_ws, F, V, K, device=device)

    def mesh_gt(self, model, Q, pose, shape, motion_2d, flips, seed, flip_prob, scale, x2d, theta, kp_3d, verts, flips_used, ws=None):
        """model, Q [K,V] as smpl_fwd takes them; pose [N,T,72], shape [N,T,10] f32, motion_2d [N,T,17,3] f32 or None; flips [N] u8 or None
        (then the flag of clip n is drawn from (seed, n) against flip_prob); outputs x2d [N,T,17,3] / theta [N,T,82] / kp_3d [N,T,K,3] /
        verts [N,T,V,3] f32 and flips_used [N] u8, each may be None; ws: a uint8 workspace of mesh_gt_ws(N T, V, K) (allocated when None)."""
        V, dev, margs = self._smpl_model('mesh_gt', model, False)
        if pose.dim() != 3 or pose.shape[2] != 72 or pose.shape[1] < 1 or tuple(shape.shape) != tuple(pose.shape[:2]) + (10,):
            raise RuntimeError(f'libmbx: mesh_gt needs pose [N,T >= 1,72] and shape [N,T,10], got {tuple(pose.shape)} / {tuple(shape.shape)}')
        N, T = pose.shape[:2]
        F = N * T
        if x2d is None and theta is None and kp_3d is None and verts is None and flips_used is None:
            raise RuntimeError('libmbx: mesh_gt: no output')
        K = self._smpl_q('mesh_gt', Q, V, True)
        if x2d is not None and motion_2d is None:
            raise RuntimeError('libmbx: mesh_gt: x2d needs motion_2d')
        self._dense('mesh_gt', torch.float32, K * V, dev, Q=Q)
        self._dense('mesh_gt', torch.float32, F * 72, dev, pose=pose)
        self._dense('mesh_gt', torch.float32, F * 10, dev, shape=shape)
        self._dense('mesh_gt', torch.float32, F * 51, dev, motion_2d=motion_2d, x2d=x2d)
        self._dense('mesh_gt', torch.float32, F * 82, dev, theta=theta)
        self._dense('mesh_gt', torch.float32, F * K * 3, dev, kp_3d=kp_3d)
        self._dense('mesh_gt', torch.float32, F * V * 3, dev, verts=verts)
        self._dense('mesh_gt', torch.uint8, N, dev, flips=flips, flips_used=flips_used)
        if ws is None:
            ws = self.mesh_gt_ws(F, V, K, dev)
        self._dense('mesh_gt', torch.uint8, None, dev, ws=ws)
        self._ck(self.lib.mbx_mesh_gt(_p(pose), _p(shape), _p(motion_2d), _p(flips), int(seed), float(flip_prob), *margs, _p(Q), K, float(scale),
                                      _p(x2d), _p(theta), _p(kp_3d), _p(verts), _p(flips_used), N, T, V, _p(ws), ws.numel(), self._stream()))

    # ------------------------------------------------------------------ in-the-wild mesh recovery (infer_wild_mesh.py; csrc/smpl.hip, csrc/wild.hip)
    def wild_mesh_ws(self, nT, V, K, pair, device):
        return self._ws(('wildmesh', nT, V, K, bool(pair)), self.lib.mbx_wild_mesh_ws, nT, V, K, int(bool(pair)), device=device)

    def wild_mesh(self, model, Q, rotmat_a, betas_a, theta_a, theta_b, scale, dst_frames, dst_max, T, verts, kp, theta, ws=None):
        """model, Q [K,V] as smpl_fwd takes them; pass A: rotmat_a [nT,24,9] (or [nT,24,3,3]), betas_a [nT,10], theta_a [nT,82] or None;
        pass B: theta_b [nT,82] or None (single-pass mode); dst_frames [n] i32 on the device with nT = n T, dst_max its largest entry (host);
        outputs verts [F,V,3] / kp [F,K,3] / theta [F,82] f32, each may be None; ws: a uint8 workspace of wild_mesh_ws (allocated when
        None)."""
        V, dev, margs = self._smpl_model('wild_mesh', model, False)
        nT = self._smpl_frames('wild_mesh', betas_a, rotmat_a)
        T = int(T)
        n = dst_frames.numel()
        if T < 1 or n * T != nT:
            raise RuntimeError(f'libmbx: wild_mesh: {n} clips of {T} frames, but parameters of {nT} frames')
        if verts is None and kp is None and theta is None:
            raise RuntimeError('libmbx: wild_mesh: no output')
        F = (verts if verts is not None else kp if kp is not None else theta).shape[0]
        K = self._smpl_q('wild_mesh', Q, V, kp is not None and 'kp')
        if theta is not None and theta_a is None:
            raise RuntimeError('libmbx: wild_mesh: theta needs theta_a')
        if n and not 0 <= int(dst_max) <= F - T:
            raise RuntimeError(f'libmbx: wild_mesh: a clip of {T} frames at row {int(dst_max)} does not fit the {F} rows of the result')
        self._dense('wild_mesh', torch.float32, K * V, dev, Q=Q)
        self._dense('wild_mesh', torch.float32, nT * 10, dev, betas_a=betas_a)
        self._dense('wild_mesh', torch.float32, nT * 216, dev, rotmat_a=rotmat_a)
        self._dense('wild_mesh', torch.float32, nT * 82, dev, theta_a=theta_a, theta_b=theta_b)
        self._dense('wild_mesh', torch.float32, F * V * 3, dev, verts=verts)
        self._dense('wild_mesh', torch.float32, F * K * 3, dev, kp=kp)
        self._dense('wild_mesh', torch.float32, F * 82, dev, theta=theta)
        self._dense('wild_mesh', torch.int32, n, dev, dst_frames=dst_frames)
        if not n:
            return
        pair = theta_b is not None
        if ws is None:
            ws = self.wild_mesh_ws(nT, V, K if kp is not None else 0, pair, dev)
        self._dense('wild_mesh', torch.uint8, None, dev, ws=ws)
        self._ck(self.lib.mbx_wild_mesh(*margs, _p(Q), K, _p(rotmat_a), _p(betas_a), _p(theta_a), _p(theta_b), float(scale), _p(dst_frames),
                                        int(dst_max), n, T, F, _p(verts), _p(kp), _p(theta), V, _p(ws), ws.numel(), self._stream()))

    def scale_fit(self, ref, kp, seq_ptr, fit):
        """ref [F,17,3] f64, kp [F,17,3] f32, seq_ptr [S+1] i32 -> fit [S,6] f64 = scale, t [3], objective, iterations (< 0: a status)"""
        if ref.dim() != 3 or tuple(ref.shape[1:]) != (17, 3) or tuple(kp.shape) != tuple(ref.shape):
            raise RuntimeError(f'libmbx: scale_fit needs ref and kp [F,17,3], got {tuple(ref.shape)} / {tuple(kp.shape)}')
        F, S, dev = ref.shape[0], seq_ptr.numel() - 1, fit.device
        if S < 0 or tuple(fit.shape) != (S, 6):
            raise RuntimeError(f'libmbx: scale_fit needs seq_ptr [S+1] and fit [S,6], got {tuple(seq_ptr.shape)} / {tuple(fit.shape)}')
        self._dense('scale_fit', torch.float64, F * 51, dev, ref=ref)
        self._dense('scale_fit', torch.float32, F * 51, dev, kp=kp)
        self._dense('scale_fit', torch.int32, S + 1, dev, seq_ptr=seq_ptr)
        self._dense('scale_fit', torch.float64, S * 6, dev, fit=fit)
        self._ck(self.lib.mbx_scale_fit(_p(ref), _p(kp), _p(seq_ptr), S, F, _p(fit), self._stream()))

    def wild_mesh_place(self, verts, kp, ref, seq_ptr, fit):
        """verts [F,V,3] f32 in place, kp [F,K,3] f32, ref [F,17,3] f64, seq_ptr [S+1] i32, fit [S,6] f64"""
        if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] < 1 or kp.dim() != 3 or kp.shape[0] != verts.shape[0] or kp.shape[2] != 3 \
                or not 1 <= kp.shape[1] <= 32 or tuple(ref.shape) != (verts.shape[0], 17, 3):
            raise RuntimeError(f'libmbx: wild_mesh_place needs verts [F,V,3], kp [F,K,3] and ref [F,17,3], got {tuple(verts.shape)} / '
                               f'{tuple(kp.shape)} / {tuple(ref.shape)}')
        F, V, K, S, dev = verts.shape[0], verts.shape[1], kp.shape[1], seq_ptr.numel() - 1, verts.device
        if S < 0 or tuple(fit.shape) != (S, 6):
            raise RuntimeError(f'libmbx: wild_mesh_place needs seq_ptr [S+1] and fit [S,6], got {tuple(seq_ptr.shape)} / {tuple(fit.shape)}')
        self._dense('wild_mesh_place', torch.float32, F * V * 3, dev, verts=verts)
        self._dense('wild_mesh_place', torch.float32, F * K * 3, dev, kp=kp)
        self._dense('wild_mesh_place', torch.float64, F * 51, dev, ref=ref)
        self._dense('wild_mesh_place', torch.int32, S + 1, dev, seq_ptr=seq_ptr)
        self._dense('wild_mesh_place', torch.float64, S * 6, dev, fit=fit)
        self._ck(self.lib.mbx_wild_mesh_place(_p(verts), _p(kp), K, _p(ref), _p(seq_ptr), S, _p(fit), F, V, self._stream()))

    # ------------------------------------------------------------------ mesh video frames (motionbert_amd/render.py)
    def render_project(self, verts, cube, seq_ptr, size, ss, out):
        """verts [F,V,3] f32, cube [n_tracks,4] f32, seq_ptr [n_tracks+1] i32 -> out [F,V,3] i32 (mbx_render_project)"""
        if verts.dim() != 3 or verts.shape[2] != 3 or cube.dim() != 2 or cube.shape[1] != 4 or cube.shape[0] < 1:
            raise RuntimeError(f'libmbx: render_project needs verts [F,V,3] and cube [n_tracks,4], got {tuple(verts.shape)} / {tuple(cube.shape)}')
        F, V, n_tracks, dev = verts.shape[0], verts.shape[1], cube.shape[0], verts.device
        self._dense('render_project', torch.float32, F * V * 3, dev, verts=verts)
        self._dense('render_project', torch.float32, n_tracks * 4, dev, cube=cube)
        self._dense('render_project', torch.int32, n_tracks + 1, dev, seq_ptr=seq_ptr)
        self._dense('render_project', torch.int32, F * V * 3, dev, out=out)
        self._ck(self.lib.mbx_render_project(_p(verts), _p(cube), _p(seq_ptr), n_tracks, F, V, int(size), int(ss), _p(out), self._stream()))

    def render_raster(self, vq, verts, faces, size, ss, color, alpha, rgb, face_id=None, depth=None):
        """vq [F,V,3] i32, verts [F,V,3] f32, faces [Nf,3] i32 -> rgb [F,size,size,3] u8, face_id / depth [F,S,S] i32 or None
        (mbx_render_raster)"""
        if vq.dim() != 3 or vq.shape[2] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise RuntimeError(f'libmbx: render_raster needs vq [F,V,3] and faces [Nf,3], got {tuple(vq.shape)} / {tuple(faces.shape)}')
        F, V, Nf, dev, S = vq.shape[0], vq.shape[1], faces.shape[0], vq.device, int(size) * int(ss)
        self._dense('render_raster', torch.int32, F * V * 3, dev, vq=vq)
        self._dense('render_raster', torch.float32, F * V * 3, dev, verts=verts)
        self._dense('render_raster', torch.int32, Nf * 3, dev, faces=faces)
        self._dense('render_raster', torch.uint8, F * int(size) * int(size) * 3, dev, rgb=rgb)
        self._dense('render_raster', torch.int32, F * S * S, dev, face_id=face_id, depth=depth)
        ws = self._ws(('render', F, Nf), self.lib.mbx_render_raster_ws, F, Nf, device=dev)
        self._ck(self.lib.mbx_render_raster(_p(vq), _p(verts), _p(faces), F, V, Nf, int(size), int(ss), float(color[0]), float(color[1]),
                                            float(color[2]), float(alpha), _p(rgb), _p(face_id), _p(depth), _p(ws), ws.numel(), self._stream()))

    # ------------------------------------------------------------------ skeleton video frames (motionbert_amd/render.py)
    def skeleton_project(self, x, view, size, ss, jq):
        """x [F,J,3] f32 on the device, view: 15 float64 values on the host (rows 0, 1, 3 of M, u_lo, v_hi, inv_w) -> jq [F,J,2] i32
        (mbx_skeleton_project)"""
        if x.dim() != 3 or x.shape[2] != 3 or len(view) != 15:
            raise RuntimeError(f'libmbx: skeleton_project needs x [F,J,3] and a view of 15 values, got {tuple(x.shape)} / {len(view)}')
        F, J, dev = x.shape[0], x.shape[1], x.device
        self._dense('skeleton_project', torch.float32, F * J * 3, dev, x=x)
        self._dense('skeleton_project', torch.int32, F * J * 2, dev, jq=jq)
        self._ck(self.lib.mbx_skeleton_project(_p(x), (C.c_double * 15)(*[float(v) for v in view]), F, J, int(size), int(ss), _p(jq), self._stream()))

    def skeleton_raster(self, jq, bones, colors, radii, size, ss, rgb, prim_id=None):
        """jq [F,J,2] i32, bones [Nb,2] i32, colors [Nb,3] u8, radii = (r_line, r_out, r_in) in 1/16 sample -> rgb [F,size,size,3] u8,
        prim_id [F,S,S] i32 or None (mbx_skeleton_raster)"""
        if jq.dim() != 3 or jq.shape[2] != 2 or bones.dim() != 2 or bones.shape[1] != 2 or len(radii) != 3:
            raise RuntimeError(f'libmbx: skeleton_raster needs jq [F,J,2], bones [Nb,2] and three radii, got {tuple(jq.shape)} / {tuple(bones.shape)} / {radii!r}')
        F, J, Nb, dev, S = jq.shape[0], jq.shape[1], bones.shape[0], jq.device, int(size) * int(ss)
        self._dense('skeleton_raster', torch.int32, F * J * 2, dev, jq=jq)
        self._dense('skeleton_raster', torch.int32, Nb * 2, dev, bones=bones)
        self._dense('skeleton_raster', torch.uint8, Nb * 3, dev, colors=colors)
        self._dense('skeleton_raster', torch.uint8, F * int(size) * int(size) * 3, dev, rgb=rgb)
        self._dense('skeleton_raster', torch.int32, F * S * S, dev, prim_id=prim_id)
        self._ck(self.lib.mbx_skeleton_raster(_p(jq), _p(bones), _p(colors), F, J, Nb, int(radii[0]), int(radii[1]), int(radii[2]), int(size), int(ss),
                                              _p(rgb), _p(prim_id), self._stream()))

    # ------------------------------------------------------------------ crowd video frames (motionbert_amd/render.py)
    def scene_project(self, x, ss, jq):
        """x [R,J,2|3] f32 on the device, in video pixels -> jq [R,J,2] i32 (mbx_scene_project)"""
        if x.dim() != 3 or x.shape[2] not in (2, 3):
            raise RuntimeError(f'libmbx: scene_project needs x [R,J,2|3], got {tuple(x.shape)}')
        R, J, C_, dev = x.shape[0], x.shape[1], x.shape[2], x.device
        self._dense('scene_project', torch.float32, R * J * C_, dev, x=x)
        self._dense('scene_project', torch.int32, R * J * 2, dev, jq=jq)
        self._ck(self.lib.mbx_scene_project(_p(x), R, J, C_, int(ss), _p(jq), self._stream()))

    def scene_raster(self, jq, frame_ptr, rows, person, bones, palette, radii, width, height, ss, background, rgb, prim_id=None):
        """jq [R,J,2] i32, the scene table (frame_ptr [Fv+1], rows [n], person [n], i32), bones [Nb,2] i32, palette [P,Nb,3] u8, radii = (r_line,
        r_out, r_in), background: three ints or u8 frames [Fv or 1,H,W,3] -> rgb [Fv,H,W,3] u8, prim_id [Fv, H ss, W ss] i32 or None
        (mbx_scene_raster)"""
        if (jq.dim() != 3 or jq.shape[2] != 2 or bones.dim() != 2 or bones.shape[1] != 2 or palette.dim() != 3 or palette.shape[1:] != (bones.shape[0], 3)
                or frame_ptr.dim() != 1 or frame_ptr.numel() < 1 or rows.dim() != 1 or len(radii) != 3):
            raise RuntimeError(f'libmbx: scene_raster needs jq [R,J,2], frame_ptr [Fv+1], rows [n], bones [Nb,2], palette [P,Nb,3] and three radii, got '
                               f'{tuple(jq.shape)} / {tuple(frame_ptr.shape)} / {tuple(rows.shape)} / {tuple(bones.shape)} / {tuple(palette.shape)} / {radii!r}')
        R, J, Nb, P, Fv, n, dev = jq.shape[0], jq.shape[1], bones.shape[0], palette.shape[0], frame_ptr.numel() - 1, rows.numel(), jq.device
        W, H, ss = int(width), int(height), int(ss)
        self._dense('scene_raster', torch.int32, R * J * 2, dev, jq=jq)
        self._dense('scene_raster', torch.int32, Fv + 1, dev, frame_ptr=frame_ptr)
        self._dense('scene_raster', torch.int32, n, dev, rows=rows, person=person)
        self._dense('scene_raster', torch.int32, Nb * 2, dev, bones=bones)
        self._dense('scene_raster', torch.uint8, P * Nb * 3, dev, palette=palette)
        self._dense('scene_raster', torch.uint8, Fv * H * W * 3, dev, rgb=rgb)
        self._dense('scene_raster', torch.int32, Fv * H * ss * W * ss, dev, prim_id=prim_id)
        if isinstance(background, torch.Tensor):
            if background.dim() != 4 or background.shape[0] not in (1, Fv):
                raise RuntimeError(f'libmbx: scene_raster: background frames must be [{Fv} or 1,{H},{W},3], got {tuple(background.shape)}')
            bg_n, bg_rgb = background.shape[0], 0
            self._dense('scene_raster', torch.uint8, bg_n * H * W * 3, dev, background=background)
        else:
            r, g, b = (int(c) for c in background)
            if not all(0 <= c <= 255 for c in (r, g, b)):
                raise RuntimeError(f'libmbx: scene_raster: a background colour is three values in [0, 255], got {background!r}')
            background, bg_n, bg_rgb = None, 1, r | g << 8 | b << 16
        self._ck(self.lib.mbx_scene_raster(_p(jq), _p(frame_ptr), _p(rows), _p(person), n, _p(bones), _p(palette), Fv, R, J, Nb, P, int(radii[0]),
                                           int(radii[1]), int(radii[2]), W, H, ss, _p(background), bg_n, bg_rgb, _p(rgb), _p(prim_id), self._stream()))

    # ------------------------------------------------------------------ video files (motionbert_amd/video.py)
    @staticmethod
    def _jpeg_blocks(H, W, sub):
        m = 16 if sub else 8
        return -(-H // m) * -(-W // m) * (6 if sub else 3)

    def jpeg_ws(self, F, H, W, sub, restart, device):
        """the workspace that jpeg_sizes fills and jpeg_emit reads (mbx_jpeg_entropy_ws)"""
        return self._ws(('jpeg', F, H, W, sub, restart), self.lib.mbx_jpeg_entropy_ws, F, H, W, int(sub), int(restart), device=device)

    def jpeg_blocks(self, rgb, quality, sub, coef):
        """rgb [F,H,W,3] u8 -> coef [F, n_mcu, blocks per MCU, 64] i16, quantised, zigzag (mbx_jpeg_blocks)"""
        if rgb.dim() != 4 or rgb.shape[3] != 3:
            raise RuntimeError(f'libmbx: jpeg_blocks needs rgb [F,H,W,3], got {tuple(rgb.shape)}')
        F, H, W, dev = rgb.shape[0], rgb.shape[1], rgb.shape[2], rgb.device
        self._dense('jpeg_blocks', torch.uint8, F * H * W * 3, dev, rgb=rgb)
        self._dense('jpeg_blocks', torch.int16, F * self._jpeg_blocks(H, W, sub) * 64, dev, coef=coef)
        self._ck(self.lib.mbx_jpeg_blocks(_p(rgb), F, H, W, int(quality), int(sub), _p(coef), self._stream()))

    def jpeg_sizes(self, coef, H, W, sub, quality, restart, offsets, ws):
        """coef [F, ...] i16 -> offsets [F+1] i64 on the device: where every file will lie (mbx_jpeg_entropy_sizes); no host read"""
        F, dev = coef.shape[0], coef.device
        self._dense('jpeg_sizes', torch.int16, F * self._jpeg_blocks(H, W, sub) * 64, dev, coef=coef)
        self._dense('jpeg_sizes', torch.int64, F + 1, dev, offsets=offsets)
        self._dense('jpeg_sizes', torch.uint8, None, dev, ws=ws)
        self._ck(self.lib.mbx_jpeg_entropy_sizes(_p(coef), F, int(H), int(W), int(sub), int(quality), int(restart), _p(offsets), _p(ws), ws.numel(),
                                                 self._stream()))

    def jpeg_emit(self, coef, H, W, sub, quality, restart, offsets, data, ws):
        """the files themselves into data [offsets[F]] u8, with the coef, parameters and ws of jpeg_sizes (mbx_jpeg_entropy)"""
        F, dev = coef.shape[0], coef.device
        self._dense('jpeg_emit', torch.int16, F * self._jpeg_blocks(H, W, sub) * 64, dev, coef=coef)
        self._dense('jpeg_emit', torch.int64, F + 1, dev, offsets=offsets)
        self._dense('jpeg_emit', torch.uint8, None, dev, data=data, ws=ws)
        self._ck(self.lib.mbx_jpeg_entropy(_p(coef), F, int(H), int(W), int(sub), int(quality), int(restart), _p(offsets), _p(data), data.numel(),
                                           _p(ws), ws.numel(), self._stream()))

    # ------------------------------------------------------------------ reading video (motionbert_amd/video.py)
    JPEG_DEC_TABLE_WORDS = 228

    @staticmethod
    def _jpeg_dec_blocks(H, W, sub):
        h, v = (1, 1) if sub == 0 else (2, 2) if sub == 1 else (2, 1)
        return -(-H // (8 * v)) * -(-W // (8 * h)) * (h * v + 2)

    def jpeg_dec_tables(self, dht):
        """(bits [16], vals [256]) of the DC and AC table of each component, uint8 [6,272] on the host, or None for Annex K -> the decode
        tables as a host int32 tensor [6, 228] (mbx_jpeg_dec_tables); a set that is no Huffman table raises ValueError"""
        out = np.zeros((6, self.JPEG_DEC_TABLE_WORDS), np.uint32)
        if dht is not None:
            dht = np.ascontiguousarray(dht, np.uint8)
            if dht.shape != (6, 272):
                raise RuntimeError(f'libmbx: jpeg_dec_tables needs uint8 [6,272], got {dht.shape}')
        if self.lib.mbx_jpeg_dec_tables(None if dht is None else dht.ctypes.data, out.ctypes.data) != 0:
            raise ValueError('libmbx: ' + self.lib.mbx_last_error().decode())
        return torch.from_numpy(out.view(np.int32))

    def jpeg_dec_ws(self, F, H, W, sub, device):
        """the component planes mbx_jpeg_dec_pixels writes between its two launches (mbx_jpeg_dec_ws)"""
        return self._ws(('jpeg_dec', F, H, W, sub), self.lib.mbx_jpeg_dec_ws, F, H, W, int(sub), device=device)

    def jpeg_dec_index(self, data, scans, n_int, pos, status):
        """data u8 [n], scans i64 [F,2] -> pos i64 [F, n_int + 1], status i32 [F, n_int] (mbx_jpeg_dec_index)"""
        F, dev = scans.shape[0], data.device
        self._dense('jpeg_dec_index', torch.uint8, None, dev, data=data)
        self._dense('jpeg_dec_index', torch.int64, F * 2, dev, scans=scans)
        self._dense('jpeg_dec_index', torch.int64, F * (n_int + 1), dev, pos=pos)
        self._dense('jpeg_dec_index', torch.int32, F * n_int, dev, status=status)
        self._ck(self.lib.mbx_jpeg_dec_index(_p(data), data.numel(), _p(scans), F, int(n_int), _p(pos), _p(status), self._stream()))

    def jpeg_dec_entropy(self, data, pos, tables, H, W, sub, restart, coef, status):
        """the restart intervals pos names -> coef i16 [F, n_mcu, blocks per MCU, 64], zigzag, and status (mbx_jpeg_dec_entropy)"""
        F, dev = coef.shape[0], data.device
        n_mcu = self._jpeg_dec_blocks(H, W, sub) // (3 if sub == 0 else 6 if sub == 1 else 4)
        n_int = -(-n_mcu // restart) if restart else 1
        self._dense('jpeg_dec_entropy', torch.uint8, None, dev, data=data)
        self._dense('jpeg_dec_entropy', torch.int64, F * (n_int + 1), dev, pos=pos)
        self._dense('jpeg_dec_entropy', torch.int32, 6 * self.JPEG_DEC_TABLE_WORDS, dev, tables=tables)
        self._dense('jpeg_dec_entropy', torch.int16, F * self._jpeg_dec_blocks(H, W, sub) * 64, dev, coef=coef)
        self._dense('jpeg_dec_entropy', torch.int32, F * n_int, dev, status=status)
        self._ck(self.lib.mbx_jpeg_dec_entropy(_p(data), data.numel(), _p(pos), _p(tables), F, int(H), int(W), int(sub), int(restart), _p(coef),
                                               _p(status), self._stream()))

    JPEG_SYNC_MAX_BYTES = 1 << 27

    def jpeg_dec_sync_ws(self, F, n_int, max_interval_bytes, device):
        """the lane states, chunk exits and sums of jpeg_dec_entropy_sync (mbx_jpeg_dec_sync_ws)"""
        if not 0 <= int(max_interval_bytes) <= self.JPEG_SYNC_MAX_BYTES:
            raise RuntimeError(f'libmbx: jpeg_dec_sync_ws: max_interval_bytes {max_interval_bytes} (0 .. {self.JPEG_SYNC_MAX_BYTES})')
        n = int(self.lib.mbx_jpeg_dec_sync_ws(int(F), int(n_int), int(max_interval_bytes)))   # not cached: the longest scan differs in every call
        return torch.empty(max(n, 16), dtype=torch.uint8, device=device)

    def jpeg_dec_entropy_sync(self, data, pos, tables, H, W, sub, restart, max_interval_bytes, coef, status, route, ws):
        """jpeg_dec_entropy with many lanes per interval: the same coef and status, and route i32 [F, n_int]: 0 where the interval was
        decoded in parallel, else why the one-lane body decoded it (mbx_jpeg_dec_entropy_sync)"""
        F, dev = coef.shape[0], data.device
        n_mcu = self._jpeg_dec_blocks(H, W, sub) // (3 if sub == 0 else 6 if sub == 1 else 4)
        n_int = -(-n_mcu // restart) if restart else 1
        self._dense('jpeg_dec_entropy_sync', torch.uint8, None, dev, data=data, ws=ws)
        self._dense('jpeg_dec_entropy_sync', torch.int64, F * (n_int + 1), dev, pos=pos)
        self._dense('jpeg_dec_entropy_sync', torch.int32, 6 * self.JPEG_DEC_TABLE_WORDS, dev, tables=tables)
        self._dense('jpeg_dec_entropy_sync', torch.int16, F * self._jpeg_dec_blocks(H, W, sub) * 64, dev, coef=coef)
        self._dense('jpeg_dec_entropy_sync', torch.int32, F * n_int, dev, status=status, route=route)
        self._ck(self.lib.mbx_jpeg_dec_entropy_sync(_p(data), data.numel(), _p(pos), _p(tables), F, int(H), int(W), int(sub), int(restart),
                                                    int(max_interval_bytes), _p(coef), _p(status), _p(route), _p(ws), ws.numel(), self._stream()))

    def jpeg_dec_pixels(self, coef, q, H, W, sub, rgb, ws):
        """coef, q (uint8 [3,64] on the host: each component's table, zigzag order) -> rgb u8 [F,H,W,3] (mbx_jpeg_dec_pixels)"""
        F, dev = coef.shape[0], coef.device
        q = np.ascontiguousarray(q, np.uint8)
        if q.shape != (3, 64):
            raise RuntimeError(f'libmbx: jpeg_dec_pixels needs q uint8 [3,64], got {q.shape}')
        self._dense('jpeg_dec_pixels', torch.int16, F * self._jpeg_dec_blocks(H, W, sub) * 64, dev, coef=coef)
        self._dense('jpeg_dec_pixels', torch.uint8, F * H * W * 3, dev, rgb=rgb)
        self._dense('jpeg_dec_pixels', torch.uint8, None, dev, ws=ws)
        self._ck(self.lib.mbx_jpeg_dec_pixels(_p(coef), q.ctypes.data, F, int(H), int(W), int(sub), _p(rgb), _p(ws), ws.numel(), self._stream()))

    # ------------------------------------------------------------------ dropout / drop-path
    def dropout(self, x, y, p, seed):
        self._ck(self.lib.mbx_dropout(_p(x), _p(y), x.numel(), float(p), int(seed), _DT[x.dtype], self._stream()))

    def residual_drop(self, y, x, rows_per_sample, p, seed, p_path, seed_path):
        rows, Cc = y.shape
        self._ck(self.lib.mbx_residual_drop(_p(y), _p(x), rows, Cc, int(rows_per_sample), float(p), int(seed), float(p_path),
                                            int(seed_path), self._stream()))

    def grad_drop(self, dy, dy_t, rows_per_sample, p, seed, p_path, seed_path):
        rows, Cc = dy.shape
        self._ck(self.lib.mbx_grad_drop(_p(dy), _p(dy_t), rows, Cc, int(rows_per_sample), float(p), int(seed), float(p_path),
                                        int(seed_path), _DT[dy_t.dtype], self._stream()))

    # ------------------------------------------------------------------ ActionNet pooling
    def pool_rep_fwd(self, rep, pooled, N, Mp, T, J, p=0.0, seed=0):
        self._ck(self.lib.mbx_pool_rep_fwd(_p(rep), _p(pooled), N, Mp, T, J, rep.shape[-1], float(p), int(seed), self._stream()))

    def tanh_pool_bwd(self, dpooled, rep, dpre_t, N, Mp, T, J, p=0.0, seed=0):
        self._ck(self.lib.mbx_tanh_pool_bwd(_p(dpooled), _p(rep), _p(dpre_t), N, Mp, T, J, rep.shape[-1], float(p), int(seed),
                                            _DT[dpre_t.dtype], self._stream()))

    # ------------------------------------------------------------------ training step
    def pose_loss(self, pred, gt, lambda_scale, lambda_velocity, losses, dpred, grad_scale=1.0):
        B, T, J, D = pred.shape
        if D != 3 or gt.shape != pred.shape:
            raise RuntimeError(f'libmbx: pose_loss needs pred, gt [B,T,J,3], got {tuple(pred.shape)} / {tuple(gt.shape)}')
        ws = self._ws(('pl', B, T), self.lib.mbx_pose_loss_ws, B, T, device=pred.device)
        self._ck(self.lib.mbx_pose_loss(_p(pred), _p(gt), float(lambda_scale), float(lambda_velocity), _p(losses), _p(dpred),
                                        float(grad_scale), B, T, J, _p(ws), self._stream()))

    def pose_loss_full(self, pred, gt, lambdas6, losses, dpred, grad_scale=1.0):
        """lambdas6 = (lambda_scale, lambda_velocity, lambda_lv, lambda_lg, lambda_a, lambda_av); losses [8] =
        [mpjpe, n_mpjpe, velocity, lv, lg, angle, angle_velocity, total]; dpred [B,T,17,3] or None."""
        B, T, J, D = pred.shape
        if D != 3 or gt.shape != pred.shape or len(lambdas6) != 6:
            raise RuntimeError(f'libmbx: pose_loss_full needs pred, gt [B,T,17,3] and six lambdas, got {tuple(pred.shape)} / {tuple(gt.shape)} / '
                               f'{len(lambdas6)} lambdas')
        ws = self._ws(('plf', B, T), self.lib.mbx_pose_loss_full_ws, B, T, device=pred.device)
        self._ck(self.lib.mbx_pose_loss_full(_p(pred), _p(gt), *[float(v) for v in lambdas6], _p(losses), _p(dpred), float(grad_scale),
                                             B, T, J, _p(ws), self._stream()))

    def loss_2d_weighted(self, pred, target, conf, loss, dpred, grad_scale=1.0):
        """pred [B,T,J,3]; target [B,T,J,>=2] (x, y first) and conf [B,T,J] or [B,T,J,1] may be strided VIEWS of one [B,T,J,3]
        2D batch (target = batch, conf = batch[..., 2]): only their last-dimension element stride is passed down."""
        B, T, J, D = pred.shape
        if D != 3 or tuple(target.shape[:3]) != (B, T, J) or target.shape[-1] < 2 or conf.numel() != B * T * J:
            raise RuntimeError(f'libmbx: loss_2d_weighted needs pred [B,T,J,3], target [B,T,J,>=2], conf [B,T,J(,1)], got '
                               f'{tuple(pred.shape)} / {tuple(target.shape)} / {tuple(conf.shape)}')
        cf = conf.reshape(B, T, J) if conf.dim() == 4 else conf
        ts, cs = target.stride(2), cf.stride(2)
        if (target.stride(3) != 1 or target.stride(1) != J * ts or target.stride(0) != T * J * ts or
                cf.stride(1) != J * cs or cf.stride(0) != T * J * cs or target.dtype != torch.float32 or cf.dtype != torch.float32):
            raise RuntimeError('libmbx: loss_2d_weighted: target / conf must be fp32 and dense over (B, T, J) with a constant per-joint stride')
        ws = self._ws(('l2d', B, T), self.lib.mbx_loss_2d_weighted_ws, B, T, device=pred.device)
        self._ck(self.lib.mbx_loss_2d_weighted(_p(pred), _p(target), int(ts), _p(cf), int(cs), _p(loss), _p(dpred), float(grad_scale),
                                               B, T, J, _p(ws), self._stream()))

    def adamw_step(self, p, g, m, v, state, beta1, beta2, eps, weight_decay, tick=True):
        self._ck(self.lib.mbx_adamw_step(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(state), float(beta1), float(beta2), float(eps),
                                         float(weight_decay), int(bool(tick)), self._stream()))


_OPS: Optional[HipOps] = None
_OPS_LOCK = threading.Lock()


def get() -> HipOps:
    """Process-wide HipOps instance; raises if libmbx.so is missing (no fallback)."""
    global _OPS
    if _OPS is None:
        with _OPS_LOCK:
            if _OPS is None:
                _OPS = HipOps()
    return _OPS


def provider(ops, where: str, *tensors, move: str = 'the tensors'):
    """The kernel provider of a task-layer call made as `where` (its full dotted name): an injected `ops` as it is (it decides where
    its tensors live); otherwise the process-wide instance, once every tensor is on the ROCm device.  The check comes first: a host
    tensor raises without loading libmbx.so."""
    if ops is not None:
        return ops
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f'{where} runs on the ROCm device (move {move} first); there is no CPU path')
    return get()


def model_device(model, where: str) -> torch.device:
    """The ROCm device of `model`'s first parameter, for a drop-in evaluation called as `where`; a model on the host, or one without
    parameters, raises."""
    p = next(iter(model.parameters()), None) if hasattr(model, 'parameters') else None
    if p is None or not p.is_cuda:
        raise RuntimeError(f'{where} runs on the ROCm device (move the model first); there is no CPU path')
    return p.device


def evaluator_provider(ops, device, where: str):
    """`(ops, device)` of an evaluator's constructor: an injected `ops` with `device` (default: the host); otherwise the process-wide
    instance with a ROCm `device` (default: the current one)."""
    if ops is not None:
        return ops, torch.device('cpu' if device is None else device)
    device = None if device is None else torch.device(device)
    if not torch.cuda.is_available() or (device is not None and device.type != 'cuda'):
        raise RuntimeError(f'{where} runs on the ROCm device; there is no CPU path')
    return get(), torch.device('cuda', torch.cuda.current_device()) if device is None else device


def peek() -> Optional[HipOps]:
    """The process-wide instance if one has been created, else None (never loads the library: model.train() on a CPU box)."""
    return _OPS
