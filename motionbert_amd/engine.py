"""Host-side sequencing of the DSTformer hot path over the HIP kernel set.

This module owns no arithmetic.  It walks the dual-stream block structure of
the reference model (`lib/model/DSTformer.py:329-358` forward, `:239-249`
Block) and issues one call per kernel on an `ops` object whose methods map
1:1 onto the C-ABI entry points declared in `include/mbx.h`.  The product
`ops` is `motionbert_amd.hip_ops.HipOps` (ctypes -> libmbx.so -> gfx950
kernels); there is no CPU implementation in the package.

Data layout in HBM (all row-major, token index m = (b*T + t)*J + j):
  residual stream   [M, C]  fp32   one fresh buffer per sub-layer output
  GEMM operands     [M, K]  T      T = compute dtype (bf16 or fp32)
  qkv               [M, 3C] T      channel order [3][H][hd]  (DSTformer.py:143)
  attention out     [M, C]  T      heads concatenated head-major
  softmax stats     [M, H]  fp32   log-sum-exp per (token, head)
  LN stats          [M]     fp32   mean, rstd
The temporal attention reads its (b, j, h) sequences straight out of the
[B, T, J, 3C] qkv tensor with a row stride of J*3C elements: the three
permute->contiguous copies of `DSTformer.py:190-192` do not exist here.

What is saved for backward (per sub-layer).  Folded sequencing (bf16 default): the plain normalisation xhat (T), rstd, and
qkv / o / lse (attention) or the pre-/post-GELU hidden (MLP); the fp32 sub-layer input is NOT kept.  Plain sequencing (fp32-class
modes, dropout): the fp32 input, LN mean / rstd, the normalised T-typed GEMM input and the same.  Attention probabilities are never
stored: the backward kernels recompute them from q, k and lse.

No-grad sequencing (bf16, `rawln`): nothing is saved, and inside a Block no LayerNorm pass, no bf16 copy of the residual stream and
no hidden tensor exist.  Both consumers of a LayerNorm read the fp32 rows of the residual stream themselves, round them to the bf16
operand and take the row statistics from the same loads: the attention's qkv Linear as a row-owner GEMM that applies the LayerNorm
as row constants in its epilogue (mbx_rows_gemm_nk_ln), the MLP as ONE kernel (mbx_mlp_fused_fwd).  4 launches per sub-layer pair
(qkv, attention, proj + residual, MLP) instead of 7.
"""
from __future__ import annotations

import functools
from collections import namedtuple
from dataclasses import dataclass
from typing import Any, ClassVar, Dict, List, Optional

import os

import torch

# GEMM epilogues (values mirror enum mbx_epilogue in include/mbx.h)
EPI_STORE = 0      # out_t  = acc + bias                      (T)
EPI_GELU = 1       # out_t  = acc + bias ; out2_t = gelu(out) (T, T)
EPI_RESID = 2      # out_f  = resid + acc + bias              (fp32)
EPI_TANH = 3       # out_f  = tanh(acc + bias)                (fp32)
EPI_DGELU = 4      # out_t  = acc * gelu'(aux_t)              (T)

MODE_SPATIAL = 0
MODE_TEMPORAL = 1


@dataclass(frozen=True)
class ModelCfg:
    dim_in: int
    dim_out: int
    C: int          # dim_feat
    R: int          # dim_rep
    depth: int
    H: int
    hidden: int
    J: int
    maxlen: int
    eps: float
    scale: float
    att_fuse: bool
    qkv_bias: bool
    drop: float = 0.0            # drop_rate: pos_drop, proj_drop, both MLP drops (DSTformer.py:77,104,278)
    attn_drop: float = 0.0       # attn_drop_rate: on the attention probabilities (DSTformer.py:96)
    dpr: tuple = ()              # DropPath rate per level, linspace(0, drop_path_rate, depth) (DSTformer.py:279)

    @property
    def hd(self) -> int:
        return self.C // self.H


@dataclass(frozen=True)
class Switches:
    """The A/B switches of the sequencing: one `MBX_*` environment variable each, every one ON by default.
    They are read ONCE, when this module is imported (`SWITCHES`); a test or a tool that flips one afterwards calls
    `reload_switches()` (or patches `engine.SWITCHES` with `Switches.from_env({...})`).  What each one selects is described where
    it is decided: in `_plan` (the scheduling ones, dual_stream and x3_planes, in `Engine.__init__`)."""
    x3_planes: bool       # MBX_X3_PLANES      bf16x3: producers write the operand planes themselves (0: every operand through mbx_split_bf16)
    dual_stream: bool     # MBX_DUAL_STREAM    the ts Block of a level on a second HIP stream
    fold_ln: bool         # MBX_FOLD_LN        LayerNorm folded into the Linear it feeds (bf16)
    grad_stream: bool     # MBX_GRAD_STREAM    gradient of the residual stream in the operand type between sub-layers
    rows_lnbwd: bool      # MBX_ROWS_LNBWD     row-owner LayerNorm-backward GEMM
    rows_resid_ln: bool   # MBX_ROWS_RESID_LN  row-owner residual GEMM + next LayerNorm
    block_grad_t: bool    # MBX_BLOCK_GRAD_T   ... and across Block boundaries
    gelu_d: bool          # MBX_GELU_D         fc1 saves gelu'(u) instead of u
    rawln: bool           # MBX_RAWLN          no-grad sequencing (raw-operand LayerNorm + fused MLP)
    proj_mlp: bool        # MBX_PROJ_MLP       no-grad: proj + residual inside the MLP kernel

    _ENV: ClassVar[tuple] = (('x3_planes', 'MBX_X3_PLANES', '1'), ('dual_stream', 'MBX_DUAL_STREAM', '1'),
            ('fold_ln', 'MBX_FOLD_LN', '1'), ('grad_stream', 'MBX_GRAD_STREAM', '1'),
            ('rows_lnbwd', 'MBX_ROWS_LNBWD', '1'), ('rows_resid_ln', 'MBX_ROWS_RESID_LN', '1'), ('block_grad_t', 'MBX_BLOCK_GRAD_T', '1'),
            ('gelu_d', 'MBX_GELU_D', '1'), ('rawln', 'MBX_RAWLN', '1'), ('proj_mlp', 'MBX_PROJ_MLP', '1'))

    @classmethod
    def from_env(cls, env=None) -> 'Switches':
        env = os.environ if env is None else env
        return cls(**{field: env.get(var, default) == '1' for field, var, default in cls._ENV})


SWITCHES = Switches.from_env()


def reload_switches(env=None) -> Switches:
    """Re-read the MBX_* switches (tests and A/B tools that change the environment after import)."""
    global SWITCHES
    SWITCHES = Switches.from_env(env)
    return SWITCHES


# sub-layer order of the two Block flavours (DSTformer.py:240-249)
ORDER = {
    'st': (('attn', 'norm1_s', 'attn_s', MODE_SPATIAL), ('mlp', 'norm2_s', 'mlp_s', None),
           ('attn', 'norm1_t', 'attn_t', MODE_TEMPORAL), ('mlp', 'norm2_t', 'mlp_t', None)),
    'ts': (('attn', 'norm1_t', 'attn_t', MODE_TEMPORAL), ('mlp', 'norm2_t', 'mlp_t', None),
           ('attn', 'norm1_s', 'attn_s', MODE_SPATIAL), ('mlp', 'norm2_s', 'mlp_s', None)),
}


STREAMS = (('blocks_st', 'st'), ('blocks_ts', 'ts'))      # (module list, Block flavour) of the two streams
LINEARS = {'attn': ('qkv', 'proj'), 'mlp': ('fc1', 'fc2')}      # (Linear-in, Linear-out) of a sub-layer


def sublayers(cfg: ModelCfg):
    """(prefix, level, sub, typ, norm, mod, mode) of every sub-layer in execution order: stream by stream, level by level, ORDER."""
    for stream, kind in STREAMS:
        for i in range(cfg.depth):
            for sub, (typ, norm, mod, mode) in enumerate(ORDER[kind]):
                yield f'{stream}.{i}', i, sub, typ, norm, mod, mode


def linear_names(cfg: ModelCfg) -> List[str]:
    """Every nn.Linear whose weight runs through the MFMA GEMM (prefix without '.weight')."""
    names = []
    for pre, _, sub, *_ in sublayers(cfg):
        if sub == 0:      # per Block in this order, whatever its flavour: the flat gradient layout follows it
            for mod in ('attn_s', 'attn_t', 'mlp_s', 'mlp_t'):
                names += [f'{pre}.{mod}.{lin}' for lin in LINEARS[mod[:-2]]]
    return names + ['pre_logits.fc']


def folded_pairs(cfg: ModelCfg) -> List[tuple]:
    """(linear, norm) pairs whose LayerNorm is folded into the Linear it feeds (bf16 path): every norm1 -> qkv and norm2 -> fc1
    of every Block (DSTformer.py:241-249).  The final `norm` -> pre_logits.fc keeps the plain kernels."""
    pairs = []
    for pre, _, sub, *_ in sublayers(cfg):
        if sub == 0:      # per Block the spatial pairs first, whatever its flavour: the descriptor tables follow this order
            for mod, norm in (('attn_s', 'norm1_s'), ('mlp_s', 'norm2_s'), ('attn_t', 'norm1_t'), ('mlp_t', 'norm2_t')):
                pairs.append((f'{pre}.{mod}.{LINEARS[mod[:-2]][0]}', f'{pre}.{norm}'))
    return pairs


def grad_bucket(name: str, depth: int) -> int:
    """Bucket of a parameter in backward completion order: tail first, then the levels from the
    last to the first, the embedding last.  The flat gradient buffer is laid out bucket by bucket."""
    if name.startswith(('head.', 'pre_logits.', 'norm.')):
        return 0
    if name.startswith(('blocks_st.', 'blocks_ts.', 'ts_attn.')):
        return depth - int(name.split('.')[1])
    return depth + 1


# The N-resident row-owner kernels (gemm_rows_n.hip) address every tensor as a wave-uniform 64-bit base plus ONE unsigned 32-bit byte
# offset per lane, so each of their [M, .] tensors has to stay below this many bytes.  The C entries refuse more (mbx_rows_lnbwd_t,
# mbx_rows_resid_ln); the same limits are restated here -- once -- because the choice of the sequencing is made per forward, BEFORE
# anything runs: a refusal in backward would come after the forward has dropped what the tile kernels need.  tests/test_row_limits.py
# pins both functions to the library's checks at the boundary.
ROW_OFFSET_LIMIT = 1 << 32


def rows_lnbwd_fits(M: int, N: int, K: int) -> bool:
    """mbx_rows_lnbwd_t takes M rows: xhat / dres / dx_t bf16 [M, N] and dy bf16 [M, K] inside the 32-bit offsets."""
    return M * N * 2 < ROW_OFFSET_LIMIT and M * K * 2 < ROW_OFFSET_LIMIT


def rows_resid_ln_fits(M: int, N: int, K: int) -> bool:
    """mbx_rows_resid_ln takes M rows: resid / y fp32 [M, N] and a bf16 [M, K] inside the 32-bit offsets."""
    return M * N * 4 < ROW_OFFSET_LIMIT and M * K * 2 < ROW_OFFSET_LIMIT


@dataclass(frozen=True)
class Caps:
    """What a pass may use: every A/B switch ANDed with the provider's capability, as the engine holds them when the pass is prepared
    (`Engine.__init__`; model.py lowers fold / gelu_d / recompute afterwards)."""
    fold: bool = False             # LayerNorm folded into the Linear it feeds: bf16 without dropout only (Engine.__init__)
    x3: bool = False               # precision bf16x3 (the plain weights then come as operand planes)
    recompute: bool = False        # low-memory mode
    gelu_d: bool = False           # fc1 may save gelu'(u)
    grad_stream: bool = False      # gradient of the residual stream in the operand type
    rows_lnbwd: bool = False       # mbx_rows_lnbwd_t
    rows_resid_ln: bool = False    # mbx_rows_resid_ln
    block_grad_t: bool = False     # ... and the operand-typed gradient across Block boundaries
    proj_mlp: bool = False         # mbx_proj_mlp_fused_fwd
    fuse_ln: bool = False          # mbx_fuse_ln_fwd


class SubPlan(namedtuple('SubPlan', 'lin_in lin_out front save tail')):
    """One sub-layer of the plan.
    lin_in   'ln'    tile GEMM on the output of a LayerNorm (its own, or the one that came with x from its producer)
             'raw'   row-owner GEMM / fused MLP straight from the fp32 rows (no-grad sequencing)
    lin_out  'tile'  proj / fc2 as a tile GEMM with the residual epilogue
             'rows'  mbx_rows_resid_ln: residual GEMM + the plain normalisation for the next sub-layer
             'deferred'  the proj is left to the MLP kernel that follows;  'fused'  the MLP is one kernel (`front`: the proj it runs first)
    save     what an MLP keeps for GELU': 'u' the pre-activation, 'd' the derivative itself (None: attention, no backward)
    tail     backward from the Linear-in's output gradient: 'plain' (dX GEMM + LayerNorm backward), 'fold' (tile dX GEMM with the folded
             LayerNorm backward as its epilogue, row dots from the core) or 'rows' (mbx_rows_lnbwd_t; no row dots).  The FIRST sub-layer
             of a Block is only eligible for 'rows': it takes it when its caller wants the operand-typed gradient alone and adds nothing."""


@dataclass(frozen=True)
class Plan:
    """Which kernel serves every sub-layer of one pass: decided once (`plan_pass`), read by every sequencing method."""
    fold: bool              # folded sequencing (else plain: fp32-class modes, dropout)
    gstream: bool           # backward: the gradient of the residual stream travels in the operand type inside a Block
    sub: Dict[tuple, SubPlan]      # (block prefix, sub) -> SubPlan
    out_t: tuple            # per level: the Blocks hand their input gradients down operand-typed, as a pair
    embed_norm: bool        # the embedding's rows come with ONE plain normalisation for both Blocks of level 0
    fuse_norm: tuple        # per level, what the fusion kernel normalises: None, 'xhat' (one plain normalisation for both Blocks of the
                            # next level), 'pair' (their two LayerNorms) or 'norm' (the final one)
    pack_f: tuple           # proj / fc2 in the fragment order of mbx_rows_resid_ln           (lin_out 'rows')
    pack_n: tuple           # transposed folded qkv / fc1 in the order of mbx_rows_lnbwd_t    (tail 'rows')
    pack_k: tuple           # no-grad: ('mlp', module, proj in front or None) / ('qkv', Linear, None) in packing order
    formats: tuple          # everything above that selects a prepared-weight format (key of the weight cache)


def plan_pass(cfg: ModelCfg, caps: Caps, M: int, need_grad: bool, rawln: bool) -> Plan:
    """The plan of a pass over M rows: a pure function of its arguments (and of ROW_OFFSET_LIMIT)."""
    return _plan(cfg, caps, M, need_grad, rawln, ROW_OFFSET_LIMIT)


@functools.lru_cache(maxsize=64)      # (building it takes ~65 us at depth 5, 3 % of a one-clip no-grad forward; a hit under 1 us)
def _plan(cfg, caps, M, need_grad, rawln, _limit):
    # The folded sequencing (round 3, bf16 path; include/mbx.h "LayerNorm folded into the Linear it feeds"): the LayerNorm kernels write
    # the plain normalisation xhat, the affine part lives in the qkv / fc1 weights, and the LayerNorm BACKWARD runs as the epilogue of the
    # dX GEMM -- 40 LayerNorm-backward launches and the saved fp32 sub-layer inputs disappear.  Never with dropout (the masks sit between
    # the producer and the row dots) nor in the fp32-class modes (bf16 kernels only): the engine grants `caps.fold` only without them, so
    # NOTHING below asks about dropout or bf16x3 -- every folded, row-owner or no-grad entry implies that there is neither.
    fold = caps.fold
    rawln = rawln and fold
    # Gradient residual stream in the operand type BETWEEN the four sub-layers of a Block (round 4; fp32 arithmetic in the kernels): the
    # folded LayerNorm-backward GEMM reads its dres as bf16 and writes ONLY the bf16 dx, which is the stream and the next GEMMs' operand
    # at once -- 4 instead of 12 bytes per element and launch.  Numerics: tools/gradstream_numerics.py / profiles/r04_gradstream_numerics.txt.
    gstream = fold and caps.grad_stream
    # The row-owner kernels serve a bounded row count (ROW_OFFSET_LIMIT): whether they run is a matter of THIS pass's M and of the longest
    # contraction each of them meets -- dX of qkv: 3 C, dX of fc1 and fc2 itself: hidden.  Beyond it the tile kernels run, in forward and
    # backward alike, exactly as with the A/B switch off.
    # Round 5, backward: inside a Block (bf16 gradient stream in and out, no second summand) the folded LayerNorm backward is the epilogue
    # of a row-owner GEMM that takes both row means from its own accumulators (mbx_rows_lnbwd_t): the producers of dY -- attention
    # backward, the GELU' GEMM -- run WITHOUT their row dots there, and no row-constant launch is needed.
    lnbwd_rows = need_grad and gstream and caps.rows_lnbwd and rows_lnbwd_fits(M, cfg.C, max(3 * cfg.C, cfg.hidden))
    # ... and ACROSS Block boundaries: the first sub-layer of a Block then takes the row-owner tail too (no row dots, no row constants,
    # bf16 out), and the fusion backward of the level below (the embedding backward below level 0) reads the two Blocks' input gradients
    # as a bf16 pair and adds them (same bytes as one fp32 tensor).  Numerics: profiles/r05_boundary_numerics.txt.  Otherwise a Block's
    # input gradient leaves in fp32 with the other stream's gradient added: the tile kernel's epilogue.
    first_rows = lnbwd_rows and caps.block_grad_t and cfg.att_fuse
    # Round 5, forward: the residual GEMM (proj / fc2) of a sub-layer that is followed by a LayerNorm runs on the same row-owner shape
    # and leaves the plain normalisation of its output rows with them (mbx_rows_resid_ln): three of the four LayerNorm launches of a
    # Block -- each a second read of the fp32 rows -- disappear.  Folded sequencing only (the kernel writes xhat, not gamma xhat + beta);
    # the fourth sub-layer feeds the fusion, not a LayerNorm.
    resid_rows = fold and not rawln and caps.rows_resid_ln and rows_resid_ln_fits(M, cfg.C, max(cfg.C, cfg.hidden))
    sub, pack_f, pack_k, rows_in = {}, [], [], set()
    for stream, kind in STREAMS:
        order = ORDER[kind]
        for i in range(cfg.depth):
            pre, front = f'{stream}.{i}', None
            for s, (typ, _, mod, _) in enumerate(order):
                if rawln and typ == 'attn':
                    # no-grad: proj + residual run inside the MLP kernel that follows the attention in its Block
                    defer = caps.proj_mlp and s + 1 < len(order) and order[s + 1][0] == 'mlp'
                    front = f'{pre}.{mod}.proj' if defer else None
                    sp = SubPlan('raw', 'deferred' if defer else 'tile', None, None, None)
                elif rawln:
                    sp, front = SubPlan('raw', 'fused', front, None, None), None
                    pack_k.append(('mlp', f'{pre}.{mod}', sp.front))
                else:
                    tail = None if not need_grad else 'plain' if not fold else 'rows' if lnbwd_rows and (s > 0 or first_rows) else 'fold'
                    # Round 5: where the row-owner tail takes the row means, the GELU' epilogue no longer has to
                    # produce the dot of du with the pre-activation: fc1's forward epilogue saves gelu'(u) -- from the fp32 accumulator
                    # -- INSTEAD of u (same bytes) and the backward epilogue is one multiply (mbx_gemm_nt_gelu_d / mbx_gemm_nt_mul).
                    # Never for a first sub-layer, whose tail still depends on its caller; recompute rebuilds g from u.
                    save = None if typ == 'attn' or not need_grad else 'd' if tail == 'rows' and s > 0 and caps.gelu_d and not caps.recompute else 'u'
                    sp = SubPlan('ln', 'rows' if resid_rows and s + 1 < len(order) else 'tile', None, save, tail)
                sub[pre, s] = sp
                if sp.lin_out == 'rows':
                    pack_f.append(f'{pre}.{mod}.{LINEARS[typ][1]}')
                if sp.tail == 'rows':
                    rows_in.add(f'{pre}.{mod}.{LINEARS[typ][0]}')
            if rawln:      # the Block is complete: its two qkv
                pack_k += [('qkv', f'{pre}.{a}.qkv', None) for a in ('attn_s', 'attn_t')]
    out_t = tuple(all(sub[f'{stream}.{i}', 0].tail == 'rows' for stream, _ in STREAMS) for i in range(cfg.depth))
    # the fusion kernel also normalises its output for its consumers: the first LayerNorm of both Blocks of the next level (folded: ONE
    # plain normalisation, no gamma / beta, serves both) or the final `norm`; no-grad: the next level's consumers read the fp32 rows
    fuse_norm = tuple(None if not (cfg.att_fuse and caps.fuse_ln) else 'norm' if i + 1 == cfg.depth else None if rawln else
                      'xhat' if fold else 'pair' for i in range(cfg.depth))
    pack_f, pack_k = tuple(pack_f), tuple(pack_k)
    pack_n = tuple(lin for lin, _ in folded_pairs(cfg) if lin in rows_in)
    # folded: both Blocks of a level read the SAME plain normalisation of h (their gamma / beta live in their own weights) -- one launch
    # for level 0 too, or none where the embedding kernel normalises its own rows
    return Plan(fold=fold, gstream=gstream, sub=sub, out_t=out_t, embed_norm=fold and not rawln, fuse_norm=fuse_norm,
                pack_f=pack_f, pack_n=pack_n, pack_k=pack_k, formats=(fold, caps.x3, pack_f, pack_k))


class Drops(namedtuple('Drops', 'p seed_branch seed_act p_path seed_path p_attn seed_attn')):
    """Active dropout of one sub-layer (`Engine._drops`): rates and mask seeds of proj_drop / the MLP drops (on the branch output, after
    the activation), of DropPath and of the dropout on the attention probabilities."""
    branch = property(lambda d: d.p > 0 or d.p_path > 0)      # dropout or DropPath on the branch output (DSTformer.py:84,148-149,241-242)
    attn = property(lambda d: (d.p_attn, d.seed_attn) if d.p_attn > 0 else None)      # `drop` of the attention kernels (mask applied inside)


class Engine:
    """One forward (and optionally backward) pass.  `P` maps reference state_dict
    names to fp32 device tensors; `Wn[name]` / `Wt[name]` are the T-typed [N,K]
    and transposed [K,N] copies produced by ops.prep_weights."""

    _side_streams: Dict[int, Any] = {}

    def __init__(self, ops, cfg: ModelCfg, P: Dict[str, torch.Tensor], tdtype: torch.dtype, x3: bool = False, drop_seed=None):
        self.ops, self.cfg, self.P, self.T = ops, cfg, P, tdtype
        sw = SWITCHES      # the A/B switches, read once at import (class Switches)
        # Dropout / DropPath: active only in training with a rate > 0 -- `drop_seed` is then the base seed of this
        # forward pass (None = everything off, the case of every shipped config).  Masks are counter-based (dropmask.py): the
        # element-wise ones and DropPath run as three small kernels around the fused path, the attention-probability dropout
        # inside the attention kernels (round 3: the mask is a hash of the element's index in the reference's attn tensor).
        self.drop_seed = drop_seed
        # low-memory mode (model.recompute): what only feeds GEMMs in backward -- the LayerNorm output of every sub-layer and the
        # MLP's post-activation -- is rebuilt there (one LayerNorm-forward / one GELU launch each) instead of being kept: 14 -> 12
        # bytes per residual element for an attention sub-layer, 14 -> 6 for an MLP; the full model then trains at 256 clips x 243
        # frames inside the 288 GB of one MI355X.
        self.recompute = False
        # precision 'bf16x3': T-typed tensors are fp32; a tensor that feeds a GEMM is split into (hi, lo) bf16 planes first
        # (`_mm`), and where it ONLY feeds GEMMs (LayerNorm output, GELU output) the planes are what is kept for backward
        self.x3 = x3
        self.x3_planes = sw.x3_planes and hasattr(ops, 'layernorm_fwd_planes_ok')      # A/B switch: 0 = every operand through mbx_split_bf16
        self.Wn: Dict[str, torch.Tensor] = {}
        self.Wt: Dict[str, torch.Tensor] = {}
        # The st and ts blocks of a level are independent (DSTformer.py:341-342 feeds both the same x): with
        # MBX_DUAL_STREAM=1 the ts block runs on a second HIP stream so that HBM-bound kernels of one stream
        # (LayerNorm, GEMM epilogues) overlap MFMA-bound kernels of the other.
        self.dual = sw.dual_stream and getattr(ops, 'multi_stream', False)
        # (Measured and dropped: the weight-gradient GEMMs on a third stream -- 137.0 -> 136.0 ms per step at 64 clips, but the
        # operands stay alive until that stream catches up (record_stream), which at 256 clips (231 GiB resident) sends the
        # allocator into retries: 421 -> 37 clips/s.)
        # What the plan of a pass may use (`Caps`, `_plan` says what each is for): A/B switch AND the provider's capability.  `fold`
        # also by request (model.fold_ln = False), `gelu_d` likewise; model.py lowers both, and sets `recompute`, after construction.
        self.fold = sw.fold_ln and not x3 and drop_seed is None and self._can('can_fold')
        self.gstream_allowed = sw.grad_stream and bool(getattr(ops, 'grad_stream_t', False))
        self.rows_lnbwd = sw.rows_lnbwd and self._can('can_rows_lnbwd')
        self.rows_resid_ln = sw.rows_resid_ln and self._can('can_rows_resid_ln')
        self.block_grad_t = sw.block_grad_t and self.rows_lnbwd and hasattr(ops, 'fuse_bwd_pair') and hasattr(ops, 'embed_bwd_pair')
        self.gelu_d = sw.gelu_d and self.rows_lnbwd and self._can('can_gelu_d')
        self.proj_mlp = sw.proj_mlp and hasattr(ops, 'proj_mlp_fused_fwd')      # 0 = proj + residual as its own GEMM
        self.rawln_allowed = sw.rawln      # A/B switch: 0 = the training sequencing without saves
        # State of a pass; complete here, so that a caller may drive a Block without `forward()` (bench.py): it sets dev / B / Tlen / M
        # (and rawln, grads) itself and calls prepare_weights(), which makes the plan.
        self.rawln = False        # no-grad sequencing of a Block (decided per forward): raw-operand LayerNorm + fused MLP, see the module docstring
        self.gstream = False      # read by nothing (the plan has it); kept assignable for bench.py, which still sets it
        self.ragged = None        # (clip_tab, n_clips, max_len) of a ragged batch
        self.plan: Optional[Plan] = None
        self.grads = None
        self.Bf: Dict[str, torch.Tensor] = {}
        self.Rs: Dict[str, torch.Tensor] = {}
        self.Pn: Dict[str, torch.Tensor] = {}       # plan.pack_n: transposed folded weights in the fragment order of mbx_rows_lnbwd_t
        self.Pf: Dict[str, torch.Tensor] = {}       # plan.pack_f: proj / fc2 in the fragment order of the row-owner kernels
        self.Pk: Dict[str, torch.Tensor] = {}       # plan.pack_k: fc1 / fc2 of every MLP (with the proj in front of it) and every qkv, fused kernels' order

    def _make_plan(self, need_grad: bool) -> Plan:
        caps = Caps(fold=self.fold, x3=self.x3, recompute=self.recompute, gelu_d=self.gelu_d,
                    grad_stream=self.gstream_allowed, rows_lnbwd=self.rows_lnbwd, rows_resid_ln=self.rows_resid_ln,
                    block_grad_t=self.block_grad_t, proj_mlp=self.proj_mlp, fuse_ln=hasattr(self.ops, 'fuse_ln_fwd'))
        return plan_pass(self.cfg, caps, self.M, need_grad, self.rawln)

    def _streams(self):
        """(main, side) streams for the dual-stream schedule, or (None, None)."""
        if not (self.dual and self.dev.type == 'cuda'):
            return None, None
        idx = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        side = Engine._side_streams.get(idx)
        if side is None:
            side = Engine._side_streams[idx] = torch.cuda.Stream(device=idx)
        return torch.cuda.current_stream(idx), side

    # ------------------------------------------------------------------ helpers
    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def _t(self, *shape):
        return torch.empty(shape, dtype=self.T, device=self.dev)

    def _can(self, name: str) -> bool:      # capability probe of the kernel provider (none: no)
        return bool(getattr(self.ops, name, lambda *_: False)(self.T, self.cfg))

    @staticmethod
    def _await(extra):      # dual-stream backward: the other block's input gradient, awaited only now
        return extra() if callable(extra) else extra

    def _drops(self, pre: str, sub: int) -> Optional[Drops]:
        """Active dropout of sub-layer `sub` of block `pre` ('blocks_st.3'), or None."""
        if self.drop_seed is None:
            return None
        from .dropmask import site_seed
        cfg = self.cfg
        stream, level = (0 if pre.startswith('blocks_st') else 1), int(pre.split('.')[1])
        pp = float(cfg.dpr[level]) if cfg.dpr else 0.0
        if cfg.drop <= 0 and pp <= 0 and cfg.attn_drop <= 0:
            return None
        ss = lambda kind: site_seed(self.drop_seed, level, stream, sub, kind)
        return Drops(cfg.drop, ss(1), ss(2), pp, ss(3), cfg.attn_drop, ss(0))

    def _xn(self, sv, pre, norm):
        """The normalised GEMM operand of a sub-layer in backward: the saved one, or (recompute mode) LayerNorm of the saved input."""
        return sv['xn'] if sv['xn'] is not None else self._mm(self._layernorm(sv['x'], f'{pre}.{norm}')[0])

    def _layernorm(self, x, norm):      # -> (xn, mean, rstd): LayerNorm `norm` of x, or (None) its plain normalisation xhat
        xn, mean, rstd = self._op(self.M, self.cfg.C), self._f(self.M), self._f(self.M)
        self.ops.layernorm_fwd(x, self.P[norm + '.weight'] if norm else None, self.P[norm + '.bias'] if norm else None, self.cfg.eps, xn, mean, rstd)
        return xn, mean, rstd

    def _norm_in(self, x, pre, norm, ln):
        """(GEMM operand, mean, rstd) of a sub-layer's LayerNorm; `ln` when LayerNorm(x) came with x from its producer."""
        xn, mean, rstd = ln if ln is not None else self._layernorm(x, None if self.plan.fold else f'{pre}.{norm}')
        return self._mm(xn), mean, rstd

    def _mm(self, t):
        """GEMM operand form of a T-typed tensor: itself, or its (hi, lo) bf16 planes in bf16x3 mode (already planes: unchanged)."""
        return self.ops.split(t) if self.x3 and not isinstance(t, tuple) else t

    def _op(self, *shape):
        """A tensor that is ONLY read as a GEMM operand: T-typed, or -- bf16x3 -- the pair of bf16 planes its producer writes directly
        (no fp32 copy for mbx_split_bf16 to read again)."""
        if self.x3 and self.x3_planes:
            return (torch.empty(shape, dtype=torch.bfloat16, device=self.dev), torch.empty(shape, dtype=torch.bfloat16, device=self.dev))
        return self._t(*shape)

    def _weight_cache_key(self, need_grad: bool):
        """Key of the prepared-weight cache of the no-grad path: the parameters' storage and version counters (every
        in-place update -- optimizer.step(), FlatAdamW, load_state_dict -- bumps them) and everything that selects a format.  None =
        do not cache: a backward follows (training re-prepares every step anyway), or a hipGraph is being captured (the re-pack has
        to be part of the graph so that a replay picks up weights updated in place, graph.py).  Edits through `param.data` bypass the
        version counters (as they bypass autograd's own checks); what covers the ordinary train-then-eval loop is that every
        need_grad forward, `model.train()` and `load_state_dict()` drop the cache (prepare_weights, model.py).  An edit through
        `.data` in a pure inference process still needs `hip_ops.get().weight_cache.clear()`."""
        if need_grad or not hasattr(self.ops, 'weight_cache') or self.dev.type != 'cuda' or torch.cuda.is_current_stream_capturing():
            return None
        return (tuple((p.data_ptr(), p._version) for p in self.P.values()), self.T, self.plan.formats)

    def prepare_weights(self, need_grad: bool):
        """T-typed copies of every Linear weight (and their transposes when a backward follows); with LayerNorm folding the
        qkv / fc1 weights are W diag(gamma) and come with their folded bias and row sums.  Under no_grad the prepared set is kept
        on the kernel provider and reused as long as no parameter changed: an inference call then launches no fold / pack kernels
        (at depth 5 they were ~60 small launches per forward, as many as a B = 1 forward has kernels of its own)."""
        ops, P = self.ops, self.P
        self.plan = self._make_plan(need_grad)      # (every call: a caller may have changed M or rawln since the last one)
        if need_grad and hasattr(ops, 'weight_cache') and self.dev.type == 'cuda':
            # a training step follows: whatever it does to the parameters -- also through `p.data`, which bumps no version counter
            # (legacy optimizers, EMA code, a replayed graph) -- the next no-grad forward must not find this forward's prepared set
            # (ADVICE r5).  model.train() / load_state_dict() drop it as well (model.py).
            ops.weight_cache.pop(self.dev.index, None)
        key = self._weight_cache_key(need_grad)
        if key is not None:
            hit = ops.weight_cache.get(self.dev.index)
            # same storage + same versions is not enough: a NEW model built after the old one died gets the same addresses and the
            # same (small) version numbers from the allocator -- the entry must be about these very tensor objects
            if hit is not None and hit[0] == key and len(hit[1]) == len(P) and all(r() is p for r, p in zip(hit[1], P.values())):
                self.Wn, self.Wt, self.Bf, self.Rs, self.Pk, self.Pf = hit[2]
                return
        self._prepare_weights(need_grad)
        if key is not None:
            import weakref
            ops.weight_cache[self.dev.index] = (key, [weakref.ref(p) for p in P.values()], (self.Wn, self.Wt, self.Bf, self.Rs, self.Pk, self.Pf))

    def _prepare_weights(self, need_grad: bool):
        cfg, ops, P, plan = self.cfg, self.ops, self.P, self.plan
        if not plan.fold:
            self.Wn, self.Wt = ops.prep_weights(P, linear_names(cfg), self.T, need_grad, x3=self.x3)
            return
        pairs = folded_pairs(cfg)
        folded = {l for l, _ in pairs}
        self.Wn, self.Wt = ops.prep_weights(P, [n for n in linear_names(cfg) if n not in folded], self.T, need_grad)
        fn, ft, self.Bf, self.Rs = ops.fold_norm_weights(P, pairs, need_grad, self.T)
        self.Wn.update(fn)
        self.Wt.update(ft)
        if plan.pack_f:
            self.Pf = dict(zip(plan.pack_f, ops.rows_n_pack_many([self.Wn[lin] for lin in plan.pack_f])))
        if plan.pack_n:
            self.Pn = dict(zip(plan.pack_n, ops.rows_n_pack_many([ft[lin] for lin in plan.pack_n])))
        for what, name, front in plan.pack_k:
            if what == 'qkv':
                self.Pk[name] = ops.rows_pack_nk(self.Wn[name])
            elif front is not None:
                self.Pk[name] = ops.proj_mlp_pack_weights(self.Wn[front], self.Wn[name + '.fc1'], self.Wn[name + '.fc2'])
            else:
                self.Pk[name] = ops.mlp_pack_weights(self.Wn[name + '.fc1'], self.Wn[name + '.fc2'])

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, return_rep, need_grad: bool, tta_perm=None, ragged=None):
        """`return_rep`: False (pose output), True (representation, DSTformer.py:360) or a tuple ('pool', persons, p, seed):
        the ActionNet pooling of model_action.py:15-24 fused onto the representation (mean over persons and frames of the
        dropped-out representation -> [B / persons, J, R]).
        `ragged` = (clip_tab, frame_t, n_clips, max_len), inference only: x [1,F,J,Din] holds clips of different lengths one after
        another; clip_tab [n_clips,2] int32 = (first frame, frames) and frame_t [F] int32 = the index of every frame inside its clip, both
        on the device.  Only the embedding and the temporal attention know where a clip starts; every other kernel runs on the F J rows
        as on a batch of one clip of F frames."""
        cfg, ops, P = self.cfg, self.ops, self.P
        pool = return_rep if isinstance(return_rep, tuple) else None
        return_rep = bool(return_rep)
        self.dev = x.device
        B, T, J, Din = x.shape
        self.ragged = None
        if ragged is not None:
            if need_grad or self.drop_seed is not None or pool is not None:
                raise RuntimeError('a ragged batch is an inference path: no gradient, no dropout and no pooled representation')
            clip_tab, frame_t, n_clips, max_len = ragged
            if B != 1 or frame_t.numel() != T or clip_tab.numel() != 2 * n_clips or not 1 <= n_clips <= T:
                raise RuntimeError(f'a ragged batch is x [1,F,J,C] with frame_t [F] and clip_tab [n_clips,2]: got x {tuple(x.shape)}, frame_t '
                                   f'{tuple(frame_t.shape)}, clip_tab {tuple(clip_tab.shape)} for {n_clips} clips')
            if not 1 <= max_len <= min(cfg.maxlen, 256):
                raise RuntimeError(f'a ragged batch takes clips of 1 .. {min(cfg.maxlen, 256)} frames, got max_len = {max_len}')
            if 2 * T * max(cfg.H, J) >= 1 << 31:      # the problem counts of the spatial attention (2 F H) and the token index are 32-bit
                raise RuntimeError(f'a ragged batch of {T} frames is too large')
            if tta_perm is not None:      # the doubled batch: the same clips again, F frames further on
                clip_tab = clip_tab.reshape(n_clips, 2).repeat(2, 1)
                clip_tab[n_clips:, 0] += T
                n_clips = 2 * n_clips
            self.ragged = (clip_tab.contiguous(), n_clips, int(max_len))
        if tta_perm is not None:      # flip test-time augmentation: the batch doubles, the second half is the flipped view
            B = 2 * B
        M, C = B * T * J, cfg.C
        self.B, self.Tlen, self.M = B, T, M
        self.rawln = not need_grad and self.fold and self.rawln_allowed and self._can('can_fuse_mlp')
        self.prepare_weights(need_grad)
        plan = self.plan
        h = self._f(M, C)
        ln0 = None      # (xhat, mean, rstd) of h when the embedding kernel normalises its own rows (a plain batch)
        if plan.embed_norm and ragged is None and tta_perm is None and hasattr(ops, 'embed_ln_fwd') and self._can('can_embed_ln'):
            ln0 = (self._t(M, C), self._f(M), self._f(M))
            ops.embed_ln_fwd(x, P['joints_embed.weight'], P['joints_embed.bias'], P['pos_embed'], P['temp_embed'], cfg.eps, h, *ln0, B, T, J)
        elif ragged is not None and tta_perm is not None:
            ops.embed_fwd_tta_ragged(x, tta_perm, P['joints_embed.weight'], P['joints_embed.bias'], P['pos_embed'], P['temp_embed'], frame_t, h, T, J)
        elif ragged is not None:
            ops.embed_fwd_ragged(x, P['joints_embed.weight'], P['joints_embed.bias'], P['pos_embed'], P['temp_embed'], frame_t, h, T, J)
        elif tta_perm is not None:
            ops.embed_fwd_tta(x, tta_perm, P['joints_embed.weight'], P['joints_embed.bias'], P['pos_embed'], P['temp_embed'], h, B // 2, T, J)
        else:
            ops.embed_fwd(x, P['joints_embed.weight'], P['joints_embed.bias'], P['pos_embed'], P['temp_embed'], h, B, T, J)
        if self.drop_seed is not None and cfg.drop > 0:      # pos_drop (DSTformer.py:337)
            from .dropmask import site_seed
            ops.dropout(h, h, cfg.drop, site_seed(self.drop_seed, -1, 0, 0, 1))
        saved: Dict[str, Any] = dict(x=x, levels=[], return_rep=return_rep)
        main, side = self._streams()
        ln_st = ln_ts = ln_tail = None      # (xn, mean, rstd) of h already produced by the fusion kernel of the previous level
        if plan.embed_norm:
            ln_st = ln_ts = ln0 if ln0 is not None else self._layernorm(h, None)
        for i in range(cfg.depth):
            if side is not None:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    x_ts, sv_ts = self._block_fwd(h, f'blocks_ts.{i}', 'ts', need_grad, ln_ts)
                x_st, sv_st = self._block_fwd(h, f'blocks_st.{i}', 'st', need_grad, ln_st)
                main.wait_stream(side)
            else:
                x_st, sv_st = self._block_fwd(h, f'blocks_st.{i}', 'st', need_grad, ln_st)
                x_ts, sv_ts = self._block_fwd(h, f'blocks_ts.{i}', 'ts', need_grad, ln_ts)
            ln_st = ln_ts = None      # consumed; the fusion kernel below may provide the next level's
            hn = self._f(M, C)
            what = plan.fuse_norm[i]
            if what is not None:      # the fusion kernel also normalises its output for its consumers (one mean / rstd for the two)
                alpha, mean, rstd = self._f(M, 2), self._f(M), self._f(M)
                n1, n2 = (('norm', None) if what == 'norm' else (None, None) if what == 'xhat' else
                          (f"blocks_st.{i + 1}.{ORDER['st'][0][1]}", f"blocks_ts.{i + 1}.{ORDER['ts'][0][1]}"))
                xn1, xn2 = self._t(M, C), (self._t(M, C) if n2 else None)
                gb = [P[f'{n}.{k}'] if n else None for n in (n1, n2) for k in ('weight', 'bias')]
                ops.fuse_ln_fwd(x_st, x_ts, P[f'ts_attn.{i}.weight'], P[f'ts_attn.{i}.bias'], hn, alpha,
                                gb[0], gb[1], xn1, gb[2], gb[3], xn2, cfg.eps, mean, rstd)
                if what == 'norm':
                    ln_tail = (xn1, mean, rstd)
                else:
                    ln_st, ln_ts = (xn1, mean, rstd), (xn2 if n2 else xn1, mean, rstd)
            elif cfg.att_fuse:
                alpha = self._f(M, 2)
                ops.fuse_fwd(x_st, x_ts, P[f'ts_attn.{i}.weight'], P[f'ts_attn.{i}.bias'], hn, alpha)
            else:
                alpha = None
                ops.average(x_st, x_ts, hn)
            if need_grad:
                saved['levels'].append(dict(st=sv_st, ts=sv_ts, x_st=x_st, x_ts=x_ts, alpha=alpha))
            h = hn
        if ln_tail is not None:
            xn, mean, rstd = ln_tail
        else:
            xn, mean, rstd = self._layernorm(h, 'norm')
        xn = self._mm(xn)
        # the returned tensor is allocated in its final 4-D shape (the kernels see [M, .] views of it): autograd refuses
        # in-place writes into an output that is itself a view (callers do `out[:, :, 0, :] = 0`, train.py:76)
        rep4 = self._f(B, T, J, cfg.R)
        rep = rep4.view(M, cfg.R)
        ops.gemm_nt(xn, self.Wn['pre_logits.fc'], P['pre_logits.fc.bias'], EPI_TANH, out_f=rep)
        if need_grad:
            saved.update(h=h, xn=xn, mean=mean, rstd=rstd, rep=rep, pool=pool)
        if pool is not None:
            _, persons, p_drop, seed = pool
            if B % persons:
                raise RuntimeError(f'pooled representation: batch {B} is not a multiple of persons={persons}')
            out = self._f(B // persons, J, cfg.R)
            ops.pool_rep_fwd(rep, out, B // persons, persons, T, J, p_drop, seed)
        elif return_rep:
            out = rep4
        else:
            out = self._f(B, T, J, cfg.dim_out)
            ops.head_fwd(rep, P['head.weight'], P['head.bias'], out.view(M, cfg.dim_out))
            if tta_perm is not None:      # flip back + average (train.py:70-72)
                both, out = out, self._f(B // 2, T, J, cfg.dim_out)
                ops.flip_average(both, tta_perm, out)
        return out, saved

    def _block_fwd(self, x, pre, kind, need_grad, ln=None):
        """`ln` = (xn, mean, rstd) of x when its producer already normalised it (the fusion kernel of the previous level, for the
        first sub-layer of a Block); never anything else."""
        svs = []
        o = None      # no-grad: output of an attention whose proj + residual is left to the MLP kernel that follows
        for sub, (typ, norm, mod, mode) in enumerate(ORDER[kind]):
            sp = self.plan.sub[pre, sub]
            if typ == 'attn':
                x, sv, ln, o = self._attn_fwd(x, pre, norm, mod, mode, need_grad, sub, ln, sp)
            else:
                x, sv, ln = self._mlp_fwd(x, pre, norm, mod, need_grad, sub, ln, sp, o)
                o = None
            svs.append(sv)
        return x, svs

    def _resid_gemm(self, a, lin, x, dm, sp):
        """y = x + a . W^T + b (fp32 residual stream): returns (y, ln) -- ln = (xhat, mean, rstd) of y for the next sub-layer when the
        row-owner kernel ran (it owns whole rows, so LayerNorm's statistics cost it nothing), else None."""
        cfg, ops, P = self.cfg, self.ops, self.P
        y = self._f(self.M, cfg.C)
        if sp.lin_out == 'rows':
            xn, mean, rstd = self._op(self.M, cfg.C), self._f(self.M), self._f(self.M)
            ops.rows_resid_ln(a, self.Pf[lin], P[lin + '.bias'], x, y, xn, mean, rstd, cfg.eps)
            return y, (xn, mean, rstd)
        ops.gemm_nt(a, self.Wn[lin], P[lin + '.bias'], EPI_RESID, resid=x, out_f=y)
        if dm is not None and dm.branch:      # proj_drop / MLP drop + DropPath on the branch (DSTformer.py:84,148-149,241-242)
            ops.residual_drop(y, x, cfg.J, dm.p, dm.seed_branch, dm.p_path, dm.seed_path)
        return y, None

    def _attn_fwd(self, x, pre, norm, attn, mode, need_grad, sub, ln, sp):
        cfg, ops, P = self.cfg, self.ops, self.P
        M, C = self.M, cfg.C
        qkv = self._t(M, 3 * C)
        lin = f'{pre}.{attn}.qkv'
        if sp.lin_in == 'raw':      # no-grad: LayerNorm + qkv straight from the fp32 rows (operand, statistics and row constants made in the kernel)
            xn = mean = rstd = None
            ops.rows_gemm_nk_ln(x, self.Pk[lin], self.Bf[lin], self.Rs[lin], cfg.eps, qkv)
        else:
            xn, mean, rstd = self._norm_in(x, pre, norm, ln)
            ops.gemm_nt(xn, self.Wn[lin], self.Bf[lin] if self.plan.fold else P.get(lin + '.bias'), EPI_STORE, out_t=qkv)
        dm = self._drops(pre, sub)
        o, lse = self._t(M, C), self._f(M, cfg.H)
        if self.ragged is not None and mode == MODE_TEMPORAL:      # every clip its own length; the B Tlen frames are one packed batch
            clip_tab, n_clips, max_len = self.ragged
            ops.attn_fwd_ragged(qkv, o, lse, clip_tab, n_clips, self.B * self.Tlen, max_len, cfg.J, cfg.H, cfg.scale)
        else:
            ops.attn_fwd(qkv, o, lse, self.B, self.Tlen, cfg.J, cfg.H, cfg.scale, mode, drop=dm.attn if dm else None)
        if sp.lin_out == 'deferred':
            return x, None, None, o
        o_op = self._mm(o)      # (bf16x3: the operand planes are kept for the weight gradient too -- o itself stays fp32 for the attention backward)
        y, ln_y = self._resid_gemm(o_op, f'{pre}.{attn}.proj', x, dm, sp)
        sv = self._saved(x, xn, mean, rstd, dm, qkv=qkv, o=o, lse=lse) if need_grad else None
        if sv is not None and self.x3 and self.x3_planes and not self.recompute:
            sv['o_op'] = o_op
        return y, sv, ln_y, None

    def _saved(self, x, xn, mean, rstd, dm, **core):
        if self.plan.fold:      # backward needs xhat and rstd only: the fp32 sub-layer input is not kept
            return dict(x=None, mean=None, rstd=rstd, xn=xn, dm=dm, **core)
        return dict(x=x, mean=mean, rstd=rstd, xn=None if self.recompute else xn, dm=dm, **core)

    def _mlp_fwd(self, x, pre, norm, mlp, need_grad, sub, ln, sp, o=None):
        cfg, ops, P = self.cfg, self.ops, self.P
        M, C = self.M, cfg.C
        lin = f'{pre}.{mlp}.fc1'
        if sp.lin_out == 'fused':     # no-grad: the whole sub-layer is one kernel; the hidden never reaches HBM, the operand is bf16(x) made in the kernel
            y = self._f(M, C)
            if sp.front is not None:      # x + proj(o) first, in the same kernel
                ops.proj_mlp_fused_fwd(o, self.Pk[f'{pre}.{mlp}'], P[sp.front + '.bias'], self.Bf[lin], P[f'{pre}.{mlp}.fc2.bias'], self.Rs[lin], x, y, cfg.eps)
            else:
                ops.mlp_fused_fwd(None, True, self.Pk[f'{pre}.{mlp}'], self.Bf[lin], P[f'{pre}.{mlp}.fc2.bias'], self.Rs[lin], x, y, None,
                                  cfg.eps, None, None)
            return y, None, None
        xn, mean, rstd = self._norm_in(x, pre, norm, ln)
        dm = self._drops(pre, sub)
        mlp_drop = dm is not None and dm.p > 0
        # u only feeds GELU' in backward; g is only fc2's operand (and the weight gradient's) unless the MLP dropout touches it first
        u, g = (self._t(M, cfg.hidden) if need_grad else None), (self._t(M, cfg.hidden) if mlp_drop else self._op(M, cfg.hidden))
        save_d = need_grad and sp.save == 'd'      # (a forward-only pass over a plan made for training saves nothing)
        if save_d:
            ops.gemm_nt_gelu_d(xn, self.Wn[lin], self.Bf[lin], u, g)
        else:
            ops.gemm_nt(xn, self.Wn[lin], self.Bf[lin] if self.plan.fold else P[lin + '.bias'], EPI_GELU, out_t=u, out2_t=g)
        if mlp_drop:                                          # MLP drop after the activation (DSTformer.py:82)
            ops.dropout(g, g, dm.p, dm.seed_act)
        g = self._mm(g)
        y, ln_y = self._resid_gemm(g, f'{pre}.{mlp}.fc2', x, dm, sp)
        sv = self._saved(x, xn, mean, rstd, dm, u=None if save_d else u, d=u if save_d else None, g=None if self.recompute else g) if need_grad else None
        return y, sv, ln_y

    # ----------------------------------------------------------------- backward
    def backward(self, saved, dout: torch.Tensor, grads: Dict[str, torch.Tensor], want_dx: bool, on_ready=None):
        """Fills `grads[name]` (fp32, pre-allocated, same shapes as the parameters) and
        returns d(input) or None.  `dout` is d(out) with the shape `forward` returned.
        `on_ready(bucket)` is called as soon as every gradient of a bucket has been enqueued
        (bucket 0 = tail, 1..depth = levels depth-1..0, depth+1 = embedding; see `grad_bucket`):
        the data-parallel wrapper starts that bucket's all-reduce while backward continues."""
        cfg, ops, P = self.cfg, self.ops, self.P
        M, C, R = self.M, cfg.C, cfg.R
        B, T, J = self.B, self.Tlen, cfg.J
        G = self.grads = grads
        plan = self.plan
        dpre = self._t(M, R)
        if saved.get('pool') is not None:
            _, persons, p_drop, seed = saved['pool']
            ops.tanh_pool_bwd(dout.reshape(B // persons, J, R), saved['rep'], dpre, B // persons, persons, T, J, p_drop, seed)
        elif saved['return_rep']:
            ops.tanh_bwd(dout.reshape(M, R), saved['rep'], dpre)
        if saved['return_rep']:
            if 'head.weight' in G:
                G['head.weight'].zero_()
                G['head.bias'].zero_()
        else:
            ops.head_bwd(dout.reshape(M, cfg.dim_out), saved['rep'], P['head.weight'], dpre,
                         G['head.weight'], G['head.bias'])
        dxn = self._t(M, C)
        dpre = self._mm(dpre)
        ops.gemm_tn(dpre, saved['xn'], G['pre_logits.fc.weight'], G['pre_logits.fc.bias'])
        ops.gemm_nt(dpre, self.Wt['pre_logits.fc'], None, EPI_STORE, out_t=dxn)
        dh = self._f(M, C)
        ops.layernorm_bwd(dxn, saved['h'], saved['mean'], saved['rstd'], P['norm.weight'],
                          None, None, dh, None, G['norm.weight'], G['norm.bias'])
        del dxn, dpre
        if on_ready is not None:
            on_ready(0)
        pair = None      # the two Blocks' input gradients of the level above, T-typed (plan.out_t), instead of their fp32 sum dh
        for i in reversed(range(cfg.depth)):
            lv = saved['levels'][i]
            # (gradient stream in the operand type: the Blocks read the T-typed copies only, the fp32 ones are not even written)
            d_st, d_ts = (None, None) if (plan.gstream and cfg.att_fuse) else (self._f(M, C), self._f(M, C))
            d_st_t, d_ts_t = self._t(M, C), self._t(M, C)
            if cfg.att_fuse:
                if pair is not None:
                    ops.fuse_bwd_pair(pair[0], pair[1], lv['x_st'], lv['x_ts'], lv['alpha'], P[f'ts_attn.{i}.weight'],
                                      d_st_t, d_ts_t, G[f'ts_attn.{i}.weight'], G[f'ts_attn.{i}.bias'])
                else:
                    ops.fuse_bwd(dh, lv['x_st'], lv['x_ts'], lv['alpha'], P[f'ts_attn.{i}.weight'],
                                 d_st, d_ts, d_st_t, d_ts_t, G[f'ts_attn.{i}.weight'], G[f'ts_attn.{i}.bias'])
            else:
                ops.average_bwd(dh, d_st, d_ts, d_st_t, d_ts_t)
            pair = dh = None
            main, side = self._streams()
            if plan.out_t[i]:      # the row-owner tail takes both Blocks' first sub-layers: their input gradients go down T-typed
                if side is not None:
                    side.wait_stream(main)
                _, a_t = self._block_bwd(d_st, d_st_t, lv['st'], f'blocks_st.{i}', 'st', None, last_needs_t=True)
                if side is not None:
                    with torch.cuda.stream(side):
                        _, b_t = self._block_bwd(d_ts, d_ts_t, lv['ts'], f'blocks_ts.{i}', 'ts', None, last_needs_t=True)
                    main.wait_stream(side)
                    b_t.record_stream(main)
                else:
                    _, b_t = self._block_bwd(d_ts, d_ts_t, lv['ts'], f'blocks_ts.{i}', 'ts', None, last_needs_t=True)
                pair = (a_t, b_t)
                del a_t, b_t
            elif side is not None:
                # the st block runs on the main stream, the ts block on the side stream; the side stream's LAST kernel (the
                # LayerNorm backward at the block input) waits for the main block and adds its input gradient as `extra`
                # -- no separate d1 + d2 pass over the residual stream (1.6 GB per level)
                side.wait_stream(main)
                d1, _ = self._block_bwd(d_st, d_st_t, lv['st'], f'blocks_st.{i}', 'st', None, last_needs_t=False)

                def other(d1=d1, main=main, side=side):
                    side.wait_stream(main)
                    d1.record_stream(side)
                    return d1
                with torch.cuda.stream(side):
                    dh, _ = self._block_bwd(d_ts, d_ts_t, lv['ts'], f'blocks_ts.{i}', 'ts', other, last_needs_t=False)
                main.wait_stream(side)
                dh.record_stream(main)
                del d1
            else:
                d1, _ = self._block_bwd(d_st, d_st_t, lv['st'], f'blocks_st.{i}', 'st', None, last_needs_t=False)
                # the second stream's last LN-backward also adds the first stream's input gradient
                dh, _ = self._block_bwd(d_ts, d_ts_t, lv['ts'], f'blocks_ts.{i}', 'ts', d1, last_needs_t=False)
                del d1
            del d_st, d_st_t, d_ts, d_ts_t
            saved['levels'][i] = None  # release this level's activations
            if on_ready is not None:
                on_ready(cfg.depth - i)
        if self.drop_seed is not None and cfg.drop > 0:
            from .dropmask import site_seed
            ops.dropout(dh, dh, cfg.drop, site_seed(self.drop_seed, -1, 0, 0, 1))
        dx = torch.empty_like(saved['x']) if want_dx else None
        if pair is not None:
            ops.embed_bwd_pair(pair[0], pair[1], saved['x'], P['joints_embed.weight'], G['joints_embed.weight'], G['joints_embed.bias'],
                               G['pos_embed'], G['temp_embed'], dx, B, T, J)
        else:
            ops.embed_bwd(dh, saved['x'], P['joints_embed.weight'], G['joints_embed.weight'], G['joints_embed.bias'],
                          G['pos_embed'], G['temp_embed'], dx, B, T, J)
        if on_ready is not None:
            on_ready(cfg.depth + 1)
        return dx

    def _block_bwd(self, dy, dy_t, svs, pre, kind, extra_last, last_needs_t):
        for idx in reversed(range(4)):
            typ, norm, mod, mode = ORDER[kind][idx]
            extra = extra_last if idx == 0 else None
            need_t = True if idx > 0 else last_needs_t
            dy, dy_t = self._sub_bwd(self.plan.sub[pre, idx], typ, dy, dy_t, svs[idx], pre, norm, mod, mode, extra, need_t)
            svs[idx] = None
        return dy, dy_t

    def _sub_bwd(self, sp, typ, dy, dy_t, sv, pre, norm, mod, mode, extra, need_t):
        """One sub-layer: branch gradient, the core back to the Linear-in's output gradient dY, and a tail: returns (dx, dx_t)."""
        ops, G = self.ops, self.grads
        lin = f'{pre}.{mod}.{LINEARS[typ][0]}'
        dy_t = self._branch_grad(dy, dy_t, sv.get('dm'))
        # the row-owner tail serves a gradient that arrives and leaves in the operand type only (always so inside a Block; at its first
        # sub-layer when the caller asks for that and adds nothing); it takes its row means itself, so the core runs without row dots
        tail = sp.tail if sp.tail != 'rows' or (need_t and extra is None) else 'fold'
        dY, part = self._attn_bwd(dy_t, sv, pre, mod, mode, tail) if typ == 'attn' else self._mlp_bwd(dy_t, sv, pre, mod, sp, tail)
        if tail != 'plain':
            return self._fold_tail(dY, part, sv, lin, f'{pre}.{norm}', dy, dy_t, extra, need_t)
        dxn = self._t(self.M, self.cfg.C)
        dY = self._mm(dY)
        ops.gemm_tn(dY, self._xn(sv, pre, norm), G[lin + '.weight'], G.get(lin + '.bias'))
        ops.gemm_nt(dY, self.Wt[lin], None, EPI_STORE, out_t=dxn)
        del dY      # (the largest tensor of the sub-layer: released before the tail allocates)
        return self._plain_tail(dxn, sv, pre, norm, dy, extra, need_t)

    def _branch_grad(self, dy, dy_t, dm):
        """GEMM operand of the gradient that enters a sub-layer's branch (the residual path keeps dy)."""
        if dm is not None and dm.branch:      # gradient entering the dropped branch
            dy_t = self._t(self.M, self.cfg.C)
            self.ops.grad_drop(dy, dy_t, self.cfg.J, dm.p, dm.seed_branch, dm.p_path, dm.seed_path)
            return self._mm(dy_t)
        if self.x3 and not isinstance(dy_t, tuple):
            return self._mm(dy)          # bf16x3: the GEMM operand is the split of the fp32 gradient itself (unless its producer wrote the planes)
        return dy_t

    def _attn_bwd(self, dy_t, sv, pre, attn, mode, tail):      # -> (dqkv, its row dots for the folded tile tail or None)
        cfg, ops, G = self.cfg, self.ops, self.grads
        M, C = self.M, cfg.C
        lin, proj = f'{pre}.{attn}.qkv', f'{pre}.{attn}.proj'
        do = self._t(M, C)
        ops.gemm_tn(dy_t, sv['o_op'] if 'o_op' in sv else self._mm(sv['o']), G[proj + '.weight'], G[proj + '.bias'])
        ops.gemm_nt(dy_t, self.Wt[proj], None, EPI_STORE, out_t=do)
        dqkv = self._t(M, 3 * C) if tail != 'plain' else self._op(M, 3 * C)     # (bf16x3: the attention backward writes the operand planes itself)
        dims = (self.B, self.Tlen, cfg.J, cfg.H, cfg.scale, mode)
        if tail == 'fold':
            part = self._f(2 * cfg.H, M, 2)       # block-major; per head: the q columns, the k + v columns
            ops.attn_bwd_stats(sv['qkv'], sv['o'], do, sv['lse'], dqkv, self.Bf[lin], self.Rs[lin], part, *dims)
            return dqkv, part
        dm = sv.get('dm')
        ops.attn_bwd(sv['qkv'], sv['o'], do, sv['lse'], dqkv, *dims, drop=dm.attn if dm else None)
        return dqkv, None

    def _plain_tail(self, dxn, sv, pre, norm, dy, extra, need_t):
        """The counterpart of `_fold_tail`: (dx, dx_t), dx = dy [+ extra] + LayerNorm'(dxn) (dx_t -- bf16x3: operand planes -- if need_t)."""
        P, G = self.P, self.grads
        M, C = self.M, self.cfg.C
        dx = self._f(M, C)
        dx_t = (self._t(M, C) if not self.x3 else (self._op(M, C) if self.x3_planes else None)) if need_t else None
        self.ops.layernorm_bwd(dxn, sv['x'], sv['mean'], sv['rstd'], P[f'{pre}.{norm}.weight'], dy, self._await(extra),
                               dx, dx_t, G[f'{pre}.{norm}.weight'], G[f'{pre}.{norm}.bias'])
        return dx, dx_t

    def _fold_tail(self, dY, part, sv, lin, norm, dy, dy_t, extra, need_t):
        """Folded (LayerNorm -> Linear) pair, backward from the Linear's output gradient dY and its row dots `part`: weight
        gradient, then dx = dy [+ extra] + LayerNorm'(dY . W') as the epilogue of the dX GEMM, then the parameter gradients of
        W, gamma and beta from the folded weight gradient.  With the gradient stream in the operand type (plan.gstream) the incoming
        dy is read as dy_t and, inside a Block (need_t), only the T-typed dx is written: returns (None, dx_t)."""
        cfg, ops, P, G = self.cfg, self.ops, self.P, self.grads
        M, C = self.M, cfg.C
        rows = part is None                # the row-owner tail: row means taken by the dX kernel itself, no row dots, no row constants
        if not rows:
            rowc = self._f(M, 4)
            ops.lnbwd_rowc(part, sv['rstd'], rowc, C)
        db = G.get(lin + '.bias')
        if db is None:                     # qkv_bias=False: the column sums of dY are still needed for d(beta)
            db = self._f(dY.shape[1])
        stream = self.plan.gstream      # (a folded sub-layer always gets dy_t: from the tail above it, or from the fusion backward)
        dres = dy_t if stream else dy
        ops.gemm_tn(dY, sv['xn'], G[lin + '.weight'], db)
        ops.unfold_norm_grads(G[lin + '.weight'], db, P[lin + '.weight'], P[norm + '.weight'], P[norm + '.bias'],
                              G[norm + '.weight'], G[norm + '.bias'])
        if rows:
            dx_t = self._t(M, C)
            ops.rows_lnbwd_t(dY, self.Pn[lin], sv['xn'], sv['rstd'], dres, dx_t)
            return None, dx_t
        dx = None if (stream and need_t) else self._f(M, C)
        dx_t = self._t(M, C) if need_t else None
        ops.gemm_nt_lnbwd(dY, self.Wt[lin], sv['xn'], rowc, dres, self._await(extra), dx, dx_t)
        return dx, dx_t

    def _mlp_bwd(self, dy_t, sv, pre, mlp, sp, tail):      # -> (du, its row dots for the folded tile tail or None)
        cfg, ops, G = self.cfg, self.ops, self.grads
        M = self.M
        lin, fc2 = f'{pre}.{mlp}.fc1', f'{pre}.{mlp}.fc2'
        du = self._t(M, cfg.hidden)
        dm = sv.get('dm')
        act_drop = dm is not None and dm.p > 0      # the MLP's drop after the activation
        g = sv['g']
        if g is None:                                         # recompute mode: post-activation from the saved pre-activation
            g = self._t(M, cfg.hidden)
            ops.gelu_fwd(sv['u'], g)
            if act_drop:
                ops.dropout(g, g, dm.p, dm.seed_act)
            g = self._mm(g)
        ops.gemm_tn(dy_t, g, G[fc2 + '.weight'], G[fc2 + '.bias'])
        del g
        if sp.save == 'd':                                    # forward saved gelu'(u): one multiply, then the row-owner tail
            ops.gemm_nt_mul(dy_t, self.Wt[fc2], sv['d'], du)
            return du, None
        if tail == 'fold':
            part = self._f(cfg.hidden // 64, M, 2)
            ops.gemm_nt_dgelu_stats(dy_t, self.Wt[fc2], du, sv['u'], self.Bf[lin], self.Rs[lin], part)
            return du, part
        if self.x3 and not act_drop:
            du = self._op(M, cfg.hidden)                      # bf16x3: the GELU' epilogue writes the operand planes itself
        ops.gemm_nt(dy_t, self.Wt[fc2], None, EPI_DGELU, out_t=du, aux_t=sv['u'])
        if act_drop:                                          # backward of the drop after the activation (commutes with GELU')
            ops.dropout(du, du, dm.p, dm.seed_act)
        return du, None
