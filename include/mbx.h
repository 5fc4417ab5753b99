/* mbx.h -- C ABI of libmbx.so: the MI355X (gfx950) kernel set behind the DSTformer hot path.
 *
 * The reference (Walter0807/MotionBERT) has no FFI: its hot path is the Python class
 * lib/model/DSTformer.py:269-361 running on stock ATen ops.  This header is therefore the
 * boundary this project defines for that path; each entry names the reference arithmetic it
 * replaces (file:line in the reference checkout).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C types only; every pointer is DEVICE memory owned by the caller (PyTorch);
 *     the library never allocates, frees, caches or synchronises;
 *   - every call enqueues kernels on `stream` (a hipStream_t passed as void*) and returns;
 *   - return 0 on success, non-zero on argument/launch error; mbx_last_error() gives the
 *     text (thread-local).  No C++ exceptions cross the ABI;
 *   - re-entrant, no mutable global state (DataParallel replica threads, autograd thread);
 *   - `dtype` selects the operand type T of GEMM/attention tensors:
 *       MBX_BF16  bf16 operands, fp32 MFMA accumulation      (v_mfma_f32_32x32x16_bf16)
 *       MBX_F32   fp32 operands, exact fp32 MFMA              (v_mfma_f32_32x32x2_f32)
 *     residual stream, statistics and parameter gradients are always fp32;
 *   - token index m = (b*T + t)*J + j; tensors are dense row-major.
 */
#ifndef MBX_H
#define MBX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum mbx_dtype {
    MBX_F32 = 0,
    MBX_BF16 = 1,
    MBX_BF16_LO = 2 /* mbx_prep_weights only: writes bf16(w - float(bf16(w))), the 'lo' plane of the bf16x3 split */
};

/* GEMM epilogues (fused into the store of the accumulator tile) */
enum mbx_epilogue {
    MBX_EPI_STORE = 0, /* out_t = acc + bias                          qkv (DSTformer.py:103,143) / dX GEMMs */
    MBX_EPI_GELU  = 1, /* out2_t = gelu_erf(acc + bias); out_t = acc + bias if non-NULL   fc1 + nn.GELU (:80-81) */
    MBX_EPI_RESID = 2, /* out_f = resid + acc + bias                  proj / fc2 + residual (:241-249)     */
    MBX_EPI_TANH  = 3, /* out_f = tanh(acc + bias)                    pre_logits fc + Tanh (:294-297,354)  */
    MBX_EPI_DGELU = 4, /* out_t = acc * gelu_erf'(aux_t)              backward of nn.GELU                  */
    MBX_EPI_LNBWD = 5, /* internal to mbx_gemm_nt_lnbwd (LayerNorm backward as a GEMM epilogue); not accepted by mbx_gemm_nt */
    /* 6, 7, 8: epilogues of rounds 3 / 4 that never had a caller in the default path; removed in round 5 */
    MBX_EPI_LNBWD_T = 9,  /* internal to mbx_gemm_nt_lnbwd_t (MBX_EPI_LNBWD with the gradient residual stream in bf16) */
    MBX_EPI_GELU_D = 10,  /* internal to mbx_gemm_nt_gelu_d: out2_t = gelu_erf(acc + bias), out_t = gelu_erf'(acc + bias) */
    MBX_EPI_MULAUX = 11   /* internal to mbx_gemm_nt_mul:    out_t = acc * aux_t */
};

enum mbx_attn_mode {
    MBX_ATTN_SPATIAL  = 0, /* softmax over the J joints of one frame   (DSTformer.py:178-186) */
    MBX_ATTN_TEMPORAL = 1  /* softmax over the T frames of one joint   (DSTformer.py:188-200) */
};

const char* mbx_last_error(void);
int mbx_version(void);

/* ---- weights ------------------------------------------------------------------------------
 * One launch converts every nn.Linear weight of the model: for descriptor i, src fp32 [N,K] ->
 * dst_n T [N,K] (may be NULL) and dst_t T [K,N] (transposed copy for the dX GEMMs, may be NULL).
 * `desc` is a device array of n_desc records {src, dst_n, dst_t, N, K} (5 x int64). */
int mbx_prep_weights(const int64_t* desc, int n_desc, int max_n, int max_k, int dtype, void* stream);

/* ---- embedding: joints_embed + pos_embed + temp_embed (DSTformer.py:330-337) --------------
 * x [B,T,J,Din] f32, w [C,Din], b [C], pos [J,C], temp [>=T,C]  ->  h [M,C] f32 */
int mbx_embed_fwd(const float* x, const float* w, const float* b, const float* pos, const float* temp,
                  float* h, int B, int T, int J, int Din, int C, void* stream);
/* mbx_embed_fwd plus the plain normalisation of its rows (the folded path's level-0 operand) in one launch: h [M,C] f32 as above,
 * xhat bf16 [M,C], mean / rstd [M] -- bit for bit what mbx_layernorm_fwd(h, NULL, NULL, eps, xhat, ..., bf16) gives.  Din <= 4, C <= 1024. */
int mbx_embed_ln_fwd(const float* x, const float* w, const float* b, const float* pos, const float* temp, float eps, float* h,
                     void* xhat, float* mean, float* rstd, int B, int T, int J, int Din, int C, void* stream);
/* dh [M,C] -> dw [C,Din], db [C], dpos [J,C], dtemp [T,C] (rows >= T untouched), dx [M,Din] or NULL.
 * ws: >= mbx_embed_bwd_ws(T,J,Din,C) bytes. */
size_t mbx_embed_bwd_ws(int T, int J, int Din, int C);
int mbx_embed_bwd(const float* dh, const float* x, const float* w, float* dw, float* db, float* dpos,
                  float* dtemp, float* dx, int B, int T, int J, int Din, int C, void* ws, void* stream);
/* mbx_embed_bwd with dh = dh_a + dh_b, both bf16 [B*T*J, C] (the input gradients of the two Blocks of level 0; see mbx_fuse_bwd_pair) */
int mbx_embed_bwd_pair(const void* dh_a, const void* dh_b, const float* x, const float* w, float* dw, float* db, float* dpos,
                       float* dtemp, float* dx, int B, int T, int J, int Din, int C, void* ws, void* stream);

/* ---- LayerNorm (nn.LayerNorm, biased variance, eps inside sqrt; DSTformer.py:221-222,230-231,292)
 * x [M,C] f32 -> y [M,C] T, mean [M], rstd [M].  gamma = beta = NULL: y = (x - mean) rstd (see "LayerNorm folded" below) */
int mbx_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, void* y,
                      float* mean, float* rstd, int M, int C, int dtype, void* stream);
/* dx = LN'(dy) [+ dres] [+ extra]  (f32);  dx_t = T copy of dx (or NULL);  dgamma, dbeta [C].
 * ws: >= mbx_layernorm_bwd_ws(C) bytes. */
size_t mbx_layernorm_bwd_ws(int C);
int mbx_layernorm_bwd(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                      const float* dres, const float* extra, float* dx, void* dx_t, float* dgamma, float* dbeta,
                      int M, int C, int dtype, void* ws, void* stream);
/* mbx_layernorm_bwd (T = f32) with the T copy of dx written as operand planes (dx_hi, dx_lo bf16 [M,C]): in the fp32-class mode the next
 * sub-layer's backward reads the gradient of the residual stream as fp32 (dx) and as a split-operand GEMM operand. */
int mbx_layernorm_bwd_planes(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dres,
                             const float* extra, float* dx, void* dx_hi, void* dx_lo, float* dgamma, float* dbeta, int M, int C,
                             void* ws, void* stream);

/* ---- GEMMs on MFMA -------------------------------------------------------------------------
 * acc[M,N] = a[M,K] . w[N,K]^T  (nn.Linear, DSTformer.py:74,76,97,103,295), epilogue per mbx_epilogue.
 * K % 64 == 0 (bf16) / K % 32 == 0 (f32), N % 8 == 0. Unused pointers NULL. */
int mbx_gemm_nt(const void* a, const void* w, const float* bias, int epilogue, void* out_t, void* out2_t,
                float* out_f, const float* resid, const void* aux_t, int M, int N, int K, int dtype, void* stream);
/* dw[N,K] = dy[M,N]^T . a[M,K] (f32);  db[N] = column sums of dy (or NULL).  N % 32 == 0, K % 32 == 0.
 * ws: >= mbx_gemm_tn_ws(M,N,K) bytes: `splits` fp32 partial tiles [N,K] and up to four partial bias rows [N] per split (+ 256), the
 * larger of the f32 and the bf16 launch plan (one workspace serves either dtype).  The token-split count is at most 64 (f32) or 128
 * (bf16), except that since round 6 the bf16 / bf16x3 kernel with 1 or 3 output tiles of 256 x 256 searches up to 256 splits: the
 * workspace, and the rows the column-sum pass reads, can therefore reach 256 (N K + 4 N) floats.  The launcher lays its partials out
 * by the same plan that this size comes from; a smaller buffer is written past its end. */
size_t mbx_gemm_tn_ws(int M, int N, int K);
int mbx_gemm_tn(const void* dy, const void* a, float* dw, float* db, int M, int N, int K, int dtype,
                void* ws, void* stream);

/* ---- LayerNorm folded into the Linear it feeds (bf16 path) ---------------------------------------------------------------
 * Every norm1 / norm2 of a Block feeds exactly one Linear (DSTformer.py:241-249 -> Attention.qkv :143 / MLP.fc1 :80):
 *     Linear(LayerNorm(x)) = xhat . (W diag(gamma))^T + (b + W beta) = xhat . W'^T + b',   xhat = (x - mean) rstd.
 * Forward: mbx_layernorm_fwd / mbx_fuse_ln_fwd with gamma = beta = NULL write xhat as the GEMM operand; the weights come from
 * mbx_fold_norm_weights.  Backward: with rsum[n] = sum_k W'[n,k] the two row means of nn.LayerNorm's backward are row dots of
 * dY with quantities the PRODUCER of dY holds,
 *     c1[m] = mean_k dxhat = (1/C) sum_n dY[m,n] rsum[n],    c2[m] = mean_k dxhat xhat = (1/C) sum_n dY[m,n] (Y[m,n] - b'[n]),
 * so mbx_attn_bwd_stats / mbx_gemm_nt_dgelu_stats emit them as partial sums, mbx_lnbwd_rowc finalises them and
 * mbx_gemm_nt_lnbwd applies  dx = dres [+ extra] + rstd (dY . W' - c1 - xhat c2)  as the epilogue of the dX GEMM: no stand-alone
 * LayerNorm-backward pass, no bf16 round trip of d(xn).  mbx_unfold_norm_grads turns the folded weight gradient into the
 * gradients of W, gamma and beta.  (The final `norm` -> pre_logits path, :350-354, keeps the plain kernels.)
 *
 * mbx_fold_norm_weights: `desc` = n_desc records of 10 x int64 {w f32 [N,K], bias f32 [N] or 0, gamma f32 [K], beta f32 [K],
 *   dst_n bf16 [N,K], dst_t bf16 [K,N] or 0, bias_f f32 [N], rsum f32 [N], N, K}; rsum sums the bf16-ROUNDED folded weights. */
int mbx_fold_norm_weights(const int64_t* desc, int n_desc, int max_n, int max_k, void* stream);
/* MBX_EPI_DGELU + part[N/64][M][2] f32 = per 64-column block and row { sum du rsum, sum du (aux_t - bias_f) } of the rounded
 * output du (rsum, bias_f enter rounded to bf16: packed-bf16 dot products).  bf16; N % 64 == 0, K % 64 == 0. */
int mbx_gemm_nt_dgelu_stats(const void* a, const void* w, void* out_t, const void* aux_t, const float* bias_f,
                            const float* rsum, float* part, int M, int N, int K, void* stream);
/* fc1 + nn.GELU with the DERIVATIVE saved for backward instead of the pre-activation (DSTformer.py:80-81; round 5):
 * out_g = gelu_erf(a . w^T + bias), out_d = gelu_erf'(a . w^T + bias) (from the fp32 accumulator), both bf16 [M,N]; the backward of the
 * activation is then mbx_gemm_nt_mul: out = (a . w^T) * aux.  bf16; N >= 256, N % 8 == 0, K % 64 == 0. */
int mbx_gemm_nt_gelu_d(const void* a, const void* w, const float* bias, void* out_d, void* out_g, int M, int N, int K, void* stream);
int mbx_gemm_nt_mul(const void* a, const void* w, const void* aux, void* out, int M, int N, int K, void* stream);
/* rowc[M][4] f32 = {rstd, rstd c1, rstd c2, 0} from part[nb][M][2] (block-major; nb = 2 x heads, or N/64 column blocks) */
int mbx_lnbwd_rowc(const float* part, int nb, const float* rstd, float* rowc, int M, int C, void* stream);
/* dx[M,N] f32 = dres [+ extra] + rowc.x (a . w^T) - rowc.y - xhat rowc.z;  dx_t = bf16 copy of dx or NULL.
 * a bf16 [M,K] (dY), w bf16 [N,K] (the transposed folded weight), xhat bf16 [M,N].  N % 8 == 0, K % 64 == 0. */
int mbx_gemm_nt_lnbwd(const void* a, const void* w, const void* xhat, const float* rowc, const float* dres,
                      const float* extra, float* dx, void* dx_t, int M, int N, int K, void* stream);
/* The same with the gradient of the residual stream carried as bf16 BETWEEN the four sub-layers of a Block (fp32 at the Block
 * boundaries, fp32 accumulation and arithmetic in the kernel): dres_t bf16 [M,N]; dx f32 or NULL; dx_t bf16 or NULL (at least one
 * of them).  Inside a Block dx_t alone is written -- it is the stream and the next dX / dW GEMMs' operand at once: 4 instead of 12
 * bytes per element and launch.  Numerics: tools/gradstream_numerics.py (every gate of the bf16 path unchanged). */
int mbx_gemm_nt_lnbwd_t(const void* a, const void* w, const void* xhat, const float* rowc, const void* dres_t,
                        const float* extra, float* dx, void* dx_t, int M, int N, int K, void* stream);
/* in place: dw[N,K] (= dY^T xhat, the folded weight gradient) <- gamma[k] dw[n,k] + db[n] beta[k];
 * dgamma[k] = sum_n w[n,k] dw'[n,k];  dbeta[k] = sum_n w[n,k] db[n].  ws: >= mbx_unfold_norm_grads_ws(N,K) bytes. */
size_t mbx_unfold_norm_grads_ws(int N, int K);
int mbx_unfold_norm_grads(float* dw, const float* db, const float* w, const float* gamma, const float* beta,
                          float* dgamma, float* dbeta, int N, int K, void* ws, void* stream);

/* ---- LayerNorm as a raw operand + the fused MLP forward (bf16, no-grad / inference path) -------------------------------------
 * One step beyond the folding above.  With W' = W diag(gamma), b' = b + W beta, rsum[n] = sum_k W'[n,k] (mbx_fold_norm_weights):
 *     Linear(LayerNorm(y)) = rstd (y . W'^T - mean rsum) + b',
 * so the CONSUMER of a residual-stream tensor y (the qkv / fc1 Linear behind norm1 / norm2, DSTformer.py:241-249) multiplies the
 * RAW rows and applies the row constants where its accumulators are: the stand-alone LayerNorm passes of a forward (read fp32 y,
 * write bf16 xhat) disappear.  The consumers read the fp32 rows of y themselves (mbx_rows_gemm_nk_ln, mbx_mlp_fused_fwd with
 * a = NULL, mbx_proj_mlp_fused_fwd) and round the row SHIFTED by its first element, so that the rounding error scales with the
 * spread of the row, not with its magnitude (LayerNorm does not see the shift).
 *
 * mbx_mlp_fused_fwd:   the whole MLP sub-layer of a Block (MLP.forward, DSTformer.py:79-85, inside :242 / :244 / :246 / :248)
 *     y = resid + fc2(gelu_erf(fc1(LN(.)))) in ONE kernel -- the [M, hidden] tensor never exists in HBM:
 *       a        bf16 [M,C]: raw_in = 0: the normalised operand xhat (mbx_layernorm_fwd / mbx_fuse_ln_fwd with gamma = NULL);
 *                            raw_in = 1: bf16(x) itself; mean / rstd of the row are taken in the kernel from these values;
 *                            a = NULL (raw_in = 1): the operand is bf16(resid), rounded in the kernel from the fp32 rows it loads for
 *                            the residual anyway (no second input stream), statistics of the fp32 rows
 *       packed   the fc1 (folded) and fc2 weights in MFMA-fragment order: mbx_mlp_pack_weights(w1 bf16 [hidden,C], w2 bf16 [C,hidden])
 *                -> mbx_mlp_pack_bytes(C, hidden) bytes
 *       b1 [hidden] (folded bias b'), b2 [C], rsum [hidden] (raw_in only), resid f32 [M,C] (= x; may alias y)
 *       y f32 [M,C];  y_t bf16 [M,C] = bf16(y) or NULL;  mean, rstd f32 [M] = LayerNorm statistics of the rows of y (eps) or NULL
 *     C in {256, 512}, hidden % 64 == 0, hidden <= 1536. */
size_t mbx_mlp_pack_bytes(int C, int hidden);
int mbx_mlp_pack_weights(const void* w1, const void* w2, void* packed, int C, int hidden, void* stream);
int mbx_mlp_fused_fwd(const void* a, int raw_in, const void* packed, const float* b1, const float* b2, const float* rsum,
                      const float* resid, float* y, void* y_t, float eps, float* mean, float* rstd, int M, int C, int hidden,
                      void* stream);
/* The attention's proj + residual in front of the MLP, same kernel (DSTformer.py:241-249: x + attn(..) then x + mlp(norm(..)); :103 proj):
 *     y1 = resid + o . Wp^T + bp        y = y1 + fc2(gelu_erf(fc1(LN(y1))))
 * o bf16 [M,C] = the attention output (mbx_attn_fwd); y1 exists only in the accumulator registers: its bf16 rounding is fc1's operand,
 * its LayerNorm statistics are taken from the same registers.  packed: mbx_proj_mlp_pack_weights(wp bf16 [C,C], w1 (folded), w2) ->
 * mbx_proj_mlp_pack_bytes(C, hidden) bytes;  bp [C], b1 [hidden] (folded), b2 [C], rsum [hidden];  y may alias resid. */
size_t mbx_proj_mlp_pack_bytes(int C, int hidden);
int mbx_proj_mlp_pack_weights(const void* wp, const void* w1, const void* w2, void* packed, int C, int hidden, void* stream);
int mbx_proj_mlp_fused_fwd(const void* o, const void* packed, const float* bp, const float* b1, const float* b2, const float* rsum,
                           const float* resid, float* y, float eps, int M, int C, int hidden, void* stream);

/* ---- "row owner" NT GEMMs (bf16; csrc/gemm_rows.hip) -----------------------------------------------
 * The same Linear layers (DSTformer.py:97 qkv, :69 fc1; the input gradients of :70 fc2 and :103 proj) on a kernel whose workgroup
 * owns 128 complete token rows: the token operand lives in registers, the weights stream as pre-packed MFMA fragments.
 * mbx_rows_pack_nk: w bf16 [N,K] row-major -> packed (mbx_rows_pack_bytes(N, K) bytes); K in {256, 512}, N % 64 == 0.
 * mbx_rows_gemm_nk: out bf16 [M,N] = a . w^T + bias (bias may be NULL);  with mean != NULL the raw-operand LayerNorm form of
*                   Linear: out = rstd[m] (a . w^T - mean[m] rsum[n]) + bias[n].
 * mbx_rows_gemm_nk_ln: the same from the fp32 rows x [M,K] of the residual stream themselves: operand bf16(x) rounded in the kernel,
 *                   (mean, rstd) of every row taken from the same loads (eps as in nn.LayerNorm): Linear(LayerNorm(x)) without a
 *                   LayerNorm pass and without a bf16 copy of x (norm1 + attn.qkv of a Block, DSTformer.py:241-249 / :139-143). */
size_t mbx_rows_pack_bytes(int N, int K);
int mbx_rows_pack_nk(const void* w, void* packed, int N, int K, void* stream);
int mbx_rows_gemm_nk(const void* a, const void* packed, const float* bias, const float* rsum, const float* mean, const float* rstd,
                     void* out, int M, int N, int K, void* stream);
int mbx_rows_gemm_nk_ln(const float* x, const void* packed, const float* bias, const float* rsum, float eps, void* out, int M, int N,
                        int K, void* stream);

/* g = gelu_erf(u), T-typed, n % 4 == 0: rebuilds the MLP's post-activation from the saved pre-activation in the engine's
 * low-memory (recompute) mode (nn.GELU, DSTformer.py:70,80-81). */
int mbx_gelu_fwd(const void* u, void* g, size_t n, int dtype, void* stream);

/* ---- fp32-class split-operand GEMMs (precision 'bf16x3') ------------------------------------------
 * The north-star gate (outputs within 1e-3 of the fp32 reference, BASELINE.json) cannot be met with bf16 operands and
 * gfx950 has no TF32: every fp32 operand x is split into two bf16 planes, hi = bf16(x), lo = bf16(x - hi), and
 * a.w^T = a_hi.w_hi^T + a_hi.w_lo^T + a_lo.w_hi^T runs as three bf16 MFMA passes into ONE fp32 accumulator (products
 * of bf16 are exact in fp32; the dropped lo.lo term is 2^-16 relative).  Same arithmetic sites as mbx_gemm_nt / mbx_gemm_tn;
 * every T-typed tensor (out_t, out2_t, aux_t) is fp32.  K % 64 == 0, N % 8 == 0. */
int mbx_split_bf16(const float* x, void* hi, void* lo, size_t n, void* stream);   /* n % 4 == 0 */
int mbx_gemm_nt_x3(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias, int epilogue,
                   float* out_t, float* out2_t, float* out_f, const float* resid, const float* aux_t, int M, int N, int K,
                   void* stream);
/* The same with the LAST output of the epilogue written as the two bf16 planes of the operand split (hi = bf16(v), lo = bf16(v - hi),
 * the arithmetic of mbx_split_bf16) instead of fp32 -- for outputs whose only reader is another split-operand GEMM (the MLP's
 * activation, DSTformer.py:80-83, and its gradient): MBX_EPI_STORE (planes = out), MBX_EPI_GELU (out_t = pre-activation f32 or NULL,
 * planes = gelu), MBX_EPI_DGELU (planes = acc * gelu'(aux_t)). */
int mbx_gemm_nt_x3p(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias, int epilogue,
                    float* out_t, void* pl_hi, void* pl_lo, const float* aux_t, int M, int N, int K, void* stream);
/* mbx_layernorm_fwd (T = f32) with y written as the operand planes (y_hi, y_lo bf16 [M,C]) of the Linear that follows. */
int mbx_layernorm_fwd_planes(const float* x, const float* gamma, const float* beta, float eps, void* y_hi, void* y_lo, float* mean,
                             float* rstd, int M, int C, void* stream);
/* ws of mbx_gemm_tn_x3: exactly splits x (N K + 4 N) floats + 256 bytes, from the launch plan that the launcher follows.  The split
 * count is bounded as for bf16 (mbx_gemm_tn_ws): up to 128, and up to 256 where the round-6 search runs (1 or 3 output tiles). */
size_t mbx_gemm_tn_x3_workspace(int M, int N, int K);
int mbx_gemm_tn_x3(const void* dy_hi, const void* dy_lo, const void* a_hi, const void* a_lo, float* dw, float* db, int M,
                   int N, int K, void* ws, void* stream);

/* ---- attention core (DSTformer.py:178-200), qkv [M,3C] T with channel order [3][H][hd] --------
 * o [M,C] T (heads concatenated), lse [M,H] f32 = log-sum-exp of the scaled scores.
 * hd = C/H must be 32 or 64; J <= 32.  Any T: sequences longer than 256 run the streamed kernels (K / V or Q / dO through LDS in
 * 64-row tiles) -- every entry below, all forms included; a shape whose launch grid exceeds 2^31 workgroups is refused. */
int mbx_attn_fwd(const void* qkv, void* o, float* lse, int B, int T, int J, int H, int hd, float scale,
                 int mode, int dtype, void* stream);
/* mbx_attn_fwd with nn.Dropout(p) on the probabilities (attn_drop, DSTformer.py:96,182,196): o = (mask P / (1 - p)) V with the
 * softmax statistics (and lse) of the undropped probabilities.  The mask is counter-based: element (query i, key j) of a
 * problem survives iff keep(flat index of that element in the reference's attn tensor -- [B T, H, J, J] spatial,
 * [B, H, J, T, T] temporal --, p, seed), motionbert_amd/dropmask.py.  0 <= p < 1; p = 0 is mbx_attn_fwd. */
int mbx_attn_fwd_drop(const void* qkv, void* o, float* lse, int B, int T, int J, int H, int hd, float scale,
                      int mode, int dtype, float p, uint64_t seed, void* stream);
/* dqkv [M,3C] T from do [M,C] T; probabilities are recomputed from q, k and lse. */
int mbx_attn_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, int B, int T,
                 int J, int H, int hd, float scale, int mode, int dtype, void* stream);
/* backward of mbx_attn_fwd_drop (same p and seed; o is the dropped forward output): dP = mask (dO V^T) / (1 - p), dV from the
 * dropped probabilities, dS = P (dP - rowsum(dO o)). */
int mbx_attn_bwd_drop(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, int B, int T,
                      int J, int H, int hd, float scale, int mode, int dtype, float p, uint64_t seed, void* stream);
/* mbx_attn_bwd / mbx_attn_bwd_drop of the fp32 kernels (precision 'bf16x3') with dq | dk | dv written as the two bf16 planes of the
 * operand split (dqkv_hi, dqkv_lo [M,3C]) instead of fp32: their only readers are the split-operand GEMMs of qkv's backward.  p = 0:
 * no dropout. */
int mbx_attn_bwd_planes(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv_hi, void* dqkv_lo, int B, int T,
                        int J, int H, int hd, float scale, int mode, float p, uint64_t seed, void* stream);
/* mbx_attn_bwd (bf16) + part[2H][M][2] f32 = per (head, role, token) { sum dqkv rsum, sum dqkv (qkv - bias_f) } of the rounded
 * output over the head's q columns (role 0) and over its k and v columns (role 1) (LayerNorm folding, above; nb = 2H for
 * mbx_lnbwd_rowc; rsum, bias_f f32 [3C], entering rounded to bf16).  part must be 8-byte aligned. */
int mbx_attn_bwd_stats(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, const float* bias_f,
                       const float* rsum, float* part, int B, int T, int J, int H, int hd, float scale, int mode, void* stream);

/* ---- adaptive fusion of the two streams (DSTformer.py:343-349) -------------------------------
 * alpha = softmax(w . cat[x_st, x_ts] + b)  [M,2];  out = x_st*alpha0 + x_ts*alpha1.  w [2,2C], b [2]. */
int mbx_fuse_fwd(const float* x_st, const float* x_ts, const float* w, const float* b, float* out, float* alpha,
                 int M, int C, void* stream);
/* mbx_fuse_fwd plus the LayerNorm(s) that read its output (next level's Block.norm1_s / norm1_t, DSTformer.py:241,247, or the
 * final norm, :350): xn1 = LN(out; g1, b1), optionally xn2 = LN(out; g2, b2) (g2 = b2 = xn2 = NULL: one consumer), both T-typed,
 * sharing mean / rstd [M].  Same arithmetic as mbx_fuse_fwd followed by mbx_layernorm_fwd. */
int mbx_fuse_ln_fwd(const float* x_st, const float* x_ts, const float* w, const float* b, float* out, float* alpha,
                    const float* g1, const float* b1, void* xn1, const float* g2, const float* b2, void* xn2, float eps,
                    float* mean, float* rstd, int M, int C, int dtype, void* stream);
/* backward: d_st / d_ts f32 [M,C] and their T-typed copies d_st_t / d_ts_t; d_st = d_ts = NULL writes the T-typed copies only
 * (the gradient stream in the operand type, see mbx_gemm_nt_lnbwd_t) */
size_t mbx_fuse_bwd_ws(int C);
int mbx_fuse_bwd(const float* dh, const float* x_st, const float* x_ts, const float* alpha, const float* w,
                 float* d_st, float* d_ts, void* d_st_t, void* d_ts_t, float* dw, float* db, int M, int C,
                 int dtype, void* ws, void* stream);
/* mbx_fuse_bwd with dh = dh_a + dh_b, both bf16 [M,C]: the input gradients of the two Blocks of the level above, as their row-owner
 * LayerNorm-backward kernels (mbx_rows_lnbwd_t) leave them (round 5: the gradient of the residual stream in the operand type across
 * Block boundaries too).  bf16 outputs only (d_st_t, d_ts_t); ws as mbx_fuse_bwd. */
int mbx_fuse_bwd_pair(const void* dh_a, const void* dh_b, const float* x_st, const float* x_ts, const float* alpha, const float* w,
                      void* d_st_t, void* d_ts_t, float* dw, float* db, int M, int C, void* ws, void* stream);
/* att_fuse=False variant (DSTformer.py:351): out = (x_st + x_ts)/2 and its backward */
int mbx_average(const float* x_st, const float* x_ts, float* out, size_t n, void* stream);
int mbx_average_bwd(const float* dh, float* d_st, float* d_ts, void* d_st_t, void* d_ts_t, size_t n, int dtype,
                    void* stream);

/* ---- tail: head Linear(R -> Dout<=8) (DSTformer.py:300,357) and tanh' ---------------------------- */
int mbx_head_fwd(const float* rep, const float* w, const float* b, float* out, int M, int R, int Dout, void* stream);
size_t mbx_head_bwd_ws(int R, int Dout);
/* dpre_t = (dout . w) * (1 - rep^2) (T);  dw [Dout,R];  db [Dout] */
int mbx_head_bwd(const float* dout, const float* rep, const float* w, void* dpre_t, float* dw, float* db,
                 int M, int R, int Dout, int dtype, void* ws, void* stream);
int mbx_tanh_bwd(const float* drep, const float* rep, void* dpre_t, size_t n, int dtype, void* stream);

/* ---- the training step around the backbone (train.py:174-206,289) -----------------------------
 * Fused 3D pose loss of train.py:176-189 with the lambdas of configs/pose3d/MB_train_h36m.yaml:36-43 that are non-zero:
 *   total = loss_mpjpe + lambda_scale * n_mpjpe + lambda_velocity * loss_velocity        (lib/model/loss.py:56-62,81-91,133-142)
 * pred, gt [B,T,J,3] f32.  losses[4] = {mpjpe, n_mpjpe, velocity, total} stay on the device (the reference synchronises with
 * eight .item() calls per step).  dpred (or NULL) = grad_scale * d total / d pred, the cotangent to hand to backward.
 * ws: >= mbx_pose_loss_ws(B,T) bytes. */
size_t mbx_pose_loss_ws(int B, int T);
int mbx_pose_loss(const float* pred, const float* gt, float lambda_scale, float lambda_velocity, float* losses, float* dpred,
                  float grad_scale, int B, int T, int J, void* ws, void* stream);
/* All seven 3D losses of train.py:177-199 and the weighted total of :185-191:
 *   total = loss_mpjpe + lambda_scale * n_mpjpe + lambda_velocity * loss_velocity + lambda_lv * loss_limb_var
 *           + lambda_lg * loss_limb_gt + lambda_a * loss_angle + lambda_av * loss_angle_velocity    (lib/model/loss.py:98-203)
 * losses[8] = {mpjpe, n_mpjpe, velocity, lv, lg, angle, angle_velocity, total}, the reference's log order; dpred (or NULL) =
 * grad_scale * d total / d pred.  J must be 17: the 16 limbs and 18 limb pairs are those of the H36M skeleton.  The first three terms are
 * the arithmetic of mbx_pose_loss: with the four new lambdas 0, losses[{0,1,2,7}] and dpred equal its outputs bit for bit.
 * ws: >= mbx_pose_loss_full_ws(B,T) bytes. */
size_t mbx_pose_loss_full_ws(int B, int T);
int mbx_pose_loss_full(const float* pred, const float* gt, float lambda_scale, float lambda_velocity, float lambda_lv, float lambda_lg,
                       float lambda_a, float lambda_av, float* losses, float* dpred, float grad_scale, int B, int T, int J, void* ws,
                       void* stream);
/* 2D re-projection loss of the pre-training's 2D branch (lib/model/loss.py:72-77 loss_2d_weighted, train.py:200-203):
 * loss[1] = mean |(pred_xy - target_xy) * conf| and, if dpred != NULL, dpred [B,T,J,3] = grad_scale * d loss / d pred (z row 0).
 * pred [B,T,J,3] f32; target: x, y at target[tok * target_stride + {0,1}]; conf at conf[tok * conf_stride] -- with strides 3 / 3
 * the [B,T,J,3] 2D batch itself is target and (channel 2) confidence.  ws: >= mbx_loss_2d_weighted_ws(B,T) bytes. */
size_t mbx_loss_2d_weighted_ws(int B, int T);
int mbx_loss_2d_weighted(const float* pred, const float* target, int target_stride, const float* conf, int conf_stride, float* loss,
                         float* dpred, float grad_scale, int B, int T, int J, void* ws, void* stream);
/* AdamW (torch.optim.AdamW semantics, train.py:289) over ONE flat fp32 buffer -- or one contiguous RANGE of it -- of n
 * parameters, one launch.  p, g, m, v are parallel buffers: 4-byte aligned, same offset within a 16-byte line (a range that
 * skips frozen parameters, learning.py:69-77 / train.py:284-289, need not start on a 16-byte boundary).
 * state[2] on the device = {step count, learning rate}; tick != 0 advances the step count first (once per optimizer step). */
int mbx_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float* state, float beta1, float beta2, float eps,
                   float weight_decay, int tick, void* stream);

/* ---- ActionNet pooling on the representation (lib/model/model_action.py:15-24,62-70) ---------------
 * rep [N*Mp*T*J, R] f32 (token order ((n Mp + m) T + t) J + j) -> pooled [N, J, R] = mean over persons and frames of the
 * element-wise dropped-out representation (p = dropout_ratio, 0 in evaluation; the keep mask is a counter-based hash of
 * (seed, element index), reproduced in backward, never stored). */
int mbx_pool_rep_fwd(const float* rep, float* pooled, int N, int Mp, int T, int J, int R, float p, uint64_t seed, void* stream);
/* dpre_t [tokens, R] T = broadcast(dpooled) / (Mp T) * keep / (1-p) * (1 - rep^2): the tail's tanh' (DSTformer.py:296) fused
 * with the backward of both means and of the dropout; the [N,Mp,T,J,R] cotangent is never materialised. */
int mbx_tanh_pool_bwd(const float* dpooled, const float* rep, void* dpre_t, int N, int Mp, int T, int J, int R, float p,
                      uint64_t seed, int dtype, void* stream);

/* ---- Dropout / DropPath with p > 0 in training (DSTformer.py:77,96,104,278; lib/model/drop.py:17-32) ------
 * Counter-based masks keep(seed, flat element index), recomputed in backward from the seed.
 * mbx_dropout: y = x * keep/(1-p) (in place allowed); T-typed by `dtype`; also the backward of itself. */
int mbx_dropout(const void* x, void* y, size_t n, float p, uint64_t seed, int dtype, void* stream);
/* y [rows,C] f32 holds x + branch (fused RESID epilogue): y <- x + branch * keep_e/(1-p) * keep_path/(1-p_path); DropPath draws
 * one value per `rows_per_sample` consecutive rows (drop.py:27: per leading index of the [B*T, J, C] tensor -> J). */
int mbx_residual_drop(float* y, const float* x, size_t rows, int C, int rows_per_sample, float p, uint64_t seed, float p_path,
                      uint64_t seed_path, void* stream);
/* dy_t [rows,C] T = dy * the same two masks: the gradient entering that branch. */
int mbx_grad_drop(const float* dy, void* dy_t, size_t rows, int C, int rows_per_sample, float p, uint64_t seed, float p_path,
                  uint64_t seed_path, int dtype, void* stream);

/* ---- the input stage on the device ---------------------------------------------------------------
 * Augmenter2D.add_noise (flags bit 0) and add_mask (bit 1) of lib/data/augmentation.py:29-81 in one kernel: x [B,T,J,Cin]
 * (Cin 2 or 3; only x, y are read when noise is on, as in the reference) -> y [B,T,J,3].  noise_mean / noise_std [J,2] and
 * noise_weight [J] are params/synthetic_noise.pth, d2c_* params/d2c_params.pkl, uniform_range 0.06, jitter_std 0.002 (:20,35),
 * mask ratios MB_pretrain.yaml:49-50.  Counter-based random numbers from `seed` (oracle/augment_oracle.py restates every draw). */
int mbx_augment2d(const float* x, float* y, int B, int T, int J, int Cin, const float* noise_mean, const float* noise_std,
                  const float* noise_weight, float uniform_range, float jitter_std, float d2c_a, float d2c_b, float d2c_m,
                  float d2c_s, float mask_ratio, float mask_T_ratio, int flags, uint64_t seed, void* stream);
/* flip test-time augmentation (train.py:67-72; lib/utils/utils_data.py:54-66): embedding of 2B samples from x [B,T,J,Din], sample
 * B+b = flip_data(x[b]) as an index remap (perm[j] = the joint whose values joint j takes; channel 0 negated); and the
 * flip-back + average of the [2B,T,J,D] output -> out [B,T,J,D]. */
int mbx_embed_fwd_tta(const float* x, const int* perm, const float* w, const float* b, const float* pos, const float* temp,
                      float* h, int B, int T, int J, int Din, int C, void* stream);
int mbx_flip_average(const float* out2, const int* perm, float* out, int B, int T, int J, int D, void* stream);

/* ---- evaluation on the device: Protocol #1 / #2 errors of train.py:56-153 (csrc/pose_eval.hip) ----------------------------------------
 * mbx_pose_errors: per frame of pred [N,T,J,3] f32 (the raw network output, normalised image coordinates) against gt [N,T,J,3] f32
 * (the dataset's joints_2.5d_image), in the reference's order:
 *   rootrel != 0: pred[:,:,0,:] = 0 (train.py:75-76);   gt_2d != 0: pred[...,:2] = x[...,:2] (train.py:80-81; x [N,T,J,x_channels>=2] f32,
 *   the model input; read only then);   hw != NULL ([N,2] f32 = (res_w, res_h) per clip, DataReaderH36M.get_hw()): xy = (xy + [1, h/w]) w/2,
 *   z = z w/2 (datareader_h36m.py:125-136);   factor != NULL ([N,T] f32, 2.5d_factor): pred *= factor (train.py:118-121);
 *   both poses minus their joint 0 (train.py:124-125);
 *   e1 = mean_j |p_j - g_j|                                                                   (lib/model/loss.py:8-14   mpjpe)
 *   e2 = mean_j |a p_j R + t - g_j|, (a, R, t) the optimal similarity transform of p onto g    (lib/model/loss.py:16-51  p_mpjpe)
 * e1, e2 [N,T] f64; all arithmetic after the f32 loads is f64.  The 3x3 decomposition is a fixed 8 sweeps of cyclic Jacobi on H^T H
 * with the third singular vectors taken as cross products (planar poses are fine; no data-dependent loop, terminates on NaN input).
 * Accuracy of e2, in the singular values s0 >= s1 of H = X0^T Y0 (centred gt, centred pred): 1e-10 relative against a LAPACK SVD where
 * s1 / s0 >= 1e-3, which every human pose is; for a needle-shaped pose below that the roll about the needle's axis degrades and e2 is
 * off by at most (2 s1 |X0| + 2 min(|X0_T|, a |Y0_T|)) / sqrt(J), the transverse extents (csrc/pose_solve.h); a pose exactly on a line
 * and J = 2 (H of rank one) give the reference's value to rounding.  e2 is finite for every pair of finite poses of non-zero extent.
 * 1 < J <= 64.  pred / gt / x need 4-byte alignment only.  A frame whose pred or gt has zero extent (all joints equal) gives e2 = NaN,
 * the reference's 0/0; a non-finite e1 is dropped by mbx_eval_reduce as the reference's `e1_all[idx] > 0` drops it. */
int mbx_pose_errors(const float* pred, const float* gt, const float* hw, const float* factor, const float* x, int x_channels, int rootrel,
                    int gt_2d, double* e1, double* e2, int N, int T, int J, void* stream);
/* mbx_eval_reduce: the aggregation of train.py:100-149.  e1, e2 [n_err] f64 (n_err = N T slots, slot = clip * T + frame in clip);
 * CSR over the F test frames: row_ptr [n_row_ptr = F + 1] i32, slots [nnz] i32 = the slots that cover test frame f, in clip order
 * (the host leaves out the clips of blocked sources, train.py:109-115); action [F] i32 in [0, A).
 *   frame mean   m(f) = sum over its slots / their number; f is left out when it has no slot or m1(f) is not > 0 (train.py:131-137)
 *   per_action [2,A] f64 = mean of m1 / m2 over the frames of the action that are left in;  count [A] i32 = their number
 *   summary [2] f64      = mean of per_action over the A actions (train.py:148-149)
 * An action without a frame left in gives NaN (np.mean of an empty list), and so does the summary then.  Every sum runs in a fixed
 * order and there are no floating-point atomics: two calls on the same inputs give the same bits.  Slot indices outside [0, n_err)
 * and row bounds outside [0, nnz] are ignored, never followed.  ws: >= mbx_eval_reduce_ws(F, A) bytes. */
size_t mbx_eval_reduce_ws(int F, int A);
int mbx_eval_reduce(const double* e1, const double* e2, int n_err, const int* row_ptr, int n_row_ptr, const int* slots, int nnz,
                    const int* action, int F, int A, double* per_action, double* summary, int* count, void* ws, void* stream);

/* ---- "N-resident" row-owner GEMM with the LayerNorm backward as its epilogue (bf16; csrc/gemm_rows_n.hip; round 5) ---------------------
 * The input gradient of a folded (LayerNorm -> Linear) pair INSIDE a Block (DSTformer.py:241-249: norm1 -> attn.qkv :143, norm2 ->
 * mlp.fc1 :80; backward by autograd in the reference) in one launch, without row dots from the producers of dY:
 *     dxhat = dy . w^T   (dy bf16 [M,K], w bf16 [512,K] = mbx_fold_norm_weights' transposed folded weight, packed by mbx_rows_n_pack_many)
 *     dx_t  = bf16( dres_t + rstd (dxhat - mean_k dxhat - xhat mean_k(dxhat xhat)) )          all [M,512]
 * A workgroup owns 128 complete rows (256 accumulator registers per wave), so both row means come from the accumulators; xhat bf16
 * [M,512] and rstd f32 [M] are what mbx_layernorm_fwd (gamma = NULL) left, dres_t / dx_t the gradient of the residual stream in the
 * operand type (as mbx_gemm_nt_lnbwd_t with dx = NULL).  N = 512 (K >= 512) or, round 6, N = 256 (dim_feat of MotionBERT-Lite; 128
 * accumulator registers per wave, K >= 256), K % 256 == 0; M * N * 2 < 2^32 and M * K * 2 < 2^32 (32-bit lane offsets into dx_t / dy; checked).  dx_t must not alias
 * an input (checked for dres_t, xhat and dy).  Round 6: xhat is fetched by LDS-DMA during the last trip of the loop, in the 26 slots in
 * which the weight stream has nothing left to request (csrc/gemm_rows_n.hip). */
size_t mbx_rows_n_pack_bytes(int N, int K);
/* packs n_desc operands in ONE launch (a training step re-packs 60 weights): record r of desc = {w bf16 [N,K_r], packed_r
 * (mbx_rows_n_pack_bytes(N, K_r) bytes), K_r} (3 x int64, device memory); N = 512 or 256 for all of them; max_k = the largest K_r; every
 * K_r % 256 == 0 and >= 512 (N = 512) / >= 256 (N = 256) (the caller's responsibility: the records live on the device). */
int mbx_rows_n_pack_many(const int64_t* desc, int n_desc, int N, int max_k, void* stream);
int mbx_rows_lnbwd_t(const void* dy, const void* packed, const void* xhat, const float* rstd, const void* dres_t, void* dx_t, int M,
                     int N, int K, void* stream);
/* The FORWARD residual GEMM of a sub-layer that is followed by a LayerNorm, on the same row-owner shape (proj / fc2 + residual,
 * DSTformer.py:241-249, and the next norm1 / norm2): y = resid + a . w^T + bias (fp32 [M,512]); xhat = (y - mean(y)) rstd(y) (bf16 [M,512],
 * the plain normalisation: gamma and beta live in the folded weights of the Linear the LayerNorm feeds), mean / rstd fp32 [M] (two-pass
 * statistics of the fp32 rows, eps inside the square root).  packed = mbx_rows_n_pack_many's image of w [N,K].  bf16; N = 512 (K >= 512) or
 * 256 (K >= 256), K % 256 == 0, M * N * 4 < 2^32, M * K * 2 < 2^32 (checked).  y must not alias resid and xhat must not alias a (checked): rows past M are computed from row M - 1's
 * inputs and stored onto row M - 1 again, which is only harmless while those inputs are still the original ones. */
int mbx_rows_resid_ln(const void* a, const void* packed, const float* bias, const float* resid, float* y, void* xhat, float* mean,
                      float* rstd, float eps, int M, int N, int K, void* stream);

/* ---- one-shot action recognition (csrc/oneshot.hip; train_action_1shot.py:58-69,186-198, lib/model/loss_supcon.py:57-98) ----------------
 * mbx_supcon_loss: SupConLoss.forward(features, labels) with contrast_mode 'all' and its gradient in one call.  feat f32
 * [bsz, n_views, D], labels i32 [bsz]; A = bsz * n_views anchors, row r carries labels[r / n_views].  With S_ij = x_i . x_j / tau,
 * m_i = max_j S_ij (diagonal included), lse_i = log sum_{j != i} exp(S_ij - m_i), P(i) = {j != i : label_j = label_i}, n_i = |P(i)|:
 *     loss[0] = mean_i -(tau / tau_b) (1 / n_i) sum_{j in P(i)} (S_ij - m_i - lse_i)
 *     dfeat   = grad_scale * d loss / d feat   (NULL: not computed; the loss has the same bits either way)
 * normalize != 0: feat is the embedding BEFORE F.normalize; x = z / max(|z|, 1e-12) and dfeat is the gradient with respect to z.
 * An anchor without a positive gives NaN in the loss and in every element of dfeat, as the reference's 0 / 0 does.
 * 2 <= A <= 128, D >= 1, temperatures > 0 (checked).  fp32 arithmetic, fixed summation order, no floating-point atomics.
 * ws: >= mbx_supcon_loss_ws(A, D) bytes. */
size_t mbx_supcon_loss_ws(int A, int D);
int mbx_supcon_loss(const float* feat, const int* labels, int bsz, int n_views, int D, float temperature, float base_temperature,
                    int normalize, float grad_scale, float* loss, float* dfeat, void* ws, void* stream);
/* mbx_nn_cosine: for every test row t [N,D] the exemplar a [M,D] of the largest (a . t) / (max(|a|, 1e-8) max(|t|, 1e-8)); ties go to
 * the lowest index and NaN counts as maximal, the first NaN winning (torch.argmax).  pred_label[t] = anchor_labels[argmax] (i32),
 * best_sim[t] (f32, may be NULL), hits[0] += #(pred_label == test_labels) (i64, integer atomic; test_labels may be NULL).
 * Any M >= 1 (exemplars are streamed in tiles), any D >= 1, N = 0 is a no-op.
 * There is no workspace argument, so the norms are not kept between workgroups: a workgroup (32 test rows) forms the norm of an exemplar
 * once per exemplar tile and the norms of its test rows once per tile, from the elements it stages for the dots anyway (one fma per staged
 * element); with M > 32 it reads its test rows once per tile of 32 exemplars. */
int mbx_nn_cosine(const float* anchors, const int* anchor_labels, int M, const float* test, const int* test_labels, int N, int D,
                  int* pred_label, float* best_sim, long long* hits, void* stream);

/* ---- mesh recovery around a user-supplied SMPL layer (csrc/mesh.hip; lib/model/model_mesh.py:57-79, loss_mesh.py:49-68, ------------------
 *      lib/utils/utils_mesh.py) -- mbx_version() >= 110
 * mbx_rot6d_theta_fwd: the head's rotation chain for M joints, one thread per joint, fp32.  x6 [M,6] f32, row = the reference's
 * view(-1,3,2): (a1x, a2x, a1y, a2y, a1z, a2z).
 *   rotmat [M,9] (row-major 3x3, or NULL) = rot6d_to_rotmat (utils_mesh.py:316-330): b1 = a1 / max(|a1|, 1e-6),
 *       b2 = u / max(|u|, 1e-6) with u = a2 - (b1 . a2) b1, b3 = b1 x b2, R = [b1 b2 b3] by columns;
 *   aa [M,3] (or NULL) = rotation_matrix_to_angle_axis(rotmat) (:54-83) along the reference's own path: the TRANSPOSED matrix of
 *       rotation_matrix_to_quaternion, its four mask cases with eps = 1e-6, q = 0.5 q_case / sqrt(t_case), then quaternion_to_angle_axis:
 *       2 theta = 2 atan2(-sin, -cos) where cos < 0 and 2 atan2(sin, cos) otherwise, k = 2 theta / sin, k = 2 where sin^2 == 0, NaN -> 0.
 * mbx_rot6d_theta_bwd: dx6 [M,6] = the cotangents drotmat [M,9] and daa [M,3] (either may be NULL: zero) pulled back to x6.  The forward
 * is recomputed in registers.  It is the gradient autograd gives the reference: through the selected quaternion case only and through
 * both normalisations (above and below their clamp).  ONE deviation: where sin^2 == 0 (an exact identity) the reference's autograd
 * returns NaN for the whole joint (0 * inf through the unselected 2 theta / sin); here the continuous extension d aa = 2 d q_xyz is used.
 * An element of aa that the NaN rule set to 0 passes no gradient.  dx6 must not alias x6.  Rows need 4-byte alignment only. */
int mbx_rot6d_theta_fwd(const float* x6, float* rotmat, float* aa, int M, void* stream);
int mbx_rot6d_theta_bwd(const float* x6, const float* drotmat, const float* daa, float* dx6, int M, void* stream);
/* mbx_mesh_param_loss: the three parameter terms of MeshLoss.forward (loss_mesh.py:49-68) and their gradient in one call.  pred_theta,
 * gt_theta [F,82] f32 = 24 axis-angle joints | 10 shape coefficients.  loss_type 0 = MSE, 1 = L1 (the shipped configs).
 *   losses[0] loss_pose  = mean over F*24*9 of (R_p - R_g)^2 or |R_p - R_g|, R = batch_rodrigues (utils_mesh.py:8-51: |a + 1e-8| as the
 *                          angle, the quaternion normalised once more in quat2mat) of both pose vectors
 *   losses[1] loss_shape = mean over F*10 of the shape difference, by the same loss_type
 *   losses[2] loss_norm  = mean over frames of |pred_theta|_2 (all 82 elements)
 *   losses[3]            = lambda_pose * loss_pose + lambda_shape * loss_shape + lambda_norm * loss_norm
 *   dtheta [F,82] (or NULL) = grad_scale * d losses[3] / d pred_theta; the L1 subgradient at a zero difference is 0 (torch's sign)
 * It takes theta rather than rotation matrices because the evaluation feeds it flip-averaged thetas.  fp32; a workgroup leaves three
 * partial sums and one finishing launch adds them in workgroup order.  ws: >= mbx_mesh_param_loss_ws(F) bytes. */
size_t mbx_mesh_param_loss_ws(int F);
int mbx_mesh_param_loss(const float* pred_theta, const float* gt_theta, int loss_type, float lambda_pose, float lambda_shape,
                        float lambda_norm, float grad_scale, float* losses, float* dtheta, int F, void* ws, void* stream);
/* mbx_mesh_errors: per frame, in the order of compute_error / evaluate_mesh (utils_mesh.py:333-438), fp64 after the f32 loads.
 * verts_p, verts_g [F,V,3] f32 (both NULL: row 0 is NaN, for callers that only have joints), kp_p, kp_g [F,17,3] f32, err [5,F] f64:
 *   err[0] MPVE            mean over vertices of |(v_p - kp_p[0]) - (v_g - kp_g[0])|
 *   err[1] MPJPE, 17 joints, both sides minus their joint 0          ('mpjpe_17j')
 *   err[2] MPJPE, the 14 joints h36m_17_to_14 = (1..6, 8, 10..16)    ('mpjpe')
 *   err[3] PA-MPJPE, 17 joints: after rigid_align's similarity transform of the prediction onto the target   ('pa_mpjpe_17j')
 *   err[4] PA-MPJPE, 14 joints                                       ('pa_mpjpe')
 * One workgroup per frame streams the vertices with 4-byte loads (frame bases need no more alignment).  The 3x3 decomposition is the
 * fixed-sweep Jacobi of mbx_pose_errors (csrc/pose_solve.h), with its accuracy: rows 3 / 4 agree with the reference to 1e-10 relative
 * where s1 / s0 >= 1e-3, within the transverse extent of the thinner pose below that, and are finite down to rank one.  A frame whose predicted joints have zero extent gives NaN in rows 3 / 4
 * as the reference's 0 / 0 does; a target of zero extent alone gives the reference's scale 0.  1 <= V. */
int mbx_mesh_errors(const float* verts_p, const float* verts_g, const float* kp_p, const float* kp_g, double* err, int F, int V,
                    void* stream);

/* ---- the SMPL body model (csrc/smpl.hip; linear blend skinning as smplx.lbs.lbs evaluates it) -- mbx_version() >= 120 -------------------
 * Model (all f32 on the device but `parents`): v_template [V,3], shapedirs [V,3,10], posedirs [207,3V] (column 3v+c; rows = the row-major
 * flattening of R_1..R_23 - I), Jt [24,3] = J_regressor . v_template and Jd [24,3,10] = J_regressor . shapedirs (folded by the caller),
 * parents: 24 ints ON THE HOST, parents[0] = -1 and 0 <= parents[j] < j, lbs_weights [V,24], Q [K,V] (a joint regressor, K <= 32, or NULL
 * with K = 0), packed_t [3V,224] from mbx_smpl_pack = [posedirs^T | shapedirs | 0].
 * Forward, per frame (betas [F,10], rotmat [F,24,9] row-major, global orientation first):
 *   J_j = Jt_j + Jd_j beta;  Grot_0 = R_0, Gt_0 = J_0;  Grot_j = Grot_p R_j, Gt_j = Grot_p (J_j - J_p) + Gt_p;  A_j = [Grot_j | Gt_j - Grot_j J_j]
 *   vp_v = v_template_v + shapedirs_v beta + posedirs[:, 3v:3v+3]^T vec(R_1 - I, ..., R_23 - I);  T_v = sum_j w_vj A_j;  x_v = T_v [vp_v; 1]
 *   verts [F,V,3] = scale x;  kp [F,K,3] = scale Q x;  joints [F,24,3] = scale Gt.   Each output may be NULL (not all three).
 * Backward: dverts [F,V,3], dkp [F,K,3], djoints [F,24,3] (each may be NULL: zero) pulled back to drotmat [F,24,9] and dbetas [F,10]; only
 * betas and rotmat are read again, every per-vertex value is recomputed.  Nothing of size [F,V,...] but verts touches global memory.
 * fp32, fixed summation order, no float atomics (tile / split partials and finishing launches).  ws: >= mbx_smpl_fwd_ws(F, V, K with kp,
 * else 0) / mbx_smpl_bwd_ws(F, V, K) bytes, 16-byte aligned; ws_bytes is checked.  F = 0 is a no-op.  Refused: V < 1, K > 32, parents that
 * are not a forward-ordered tree, an undersized workspace. */
int mbx_smpl_pack(const float* shapedirs, const float* posedirs, float* packed_t, int V, void* stream);
size_t mbx_smpl_fwd_ws(int F, int V, int K);
size_t mbx_smpl_bwd_ws(int F, int V, int K);
int mbx_smpl_fwd(const float* v_template, const float* shapedirs, const float* posedirs, const float* Jt, const float* Jd,
                 const int* parents, const float* lbs_weights, const float* Q, int K, const float* betas, const float* rotmat,
                 float scale, float* verts, float* kp, float* joints, int F, int V, void* ws, size_t ws_bytes, void* stream);
int mbx_smpl_bwd(const float* v_template, const float* shapedirs, const float* posedirs, const float* packed_t, const float* Jt,
                 const float* Jd, const int* parents, const float* lbs_weights, const float* Q, int K, const float* betas,
                 const float* rotmat, float scale, const float* dverts, const float* dkp, const float* djoints, float* drotmat,
                 float* dbetas, int F, int V, void* ws, size_t ws_bytes, void* stream);

/* ---- action recognition around the backbone (csrc/action.hip; lib/data/dataset_action.py:76-112,173-182, lib/utils/utils_data.py:7-29, ------
 *      train_action.py:55-61,172-188, lib/utils/learning.py:25-37) -- mbx_version() >= 130
 * mbx_action_input: NTURGBD.__getitem__ for a batch x [N,M,T,J,3] (x, y, confidence; f32) -> y of the same shape, one launch, one
 * workgroup per sample.  Nine draws per sample, params [N,9] = A0 A1 (degrees) S0 S1 Tx0 Tx1 Ty0 Ty1 ratio: params_in as they are, or
 * (params_in NULL) min(fma(hi - lo, u(stream k, index n), lo), hi) of the range of draw k with the counter-based hash of mbx_augment2d; params_out
 * (may be NULL) receives them.  With f_t = t / (T - 1) (0 for T = 1), a_t = (A0 + (A1 - A0) f_t) pi / 180, s_t, tx_t, ty_t likewise:
 *     x' = cos(a_t) s_t x - sin(a_t) s_t y + tx_t,  y' = sin(a_t) s_t x + cos(a_t) s_t y + ty_t     for EVERY joint of every person
 * (an all-zero second person lands on (tx_t, ty_t), as in the reference).  Over the joints with confidence != 0: fewer than 4 -> the sample
 * is 0; scale = max(xmax - xmin, ymax - ymin) ratio, scale == 0 -> the sample is 0; xs = (xmin + xmax - scale) / 2, ys likewise;
 * x'' = ((x' - xs) / scale - 0.5) 2, y'' likewise; all three channels clipped to [-1, 1].
 * flags: bit 0 the move (off: x' = x), bit 1 the crop (off: x', y' and the confidence are written as they are).
 * N, M, T, J >= 1, J <= 32; every range lo <= hi (checked).  y may be x. */
int mbx_action_input(const float* x, float* y, int N, int M, int T, int J, const float* params_in, float* params_out, float angle_lo,
                     float angle_hi, float scale_lo, float scale_hi, float trans_lo, float trans_hi, float crop_lo, float crop_hi,
                     int flags, uint64_t seed, void* stream);
/* mbx_xent_topk: CrossEntropyLoss() (mean) of logits [N,C] f32 with labels [N] i32, its gradient and the top-1 / top-5 hits in one launch.
 * Row loss = log sum_j exp(z_j - max z) - (z_y - max z); rank = #{j : z_j > z_y} + #{j < y : z_j == z_y}, a top-k hit iff rank < k.
 *   values [3] f32 = mean loss, top-1 hits, top-5 hits;  dlogits [N,C] (may be NULL) = (softmax - onehot) grad_scale / N;
 *   acc [4] f64 (may be NULL) += sum of row losses, top-1 hits, top-5 hits, N.
 * One workgroup, fixed summation order (row losses are added in fp64): two calls on the same input return the same bits.  A label outside
 * [0, C) gives NaN in its row's loss (hence the mean) and gradient, counts no hit and is never used as an index.
 * 1 <= N <= 65536, 1 <= C <= 4096 (checked). */
int mbx_xent_topk(const float* logits, const int* labels, int N, int C, float grad_scale, float* values, float* dlogits, double* acc,
                  void* stream);

/* ---- mesh targets (csrc/smpl.hip; MotionSMPL.__getitem__, lib/data/dataset_mesh.py:63-97, for a batch of clips) -- mbx_version() >= 140 ----
 * Inputs for N clips of T frames (F = N T <= 2^20), f32: pose [N,T,72] axis-angle, shape [N,T,10], motion_2d [N,T,17,3] (may be NULL without
 * x2d); the model arrays, parents, Q [K,V] (1 <= K <= 32, row 0 = the root) as mbx_smpl_fwd takes them; scale (the data set: 1000).
 * The flag of clip n is flips[n] != 0 (u8 [N]), or with flips NULL  u(seed, stream 0, index n) < flip_prob  of the counter-based hash of
 * mbx_augment2d (flip_prob 0: never, 1: always).  Outputs, each may be NULL (not all five):
 *   x2d [N,T,17,3]    motion_2d with the confidence clipped to [0,1]; a flipped clip is flip_data (utils_data.py:54-66): x negated, left and
 *                     right joints swapped.  Must not alias motion_2d.
 *   theta [N,T,82]    the pose, after flip_thetas (utils_mesh.py:458-484) in a flipped clip: components 1 and 2 of every joint negated, the
 *                     nine left / right pairs swapped; then the ten shape values.  Copies and negations: bit-exact, signed zeros included.
 *   kp_3d [N,T,K,3]   scale Q x - root,  verts [N,T,V,3]  scale x - root,  root = scale (Q x)[0] of the frame: scaled first, then subtracted
 *                     (dataset_mesh.py:85-90).  x = the forward of mbx_smpl_fwd on betas = shape and R = Rodrigues of the (flipped) pose
 *                     in smplx's form: angle = |r + 1e-8|, R = I + sin K + (1 - cos) K^2 (precise sinf / cosf; r = 0 gives I exactly).
 *   flips_used [N]    u8, the flags applied.
 * Launches: prepare (flips, Rodrigues into the workspace) -> the chain and vertex kernels of mbx_smpl_fwd (verts written once, keypoint
 * partials per vertex tile; without kp_3d only the root's) -> centring (every workgroup adds the root's tile partials in tile order, subtracts
 * the root from its share of verts in place; the first vertex chunk's workgroups finish and centre kp_3d).  verts equals the verts of
 * mbx_smpl_fwd minus its kp[:, 0] bit for bit.  fp32, fixed summation order, no float atomics.  Without kp_3d and verts the model arrays, Q
 * and ws are not read.  ws: >= mbx_mesh_gt_ws(F, V, K) bytes, 16-byte aligned; ws_bytes is checked.  F = 0 is a no-op.
 * No [F,24,9] tensor is returned: the rotation matrices stay in the workspace, whose layout is not part of this interface. */
size_t mbx_mesh_gt_ws(int F, int V, int K);
int mbx_mesh_gt(const float* pose, const float* shape, const float* motion_2d, const unsigned char* flips, uint64_t seed, float flip_prob,
                const float* v_template, const float* shapedirs, const float* posedirs, const float* Jt, const float* Jd, const int* parents,
                const float* lbs_weights, const float* Q, int K, float scale, float* x2d, float* theta, float* kp_3d, float* verts,
                unsigned char* flips_used, int N, int T, int V, void* ws, size_t ws_bytes, void* stream);

/* ---- in-the-wild inference around the backbone (csrc/wild.hip; infer_wild.py:56-97, lib/data/dataset_wild.py:15-86, ------------------------
 *      lib/utils/utils_data.py:7-29) -- mbx_version() >= 150
 * mbx_wild_input: halpe2h36m + the normalisation of read_input for F frames of S tracks.  kp [F,26,3] f64 (x, y, confidence of the Halpe-26
 * joints, the tracks one after another) -> y [F,17,channels] f32, channels 3 or 2 (2: without the confidence, args.no_conf).  H36M joint j
 * takes Halpe joint {19,12,14,16,11,13,15,*,18,0,17,5,7,9,6,8,10}[j]; joint 7 = (Halpe 18 + Halpe 19) * 0.5 in all three channels.
 * flags bit 0, pixel mode:  xy = (xy - (half_w, half_h)) / pix_scale    (half_w = w / 2, half_h = h / 2, pix_scale = min(w, h) / 2)
 * flags bit 1, crop mode (after the pixel mode where both are set), per track, over the joints whose mapped confidence is != 0: fewer than
 *   4 -> the track is 0 in all three channels; scale = max(xmax - xmin, ymax - ymin) * ratio, scale == 0 -> the track is 0;
 *   xs = (xmin + xmax - scale) / 2, ys likewise; xy = ((xy - (xs, ys)) / scale - 0.5) * 2; all three channels clipped to [-1, 1].
 * Every operation is float64 in this order, without contraction, rounded to f32 at the store: the reference's bits.
 * chunk_tab [n_chunks,3] i32 = (track, first frame, frames) with 1 <= frames <= MBX_WILD_CHUNK, a chunk never spans tracks, every frame in
 * exactly one chunk; seq_chunk_ptr [S+1] i32: the chunks of track s are seq_chunk_ptr[s] .. seq_chunk_ptr[s+1] - 1 (a track may have
 * none).  Both live on the device; a row that points outside [0,F) or [0,S) is skipped.  box [S,4] f64 (may be NULL) = (xs, ys, scale,
 * valid joints) per track, (0, 0, 0, valid joints) for a track that is zeroed; with box given it is computed in pixel-only mode too.
 * Three launches (chunk partials -> per-track fold in chunk order -> transform), no atomics.  ws: >= mbx_wild_input_ws(F, S) bytes, 8-byte
 * aligned; ws_bytes is checked.  F = 0 is a no-op. */
#define MBX_WILD_CHUNK 64
size_t mbx_wild_input_ws(int F, int S);
int mbx_wild_input(const double* kp, const int* chunk_tab, int n_chunks, const int* seq_chunk_ptr, int S, int F, double half_w,
                   double half_h, double pix_scale, double ratio, int flags, int channels, float* y, double* box, void* ws,
                   size_t ws_bytes, void* stream);
/* mbx_wild_output: infer_wild.py:81-96 for n clips of T frames, one launch.  pred [n,T,17,3] f32 (NOT modified), x [n,T,17,x_channels] f32
 * the network input (read with flags bit 1 only), dst_frames [n] i32 on the device: clip i is written to rows dst_frames[i] ..
 * dst_frames[i] + T - 1 of out [F,17,3] f32 (the caller guarantees that they exist; a negative entry skips the clip).
 * flags bit 0 rootrel: joint 0 of every frame = 0; otherwise only [clip, frame 0, joint 0, z] = 0 (the reference's quirk);
 * bit 1 gt_2d: then xy = x[..., :2]; bit 2 pixel mode: then p = p * pix_scale in f32 (pix_scale = float32(min(w, h) / 2)) and
 * xy = f32(f64(p) + (half_w, half_h)) -- numpy's arithmetic for a float32 array times a scalar, plus a float64 array. */
int mbx_wild_output(const float* pred, const float* x, int x_channels, const int* dst_frames, int n, int T, int flags, float pix_scale,
                    double half_w, double half_h, float* out, void* stream);

/* ---- in-the-wild mesh recovery (csrc/smpl.hip, csrc/wild.hip; infer_wild_mesh.py:42-56,108-154) -- mbx_version() >= 160 ----------------------
 * mbx_wild_mesh: infer_wild_mesh.py:115-141 for n clips of T frames (nT = n T) after the two network calls, written straight to each
 * clip's rows of the stitched results.  Pass A: rotmat_a [nT,24,9], betas_a [nT,10], the head's output on x.  Pass B (theta_b [nT,82], the
 * head's theta on flip_data(x); NULL: single-pass mode): pose = flip_thetas (utils_mesh.py:458-484) of theta_b[:, :72], R = Rodrigues in the
 * form of mbx_mesh_gt (angle = |r + 1e-8|), shape = theta_b[:, 72:].  Model arrays, parents, Q [K,V], scale as mbx_smpl_fwd takes them.
 * dst_frames [n] i32 ON THE DEVICE: clip i goes to rows dst_frames[i] .. dst_frames[i] + T - 1; dst_max: the largest entry, from the host's
 * plan (dst_max + T > F is refused; a device entry outside [0, F - T] skips its clip).  Outputs, each may be NULL (not all three), with x and
 * kp of a pass what mbx_smpl_fwd gives for its parameters:
 *   verts [F,V,3]  (scale x_a + scale x_b) * 0.5        kp [F,K,3]  (kp_a + kp_b) * 0.5
 *   theta [F,82]   (theta_a + [flipped pose_b | shape_b]) * 0.5      (needs theta_a [nT,82])
 * every product and sum rounded in fp32 (no contraction), as (a + b) / 2.0 of fp32 tensors rounds.  Single-pass mode: the bits of pass A
 * (verts and kp of mbx_smpl_fwd, theta_a copied).
 * Launches: prepare (pass B's rotations and shape and a copy of pass A's into the workspace, the theta rows) -> the chain kernel of
 * mbx_smpl_fwd over the 2 nT parameter sets -> vertex kernel (a wave evaluates both parameter sets of its frames with the per-pass operation
 * order of mbx_smpl_fwd and stores the mean once: the vertices of the single passes never reach memory; keypoint partials per vertex tile
 * and pass) -> keypoint finish (tile order).  fp32, fixed summation order, no float atomics.  ws: >= mbx_wild_mesh_ws(nT, V, K with kp else
 * 0, pair) bytes, 16-byte aligned; ws_bytes is checked.  nT = 0 is a no-op.  Refused: what mbx_smpl_fwd refuses, nT (2 nT with pass B)
 * > 2^20, a clip that does not fit F. */
size_t mbx_wild_mesh_ws(int nT, int V, int K, int pair);
int mbx_wild_mesh(const float* v_template, const float* shapedirs, const float* posedirs, const float* Jt, const float* Jd,
                  const int* parents, const float* lbs_weights, const float* Q, int K, const float* rotmat_a, const float* betas_a,
                  const float* theta_a, const float* theta_b, float scale, const int* dst_frames, int dst_max, int n, int T, int F,
                  float* verts, float* kp, float* theta, int V, void* ws, size_t ws_bytes, void* stream);
/* mbx_scale_fit: the minimiser of err(p) = mean_i |p0 x_i + (p1,p2,p3) - y_i| (infer_wild_mesh.py:42-43) for S tracks in one launch, where the
 * reference runs 400 least_squares starts on the host.  ref [F,17,3] f64 (the reference motion), kp [F,17,3] f32 (the stitched keypoints),
 * seq_ptr [S+1] i32 on the device: track s owns frames seq_ptr[s] .. seq_ptr[s+1] - 1.  x = ref - ref[:, :1] in f64; y = kp - kp[:, :1] in
 * f32 (numpy on the float32 reg3d_all), widened; everything after that is f64 without contraction.
 * The objective is convex (a mean of norms of a function affine in p).  Iteratively reweighted least squares: w_i = 1 / max(r_i, delta),
 * delta = MBX_SCALE_FIT_DELTA max|y|; every iteration is the weighted similarity fit in closed form from ten sums over the points
 * (W, W x [3], W y [3], W x.x, W x.y, sum r); first iteration w = 1; stop when |ds| <= MBX_SCALE_FIT_TOL max(|s|, 1e-300) and
 * |dt|_inf <= MBX_SCALE_FIT_TOL max|y|, at most MBX_SCALE_FIT_CAP iterations.
 * fit [S,6] f64 = scale, t [3], objective at (scale, t), iterations.  iterations < 0 is a status and the other five are NaN:
 *   -1 the track has no frames (or seq_ptr is not monotone inside [0,F]): nothing is read;  -2 the reference motion has no extent
 *   (sum w |x - xbar|^2 <= 1e-12 sum w |x|^2);  -3 the cap was reached.
 * One workgroup per track, the whole solve in the kernel: no host synchronisation, no float atomics, fixed summation order; a track's
 * result does not depend on the other tracks of the call (pooled and single-track calls give equal bits). */
#define MBX_SCALE_FIT_DELTA 1e-12
#define MBX_SCALE_FIT_TOL 1e-13
#define MBX_SCALE_FIT_CAP 2000
int mbx_scale_fit(const double* ref, const float* kp, const int* seq_ptr, int S, int F, double* fit, void* stream);
/* mbx_wild_mesh_place: infer_wild_mesh.py:153-154 in place, per track:
 *   verts[f,v] = f32( f64( f32(verts[f,v] - kp[f,0]) ) + ref[f,0] * fit[s,0] )
 * numpy 2's arithmetic for that line (a float32 difference added to a float64 root_cam), rounded to float32 once.  verts [F,V,3] f32,
 * kp [F,K,3] f32, ref [F,17,3] f64, seq_ptr [S+1] i32 and fit [S,6] f64 on the device.  One launch; a frame outside every track is left as
 * it is; a track whose fit holds a status receives that fit's NaN. */
int mbx_wild_mesh_place(float* verts, const float* kp, int K, const double* ref, const int* seq_ptr, int S, const double* fit, int F,
                        int V, void* stream);

/* ---- the 2D half of pre-training (csrc/motion2d.hip; lib/data/dataset_motion_2d.py:116-147, train.py:162-172, --------------------------------
 *      lib/utils/utils_data.py:7-29,54-66) -- mbx_version() >= 170
 * mbx_motion2d_input: InstaVDataset2D.__getitem__ and the no_grad block of train_epoch for a 2D batch x [N,T,J,3] (x, y, confidence; f32),
 * one launch, one workgroup per sample.  Two draws per sample, params [N,2] = (ratio, u_flip): params_in as they are, or (params_in NULL)
 * ratio = min(fma(hi - lo, u(stream 16, index n), lo), hi) and u_flip = u(stream 17, index n) with the counter-based hash of mbx_augment2d
 * (streams 0-14 are the augmentation's: one seed serves both); params_out (may be NULL, may be params_in) receives them.
 * flags: bit 0 crop -- over the joints with confidence != 0: fewer than 4 -> the sample is 0; scale = max(xmax - xmin, ymax - ymin) ratio,
 *          scale == 0 -> the sample is 0; xs = (xmin + xmax - scale) / 2, ys likewise; x'' = ((x - xs) / scale - 0.5) 2, y'' likewise; all three
 *          channels clipped to [-1, 1] (the operations, and the bits, of mbx_action_input's crop);
 *        bit 1 zeroing -- a joint whose confidence is 0 becomes (0, 0, 0);
 *        bit 2 flip -- if u_flip < flip_prob the clip is flip_data: x negated, joint j reads joint perm[j] of the 17-joint left / right table
 *          (J = 17 is required with this bit);
 *        bit 3 noise, bit 4 mask -- the arguments and bits of mbx_augment2d's flags 1 and 2;  bit 5 rootrel.
 * Outputs, each may be NULL (not all four):
 *   data [N,T,J,3]  the data set's item;   conf [N,T,J] = data[..., 2]
 *   gt [N,T,J,3]    rootrel: data - data[:, :, 0:1] in all three channels; otherwise data with channel 2 minus data[n,0,0,2]
 *   x_aug [N,T,J,3] what mbx_augment2d writes for data with the same seed and arguments, bit for bit
 * A sample of at most MBX_MOTION2D_RESIDENT joints (T J) is read once and kept in LDS; a larger one is read twice (the second time from L2).
 * Refused: null x, no output, N, T, J < 1, J > 32, lo > hi, flip_prob outside [0, 1], unknown flag bits, the flip with J != 17, noise without
 * its arrays, N T J >= 2^32, an output that overlaps x (the flip reads other joints of the frame). */
#define MBX_MOTION2D_RESIDENT 1536
int mbx_motion2d_input(const float* x, float* data, float* gt, float* conf, float* x_aug, int N, int T, int J, const float* params_in,
                       float* params_out, float ratio_lo, float ratio_hi, float flip_prob, const float* noise_mean,
                       const float* noise_std, const float* noise_weight, float uniform_range, float jitter_std, float d2c_a,
                       float d2c_b, float d2c_m, float d2c_s, float mask_ratio, float mask_T_ratio, int flags, uint64_t seed,
                       void* stream);

/* ---- AMASS: the regressed joints of SMPL-H + DMPL without the vertices (csrc/amass.hip; tools/preprocess_amass.py:29-60, ----------------------
 *      tools/convert_amass.py:26-31) -- mbx_version() >= 180
 * mbx_amass_joints: kp [F,K,3] f32 = Q . vertices of human_body_prior's BodyModel(num_betas=16, num_dmpls=8) (52 joints, linear blend
 * skinning as smplx.lbs.lbs evaluates it, then + trans), for poses [F,156] (52 axis-angle vectors: root, 21 body, 30 hand; smplx's
 * Rodrigues form, angle = |r + 1e-8|), betas [16] (betas_per_frame = 0: one per sequence) or [F,16], dmpls [F,8] or NULL (zeros), trans
 * [F,3] or NULL (zeros).  The vertices never exist: the model arrives folded (motionbert_amd/amass.py, in float64, once per body model):
 *   c = [betas, dmpls];  feat = [1, c, R_1 - I, .., R_51 - I]  (484 values);  J = Jt + Jd c  (Jt [52,3], Jd [52,3,24])
 *   A_k = [G_k | Gt_k - G_k J_k] from the kinematic chain over parents [52] (a host array; forward-ordered, parents[0] = -1)
 *   kp_j = sum over the pairs p = (j,k), in pair order, of  G_k (P[p] . feat) + (Gt_k - G_k J_k) s[p],   then + qs[j] trans
 * with pairs [Np,2] i32 (sorted by j, then k; j < K, k < 52), P [Np,3,484], s [Np], qs [K] on the device:
 *   P[(j,k)] = sum_v Q[j,v] w[v,k] [T_v | S_v | posedirs_v],  s[(j,k)] = sum_v Q[j,v] w[v,k],  qs[j] = sum_v Q[j,v].
 * flags: bit 0 camera -- the step of convert_amass.py in the same launch: (x, y, z) -> (x, -z, y), then x float32(0.298); equal in value
 *          to those two operations applied to the unflagged output;
 *        bit 1 -- the product P . feat on the vector unit (fmaf chains in k order) instead of the exact-fp32 MFMA: the measured
 *          alternative (tools/amass_bench.py), not the default.
 * One launch, no workspace; a workgroup owns MBX_AMASS_TILE frames.  fp32, no atomics, fixed summation order; a frame's result does not
 * depend on the other frames of the launch (a launch over [0,F) equals the launches over its single frames bit for bit).  F = 0 is a
 * no-op.  Refused: F < 0, K < 1, K > 32, Np < 0, Np > 17 * 52, unknown flag bits, null model arrays, parents that are no forward-ordered
 * tree, a P that is not 16-byte aligned. */
#define MBX_AMASS_TILE 16
int mbx_amass_joints(const float* poses, const float* betas, int betas_per_frame, const float* dmpls, const float* trans, const float* Jt,
                     const float* Jd, const int* parents, const int* pairs, const float* P, const float* s, const float* qs, int Np, int K,
                     int flags, float* kp, int F, void* stream);

/* ---- ragged batches: clips of different lengths in one inference forward (csrc/attention.hip, csrc/elementwise.hip, csrc/wild.hip) ----------
 *      -- mbx_version() >= 190
 * A ragged batch is F frames of J joints, the clips one after another (the layout mbx_wild_input writes), and two device tables:
 *   clip_tab [n_clips,2] i32 = (first frame, frames) of every clip;   frame_t [F] i32 = the index of every frame inside its clip.
 * Every row-wise kernel and the spatial attention (mbx_attn_fwd with B = 1, T = F) take such a batch as it is; the three entries below are
 * the kernels that know where a clip starts.  Inference only: there is no backward, no dropout.
 * mbx_attn_fwd_ragged: temporal attention.  Problem (clip b, joint j, head h) reads tokens first_b J + j + s J, s < frames_b, of qkv [F J,3C] T
 * and writes those rows of o [F J,C] T and lse [F J,H] f32: per problem the fragment walk and the arithmetic of
 * mbx_attn_fwd(B = 1, T = frames_b, temporal) on the clip's rows, hence its bits.  The tiles are sized for max_len (>= every frames_b):
 * max_len > 32 runs one workgroup per problem, otherwise one problem per wave, four per workgroup, each with its own length.
 * max_len <= 256 (refused beyond: the streamed kernels take one length per call).  A table row with first < 0, frames < 1, frames > max_len or
 * first + frames > F is skipped: nothing of that clip is written.  hd 32 or 64, bf16 or f32; n_clips = 0 is a no-op. */
int mbx_attn_fwd_ragged(const void* qkv, void* o, float* lse, const int* clip_tab, int n_clips, int F, int max_len, int J, int H, int hd,
                        float scale, int dtype, void* stream);
/* mbx_embed_fwd / mbx_embed_fwd_tta for a ragged batch x [F,J,Din]: the temporal row of frame f is temp[frame_t[f]] (temp [n_temp,C]);
 * same operations in the same order, hence the bits of the per-clip calls.  The TTA form writes h [2F J,C]: rows F J .. 2 F J - 1 are the
 * flipped view and use the same frame_t.  A frame whose frame_t lies outside [0, n_temp) is skipped. */
int mbx_embed_fwd_ragged(const float* x, const float* w, const float* b, const float* pos, const float* temp, const int* frame_t, float* h,
                         int F, int J, int Din, int C, int n_temp, void* stream);
int mbx_embed_fwd_tta_ragged(const float* x, const int* perm, const float* w, const float* b, const float* pos, const float* temp,
                             const int* frame_t, float* h, int F, int J, int Din, int C, int n_temp, void* stream);
/* mbx_wild_output for one ragged batch: pred [Fb,17,3] f32 (NOT modified) holds whole clips one after another and goes to rows dst0 ..
 * dst0 + Fb - 1 of out [F,17,3] f32 (refused when they do not exist); x [Fb,17,x_channels] is the batch's network input and frame_t [Fb] the
 * batch's part of the table above.  Flags and arithmetic are mbx_wild_output's; without rootrel, z of joint 0 is zeroed at every frame with
 * frame_t == 0 -- the reference's quirk at frame 0 of every clip. */
int mbx_wild_output_ragged(const float* pred, const float* x, int x_channels, const int* frame_t, int Fb, int dst0, int F, int flags,
                           float pix_scale, double half_w, double half_h, float* out, void* stream);

/* ---- mesh video frames (csrc/render.hip; the view of lib/utils/vismo.py:297-334, motion2video_mesh) -- mbx_version() >= 200 ------------------
 * A z-buffered, flat-shaded render in fixed point: orthographic along +z (smaller z is nearer), image x right with mesh x, image y down with
 * mesh y, inside the bounding cube of the whole motion of a track.  S = size ss samples per side (size <= MBX_RENDER_MAX_SIZE, ss 1 or 2).
 * mbx_render_project: verts [F,V,3] f32, cube [n_tracks,4] f32 = (cx, cy, cz, inv) with inv = 1 / (2 R), seq_ptr [n_tracks+1] i32 (track s owns
 * frames seq_ptr[s] .. seq_ptr[s+1] - 1), all on the device -> out [F,V,3] i32.  In fp32, every operation rounded on its own:
 *   xq = floor(((x - cx) inv + 0.5f) (S MBX_RENDER_SUB))    yq likewise from y    zq = floor(((z - cz) inv + 0.5f) MBX_RENDER_ZQ)
 * A product that is not finite or not below 2^30 in magnitude, and every vertex of a frame outside all tracks, gives 2^30 (outside the guard
 * below).  One launch.  F = 0 is a no-op.
 * mbx_render_raster: vq [F,V,3] i32 (the projection), verts [F,V,3] f32 (for the normals), faces [Nf,3] i32 -> rgb [F,size,size,3] u8 and,
 * where given, face_id [F,S,S] i32 (-1 where empty) and depth [F,S,S] i32 (0x7fffffff where empty); every element is written.
 *   dropped   a face with an index outside [0,V), an |xq| or |yq| > 2^17, a zq outside [0, MBX_RENDER_ZQ], or doubled area A2 = 0
 *   coverage  sample (i,j) sits at (SUB j + SUB / 2, SUB i + SUB / 2).  The face is oriented so that A2 = E01(p2) > 0 whatever its winding, with
 *             Eab(s) = (bx - ax)(sy - ay) - (by - ay)(sx - ax) in int64, and w0 = E12(s), w1 = E20(s), w2 = E01(s), w0 + w1 + w2 = A2.
 *             Covered: every w_i > 0, or w_i = 0 on an edge a -> b with by - ay > 0 or (by = ay and bx - ax > 0); the neighbour's reversed
 *             edge answers the opposite, so a sample on a shared edge belongs to exactly one face
 *   depth     d = floor((w0 z0 + w1 z1 + w2 z2) / A2), int64 (A2 < 2^38, numerator < 2^58)
 *   winner    the minimum of (d << 32) | face over the covering faces: nearer wins, then the lower face index; independent of any order
 *   shading   flat, from the fp32 vertices taken in ascending index order a < b < c: n = cross(vb - va, vc - va), I = 0.35 + 0.65 |n_z| / |n|
 *             (|n|^2 zero or not finite: |n_z| / |n| = 0), channel = floor((alpha colour) I + 255 (1 - alpha) + 0.5) clipped to [0, 255], fp32
 *             without contraction; background 255
 *   ss = 2    pixel = (a + b + c + d + 2) >> 2 of its four samples' channels, in the same launch
 * Three launches (frame boxes, face boxes and colours, tiles), no global atomics, every output element written once.  ws: >=
 * mbx_render_raster_ws(F, Nf) bytes, 8-byte aligned; ws_bytes is checked.  F = 0 is a no-op.  Refused: Nf < 1 or >= 2^28, F > 65535, size or ss
 * out of range, a colour outside [0, 255], alpha outside [0, 1]. */
#define MBX_RENDER_SUB 16
#define MBX_RENDER_ZQ (1 << 20)
#define MBX_RENDER_MAX_SIZE 2048
int mbx_render_project(const float* verts, const float* cube, const int* seq_ptr, int n_tracks, int F, int V, int size, int ss, int* out,
                       void* stream);
size_t mbx_render_raster_ws(int F, int Nf);
int mbx_render_raster(const int* vq, const float* verts, const int* faces, int F, int V, int Nf, int size, int ss, float red, float green,
                      float blue, float alpha, unsigned char* rgb, int* face_id, int* depth, void* ws, size_t ws_bytes, void* stream);

/* ---- skeleton video frames (csrc/skeleton.hip; the view of lib/utils/vismo.py:246-285, motion2video_3d) -- mbx_version() >= 210 --------------
 * The 3D-skeleton branch of render_and_save in fixed point: bones as capsules, joints as ringed discs, white background; matplotlib's panes,
 * grid, tick labels and anti-aliasing are not drawn.  S = size ss samples per side (size <= MBX_RENDER_MAX_SIZE, ss 1 or 2).
 * mbx_skeleton_project: x [F,J,3] f32 on the device (the X3D of infer_wild.py), view15 = 15 doubles in HOST memory: rows 0, 1 and 3 of the
 * 4 x 4 matrix M of Axes3D.get_proj(), then u_lo, v_hi, inv_w (the left and upper end of the 2D window of the axes and 1 / its width)
 * -> jq [F,J,2] i32 in 1/MBX_RENDER_SUB of a sample.  Per joint:
 *   ax = x + 1.0f, ay = y + 1.0f in fp32 (pixel2world_vis_motion on the float32 motion; its factor 512 / 2 is exact); from here on float64,
 *   every operation rounded on its own:  p = (-256 ax, -256 z, -256 ay), the plotted (-X, -Z, -Y);
 *   U = ((M00 px + M01 py) + M02 pz) + M03, V from row 1 and W from row 3 likewise;  u = U / W, v = V / W;
 *   xq = floor(((u - u_lo) inv_w) (16 S)),  yq = floor(((v_hi - v) inv_w) (16 S)): image x right with u, image y down with -v.
 * A joint with a component that is not finite, with W <= 0 (or not finite), or with |xq| or |yq| > 2^18 gives 2^30 in both components.  One
 * launch.  F = 0 is a no-op.  Refused: J outside [1, MBX_SKELETON_MAX_JOINTS], a view value that is not finite, size or ss out of range.
 * mbx_skeleton_raster: jq [F,J,2] i32, bones [Nb,2] i32 (joint indices), colors [Nb,3] u8, radii r_line, r_out, r_in in 1/16 sample
 * -> rgb [F,size,size,3] u8 and, where given, prim_id [F,S,S] i32 (-1 where empty); every element is written.
 *   samples     sample (i,j) has its centre at s = (16 j + 8, 16 i + 8).
 *   primitives  bone k with ends a = jq[bones[k][0]], b = jq[bones[k][1]] gives three, in the reference's plot order (Line3D artists are not
 *               depth-sorted; later plots cover earlier ones): priority 3k the capsule dist(s, segment ab) <= r_line, 3k + 1 the marker at a,
 *               3k + 2 the marker at b.  A bone with an index outside [0,J) or an end with |xq| or |yq| > 2^18 contributes nothing.
 *   capsule     with d = b - a, p = s - a, t = p.d, dd = d.d, r = r_line:  t <= 0: |p|^2 <= r^2;  t >= dd: |s - b|^2 <= r^2;  otherwise
 *               (px dy - py dx)^2 <= r^2 dd.  a = b is the disc.
 *   marker      at c: the disc |s - c|^2 <= r_out^2, white where |s - c|^2 <= r_in^2, the bone's colour elsewhere.
 *   winner      the covering primitive of highest priority: a maximum over a set, independent of any order.  No cover: background, 255.
 *   ss = 2      pixel = (a + b + c + d + 2) >> 2 of its four samples' channels, in the same launch.
 *   exactness   every comparison is an integer comparison without overflow: ends within 2^18 and sample centres within [8, 16 (4096 + 31) + 8]
 *               keep every component of p, d and s - b below 2^19 + 2^10 in magnitude, so |p|^2, t, dd and |px dy - py dx| are below 2^40
 *               (int64).  r <= MBX_SKELETON_MAX_RADIUS = 2^11 gives r^2 dd < 2^62.  A cross product of magnitude >= 2^31 has a square
 *               >= 2^62 > r^2 dd and is rejected before squaring; below that its square is < 2^62.
 * One launch, no workspace, no global atomics, every output element written once.  F = 0 is a no-op.  Refused: J outside
 * [1, MBX_SKELETON_MAX_JOINTS], Nb outside [1, MBX_SKELETON_MAX_BONES], a radius outside [0, 2^11] or r_in > r_out, size or ss out of range. */
#define MBX_SKELETON_MAX_JOINTS 32
#define MBX_SKELETON_MAX_BONES 64
#define MBX_SKELETON_MAX_RADIUS (1 << 11)
int mbx_skeleton_project(const float* x, const double* view15, int F, int J, int size, int ss, int* jq, void* stream);
int mbx_skeleton_raster(const int* jq, const int* bones, const unsigned char* colors, int F, int J, int Nb, int r_line, int r_out, int r_in,
                        int size, int ss, unsigned char* rgb, int* prim_id, void* stream);

/* ---- crowd video frames (csrc/scene.hip; every tracked person of a video frame in one image) -- mbx_version() >= 240 ---------------------------
 * The skeletons of mbx_skeleton_raster, any number per frame, in an image of W x H pixels (1 <= W, H <= MBX_RENDER_MAX_SIZE, W != H allowed, ss 1
 * or 2), over one colour or over the frames of the video.  The reference draws one person; this has no counterpart there.
 * mbx_scene_project: x [R,J,C] f32 on the device, C = 2 or 3, in video pixels (the output of in-the-wild inference with pixel coordinates; z is
 * not used: inside one skeleton the plot order decides, as above) -> jq [R,J,2] i32 in 1/MBX_RENDER_SUB of a sample.  In float64:
 *   xq = floor(double(x) (16 ss) + 0.5), yq likewise: the product is exact, the sum is rounded once.
 * A joint with a component that is not finite or with |xq| or |yq| > 2^18 gives 2^30 in both components.  One launch.  R = 0 is a no-op.
 * mbx_scene_raster: jq [R,J,2] i32; the scene table frame_ptr [Fv+1] i32, rows [n_entries] i32, person [n_entries] i32: video frame f shows the
 * entries k = frame_ptr[f] .. frame_ptr[f+1] - 1 in drawing order, entry k is the skeleton jq[rows[k]] in the colours palette[person[k]];
 * bones [Nb,2] i32; palette [P,Nb,3] u8 (P = 1: everybody in row 0, person is not looked at); radii as above; the background: bg_frames u8
 * [bg_n,H,W,3] with bg_n = Fv or 1 (frame 0 for every video frame), or, with bg_frames null, the colour bg_rgb = r | g << 8 | b << 16
 * -> rgb [Fv,H,W,3] u8 and, where given, prim_id [Fv, H ss, W ss] i32; every element is written exactly once.
 *   coverage    samples, primitives, capsule and marker exactly as in mbx_skeleton_raster: the same int64 comparisons (csrc/skeleton_prim.h).
 *               The bound stated there holds unchanged: W, H <= 2048 and ss <= 2 keep every sample centre within [8, 16 (4096 + 31) + 8].
 *   winner      with rank = k - frame_ptr[f], the covering primitive with the largest id = rank 3 Nb + priority: a later person covers an
 *               earlier one, inside a person the plot order decides.  A marker's white centre counts as white.  prim_id = that id, -1 where
 *               nothing covers.  Ranks from 2^23 on are not drawn (the id is an int32).
 *   background  a sample that nothing covers takes the colour, or the pixel of the background frame that holds it.
 *   ss = 2      pixel = (a + b + c + d + 2) >> 2 of its four samples' channels, uncovered samples counting with the background pixel.
 *   skipped     an entry with rows[k] outside [0,R) or, for P > 1, person[k] outside [0,P); frame_ptr values are cut to [0, n_entries] and
 *               to ascending order.  The tables live on the device: the host cannot check them without a synchronisation.
 * One workgroup per tile of 32 x 32 samples walks its frame's list MBX_SCENE_CHUNK persons at a time: one lane per person tests the box of
 * the person's drawn joints, grown by the largest radius, against the tile; only the survivors' primitives are set up and tested.  Nothing
 * caps the list.  One launch, no workspace, no global atomics.  Fv = 0 is a no-op; R = 0 or an empty table writes the background.  Refused: J,
 * Nb, radii as in mbx_skeleton_raster, W, H or ss out of range, P < 1, n_entries > 2^30, bg_n other than 1 or Fv, a colour beyond 0xffffff. */
#define MBX_SCENE_CHUNK 64
int mbx_scene_project(const float* x, int R, int J, int C, int ss, int* jq, void* stream);
int mbx_scene_raster(const int* jq, const int* frame_ptr, const int* rows, const int* person, int n_entries, const int* bones,
                     const unsigned char* palette, int Fv, int R, int J, int Nb, int P, int r_line, int r_out, int r_in, int W, int H, int ss,
                     const unsigned char* bg_frames, int bg_n, int bg_rgb, unsigned char* rgb, int* prim_id, void* stream);

/* ---- video files from the device (csrc/jpeg.hip; motionbert_amd/video.py) -- mbx_version() >= 230 -------------------------------------------
 * Baseline JPEG (ITU-T T.81, 8 bit, three components, one interleaved scan, the Annex K Huffman tables) exactly as libjpeg's default path
 * computes it: the file equals the one libjpeg-turbo writes for the same pixels, quality, subsampling and restart interval, byte for byte.
 * All arithmetic is int32.  sub: 0 = 4:4:4 (MCU 8 x 8: Y Cb Cr), 1 = 4:2:0 (MCU 16 x 16: Y00 Y01 Y10 Y11 Cb Cr); MCUs in raster order;
 * n_mcu = ceil(W / m) ceil(H / m) with m = 8 or 16.
 * mbx_jpeg_blocks: rgb [F,H,W,3] u8 -> coef [F, n_mcu, blocks per MCU, 64] i16, quantised, in zigzag order.
 *   colour     Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,  Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
 *              Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16
 *   padding    a sample outside the image is the nearest one inside (last column, then last row)
 *   4:2:0      chroma: rows padded to an even count, columns to a multiple of 16; c = (a + b + c + d + bias) >> 2 over each 2 x 2, bias 1 in
 *              even output columns and 2 in odd ones; only then the last downsampled row is repeated down to the MCU height.  A luma block
 *              of an MCU wholly beyond ceil(W / 8) block columns or ceil(H / 8) block rows is a dummy: AC 0, DC that of the preceding block
 *              of the MCU; in a dummy bottom row both blocks take the DC of the block in front of the row
 *   DCT        samples - 128, then MBX_JPEG_FDCT_PASS over the rows (first) and over the columns: the Loeffler-Ligtenberg-Moschytz
 *              butterfly of libjpeg's slow-integer method, 13 constant bits, 2 pass-1 bits; the result is 8 times the DCT
 *   quantise   q = clamp((base s + 50) / 100, 1, 255) with s = 5000 / quality below 50, else 200 - 2 quality, base = the Annex K table;
 *              coef = sign(c) ((|c| + (8 q >> 1)) / (8 q))
 * mbx_jpeg_entropy_sizes, then mbx_jpeg_entropy: coef as above -> F complete JFIF files back to back in data, file f at offsets[f] ..
 * offsets[f+1] - 1 (offsets [F+1] i64 on the device).  A file is the header of mbx_jpeg_header (MBX_JPEG_HEADER_BYTES: SOI, APP0 JFIF 1.01, two
 * DQT, SOF0, four DHT, DRI, SOS), the scan and EOI.  The scan: restart intervals of `restart` MCUs, RSTn with n = interval index mod 8 between
 * them; per interval the DC predictors start at 0, every block is DC difference, then (run, size) symbols with ZRL only in front of a later
 * non-zero coefficient and EOB unless coefficient 63 is non-zero; 0x00 after every 0xFF byte; the interval padded to a byte with 1-bits.
 *   sizing     nothing is truncated and no buffer is sized by a guess: mbx_jpeg_entropy_sizes codes every interval without storing it, counts
 *              its bytes after stuffing and leaves the offsets on the device; the caller reads offsets[F] -- the ONE host synchronisation of
 *              an encode -- allocates data and calls mbx_jpeg_entropy with the same coef, parameters and ws, which codes the intervals again
 *              straight into place.  data_bytes is checked against every store.
 *   worst case a block is at most MBX_JPEG_MAX_BLOCK_BITS = 22 + 63 (16 + 10) bits: the longest DC code with its 11 bits, and 63 coefficients
 *              of the longest AC code with 10 bits each (a ZRL stands for 16 zeros in fewer bits than 16 such coefficients; without a zero
 *              there is no EOB).  The kernel's LDS buffer holds that many bits for every block of a piece.  Coefficients outside the baseline
 *              range (a DC difference beyond +-2047, an AC beyond +-1023) are clamped to it, so the bound holds for any input
 *   ws         >= mbx_jpeg_entropy_ws(F, H, W, sub, restart) bytes, 16-byte aligned; ws_bytes is checked
 * F = 0 is a no-op.  Refused, not clamped: H or W outside [1, MBX_JPEG_MAX_SIZE], F > MBX_JPEG_MAX_FRAMES, quality outside [1, 100], restart
 * outside [1, 65535], sub other than 0 or 1, a small ws or data.  Everything is launched on the caller's stream. */
#define MBX_JPEG_MAX_SIZE 2048
#define MBX_JPEG_MAX_FRAMES 65535
#define MBX_JPEG_HEADER_BYTES 629
#define MBX_JPEG_MAX_BLOCK_BITS (22 + 63 * 26)
#define MBX_JPEG_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
/* one pass over int d[8], in place; `first`: the row pass (outputs scaled up by 2 bits), else the column pass (scaled back down) */
#define MBX_JPEG_FDCT_PASS(d, first)                                                                        \
    do {                                                                                                    \
        const int n_ = (first) ? 11 : 15;                                                                   \
        const int t0_ = d[0] + d[7], t7_ = d[0] - d[7], t1_ = d[1] + d[6], t6_ = d[1] - d[6];               \
        const int t2_ = d[2] + d[5], t5_ = d[2] - d[5], t3_ = d[3] + d[4], t4_ = d[3] - d[4];               \
        const int t10_ = t0_ + t3_, t13_ = t0_ - t3_, t11_ = t1_ + t2_, t12_ = t1_ - t2_;                   \
        d[0] = (first) ? (t10_ + t11_) << 2 : MBX_JPEG_DESCALE(t10_ + t11_, 2);                             \
        d[4] = (first) ? (t10_ - t11_) << 2 : MBX_JPEG_DESCALE(t10_ - t11_, 2);                             \
        const int za_ = (t12_ + t13_) * 4433;                                                               \
        d[2] = MBX_JPEG_DESCALE(za_ + t13_ * 6270, n_);                                                     \
        d[6] = MBX_JPEG_DESCALE(za_ - t12_ * 15137, n_);                                                    \
        const int z5_ = (t4_ + t6_ + t5_ + t7_) * 9633;                                                     \
        const int z1_ = -(t4_ + t7_) * 7373, z2_ = -(t5_ + t6_) * 20995;                                    \
        const int z3_ = -(t4_ + t6_) * 16069 + z5_, z4_ = -(t5_ + t7_) * 3196 + z5_;                        \
        d[7] = MBX_JPEG_DESCALE(t4_ * 2446 + z1_ + z3_, n_);                                                \
        d[5] = MBX_JPEG_DESCALE(t5_ * 16819 + z2_ + z4_, n_);                                               \
        d[3] = MBX_JPEG_DESCALE(t6_ * 25172 + z2_ + z3_, n_);                                               \
        d[1] = MBX_JPEG_DESCALE(t7_ * 12299 + z1_ + z4_, n_);                                               \
    } while (0)
int mbx_jpeg_header(int H, int W, int quality, int sub, int restart, unsigned char* out);      /* out: MBX_JPEG_HEADER_BYTES of HOST memory */
int mbx_jpeg_blocks(const unsigned char* rgb, int F, int H, int W, int quality, int sub, short* coef, void* stream);
size_t mbx_jpeg_entropy_ws(int F, int H, int W, int sub, int restart);
int mbx_jpeg_entropy_sizes(const short* coef, int F, int H, int W, int sub, int quality, int restart, long long* offsets, void* ws,
                           size_t ws_bytes, void* stream);
int mbx_jpeg_entropy(const short* coef, int F, int H, int W, int sub, int quality, int restart, const long long* offsets, unsigned char* data,
                     long long data_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---- reading video on the device (csrc/jpeg_dec.hip; motionbert_amd/video.py) -- mbx_version() >= 250 ------------------------------------------
 * Baseline JPEG decoded exactly as libjpeg's default path decodes it (jpeg_idct_islow, do_fancy_upsampling, 16-bit colour tables): the
 * pixels equal the ones libjpeg-turbo gives, with no tolerance.  Accepted (the host parser, video.parse_jpeg, refuses the rest before a
 * launch): SOF0, 8 bit, three components in one interleaved scan, luma sampling 1x1 (sub 0, 4:4:4), 2x2 (sub 1, 4:2:0) or 2x1 (sub 2,
 * 4:2:2: MCU 16 x 8, Y0 Y1 Cb Cr) with chroma 1x1, 8-bit DQT, the file's Huffman tables or Annex K where it has none, DRI or not.
 * All frames of a call share geometry, tables and restart interval.  restart = 0: no DRI, the frame is one interval; n_int =
 * ceil(n_mcu / restart) otherwise, and interval k covers MCUs k restart .. k restart + restart - 1.
 * mbx_jpeg_dec_tables (host to host): dht [6][272] u8 = (bits [16], vals [256]) of the DC and the AC table of components 0, 1, 2, or NULL
 *   for Annex K -> out [6][MBX_JPEG_DEC_TABLE_WORDS]: per table an 8-bit look-ahead (256 x u16: length << 8 | symbol, 0: longer), maxcode
 *   [18] and valoffset [18] i32 (libjpeg's), vals [256] u8.  Refused: more than 256 symbols, more codes than a length has, a DC symbol > 15.
 * mbx_jpeg_dec_index: data u8 [data_bytes] (the files back to back, on the device), scans i64 [F,2] = where every frame's entropy-coded
 *   bytes start and where its EOI marker lies (absolute, from the host parser; clamped into the buffer) -> pos i64 [F, n_int + 1] and
 *   status i32 [F, n_int].  An RSTn is 0xFF followed by 0xD0 .. 0xD7; marker k closes interval k, which is data[pos[k] .. pos[k+1] - 3];
 *   pos[0] = the start, pos[n_int] = the EOI's position + 2.  Unless the frame has n_int - 1 markers with n = k mod 8, every interval of
 *   it gets MBX_JPEG_DEC_MARKERS, else MBX_JPEG_DEC_OK.
 * mbx_jpeg_dec_entropy: T.81 F.2.2 per interval -> coef i16 [F, n_mcu, blocks per MCU, 64] in zigzag order (the layout mbx_jpeg_blocks
 *   writes) and status.  Predictors start at 0; 0xFF 0x00 is one byte 0xFF; a DC value is stored modulo 2^16.  coef is zeroed first; an
 *   interval whose status is not OK on entry is left zero.  A malformed interval has a defined result: its status is the first of
 *     MBX_JPEG_DEC_TRUNCATED  the interval ends inside a symbol        MBX_JPEG_DEC_BAD_CODE  no such Huffman code, or an AC symbol (r, 0)
 *     MBX_JPEG_DEC_RUN        a run or a ZRL passes coefficient 63                            with r other than 0 (EOB) and 15 (ZRL)
 *     MBX_JPEG_DEC_LEFTOVER   all blocks decoded and 8 or more bits are left
 *   and the block the error lies in and all later blocks of the interval are zero.  libjpeg's resynchronisation is not reproduced.
 * mbx_jpeg_dec_pixels: coef, q u8 [3][64] (HOST memory: the quantisation table of each component in zigzag order, no entry 0) -> rgb u8
 *   [F,H,W,3] at any address.  ws >= mbx_jpeg_dec_ws(F, H, W, sub) bytes holds the component planes, whole MCUs wide and high.
 *   IDCT       multiply by the table, un-zigzag, MBX_JPEG_IDCT_PASS over the columns (shift 11) and then over the rows (shift 18) in
 *              64-bit arithmetic (libjpeg's JLONG), then sample = limit[v & 1023] with limit = 128 .. 255, 255 x 384, 0 x 384, 0 .. 127
 *   upsample   chroma has dh = ceil(H / v) real rows and dw = ceil(W / h) real columns c; nothing beyond them is read.  dw <= 2:
 *              replicated.  4:2:2: out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2, the first and the last
 *              output copies.  4:2:0: s = 3 c[r] + c[r-1] (even output row) or 3 c[r] + c[r+1] (odd), rows clamped to [0, dh - 1];
 *              out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, first (4 s[0] + 8) >> 4, last (4 s[dw-1] + 7) >> 4
 *   colour     R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16),
 *              G = Y + ((-22554 (Cb - 128) + 32768 - 46802 (Cr - 128)) >> 16), arithmetic shifts, clamped to [0, 255]
 * F = 0 is a no-op.  Refused, not clamped: sizes outside the encoder's limits, sub outside 0 .. 2, restart outside [0, 65535], a small ws,
 * misaligned pointers.  Everything is launched on the caller's stream. */
#define MBX_JPEG_DEC_TABLE_WORDS 228
#define MBX_JPEG_DEC_OK 0
#define MBX_JPEG_DEC_TRUNCATED 1
#define MBX_JPEG_DEC_BAD_CODE 2
#define MBX_JPEG_DEC_RUN 3
#define MBX_JPEG_DEC_LEFTOVER 4
#define MBX_JPEG_DEC_MARKERS 5
/* one pass of jpeg_idct_islow over long long d[8] (dequantised), in place: the butterfly of MBX_JPEG_FDCT_PASS backwards */
#define MBX_JPEG_IDCT_PASS(d, shift)                                                                        \
    do {                                                                                                    \
        const long long r_ = 1ll << ((shift) - 1);                                                          \
        const long long za_ = (d[2] + d[6]) * 4433;                                                         \
        const long long e2_ = za_ - d[6] * 15137, e3_ = za_ + d[2] * 6270;                                  \
        const long long e0_ = (d[0] + d[4]) * 8192, e1_ = (d[0] - d[4]) * 8192;                             \
        const long long t10_ = e0_ + e3_, t13_ = e0_ - e3_, t11_ = e1_ + e2_, t12_ = e1_ - e2_;             \
        const long long z5_ = (d[7] + d[3] + d[5] + d[1]) * 9633;                                           \
        const long long z1_ = -(d[7] + d[1]) * 7373, z2_ = -(d[5] + d[3]) * 20995;                          \
        const long long z3_ = -(d[7] + d[3]) * 16069 + z5_, z4_ = -(d[5] + d[1]) * 3196 + z5_;              \
        const long long o0_ = d[7] * 2446 + z1_ + z3_, o1_ = d[5] * 16819 + z2_ + z4_;                      \
        const long long o2_ = d[3] * 25172 + z2_ + z3_, o3_ = d[1] * 12299 + z1_ + z4_;                     \
        d[0] = (t10_ + o3_ + r_) >> (shift); d[7] = (t10_ - o3_ + r_) >> (shift);                           \
        d[1] = (t11_ + o2_ + r_) >> (shift); d[6] = (t11_ - o2_ + r_) >> (shift);                           \
        d[2] = (t12_ + o1_ + r_) >> (shift); d[5] = (t12_ - o1_ + r_) >> (shift);                           \
        d[3] = (t13_ + o0_ + r_) >> (shift); d[4] = (t13_ - o0_ + r_) >> (shift);                           \
    } while (0)
int mbx_jpeg_dec_tables(const unsigned char* dht, unsigned* out);                               /* both HOST memory */
int mbx_jpeg_dec_index(const unsigned char* data, long long data_bytes, const long long* scans, int F, int n_int, long long* pos, int* status,
                       void* stream);
int mbx_jpeg_dec_entropy(const unsigned char* data, long long data_bytes, const long long* pos, const unsigned* tables, int F, int H, int W,
                         int sub, int restart, short* coef, int* status, void* stream);
size_t mbx_jpeg_dec_ws(int F, int H, int W, int sub);
int mbx_jpeg_dec_pixels(const short* coef, const unsigned char* q, int F, int H, int W, int sub, unsigned char* rgb, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- Huffman decoding inside a restart interval (csrc/jpeg_sync.hip) -- mbx_version() >= 260 -----------------------------------------------------
 * mbx_jpeg_dec_entropy_sync gives the coef and status of mbx_jpeg_dec_entropy, in every coefficient and status word and for every input,
 * malformed scans included, with many lanes per interval: the self-synchronising decode (Klein & Wiseman; Weissenberger & Schmidt).
 * State (p, k, z): p the position of the next bit in the RAW bytes of the interval (stuffed bytes counted), k the block inside the MCU, z the
 * next zigzag index (0: a DC symbol is next).  The interval's bytes are cut into subsequences of MBX_JPEG_SYNC_BYTES at fixed offsets from
 * its start; a subsequence that would begin on the 00 of an FF 00 pair begins one byte later; it owns the symbols whose first bit lies in
 * it, and its exit is the state at the first symbol at or behind its end.  MBX_JPEG_SYNC_CHUNK subsequences are a chunk, one workgroup.
 *   speculate  each lane decodes its subsequence from (its first bit, 0, 0), chunk 0's first from the true (0, 0, 0); then lane i takes lane
 *              i - 1's exit and decodes again while that changes (at most MBX_JPEG_SYNC_CHUNK rounds).  The decode is LENIENT: where no code
 *              matches, one bit on with the state unchanged; a DC symbol s takes s & 15 bits; EOB ends the block; every other AC symbol
 *              (r, s) takes s bits and r + 1 coefficients, and a block ends at coefficient 63.  Behind the interval's end the bits are 0.
 *   verify     chunk c >= 1 starts lane 0 from the exit stored for chunk c - 1 and repeats the rounds; an interval all of whose chunks
 *              reproduce their stored exit has true exits throughout; otherwise route = 1.
 *   scan       exclusive sums over the subsequences of (blocks completed, DC differences per component mod 2^32).
 *   write      each lane decodes again from its true entry with the checks of mbx_jpeg_dec_entropy and stores at (block from the scan, z),
 *              every store checked against the interval's block count; the lane that completes the last block applies the LEFTOVER rule.
 *              route = 2 where a check fails, where the bytes end before the blocks do, or where the interval is empty.
 *   fall back  an interval with route != 0 is zeroed again and decoded by the lane of mbx_jpeg_dec_entropy, which defines its result.
 * route i32 [F, n_int] (out): 0 decoded in parallel (or status was not OK on entry: nothing is decoded), 1, 2 as above, 3 the interval is
 * longer than max_interval_bytes.  max_interval_bytes (0 .. 2^27, from the host's parsed scan lengths) sizes the grid and ws
 * (>= mbx_jpeg_dec_sync_ws(F, n_int, max_interval_bytes) bytes, 16-byte aligned); a longer interval never touches ws.  route is a property
 * of the bytes, the tables and the two constants.  F = 0 is a no-op; refused: null pointers, a small ws, sizes as mbx_jpeg_dec_entropy. */
#ifndef MBX_JPEG_SYNC_BYTES
#define MBX_JPEG_SYNC_BYTES 256       /* 128, 256 and 512 were measured: profiles/jpeg_sync_bench.txt */
#endif
#define MBX_JPEG_SYNC_CHUNK 256
size_t mbx_jpeg_dec_sync_ws(int F, int n_int, long long max_interval_bytes);
int mbx_jpeg_dec_entropy_sync(const unsigned char* data, long long data_bytes, const long long* pos, const unsigned* tables, int F, int H, int W,
                              int sub, int restart, long long max_interval_bytes, short* coef, int* status, int* route, void* ws,
                              size_t ws_bytes, void* stream);

/* ---- measurement aid (bench.py`roofline.sustained_mfma_tflops`; not part of the model) --------------------------------------------
 * The bf16 MFMA rate the part sustains under its power cap with nothing but v_mfma_f32_32x32x16_bf16 in the loop (pseudo-random
 * operands; n_wg workgroups of 4 waves, `iters` x 16 MFMAs per wave).  ws: >= mbx_mfma_probe_ws(n_wg) bytes = a float sink
 * [n_wg * 256] followed by int64 [n_wg][2] = {shader cycles, 100 MHz real-time ticks} of every workgroup's loop (effective clock).
 * *flops = the matrix FLOPs of the launch; the caller times it with HIP events. */
size_t mbx_mfma_probe_ws(int n_wg);
int mbx_mfma_probe(void* ws, int n_wg, int iters, unsigned seed, double* flops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MBX_H */
