/*
 * ea_hip.h -- C ABI of libea_hip.so: the MI355X (gfx950) attention hot path of
 * HKUNLP/efficient-attention.
 *
 * The reference has no FFI: its hot path is chains of torch ops inside
 *   efficient_attention/{abstract_attention,local_attention,eva,lara,kernelized_attention}.py
 * (SURVEY.md 8a/8b).  Each entry point below replaces one such chain with hand-written HIP
 * kernels; the citation on every function names the reference lines it replaces.  The host
 * mirror of the reference's nn.Module / AttentionFactory surface
 * (efficient-attention_amd/efficient_attention) binds these symbols with ctypes and passes raw
 * device pointers -- no torch types cross this boundary (INTEGRATION.md shows the binding a
 * reference maintainer would add).
 *
 * Conventions
 *   - All pointers are DEVICE pointers.  `stream` is a hipStream_t (NULL = default stream).
 *   - q/k/v/out-like tensors are logical [B, H, N, D] with the last dim contiguous and
 *     arbitrary ELEMENT strides for the other three (ea_t4), so the [B, N, 3, H, D] output of
 *     the fused qkv Linear and the [B, N, H, D] input of the output projection are addressed
 *     in place (no permute/contiguous copies: abstract_attention.py:72-78,86).
 *   - I/O element type: EA_BF16 or EA_F16 (ea_geom.dtype).  MFMA operands have that type,
 *     accumulation / softmax / statistics are fp32 (the autocast contract of vit/engine.py:47).
 *   - key_padding_mask: uint8 [B, N], 1 = padded key, or NULL.
 *   - Every function returns 0 on success, a negative EA_E* code on invalid arguments or
 *     unsupported geometry, or a positive hipError_t from the launch.  Nothing is ever
 *     computed on the host.
 */
#ifndef EA_HIP_H
#define EA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EA_BF16 0
#define EA_F16  1
#define EA_F32  2          /* accepted by the ea_performer_f32_* entry points only */

#define EA_OK            0
#define EA_E_BADARG     -1   /* null pointer / inconsistent sizes */
#define EA_E_UNSUPPORTED -2  /* geometry outside what the kernels are built for */

/* logical [B,H,N,D] tensor, D contiguous */
typedef struct {
  void*   ptr;
  int64_t sb, sh, sn;        /* element strides of batch, head, token */
} ea_t4;

/* Window / landmark geometry shared by the local, EVA and LARA entry points. */
typedef struct {
  int32_t B, H, N, D;        /* N = tokens per (b,h) AFTER EVA's 1-D padding (eva.py:127-136) */
  int32_t dtype;             /* EA_BF16 | EA_F16 */
  int32_t attn_2d;           /* 1: tokens form a gh x gw grid (row-major), 0: 1-D sequence */
  int32_t gh, gw;            /* grid (2-D); ignored in 1-D */
  int32_t window;            /* window side w (local_attention.py:36) */
  int32_t ext;               /* overlap extension e = max(1, w/2) or 0 (local_attention.py:38-41) */
  int32_t chunk;             /* EVA landmark chunk side r (eva.py:155-158); 0 when unused */
  int32_t L;                 /* number of landmarks / chunks actually produced */
  float   scale;             /* D^-0.5 */
  int32_t causal;            /* 0: symmetric windows (eva.py, local_attention.py).  causal_eva.py (1-D only):
                              * 1: the keys of window g are [g*w - e, g*w + w) (causal_window_1d_partition,
                              *    causal_eva.py:104-116), the landmark chunks carry no extension (:688-694)
                              *    and the local logits of padded QUERIES are masked as well (:742-755);
                              * 2: 1 plus the causal masks -- local key j of query i is masked when
                              *    j > i + e (:767-773) and landmark c unless c < token / chunk (:716-738).
                              * Masked logits are REPLACED by -5e4 (masked_fill), their gradient is zero. */
  int32_t lm_base;           /* causal == 2 only: landmarks that lie BEFORE the tokens of this call and are visible to
                              * every query -- landmark c is masked unless c < lm_base + token / chunk.  0 for a whole
                              * sequence.  No caller of this package sets it any more (ABI 17: incremental decoding has
                              * its own entry points, ea_ceva_decode_*); kept so that the struct layout stays stable. */
} ea_geom;

/* ---- library info -------------------------------------------------------------------- */
const char* ea_version(void);                 /* "ea_hip <semver> gfx950" */
int32_t     ea_abi_version(void);             /* bumped on any signature change */

/* ---- EVA landmark statistics (eva.py:155-196) ------------------------------------------
 * ea_eva_chunk_mean_fwd: masked means of q and k over every landmark chunk (chunk side r,
 *   same overlap extension e as the windows; masked/out-of-range slots count as zeros in the
 *   mean: rf_w_q.masked_fill(...).mean(-2), eva.py:174-180).  qmean,kmean: fp32 [B,H,L,D].
 * ea_eva_chunk_mean_bwd: dq[b,h,n,:] += sum_{c ni n} dqmean[c]/J (same for k); dq/dk are
 *   ACCUMULATED INTO (I/O dtype, fp32 math).
 * ea_eva_beta_fwd: beta_c = sum_j softmax_j(s*omega_c.k_j - s|k_j|^2/2, -5e4 on masked) v_j
 *   (prm_projection normalize=False, attn_utils.py:324-347; eva.py:192-196). omega, beta: fp32
 *   [B,H,L,D].
 * ea_eva_beta_bwd: given dbeta, ACCUMULATES dk, dv and writes domega (fp32 [B,H,L,D]). */
int ea_eva_chunk_mean_fwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const uint8_t* mask,
                          float* qmean, float* kmean, void* stream);
int ea_eva_chunk_mean_bwd(const ea_geom* g, const float* dqmean, const float* dkmean,
                          const uint8_t* mask, const ea_t4* dq, const ea_t4* dk, void* stream);
int ea_eva_beta_fwd(const ea_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                    const float* omega, float* beta, void* stream);
int ea_eva_beta_bwd(const ea_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                    const float* omega, const float* beta, const float* dbeta,
                    const ea_t4* dk, const ea_t4* dv, float* domega, void* stream);

/* ---- window attention with control-variate columns -----------------------------------------
 * One joint softmax per query over [ local window keys | L landmark keys ]:
 *     logits_local = s q.k_j + bias[h,i,j], masked_fill(-5e4)   (eva.py:204-218,
 *                                                                local_attention.py:159-170)
 *     logits_cv    = s q.lk_c                                    (eva.py:200)
 *     out = P_local V_window + P_cv lv                           (eva.py:222-227)
 * With L == 0 this is LocalAttention._apply_attention (local_attention.py:134-182).
 *   lk, lv : fp32 [B,H,L,D] (rf_k_bar and beta), may be NULL iff L == 0
 *   bias   : fp32 [H, Wq, ea_window_bias_ld(g)] dense per-head bias MULTIPLIED BY log2(e) (the
 *            softmax runs in the log2 domain), rows padded, or NULL; dbias_part is d/d(natural bias)
 *   lse    : fp32 [B,H,N] joint log-sum-exp (natural log), saved for backward; a caller that merges this
 *            attention with further softmax columns of its own (ScatterBrain's low-rank part) uses it
 *            as an output and passes its gradient `dlse` [B,H,N] to the backward (NULL otherwise)
 * With ea_geom.causal the windows, masks and chunk visibility follow causal_eva.py:666-783 (see the
 * field's comment); Wk = window + ext there.
 *   keep   : attention dropout of causal_eva.py:778 (`attn = dropout(attn)` on the joint softmax):
 *            uint8 [B,H,N, ea_window_keep_ld(g)] -- for query n, column j < Wk is local slot j and
 *            column ea_window_bias_ld(g) + c is landmark c; non-zero = kept.  Kept probabilities are
 *            multiplied by keep_scale = 1/(1-p); the normaliser (lse) is that of the full row.
 *            NULL = no dropout.  Only with ea_geom.causal != 0 (the only module that applies it).
 * Backward consumes the forward's out, lse and dout and produces dq, dk, dv (WRITTEN, not
 * accumulated).  It runs as one launch per group of (window, query block) pairs that share no key:
 * with overlapping windows (ext > 0) a token is a key of several windows, and a 1-D window whose
 * rows do not fit one LDS image (e.g. window 128 at D = 128) is processed in
 * ea_window_bwd_query_blocks(g) blocks of queries (launched together when the windows do not
 * overlap, each block with its own scratch slice).  The caller then passes two fp32 scratch buffers
 * dk_acc, dv_acc of [ea_window_bwd_acc_slices(g), B,H,N,D] (initialised inside) that collect the
 * key/value gradients before they are summed and converted into dk/dv; they may be NULL when that
 * count is 0.  With more than one query block dbias_part must be ZEROED by the caller (a block
 * writes only its own rows).
 * The landmark and bias gradients come back as per-workgroup partial sums which the caller
 * reduces over the leading axes:
 *   dlk_part, dlv_part : fp32 [ea_window_bwd_parts(g), B*H, L, D]
 *   dbias_part         : fp32 [ea_window_bwd_bias_parts(g), B, H, Wq, ld]   (NULL iff bias NULL)
 *   bias_t             : fp32 [H, ld, 16*ceil(Wq/16)] transposed copy of `bias` (rows padded with
 *                        zeros).  Only read when the head's bias table does not fit next to the
 *                        window in LDS (ea_window_bwd_needs_bias_t(g) == 1); may be NULL otherwise. */
int32_t ea_window_bias_ld(const ea_geom* g);        /* padded row length of `bias`           */
int32_t ea_window_bwd_parts(const ea_geom* g);      /* leading dim of dlk_part / dlv_part    */
int32_t ea_window_bwd_bias_parts(const ea_geom* g); /* leading dim of dbias_part             */
int32_t ea_window_bwd_needs_bias_t(const ea_geom* g);
int32_t ea_window_bwd_acc_slices(const ea_geom* g); /* [B,H,N,D] slices of dk_acc / dv_acc  */
int32_t ea_window_bwd_query_blocks(const ea_geom* g); /* > 1: dbias_part must be zeroed      */
int32_t ea_window_keep_ld(const ea_geom* g);        /* row length of `keep`                  */
int ea_window_attn_fwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                       const float* lk, const float* lv, const float* bias, const uint8_t* mask,
                       const ea_t4* out, float* lse, const uint8_t* keep, float keep_scale,
                       void* stream);
int ea_window_attn_bwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                       const float* lk, const float* lv, const float* bias, const uint8_t* mask,
                       const ea_t4* out, const ea_t4* dout, const float* lse,
                       const ea_t4* dq, const ea_t4* dk, const ea_t4* dv,
                       float* dlk_part, float* dlv_part, float* dbias_part,
                       float* dk_acc, float* dv_acc, const float* bias_t,
                       const uint8_t* keep, float keep_scale, const float* dlse, void* stream);

/* ---- LARA: linear randomized attention (lara.py:177-251) -------------------------------------
 * C landmark samples omega_c (C = L, or 2L with antithetic / multi-sample noise), each token n:
 *   log_proj_k[c,m] = s w_c.k_m - s|k_m|^2/2 (-inf on padded keys)          (lara.py:202-208)
 *   kv_stats_c = sum_m softmax_m(log_proj_k[c,:]) v_m,  lse_k[c] = LSE_m log_proj_k   (:211,241)
 *   mis-opt:  t[c,n] = softmax_n(s qbar_c.q_n); alpha = bh_c + kappa (t - mean_c t);
 *             log_alpha = log max(alpha, 1e-8)                               (:221-232)
 *   mis-biased: log_alpha = s qbar_c.q_n (qbar := mu rows)                   (:214-220)
 *   mis-bh:   log_alpha = 0                                                  (:233-236)
 *   W[c,n] = softmax_c(log_alpha + s w_c.q_n + cst_c),  cst_c = lse_k[c] - log_proposal_c
 *   out_n = sum_c W[c,n] kv_stats_c                                          (:241-246)
 * Landmark-side tensors are fp32: omega, qbar, kv, dkv, uq [B*H, C, D]; per-landmark scalars
 * [B*H, C]; per-token scalars [B*H, N].  The sequence-wide sums come back as partial results over
 * S = ea_lara_parts(g) slices that the caller merges (log-sum-exp merge for the forward
 * statistics, plain sums for the backward ones):
 *   stats_fwd : p_ml [B*H, S, C, 4] = (max_k, sum_k, max_t, sum_t) in natural-log units of the
 *               running maxima, p_kv [B*H, S, C, D] un-normalised sum_m exp(lpk - max_k) v_m
 *   bwd_qstats: p_ml = (r_c = sum_n dZ, sum_n dalpha, u_c = sum_n t dt, 0);
 *               p_dkv = d kv_stats; p_dom = sum_n dZ q_n; p_m1 = sum_n t dt q_n; p_m2 = sum_n t q_n
 *   bwd_kstats: p_dom = sum_m dBk[c,m] k_m  (caller scales d omega by s)
 * bwd_q writes the sequence-local part of dq plus the per-token scalars bwd_qstats consumes;
 * bwd_qcorr subtracts s sum_c t[c,n] uq_c (uq_c = u_c qbar_c) from dq in place (mis-opt only);
 * bwd_k writes dk, dv given dkv, lse_k, dkk_c = dkv_c.kv_c and rsum_c = r_c. */
#define EA_MIS_OPT    0
#define EA_MIS_BIASED 1
#define EA_MIS_BH     2
typedef struct {
  int32_t B, H, N, D;
  int32_t dtype;             /* EA_BF16 | EA_F16 */
  int32_t C;                 /* landmark samples, <= 128 */
  int32_t mis;               /* EA_MIS_* */
  float   kappa;             /* alpha_coeff (lara.py:231) */
  float   scale;             /* D^-0.5 */
} ea_lara_geom;

int32_t ea_lara_parts(const ea_lara_geom* g);
int ea_lara_stats_fwd(const ea_lara_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                      const uint8_t* mask, const float* omega, const float* qbar,
                      float* p_ml, float* p_kv, void* stream);
/* lseZ / tmean (both or neither; fp32 [B*H, N]): the per-token statistics of the estimator's softmax over the samples,
 * log2(sum_c alpha 2^z) and mean_c t, kept for ea_lara_bwd_q_fused (8 bytes per token-head). */
int ea_lara_out_fwd(const ea_lara_geom* g, const ea_t4* q, const float* omega, const float* qbar,
                    const float* kv, const float* lse_t, const float* bhv, const float* cst,
                    const ea_t4* out, float* lseZ, float* tmean, void* stream);
int ea_lara_bwd_q(const ea_lara_geom* g, const ea_t4* q, const ea_t4* dout, const float* omega,
                  const float* qbar, const float* kv, const float* lse_t, const float* bhv,
                  const float* cst, const ea_t4* dq, float* lseZ, float* tmean, float* rowdot,
                  float* sda, void* stream);
int ea_lara_bwd_qstats(const ea_lara_geom* g, const ea_t4* q, const ea_t4* dout, const float* omega,
                       const float* qbar, const float* kv, const float* lse_t, const float* bhv,
                       const float* cst, const float* lseZ, const float* tmean, const float* rowdot,
                       const float* sda, float* p_ml, float* p_dkv, float* p_dom, float* p_m1,
                       float* p_m2, void* stream);
int ea_lara_bwd_k(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                  const float* omega, const float* dkv, const float* lse_k, const float* dkk,
                  const float* rsum, const ea_t4* dk, const ea_t4* dv, void* stream);
int ea_lara_bwd_kstats(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                       const float* omega, const float* dkv, const float* lse_k, const float* dkk,
                       const float* rsum, float* p_dom, void* stream);
int ea_lara_bwd_qcorr(const ea_lara_geom* g, const ea_t4* q, const float* qbar, const float* uq,
                      const float* lse_t, const ea_t4* dq, void* stream);

/* Fused backward (round 2): the elementwise stage of the estimator is evaluated once per side and its
 * [C x N] weight matrices are transposed through LDS, so q/dout and k/v are each read ONCE
 * (ea_lara_bwd_q + ea_lara_bwd_qstats, ea_lara_bwd_k + ea_lara_bwd_kstats of round 1 read them
 * twice), and (round 3) the softmax statistics lseZ / tmean of ea_lara_out_fwd are re-used instead of re-derived.
 * C <= 64.  Partial outputs [BH, ea_lara_fused_parts(g), C, *] feed ea_lara_merge_bwd /
 * ea_slice_sum unchanged.  Replaces the autograd of lara.py:201-246.
 * ea_lara_bwd_finish: dq -= s sum_c t[c,n] (u q_bar)_c (softmax-over-sequence correction, uq may be
 * NULL) and, with pool_r > 0, the backward of the uniform pool_r x pool_r average pooling of q and k
 * over the gh x gw token grid (lara.py:43,48,145-151): dq += dpq[chunk(n)] / r^2, dk += dpk[...] / r^2. */
int32_t ea_lara_fused_parts(const ea_lara_geom* g);
int ea_lara_bwd_q_fused(const ea_lara_geom* g, const ea_t4* q, const ea_t4* dout, const float* omega,
                        const float* qbar, const float* kv, const float* lse_t, const float* bhv,
                        const float* cst, const float* lseZ, const float* tmean, const ea_t4* dq, float* p_ml,
                        float* p_dkv, float* p_dom, float* p_m1, float* p_m2, void* stream);
int ea_lara_bwd_k_fused(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                        const float* omega, const float* dkv, const float* lse_k, const float* dkk,
                        const float* rsum, const ea_t4* dk, const ea_t4* dv, float* p_dom, void* stream);
int ea_lara_bwd_finish(const ea_lara_geom* g, const ea_t4* q, const float* qbar, const float* uq,
                       const float* lse_t, const float* dpq, const float* dpk, int32_t pool_r,
                       int32_t gh, int32_t gw, const ea_t4* dq, const ea_t4* dk, void* stream);

/* ---- softmax baseline (abstract_attention.py:120-133) ----------------------------------------
 * out = dropout(softmax(s Q K^T, -inf on padded keys)) V, streamed (no [N,N] score matrix).
 * lse: fp32 [B*H, N] saved for backward; delta: fp32 [B*H, N] scratch (dO.O) written by the dQ
 * pass and read by the dK/dV pass of ea_softmax_attn_bwd.
 * keep: attention dropout (`attn = self.attn_drop(attn)`, :131): uint8 [B,H,N, 64*ceil(N/64)], entry
 * (n, j) non-zero = probability of key j for query n is kept and multiplied by keep_scale = 1/(1-p);
 * NULL = no dropout.  q, k, v may be views of different tensors (any strides, rows contiguous). */
int ea_softmax_attn_fwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t dtype, float scale,
                        const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                        const ea_t4* out, float* lse, const uint8_t* keep, float keep_scale,
                        int32_t key_norm_bias, void* stream);
int ea_softmax_attn_bwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t dtype, float scale,
                        const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                        const ea_t4* out, const ea_t4* dout, const float* lse, float* delta,
                        const ea_t4* dq, const ea_t4* dk, const ea_t4* dv,
                        const uint8_t* keep, float keep_scale, int32_t key_norm_bias, void* stream);
/* ABI 37.  The 16-token tiles per wave (QT) the softmax launcher uses: which 0 = forward (1, 2 or 4 query tiles), 1 = backward
 * (1 or 2; the dQ pass and the dK/dV pass use the same count); has_keep: a keep mask is passed; cus > 0: for a device of that
 * many compute units (pure, runs without a GPU); cus = 0: the current device's.  The launcher calls the same function, so
 * what this answers is what runs:
 *   forward   4 if D <= 64 and B H ceil(N / 256) >= 2 cus; else 2 if B H ceil(N / 128) >= 2 cus; else 1; at most 2 when
 *             D > 64 or a keep mask is passed
 *   backward  2 if D <= 64 and B H ceil(N / 128) >= 2 cus; else 1
 * The dev knobs EA_SM_QT (forward: 1, 2 or 4) and EA_SM_BQT (backward: 1 or 2), read once per process, replace the count
 * before the clamps for D > 64 and the keep mask; any other value of a knob is ignored.
 * -> 1, 2 or 4, or a negative EA_E* code for a geometry ea_softmax_attn_fwd refuses (B, H, N <= 0, D not 32 / 64 / 128) and
 * for which not 0 / 1 or cus < 0. */
int32_t ea_softmax_tiles(int32_t which, int32_t B, int32_t H, int32_t N, int32_t D, int32_t has_keep, int32_t cus);
/* Randomized attention (randomized_attention.py:21-52) is two passes of the kernels above:
 *   mu = q + softmax(s q k^T) k (num_samples = -1) or q + k[index] with one index per query drawn
 *   from softmax(s q k^T) (ea_softmax_sample: Gumbel-max with counter-based noise from the 64-bit
 *   device scalar `seed`; index: int64 [B*H, N]); then out = softmax_j(s w.k_j - s |k_j|^2 / 2) v_j
 *   with w = mu (+ noise): key_norm_bias = 1 adds the per-key term and its gradient to dk
 *   (not combined with `keep`). */
int ea_softmax_sample(int32_t B, int32_t H, int32_t N, int32_t D, int32_t dtype, float scale,
                      const ea_t4* q, const ea_t4* k, const uint64_t* seed, int64_t* index, void* stream);

/* ---- Performer / FAVOR+ baseline (kernelized_attention.py:20-56,116-121,326-346) ---------------
 * phi(x)[j] = M^-1/2 exp(d^-1/4 W_j.x - d^-1/2 |x|^2/2 - stab) + 1e-4 with W fp32 [H, M, D] (fresh
 * Gaussian features per training call, `eval_proj` otherwise); stab = max_j for queries, the max
 * over all keys and features of one (b,h) for keys (detached); phi(k) is zeroed at padded keys.
 *   kv[j] = sum_n phi(k_n)[j] v_n,  ksum[j] = sum_n phi(k_n)[j]
 *   out_n = phi(q_n).kv / max(phi(q_n).ksum, 1e-2)
 * Sequence-wide sums come back as partials over S = ea_performer_parts(g) slices (p_ml[...,0] holds
 * the scalar per feature: max of d^-1/4 W_j.k_n for kmax, ksum for kv, d(ksum) for bwd_qstats). */
typedef struct {
  int32_t B, H, N, D;
  int32_t dtype;
  int32_t M;                 /* number of random features (approx_attn_dim), <= 128 */
} ea_perf_geom;
int32_t ea_performer_parts(const ea_perf_geom* g);
int ea_performer_kmax(const ea_perf_geom* g, const ea_t4* k, const float* W, float* p_ml, void* stream);
int ea_performer_kv(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                    const float* W, const float* stab, float* p_ml, float* p_kv, void* stream);
int ea_performer_out(const ea_perf_geom* g, const ea_t4* q, const float* W, const float* kv,
                     const float* ksum, const ea_t4* out, void* stream);
int ea_performer_bwd_q(const ea_perf_geom* g, const ea_t4* q, const ea_t4* out, const ea_t4* dout,
                       const float* W, const float* kv, const float* ksum, const ea_t4* dq,
                       float* stabq, float* invden, float* dden, void* stream);
int ea_performer_bwd_qstats(const ea_perf_geom* g, const ea_t4* q, const ea_t4* dout, const float* W,
                            const float* stabq, const float* invden, const float* dden,
                            float* p_ml, float* p_dkv, void* stream);
int ea_performer_bwd_k(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                       const float* W, const float* stab, const float* dkv, const float* dksum,
                       const ea_t4* dk, const ea_t4* dv, void* stream);

/* ---- LARA 'adaptive-1d' proposals with the generator INSIDE the segment kernels (ea_lara_seglin.hip; round 4) ----
 * q_bar_l = mean over segment l of LayerNorm(G_q q_n + g_q), k_bar_l likewise (lara.py:56-63,84-127), straight from the
 * stored q / k rows: generator Linear (a [64 x 64] MFMA product per 16 tokens), LayerNorm and segment mean in one pass; the
 * qkv projection stays 3C wide (the folded form below makes all three GEMMs of the layer 5C wide).  g: B, H, N, D = 64,
 * dtype, L (segments as in ea_lara_segment_*); G [64, 64] (out, in), g_b, ln_w, ln_b [64]: fp32.
 *   fwd: qbar, kbar [B*H, L, 64] fp32.
 *   bwd: ACCUMULATES G^T d z into dq / dk (the attention core's gradient rows, I/O dtype); with S = B*H*
 *        ea_lara_seglin_groups(g): part [S, 2, 4, 64] = partial sums of (d ln_w, d ln_b, d g_b, 0) per side, dG_part
 *        [S, 2, 64, 64] = partial sums of dG (side 0: q generator) -- the caller adds them over S; stats: scratch of
 *        B*H*2*N*4 floats (16-byte aligned) in which the dq / dk pass leaves every token's LayerNorm statistics for the dG
 *        pass. */
int32_t ea_lara_seglin_groups(const ea_geom* g);
int ea_lara_seglin_fwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const float* Gq, const float* gq_b, const float* Gk,
                       const float* gk_b, const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                       float* qbar, float* kbar, void* stream);
int ea_lara_seglin_bwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const float* Gq, const float* gq_b, const float* Gk,
                       const float* gk_b, const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                       const float* d_qbar, const float* d_kbar, const ea_t4* dq, const ea_t4* dk, float* part, float* dG_part,
                       float* stats, void* stream);
/* round 6: the same backward with the estimator's LAST correction of dq riding on the dq / dk pass -- what ea_lara_bwd_finish
 * applies in a pass of its own (lara.py:223 differentiated: t = softmax over the sequence of s qbar_c . q_n,
 *     dq_n -= s sum_c t[c, n] (u qbar)_c ),
 * added to the rows this pass rewrites anyway (the q rows are its MFMA operand already): one read-modify-write of dq less per
 * step.  fin_qbar, fin_uq [B*H, C, 64], fin_lse_t [B*H, C] fp32 as ea_lara_bwd_finish takes them (qbar, uq, lse_t); C <= 64
 * samples (EA_E_UNSUPPORTED beyond); scale = d^-1/2.  The caller must NOT run ea_lara_bwd_finish for the same step. */
int ea_lara_seglin_bwd_fin(const ea_geom* g, const ea_t4* q, const ea_t4* k, const float* Gq, const float* gq_b, const float* Gk,
                           const float* gk_b, const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                           const float* d_qbar, const float* d_kbar, const ea_t4* dq, const ea_t4* dk, float* part,
                           float* dG_part, float* stats, const float* fin_qbar, const float* fin_uq, const float* fin_lse_t,
                           int32_t C, float scale, void* stream);

/* ---- LARA 'adaptive-1d' proposals: the generators' per-token Linear folded into the qkv projection (ea_fold.hip) ----
 * q_bar_gen / k_bar_gen start with Linear(d, d) on every token's q / k row (lara.py:56-63,100-103).  The module computes
 * Linear_gen(q) as two more groups of output columns of the qkv GEMM (W' = G W_head per head); these two entry points
 * build the extended weight and take its gradient apart in one launch each way (round 4; ~30 framework kernels before).
 *   fwd: w_ext [5C, C] (EA dtype) = [ W ; Gq W_q,head ; Gk W_k,head ], b_ext [5C] (EA dtype, may be NULL) = [ b ; 0 ],
 *        bias_q / bias_k [heads, d] fp32 = G b_head + g_b: the bias of a folded row (consumed by ea_lara_segment_*).
 *        W [3C, C], b [3C] (may be NULL), Gq / Gk [d, d], gq_b / gk_b [d]: fp32 parameters.
 *   bwd: from dW_ext [5C, ldw] / db_ext [5C] (the weight / bias gradient of the extended projection, e.g. ea_wgrad's sums)
 *        and dbias_q / dbias_k [heads, d]: dW [3C, C], db [3C] (NULL when b is), dG [2, d, d] = (dGq, dGk), dgq_b, dgk_b [d].
 *        dG_part: scratch of (2 * ea_lara_fold_parts(heads) + 2) * d * d floats (per-head partials of dG; the entry point
 *        adds them up with ea_slice_sum).  d = 64 (EA_E_UNSUPPORTED otherwise). */
int ea_lara_fold_fwd(int32_t dtype, int32_t C, int32_t heads, const float* W, const float* b, const float* Gq, const float* gq_b,
                     const float* Gk, const float* gk_b, void* w_ext, void* b_ext, float* bias_q, float* bias_k, void* stream);
int32_t ea_lara_fold_parts(int32_t heads);
int ea_lara_fold_bwd(int32_t C, int32_t heads, const float* W, const float* b, const float* Gq, const float* Gk,
                     const float* dW_ext, int64_t ldw, const float* db_ext, const float* dbias_q, const float* dbias_k,
                     float* dW, float* db, float* dG, float* dG_part, float* dgq_b, float* dgk_b, void* stream);

/* ---- Performer in EXACT fp32 arithmetic (ea_performer_f32.hip; round 4) --------------------
 * The reference computes its linear attention in full precision whatever the AMP state (kernelized_attention.py:116-121
 * `autocast(enabled=False)`, :343-345 `.float()`), and a module called outside autocast computes everything in fp32
 * (abstract_attention.py:120-133).  These entry points are that arithmetic: q, k, v, dout of type g->dtype = EA_BF16 /
 * EA_F16 / EA_F32 (16-bit values are exact in fp32), every product on v_mfma_f32_16x16x4_f32 with fp32 operands, fp32
 * features phi, outputs in g->dtype.  D = 64, M <= 96 (multiple of 16); W [H, M, 64] fp32.
 *   S = ea_performer_f32_parts(g) sequence slices per (b,h);
 *   kmax : p_max [BH,S]  = slice maxima of d^-1/4 W_j.k_n (the key stabiliser is their maximum; padded keys included,
 *          as in the reference, which masks the features afterwards);
 *   kv   : p_kv [BH,S,M,64], p_ksum [BH,S,M] = partial sum_n phi(k_n)^T v_n, sum_n phi(k_n) (padded keys: phi = 0);
 *          the caller adds the slices (ea_slice_sum) -> kv [BH,M,64], ksum [BH,M];
 *   out  : out_n = phi(q_n) kv / max(phi(q_n).ksum, 1e-2);
 *   bwd_q: dq, and the slice partials of d kv, d ksum (same shapes as kv's);  bwd_k: dk, dv from the summed d kv, d ksum.
 * Replaces favorp_projection + linear_attention and their autograd (kernelized_attention.py:20-56,116-121). */
int32_t ea_performer_f32_parts(const ea_perf_geom* g);
int ea_performer_f32_kmax(const ea_perf_geom* g, const ea_t4* k, const float* W, float* p_max, void* stream);
int ea_performer_f32_kv(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                        const float* p_max, float* p_kv, float* p_ksum, void* stream);
int ea_performer_f32_out(const ea_perf_geom* g, const ea_t4* q, const float* W, const float* kv, const float* ksum,
                         const ea_t4* out, void* stream);
int ea_performer_f32_bwd_q(const ea_perf_geom* g, const ea_t4* q, const ea_t4* dout, const float* W, const float* kv,
                           const float* ksum, const ea_t4* dq, float* p_dkv, float* p_dksum, void* stream);
int ea_performer_f32_bwd_k(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                           const float* p_max, const float* dkv, const float* dksum, const ea_t4* dk, const ea_t4* dv,
                           void* stream);

/* ---- Kernelized attention: the reference's feature maps in EXACT fp32 arithmetic (ABI 16; ea_kernelized.hip) ---------
 * KernelizedAttention (kernelized_attention.py) with proj_method = favorp / relu / fourier / relu-only / sigmoid-only / dpfp,
 * optionally cos weighting (cosFormer): out_n = phi(q_n) kv / max(phi(q_n).ksum, 1e-2), kv = sum_n phi(k_n)^T v_n,
 * ksum = sum_n phi(k_n), phi(k) = 0 at padded keys.  c = d^-1/4, c2 = d^-1/2 / 2, r = M^-1/2, W fp32 [H, M, 64]:
 *   EA_KZ_FAVORP        r exp(c W x - c2|x|^2 - stab) + 1e-4   (stab: row max for queries, max over (tokens, j) for keys)
 *   EA_KZ_RELU          relu(r c W x) + 1e-3
 *   EA_KZ_FOURIER       r [sin(c W x), cos(c W x)] exp(c2|x|^2 - max_n c2|x_n|^2)   (max per side over the sequence)
 *   EA_KZ_RELU_ONLY     relu(x) + 0.1;   EA_KZ_SIGMOID_ONLY  sigmoid(x) + 0.1   (no W)
 *   EA_KZ_DPFP          x' = [relu(x), relu(-x)];  concat_{j=1..nu} x' * roll(x', j)   (no W)
 * Stabilisers are detached.  cos = 1 doubles the features to [phi cos t_n, phi sin t_n], t_n = (pi/2) n / N.
 * Geometry: D = 64; M <= 128, multiple of 16 (maps with W); F = features after cos weighting <= 256 (M, 2M, 64 or 128 nu,
 * times 2 with cos).  q, k, v, dout of type dtype = EA_BF16 / EA_F16 / EA_F32, fp32 features and products, outputs in dtype.
 *   S = ea_kernelized_parts(g) sequence slices per (b,h);
 *   stats (favorp, fourier only): p_st [BH,S,2] = slice maxima (favorp: of the key logits c W_j.k_n, side 0; fourier: of
 *          c2|k_n|^2, side 0, and c2|q_n|^2, side 1; padded tokens included, as in the reference);
 *   kv   : p_kv [BH,S,F,64], p_ksum [BH,S,F] partials (added by ea_slice_sum -> kv [BH,F,64], ksum [BH,F]);
 *   out  : out from the summed kv, ksum;
 *   bwd_q: dq and the partials of d kv, d ksum (shapes of p_kv, p_ksum);  bwd_k: dk, dv from the summed d kv, d ksum;
 *   p_dw : NULL, or (learnable W) [H, B, 2, S, M, 64] partials of dW, side 0 written by bwd_q, side 1 by bwd_k -- the
 *          caller adds the B * 2 * S partials of each head (ea_slice_sum).
 * p_st is NULL for the maps without statistics.  Replaces the feature maps, (cos_reweighted_)linear_attention and their
 * autograd (kernelized_attention.py:13-123,326-346). */
#define EA_KZ_FAVORP        0
#define EA_KZ_RELU          1
#define EA_KZ_FOURIER       2
#define EA_KZ_RELU_ONLY     3
#define EA_KZ_SIGMOID_ONLY  4
#define EA_KZ_DPFP          5
typedef struct {
  int32_t B, H, N, D;
  int32_t dtype;             /* EA_BF16 | EA_F16 | EA_F32 */
  int32_t map;               /* EA_KZ_* */
  int32_t M;                 /* rows of W (approx_attn_dim); ignored by the maps without W */
  int32_t F;                 /* features after cos weighting */
  int32_t nu;                /* dpfp: number of rolls, >= 1 */
  int32_t cos;               /* 1: cos weighting */
} ea_kz_geom;
int32_t ea_kernelized_parts(const ea_kz_geom* g);
int ea_kernelized_stats(const ea_kz_geom* g, const ea_t4* q, const ea_t4* k, const float* W, float* p_st, void* stream);
int ea_kernelized_kv(const ea_kz_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                     const float* p_st, float* p_kv, float* p_ksum, void* stream);
int ea_kernelized_out(const ea_kz_geom* g, const ea_t4* q, const float* W, const float* p_st, const float* kv,
                      const float* ksum, const ea_t4* out, void* stream);
int ea_kernelized_bwd_q(const ea_kz_geom* g, const ea_t4* q, const ea_t4* dout, const float* W, const float* p_st,
                        const float* kv, const float* ksum, const ea_t4* dq, float* p_dkv, float* p_dksum, float* p_dw,
                        void* stream);
int ea_kernelized_bwd_k(const ea_kz_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                        const float* p_st, const float* dkv, const float* dksum, const ea_t4* dk, const ea_t4* dv,
                        float* p_dw, void* stream);

/* ---- LARA landmark pipeline, fused (lara.py:145-198,214-238) -----------------------------------
 * One workgroup per (b,h); fp32 in and out, the row-wise steps (LayerNorm, softmax, norms, column sums) in fp32, every
 * matrix product on fp16 MFMA operands with fp32 accumulation (the gradient-side ones behind a power-of-two scale):
 *   q_bar = LN(pq Wq^T + bq), k0 = LN(pk Wk^T + bk)         (has_mlp; else q_bar = pq, k0 = pk)
 *   k_bar = softmax(s k0 k0^T) k0                            (mixed; else k_bar = k0)
 *   mu = q_bar + k_bar;  omega_c = mu[c mod L] + eps_c       (dup 0: C = L; 1 antithetic: C = 2L,
 *                                                             eps [BH,L,D], second half negated;
 *                                                             2 multi-sample: C = 2L, eps [BH,2L,D])
 *   M[c,l] = s omega_c.mu_l - s|mu_l|^2/2
 *   mis-opt   : lp_c = M[c, c mod L]; bh_c = exp(lp_c - LSE over the C (repeated) columns);
 *               qbar_rows_c = q_bar[c mod L]
 *   mis-biased: lp_c = LSE_l M[c,l]; qbar_rows_c = mu[c mod L];   mis-bh: lp_c = LSE_l M[c,l]
 * Outputs omega, qbar_rows [BH,C,D], bhv, lp [BH,C] feed ea_lara_*.  The backward takes their
 * gradients and returns d pq, d pk [BH,L,D] plus per-(b,h) partial parameter gradients
 * dW_part [BH,2,D,D] (q then k; [out][in]) and dvec_part [BH,2,3,D] (Linear bias, LN weight, LN
 * bias) which the caller sums over BH.  L, C <= 64 and D in {32, 64}: every entry of this block, the size
 * query included, answers EA_E_UNSUPPORTED for a well-formed geometry outside them (D = 128, L = 65, C = 128) and
 * EA_E_BADARG for a malformed one (C != L without dup, C != 2 L with it, mis or dup out of range, eva with dup or
 * without the MLP), before anything is launched.
 * `saved`: workspace of ea_lara_landmarks_saved_floats(g) floats in which the forward keeps its
 * intermediates (normalised rows, LayerNorm 1/std, mixing matrix, mu) for the backward.  NULL in a
 * forward that will not be differentiated; the backward of a parametrised (has_mlp) or mixed pipeline
 * REQUIRES it (EA_E_BADARG otherwise -- round 3 retired the kernels that recomputed the forward). */
typedef struct {
  int32_t BH, L, C, D;
  int32_t has_mlp, mixed, mis, dup;
  float   scale;
  int32_t eva;               /* 1: EVA's mu pipeline instead (eva.py:178-190, adaptive_proj='default'):
                                qbar_rows = rf_k_bar = LN(pk Wk^T + bk), omega = (rf_q_bar + rf_k_bar)/2 + eps;
                                bhv / lp unused; the backward takes d_omega and d_qbar_rows = d rf_k_bar */
} ea_lmk_geom;
int ea_lara_landmarks_fwd(const ea_lmk_geom* g, const float* pq, const float* pk,
                          const float* Wq, const float* bq, const float* gq, const float* cq,
                          const float* Wk, const float* bk, const float* gk, const float* ck,
                          const float* noise, float* omega, float* qbar_rows, float* bhv, float* lp,
                          float* saved, void* stream);
int64_t ea_lara_landmarks_saved_floats(const ea_lmk_geom* g);
int ea_lara_landmarks_bwd(const ea_lmk_geom* g, const float* pq, const float* pk,
                          const float* Wq, const float* bq, const float* gq, const float* cq,
                          const float* Wk, const float* bk, const float* gk, const float* ck,
                          const float* noise, const float* d_omega, const float* d_qbar_rows,
                          const float* d_bhv, const float* d_lp, float* dpq, float* dpk,
                          float* dW_part, float* dvec_part, const float* saved, void* stream);
/* '-vmixed' proposals (lara.py:171-172): colbias [BH, L] = log(|v_bar_l'| + 1e-4) is added to column l' of the mixing
 * logits s k0 k0^T before their softmax; the backward also returns d_colbias [BH, L] (column sums of the logit
 * gradients).  g->mixed must be set and `saved` (the forward intermediates) is required in the backward; geometries
 * outside the second-generation kernels (L, C <= 64, D in {32, 64}) return EA_E_UNSUPPORTED. */
int ea_lara_landmarks_fwd_cb(const ea_lmk_geom* g, const float* pq, const float* pk,
                             const float* Wq, const float* bq, const float* gq, const float* cq,
                             const float* Wk, const float* bk, const float* gk, const float* ck,
                             const float* noise, const float* colbias, float* omega, float* qbar_rows, float* bhv,
                             float* lp, float* saved, void* stream);
int ea_lara_landmarks_bwd_cb(const ea_lmk_geom* g, const float* pq, const float* pk,
                             const float* Wq, const float* bq, const float* gq, const float* cq,
                             const float* Wk, const float* bk, const float* gk, const float* ck,
                             const float* noise, const float* colbias, const float* d_omega, const float* d_qbar_rows,
                             const float* d_bhv, const float* d_lp, float* dpq, float* dpk,
                             float* dW_part, float* dvec_part, float* d_colbias, const float* saved, void* stream);

/* ---- LARA: merging the sequence slices of the token-row passes (tiny, one workgroup per (b,h)) ----
 * merge_fwd: (p_ml, p_kv of ea_lara_stats_fwd over S slices, lp) -> kv_stats [BH,C,D], lse_k,
 *   lse_t (has_t: mis-opt) and cst = lse_k - lp [BH,C].
 * merge_bwd: (p_ml, p_dkv, p_dom, p_m1, p_m2 of ea_lara_bwd_qstats) -> r, d(bh), d(lp) = -r,
 *   dkk = dkv.kv [BH,C]; dkv, domq = sum_n dZ q_n [BH,C,D]; with has_t also
 *   dqbar = s (M1 - u M2) and uq = u qbar; without, dqbar (if non-NULL) = s domq (mis-biased). */
int ea_lara_merge_fwd(int32_t BH, int32_t S, int32_t C, int32_t D, int32_t has_t,
                      const float* p_ml, const float* p_kv, const float* lp,
                      float* kv, float* lse_k, float* lse_t, float* cst, void* stream);
int ea_lara_merge_bwd(int32_t BH, int32_t S, int32_t C, int32_t D, int32_t has_t, float scale,
                      const float* p_ml, const float* p_dkv, const float* p_dom, const float* p_m1,
                      const float* p_m2, const float* kv, const float* qbar,
                      float* r, float* dbh, float* dlp, float* dkk, float* dkv, float* domq,
                      float* dqbar, float* uq, void* stream);

/* ---- projection bias gradient: db[c] = sum_t dY[t][c] ----
 * Replaces the bias-gradient reduction autograd runs for the qkv / output nn.Linear of every
 * attention module (abstract_attention.py:34-36 `self.qkv`, `self.proj`; eva.py:76-77, lara.py:88-90):
 * dY is the contiguous [rows = B*N, cols] cotangent of the projection output in the I/O dtype,
 * db is fp32 [cols].  Deterministic two-stage sum; `part` is caller workspace of
 * ea_bias_grad_parts(rows, cols) * cols floats.  cols % 8 == 0, cols <= 16384. */
int ea_bias_grad_parts(int32_t rows, int32_t cols);
int ea_bias_grad(int32_t dtype, int32_t rows, int32_t cols, const void* dy, float* part, float* db,
                 void* stream);

/* ---- small fp32 reductions around the cores (replace chains of tiny torch kernels) ----
 * ea_colsum_f32: out[c] = sum_r x[r][c], x fp32 [rows, cols] contiguous, fixed summation order.
 *   Used for the per-(b,h) partials of the landmark-MLP parameter gradients
 *   (ea_lara_landmarks_bwd dW_part / dvec_part: autograd's accumulation over the batch for
 *   q_bar_gen / k_bar_gen, lara.py:45-54, eva.py:93-103).
 * ea_slice_sum: out[bh][j] = scale * (a[bh][j] + sum_s parts[bh][s][j]), j < n (n % 4 == 0), a may
 *   be NULL.  Used for d(omega) = s (d_omega_q + sum over sequence slices of ea_lara_bwd_kstats). */
int ea_colsum_f32(int32_t rows, int32_t cols, const float* x, float* out, void* stream);
/* Two column sums over the same rows in one launch (dW_part and dvec_part of the landmark backward). */
int ea_colsum2_f32(int32_t rows, int32_t cols1, const float* x1, float* out1, int32_t cols2, const float* x2, float* out2,
                   void* stream);
/* Gradient of a table gather (the relative-position bias table read through `relative_position_index`,
 * local_attention.py:70-79): out[row][c] = sum_k g[inv[row][k]][c], inv [rows, K] int32 = the gather positions that read
 * table row `row` (-1 = unused slot), g [n, cols] fp32.  Fixed order (deterministic). */
int ea_gather_sum(int32_t rows, int32_t K, int32_t cols, const float* g, const int32_t* inv, float* out, void* stream);
/* Round 6: the dense per-head bias of the window kernels straight out of its table, in ONE launch each way (replaces the
 * index_select / permute / multiply / pad / copy chain around `relative_position_bias_table[relative_position_index]`,
 * local_attention.py:70-79, and around T5RelativePositionBias.forward, eva.py:53-65, causal_eva.py:206-300):
 *   fwd: out[hd][i][j] = scale * table[idx[i*Wk + j]][hd] for j < Wk, 0 for Wk <= j < ld      (table [rows, th] fp32, idx int32
 *        [Wq*Wk], out [h, Wq, ld] fp32 -- ld = ea_window_bias_ld(geom); `scale` carries log2(e), the kernels' logit unit)
 *   bwd: dtable[row][hd] = scale * sum_k g[hd][p / Wk][p % Wk], p = inv[row][k] >= 0           (g [h, Wq, ld] fp32 = the bias
 *        gradient the window backward returns; inv [rows, K] int32 as for ea_gather_sum).  Fixed order (deterministic).
 *   th (fwd, ABI 13) = heads of the table: h, or 1 = one column broadcast over the h heads (causal EVA's single-head T5
 *        table); bwd always fills dtable [rows, h] -- the gradient of a one-column table is its sum over the heads. */
int ea_table_bias_fwd(int32_t h, int32_t th, int32_t Wq, int32_t Wk, int32_t ld, float scale, const float* table, const int32_t* idx,
                      float* out, void* stream);
int ea_table_bias_bwd(int32_t rows, int32_t K, int32_t h, int32_t Wq, int32_t Wk, int32_t ld, float scale, const float* g,
                      const int32_t* inv, float* dtable, void* stream);
/* Round 6 (ABI 12): the autocast casts of a layer's parameters in ONE launch -- dst[k][i] = (dtype) src[k][i], i < n[k], for
 * K <= 8 fp32 tensors (round to nearest even, exactly torch's `.to(dtype)`).  The 320 / 512 / 1024-wide layers run their two
 * projections (abstract_attention.py:72-78,86-87) as library GEMMs on 16-bit operands; their weights and biases were four
 * separate cast launches per step. */
int ea_multi_cast(int32_t dtype, int32_t K, const float* const* src, const int64_t* n, void* const* dst, void* stream);
int ea_slice_sum(int32_t BH, int32_t S, int32_t n, float scale, const float* a, const float* parts,
                 float* out, void* stream);
/* Measurement aid, not on the path: dst[0 .. bytes) = src[0 .. bytes) by a plain 16-byte-per-lane device copy kernel
 * (src, dst 16-byte aligned, bytes a multiple of 16).  bench.py times it as the achievable-HBM-bandwidth yardstick next
 * to the nominal 8 TB/s ("babel-stream-style copy kernel on the same GPU"). */
int ea_stream_copy(const void* src, void* dst, int64_t bytes, void* stream);

/* ---- LARA 1-D landmark proposals (LinearRA._proposal_gen_1d, lara.py:84-127) ----
 * Segment means over the sequence, q_bar_l = mean_{n in segment l} row_n, with the reference's
 * split of N tokens into L = g->L segments (N % L == 0: equal; otherwise (segs+1)L - N segments of
 * segs = N / L tokens followed by segments of segs + 1).  Geometry: ea_geom with B, H, N, D, dtype,
 * L (other fields ignored); N > L.  D in {32, 64} and a 16-bit dtype; another D > 0, EA_F32 and N <= L are
 * EA_E_UNSUPPORTED (well-formed, outside the kernels), a non-positive size or an unknown dtype EA_E_BADARG.
 *   'adaptive-1d' (gq != NULL): row_n = LayerNorm(x_n + bias), x = the rows q2 / k2 [B,H,N,D]
 *   (element type) holding Linear(q) WITHOUT its bias -- the host folds that Linear into the qkv
 *   projection --, bias = bias_q/k [H,D] for ordinary tokens and mbias_q/k [D] for tokens under
 *   `mask` (the reference zeroes q, k of padded tokens BEFORE the Linear, so their row is
 *   LayerNorm(Linear bias)); gq, cq / gk, ck = LayerNorm weight, bias [D].
 *   Plain means (gq == NULL): row_n = x_n (+ bias when given).
 * Forward: qbar, kbar fp32 [B*H, L, D].  Backward: d_qbar, d_kbar -> dq2, dk2 (gradient of the
 * rows x, WRITTEN) and per-segment partials part [B*H*L, 2 (q,k), 4, D] = (d LN weight, d LN bias,
 * d bias (sum over unmasked rows), d mbias (sum over masked rows)) which the caller sums. */
int ea_lara_segment_fwd(const ea_geom* g, const ea_t4* q2, const ea_t4* k2, const uint8_t* mask,
                        const float* bias_q, const float* bias_k, const float* mbias_q, const float* mbias_k,
                        const float* gq, const float* cq, const float* gk, const float* ck,
                        float* qbar, float* kbar, void* stream);
int ea_lara_segment_bwd(const ea_geom* g, const ea_t4* q2, const ea_t4* k2, const uint8_t* mask,
                        const float* bias_q, const float* bias_k, const float* mbias_q, const float* mbias_k,
                        const float* gq, const float* cq, const float* gk, const float* ck,
                        const float* d_qbar, const float* d_kbar, const ea_t4* dq2, const ea_t4* dk2,
                        float* part, void* stream);

/* ---- mu networks on the chunk means (eva.py:78-98,178-183; causal_eva.py:376-392,706-707) ------
 * y_s = [LayerNorm_s](x_s W_s^T + b_s) for sides = 1 (key side only: adaptive_proj 'none') or 2
 * (query side 0, key side 1), rows [R, D] fp32 with D in {32, 64, 128}, exact fp32 arithmetic.
 * layer_norm: 1 = Linear + LayerNorm (eps 1e-5), 0 = Linear only ('no-ln').
 *   fwd: zhat [sides,R,D] and rstd [sides,R] receive the normalised rows and 1/std for the backward
 *        (both NULL when no backward follows or layer_norm == 0).
 *   bwd: dx_s = d/dx; feed [R, planes, sides, D] with planes = 3 (dz, dy o zhat, dy) or 1 (dz = dy)
 *        whose column sums over R are (d bias, d gamma, d beta); dW_part
 *        [ea_rows_mlp_parts(R, D), sides, D, D] per-workgroup partials of d W. */
int32_t ea_rows_mlp_parts(int32_t R, int32_t D);
int ea_rows_mlp_fwd(int32_t R, int32_t D, int32_t sides, int32_t layer_norm,
                    const float* x0, const float* x1, const float* W0, const float* W1,
                    const float* b0, const float* b1, const float* g0, const float* g1,
                    const float* c0, const float* c1, float* y0, float* y1,
                    float* zhat, float* rstd, void* stream);
int ea_rows_mlp_bwd(int32_t R, int32_t D, int32_t sides, int32_t layer_norm,
                    const float* dy0, const float* dy1, const float* x0, const float* x1,
                    const float* W0, const float* W1, const float* g0, const float* g1,
                    const float* zhat, const float* rstd, float* dx0, float* dx1,
                    float* feed, float* dW_part, void* stream);

/* Weight and bias gradient of a projection in one pass over the activations (ea_wgrad.hip): the autograd
 * of `qkv = self.qkv(x)` / `x = self.proj(x)` (abstract_attention.py:72-78,86-87) with respect to the
 * Linear's parameters.  dy [rows, out_features], x [rows, in_features]: contiguous, EA_BF16 / EA_F16;
 * out_features and in_features multiples of 64 (EA_E_UNSUPPORTED otherwise).
 *   Slice s leaves its partial sums at dw_part + s * part_ld ([out_features, in_features] fp32) and, when db_part is not
 *   NULL, db_part + s * part_ld ([out_features] fp32); S = ea_wgrad_parts(rows, out_features, in_features), part_ld >=
 *   out_features * in_features and a multiple of 4.  With db_part = dw_part + out_features * in_features and part_ld =
 *   out_features * (in_features + 1) one ea_part_sum adds both up.
 * ea_part_sum: out[j] = sum_s parts[s * ld + j], j < n (n, ld multiples of 4), slices added in a fixed order
 *   (deterministic; no atomics). */
int32_t ea_wgrad_parts(int32_t rows, int32_t out_features, int32_t in_features);
int ea_wgrad(int32_t dtype, int32_t rows, int32_t out_features, int32_t in_features, const void* dy, const void* x,
             float* dw_part, float* db_part, int64_t part_ld, void* stream);
int ea_part_sum(int32_t S, int32_t n, int64_t ld, const float* parts, float* out, void* stream);
/* The weight (+ bias) gradients of TWO projections over the same token rows in one launch -- a layer's qkv and output
 * projections (abstract_attention.py:72-78,86-87 differentiated): dW1 = dY1^T X1, dW2 = dY2^T X2, rows shared.  With both
 * products' tiles in one grid a token slice is longer (S = ea_wgrad_pair_parts(...) slices for BOTH, fewer than either
 * product alone takes): half the partial-sum bytes and one launch less.  Arguments per product as for ea_wgrad; both need
 * the same tile edges (EA_E_UNSUPPORTED from ea_wgrad_pair_parts otherwise: use two ea_wgrad calls). */
int32_t ea_wgrad_pair_parts(int32_t rows, int32_t out1, int32_t in1, int32_t out2, int32_t in2);
int ea_wgrad_pair(int32_t dtype, int32_t rows, int32_t out1, int32_t in1, const void* dy1, const void* x1, float* dw_part1,
                  float* db_part1, int64_t part_ld1, int32_t out2, int32_t in2, const void* dy2, const void* x2,
                  float* dw_part2, float* db_part2, int64_t part_ld2, void* stream);
/* K <= 6 such reductions in one launch: out[k][j] = sum_s parts[k][s * ld[k] + j], j < n[k] (same order of additions as
 * ea_part_sum).  The terminal sums of a layer's backward -- both projections' slice partials and the per-(b,h) partials of
 * the landmark parameters (ea_lara_layer_bwd with dparams == NULL) -- share one launch this way. */
int ea_multi_sum(int32_t K, const float* const* parts, const int32_t* S, const int32_t* n, const int64_t* ld, float* const* out,
                 void* stream);

/* LARA sampling + proposal densities for sample counts beyond the fused landmark kernels (C > 64: antithetic /
 * multi-sample draws at 49 landmarks; lara.py:187-238).  qbar, mu = q_bar + k_bar: fp32 [BH,L,D]; noise: [BH,L,D] (mode 1,
 * antithetic: omega = [mu + eps; mu - eps]) or [BH,C,D] (mode 2, multi-sample: omega = [mu; mu] + eps), NULL for mode 0
 * (C = L).  With prm[c][n] = s <omega_c, mu_n> - s |mu_n|^2 / 2 over the L landmarks:
 *   EA_MIS_OPT   : lp_c = prm[c][c mod L], bhv_c = exp(lp_c - logsumexp_n prm[c][n]) L / C, qbar_rows = q_bar repeated;
 *   EA_MIS_BIASED: lp_c = logsumexp_n prm[c][n], qbar_rows = mu repeated;      EA_MIS_BH: lp_c likewise, no qbar_rows.
 * The backward takes the gradients of omega / qbar_rows / bhv / lp (NULL = zero, d_omega required) and returns d_qbar and
 * d_mu [BH,L,D].  fp32, one workgroup per (b,h); EA_E_UNSUPPORTED when the rows do not fit 150 KB of LDS. */
int ea_lara_sample_fwd(int32_t BH, int32_t L, int32_t C, int32_t D, int32_t mis, int32_t mode, float scale,
                       const float* qbar, const float* mu, const float* noise, float* omega, float* qbar_rows, float* bhv,
                       float* lp, void* stream);
int ea_lara_sample_bwd(int32_t BH, int32_t L, int32_t C, int32_t D, int32_t mis, int32_t mode, float scale,
                       const float* qbar, const float* mu, const float* noise, const float* d_omega, const float* d_qbar_rows,
                       const float* d_bhv, const float* d_lp, float* d_qbar, float* d_mu, void* stream);

/* nn.AdaptiveAvgPool2d of one of q / k / v over a gh x gw token grid that `side` does not divide (lara.py:43,48,145-151:
 * bin o of an axis of n cells = [floor(o n / side), ceil((o + 1) n / side)), neighbouring bins overlap).  x: [B,H,N,D]
 * view in the EA dtype; mean: fp32 [B,H,side*side,D].  The backward ACCUMULATES into dx (I/O dtype, fp32 math). */
int ea_adaptive_pool2d_fwd(int32_t dtype, int32_t B, int32_t H, int32_t gh, int32_t gw, int32_t side, int32_t D,
                           const ea_t4* x, float* mean, void* stream);
int ea_adaptive_pool2d_bwd(int32_t dtype, int32_t B, int32_t H, int32_t gh, int32_t gw, int32_t side, int32_t D,
                           const float* dmean, const ea_t4* dx, void* stream);

/* The projections themselves as streaming kernels (ea_linear.hip): `qkv = self.qkv(x)`, `x = self.proj(x)`
 * (abstract_attention.py:72-78,86-87) and, with the transposed weight, their input gradients.
 *   y[rows, out] = a[rows, in] w[out, in]^T (+ bias[out])
 * a: EA dtype, or fp32 when a_f32 != 0 (the autocast cast is folded into the load; a_cast, if not NULL, receives the
 * rounded [rows, in] copy for the weight-gradient product); w: [out, in] contiguous in the EA dtype; bias fp32 or
 * NULL (rounded to the EA dtype before the add, as F.linear under autocast does); y: EA dtype, or fp32 when
 * y_f32 != 0; lda / ldy: row strides in elements.  ea_linear_supported(in, out) != 0 for the built geometries
 * (in one of 64..768 in steps the models use, out a multiple of 64); EA_E_UNSUPPORTED otherwise. */
int32_t ea_linear_supported(int32_t in_features, int32_t out_features);
int ea_linear(int32_t dtype, int32_t rows, int32_t in_features, int32_t out_features, const void* a, int32_t a_f32,
              int64_t lda, const void* w, const float* bias, void* y, int32_t y_f32, int64_t ldy, void* a_cast,
              void* stream);
/* The same product straight from the fp32 MASTER weight (nn.Linear keeps fp32 parameters under autocast,
 * abstract_attention.py:34-36): the weight is rounded to the EA dtype while it is staged, so a training step needs no
 * per-step cast kernels.  w_transposed == 0: w is [out, in]; != 0: w is [in, out] and the product is a w (the input
 * gradient dX = dY W of a layer whose weight is W [out_layer, in_layer]: in = out_layer, out = in_layer), without a
 * transposed copy. */
int ea_linear_w32(int32_t dtype, int32_t rows, int32_t in_features, int32_t out_features, const void* a, int32_t a_f32,
                  int64_t lda, const float* w, int32_t w_transposed, const float* bias, void* y, int32_t y_f32, int64_t ldy,
                  void* a_cast, void* stream);
/* `qkv = self.qkv(x)` of a 192-wide, three-head model (abstract_attention.py:72-78) TOGETHER WITH the pooled q / k rows the
 * 2-D landmark generators start from (LinearRA: adaptive average pooling, lara.py:43,48,145-151; EVA: the chunk means of
 * eva.py:178-181 with 2-D chunks and no window extension): a [B*gh*gw, 192] tokens of B images, row-major gh x gw grids;
 * pooled_q / pooled_k: fp32 [B*3, (gh/r)*(gw/r), 64], the means of the ROUNDED q / k rows over the r x r cells -- exactly what
 * ea_eva_chunk_mean_fwd computes from the stored rows, without re-reading them (the kernel walks the tokens cell by cell and
 * sums the cell's rows while they are still in registers).  r = 2 or 4, in = 192, out = 576
 * (ea_linear_pool_supported != 0), EA_E_UNSUPPORTED otherwise; the other arguments as for ea_linear_w32.
 * w_cast (ABI 9): NULL, or [out_features, in_features] in the I/O type: the rounded weight, written by the same launch for
 * the backward's input-gradient GEMM (a cast launch of its own costs more than the 220 KB it moves). */
int32_t ea_linear_pool_supported(int32_t in_features, int32_t out_features, int32_t B, int32_t gh, int32_t gw, int32_t r);
int ea_linear_w32_pool(int32_t dtype, int32_t B, int32_t gh, int32_t gw, int32_t r, int32_t in_features, int32_t out_features,
                       const void* a, int32_t a_f32, int64_t lda, const float* w, const float* bias, void* y, int64_t ldy,
                       void* a_cast, float* pooled_q, float* pooled_k, void* w_cast, void* stream);

/* Round 6 (ABI 14): the 16-bit copies of a 192-wide layer's two weights in ONE launch, and the qkv projection fed by them.
 *   ea_linear_w192_prepare: wq fp32 [576, 192], wp fp32 [192, 192] (or NULL) -> w16q [576, 192] (what ea_linear_dgrad* take),
 *       wq_sw (576 * 192 elements: the same values in the order the register-resident projection kernel stages them),
 *       w16p [192, 192] and w16pT = its transpose (the output projection and its input gradient through ea_linear).
 *       Round to nearest even, as every cast of the library.
 *   ea_linear_wsw: y[rows, 576] = a[rows, 192] W^T + bias with W given as wq_sw; r = 0: plain rows; r = 2 | 4: tokens of
 *       B images of gh x gw, pooled q / k rows written as by ea_linear_w32_pool.
 * With the fp32 master weight every CU pulls 442 KB through its L2 port before its first tile -- 13 us at ANY row count
 * (workgroup timelines) -- and the two 192 x 192 projections another 2 x 147 KB per workgroup; the prepared
 * copies halve all of it for one ~4 us launch per step. */
int ea_linear_w192_prepare(int32_t dtype, const float* wq, const float* wp, void* w16q, void* wq_sw, void* w16p, void* w16pT,
                           void* stream);
int ea_linear_wsw(int32_t dtype, int32_t rows, int32_t B, int32_t gh, int32_t gw, int32_t r, const void* a, int32_t a_f32, int64_t lda,
                  const void* wq_sw, const float* bias, void* y, int64_t ldy, void* a_cast, float* pooled_q, float* pooled_k,
                  void* stream);
/* ABI 25: ea_linear_w192_prepare with a fifth image, wqT_sw (576 * 192 elements): wq's rounded values -- the bits of w16q --
 * in the order the input-gradient kernels hold W^T in their registers: 16-byte piece (wave, ks, lane = 16 g + li), wave < 12,
 * ks < 18, = wq[32 ks + 8 g .. + 7][16 wave + li].  ea_linear_dgrad / ea_linear_dgrad_finish take it with w_f32 == 2 and load it
 * straight into registers instead of transposing the weight through LDS at the start of every launch. */
int ea_linear_w192_prepare_t(int32_t dtype, const float* wq, const float* wp, void* w16q, void* wq_sw, void* w16p, void* w16pT,
                             void* wqT_sw, void* stream);

/* The INPUT gradient of that qkv projection (abstract_attention.py:72-78 differentiated; ABI 10, ea_dgrad_rs.hip):
 *   dx[rows, in] = dy[rows, out] w[out, in]          in = 192, out = 576 (ea_linear_dgrad_supported != 0)
 * dy: EA dtype, row stride ldy elements; w: the layer's weight [out, in] contiguous -- the fp32 master (w_f32 == 1, rounded
 * to the EA dtype on its way into the registers) or a copy in the EA dtype (w_f32 == 0, e.g. ea_linear_w32_pool's w_cast) --
 * or, ABI 25, ea_linear_w192_prepare_t's wqT_sw image (w_f32 == 2); any other w_f32 is EA_E_BADARG; dx: fp32
 * (dx_f32 != 0: the gradient of an fp32 module input under autocast) or the EA dtype, row stride ldx elements.  The weight
 * stays resident in the registers of a 12-wave workgroup per CU, dy passes LDS once: no library GEMM, no cast kernel. */
int32_t ea_linear_dgrad_supported(int32_t in_features, int32_t out_features);
int ea_linear_dgrad(int32_t dtype, int32_t rows, int32_t in_features, int32_t out_features, const void* dy, int64_t ldy,
                    const void* w, int32_t w_f32, void* dx, int32_t dx_f32, int64_t ldx, void* stream);

/* ... and the same product FUSED with the last corrections of dq / dk of a 192-wide, three-head layer (ABI 10): one pass over
 * the gradient rows instead of ea_lara_bwd_finish (or ea_eva_chunk_mean_bwd) followed by the product:
 *     dq_n -= s sum_c t[c,n] (u_c qbar_c)     (uq != NULL; lara.py:223 differentiated; qbar, uq [B*3, C, 64], lse_t [B*3, C], C <= 64;
 *                                              qkv: the forward's [B*gh*gw, 576] rows, q = columns 0 .. 191)
 *     dq_n += dpq[cell(n)] / r^2,  dk_n += dpk[cell(n)] / r^2   (dpq != NULL: fp32 [B*3, (gh/r)(gw/r), 64]; lara.py:43,48,145-151,
 *                                              eva.py:178-181 differentiated)
 *     dx = [dq | dk | dv] w
 * dqkv [B*gh*gw, 576] (EA dtype) is read AND its dq / dk columns rewritten with the corrected rows (the weight-gradient pass
 * reads them).  w, dx as for ea_linear_dgrad. */
int ea_linear_dgrad_finish(int32_t dtype, int32_t B, int32_t gh, int32_t gw, int32_t pool_r, int32_t C, float scale,
                           void* dqkv, int64_t ldy, const void* qkv, int64_t ldq, const void* w, int32_t w_f32, void* dx,
                           int32_t dx_f32, int64_t ldx, const float* qbar, const float* uq, const float* lse_t,
                           const float* dpq, const float* dpk, void* stream);

/* Round 5 (ABI 10): consumer passes that merge the producing pass's per-slice partials in their prologue -- the arithmetic of
 * ea_lara_merge_fwd / _bwd and ea_slice_sum, operation for operation -- so a layer step has three launches less (7 + 14 + 6
 * us at cfg3 for a few KB per (b,h)).  S <= 4 slices, C <= 64 samples (EA_E_UNSUPPORTED otherwise: keep the merge launches).
 *   ea_lara_out_fwd_merge: ea_lara_out_fwd fed by ea_lara_stats_fwd's partials (p_ml [BH,S,C,4], p_kv [BH,S,C,D]) and lp;
 *       block 0 of every (b,h) writes the merged kv, lse_k, lse_t, cst for the backward (lara.py:205-211,241-246).
 *   ea_lara_bwd_k_fused_merge: ea_lara_bwd_k_fused fed by ea_lara_bwd_q_fused's partials (p_ml, p_dkv, p_dom, p_m1, p_m2);
 *       forms d kv_stats, dkk, r itself; block 0 writes dbh, dlp (= -r), domq (sum dZ q), dqbar, uq (NULL-able as in
 *       ea_lara_merge_bwd); p_domk [BH,S,C,D]: its own d omega partials (must not alias the inputs).
 *   ea_lara_landmarks_bwd_parts: ea_lara_landmarks_bwd with d omega = dom_scale (d_omega + sum_s dom_parts[bh][s]) formed on
 *       load (ea_slice_sum's order of additions). */
int ea_lara_out_fwd_merge(const ea_lara_geom* g, const ea_t4* q, const float* omega, const float* qbar, const float* bhv,
                          int32_t S, const float* p_ml, const float* p_kv, const float* lp, float* kv, float* lse_k,
                          float* lse_t, float* cst, const ea_t4* out, float* lseZ, float* tmean, void* stream);
int ea_lara_bwd_k_fused_merge(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* omega,
                              const float* qbar, const float* kv, const float* lse_k, int32_t S, const float* p_ml,
                              const float* p_dkv, const float* p_dom, const float* p_m1, const float* p_m2,
                              const ea_t4* dk, const ea_t4* dv, float* p_domk, float* dbh, float* dlp, float* domq,
                              float* dqbar, float* uq, void* stream);
int ea_lara_landmarks_bwd_parts(const ea_lmk_geom* g, const float* pq, const float* pk,
                                const float* Wq, const float* bq, const float* gq, const float* cq,
                                const float* Wk, const float* bk, const float* gk, const float* ck,
                                const float* noise, const float* d_omega, int32_t dom_S, const float* dom_parts, float dom_scale,
                                const float* d_qbar_rows, const float* d_bhv, const float* d_lp, float* dpq, float* dpk,
                                float* dW_part, float* dvec_part, const float* saved, void* stream);

/* ---- fp32-FAITHFUL cores (round 5, ABI 10; ea_f32_attn.hip) -------------------------------------------------------------
 * Outside torch.autocast the reference computes attention in fp32 (abstract_attention.py:120-133, local_attention.py:134-182,
 * eva.py:138-233, causal_eva.py:666-783).  One gathered-attention pair in exact fp32 arithmetic (operands, products on
 * v_mfma_f32_16x16x4_f32, softmax) covers every softmax-shaped core, stated as the reference states them:
 *   group g (a window, a landmark chunk, or the whole sequence), query slot i -> token idx_q[g][i] of q [B,H,Nq,D],
 *   Wk local key slots j -> token idx_k[g][j] of k, v [B,H,Nk,D] (-1: absent = zero row, masked), then L extra keys / values
 *   ek, ev [B,H,L,D] shared by all groups (EVA: rf_k_bar / beta):
 *     logit_ij = scale q_i.k_j [- scale |k_j|^2 / 2 (knorm)] [+ bias[b bias_bs + h bias_hs + i bias_ld + j]]
 *     masked (padded / absent key; padded query (qmask); causal_e >= 0 and j > i + causal_e): -5e4, or -inf for padded keys when
 *     neg_inf; extra key c masked (-5e4) when chunk > 0 and c >= lm_base + token(i) / chunk  (causal_eva.py:716-738)
 *     out_i = softmax over the Wk + L columns . [v ; ev] (dropout: keep [B,H,Nq,keep_ld] over those columns, kept entries x
 *     keep_scale in the value product only), lse_i = log-sum-exp (natural log, optional); stat [B,H,Nq,2] = (row max, sum of
 *     e^(logit - max)) is what the backward recomputes the probabilities from (lse alone loses the sum's digits when the
 *     maximum is the -5e4 fill of a fully masked row).
 * All tensors fp32 (ea_t4 strides in elements).  Backward: dq stored; dk, dv [B,H,Nk,D], dek, dev [B,H,L,D], dbias (bias layout)
 * are contiguous fp32 buffers ACCUMULATED into with atomics (the caller zeroes them; windows overlap); dlse optional. */
typedef struct {
  int32_t B, H, Nq, Nk, D;           /* D in {32, 64, 128} */
  int32_t G, Wq, Wk, L;
  int32_t knorm;                     /* bit 0: the key-norm term; bit 1: masked local keys carry a zero VALUE row (eva.py:167-176) */
  int32_t neg_inf, causal_e, chunk, lm_base;   /* lm_base: 0 from every caller of this package since ABI 17 (see ea_geom.lm_base) */
  int32_t bias_ld;
  int64_t bias_hs, bias_bs, keep_ld;  /* bias index = b bias_bs + h bias_hs + i bias_ld + j (0 strides: shared) */
  float   keep_scale, scale;
} ea_f32_attn;
int ea_f32_attn_fwd(const ea_f32_attn* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const ea_t4* ek, const ea_t4* ev,
                    const int32_t* idx_q, const int32_t* idx_k, const float* bias, const uint8_t* kmask, const uint8_t* qmask,
                    const uint8_t* keep, const ea_t4* out, float* lse, float* stat, void* stream);
int ea_f32_attn_bwd(const ea_f32_attn* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const ea_t4* ek, const ea_t4* ev,
                    const int32_t* idx_q, const int32_t* idx_k, const float* bias, const uint8_t* kmask, const uint8_t* qmask,
                    const uint8_t* keep, const ea_t4* out, const ea_t4* dout, const float* stat, const float* dlse,
                    const ea_t4* dq, float* dk, float* dv, float* dek, float* dev, float* dbias, void* stream);
/* mean[b,h,c,:] = (1/J) sum_j x[b,h,idx[c][j],:] over the present, unpadded tokens (EVA's masked chunk means, eva.py:167-181;
 * uniform pooling); backward accumulates into dx [B,H,N,D] contiguous fp32 (atomics). */
int ea_f32_gather_mean_fwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t Cn, int32_t J, const ea_t4* x, const int32_t* idx,
                           const uint8_t* mask, float* mean, void* stream);
int ea_f32_gather_mean_bwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t Cn, int32_t J, const int32_t* idx,
                           const uint8_t* mask, const float* dmean, float* dx, void* stream);

/* ---- composite per-module entry points: the whole LARA core in one call each way (round 3) --------------------
 * lara.py:129-175,187-246 for the 2-D pooled proposals ('pool', 'pool-mixed'): uniform r x r pooling of q, k -> landmark
 * pipeline -> estimator, i.e. the launch sequences of ea_eva_chunk_mean_fwd / ea_lara_landmarks_* / ea_lara_stats_fwd /
 * ea_lara_merge_* / ea_lara_out_fwd / ea_lara_bwd_*_fused / ea_slice_sum / ea_lara_bwd_finish / ea_colsum2_f32 issued from
 * C++ on caller-owned workspaces, so that an eagerly stepping caller (vit/engine.py:47-64) pays two FFI calls per layer
 * step instead of ~15 (and two allocations instead of ~30).  C = L (x 2 with antithetic / multi-sample noise) <= 64.
 *   ea_lara_layer_plan(cfg, out) (ABI 31): the workspace layout, a pure host function of cfg -> EA_OK with *out filled, or
 *       EA_E_* (a NULL `out`: EA_E_BADARG).
 *   keep_for_backward: bit 0 = keep the intermediates the backward needs; bit 1 (EA_LARA_POOLED_READY) = the pooled q / k
 *       rows are already in `saved` at saved_pq / saved_pk (written by ea_linear_w32_pool): the pooling pass is skipped.
 *   params: NULL or 8 pointers (Wq, bq, gamma_q, beta_q, Wk, bk, gamma_k, beta_k: q_bar_gen / k_bar_gen, lara.py:45-54);
 *   noise: [B*H, C, D] standard normal or NULL (eval); dparams: [2*D*D + 6*D] fp32 = dW_q, dW_k, then (db, dgamma, dbeta)
 *   of q and of k, summed over the batch and heads, or NULL: the partials at bwd_dW / bwd_dvec are the caller's (ea_multi_sum).
 *   flags: EA_LARA_DEFER_FINISH leaves out the finish pass -- dq lacks the softmax-over-sequence correction and dq, dk the
 *       pooling terms; ea_linear_dgrad_finish applies them (saved_qrows, saved_lse_t, bwd_uq, bwd_dpq, bwd_dpk) on its way. */
typedef struct {
  int32_t B, H, D;
  int32_t dtype;             /* EA_BF16 | EA_F16 */
  int32_t gh, gw;            /* token grid (N = gh * gw) */
  int32_t pool_r;            /* pooling side: landmarks L = (gh / r) * (gw / r) */
  int32_t has_mlp, mixed, mis, dup;   /* as in ea_lmk_geom */
  float   kappa, scale;      /* alpha_coeff (lara.py:231), D^-0.5 */
} ea_lara_layer;
typedef struct {             /* sizes in floats; saved_* / bwd_*: offsets in floats into `saved` / the backward scratch */
  int64_t n_saved, n_fwd_tmp, n_bwd_tmp;                 /* `saved` (forward -> backward), forward scratch, backward scratch */
  int64_t saved_pq, saved_pk, saved_qrows, saved_lse_t;  /* pooled q / k rows [B*H, L, D]; qbar rows [B*H, C, D]; lse_t [B*H, C] */
  int64_t bwd_dW, bwd_dvec, bwd_uq, bwd_dpq, bwd_dpk;    /* per-(b,h) partials [B*H, 2 D D] (dW_q, dW_k), [B*H, 6 D]; u qbar rows; d(pooled q / k) */
} ea_lara_layer_sizes;
#define EA_LARA_POOLED_READY 2
#define EA_LARA_DEFER_FINISH 1
int ea_lara_layer_plan(const ea_lara_layer* cfg, ea_lara_layer_sizes* out);
int ea_lara_layer_fwd(const ea_lara_layer* cfg, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                      const float* noise, const float* const* params, const ea_t4* out, float* saved, float* tmp,
                      int32_t keep_for_backward, void* stream);
int ea_lara_layer_bwd(const ea_lara_layer* cfg, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                      const float* noise, const float* const* params, const ea_t4* dout, const ea_t4* dq, const ea_t4* dk,
                      const ea_t4* dv, const float* saved, float* tmp, float* dparams, int32_t flags, void* stream);

/* ---- composite per-module entry points, EVA (round 4) -----------------------------------------------------------
 * The 2-D EVA core (eva.py:145-227: non-overlapping w x w windows, r x r landmark chunks, adaptive_proj 'default', no pad
 * mask) in one call each way -- the launch sequences of ea_eva_chunk_mean_fwd / ea_lara_landmarks_* (eva mode) /
 * ea_eva_beta_* / ea_window_attn_* / ea_slice_sum / ea_colsum_f32 / ea_eva_chunk_mean_bwd / ea_colsum2_f32 on caller-owned
 * workspaces, for the same reason as the LARA pair above (eagerly stepping call sites, vit/engine.py:47-64).
 *   ea_eva_layer_plan(cfg, out) (ABI 31): as ea_lara_layer_plan; EA_E_UNSUPPORTED: L > 64 or a window geometry whose backward
 *       needs scratch slices -- use the step-by-step entry points.
 *   bias: fp32 [H, w*w, ld] dense per-head bias multiplied by log2(e), rows padded to ld (as for ea_window_attn_fwd), or
 *       NULL (then cfg->has_bias == 0); dbias: fp32 [H, w*w, ld], gradient with respect to the NATURAL-unit bias, or NULL:
 *       its partial sums then stay at bwd_dbias_part for the caller's own reduction (ea_multi_sum, with the other sums).
 *   params: 8 pointers (W, b, gamma, beta of the q and of the k mu network: eva.py:93-103); noise: [B*H, L, D] or NULL.
 *   keep_for_backward: as for ea_lara_layer_fwd (bit 1: ea_linear_w32_pool wrote the chunk means to saved_qmean / saved_kmean).
 *   dparams: [2 D D + 6 D] fp32 as for ea_lara_layer_bwd, or NULL (partials left at bwd_dW / bwd_dvec).  dq, dk, dv are WRITTEN.
 *   flags: EA_EVA_DEFER_CHUNK_MEAN leaves out the chunk-mean backward (eva.py:178-181 differentiated): dq / dk lack the
 *       d(chunk mean) / r^2 terms, which ea_linear_dgrad_finish adds (from bwd_dqmean / bwd_dkmean) on its way. */
typedef struct {
  int32_t B, H, D;
  int32_t dtype;             /* EA_BF16 | EA_F16 */
  int32_t gh, gw;            /* token grid (N = gh * gw) */
  int32_t window;            /* window side w (gh, gw multiples of it; no overlap extension) */
  int32_t chunk;             /* landmark chunk side r: L = (gh / r) * (gw / r) <= 64 */
  int32_t has_bias;
  float   scale;             /* D^-0.5 */
} ea_eva_layer;
typedef struct {             /* as ea_lara_layer_sizes (there is no forward scratch); bias_ld and dbias_part_rows are counts */
  int64_t n_saved, n_bwd_tmp;
  int64_t saved_qmean, saved_kmean, saved_lse, bias_ld;  /* chunk means of q / k [B*H, L, D]; joint log-sum-exp [B,H,N]; = ea_window_bias_ld */
  int64_t bwd_dW, bwd_dvec, bwd_dbias_part, dbias_part_rows;   /* partials: [B*H, 2 D D], [B*H, 6 D]; of dbias, so many rows of H * w*w * ld */
  int64_t bwd_dqmean, bwd_dkmean;                        /* chunk-mean gradients [B*H, L, D] */
} ea_eva_layer_sizes;
#define EA_EVA_DEFER_CHUNK_MEAN 1
int ea_eva_layer_plan(const ea_eva_layer* cfg, ea_eva_layer_sizes* out);
int ea_eva_layer_fwd(const ea_eva_layer* cfg, const ea_t4* q, const ea_t4* k, const ea_t4* v, const float* bias,
                     const float* noise, const float* const* params, const ea_t4* out, float* saved,
                     int32_t keep_for_backward, void* stream);
int ea_eva_layer_bwd(const ea_eva_layer* cfg, const ea_t4* q, const ea_t4* k, const ea_t4* v, const float* bias,
                     const float* noise, const float* const* params, const ea_t4* out, const ea_t4* dout, const ea_t4* dq,
                     const ea_t4* dk, const ea_t4* dv, const float* saved, float* tmp, float* dbias, float* dparams,
                     int32_t flags, void* stream);

/* ---- row LayerNorm (ea_layernorm.hip) -------------------------------------------------------------------------
 * The LayerNorm of LinearRA's model-wide ('dense') landmark generators (lara.py:34-44,64-71: Linear(dim, dim) + LayerNorm(dim)
 * on the B * L pooled rows).  x [rows, C] contiguous, xtype EA_BF16 / EA_F16 / EA_F32 (under autocast torch evaluates
 * layer_norm in fp32 on the 16-bit Linear output); C a multiple of 64, <= 1024 (EA_E_UNSUPPORTED otherwise).
 *   fwd: y fp32 [rows, C] = (x - mean) rstd gamma + beta, biased variance, two-pass statistics in fp32; stats [rows, 2] =
 *        (mean, rstd) for the backward (may be NULL).
 *   bwd: dx [rows, C] in x's type; part [ea_layernorm_parts(rows), 2, C] fp32 = per-workgroup partial sums of d gamma and
 *        d beta (add them with ea_colsum_f32(parts, 2 * C, ...)). */
int32_t ea_layernorm_parts(int32_t rows);
int ea_layernorm_fwd(int32_t xtype, int32_t rows, int32_t C, const void* x, const float* gamma, const float* beta, float eps,
                     float* y, float* stats, void* stream);
int ea_layernorm_bwd(int32_t xtype, int32_t rows, int32_t C, const void* x, const float* gamma, const float* stats,
                     const float* dy, void* dx, float* part, void* stream);

/* ---- ScatterBrain, low-rank half (scatterbrain_attention.py:99-160; ea_scatter.hip) --------------------
 * The window half is ea_window_attn_fwd/bwd (it returns / takes the gradient of its per-query log-sum-exp);
 * these entry points evaluate the m random-feature columns of the same softmax and merge the two halves:
 *   ea_scatter_kmax / ea_scatter_kv : mx[c] = max_j log phi(k_j)[c] and the partial sums of
 *       z_all[c] = sum_j exp(lk_jc - mx_c), S_all[c] = sum_j exp(lk_jc - mx_c) v_j  over sequence slices
 *       (p_ml [BH,S,M,4] (first field), p_kv [BH,S,M,64], S = ea_scatter_parts(g)); padded keys excluded;
 *   ea_scatter_fwd : per window, statistics of the window's own keys, KV = (S_all - S_win) / clamp(z_all -
 *       z_win, 1e-3), joint weights of the feature columns, and out = sigma(lse_loc - r) o_loc + sigma(r -
 *       lse_loc) O with r [B,H,N] = log-sum-exp of the feature logits (returned for the backward).
 * D = 64, M <= 64 features, windows of <= 64 tokens, no window overlap.  W [H, M, 64] fp32. */
typedef struct {
  int32_t B, H, N, D;
  int32_t dtype;
  int32_t M;                 /* random features */
  int32_t attn_2d, gh, gw;   /* token grid (2-D) */
  int32_t window;            /* window side */
} ea_sb_geom;
int32_t ea_scatter_parts(const ea_sb_geom* g);
int ea_scatter_kmax(const ea_sb_geom* g, const ea_t4* k, const uint8_t* mask, const float* W, float* p_ml, void* stream);
int ea_scatter_kv(const ea_sb_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                  const float* mx, float* p_ml, float* p_kv, void* stream);
int ea_scatter_fwd(const ea_sb_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                   const float* W, const float* mx, const float* zall, const float* sall, const ea_t4* oloc,
                   const float* lse_loc, const ea_t4* out, float* r, void* stream);
/* Backward of ea_scatter_fwd (mx is a detached stabiliser, as in the reference):
 *   ea_scatter_bwd_window: per window -- dq, the window's own contributions to dk / dv (written, not
 *       accumulated), d o_loc = alpha dout and d lse_loc [B,H,N] (the cotangents of the window half, to be fed to
 *       ea_window_attn_bwd), and partial sums p_dsall [BH, P, M, 64], p_dzall [BH, P, M] of d S_all, d z_all,
 *       P = ea_scatter_bwd_parts(g);
 *   ea_scatter_bwd_global: given the summed d S_all, d z_all, ADDS every key's share to dk, dv. */
int32_t ea_scatter_bwd_parts(const ea_sb_geom* g);
int ea_scatter_bwd_window(const ea_sb_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                          const float* W, const float* mx, const float* zall, const float* sall, const ea_t4* oloc,
                          const float* lse_loc, const float* r, const ea_t4* dout, const ea_t4* dq, const ea_t4* dk,
                          const ea_t4* dv, const ea_t4* doloc, float* dlse, float* p_dsall, float* p_dzall,
                          void* stream);
int ea_scatter_bwd_global(const ea_sb_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                          const float* mx, const float* dsall, const float* dzall, const ea_t4* dk, const ea_t4* dv,
                          void* stream);

/* Overlapping windows (the module's overlap_window=True: ext = window / 2).  The key side of window g is the patch of
 * (window + 2 ext) tokens per axis around it; a slot of the patch outside the sequence is the reference's zero padding:
 * a key with log phi = 0 (phi = 1) for every feature and v = 0, which enters z_win and the stabiliser only.  So
 *   - mx handed to ea_scatter_kv and to everything below is max(max_j log phi-arguments, log(M) / 2), i.e. the output of
 *     ea_scatter_kmax raised to at least log(M) / 2 by the caller (log phi = 0 in the kernels' scaling, which keeps
 *     the -log(M)/2 of log phi apart); z_all, S_all stay sums over the real keys;
 *   - the non-local log-mass is the reference's max-shifted log_add_exp(lse_all, lse_win, mask (1,-1)): it is NaN, and
 *     with it every output row of the window, where a border window's padding outweighs the keys outside its patch
 *     (reference behaviour, not sanitised);
 *   - a key lies in the patches of up to 2 (1-D) / 4 (2-D) windows: ea_scatter_ov_bwd_window writes dq, d o_loc,
 *     d lse_loc and leaves, per window, w_ds [BH, G, M, 64] (the window's share of d S_all; d S_win[g] is its
 *     negative), w_dzall [BH, G, M] (its share of d z_all) and w_dzwin [BH, G, M] (d z_win[g]), G =
 *     ea_scatter_ov_windows(g, ext); the caller sums w_ds, w_dzall over G into dsall, dzall; ea_scatter_ov_bwd_keys
 *     then WRITES every dk, dv row once from dsall, dzall and the windows whose patch holds the key (no atomics:
 *     bit-reproducible).  Padding slots receive no gradient; mx is detached.
 * 0 <= ext <= window (-1 below, -2 above), otherwise the limits of ea_sb_geom; ext = 0 computes the non-overlapping
 * form through these kernels (the module uses ea_scatter_fwd / _bwd_* there). */
int32_t ea_scatter_ov_windows(const ea_sb_geom* g, int32_t ext);
int ea_scatter_ov_fwd(const ea_sb_geom* g, int32_t ext, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                      const uint8_t* mask, const float* W, const float* mx, const float* zall, const float* sall,
                      const ea_t4* oloc, const float* lse_loc, const ea_t4* out, float* r, void* stream);
int ea_scatter_ov_bwd_window(const ea_sb_geom* g, int32_t ext, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                             const uint8_t* mask, const float* W, const float* mx, const float* zall,
                             const float* sall, const ea_t4* oloc, const float* lse_loc, const float* r,
                             const ea_t4* dout, const ea_t4* dq, const ea_t4* doloc, float* dlse, float* w_ds,
                             float* w_dzall, float* w_dzwin, void* stream);
int ea_scatter_ov_bwd_keys(const ea_sb_geom* g, int32_t ext, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                           const float* W, const float* mx, const float* dsall, const float* dzall, const float* w_ds,
                           const float* w_dzwin, const ea_t4* dk, const ea_t4* dv, void* stream);

/* ---- causal EVA, incremental decoding (ABI 17; causal_eva.py:537-665; ea_ceva_decode.hip) --------------------------
 * One decoding step of CausalEVAttention with fairseq's incremental state, defined by prefix consistency with the
 * full-sequence causal path (the output for token t equals row t of the forward on tokens 0..t).  q, k, v address the
 * projected rows of the state's cache as [B, H, cap, D] (token n = row n); pad is uint8 [B, cap], 1 = padded position, or
 * NULL (has_mask = 0); rf_k_bar and beta are the state's fp32 [B, H, Lcap, D] landmark rows, indexed by absolute chunk.
 * Everything is computed in fp32; rows are read and out is written in `dtype` (EA_BF16 | EA_F16 | EA_F32: with fp32 rows
 * nothing is rounded to 16 bits).  D = 32, 64 or 128; w, e, r and the number of chunks are not limited.
 *   ea_ceva_decode_close: for every chunk c in [c_first, c_last] (rows c r .. c r + r - 1, all decoded), one workgroup per
 *     (c, b, h): qm, km = sum of the unpadded q / k rows / r (eva.py:167-181); rk = mu_k(km), mu = mu_q(qm) + rk with mu_* =
 *     Linear(D, D) followed (adaptive = 1, 'qk') by LayerNorm(D, eps 1e-5), or not (adaptive = 0, 'no-ln'); mu_params: a
 *     HOST array of device pointers, the module's fp32 parameters in _mu_params() order (q Linear W, b[, LN w, b], then k);
 *     beta_c = sum_j softmax_j(s mu.k_j - s|k_j|^2/2) v_j, padded rows -5e4 with a zero value row.  Writes rf_k_bar[c] = rk
 *     and beta[c].  Eval mode: no sampling noise.
 *   ea_ceva_decode_attn: the outputs of tokens t0 .. t0 + T_new - 1 (already in the cache), one workgroup per (window block
 *     touched, b, h).  Token t of block bk = t / w: local slot j < w + e is token bk w - e + j, masked with -5e4 when it is
 *     absent (< 0), padded, after t, or t itself is padded; its logit is s q.k_j + bias[t - bk w, j] (bias: fp32 [w, w + e]
 *     dense single-head table, natural-log domain, or NULL when has_bias = 0); landmark c is a column iff c < t / r (every
 *     chunk before t's own is closed).  One softmax over both, out = P [v ; beta]; out [B, H, T_new, D] row t - t0.
 * t0 is a kernel argument; nothing is read back to the host.  Replaces the per-token window launches of causal_eva.py:542-665. */
typedef struct {
  int32_t B, H, D;
  int32_t dtype;             /* EA_BF16 | EA_F16 | EA_F32: the cache rows and out */
  int32_t window, ext, chunk;  /* w, e (left extension, 0 or w), r */
  int32_t t0, T_new;         /* the step's tokens */
  int32_t c_first, c_last;   /* close: chunks to build, inclusive */
  int32_t cap;               /* cache capacity in tokens (row stride of pad) */
  int32_t adaptive;          /* 1: 'qk' (Linear + LayerNorm), 0: 'no-ln' (Linear) */
  int32_t has_bias, has_mask;
} ea_ceva_dec_geom;
int ea_ceva_decode_close(const ea_ceva_dec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                         const float* const* mu_params, const ea_t4* rf_k_bar, const ea_t4* beta, void* stream);
int ea_ceva_decode_attn(const ea_ceva_dec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                        const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, void* stream);

/* ---- causal EVA, static incremental decoding (ABI 18; CausalEVAttention.init_static_decoding; ABI 19: ring) --------------
 * The same step with the token count in DEVICE memory, so that a step can be captured into a graph and replayed: no
 * argument of these calls changes from one step to the next.  pos: int32, tokens decoded so far; status: int32, set to 1
 * by a step that would pass cap (sticky; never cleared by these calls).  cap is a multiple of window, window of chunk.
 * pad is always given (zeros where nothing is padded).  One step = these four launches, in this order, on one stream:
 *   ea_ceva_sdecode_append: rows *pos .. *pos + T_new - 1 of the cache qkv [B, cap, 3, H, D] (contiguous, `dtype`) = the
 *     step's time-first rows qkv_new [T_new, B, 3, H, D] (contiguous, `dtype`); pad [B, cap] at the same columns = new_pad
 *     [B, T_new] uint8, or 0 when new_pad is NULL.
 *   ea_ceva_sdecode_close: ea_ceva_decode_close for the chunks those tokens complete.
 *   ea_ceva_sdecode_attn: ea_ceva_decode_attn for those tokens, t0 = *pos.
 *   ea_ceva_sdecode_advance: *pos += T_new.
 * A step with *pos + T_new > cap writes no byte of the cache, the pad or the landmark rows: append sets *status = 1, attn
 * writes NaN into out, advance leaves *pos.
 * ABI 19, ring != 0 (CausalEVAttention.init_rolling_decoding): the token rows live in a ring.  qkv is [B, ring, 3, H, D], q, k, v
 * address it as [B, H, ring, D], pad is [B, ring], and token n is at row n % ring; rf_k_bar and beta stay linear
 * [B, H, cap / chunk, D], and cap bounds only them and *pos.  ring is a multiple of window with ring >= window + ext + T_new
 * (else EA_E_BADARG): a step at *pos reads back to token floor(*pos / window) window - ext and appends up to *pos + T_new - 1,
 * at most window - 1 + ext + T_new < ring tokens, so the rows it appends replace only tokens older than any it reads.  The
 * arithmetic is that of ring = 0: for one sequence of step sizes the outputs and landmark rows are equal bit for bit.
 * ABI 20, ntok != NULL (init_*_decoding(per_sequence=True)): every batch element has its own count.  pos, status and ntok
 * are int32 [B].  Of the step's T_new positions, element b's tokens are those before its first flagged one in new_pad
 * [B, T_new] (all T_new without a flag or with new_pad NULL): n_b of them, 0 <= n_b <= T_new.  append finds n_b, writes
 * ntok[b] = n_b (its only writer) and stores the n_b rows at pos[b] .. pos[b] + n_b - 1 with pad 0; nothing is stored for the
 * other positions.  close, attn and advance, behind it on the stream, take t0 = pos[b] and n_b where they take *pos and T_new
 * above; attn writes zero rows n_b .. T_new - 1 of element b; advance adds n_b to pos[b].  The launches and their grids are
 * those of T_new tokens.  An element with pos[b] + n_b > cap writes no byte of its state: status[b] = 1, its T_new output rows
 * are NaN, pos[b] stays; the other elements of the step are not affected.  For n_b = T_new everywhere the outputs and the
 * state equal those of ntok = NULL bit for bit.  ntok = NULL is exactly the contract of ABI 19.
 * ABI 21, a step of T_new <= 8 tokens with its landmark range split over workgroups (init_*_decoding(landmark_splits=P)):
 * ea_ceva_sdecode_attn streams every landmark row of a (b, h) through one workgroup; the two calls below replace it, in its
 * place between close and advance, and take the geometry unchanged.
 *   ea_ceva_sdecode_attn_split: `parts` workgroups per (window block, b, h) share the 64-column tiles of [local keys, then
 *     landmarks] -- wave s of part p takes tiles 4 p + s, + 4 parts, .. -- with the arithmetic of ea_ceva_sdecode_attn, and
 *     write, for every live query, the unnormalised partial (acc[D], max, sum) to ws: fp32 [B, H, 8, parts, D + 4], 16-byte
 *     aligned, row (b, h, t - *pos, part); a part without a tile writes max = -inf, sum = 0.  Writes `out` only where the step
 *     refuses: NaN rows (no partial) when it does not fit, zero rows n_b .. T_new - 1 of a per-sequence element.
 *   ea_ceva_sdecode_merge: out row t = sum_p f_p acc_p / sum_p f_p l_p, f_p = exp(m_p - max_p m_p) (0 for m_p = -inf), for the
 *     live queries; it leaves the NaN and zero rows alone.  Stream order puts it behind attn_split and before advance.
 * ws is scratch: every row that merge reads has been written by the attn_split before it.  EA_E_BADARG: parts outside
 * [2, 64], ws NULL or not 16-byte aligned, T_new > 8, pos NULL; every other refusal is that of ea_ceva_sdecode_attn. */
typedef struct {
  int32_t B, H, D;
  int32_t dtype;             /* EA_BF16 | EA_F16 | EA_F32: the cache rows and out */
  int32_t window, ext, chunk;  /* w, e (left extension, 0 or w), r */
  int32_t T_new;             /* tokens per step: fixed for a captured step */
  int32_t cap;               /* cache capacity in tokens (ring != 0: of the landmark rows, cap / chunk of them) */
  int32_t adaptive;          /* 1: 'qk' (Linear + LayerNorm), 0: 'no-ln' (Linear) */
  int32_t has_bias;
  int32_t ring;              /* 0: qkv and pad hold cap rows; else they hold ring rows, token n at row n % ring */
  const int32_t* pos;        /* device */
  int32_t* status;           /* device */
  int32_t* ntok;             /* device [B], or NULL: one shared count (ABI 20) */
} ea_ceva_sdec_geom;
int ea_ceva_sdecode_append(const ea_ceva_sdec_geom* g, const void* qkv_new, const uint8_t* new_pad, void* qkv, uint8_t* pad,
                           void* stream);
int ea_ceva_sdecode_close(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                          const float* const* mu_params, const ea_t4* rf_k_bar, const ea_t4* beta, void* stream);
int ea_ceva_sdecode_attn(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                         const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, void* stream);
int ea_ceva_sdecode_attn_split(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                               const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, int32_t parts,
                               float* ws, void* stream);
int ea_ceva_sdecode_merge(const ea_ceva_sdec_geom* g, const ea_t4* out, int32_t parts, const float* ws, void* stream);
int ea_ceva_sdecode_advance(const ea_ceva_sdec_geom* g, void* stream);

/* ABI 23, a static state with 16-bit landmark rows (init_*_decoding(compact_landmarks=True)): rf_k_bar and beta are rows of
 * the geometry's dtype, EA_BF16 or EA_F16, their ea_t4 strides in those elements.  The three calls below take the place of
 * their twins in a step (append, merge and advance touch no landmark row) and take the geometry unchanged.
 *   ea_ceva_sdecode_close_l16: the arithmetic of ea_ceva_sdecode_close in its order, in fp32; mu and beta are formed from the
 *     unrounded rf_k_bar, and only the stores of the two rows round, once, to nearest even: the rows written equal the
 *     twin's rows rounded, bit for bit.
 *   ea_ceva_sdecode_attn_l16, ea_ceva_sdecode_attn_split_l16: the twins' arithmetic on the rows widened to fp32 (exact).
 * Every refusal is the twin's, decided in the same order, and besides EA_E_BADARG for: dtype EA_F32 (decided with the other
 * faults of the dtype, before the head dim); a landmark pointer not 16-byte aligned; a landmark stride that is no multiple
 * of 8 elements (rows of D 16-bit elements, D >= 32, stay 16-byte aligned). */
int ea_ceva_sdecode_close_l16(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                              const float* const* mu_params, const ea_t4* rf_k_bar, const ea_t4* beta, void* stream);
int ea_ceva_sdecode_attn_l16(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                             const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, void* stream);
int ea_ceva_sdecode_attn_split_l16(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                                   const uint8_t* pad, const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta,
                                   const ea_t4* out, int32_t parts, float* ws, void* stream);

/* ABI 22, the projections of a step on weights the static state holds (init_*_decoding(hold_projections=True);
 * ea_ceva_decode_linear.hip):
 *   y[m, n] = round_y( sum_k round_w(x[m, k]) w[n, k] + bias[n] ),  1 <= M <= EA_CEVA_LINEAR_MAX_ROWS
 * x [M, ldx] rows of x_dtype = EA_F32 or w_dtype (fp32 rows are rounded to w_dtype, to nearest even, as they are loaded);
 * w [N, K] row-major and bias [N] (or NULL) of w_dtype = EA_BF16 | EA_F16; products, sums and the bias add in fp32; y [M, ldy]
 * rows of y_dtype = w_dtype or EA_F32.  ldx, ldy in elements.  One workgroup per 16 columns reads its rows of w once, its
 * waves split K and add their partial tiles in a fixed order: no atomics, bitwise reproducible.  Rows >= M and columns >= N
 * of y are not touched.
 * EA_E_BADARG: x, w, y NULL or not 16-byte aligned (bias: not 16-byte aligned); ldx < K; ldy < N; a row stride of x or y
 * that is no multiple of 16 bytes; M < 1, K < 1, N < 1; w_dtype not a 16-bit type; x_dtype neither EA_F32 nor w_dtype;
 * y_dtype neither EA_F32 nor w_dtype.  EA_E_UNSUPPORTED: M > 64, K % 32 != 0, N % 16 != 0.  Decided before any launch. */
#define EA_CEVA_LINEAR_MAX_ROWS 64
int ea_ceva_sdecode_linear(int32_t M, int32_t K, int32_t N, const void* x, int32_t x_dtype, int64_t ldx,
                           const void* w, int32_t w_dtype, const void* bias, void* y, int32_t y_dtype, int64_t ldy,
                           void* stream);

/* ABI 24, the feed-forward of a decoder layer's short step on held weights (ea_harness DecoderStack.decode;
 * ea_ceva_decode_linear.hip): ea_ceva_sdecode_linear with a LayerNorm in front and an activation and a residual behind,
 *   y[m, n] = round_y( act( sum_k round_w(LN(x)[m, k]) w[n, k] + bias[n] ) + res[m, n] )
 * in its envelope (1 <= M <= 64, K % 32 == 0, N % 16 == 0).  ln_gamma, ln_beta: fp32 [K], both NULL = no LayerNorm; else every
 * workgroup computes (mean, rstd) of the M rows over K in fp32 -- two passes, biased variance, rsqrt(var + ln_eps), as
 * ea_layernorm_fwd -- and an operand is (x - mean) rstd gamma + beta in fp32, rounded once to w_dtype as it is loaded.
 * act: 0 none, 1 relu.  res: NULL, or [M, ldr] rows of res_dtype = EA_F32 | w_dtype (res_dtype and ldr are not read without
 * res).  Sums, bias, activation and the residual add are fp32, applied by the thread that stores the element after the
 * fixed-order sum over the waves: no atomics, bitwise reproducible.  res may be exactly y (same pointer, dtype, stride: an
 * in-place residual stream); any other overlap of res and y, and x == y, are not supported.
 * Refuses what ea_ceva_sdecode_linear refuses, with its codes, and besides EA_E_BADARG: exactly one of ln_gamma / ln_beta;
 * ln_gamma, ln_beta or res not 16-byte aligned; ln_eps not finite or <= 0 with LayerNorm on; res_dtype neither EA_F32 nor
 * w_dtype; ldr < N or a residual row stride that is no multiple of 16 bytes; x == y.  EA_E_UNSUPPORTED: act outside {0, 1}.
 * Bad arguments are decided before the geometry, everything before any launch. */
int ea_ceva_sdecode_linear_fused(int32_t M, int32_t K, int32_t N, const void* x, int32_t x_dtype, int64_t ldx,
                                 const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w, int32_t w_dtype,
                                 const void* bias, int32_t act, const void* res, int32_t res_dtype, int64_t ldr, void* y,
                                 int32_t y_dtype, int64_t ldy, void* stream);

/* ABI 26, the greedy token pick of a decoding step on a vocabulary table the state holds (ea_harness
 * DecoderStack.next_tokens, init_decoding(hold_vocab=True); ea_ceva_decode_vocab.hip):
 *   logit[m, v] = sum_k round_w(x[m, k]) w[v, k]        fp32, no bias;  1 <= M <= EA_CEVA_LINEAR_MAX_ROWS, any V >= 1
 *   token[m]    = the index of the largest logit[m, 0 .. V - 1]; of equal values the lowest index; in a row that holds NaN
 *                 logits the lowest index that holds one (torch.argmax's rule), decided on the fp32 sums
 *   top[m]      = logit[m, token[m]]
 * x [M, ldx] rows of x_dtype = EA_F32 or w_dtype (fp32 rows are rounded to w_dtype, to nearest even, as they are loaded);
 * w [V, K] row-major of w_dtype = EA_BF16 | EA_F16.  A logit is summed by the operations of ea_ceva_sdecode_linear in their
 * order: it has that entry's bits (bias NULL).  logits: NULL (nothing is stored), or [M, ldl] rows of logits_dtype = EA_F32 |
 * w_dtype (logits_dtype and ldl are not read without logits); columns >= V and rows >= M are not touched.  token [M] int64,
 * top [M] fp32 or NULL.  Two launches: one workgroup per 16 table rows reads them once and writes one (value, index)
 * candidate per row of x to ws; one workgroup per row of x reduces its candidates.  No atomics, no workgroup waits for
 * another: bitwise reproducible.  ws: ea_ceva_sdecode_vocab_ws(M, V) bytes (8 M ceil(V / 16); grows with M and with V, so
 * one sized for 64 rows serves every M); that query returns < 0 for M < 1, M > 64 or V < 1.
 * EA_E_BADARG: x, w, ws, token NULL; x, w or ws not 16-byte aligned, token not 8-byte, top not 4-byte aligned, logits not
 * aligned to its element; w_dtype not a 16-bit type; x_dtype neither EA_F32 nor w_dtype; with logits: logits_dtype neither
 * EA_F32 nor w_dtype, ldl < V; M < 1, K < 1, ldx < K; a row stride of x that is no multiple of 16 bytes; ws_bytes below the
 * query's answer.  EA_E_UNSUPPORTED: M > 64, K % 32 != 0, V < 1.  Bad arguments are decided before the geometry, everything
 * before any launch. */
int64_t ea_ceva_sdecode_vocab_ws(int32_t M, int32_t V);
int ea_ceva_sdecode_vocab_argmax(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                 const void* w, int32_t w_dtype, void* logits, int32_t logits_dtype, int64_t ldl,
                                 void* ws, int64_t ws_bytes, int64_t* token, float* top, void* stream);

/* ABI 27, the SAMPLED token pick on that table (ea_harness DecoderStack.init_sampling, sample_tokens): temperature, top-k and
 * top-p inside the top-k, drawn from a counter-based generator whose per-row counters live on the device.  Two launches.
 * The first is ea_ceva_sdecode_vocab_argmax's first: fp32 logits into logits [M, ldl] (required here; they have
 * ea_ceva_sdecode_linear's bits) and one (value, index) candidate per 16-column tile into ws.  The second, one workgroup per
 * row of x; (value, index) pairs are ordered as the greedy pick orders them -- the larger value first, equal values (+0 and
 * -0 too) by the lower index, NaN (every NaN alike) above every number -- a total order:
 *   1. of the row's NB = ceil(V / 16) candidates the min(top_k, NB) best: the top_k best logits lie in those tiles;
 *   2. of those tiles' logits (columns < V) the k' = min(top_k, V) best, in order: val_0 .. val_{k'-1}, their columns sel_idx;
 *   3. w_j = exp((val_j - val_0) / temperature) in fp32 (expf of library accuracy), c_j = ((w_0 + w_1) + ..) + w_j;
 *   4. kept = the smallest n >= 1 with c_{n-1} >= top_p c_{k'-1}; top_p = 1: k';
 *   5. n = ctr[m]; Philox4x32-10 with the key (seed's low word, seed's high word) and the counter (n's low word, n's high
 *      word, sid[m], 0); u = ((word 0 >> 8) + 0.5) 2^-24 in fp32 (rounded to nearest even where the sum has 25 bits: never 0;
 *      1 for the one largest word); r = u c_{kept-1}; token[m] = sel_idx[j] for the first j < kept with c_j > r, j = kept - 1
 *      when none is; ctr[m] = n + 1.
 *   6. val_0 NaN or infinite: token[m] = sel_idx[0] (the greedy pick's answer), kept = 0, ctr[m] = n + 1.  (A -inf entry
 *      further down has weight 0.)
 * Only row m's workgroup touches ctr[m]; no atomics on memory, no workgroup waits for another: token is a function of the
 * row's logits, (seed, ctr[m], sid[m]) and the three scalars -- not of the batch the row sits in, nor of its position in it.
 * token [M] int64; ctr [M] int64 in / out; sid [M] int32; optional sel_idx [M, top_k] int32, sel_val [M, top_k] fp32 (the
 * stored logits' bits) and kept [M] int32 report the selection: entries j >= k' are not written.  top_k, top_p, temperature
 * and seed are host scalars: a capture fixes them.  ws: ea_ceva_sdecode_vocab_sample_ws(M, V) bytes, which is
 * ea_ceva_sdecode_vocab_ws(M, V): the two entries can share one workspace.
 * EA_E_BADARG: what ea_ceva_sdecode_vocab_argmax answers with it (pointers, alignment, types, strides, ws_bytes); logits,
 * ctr or sid NULL; logits, sid, sel_idx, sel_val or kept not 4-byte, ctr not 8-byte aligned; top_p outside (0, 1];
 * temperature not finite or <= 0; top_k < 1.  EA_E_UNSUPPORTED: top_k > 64, M > 64, K % 32 != 0, V < 1.  Bad arguments are
 * decided before the geometry, everything before any launch. */
int64_t ea_ceva_sdecode_vocab_sample_ws(int32_t M, int32_t V);
int ea_ceva_sdecode_vocab_sample(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                 const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws, int64_t ws_bytes,
                                 int32_t top_k, float top_p, float temperature, uint64_t seed, int64_t* ctr,
                                 const int32_t* sid, int64_t* token, int32_t* sel_idx, float* sel_val, int32_t* kept,
                                 void* stream);

/* ABI 28, TOKEN LOG-PROBABILITIES on that table (ea_harness DecoderStack.init_logprobs, token_logprobs,
 * sample_tokens_logprobs, score): what the greedy and the sampled pick give, and with it
 *   lse[m]  = log sum_{v < V} exp(logit[m, v])          the normaliser of the row's whole, RAW distribution
 *   logp[m] = tl - lse[m]                               one fp32 subtraction
 * The log-probability is that of the model's own, untruncated distribution at temperature 1 -- in the sampled entry too,
 * whatever temperature, top_k and top_p the token was drawn with (what serving stacks report by default).
 * ea_ceva_sdecode_vocab_logprob, two launches.  The first is ea_ceva_sdecode_vocab_argmax's first (logits, candidates and
 * therefore token and top have that entry's bits) and besides writes, per row and 16-column tile t with the maximum m_t,
 * s_t = sum over the tile's columns < V of expf(logit - m_t), summed by an xor butterfly (offsets 8, 4, 2, 1), to lws; with
 * targets it also keeps logit[m, targets[m]].  The second, one workgroup of 512 threads per row, reduces the candidates to
 * token[m], top[m] as the greedy pick does, then by cases on top[m]: NaN -> lse NaN; +inf -> +inf; -inf (every logit is
 * -inf) -> -inf; else lse = top + logf(S), S = sum_t s_t expf(m_t - top) over the tiles with m_t != -inf (such a tile is
 * skipped, never multiplied), each thread its tiles t = thread, thread + 512, .. in order, six xor exchanges per wave, the 8
 * waves added in wave order.  tl is logit[m, targets[m]] with targets (int64 [M], on the device; a target outside [0, V):
 * logp NaN), top[m] without.  Ordinary stores only, no atomics, no workgroup waits for another: bitwise reproducible, and a
 * row's results do not depend on its batch, nor on whether logits are stored.  lse, logp [M] fp32.
 * lws: ea_ceva_sdecode_vocab_lse_ws(M, V) bytes (4 M ceil(V / 16) + 4 M: the tile sums and the targets' logits; grows with M
 * and V); < 0 for M < 1, M > 64 or V < 1.  ws is ea_ceva_sdecode_vocab_ws(M, V) bytes as before.
 * ea_ceva_sdecode_vocab_sample_logprob, three launches: that first launch, ea_ceva_sdecode_vocab_sample's second unchanged
 * (token, ctr, sel_idx, sel_val, kept are that entry's), then the second launch above with tl = logits[m, token[m]], the
 * stored fp32 logit of the token just drawn; token and top are not written by it.
 * EA_E_BADARG: what ea_ceva_sdecode_vocab_argmax / ea_ceva_sdecode_vocab_sample answer with it; lws, lse or logp NULL; lws
 * not 16-byte, lse or logp not 4-byte, targets not 8-byte aligned; lws_bytes below the query's answer.  EA_E_UNSUPPORTED:
 * what those entries answer with it.  Bad arguments are decided before the geometry, everything before any launch. */
int64_t ea_ceva_sdecode_vocab_lse_ws(int32_t M, int32_t V);
int ea_ceva_sdecode_vocab_logprob(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                  const void* w, int32_t w_dtype, void* logits, int32_t logits_dtype, int64_t ldl,
                                  void* ws, int64_t ws_bytes, int64_t* token, float* top, void* lws, int64_t lws_bytes,
                                  const int64_t* targets, float* lse, float* logp, void* stream);
int ea_ceva_sdecode_vocab_sample_logprob(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                         const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws,
                                         int64_t ws_bytes, int32_t top_k, float top_p, float temperature, uint64_t seed,
                                         int64_t* ctr, const int32_t* sid, int64_t* token, int32_t* sel_idx, float* sel_val,
                                         int32_t* kept, void* lws, int64_t lws_bytes, float* lse, float* logp, void* stream);

/* ABI 29, the LARA forward combine with the OUTPUT PROJECTION inside (ea_lara_xp.hip): for a model of three heads of 64
 * channels, y = out W_proj^T + bias is formed by the pass that forms `out`, from registers and LDS -- one launch instead of
 * ea_lara_out_fwd_merge + ea_linear[192->192], `out` written once (the weight gradient reads it) and not read back.
 *   ea_lara_out_proj_fwd_merge: ea_lara_out_fwd_merge plus w_proj16 [192,192] in the EA dtype (contiguous, 16-byte aligned:
 *       ea_linear's weight operand, w16p of ea_linear_w192_prepare), bias [192] fp32 or NULL (rounded to the EA dtype before
 *       it is added, the sum rounded once, as ea_linear does), y [B*N, 192] in the EA dtype with row stride ldy elements
 *       (ldy >= 192, a multiple of 4; y 8-byte aligned).  out, lseZ, tmean, kv, lse_k, lse_t, cst have ea_lara_out_fwd_merge's
 *       bits and y those of ea_linear on that `out` (its k-slots, its order of accumulation).
 *   ea_lara_layer_fwd_proj: ea_lara_layer_fwd with that pass as its last launch.
 * EA_E_UNSUPPORTED -- before anything is launched, so the caller can fall back to the two calls -- unless H = 3, D = 64,
 * C <= 64 samples and the folded merge applies (S = ea_lara_parts <= 4; EA_LARA_FOLD not 0). */
int ea_lara_out_proj_fwd_merge(const ea_lara_geom* g, const ea_t4* q, const float* omega, const float* qbar, const float* bhv,
                               int32_t S, const float* p_ml, const float* p_kv, const float* lp, float* kv, float* lse_k,
                               float* lse_t, float* cst, const ea_t4* out, float* lseZ, float* tmean, const void* w_proj16,
                               const float* bias, void* y, int64_t ldy, void* stream);
int ea_lara_layer_fwd_proj(const ea_lara_layer* cfg, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                           const float* noise, const float* const* params, const ea_t4* out, float* saved, float* tmp,
                           int32_t keep_for_backward, const void* w_proj16, const float* bias, void* y, int64_t ldy,
                           void* stream);

/* ABI 30, the MANY-ROW vocabulary pass (ea_harness DecoderStack.rows_logprobs, evaluate; ea_vocab_score.hip): what
 * ea_ceva_sdecode_vocab_logprob gives, for any number of rows in one call -- a GEMM on the matrix cores whose epilogue is the
 * pick and an online log-sum-exp, so that no logit leaves the chip and the table is read once per 128 rows, not per 64:
 *   logit[m, v] = sum_k round_w(x[m, k]) w[v, k]        fp32, no bias;  any M >= 1, K % 32 == 0, any V >= 1
 *   token[m]    = the index of the largest logit[m, 0 .. V - 1]; of equal values the lowest index; in a row that holds NaN
 *                 logits the lowest index that holds one (torch.argmax's rule), decided on the fp32 sums
 *   top[m]      = logit[m, token[m]]
 *   lse[m]      = by cases on top[m]: NaN -> NaN; +inf -> +inf; -inf (every logit is -inf) -> -inf; else top + logf(S),
 *                 S = sum_v expf-weights of the row against top; partials whose maximum is -inf are skipped, never multiplied
 *   logp[m]     = logit[m, targets[m]] - lse[m] with targets (int64 [M] on the device; one outside [0, V): NaN), else
 *                 top[m] - lse[m]; one fp32 subtraction
 * x [M, ldx] rows of x_dtype = EA_F32 or w_dtype (fp32 rows are rounded to w_dtype, to nearest even, as they are loaded);
 * w [V, K] row-major of w_dtype = EA_BF16 | EA_F16.  The order of a logit's summation is this kernel's own (k in steps of 32
 * on one accumulator): a logit need NOT have the bits ea_ceva_sdecode_vocab_argmax gives it.  logits: NULL (nothing is
 * stored: the normal case), or [M, ldl] rows of logits_dtype = EA_F32 | w_dtype (not read without logits); columns >= V and
 * rows >= M are not touched; token, top, lse and logp have the same bits with and without it.  top [M] fp32 or NULL.
 * Two launches.  The first: workgroup (slice, row tile) owns EA_VOCAB_SCORE_BM rows of x and one slice of EA_VOCAB_SCORE_SL
 * columns, walks it in blocks of EA_VOCAB_SCORE_BN columns (v_mfma_f32_16x16x32 on LDS-staged tiles) and keeps per row a
 * running (maximum, index, sum of exponentials, the target's logit) across the blocks; the sum is rescaled only when the
 * maximum rises; one partial per (row, slice) goes to ws.  The second: one thread per row folds the row's slices in slice
 * order.  The three widths are compile-time constants (ea_vocab_score_tile(0 | 1 | 2) = BM | BN | SL; another argument:
 * EA_E_BADARG), so the partition of the columns depends on V alone: a row's four results do not depend on M, on the rows
 * beside it or on its place in the batch.  Ordinary stores only, no atomics, no workgroup waits for another: bitwise
 * reproducible.  ws: ea_vocab_score_ws(M, V) bytes (12 M ceil(V / SL) + 4 M, rounded up to 16; grows with M and with V);
 * < 0 for M < 1, V < 1 or more than 2^23 workgroups (ceil(M / BM) ceil(V / SL)).
 * EA_E_BADARG: x, w, ws, token, lse, logp NULL; x, w or ws not 16-byte aligned, token or targets not 8-byte, top, lse or logp
 * not 4-byte aligned, logits not aligned to its element; w_dtype not a 16-bit type; x_dtype neither EA_F32 nor w_dtype; with
 * logits: logits_dtype neither EA_F32 nor w_dtype, ldl < V; M < 1, K < 1, ldx < K; a row stride of x that is no multiple of
 * 16 bytes; ws_bytes below the query's answer.  EA_E_UNSUPPORTED: K % 32 != 0, V < 1, more than 2^23 workgroups.  Bad
 * arguments are decided before the geometry, everything before any launch. */
#define EA_VOCAB_SCORE_BM 128
#define EA_VOCAB_SCORE_BN 128
#define EA_VOCAB_SCORE_SL 2048
int64_t ea_vocab_score_ws(int32_t M, int32_t V);
int32_t ea_vocab_score_tile(int32_t which);
int ea_vocab_score(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                   int32_t w_dtype, const int64_t* targets, void* logits, int32_t logits_dtype, int64_t ldl, void* ws,
                   int64_t ws_bytes, int64_t* token, float* top, float* lse, float* logp, void* stream);

/* ABI 32, the BEAM STEP on the held vocabulary table (ea_harness DecoderStack.init_beam_search, beam_step, beam_search;
 * ea_ceva_decode_vocab.hip): one step of a beam search whose whole state lives on the device, so that a captured step can
 * be replayed.  S sentences, beam width W, M = S W rows, row m = s W + b is beam b of sentence s; 1 <= W <= 32, M <= 64,
 * 0 <= eos < V; max_new >= 1 is the largest number of generated tokens of a hypothesis, the closing eos included.
 * State, in / out: score [M] fp32 (the sum of the log-probabilities of a beam's tokens; to start: 0 for beam 0, -inf for the
 * others, so that of W copies of a prompt only the first counts), t [S] int32 (tokens generated), nfin [S] int32 (finished
 * hypotheses, <= W), done [S] int32; t = nfin = done = 0 to start.
 * ea_ceva_sdecode_vocab_beam, three launches.  The first is ea_ceva_sdecode_vocab_logprob's first: fp32 logits into logits
 * [M, ldl] (required), one (value, index) candidate and one sum of exponentials per 16-column tile into the workspace.
 *   A. the rows, one workgroup of 512 threads per row of a sentence that is not done; t = t[s]:
 *      lse[m]: ea_ceva_sdecode_vocab_logprob's, by the same operations in the same order: the same bits;
 *      forced step (t + 1 == max_new): one candidate (k' = 1), token eos, value logits[m, eos]; otherwise the row's
 *      k' = min(2 W, V) best logits in order, steps 1-2 of ea_ceva_sdecode_vocab_sample at top_k = 2 W: sel_idx, sel_val;
 *      cand_idx[m, j] = sel_idx[j], cand_score[m, j] = score[m] + (sel_val[j] - lse[m]): two fp32 operations, the subtraction
 *      first, nothing fused or reassociated.  Entries j >= k' are not written.
 *   B. the merge, one workgroup per sentence that is not done: its W k' candidates are ordered by score under the sampler's
 *      total order -- NaN above every number, the larger first, +0 and -0 equal, equal scores by the lower flat index
 *      f = b k' + j -- and the first n2 = min(2 W, W k') are walked in order, i = 0 .. n2 - 1.  A candidate whose token is eos
 *      never continues; it is recorded as a finished hypothesis iff i < W, its score is not -inf and nfin[s] < W, in slot
 *      nfin[s]++: fin_score (the raw score), fin_len = t + 1, fin_beam = b (the beam it extends).  The first W candidates
 *      whose token is not eos become the beams r = 0 .. W - 1 of the next step: token[s W + r], parent[s W + r] = s W + b (a
 *      global row: the new_order of a state reorder), score[s W + r], hist_tok[t, s W + r], hist_par[t, s W + r] = b.  Where
 *      fewer than W go on, the remaining beams are dead: token eos, parent their own row, score -inf, hist_tok eos,
 *      hist_par their own beam.  Then t[s] += 1, and done[s] = 1 if nfin[s] == W or the step was the forced one.
 *   C. a done sentence: token eos and parent = own row for its W rows; score, t, nfin, the records and the history stay.
 * The normalised score (fin_score / fin_len ** len_penalty) is the host's: it never feeds back into the search.  Tokens of a
 * hypothesis: backtrack hist_par / hist_tok from (fin_len - 2, fin_beam), then eos.
 * token, parent [M] int64; hist_tok, hist_par [max_new, M] int32; fin_score [S, W] fp32; fin_len, fin_beam [S, W] int32.
 * Optional reports, each NULL or: cand_idx [M, 2 W] int32, cand_score [M, 2 W] fp32, lse [M] fp32 (the merge then reads the
 * lists from there), sel_val [M, 2 W] fp32 (the selected logits' stored bits).  W, eos and max_new are host scalars: a capture
 * fixes them.  Ordinary stores only, no atomics on memory, no workgroup waits for another; only sentence s's workgroup touches
 * t[s], nfin[s], done[s] and its records: bitwise reproducible, and a sentence's results do not depend on its batch.
 * ws: ea_ceva_sdecode_vocab_beam_ws(M, V, W) bytes = r16(8 M NB) + r16(4 M NB + 4 M) + 2 r16(8 M W) + r16(4 M), NB =
 * ceil(V / 16), r16 rounding up to a multiple of 16: the candidates, the tile sums (with ea_ceva_sdecode_vocab_lse_ws' M
 * spare floats), the two [M, 2 W] lists and lse; < 0 for M < 1, M > 64, V < 1, W < 1, W > 32 or M % W != 0.
 * EA_E_BADARG: what ea_ceva_sdecode_vocab_sample answers with it for x, w, logits and their strides; ws NULL or not 16-byte
 * aligned; a state or output pointer NULL; token or parent not 8-byte, any other one (the reports too) not 4-byte aligned;
 * W < 1, eos outside [0, V), max_new < 1; ws_bytes below the query's answer.  EA_E_UNSUPPORTED: W > 32, M > 64, M % W != 0,
 * K % 32 != 0, V < 1.  Bad arguments are decided before the geometry, everything before any launch.
 * ea_beam_merge: launch B / C alone, on candidate lists the caller supplies: cand_idx, cand_score [S W, 2 W] (the row stride
 * is 2 W whatever kc), kc <= 2 W live per row (k' = kc; the forced step reads entry 0 of each row alone: k' = 1), the same
 * state and outputs; eos is any token id >= 0.  ea_ceva_sdecode_vocab_beam launches the same kernel.  EA_E_BADARG: S < 1,
 * W < 1, kc outside 1 .. 2 W, eos < 0, max_new < 1, a NULL or misaligned pointer; EA_E_UNSUPPORTED: W > 32, S W > 64. */
int64_t ea_ceva_sdecode_vocab_beam_ws(int32_t M, int32_t V, int32_t W);
int ea_ceva_sdecode_vocab_beam(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                               const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws, int64_t ws_bytes,
                               int32_t W, int32_t eos, int32_t max_new, float* score, int32_t* t, int32_t* nfin,
                               int32_t* done, int64_t* token, int64_t* parent, int32_t* hist_tok, int32_t* hist_par,
                               float* fin_score, int32_t* fin_len, int32_t* fin_beam, int32_t* cand_idx, float* cand_score,
                               float* lse, float* sel_val, void* stream);
int ea_beam_merge(int32_t S, int32_t W, int32_t kc, const int32_t* cand_idx, const float* cand_score, int32_t eos,
                  int32_t max_new, float* score, int32_t* t, int32_t* nfin, int32_t* done, int64_t* token, int64_t* parent,
                  int32_t* hist_tok, int32_t* hist_par, float* fin_score, int32_t* fin_len, int32_t* fin_beam, void* stream);

/* ABI 33, ADAPTIVE-SOFTMAX SCORING (ea_harness DecoderStack.adaptive_tables, rows_logprobs, evaluate on an adaptive stack;
 * ea_adaptive_score.hip): teacher-forced log-probabilities under fairseq's adaptive softmax, on the tile loop of ABI 30.
 * cutoffs [n_tails + 1] (a HOST array, read before the first launch): 1 <= c0 < c1 < .. < c_n = V < 2^31.  The head holds the
 * tokens [0, c0) and one class column per tail, c0 + n_tails columns; tail i holds [c_i, c_{i+1}), V_i tokens at width d_i.
 * 1 <= n_tails <= EA_ADAPTIVE_MAX_TAILS.  Every kernel: ordinary stores only, no atomics, no workgroup waits for another,
 * bitwise reproducible, launches only (a call can be captured; sizes and cutoffs are host scalars a capture fixes).
 *
 * ea_adaptive_route, one launch of one workgroup: targets [M] int64 ->
 *   head_target[m] (int64) = t for 0 <= t < c0; c0 + i for t in tail i; -1 for t outside [0, V)
 *   rows[i][0 .. count[i]) (int32, rows is [n_tails][M], row stride M) = the rows whose target lies in tail i, ASCENDING (a
 *   stable compaction); entries at or beyond count[i] are left as they were;  count [n_tails] int32, on the device.
 * EA_E_BADARG: M < 1, n_tails < 1, cutoffs NULL, not increasing or c0 < 1, a NULL pointer, targets or head_target not 8-byte,
 * rows or count not 4-byte aligned.  EA_E_UNSUPPORTED: n_tails > EA_ADAPTIVE_MAX_TAILS, V >= 2^31.
 *
 * ea_vocab_score_rows: ea_vocab_score over a gathered, device-counted set of rows.  Its arguments, then
 *   rows         int32 [M] on the device, indices of rows of x and of entries of targets; NULL: the identity
 *   count        int32 device scalar, 0 <= *count <= M (kept inside that range); NULL: M
 *   target_base  >= 0, subtracted from a target before the test against [0, V): logp[j] = logit[j, targets[rows[j]] -
 *                target_base] - lse[j]
 *   logits_only  0 | 1.  1: the first launch alone, without the pick / log-sum-exp bookkeeping: a GEMM whose output is
 *                `logits` (then required; token, top, lse, logp, targets are neither read nor written and may be NULL)
 * M is the number of POSITIONS: the grid and ws (ea_vocab_score_rows_ws(M, V) = ea_vocab_score_ws(M, V)) are sized for it.
 * Position j < *count reads row rows[j] of x and writes token[j], top[j], lse[j], logp[j] and row j of logits.  A workgroup
 * whose row tile starts at or beyond *count returns before its first operand load; inside the last live tile a position
 * >= *count is clamped to position *count - 1 BEFORE rows[] is read, so a list entry at or beyond *count is never
 * dereferenced; results at positions >= *count are not written; *count == 0 writes nothing.  A position's results depend on
 * the row it names, on V and on K alone; with rows = count = NULL, target_base = 0 they have ea_vocab_score's bits.
 * Errors: ea_vocab_score's; also target_base < 0, logits_only outside {0, 1}, rows or count not 4-byte aligned: EA_E_BADARG.
 *
 * ea_adaptive_score: the whole score in one call, 4 + 3 n_tails launches.  x [M, ldx] of x_dtype = EA_F32 | w_dtype, targets
 * [M] int64; the held operands, all of w_dtype = EA_BF16 | EA_F16, row-major, 16-byte aligned: head [c0 + n_tails, C] (the
 * band-0 table with the class rows behind it); proj[i] [d_i, C] (K-contiguous: a tied [C, d_i] projection transposed once);
 * tables[i] [V_i, d_i].  dims, proj, tables are HOST arrays of n_tails entries.
 *   route;  head: ea_vocab_score_rows' two launches on every row with head_target;  per tail i: the projection (one launch,
 *   logits_only, rows[i] / count[i]: h_i = round_w(x[rows[i][j]] proj_i^T), compact, row j of h_i for position j), then the
 *   tail (two launches on h_i, identity rows, count[i], targets read through rows[i], target_base = c_i);  combine (one
 *   launch): logp[m] = logp_head[m] for a head row, logp_head[m] + logp_tail_i[j] where rows[i][j] == m: one fp32 addition.
 * A row whose target is outside [0, V) gets NaN.  token_head [M] int64 or NULL: the greedy pick among the head's columns.
 * ws, r16 rounding up to a multiple of 16, the parts in this order from byte 0:
 *   head_target int64 [M]  r16(8 M) | rows int32 [n_tails][M]  r16(4 n_tails M) | count int32 [EA_ADAPTIVE_MAX_TAILS]  16 |
 *   token_head int64 [M]  r16(8 M) | lse_head fp32 [M]  r16(4 M) | logp_head fp32 [M]  r16(4 M) |
 *   for i = 0 .. n_tails - 1:  h_i w_dtype [M][d_i]  r16(2 M d_i) | token_i int64 [M]  r16(8 M) | lse_i  r16(4 M) | logp_i
 *   r16(4 M)  (position-indexed: entry j belongs to row rows[i][j]) |
 *   inner: ONE ea_vocab_score_rows workspace the passes use in turn, the largest of ea_vocab_score_ws(M, c0 + n_tails),
 *   ea_vocab_score_ws(M, d_i), ea_vocab_score_ws(M, V_i)
 * ea_adaptive_score_ws(M, n_tails, cutoffs, dims) = 16 + r16(4 n_tails M) + 2 r16(8 M) + 2 r16(4 M) + sum_i (r16(2 M d_i) +
 * r16(8 M) + 2 r16(4 M)) + inner; < 0 for M < 1, n_tails outside 1 .. EA_ADAPTIVE_MAX_TAILS, cutoffs not increasing, c0 < 1,
 * V >= 2^31, d_i < 1, or an inner pass outside ea_vocab_score_ws' envelope.
 * EA_E_BADARG: a NULL array or operand, misaligned operands (x, head, proj[i], tables[i], ws: 16 bytes; targets, token_head: 8;
 * logp: 4), cutoffs as above, w_dtype not 16-bit, x_dtype neither EA_F32 nor w_dtype, M < 1, C < 1, ldx < C or a row stride of
 * x that is no multiple of 16 bytes, d_i < 1, ws_bytes below the query's answer.  EA_E_UNSUPPORTED: n_tails >
 * EA_ADAPTIVE_MAX_TAILS, C % 32 != 0, d_i % 32 != 0, a geometry the query refuses.  Bad arguments are decided before the
 * geometry, everything before any launch. */
#define EA_ADAPTIVE_MAX_TAILS 4
int ea_adaptive_route(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int64_t* targets, int64_t* head_target,
                      int32_t* rows, int32_t* count, void* stream);
int64_t ea_vocab_score_rows_ws(int32_t M, int32_t V);
int ea_vocab_score_rows(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                        int32_t w_dtype, const int64_t* targets, void* logits, int32_t logits_dtype, int64_t ldl, void* ws,
                        int64_t ws_bytes, int64_t* token, float* top, float* lse, float* logp, const int32_t* rows,
                        const int32_t* count, int64_t target_base, int32_t logits_only, void* stream);
int64_t ea_adaptive_score_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims);
int ea_adaptive_score(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                      int32_t x_dtype, int64_t ldx, const int64_t* targets, const void* head, int32_t w_dtype,
                      const void* const* proj, const void* const* tables, void* ws, int64_t ws_bytes, float* logp,
                      int64_t* token_head, void* stream);

/* ABI 34, THE GREEDY PICK FROM THE ADAPTIVE HEAD (ea_harness DecoderStack.init_adaptive_decoding, next_tokens,
 * token_logprobs, score, generate on such a state; ea_adaptive_pick.hip): fairseq's get_log_prob(x, None) followed by an
 * argmax, for the 1 <= M <= 64 rows of a decoding step, from the held tables of ABI 33 and without a [M, V] tensor.
 * cutoffs, dims, proj, tables: HOST arrays as in ea_adaptive_score; x [M, ldx] of x_dtype = EA_F32 | w_dtype; targets [M]
 * int64 on the device, or NULL; token [M] int64, logp [M] fp32.  For row m, every operation in fp32:
 *   a[v], v < c0 + n         the head's logits, x against head (ea_ceva_sdecode_vocab_logprob's bits)
 *   h_i = round_w(x proj_i^T) ea_ceva_sdecode_linear's bits (bias NULL, y_dtype = w_dtype)
 *   b_i[u], u < V_i          tail i's logits, h_i against tables[i]
 *   lse_h over ALL c0 + n head columns, lse_i over tail i;  lse by ABI 28's cases on the maximum: NaN -> NaN; +inf -> +inf;
 *                            -inf -> -inf; else max + logf(S), a partial whose maximum is -inf skipped, never multiplied
 *   s(v) = a[v] - lse_h for a word v < c0;  s(c_i + u) = (a[c0 + i] - lse_h) + (b_i[u] - lse_i): those operations, that order
 *   token[m] = the index of the largest s: per band the candidate is the largest RAW logit under the pick's total order
 *              (the larger value, of equals the lower index, NaN above every number); the n + 1 candidates' scores are
 *              compared under the same order on (s, vocabulary index): equal scores go to the lower token.  Always in [0, V).
 *   logp[m]  = s(targets[m]) with targets (one outside [0, V): NaN), else s(token[m]).
 * A row with non-finite logits follows the cases per band: its logp may be NaN; no other row's bits change.
 * Launches: 4 + n_tails with joined projections (3.), n_tails - 1 more with separate ones, and one more per tail wider than
 * EA_ADAPTIVE_PICK_MAX_K when targets are given:
 *   1. the head's words: ea_ceva_sdecode_vocab_logprob's first launch on head[0 .. c0): per 16-column tile (maximum, index,
 *      sum of exponentials), and the target's logit;
 *   2. the head's classes: the same kernel on the n rows at head + c0 C, the fp32 logits stored;
 *   3. the projections: ea_ceva_sdecode_linear's kernel into h [M][D], D = sum d_i, h_i in columns off_i = d_0 + .. + d_{i-1};
 *      ONE launch where proj[i + 1] == proj[i] + d_i C elements for every i (one concatenated copy), else one per tail;
 *   4. per tail: d_i <= EA_ADAPTIVE_PICK_MAX_K: the column-split kernel.  A workgroup of 8 waves owns EA_ADAPTIVE_PICK_SPAN
 *      columns, a wave EA_ADAPTIVE_PICK_SPAN / 128 whole 16-column tiles; a logit is ONE v_mfma_f32_16x16x32 accumulator
 *      chained over the d_i / 32 k-steps in ascending order -- this kernel's own summation order, NOT
 *      ea_ceva_sdecode_linear's.  Per row and wave the vocab epilogue's partial over the wave's columns: a lane folds its
 *      column of the wave's tiles in tile order, the 16 lanes of a row reduce once (the candidate; then the sum of
 *      expf(logit - its value), a lane's terms in tile order, the xor butterfly 8, 4, 2, 1); the workgroup merges its waves
 *      in wave order (the better candidate; sum = s_a expf(m_a - m) + s_b expf(m_b - m), a side whose maximum is -inf
 *      skipped): one partial per row and span.  d_i > EA_ADAPTIVE_PICK_MAX_K: launch 1's kernel on h_i
 *      (K split over the waves; one partial per 16 columns), behind a launch that writes targets - c_i where targets are given;
 *   5. the pick, one workgroup of 256 threads per row: per band the best partial (thread j its partials j, j + 256, .. in
 *      order, six xor exchanges per wave, the 4 waves in wave order), then S = sum_j s_j expf(m_j - top) the same way, added
 *      in wave order; the head's top is the larger of the words' and the classes' maximum and its S takes the class tile's
 *      partial last; then the scores, token and logp.  token may be a captured step's static input.
 * Ordinary stores only, no atomics, no workgroup waits for another: bitwise reproducible; a row's results depend on that row
 * alone (not on M, nor on the rows beside it).
 * ws, r16 rounding up to a multiple of 16, the parts in this order from byte 0; after a call it holds
 *   cls fp32 [M][n]  r16(4 M n): a[c0 + i] | h w_dtype [M][D]  r16(2 M D) |
 *   for b = 0 .. n (band 0: the head's words; band i + 1: tail i):  best (fp32 value, int32 index IN the band) [M]  r16(8 M) |
 *   lse fp32 [M]  r16(4 M) (band 0: lse_h) | tlogit fp32 [M]  r16(4 M) (written only where the row's target lies in the band) |
 *   for each tail with d_i > EA_ADAPTIVE_PICK_MAX_K: int64 [M]  r16(8 M) |
 *   the class tile's partial: r16(8 M), r16(4 M) |
 *   for b = 0 .. n the passes' partials: (value, index) [M][P_b]  r16(8 M P_b), sums fp32 [M][P_b]  r16(4 M P_b);
 *   P_0 = ceil(c0 / 16); P_{i+1} = ceil(V_i / EA_ADAPTIVE_PICK_SPAN) for d_i <= EA_ADAPTIVE_PICK_MAX_K, else ceil(V_i / 16)
 * ea_adaptive_pick_ws(M, n_tails, cutoffs, dims) is their sum (it grows with M); < 0 for M < 1, M > 64, n_tails outside
 * 1 .. EA_ADAPTIVE_MAX_TAILS, cutoffs not increasing, c0 < 1, d_i < 1, V > 2^31 - 1 - 2 EA_ADAPTIVE_PICK_SPAN.
 * EA_E_BADARG: a NULL array or operand, misaligned operands (x, head, proj[i], tables[i], ws: 16 bytes; targets, token: 8;
 * logp: 4), cutoffs as above, w_dtype not 16-bit, x_dtype neither EA_F32 nor w_dtype, M < 1, C < 1, ldx < C or a row stride of
 * x that is no multiple of 16 bytes, d_i < 1, ws_bytes below the query's answer.  EA_E_UNSUPPORTED: M > 64, n_tails >
 * EA_ADAPTIVE_MAX_TAILS, C % 32 != 0, d_i % 32 != 0, a geometry the query refuses.  Bad arguments are decided before the
 * geometry, everything before any launch. */
#ifndef EA_ADAPTIVE_PICK_SPAN                 /* (a build may try another multiple of 128) */
#define EA_ADAPTIVE_PICK_SPAN 512
#endif
#define EA_ADAPTIVE_PICK_MAX_K 256
int64_t ea_adaptive_pick_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims);
int ea_adaptive_pick(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                     int32_t x_dtype, int64_t ldx, const int64_t* targets, const void* head, int32_t w_dtype,
                     const void* const* proj, const void* const* tables, void* ws, int64_t ws_bytes, int64_t* token,
                     float* logp, void* stream);

/* ABI 35, SAMPLING AND THE BEAM STEP FROM THE ADAPTIVE HEAD (ea_harness DecoderStack.init_sampling, sample_tokens,
 * sample_tokens_logprobs, init_beam_search, beam_step, beam_search, generate on a state with an adaptive pick;
 * ea_adaptive_pick.hip): the exact k best JOINT log-probabilities of a row across the head and the tails, 1 <= k <= 64, then
 * ea_ceva_sdecode_vocab_sample's draw on them (k = top_k) or the beam step's candidates (k = 2 W) and ea_beam_merge.  Names
 * and operands are ABI 34's (no targets); 1 <= M <= 64 rows, 16-bit tables.
 * THE RULE.  The joint score of a token is formed in fp32 by these operations only, in this order (a host program that reads
 * the stored logits, cls and lse out of the workspace reproduces the bits):
 *   a word v < c0:     s = a[v] - lse_h
 *   a token c_i + u:   s = (a[c0 + i] - lse_h) + (b_i[u] - lse_i)
 * Bands: band 0 is the head's words (V_0 = c0 columns), band i + 1 is tail i.  Per band the min(k, V_b) best RAW logits under
 * the pick's total order (the larger value, of equals -- +0 and -0 are equal -- the lower index, NaN above every number) are
 * taken; their joint scores are formed; the min(k, V) best of those (at most (n + 1) k) under the same order on
 * (s, vocabulary index) are the selection, sorted, the best first.  One consequence: where fp32 rounding makes two logits of
 * one band equal as joint scores exactly at that band's k-th place, the band's RAW order has decided which of them is a
 * candidate; and inside the selection equal joint scores stand in the order of their vocabulary indices.  With k = 1 the
 * selection is ea_adaptive_pick's token and logp bit for bit (the same launches, the same lse device function); with k > 1
 * entry 0 has ea_adaptive_pick's logp, and its token unless rounding has made a lower-indexed logit of the winner's band equal
 * to it as a joint score.  A row with non-finite logits follows ABI 34's cases per band; a best joint score that is NaN or
 * infinite gives the greedy token (entry 0) and kept = 0, as ea_ceva_sdecode_vocab_sample does.
 * LAUNCHES, 6 + n_tails with joined projections (the beam step: one more):
 *   1 .. 4. ea_adaptive_pick's launches 1 .. 4, with every band's fp32 logits stored: the table pass with `logits` set for the
 *      head's words and for tails with d_i > EA_ADAPTIVE_PICK_MAX_K (its 16-column partials are the tile candidates); for
 *      d_i <= EA_ADAPTIVE_PICK_MAX_K the column-split kernel's instance that also stores its logits and writes one (value,
 *      index) candidate per 16-column tile -- a 16-lane reduction per tile, before the fold across tiles; the span partials
 *      and sums are what launch 4 of ABI 34 writes.
 *   5. the select, grid (row, band), 512 threads: the band's lse by the pick kernel's two passes (its first 256 threads, its
 *      order; the head takes the class tile's partial last), then ea_ceva_sdecode_vocab_sample's steps 1-2 (the exact radix
 *      selection) over the band's tile candidates and stored logits: lse[b][m] and the band's sorted (column, raw logit) list.
 *   6. the joint, one workgroup of 512 threads per row: the lists' joint scores as 64-bit keys (score image, complement of the
 *      vocabulary index), the radix threshold, compaction and rank sort in LDS, entry j in lane j of one wave, its score formed
 *      again from the stored logit.  Then one of
 *      sampled: ea_ceva_sdecode_vocab_sample's steps 3-6 on the joint scores: weights expf((s_j - s_0) / temperature) -- the
 *        temperature acts on the joint log-probabilities --, c_j = ((w_0 + w_1) + ..) + w_j, the smallest head reaching top_p of
 *        the list's weight (kept), one Philox4x32-10 word at counter (ctr[m], sid[m]) under `seed`, ctr[m] += 1; token [M]
 *        int64, logp[m] = s(token[m]) (the RAW distribution's, temperature 1, nothing truncated), and, each NULL or: sel_idx
 *        [M, top_k] int32 (vocabulary indices), sel_val [M, top_k] fp32 (joint scores), kept [M] int32; entries from
 *        min(top_k, V) on are not written.
 *      beam (k = 2 W): cand_idx[m, j] = the token, cand_score[m, j] = score[m] + s_j (one fp32 addition), j < min(2 W, V); the
 *        rows of a done sentence are skipped (by launch 5 too); on the forced step (t[s] + 1 >= max_new) the single candidate is
 *        eos with its joint score from the stored logits of the band eos lies in.
 *   7. the beam step: ea_beam_merge's launch on those lists, unchanged (ABI 32, B / C); kc = min(2 W, V).
 * Ordinary vector stores only; integer LDS atomics in the radix histograms (their counts do not depend on their order); no
 * atomics on memory; no workgroup waits for another; launches only: capturable, bitwise reproducible, and a row's (the beam
 * step: a sentence's) results do not depend on the rows beside it nor on M.
 * ws, r16 rounding up to a multiple of 16, the parts in this order from byte 0:
 *   ea_adaptive_pick's workspace for the same (M, n_tails, cutoffs, dims), ea_adaptive_pick_ws bytes: after a call cls, h, lse
 *   (per band), the class tile's partial and the passes' partials are what ea_adaptive_pick leaves; best and tlogit are not
 *   written |
 *   for b = 0 .. n: the band's logits fp32 [M][V_b]  r16(4 M V_b) |
 *   for each tail with d_i <= EA_ADAPTIVE_PICK_MAX_K: tile candidates (value, index) [M][ceil(V_i / 16)]  r16(8 M ceil(V_i / 16)) |
 *   the bands' lists: columns IN the band int32 [M][n + 1][64]  r16(256 M (n + 1)), raw logits fp32 [M][n + 1][64]  the same
 *   (entries from min(k, V_b) on are not written) |
 *   ea_adaptive_beam alone: cand_idx int32 [M][2 W]  r16(8 M W), cand_score fp32 [M][2 W]  r16(8 M W) (used where the
 *   caller passes NULL for them)
 * ea_adaptive_sample_ws / ea_adaptive_beam_ws are their sums: about 4 M V bytes; < 0 where ea_adaptive_pick_ws is, and for
 * W < 1, W > 32 or M % W != 0.
 * EA_E_BADARG: ea_adaptive_pick's for the operands and ws; token NULL or not 8-byte aligned, logp NULL; ctr, sid NULL or
 * misaligned (8, 4 bytes), a misaligned report, top_k < 1, top_p outside (0, 1], temperature not finite or <= 0; the beam's state
 * as in ea_ceva_sdecode_vocab_beam (a state or output pointer NULL or misaligned, W < 1, eos outside [0, V), max_new < 1);
 * ws_bytes below the query's answer.  EA_E_UNSUPPORTED: top_k > 64, W > 32, M > 64, M % W != 0, and ea_adaptive_pick's
 * geometry refusals.  Bad arguments are decided before the geometry, everything before any launch.  ea_adaptive_pick and
 * ea_adaptive_pick_ws are what they were. */
int64_t ea_adaptive_sample_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims);
int ea_adaptive_sample(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                       int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype, const void* const* proj,
                       const void* const* tables, void* ws, int64_t ws_bytes, int32_t top_k, float top_p, float temperature,
                       uint64_t seed, int64_t* ctr, const int32_t* sid, int64_t* token, float* logp, int32_t* sel_idx,
                       float* sel_val, int32_t* kept, void* stream);
int64_t ea_adaptive_beam_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, int32_t W);
int ea_adaptive_beam(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                     int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype, const void* const* proj,
                     const void* const* tables, void* ws, int64_t ws_bytes, int32_t W, int32_t eos, int32_t max_new,
                     float* score, int32_t* t, int32_t* nfin, int32_t* done, int64_t* token, int64_t* parent,
                     int32_t* hist_tok, int32_t* hist_par, float* fin_score, int32_t* fin_len, int32_t* fin_beam,
                     int32_t* cand_idx, float* cand_score, void* stream);

/* ABI 36, THE CONSTRAINED BEAM STEP: min_len, n-gram blocking and static bans in the beam step of both heads (ea_harness
 * DecoderStack.init_beam_constraints, set_beam_prompt, constrained_beam_search; beam_search on a state that carries them;
 * ea_ceva_decode_vocab.hip, ea_voc_ban.h, ea_adaptive_pick.hip).  fairseq's SequenceGenerator options --min-len and
 * --no-repeat-ngram-size and its ban on pad, decided on the device from state the captured step already carries.
 * THE RULE, for row m of sentence s at t = t[s], the sentence not done and the step not the forced one (t + 1 < max_new):
 *   the row's sequence is x = prompt_s[0 .. plen_s) ++ g_m[0 .. t), L = plen_s + t tokens: the prompt counts (in fairseq's
 *   language-model generation the prompt is part of `tokens`), g_m are the tokens this beam has generated;
 *   its banned set is the union of
 *     the static bans   ban_tokens[0 .. n_ban_tokens), at most 16 host scalars a capture fixes, none of them eos;
 *     minimum length    eos, while t < min_len: a finished hypothesis has at least min_len tokens before its eos;
 *     n-gram blocking   n = ngram >= 1: for every i in 0 .. L - n (none when L < n) with x[i .. i + n - 1) == x[L - n + 1 .. L),
 *                       the token x[i + n - 1]; n = 1 bans every token of x.  NGramRepeatBlock._no_repeat_ngram of fairseq,
 *                       position for position.
 *   lse[m] (the adaptive head: every band's) comes from the UNCONSTRAINED logits, by the unconstrained entry's operations: the
 *   same bits (fairseq bans after log_softmax).  The row's k' = min(2 W, V) candidates are its best logits (joint scores) with
 *   every banned column at -inf; the total order is unchanged, ties to the lower index.  With fewer than k' columns unbanned
 *   a banned one is selected, with score -inf; rule B drops an eos whose score is -inf.
 *   THE FORCED STEP IGNORES EVERY CONSTRAINT: eos alone, as in ABI 32 -- a departure from fairseq, the only way the length
 *   cap and a ban on eos both hold.  Rules B and C, the records, the history and the host's backtracking are ABI 32's.
 * Not built: prefix_tokens (the prompt is prefilled), match_source_len (no encoder), unk_penalty.
 * LAUNCHES: the unconstrained entry's, one more (the ban list), and the constrained instance of the row kernel:
 *   ea_beam_bans, one wave per row of a sentence that is not done.  gen int32 [2, M, max_new] holds the beams' generated tokens
 *   row-major, a ping-pong pair: at t >= 1 row m copies gen[(t - 1) & 1][s W + hist_par[t - 1, m]][0 .. t - 1) into
 *   gen[t & 1][m] and appends hist_tok[t - 1, m] (what the previous merge wrote); nobody walks hist_par back t steps.  In the
 *   same pass it writes the row's banned tokens into ban[m, 0 .. nban[m]) (int32 [M, cap], cap >= prompt_cap + max_new + 17;
 *   duplicates allowed; the static bans, eos, then the n-gram bans by window position): every window yields at most one
 *   entry, so the list cannot overflow.  The forced step writes nban[m] = 0.  prompt_tok int32 [S, prompt_cap], prompt_len
 *   int32 [S] (clamped to 0 .. prompt_cap; both unread at prompt_cap = 0).  A workgroup writes its own row of buffer t & 1
 *   and of ban / nban alone and reads buffer (t - 1) & 1: no atomics on memory, no workgroup waits for another, the list's
 *   order is fixed: bitwise reproducible.  gen need not be cleared: entries from t on are never read.
 *   Plain head (ea_ceva_sdecode_vocab_beam_c): launch A with the list applied behind lse[m] and ahead of the selection: -inf
 *   is stored into logits[m, v] for every listed v < V, then every such v's tile candidate is formed again, the best of the
 *   tile's stored logits below V under the pick's order.  AFTER THE CALL logits [M, ldl] HOLDS -inf AT THE BANNED COLUMNS of
 *   the rows of live sentences (not on the forced step).
 *   Adaptive head (ea_adaptive_beam_c): launch 5 of ABI 35 with the listed tokens that fall in band b applied to that band's
 *   stored logits and tile candidates, behind the band's fold; class columns are never banned; launch 6 re-reads the stored
 *   logits, so a banned pick scores -inf there.  ea_adaptive_sample and the unconstrained entries launch what they launched.
 * ARGUMENTS: the unconstrained entry's, then min_len, ngram, ban_tokens (host, NULL at n_ban_tokens = 0), n_ban_tokens,
 * prompt_tok, prompt_cap, prompt_len, gen.  ws: the unconstrained entry's workspace from byte 0, then ban r16(4 M cap) and nban
 * r16(4 M), cap = prompt_cap + max_new + 17: the _c_ws queries; < 0 where the unconstrained query is, and for prompt_cap < 0 or
 * max_new < 1.  The ban list can later serve the greedy and the sampled pick too: it is a launch of its own.
 * EA_E_BADARG: what the unconstrained entry answers with it; min_len outside 0 .. max_new - 1; ngram outside 0 .. 16;
 * n_ban_tokens outside 0 .. 16, a static ban outside [0, V) (ea_beam_bans: < 0) or equal to eos; prompt_cap < 0; prompt_tok or
 * prompt_len NULL at prompt_cap > 0; gen NULL; one of them not 4-byte aligned; ea_beam_bans: cap below prompt_cap + max_new + 17,
 * S < 1, W < 1, eos < 0, a NULL or misaligned pointer.  EA_E_UNSUPPORTED: the unconstrained entry's refusals.  Bad arguments
 * are decided before the geometry, everything before any launch.  prompt_len[s] <= prompt_cap is the caller's promise; the
 * kernel clamps it. */
int ea_beam_bans(int32_t S, int32_t W, int32_t eos, int32_t max_new, int32_t min_len, int32_t ngram, const int32_t* ban_tokens,
                 int32_t n_ban_tokens, const int32_t* prompt_tok, int32_t prompt_cap, const int32_t* prompt_len,
                 const int32_t* t, const int32_t* done, const int32_t* hist_tok, const int32_t* hist_par, int32_t* gen,
                 int32_t* ban, int32_t cap, int32_t* nban, void* stream);
int64_t ea_ceva_sdecode_vocab_beam_c_ws(int32_t M, int32_t V, int32_t W, int32_t prompt_cap, int32_t max_new);
int ea_ceva_sdecode_vocab_beam_c(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                 const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws, int64_t ws_bytes,
                                 int32_t W, int32_t eos, int32_t max_new, float* score, int32_t* t, int32_t* nfin,
                                 int32_t* done, int64_t* token, int64_t* parent, int32_t* hist_tok, int32_t* hist_par,
                                 float* fin_score, int32_t* fin_len, int32_t* fin_beam, int32_t* cand_idx, float* cand_score,
                                 float* lse, float* sel_val, int32_t min_len, int32_t ngram, const int32_t* ban_tokens,
                                 int32_t n_ban_tokens, const int32_t* prompt_tok, int32_t prompt_cap,
                                 const int32_t* prompt_len, int32_t* gen, void* stream);
int64_t ea_adaptive_beam_c_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, int32_t W,
                              int32_t prompt_cap, int32_t max_new);
int ea_adaptive_beam_c(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                       int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype, const void* const* proj,
                       const void* const* tables, void* ws, int64_t ws_bytes, int32_t W, int32_t eos, int32_t max_new,
                       float* score, int32_t* t, int32_t* nfin, int32_t* done, int64_t* token, int64_t* parent,
                       int32_t* hist_tok, int32_t* hist_par, float* fin_score, int32_t* fin_len, int32_t* fin_beam,
                       int32_t* cand_idx, float* cand_score, int32_t min_len, int32_t ngram, const int32_t* ban_tokens,
                       int32_t n_ban_tokens, const int32_t* prompt_tok, int32_t prompt_cap, const int32_t* prompt_len,
                       int32_t* gen, void* stream);

/* ABI 38, THE VOCABULARY CROSS-ENTROPY'S BACKWARD (ea_harness.vocab_loss.vocab_nll, DecoderStack.loss; ea_vocab_nll.hip): the
 * gradient of logp[m] = logit[m, t_m] - lse[m], ea_vocab_score's result on a plain [V, K] table, without a [M, V] tensor.
 * Nothing is fused (a dX or dW tile of 128 rows by K = 1024 would be 512 KB of fp32 accumulators): the logit gradient is
 * materialised in 16 bits one column CHUNK at a time and two plain GEMMs per chunk contract over it.  E is w_dtype.
 * ea_vocab_nll_grad, one launch: for the table rows [v0, v0 + Vc) and all M rows of x the tile loop of ea_vocab_score forms
 * the logits a[m, v] again -- the same k order per accumulator: the bits ea_vocab_score stores with fp32 logits -- and writes
 *   G[m, v] = E( d[m] * ((v == targets[m]) - expf(a[m, v] - lse[m])) )      every operation in fp32, one rounding to E
 * as g [M, ldg] (G[m, v0 + c] at g[m * ldg + c]) and as its transpose gt [Vc, ldm] (at gt[c * ldm + m]).  A row with
 * d[m] == 0 is exact zeros, by a select: its logits and lse may be anything, NaN included.  A target outside [0, V) has no
 * (v == target) term.  Columns Vc .. ldg - 1 of g and columns M .. ldm - 1 of gt are WRITTEN as zeros: the GEMMs below
 * contract over them.  x, w (the WHOLE table, [V, K] row-major), targets as in ea_vocab_score; lse, d: fp32 [M].  A row's values
 * do not depend on the rows beside it, on M or on the chunking.  Ordinary vector stores, no atomics, no workgroup waits for
 * another, every element written once: bitwise reproducible.
 * EA_E_BADARG: x, w, targets, lse, d, g, gt NULL; x, w, g or gt not 16-byte aligned, targets not 8-byte, lse or d not 4-byte
 * aligned; the dtype rules and the stride rules of ea_vocab_score for x and w; M < 1, K < 1; v0 < 0, Vc < 1, v0 + Vc > V
 * (with V >= 1), v0 no multiple of EA_VOCAB_SCORE_SL; ldg < Vc, ldm < M, ldg or ldm no multiple of 64.  EA_E_UNSUPPORTED:
 * K % 32 != 0, V < 1, more than 2^23 workgroups (ceil(M / BM) ceil(Vc / SL)).  Bad arguments first, all before the launch.
 * ea_gemm_nt16, one launch, the same tile loop as a plain GEMM:  out[m, n] (+)= sum_k a[m, k] b[n, k], fp32 sums of exact
 * products; a [M, lda] and b [N, ldb] of dtype = EA_BF16 | EA_F16, out [M, ldo] fp32; accumulate = 0 stores (out is not
 * read: NaNs in it are gone), 1 reads, adds once and stores.  Per chunk of the backward:
 *   dX += G_c W_c         a = g [M, ldg],   b = W_c^T [K, ldg] (pad columns zeros), contracting over ldg, accumulate
 *   dW[v0 ..] = G_c^T X   a = gt [Vc, ldm], b = X^T [K, ldm] (pad columns zeros), contracting over ldm, a plain store
 * EA_E_BADARG: a, b, out NULL; a or b not 16-byte aligned, out not 4-byte aligned; dtype not a 16-bit type; M, N, K < 1;
 * lda < K, ldb < K, ldo < N; lda or ldb no multiple of 8 elements; accumulate outside {0, 1}.  EA_E_UNSUPPORTED: K % 32 != 0,
 * more than 2^23 workgroups (ceil(M / BM) ceil(N / BN)).
 * ea_vocab_nll_ws(M, K, V, chunk_cols): the bytes a backward holds beyond its outputs, with Vc = min(chunk_cols, V),
 * ldg = up64(Vc), ldm = up64(M):   2 (M ldg + Vc ldm + K ldg + K ldm)
 * -- g, gt, W_c^T, X^T.  (The gradients are outputs and not counted; 16-bit rows get their gradient through an fp32 [M, K]
 * accumulator, which the caller counts with them.)
 * It does not grow with M V.  chunk_cols: a multiple of EA_VOCAB_SCORE_SL, or 0: ea_vocab_nll_chunk(M, V), the largest
 * such width at which g and gt fit EA_VOCAB_NLL_BUDGET bytes, never below one slice and never beyond V rounded up to slices.
 * < 0: M, K or V < 1, chunk_cols negative or no multiple of the slice, a grid beyond 2^23 workgroups. */
#define EA_VOCAB_NLL_BUDGET 268435456 /* 256 MiB: a guess; no chunk width has been measured against another */
int32_t ea_vocab_nll_chunk(int32_t M, int32_t V);
int64_t ea_vocab_nll_ws(int32_t M, int32_t K, int32_t V, int32_t chunk_cols);
int ea_vocab_nll_grad(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                      int32_t w_dtype, const int64_t* targets, const float* lse, const float* d, int32_t v0, int32_t Vc,
                      void* g, int64_t ldg, void* gt, int64_t ldm, void* stream);
int ea_gemm_nt16(int32_t M, int32_t N, int32_t K, const void* a, int64_t lda, const void* b, int64_t ldb, int32_t dtype,
                 float* out, int64_t ldo, int32_t accumulate, void* stream);

/* ADDITIONS TO ABI 38, THE ADAPTIVE-SOFTMAX TRAINING LOSS (ea_harness.adaptive_loss.adaptive_nll, DecoderStack.adaptive_loss;
 * ea_adaptive_nll.hip).  No existing signature changes, so the ABI number stays 38: the entries below are additions.
 * The forward is ea_adaptive_score (or ea_adaptive_score_masked) and its workspace is kept: head_target, rows, count, lse_head,
 * h_i and lse_i are read out of it (the layout above).  With d = dlogp (fp32 [M]):
 *   head, every row:  ea_vocab_nll's chunk loop on the head table [c0 + n, C] with head_target and lse_head: dX, d head.
 *   tail i, positions j < count_i:  G_i[j, u] = d[rows_i[j]] ((u == t - c_i) - exp(b_i[j, u] - lse_i[j]));  dE_i = G_i^T h_i;
 *   dh_i = G_i E_i (fp32, summed over the chunks in table order);  dQ_i = dh_i^T x[rows_i];  dX[rows_i] += dh_i Q_i.
 * The rounding of h_i passes the gradient straight through.  Launches per tail: ea_rows_transpose16 (h_i^T), per chunk
 * ea_vocab_nll_grad_rows, ea_gemm_nt16_rows (dh_i) and ea_gemm_nt16 (dE_i), then ea_rows_transpose16 (x[rows_i]^T), ea_gemm_nt16
 * (dQ_i) and ea_gemm_nt16_rows (dX).  Everything is sized for M positions per tail; the counts stay on the device.  Every
 * kernel: ordinary vector stores, no atomics, no workgroup waits for another, every output element written by one thread of
 * one launch: bitwise reproducible.
 *
 * ea_vocab_nll_grad_rows: ea_vocab_nll_grad over a device-counted set of M POSITIONS.  Its arguments, then trows (int32 [M] or
 * NULL: targets and d are read at trows[j]; x and lse are indexed by the position j, as in the tail pass of the scorer), count
 * (int32 device scalar or NULL: M; kept inside [0, M]) and target_base (>= 0, taken off a target before the range test).
 * Positions at or beyond *count: their rows of g (columns 0 .. ldg - 1) and their columns of gt are WRITTEN as zeros, also by
 * workgroups whose whole row tile is dead, which store zeros and load nothing.  Inside the last live tile a position >= *count
 * is clamped to *count - 1 before any list is read: a stale list entry is never dereferenced; *count == 0 reads nothing through
 * a list.  With trows = count = NULL and target_base = 0: ea_vocab_nll_grad's bits.
 * EA_E_BADARG: ea_vocab_nll_grad's; also trows or count not 4-byte aligned, target_base < 0.  EA_E_UNSUPPORTED: its own.
 *
 * ea_gemm_nt16_rows: ea_gemm_nt16 over M positions of which *count are live: out[orows[j], n] (+)= sum_k a[j, k] b[n, k] for
 * j < *count (orows int32 [M] or NULL: the identity; count NULL: M).  Positions at or beyond *count write nothing and read no
 * list entry; a workgroup whose tile is dead returns before its first load.  The rows named by orows must be distinct.
 * EA_E_BADARG: ea_gemm_nt16's; also orows or count not 4-byte aligned.  EA_E_UNSUPPORTED: its own.
 *
 * ea_rows_transpose16: out[k, j] = E(src[rows[j], k]) for j < *count and k < K, ZEROS for *count <= j < ldm: a 16-bit [K, ldm]
 * image (E = out_dtype) of rows of src [*, ld] (src_dtype = EA_F32, rounded to nearest even, or out_dtype), through an optional
 * int32 list (NULL: the identity) and an optional device count (NULL: M).  A row at or beyond the count is not read, whatever
 * it holds.  EA_E_BADARG: src or out NULL, src, rows or count not 4-byte, out not 2-byte aligned; out_dtype not 16-bit,
 * src_dtype neither EA_F32 nor out_dtype; M < 1, K < 1, ld < K, ldm < M, ldm no multiple of 64.  EA_E_UNSUPPORTED: K > 64 * 65535.
 *
 * ea_adaptive_score_masked: ea_adaptive_score plus hmask, a HOST array of n_tails entries: hmask[i] NULL or 16-bit multipliers
 * [M, d_i] of w_dtype, indexed by POSITION, 16-byte aligned.  A non-NULL entry adds one elementwise launch between the
 * projection and the tail pass of that band, h_i = E(fp32(h_i) * fp32(mask)) on the live positions -- the Dropout inside
 * fairseq's tail[i].  With every entry NULL it is ea_adaptive_score's code path and gives its bits.  EA_E_BADARG:
 * ea_adaptive_score's; also hmask NULL or an entry not 16-byte aligned.  EA_E_UNSUPPORTED: ea_adaptive_score's.
 *
 * ea_adaptive_nll_ws(M, C, n_tails, cutoffs, dims, chunk_cols): the bytes the backward holds beyond its outputs (the fp32
 * gradients) and the saved workspace, with ldm = up64(M), V_i = c_{i+1} - c_i:
 *   max(ea_vocab_nll_ws(M, C, c0 + n_tails, chunk_cols), max_i ea_vocab_nll_ws(M, d_i, V_i, chunk_cols))
 *   + 2 C ldm + max_i (6 M d_i + 2 d_i ldm + 2 C d_i)
 * -- the largest chunk pass (g, gt, the chunk's transposed table, and X^T or h_i^T), x[rows_i]^T, and of the largest tail dh_i
 * in fp32, dh_i in 16 bits, its transpose and Q_i^T.  It does not grow with M V.  chunk_cols as in ea_vocab_nll_ws (0: each
 * pass's default).  < 0: M < 1, C < 1, n_tails outside 1 .. EA_ADAPTIVE_MAX_TAILS, cutoffs not increasing, c0 < 1, V >= 2^31,
 * d_i < 1, or a pass ea_vocab_nll_ws refuses.  A host-known cap on the rows per tail would shrink it; there is none. */
int64_t ea_adaptive_nll_ws(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims,
                           int32_t chunk_cols);
int ea_vocab_nll_grad_rows(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                           int32_t w_dtype, const int64_t* targets, const float* lse, const float* d, int32_t v0, int32_t Vc,
                           void* g, int64_t ldg, void* gt, int64_t ldm, const int32_t* trows, const int32_t* count,
                           int64_t target_base, void* stream);
int ea_gemm_nt16_rows(int32_t M, int32_t N, int32_t K, const void* a, int64_t lda, const void* b, int64_t ldb, int32_t dtype,
                      float* out, int64_t ldo, int32_t accumulate, const int32_t* orows, const int32_t* count, void* stream);
int ea_rows_transpose16(int32_t M, int32_t K, const void* src, int32_t src_dtype, int64_t ld, const int32_t* rows,
                        const int32_t* count, void* out, int32_t out_dtype, int64_t ldm, void* stream);
int ea_adaptive_score_masked(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                             int32_t x_dtype, int64_t ldx, const int64_t* targets, const void* head, int32_t w_dtype,
                             const void* const* proj, const void* const* tables, const void* const* hmask, void* ws,
                             int64_t ws_bytes, float* logp, int64_t* token_head, void* stream);

/* ADDITIONS TO ABI 38, THE 192 -> 192 PROJECTION WITH ITS WEIGHT IN REGISTERS (ea_linear_rs192.hip).  No existing signature
 * changes, so the ABI number stays 38: the two entries below are additions.
 *
 * ea_linear_rs192: Y[t][o] = sum_k A[t][k] W[o][k] (+ bias[o]) for K = out = 192, `rows` rows, A and Y in the EA dtype (bf16 /
 * fp16) with row strides lda / ldy elements, `image` = the weight in the kernel's register order (below), bias fp32 [192] or
 * NULL (rounded to the EA dtype before it is added, the sum rounded once).  One 12-wave workgroup per CU keeps the weight in
 * registers for the whole launch and streams the rows through LDS once.  Y has the bits ea_linear gives on the same operands
 * (its MFMA, its k-slots, its order of accumulation, its rounding of the bias).
 *   image: 4608 pieces of 16 bytes; piece ((pair * 2 + j) * 6 + ks) * 64 + lane, with lane = 16 g + li, pair 0 .. 5, j 0 .. 1,
 *   ks 0 .. 5, holds W[32 pair + 8 (li >> 2) + (li & 3) + 4 j][32 ks + 8 g .. 32 ks + 8 g + 7].
 * rows <= 0: EA_OK, nothing launched.  EA_E_BADARG: dtype not 16-bit; a, image or y NULL.  EA_E_UNSUPPORTED, before any launch:
 * a, image, y or bias not 16-byte aligned; lda or ldy below 192 or no multiple of 8; rows above 2^30 or rows * ld >= 2^40.
 *
 * ea_linear_w192_prepare_rs: ea_linear_w192_prepare_t (every pointer required, wp included) with two more images from the SAME
 * launch, 192 * 192 elements each: wp_rs = W_proj (the bits of w16p) and wpT_rs = W_proj^T (the bits of w16pT) in
 * ea_linear_rs192's image order -- the output projection and its input gradient.  EA_E_BADARG: a NULL or misaligned pointer. */
int ea_linear_rs192(int32_t dtype, const void* a, int64_t lda, const void* image, const float* bias, void* y, int64_t ldy,
                    int32_t rows, void* stream);
int ea_linear_w192_prepare_rs(int32_t dtype, const float* wq, const float* wp, void* w16q, void* wq_sw, void* w16p, void* w16pT,
                              void* wqT_sw, void* wp_rs, void* wpT_rs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EA_HIP_H */
