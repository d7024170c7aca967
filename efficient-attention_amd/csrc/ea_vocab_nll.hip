// ea_vocab_nll.hip -- the backward of the vocabulary cross-entropy (ABI 38): logp[m] = logit[m, t_m] - lse[m] on a plain [V, K]
// table, whose forward is ea_vocab_score (ea_vocab_score.hip)
//
//   G[m, v] = E( d_m ((v == t_m) - expf(a[m, v] - lse_m)) )      a: the fp32 logit as ea_vocab_score forms it, E: the table's type
//   dX      = G W            [M, K]
//   dW      = G^T X          [V, K]
//
// A dX or dW tile of 128 rows by K = 1024 is 512 KB of fp32 accumulators, and a logit tile costs a full K loop, so nothing is
// fused: G is materialised in 16 bits one column CHUNK at a time (a whole number of slices), in a workspace of fixed budget,
// and two plain GEMMs per chunk contract over it.  Per chunk [v0, v0 + Vc):
//   ea_vocab_nll_grad   the tile loop of ea_vocab_score_tile.h with the VS_EPI_GRAD epilogue: G_c [M, ldg] and G_c^T [Vc, ldm]
//   ea_gemm_nt16        dX (+)= G_c (W_c^T)^T     a = G_c, b = W_c^T [K, ldg], contracting over ldg (pad columns: zeros)
//   ea_gemm_nt16        dW[v0 ..] = G_c^T (X^T)^T  a = G_c^T, b = X^T [K, ldm], contracting over ldm (pad columns: zeros)
// Both GEMMs are the same tile loop with the VS_EPI_GEMM epilogue (out = or out += in fp32): K-contiguous operands on both
// sides, which is why the two transposed 16-bit images exist.  Ordinary vector stores only; no atomics; no workgroup waits
// for another; every output element is written by one thread of one launch: bitwise reproducible.
#include "ea_vocab_score_tile.h"

namespace ea {
namespace {

int64_t up64(int64_t n) { return (n + 63) / 64 * 64; }

}  // namespace

int vocab_nll_chunk(int M, int V) {
  if (M < 1 || V < 1) return -1;
  const int64_t per_col = 2 * ((int64_t)M + up64(M));                 // bytes of one column of G and one row of G^T
  int64_t cc = EA_VOCAB_NLL_BUDGET / per_col / VS_SL * VS_SL;
  const int64_t whole = ((int64_t)V + VS_SL - 1) / VS_SL * VS_SL;
  if (cc > whole) cc = whole;
  if (cc < VS_SL) cc = VS_SL;                                         // never below one slice
  return (int)cc;
}

int64_t vocab_nll_ws(int M, int K, int V, int chunk_cols) {
  if (M < 1 || K < 1 || V < 1 || chunk_cols < 0 || chunk_cols % VS_SL) return -1;
  if (chunk_cols == 0) chunk_cols = vocab_nll_chunk(M, V);
  const int64_t Vc = chunk_cols < V ? chunk_cols : V, ldg = up64(Vc), ldm = up64(M);
  const int64_t MT = ((int64_t)M - 1) / VS_BM + 1, NS = (Vc - 1) / VS_SL + 1;
  if (MT * NS > VS_MAX_WORKGROUPS || MT * (((int64_t)K - 1) / VS_BN + 1) > VS_MAX_WORKGROUPS) return -1;
  return 2 * ((int64_t)M * ldg + Vc * ldm + (int64_t)K * ldg + (int64_t)K * ldm);
}

int vocab_nll_grad(VocabNllGradP p, hipStream_t st) {
  p.MT = (p.M - 1) / VS_BM + 1;
  p.NS = (p.Vc - 1) / VS_SL + 1;
  if (p.dtype == EA_BF16)
    return p.x_f32 ? vs_launch<BF16, true, false, VS_EPI_GRAD>(p, st) : vs_launch<BF16, false, false, VS_EPI_GRAD>(p, st);
  return p.x_f32 ? vs_launch<F16, true, false, VS_EPI_GRAD>(p, st) : vs_launch<F16, false, false, VS_EPI_GRAD>(p, st);
}

int gemm_nt16(GemmNt16P p, hipStream_t st) {
  p.MT = (p.M - 1) / VS_BM + 1;
  p.NS = (p.V - 1) / VS_BN + 1;                                       // (a "slice" of this instance is one column block)
  return p.dtype == EA_BF16 ? vs_launch<BF16, false, false, VS_EPI_GEMM>(p, st) : vs_launch<F16, false, false, VS_EPI_GEMM>(p, st);
}

}  // namespace ea
