// ea_vocab_score.hip -- the many-row vocabulary pass (ABI 30): token, top logit, log-sum-exp and a log-probability per row
// of x against a 16-bit vocabulary table, for thousands of rows, without a [rows, V] tensor
//
//   logit[m, v] = sum_k round_w(x[m, k]) w[v, k]            fp32, no bias;  any M >= 1, w [V, K] 16-bit row-major, K % 32 == 0
//   token[m]    = argmax_v logit[m, v], top[m] its value    torch.argmax's rule: equal values: the lowest index; NaN wins
//   lse[m]      = log sum_v exp(logit[m, v])                 by cases on top: NaN, +inf, -inf stay; else top + logf(S)
//   logp[m]     = logit[m, targets[m]] - lse[m]              (no targets: top[m] - lse[m])
//
// The few-row entries (ea_ceva_decode_vocab.hip) stream the whole table for at most 64 rows: bound by 2 V K bytes per call.
// With M in the thousands the work is a GEMM, M x V x K, and both operands are K-contiguous: a lane's eight k of a row of x
// (the MFMA's A operand) and of a row of w (its B operand) are one 16-byte piece of a row, so tiles go through LDS as they
// lie in memory and no transposed read is needed.
//
// Launch one, vocab_score_kernel: workgroup (slice t, row tile) owns VS_BM = 128 rows of x and the VS_SL = 2048 columns
// t VS_SL .. of the table.  It walks the slice in column blocks of VS_BN = 128 and K in stages of VS_BK = 64: eight waves, 4 x 2,
// each a 32 x 64 accumulator acc[2][4] of v_mfma_f32_16x16x32 (with four waves of 64 x 64 the running state of 16 rows per
// lane beside 64 accumulator registers did not fit 256 VGPRs).  A stage is two tiles [128][64] of 16-bit, 128-byte rows whose
// 16-byte chunks are swizzled by psi (ea_lds_swizzle.h: conflict-free for chunk 4 ks + g of row li); the next stage's global
// loads are issued before the MFMAs of this one and stored to the other LDS buffer behind them: one barrier per stage.  fp32
// rows of x are rounded to the table's type as they are stored to LDS.  Rows >= M and table rows >= V are read as row M - 1 /
// the slice's last row (never beyond the allocations); k >= K of the last stage is a zero operand.
// Behind a block's last stage a lane holds, of each of its 8 rows, the four columns 16 j + li of its wave's half: it folds
// them into the row's running (best value, best index, sum of exp(logit - best value)) -- its OWN columns' only, in
// registers, across the blocks of the slice.  A column >= V is -inf with no index: it takes no part.  The sum is rescaled
// only when the best value rises (the factor is exactly 1 otherwise).  The target's logit is stored by the lane that holds it.
// After the slice's last block the 16 lanes of a row merge (xor butterfly 8, 4, 2, 1: the best pair, each lane's sum rescaled
// once to it, the sums added), then the wave pair through LDS, and one partial per (row, slice) goes to ws.
// Launch two, vocab_score_fold_kernel: one thread per row folds the row's slices in slice order.
//
// The order of summation is this kernel's own: the logits need not have the few-row entries' bits.  Slice and block widths
// are compile-time constants, so the partition of the columns depends on V alone: a row's results do not depend on M, on the
// rows beside it or on its place in the batch.  Ordinary vector stores only; no atomics; no workgroup waits for another.
//
// The two kernels are templates in ea_vocab_score_tile.h, shared with the gathered, device-counted pass of
// ea_adaptive_score.hip; this file instantiates them with ROWS = false: the kernels of ABI 30, on a VocabScoreP.
#include "ea_vocab_score_tile.h"

namespace ea {

int64_t vocab_score_ws(int M, int V) {
  if (M < 1 || V < 1) return -1;
  const int64_t MT = ((int64_t)M - 1) / VS_BM + 1, NS = ((int64_t)V - 1) / VS_SL + 1;
  if (MT * NS > VS_MAX_WORKGROUPS) return -1;
  const int64_t bytes = (int64_t)M * NS * (int64_t)(sizeof(VsPick) + sizeof(float)) + (int64_t)M * (int64_t)sizeof(float);
  return (bytes + 15) / 16 * 16;
}

// (Every argument has been checked by the one caller, ea_vocab_score in ea_capi.hip: nothing is checked again here.)
int vocab_score(VocabScoreP p, hipStream_t st) {
  p.MT = (p.M - 1) / VS_BM + 1;
  p.NS = (p.V - 1) / VS_SL + 1;
  p.sum = reinterpret_cast<float*>(p.pick + (int64_t)p.M * p.NS);
  p.tlogit = p.sum + (int64_t)p.M * p.NS;
  if (const int rc = vs_launch_typed<false>(p, st)) return rc;
  return vs_launch_fold<false>(p, st);
}

}  // namespace ea
