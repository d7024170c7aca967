// ea_vocab_score.h -- the many-row vocabulary pass (ABI 30): tile constants, workspace layout and parameter block
// (ea_vocab_score.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/ea_hip.h"

namespace ea {

constexpr int VS_BM = EA_VOCAB_SCORE_BM;   // rows of x of one workgroup
constexpr int VS_BN = EA_VOCAB_SCORE_BN;   // columns of one column block: the accumulator tile is VS_BM x VS_BN
constexpr int VS_BK = 64;                  // k of one LDS stage: 128-byte tile rows, two MFMA k-steps
constexpr int VS_SL = EA_VOCAB_SCORE_SL;   // columns of one slice: VS_SL / VS_BN column blocks fold into one partial per row
constexpr int64_t VS_MAX_WORKGROUPS = (int64_t)1 << 23;   // row tiles x slices of the first launch: 2^31 threads

// one candidate of a row and slice: the largest fp32 sum and its column (the layout of ea_ceva_decode_vocab.h's VocPick)
struct alignas(8) VsPick {
  float v;
  int32_t i;
};

// ws, for NS = ceil(V / VS_SL) slices:  VsPick pick[NS][M] | float sum[NS][M] | float tlogit[M]
//   pick[t][m]  the best (value, index) of row m in slice t
//   sum[t][m]   sum over the slice's columns of exp(logit - pick[t][m].v)
//   tlogit[m]   logit[m, targets[m]], written by the one thread that holds it (a target outside [0, V): by nobody)
struct VocabScoreP {
  const char* x;              // [M, ldx] rows, fp32 or the table's type
  const char* w;              // [V, K] row-major 16-bit table
  const int64_t* targets;     // [M], or null
  char* logits;               // [M, ldl] rows, fp32 or the table's type, or null: nothing is stored
  VsPick* pick;               // ws
  float* sum;
  float* tlogit;
  int64_t* token;             // [M]
  float* top;                 // [M], or null
  float* lse;                 // [M]
  float* logp;                // [M]
  int64_t ldx, ldl;           // row strides in elements
  int M, K, V;                // M >= 1, K % 32 == 0, V >= 1
  int MT, NS;                 // row tiles, slices
  int dtype;                  // EA_BF16 | EA_F16: w
  int x_f32, l_f32;           // 1: fp32 rows (x is rounded to `dtype` on load)
};

// the same pass over a gathered, device-counted set of rows (ABI 33, ea_adaptive_score.hip): M is the number of POSITIONS the
// grid and ws are sized for; position j < live reads row xrows[j] of x and targets[trows[j]] and writes results j
struct VocabScoreRowsP : VocabScoreP {
  const int32_t* xrows;       // [M] rows of x, or null: the identity
  const int32_t* trows;       // [M] entries of targets, or null: the identity
  const int32_t* count;       // device scalar, the live positions (kept inside [0, M]), or null: M
  int64_t target_base;        // >= 0, taken off a target before the range test against [0, V)
  int logits_only;            // 1: the first launch alone, without pick, sums and target logits: a GEMM into `logits`
};

// the logit gradient of a column chunk (ABI 38, ea_vocab_nll.hip): of the base block x, w (the WHOLE table), targets, ldx, M, K,
// V, dtype and x_f32 are read; MT row tiles, NS slices of the chunk
struct VocabNllGradP : VocabScoreP {
  const float* lse_in;        // [M] the rows' log-sum-exp, as ea_vocab_score wrote it
  const float* d;             // [M] dL / dlogp
  uint16_t* g;                // [M, ldg]: G of the chunk; columns Vc .. ldg - 1 are written as zeros
  uint16_t* gt;               // [Vc, ldm]: its transpose; columns M .. ldm - 1 are written as zeros
  int64_t ldg, ldm;           // multiples of 64, ldg >= Vc, ldm >= M
  int v0, Vc;                 // the chunk: table rows [v0, v0 + Vc), v0 % VS_SL == 0
};

// out (+)= a b^T (ABI 38, ea_vocab_nll.hip): x = a [M, ldx], w = b [V, ldw], logits = out [M, ldl] fp32, K % 32 == 0
struct GemmNt16P : VocabScoreP {
  int64_t ldw;                // the row stride of b in elements
  int accumulate;             // 1: out += , 0: out =
};

// the same two over a device-counted set of POSITIONS (the adaptive-softmax loss, ea_adaptive_nll.hip): x and lse_in are indexed
// by position, targets and d through trows; positions >= live are written as zeros in g and gt (the GEMMs contract over them)
struct VocabNllGradRowsP : VocabScoreRowsP {
  const float* lse_in;        // [M] by position
  const float* d;             // read at trows[j]
  uint16_t* g;                // [M, ldg]
  uint16_t* gt;               // [Vc, ldm]
  int64_t ldg, ldm;
  int v0, Vc;
};

// out[orows[j], :] (+)= a[j, :] b^T for j < live; positions >= live write nothing and read no list entry
struct GemmNt16RowsP : VocabScoreRowsP {
  const int32_t* orows;       // [M] rows of out, or null: the identity
  int64_t ldw;
  int accumulate;
};

// out [K, ldm] 16-bit: out[k, j] = E(src[rows[j], k]) for j < live, zeros for live <= j < ldm
struct RowsTransposeP {
  const char* src;            // [*, ld] fp32 or 16-bit
  const int32_t* rows;        // [M] or null: the identity
  const int32_t* count;       // device scalar or null: M
  uint16_t* out;
  int64_t ld, ldm;
  int M, K, dtype, src_f32;
};

// h[j, :] = E(h[j, :] * mask[j, :]) for j < live, in fp32, one rounding (the Dropout inside an adaptive tail)
struct RowsMaskP {
  uint16_t* h;                // [M, D]
  const uint16_t* mask;       // [M, D]
  const int32_t* count;
  int M, D, dtype;
};

// bytes of ws for (M, V); < 0: outside the envelope (M < 1, V < 1, more than VS_MAX_WORKGROUPS workgroups)
int64_t vocab_score_ws(int M, int V);
// the two launches; the C entry point has checked pointers, alignment, strides, types and the size of ws
int vocab_score(VocabScoreP p, hipStream_t st);

// ABI 38 (ea_vocab_nll.hip).  The default chunk width for (M, V); the workspace of a backward; the two launches' entries,
// on arguments their C entry points have checked
int vocab_nll_chunk(int M, int V);
int64_t vocab_nll_ws(int M, int K, int V, int chunk_cols);
int vocab_nll_grad(VocabNllGradP p, hipStream_t st);
int gemm_nt16(GemmNt16P p, hipStream_t st);

// the adaptive-softmax loss (ea_adaptive_nll.hip), on arguments the C entry points have checked
int vocab_nll_grad_rows(VocabNllGradRowsP p, hipStream_t st);
int gemm_nt16_rows(GemmNt16RowsP p, hipStream_t st);
int rows_transpose16(const RowsTransposeP& p, hipStream_t st);
int rows_mask16(const RowsMaskP& p, hipStream_t st);
int64_t adaptive_nll_ws(int M, int C, int n, const int64_t* cut, const int32_t* dims, int chunk_cols);

}  // namespace ea
