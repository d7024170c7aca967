// ea_adaptive_score.h -- adaptive-softmax scoring (ABI 33): the routing of targets to bands, the many-row vocabulary pass
// over a gathered, device-counted row set, and the composite score (ea_adaptive_score.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "ea_vocab_score.h"

namespace ea {

constexpr int AS_MAX_TAILS = EA_ADAPTIVE_MAX_TAILS;

// cut[0 .. n]: c0 < c1 < .. < c_n = V; tail i is [cut[i], cut[i + 1])
struct AdaptiveRouteP {
  const int64_t* targets;     // [M]
  int64_t* head_target;       // [M]: t (head), c0 + i (tail i), -1 (outside [0, V))
  int32_t* rows;              // [n][M]: rows[i][0 .. count[i]) the rows of tail i, ascending
  int32_t* count;             // [n]
  int64_t cut[AS_MAX_TAILS + 1];
  int M, n;
};

// where the parts of ea_adaptive_score's workspace lie (bytes from its start; include/ea_hip.h documents the layout)
struct AdaptivePlan {
  int64_t head_target, rows, count, token_head, lse_head, logp_head;
  int64_t h[AS_MAX_TAILS], token[AS_MAX_TAILS], lse[AS_MAX_TAILS], logp[AS_MAX_TAILS];
  int64_t inner, inner_bytes, total;
};

struct AdaptiveScoreP {
  const char* x;              // [M, ldx] fp32 or the tables' type
  const int64_t* targets;     // [M]
  const char* head;           // [c0 + n, C]
  const char* proj[AS_MAX_TAILS];    // [d_i, C]
  const char* table[AS_MAX_TAILS];   // [V_i, d_i]
  const char* hmask[AS_MAX_TAILS];   // [M, d_i] 16-bit multipliers by position, or null (ea_adaptive_score_masked): h_i = E(h_i mask)
  char* ws;
  float* logp;                // [M]
  int64_t* token_head;        // [M] or null
  int64_t ldx;
  int64_t cut[AS_MAX_TAILS + 1];
  int dims[AS_MAX_TAILS];
  int M, C, n, dtype, x_f32;
};

// one launch; the caller has checked the arguments
int adaptive_route(const AdaptiveRouteP& p, hipStream_t st);
// the two launches of ea_vocab_score on a row set (logits_only: the first alone); ws = pick as in vocab_score
int vocab_score_rows(VocabScoreRowsP p, hipStream_t st);
// the layout for (M, n, cut, dims) -> total bytes, or < 0 outside the envelope (of the route or of an inner pass)
int64_t adaptive_plan(int M, int n, const int64_t* cut, const int32_t* dims, AdaptivePlan* plan);
int adaptive_score(const AdaptiveScoreP& p, hipStream_t st);

}  // namespace ea
