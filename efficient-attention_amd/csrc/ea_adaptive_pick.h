// ea_adaptive_pick.h -- the greedy pick with its log-probability from a held adaptive softmax (ABI 34): the plan of the
// workspace and the composite call (ea_adaptive_pick.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "ea_adaptive_score.h"

namespace ea {

constexpr int AP_MAX_ROWS = 64;                        // a decoding step's rows: EA_CEVA_LINEAR_MAX_ROWS
constexpr int AP_WAVES = 8;                            // waves of a tail workgroup
constexpr int AP_TPW = EA_ADAPTIVE_PICK_SPAN / (16 * AP_WAVES);   // 16-column tiles a wave walks
constexpr int AP_SPAN = EA_ADAPTIVE_PICK_SPAN;         // columns of one tail workgroup: one partial per row
constexpr int AP_MAX_K = EA_ADAPTIVE_PICK_MAX_K;       // the widest tail of the column-split kernel
static_assert(AP_TPW >= 1 && AP_TPW * 16 * AP_WAVES == AP_SPAN, "a span is whole tiles of whole waves");

// where the parts of ea_adaptive_pick's workspace lie (bytes from its start; include/ea_hip.h documents the layout)
struct AdaptivePickPlan {
  int64_t cls, h;                                      // fp32 [M][n]; 16-bit [M][D], D = sum d_i
  int64_t best[AS_MAX_TAILS + 1], lse[AS_MAX_TAILS + 1], tlogit[AS_MAX_TAILS + 1];   // band 0 = the head's words
  int64_t shifted[AS_MAX_TAILS];                       // int64 [M], tails wider than AP_MAX_K alone (else -1)
  int64_t cand[AS_MAX_TAILS + 1], sum[AS_MAX_TAILS + 1];   // the passes' partials [M][parts[b]]
  int64_t cls_cand, cls_sum;                           // the class pass's one partial per row
  int32_t parts[AS_MAX_TAILS + 1];
  int32_t D;
  int64_t total;
};

struct AdaptivePickP {
  const char* x;              // [M, ldx] fp32 or the tables' type
  const int64_t* targets;     // [M] or null
  const char* head;           // [c0 + n, C]
  const char* proj[AS_MAX_TAILS];    // [d_i, C]
  const char* table[AS_MAX_TAILS];   // [V_i, d_i]
  char* ws;
  int64_t* token;             // [M]
  float* logp;                // [M]
  int64_t ldx;
  int64_t cut[AS_MAX_TAILS + 1];
  int dims[AS_MAX_TAILS];
  int M, C, n, dtype, x_f32;
};

// the layout for (M, n, cut, dims) -> total bytes, or < 0 outside the envelope
int64_t adaptive_pick_plan(int M, int n, const int64_t* cut, const int32_t* dims, AdaptivePickPlan* plan);
// the caller has checked the arguments
int adaptive_pick(const AdaptivePickP& p, hipStream_t st);

}  // namespace ea
