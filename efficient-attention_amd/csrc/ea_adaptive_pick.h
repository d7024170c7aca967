// ea_adaptive_pick.h -- the greedy pick with its log-probability from a held adaptive softmax (ABI 34), and the sampled pick
// and the beam step from it (ABI 35): the plans of the workspaces and the composite calls (ea_adaptive_pick.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "ea_adaptive_score.h"
#include "ea_ceva_decode_vocab.h"

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

// ---- the k best joint log-probabilities of a row (ABI 35) -----------------------------------------------------------------
constexpr int ASEL_MAX_K = VOC_SAMPLE_MAX_K;           // a band's list, and the joint selection: one wave sorts it

// ea_adaptive_sample's and ea_adaptive_beam's workspace: ea_adaptive_pick's for the same (M, n, cut, dims) from byte 0 (`pick`),
// then what the selection adds
struct AdaptiveSelectPlan {
  AdaptivePickPlan pick;
  int64_t logits[AS_MAX_TAILS + 1];                    // fp32 [M][V_b]: every band's raw logits
  int64_t tcand[AS_MAX_TAILS];                         // (value, index) [M][ceil(V_i / 16)], tails of the column-split kernel (else -1)
  int64_t list_idx, list_val;                          // int32, fp32 [M][n + 1][ASEL_MAX_K]: a band's best columns and logits
  int64_t cand_idx, cand_score;                        // int32, fp32 [M][2 W]: the beam step's (W = 0: -1)
  int64_t total;
};

// the draw of ea_adaptive_sample, or (W > 0) the beam step's state; exactly one of the two tails runs
struct AdaptiveJointArgs {
  // sampled
  int top_k;
  float top_p, temperature;
  uint32_t seed_lo, seed_hi;
  int64_t* ctr;               // [M]
  const int32_t* sid;         // [M]
  int64_t* token;             // [M]
  float* logp;                // [M]
  int32_t* sel_idx;           // [M, top_k] or null
  float* sel_val;             // [M, top_k] or null
  int32_t* kept;              // [M] or null
  // beam: the merge's block (cand_idx, cand_score null: the workspace's)
  DecBeamP beam;
  int W;                      // 0: sampled
};

// the layout for (M, n, cut, dims, W) (W = 0: the sampled pick's) -> total bytes, or < 0 outside the envelope
int64_t adaptive_select_plan(int M, int n, const int64_t* cut, const int32_t* dims, int W, AdaptiveSelectPlan* plan);
// the band passes with their logits kept, the select and the joint launch; beam: then the merge.  p.targets is not read.
// The caller has checked the arguments.
// bans (ABI 36, the beam step alone; or null): ceva_beam_bans on it ahead of the select launch, which then applies the list.
int adaptive_select(const AdaptivePickP& p, const AdaptiveJointArgs& j, hipStream_t st, const BeamBanP* bans = nullptr);

}  // namespace ea
