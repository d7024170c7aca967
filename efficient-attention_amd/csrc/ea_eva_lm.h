// ea_eva_lm.h -- parameter block and launch plan of the dense landmark-column kernels of non-causal EVA (ea_eva_lm.hip):
// attention of N queries over all L landmark keys, joined with the window half through the two log-sum-exps.
#pragma once
#include <algorithm>
#include "ea_common.h"
#include "ea_t4.h"

namespace ea {

constexpr int ELM_TILE = 64;                      // queries per tile (4 waves x 16) / landmark rows per LDS tile
constexpr int ELM_MIN_L = 65, ELM_MAX_L = 8192;   // below: the window kernels hold the landmarks themselves
constexpr int ELM_MAX_N = 1 << 20;
constexpr int ELM_MAX_WALK = 8;                   // query tiles one workgroup of the query-side kernels walks at most
constexpr int ELM_MAX_SLICES = 32;                // query slices of the key-side backward
constexpr size_t ELM_LDS_RESIDENT = 128 * 1024;   // both landmark images stay in LDS up to this size (of 160 KB per CU)

struct EvaLmP {
  T4 q, oloc, out, dout, doloc;          // 16-bit [B,H,N,D] views
  const char *lk16, *lv16;               // 16-bit images [B*H, Lp, D] of rf_k_bar / beta, rows >= L zero
  const float *lk, *lv;                  // prepare: the fp32 masters [B*H, L, D]
  const float* lse_loc;                  // [B*H, N] log-sum-exp of the window half
  float* zl;                             // [B*H, N, 2] (joint lse Z, landmark lse)
  float* delta;                          // [B*H, N] rowsum(dout * out)
  float* dlse_loc;                       // [B*H, N]
  float* dq;                             // fp32 [B, N, H, D]: scale * dS . lk
  float *dlk, *dlv;                      // fp32 [S][B*H, L, D]: slice s of the key-side backward writes plane s
  int B, H, N, L, Lp, nQT, nLT;
  int walk, nWQ, resident;               // query side: tiles per workgroup, workgroups per (b, h), images stay in LDS
  int S, per;                            // key side: slices, query tiles per slice
  float scale, scale_log2;
};

// The query-side kernels (forward, query-side backward): a workgroup walks `walk` consecutive 64-query tiles of one (b, h).
// Where both landmark images fit ELM_LDS_RESIDENT they are loaded once per workgroup, so the walk is as long as still leaves
// two workgroups per CU (<= ELM_MAX_WALK), evened out over the (b, h)'s workgroups; streamed tiles gain nothing from a walk.
inline void elm_plan_query(EvaLmP& p, int D, int cus) {
  p.resident = (size_t)4 * p.Lp * D <= ELM_LDS_RESIDENT ? 1 : 0;
  int walk = 1;
  if (p.resident) {
    const long long tiles = (long long)p.B * p.H * p.nQT;
    walk = (int)std::min<long long>(std::max<long long>(tiles / (2LL * cus), 1), ELM_MAX_WALK);
  }
  p.nWQ = (p.nQT + walk - 1) / walk;
  p.walk = (p.nQT + p.nWQ - 1) / p.nWQ;
}
// The key-side backward: a workgroup owns (slice, b, h, 64-landmark tile) and streams its slice's query tiles.  S = slices that
// bring the grid to two workgroups per CU, at most ELM_MAX_SLICES and one per query tile; `forced` > 0 overrides the count.
inline void elm_plan_key(EvaLmP& p, int cus, int forced) {
  int S = forced;
  if (S <= 0) {
    const long long base = (long long)p.B * p.H * p.nLT;
    S = (int)std::min<long long>((2LL * cus + base - 1) / base, std::min(p.nQT, ELM_MAX_SLICES));
    S = std::max(S, 1);
  }
  p.per = (p.nQT + S - 1) / S;
  p.S = forced > 0 ? S : (p.nQT + p.per - 1) / p.per;
}

// which: 0 prepare, 1 forward, 2 query-side backward, 3 key-side backward (S > 1: into the slice planes; the caller folds)
int eva_lm_dispatch(int which, const EvaLmP& p, int dtype, int D, hipStream_t st);

}  // namespace ea
