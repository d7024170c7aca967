// ea_lara_lm.h -- parameter block and launch plan of the LARA token-column passes for 128 < C <= 512 samples (ea_lara_lm.hip).
#pragma once
#include <algorithm>
#include "ea_common.h"
#include "ea_t4.h"

namespace ea {

constexpr int LLM_GROUP = 64;                      // samples per turn of the landmark loop / rows of a streamed tile
constexpr int LLM_MIN_C = 129, LLM_MAX_C = 512;    // below: lara_x_body holds every 16-sample tile in registers
constexpr size_t LLM_LDS_RESIDENT = 144 * 1024;    // the images of a pass stay in LDS up to this size (of 160 KB per CU)
enum { LLM_FWD = 0, LLM_BWDQ = 1, LLM_BWDK = 2, LLM_QCORR = 3 };
enum { LLM_PLAN_AUTO = 0, LLM_PLAN_RESIDENT = 1, LLM_PLAN_STREAMED = 2 };

struct LaraLmP {
  T4 q, k, v, o, dout, dq, dk, dv;       // 16-bit [B,H,N,64] views
  const uint8_t* mask;                   // [B,N] key padding mask or null
  // 16-bit images [BH, Cp, 64], rows >= C zero: omega | qbar | (kv, d kv, u qbar)
  const char* img[3];
  // prepared scalar columns fp32 [BH, 3, Cp]: (cst2, lse_t2, bhv) | (lse_k2, dkk, r); the pad slots hold the value that gives
  // the slot weight exactly 0: cst2 = -inf, lse_t2 = lse_k2 = +inf, bhv = 1, dkk = r = 0
  const float* sc;
  float *lseZ, *tmean, *rowdot, *sda;    // per-token scalars [BH, N] (lseZ in log2 units)
  int B, H, N, C, Cp, NG;                // Cp = 64 NG
  int mis;
  int nsplit, tok_per_block, resident;   // workgroups per (b, h), tokens of one (multiple of 64), the plan
  float kappa, scale, scale_log2;
  // prepare: fp32 masters [BH, C, 64] / [BH, C] (null: zero rows / the pad value everywhere) -> images and columns
  const float* src[3];
  char* dst[3];
  const float* ssrc[3];
  float* sdst;
  float smul[3], spad[3];
};

// images a pass stages: omega (all but QCORR), qbar (where t or the biased logit enters), the third
inline int llm_images(int mode, int mis) {
  if (mode == LLM_BWDK || mode == LLM_QCORR) return 2;
  return mis == 2 ? 2 : 3;
}
inline size_t llm_lds(int mode, int mis, int Cp, bool resident) {
  const size_t rows = resident ? (size_t)Cp : 2 * LLM_GROUP;
  return (size_t)3 * Cp * sizeof(float) + (size_t)llm_images(mode, mis) * rows * 64 * 2;
}
// plan: resident where the pass's images fit; then a workgroup walks as many 64-token tiles as it takes to bring the grid down
// to the workgroups the chip holds at once (the images are staged once per workgroup).  Streamed groups gain nothing from a
// walk: one tile per workgroup.  `force`: LLM_PLAN_*.  -> false when a forced resident plan does not fit.
inline bool llm_plan(LaraLmP& p, int mode, int force, int cus) {
  const bool fits = llm_lds(mode, p.mis, p.Cp, true) <= LLM_LDS_RESIDENT;
  if (force == LLM_PLAN_RESIDENT && !fits) return false;
  p.resident = force == LLM_PLAN_STREAMED ? 0 : (fits ? 1 : 0);
  const int tiles = (p.N + 63) / 64;
  int walk = 1;
  if (p.resident) {
    const long long per_cu = std::max<long long>(1, (long long)(160 * 1024) / (long long)llm_lds(mode, p.mis, p.Cp, true));
    const long long total = (long long)p.B * p.H * tiles;
    walk = (int)std::min<long long>(std::max<long long>((total + per_cu * cus - 1) / (per_cu * cus), 1), tiles);
  }
  p.nsplit = (tiles + walk - 1) / walk;
  p.tok_per_block = 64 * ((tiles + p.nsplit - 1) / p.nsplit);
  p.nsplit = (p.N + p.tok_per_block - 1) / p.tok_per_block;
  return true;
}

// which: -1 prepare, else LLM_*
int lara_lm_dispatch(int which, const LaraLmP& p, int dtype, hipStream_t st);

}  // namespace ea
