// ea_ceva_lm.h -- parameter block of the causal-EVA landmark-column kernels (ea_ceva_lm.hip): block-lower-triangular
// attention of N queries over L = N / r landmark keys, joined with the window half through the two log-sum-exps.
#pragma once
#include "ea_common.h"
#include "ea_t4.h"
#include "ea_lm_frag.h"

namespace ea {

constexpr int CLM_MAX_QT = 1024;         // query tiles per (b, h) the key-side kernel lists in LDS (N <= 65536)
constexpr float CLM_DEGENERATE = -4e4f;  // a row whose joint lse lies below this has nothing but -5e4 fills: they all count

struct CevaLmP {
  T4 q, oloc, out, dout, doloc;          // 16-bit [B,H,N,D] views
  const char *lk16, *lv16;               // 16-bit images [B*H, Lp, D] of rf_k_bar / beta, rows >= L zero
  const float *lk, *lv;                  // prepare: the fp32 masters [B*H, L, D]
  const float* lse_loc;                  // [B*H, N] log-sum-exp of the window half
  float* zl;                             // [B*H, N, 2] (joint lse Z, landmark lse)
  float* delta;                          // [B*H, N] rowsum(dout * out)
  float* dlse_loc;                       // [B*H, N]
  float* dq;                             // fp32 [B, N, H, D]: scale * dS . lk
  float *dlk, *dlv;                      // fp32 [B*H, L, D]
  int* flags;                            // [B*H, nQT] query tile holds a degenerate row (written by bwd_q, read by bwd_k)
  const uint8_t* keep;                   // [B*H, N, keep_ld] dropout keep mask of the landmark columns, or null
  int keep_ld;
  float keep_scale;
  int B, H, N, L, Lp, r, lm_base, nQT;
  float scale, scale_log2;
};

inline int clm_lp(int L) { return (L + CLM_TILE - 1) / CLM_TILE * CLM_TILE; }

// which: 0 prepare, 1 forward, 2 query-side backward, 3 key-side backward
int ceva_lm_dispatch(int which, const CevaLmP& p, int dtype, int D, hipStream_t st);

}  // namespace ea
