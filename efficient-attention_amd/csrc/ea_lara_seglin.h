// ea_lara_seglin.h -- parameter block and dispatchers of the segment kernels with the generator Linear inside (ea_lara_seglin.hip).
#pragma once
#include "ea_common.h"

namespace ea {

struct SegLinP {
  char *q, *k;                       // stored q / k rows (element type), [B,H,N,64] views
  int64_t q_sb, q_sh, q_sn, k_sb, k_sh, k_sn;
  char *dq, *dk;                     // backward: accumulated into
  int64_t dq_sb, dq_sh, dq_sn, dk_sb, dk_sh, dk_sn;
  const float *Gq, *Gk, *gqb, *gkb;  // generator Linear [64, 64] (out, in), bias [64]
  const float *lnq_w, *lnq_b, *lnk_w, *lnk_b;   // LayerNorm weight / bias [64]
  float *qbar, *kbar;                // forward outputs [B*H, L, 64]
  const float *d_qbar, *d_kbar;      // backward inputs
  float* part;                       // backward: [B*H*groups, 2, 4, 64] partial sums (d ln_w, d ln_b, d g_b, unused)
  f32x4* stats;                      // backward scratch [B*H, 2, N]: (mean, rstd, mean(a xhat), -) of every token's LayerNorm
  float* dG_part;                    // backward: [nG, 2, 64, 64] partial sums of dG (nG = B*H*groups)
  int B, H, N, L, segs, nshort, groups, seg_per_group, cgroups, cseg_per_group;
  // the estimator's last dq correction riding on the dq / dk pass (ea_lara_seglin_bwd_fin, round 6): dq_n -= s sum_c t[c,n] (u qbar)_c
  const float *fin_qbar, *fin_uq, *fin_lse;   // [B*H, C, 64], [B*H, C, 64], [B*H, C]; null: none
  int C;
  float fin_scale, fin_scale_log2;
};

int seglin_groups(int BH, int L);
int seglin_dispatch(int which, const SegLinP& p, int dtype, hipStream_t st);

}  // namespace ea
