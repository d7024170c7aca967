// ea_capi.hip -- extern "C" entry points of libea_hip.so (declared in include/ea_hip.h).
// Argument validation and launch-parameter construction only; every kernel lives in its own
// translation unit and is reached through a *_dispatch function.
#include <stdlib.h>
#include <cmath>
#include "ea_window.h"
#include "ea_landmark_params.h"
#include "ea_lara.h"
#include "ea_softmax.h"
#include "ea_lara_lmk.h"
#include "ea_lara_merge.h"
#include "ea_layernorm.h"
#include "ea_lara_segment.h"
#include "ea_scatter.h"
#include "ea_rows_mlp.h"
#include "ea_performer_f32.h"
#include "ea_kernelized.h"
#include "ea_f32_tile.h"
#include "ea_f32_attn.h"
#include "ea_linear.h"
#include "ea_proj.h"
#include "ea_fold.h"
#include "ea_lara_seglin.h"

using namespace ea;

// kernels that form token * stride in 32-bit arithmetic additionally need N * sn < 2^31 elements
static bool t4_ok32(const ea_t4* t, int D, int N) {
  return view_ok(t, D, 2) && (int64_t)N * t->sn < ((int64_t)1 << 31);
}
static bool geom_ok(const ea_geom* g) {
  return g && g->B > 0 && g->H > 0 && g->N > 0 && (g->D == 32 || g->D == 64 || g->D == 128) &&
         (g->dtype == EA_BF16 || g->dtype == EA_F16) && g->ext >= 0 && g->causal >= 0 && g->causal <= 2 && g->lm_base >= 0;
}
static Geo mk_geo(const ea_geom* g) {
  Geo G;
  G.N = g->N; G.attn2d = g->attn_2d; G.gh = g->attn_2d ? g->gh : 1; G.gw = g->attn_2d ? g->gw : g->N;
  return G;
}

extern "C" {

const char* ea_version(void) { return "ea_hip 0.1.0 gfx950"; }
int32_t ea_abi_version(void) { return 38; }

int32_t ea_window_bias_ld(const ea_geom* g) {
  WinTiling t;
  if (!geom_ok(g) || win_tiling(*g, t, false) != EA_OK) return EA_E_BADARG;
  return t.biasLd;
}
int32_t ea_window_keep_ld(const ea_geom* g) {
  WinTiling t;
  if (!geom_ok(g) || win_tiling(*g, t, false) != EA_OK) return EA_E_BADARG;
  return t.biasLd + t.nCT * 16;
}
int32_t ea_window_bwd_parts(const ea_geom* g) {
  WinTiling t;
  if (!geom_ok(g) || win_tiling(*g, t, true) != EA_OK) return EA_E_BADARG;
  return t.parts_total;
}
int32_t ea_window_bwd_needs_bias_t(const ea_geom* g) {
  WinTiling t;
  if (!geom_ok(g) || win_tiling(*g, t, true) != EA_OK) return EA_E_BADARG;
  int any = 0;                                             // a launch reads the bias from global memory
  win_bwd_launches(*g, t, [&](const WinTiling& tl) { any |= window_bwd_lds(tl, g->D, true, true) > WIN_LDS_MAX; });
  return any;
}
int32_t ea_window_bwd_bias_parts(const ea_geom* g) {
  WinTiling t;
  if (!geom_ok(g) || win_tiling(*g, t, true) != EA_OK) return EA_E_BADARG;
  return win_bwd_bias_parts(*g, t);
}
int32_t ea_window_bwd_acc_slices(const ea_geom* g) {
  WinTiling t;
  if (!geom_ok(g) || win_tiling(*g, t, true) != EA_OK) return EA_E_BADARG;
  return win_bwd_acc_slices(t);
}
int32_t ea_window_bwd_query_blocks(const ea_geom* g) {
  WinTiling t;
  if (!geom_ok(g) || win_tiling(*g, t, true) != EA_OK) return EA_E_BADARG;
  return t.qsplit;
}

static int fill_win(const ea_geom* g, WinP& p, bool backward) {
  if (!geom_ok(g)) return EA_E_BADARG;
  int rc = win_tiling(*g, p.t, backward);
  if (rc != EA_OK) return rc;
  if (g->L < 0 || g->L > 64) return EA_E_UNSUPPORTED;      // landmark tiles owned 1:1 by 4 waves
  p.G = mk_geo(g);
  p.B = g->B; p.H = g->H; p.L = g->L; p.w = g->window; p.e = g->ext;
  p.causal = g->causal; p.chunk = g->chunk; p.lm_base = g->causal == 2 ? g->lm_base : 0;
  p.scale = g->scale;
  p.scale_log2 = g->scale * LOG2E;
  return EA_OK;
}

int ea_window_attn_fwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                       const float* lk, const float* lv, const float* bias, const uint8_t* mask,
                       const ea_t4* out, float* lse, const uint8_t* keep, float keep_scale, void* stream) {
  WinP p = {};
  int rc = fill_win(g, p, false);
  if (rc != EA_OK) return rc;
  if (keep && !g->causal) return EA_E_UNSUPPORTED;
  p.keep = keep; p.keep_scale = keep_scale; p.keep_ld = p.t.biasLd + p.t.nCT * 16;
  if (!view_ok(q, g->D, 2) || !view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !view_ok(out, g->D, 2) || !lse) return EA_E_BADARG;
  if (g->L > 0 && (!lk || !lv)) return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.v = mk(v); p.o = mk(out);
  p.lk = lk; p.lv = lv; p.bias = bias; p.mask = mask; p.lse = lse;
  return window_fwd_dispatch(p, g->dtype, g->D, (hipStream_t)stream);
}

int ea_window_attn_bwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                       const float* lk, const float* lv, const float* bias, const uint8_t* mask,
                       const ea_t4* out, const ea_t4* dout, const float* lse,
                       const ea_t4* dq, const ea_t4* dk, const ea_t4* dv,
                       float* dlk_part, float* dlv_part, float* dbias_part,
                       float* dk_acc, float* dv_acc, const float* bias_t,
                       const uint8_t* keep, float keep_scale, const float* dlse, void* stream) {
  WinP p = {};
  int rc = fill_win(g, p, true);
  if (rc != EA_OK) return rc;
  p.dlse = dlse;
  if (keep && !g->causal) return EA_E_UNSUPPORTED;
  p.keep = keep; p.keep_scale = keep_scale; p.keep_ld = p.t.biasLd + p.t.nCT * 16;
  const int N = g->N;
  if (!t4_ok32(q, g->D, N) || !t4_ok32(k, g->D, N) || !t4_ok32(v, g->D, N) || !t4_ok32(dout, g->D, N) ||
      !t4_ok32(out, g->D, N) || (win_bwd_acc_slices(p.t) > 0 && (!dk_acc || !dv_acc)) || !t4_ok32(dq, g->D, N) ||
      !t4_ok32(dk, g->D, N) || !t4_ok32(dv, g->D, N) || !lse) return EA_E_BADARG;
  if (g->L > 0 && (!lk || !lv || !dlk_part || !dlv_part)) return EA_E_BADARG;
  if (bias && (!dbias_part || (!bias_t && ea_window_bwd_needs_bias_t(g) != 0))) return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.v = mk(v); p.o = mk(dout);
  p.dq = mk(dq); p.dk = mk(dk); p.dv = mk(dv);
  p.lk = lk; p.lv = lv; p.bias = bias; p.mask = mask; p.lse = const_cast<float*>(lse);
  p.dlk_part = dlk_part; p.dlv_part = dlv_part; p.dbias_part = dbias_part;
  p.dk32 = dk_acc; p.dv32 = dv_acc;
  return window_bwd_dispatch(p, *g, mk(out), bias ? bias_t : nullptr, g->dtype, g->D, (hipStream_t)stream);
}

// ---- EVA landmark statistics ----
static int fill_lm(const ea_geom* g, LmP& p) {
  if (!geom_ok(g) || g->chunk <= 0 || g->L <= 0) return EA_E_BADARG;
  p.G = mk_geo(g);
  if (g->attn_2d && (g->gh * g->gw != g->N)) return EA_E_BADARG;
  if (g->causal && (g->attn_2d || g->N % g->chunk)) return EA_E_BADARG;
  const int ext = g->causal ? 0 : g->ext;                  // causal_eva.py:688-694: chunks are not extended
  const int side = g->chunk + 2 * ext;
  const int nchunks = g->attn_2d ? (g->gh / g->chunk) * (g->gw / g->chunk) : g->N / g->chunk;
  if (nchunks != g->L) return EA_E_BADARG;
  p.B = g->B; p.H = g->H; p.L = g->L; p.r = g->chunk; p.e = ext;
  p.J = g->attn_2d ? side * side : side;
  p.scale = g->scale;
  return EA_OK;
}
#define SET3(dst, src) do { p.dst = (char*)(src)->ptr; p.dst##_sb = (src)->sb; p.dst##_sh = (src)->sh; p.dst##_sn = (src)->sn; } while (0)

int ea_eva_chunk_mean_fwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const uint8_t* mask,
                          float* qmean, float* kmean, void* stream) {
  LmP p = {};
  int rc = fill_lm(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(k, g->D, 2) || !qmean || !kmean) return EA_E_BADARG;
  SET3(q, q); SET3(k, k);
  p.mask = mask; p.qmean = qmean; p.kmean = kmean;
  return landmark_dispatch(0, p, g->dtype, g->D, (hipStream_t)stream);
}

int ea_eva_chunk_mean_bwd(const ea_geom* g, const float* dqmean, const float* dkmean,
                          const uint8_t* mask, const ea_t4* dq, const ea_t4* dk, void* stream) {
  LmP p = {};
  int rc = fill_lm(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(dq, g->D, 2) || !view_ok(dk, g->D, 2) || !dqmean || !dkmean) return EA_E_BADARG;
  SET3(dq, dq); SET3(dk, dk);
  p.mask = mask; p.dqmean = dqmean; p.dkmean = dkmean;
  return landmark_dispatch(1, p, g->dtype, g->D, (hipStream_t)stream);
}

int ea_eva_beta_fwd(const ea_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                    const float* omega, float* beta, void* stream) {
  LmP p = {};
  int rc = fill_lm(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !omega || !beta) return EA_E_BADARG;
  SET3(k, k); SET3(v, v);
  p.mask = mask; p.omega = omega; p.beta_out = beta;
  return landmark_dispatch(2, p, g->dtype, g->D, (hipStream_t)stream);
}

// dbeta_S > 1 (composite EVA backward, round 6): dbeta = slice 0 of dbeta_S <= 4 slice partials `dbeta_stride` floats apart
static int eva_beta_bwd_parts(const ea_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                              const float* omega, const float* beta, const float* dbeta, int dbeta_S, long dbeta_stride,
                              const ea_t4* dk, const ea_t4* dv, float* domega, void* stream) {
  LmP p = {};
  int rc = fill_lm(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !view_ok(dk, g->D, 2) || !view_ok(dv, g->D, 2) || !omega ||
      !beta || !dbeta || !domega || dbeta_S < 1 || dbeta_S > 4) return EA_E_BADARG;
  SET3(k, k); SET3(v, v); SET3(dk, dk); SET3(dv, dv);
  p.mask = mask; p.omega = omega; p.beta = beta; p.dbeta = dbeta; p.domega = domega;
  p.dbeta_S = dbeta_S; p.dbeta_stride = dbeta_stride;
  return landmark_dispatch(3, p, g->dtype, g->D, (hipStream_t)stream);
}

int ea_eva_beta_bwd(const ea_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                    const float* omega, const float* beta, const float* dbeta,
                    const ea_t4* dk, const ea_t4* dv, float* domega, void* stream) {
  return eva_beta_bwd_parts(g, k, v, mask, omega, beta, dbeta, 1, 0, dk, dv, domega, stream);
}

}  // extern "C"

// ---- LARA ----
static int lara_nsub(int NCT) { return NCT == 1 ? 4 : (NCT == 2 ? 2 : 1); }
// X passes: blocks per (b,h) and tokens per block; Y passes: sequence splits
static int fill_lara(const ea_lara_geom* g, LaraP& p, bool ypass) {
  if (!g || g->B <= 0 || g->H <= 0 || g->N <= 0 || (g->D != 32 && g->D != 64) || g->C <= 0 ||
      (g->dtype != EA_BF16 && g->dtype != EA_F16) || g->mis < 0 || g->mis > 2) return EA_E_BADARG;
  if (g->C > 128) return EA_E_UNSUPPORTED;
  p.B = g->B; p.H = g->H; p.N = g->N; p.D = g->D; p.C = g->C; p.NCT = (g->C + 15) / 16;
  p.mis = g->mis; p.kappa = g->kappa; p.scale = g->scale; p.scale_log2 = g->scale * LOG2E;
  p.norm_coef2 = 0.5f * g->scale * LOG2E;      // s |k|^2 / 2 in the log2 domain
  p.knorm_coef = g->scale;
  const long bh = (long)g->B * g->H;
  const int gran = ypass ? 128 : 64;
  const int maxblk = (g->N + gran - 1) / gran;
  // X passes re-stage the landmark matrices per workgroup: fewer, longer workgroups (~3 per CU);
  // Y passes only keep landmark fragments in registers: more, shorter slices
  // (Y-pass partial results are [BH, nsplit, C, D] fp32 per accumulator -- as large as the token
  // tensors themselves at 6 slices -- so both passes aim at ~3 workgroups per CU, not more)
  int nblk = (int)((768 + bh - 1) / bh);
  if (nblk < 1) nblk = 1;
  if (nblk > maxblk) nblk = maxblk;
  if (ypass) {
    // the slice boundaries are laid out at launch (lara_y_plan: they depend on how many
    // workgroups of the particular pass fit on the chip); only the count is fixed here
    p.nsplit = nblk > 16 ? 16 : nblk;
    p.tok_per_block = 0;
    return EA_OK;
  }
  int tpb = (g->N + nblk - 1) / nblk;
  tpb = (tpb + gran - 1) / gran * gran;
  p.tok_per_block = tpb;
  p.nsplit = (g->N + tpb - 1) / tpb;
  return EA_OK;
}

extern "C" {

int32_t ea_lara_parts(const ea_lara_geom* g) {
  LaraP p = {};
  if (const int rc = fill_lara(g, p, true)) return rc;      // (C > 128 is an unsupported geometry, not a bad argument)
  return p.nsplit * lara_nsub(p.NCT);
}

int ea_lara_stats_fwd(const ea_lara_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                      const uint8_t* mask, const float* omega, const float* qbar,
                      float* p_ml, float* p_kv, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, true);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !omega || !p_ml || !p_kv ||
      (g->mis == EA_MIS_OPT && !qbar)) return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.v = mk(v); p.mask = mask; p.omega = omega; p.qbar = qbar;
  p.p_ml = p_ml; p.p_acc0 = p_kv;
  return lara_y_dispatch(LY_FWD, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_out_fwd(const ea_lara_geom* g, const ea_t4* q, const float* omega, const float* qbar,
                    const float* kv, const float* lse_t, const float* bhv, const float* cst,
                    const ea_t4* out, float* lseZ, float* tmean, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(out, g->D, 2) || !omega || !kv || !cst) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar || !lse_t || !bhv)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !qbar) return EA_E_BADARG;
  if ((lseZ == nullptr) != (tmean == nullptr)) return EA_E_BADARG;
  p.q = mk(q); p.o = mk(out); p.omega = omega; p.qbar = qbar; p.kv = kv; p.lse_t = lse_t;
  p.bhv = bhv; p.cst = cst; p.lseZ = lseZ; p.tmean = tmean;
  return lara_x_dispatch(LX_FWD, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_q(const ea_lara_geom* g, const ea_t4* q, const ea_t4* dout, const float* omega,
                  const float* qbar, const float* kv, const float* lse_t, const float* bhv,
                  const float* cst, const ea_t4* dq, float* lseZ, float* tmean, float* rowdot,
                  float* sda, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(dout, g->D, 2) || !view_ok(dq, g->D, 2) || !omega || !kv || !cst ||
      !lseZ || !tmean || !rowdot || !sda) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar || !lse_t || !bhv)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !qbar) return EA_E_BADARG;
  p.q = mk(q); p.dout = mk(dout); p.dq = mk(dq); p.omega = omega; p.qbar = qbar; p.kv = kv;
  p.lse_t = lse_t; p.bhv = bhv; p.cst = cst;
  p.lseZ = lseZ; p.tmean = tmean; p.rowdot = rowdot; p.sda = sda;
  return lara_x_dispatch(LX_BWDQ, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_qstats(const ea_lara_geom* g, const ea_t4* q, const ea_t4* dout, const float* omega,
                       const float* qbar, const float* kv, const float* lse_t, const float* bhv,
                       const float* cst, const float* lseZ, const float* tmean, const float* rowdot,
                       const float* sda, float* p_ml, float* p_dkv, float* p_dom, float* p_m1,
                       float* p_m2, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, true);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(dout, g->D, 2) || !omega || !kv || !cst || !lseZ || !tmean ||
      !rowdot || !sda || !p_ml || !p_dkv || !p_dom) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar || !lse_t || !bhv || !p_m1 || !p_m2)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !qbar) return EA_E_BADARG;
  p.q = mk(q); p.dout = mk(dout); p.omega = omega; p.qbar = qbar; p.kv = kv; p.lse_t = lse_t;
  p.bhv = bhv; p.cst = cst;
  p.lseZ = const_cast<float*>(lseZ); p.tmean = const_cast<float*>(tmean);
  p.rowdot = const_cast<float*>(rowdot); p.sda = const_cast<float*>(sda);
  p.p_ml = p_ml; p.p_acc0 = p_dkv; p.p_acc1 = p_dom; p.p_acc2 = p_m1; p.p_acc3 = p_m2;
  return lara_y_dispatch(LY_BWDQ, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_k(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                  const float* omega, const float* dkv, const float* lse_k, const float* dkk,
                  const float* rsum, const ea_t4* dk, const ea_t4* dv, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !view_ok(dk, g->D, 2) || !view_ok(dv, g->D, 2) || !omega ||
      !dkv || !lse_k || !dkk || !rsum) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.dk = mk(dk); p.dv = mk(dv); p.mask = mask; p.omega = omega;
  p.dkv = dkv; p.lse_k = lse_k; p.dkk = dkk; p.rsum = rsum;
  return lara_x_dispatch(LX_BWDK, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_kstats(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                       const float* omega, const float* dkv, const float* lse_k, const float* dkk,
                       const float* rsum, float* p_dom, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, true);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !omega || !dkv || !lse_k || !dkk || !rsum || !p_dom)
    return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.mask = mask; p.omega = omega; p.dkv = dkv; p.lse_k = lse_k;
  p.dkk = dkk; p.rsum = rsum; p.p_acc0 = p_dom;
  return lara_y_dispatch(LY_BWDK, p, g->dtype, (hipStream_t)stream);
}

// ---- fused backward (ea_lara_f.hip): one pass per side + one finish pass ----
int32_t ea_lara_fused_parts(const ea_lara_geom* g) {
  LaraP p = {};
  if (const int rc = fill_lara(g, p, false)) return rc;
  if (p.NCT > 4) return EA_E_UNSUPPORTED;
  return p.nsplit * (p.NCT <= 2 ? 2 : 1);
}

int ea_lara_bwd_q_fused(const ea_lara_geom* g, const ea_t4* q, const ea_t4* dout, const float* omega,
                        const float* qbar, const float* kv, const float* lse_t, const float* bhv,
                        const float* cst, const float* lseZ, const float* tmean, const ea_t4* dq, float* p_ml,
                        float* p_dkv, float* p_dom, float* p_m1, float* p_m2, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (p.NCT > 4) return EA_E_UNSUPPORTED;
  if (!view_ok(q, g->D, 2) || !view_ok(dout, g->D, 2) || !view_ok(dq, g->D, 2) || !omega || !kv || !cst || !p_ml ||
      !p_dkv || !p_dom || !lseZ || !tmean) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar || !lse_t || !bhv || !p_m1 || !p_m2)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !qbar) return EA_E_BADARG;
  p.q = mk(q); p.dout = mk(dout); p.dq = mk(dq); p.omega = omega; p.qbar = qbar; p.kv = kv;
  p.lse_t = lse_t; p.bhv = bhv; p.cst = cst;
  p.lseZ = const_cast<float*>(lseZ); p.tmean = const_cast<float*>(tmean);
  p.p_ml = p_ml; p.p_acc0 = p_dkv; p.p_acc1 = p_dom; p.p_acc2 = p_m1; p.p_acc3 = p_m2;
  return lara_f_dispatch(0, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_k_fused(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                        const float* omega, const float* dkv, const float* lse_k, const float* dkk,
                        const float* rsum, const ea_t4* dk, const ea_t4* dv, float* p_dom, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (p.NCT > 4) return EA_E_UNSUPPORTED;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !view_ok(dk, g->D, 2) || !view_ok(dv, g->D, 2) || !omega ||
      !dkv || !lse_k || !dkk || !rsum || !p_dom) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.dk = mk(dk); p.dv = mk(dv); p.mask = mask; p.omega = omega;
  p.dkv = dkv; p.lse_k = lse_k; p.dkk = dkk; p.rsum = rsum; p.p_acc0 = p_dom;
  return lara_f_dispatch(1, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_finish(const ea_lara_geom* g, const ea_t4* q, const float* qbar, const float* uq,
                       const float* lse_t, const float* dpq, const float* dpk, int32_t pool_r,
                       int32_t gh, int32_t gw, const ea_t4* dq, const ea_t4* dk, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (p.NCT > 4) return EA_E_UNSUPPORTED;
  if (!view_ok(dq, g->D, 2)) return EA_E_BADARG;
  const bool has_t = uq != nullptr;
  if (has_t && (g->mis != EA_MIS_OPT || !view_ok(q, g->D, 2) || !qbar || !lse_t)) return EA_E_BADARG;
  if (pool_r > 0) {
    if (!dpq || !dpk || !view_ok(dk, g->D, 2) || gh <= 0 || gw <= 0 || gh * gw != g->N || gh % pool_r || gw % pool_r)
      return EA_E_BADARG;
    p.dpq = dpq; p.dpk = dpk; p.pool_r = pool_r; p.pool_gw = gw;
    p.pool_L = (gh / pool_r) * (gw / pool_r);
    p.pool_inv = 1.f / (float)(pool_r * pool_r);
    p.dk = mk(dk);
  } else if (!has_t) {
    return EA_OK;                                   // nothing to do
  }
  if (has_t) { p.q = mk(q); p.qbar = qbar; p.uq = uq; p.lse_t = lse_t; }
  p.dq = mk(dq);
  return lara_f_dispatch(2, p, g->dtype, (hipStream_t)stream);
}

// ---- round 5: consumers that merge the producing pass's slice partials in their prologue (no merge launches) ----
int ea_lara_out_fwd_merge(const ea_lara_geom* g, const ea_t4* q, const float* omega, const float* qbar, const float* bhv,
                          int32_t S, const float* p_ml, const float* p_kv, const float* lp, float* kv, float* lse_k,
                          float* lse_t, float* cst, const ea_t4* out, float* lseZ, float* tmean, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (p.NCT > 4 || S < 1 || S > 4) return EA_E_UNSUPPORTED;
  if (!view_ok(q, g->D, 2) || !view_ok(out, g->D, 2) || !omega || !p_ml || !p_kv || !lp || !kv || !lse_k || !cst) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar || !lse_t || !bhv)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !qbar) return EA_E_BADARG;
  if ((lseZ == nullptr) != (tmean == nullptr)) return EA_E_BADARG;
  p.q = mk(q); p.o = mk(out); p.omega = omega; p.qbar = qbar; p.bhv = bhv; p.lseZ = lseZ; p.tmean = tmean;
  p.m_S = S; p.m_ml = p_ml; p.m_acc0 = p_kv; p.m_lp = lp;
  p.m_kv = kv; p.m_lsek = lse_k; p.m_lset = lse_t; p.m_cst = cst;
  return lara_x_dispatch(LX_FWDM, p, g->dtype, (hipStream_t)stream);
}

// ABI 29: the same pass with the output projection inside (ea_lara_xp.hip).  Out-of-scope geometry is refused first, so a
// caller that probes with it falls back to ea_lara_out_fwd_merge + ea_linear without having launched anything.
int ea_lara_out_proj_fwd_merge(const ea_lara_geom* g, const ea_t4* q, const float* omega, const float* qbar, const float* bhv,
                               int32_t S, const float* p_ml, const float* p_kv, const float* lp, float* kv, float* lse_k,
                               float* lse_t, float* cst, const ea_t4* out, float* lseZ, float* tmean, const void* w_proj16,
                               const float* bias, void* y, int64_t ldy, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (!lara_xp_supported(g->H, g->D, g->C, S)) return EA_E_UNSUPPORTED;
  if (!view_ok(q, g->D, 2) || !view_ok(out, g->D, 2) || !omega || !p_ml || !p_kv || !lp || !kv || !lse_k || !cst) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar || !lse_t || !bhv)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !qbar) return EA_E_BADARG;
  if ((lseZ == nullptr) != (tmean == nullptr)) return EA_E_BADARG;
  if (!w_proj16 || ((uintptr_t)w_proj16 & 15) || !y || ((uintptr_t)y & 7) || ldy < 192 || (ldy & 3) ||
      (bias && ((uintptr_t)bias & 3))) return EA_E_BADARG;
  p.q = mk(q); p.o = mk(out); p.omega = omega; p.qbar = qbar; p.bhv = bhv; p.lseZ = lseZ; p.tmean = tmean;
  p.m_S = S; p.m_ml = p_ml; p.m_acc0 = p_kv; p.m_lp = lp;
  p.m_kv = kv; p.m_lsek = lse_k; p.m_lset = lse_t; p.m_cst = cst;
  LaraXpP xp;
  xp.w = (const char*)w_proj16; xp.bias = bias; xp.y = (char*)y; xp.ldy = (long)ldy;
  return lara_xp_dispatch(p, xp, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_k_fused_merge(const ea_lara_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* omega,
                              const float* qbar, const float* kv, const float* lse_k, int32_t S, const float* p_ml,
                              const float* p_dkv, const float* p_dom, const float* p_m1, const float* p_m2,
                              const ea_t4* dk, const ea_t4* dv, float* p_domk, float* dbh, float* dlp, float* domq,
                              float* dqbar, float* uq, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (p.NCT > 4 || S < 1 || S > 4) return EA_E_UNSUPPORTED;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !view_ok(dk, g->D, 2) || !view_ok(dv, g->D, 2) || !omega || !kv || !lse_k || !p_ml ||
      !p_dkv || !p_dom || !p_domk || !dlp || !domq) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar || !p_m1 || !p_m2 || !dqbar || !uq || !dbh)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !dqbar) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.dk = mk(dk); p.dv = mk(dv); p.mask = mask; p.omega = omega; p.qbar = qbar;
  p.kv = kv; p.lse_k = lse_k; p.p_acc0 = p_domk;
  p.m_S = S; p.m_ml = p_ml; p.m_acc0 = p_dkv; p.m_acc1 = p_dom; p.m_acc2 = p_m1; p.m_acc3 = p_m2;
  p.m_dbh = dbh; p.m_dlp = dlp; p.m_domq = domq; p.m_dqbar = dqbar; p.m_uq = uq;
  return lara_f_dispatch(3, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_bwd_qcorr(const ea_lara_geom* g, const ea_t4* q, const float* qbar, const float* uq,
                      const float* lse_t, const ea_t4* dq, void* stream) {
  LaraP p = {};
  int rc = fill_lara(g, p, false);
  if (rc != EA_OK) return rc;
  if (g->mis != EA_MIS_OPT) return EA_E_BADARG;
  if (!view_ok(q, g->D, 2) || !view_ok(dq, g->D, 2) || !qbar || !uq || !lse_t) return EA_E_BADARG;
  p.q = mk(q); p.dq = mk(dq); p.qbar = qbar; p.uq = uq; p.lse_t = lse_t;
  return lara_x_dispatch(LX_QCORR, p, g->dtype, (hipStream_t)stream);
}

}  // extern "C"

// ---- softmax baseline ----
#define SM_SET(dst, src) do { if (src) { p.dst.p = (char*)(src)->ptr; p.dst.sb = (src)->sb; p.dst.sh = (src)->sh; p.dst.sn = (src)->sn; } } while (0)
static int fill_sm(int B, int H, int N, int D, int dtype, float scale, SmP& p) {
  if (B <= 0 || H <= 0 || N <= 0 || (D != 32 && D != 64 && D != 128) || (dtype != EA_BF16 && dtype != EA_F16))
    return EA_E_BADARG;
  p.B = B; p.H = H; p.N = N; p.scale = scale; p.scale_log2 = scale * LOG2E;
  return EA_OK;
}

extern "C" {

int ea_softmax_attn_fwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t dtype, float scale,
                        const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                        const ea_t4* out, float* lse, const uint8_t* keep, float keep_scale,
                        int32_t key_norm_bias, void* stream) {
  SmP p = {};
  int rc = fill_sm(B, H, N, D, dtype, scale, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, D, 2) || !view_ok(k, D, 2) || !view_ok(v, D, 2) || !view_ok(out, D, 2) || !lse) return EA_E_BADARG;
  if (key_norm_bias && keep) return EA_E_UNSUPPORTED;
  p.key_norm_bias = key_norm_bias;
  p.keep = keep; p.keep_scale = keep_scale; p.keep_ld = (N + 63) / 64 * 64;
  SM_SET(q, q); SM_SET(k, k); SM_SET(v, v); SM_SET(o, out);
  p.mask = mask; p.lse = lse;
  return softmax_dispatch(0, p, dtype, D, (hipStream_t)stream);
}

int ea_softmax_attn_bwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t dtype, float scale,
                        const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                        const ea_t4* out, const ea_t4* dout, const float* lse, float* delta,
                        const ea_t4* dq, const ea_t4* dk, const ea_t4* dv,
                        const uint8_t* keep, float keep_scale, int32_t key_norm_bias, void* stream) {
  SmP p = {};
  int rc = fill_sm(B, H, N, D, dtype, scale, p);
  if (rc != EA_OK) return rc;
  if (key_norm_bias && keep) return EA_E_UNSUPPORTED;
  p.key_norm_bias = key_norm_bias;
  p.keep = keep; p.keep_scale = keep_scale; p.keep_ld = (N + 63) / 64 * 64;
  if (!view_ok(q, D, 2) || !view_ok(k, D, 2) || !view_ok(v, D, 2) || !view_ok(out, D, 2) || !view_ok(dout, D, 2) ||
      !view_ok(dq, D, 2) || !view_ok(dk, D, 2) || !view_ok(dv, D, 2) || !lse || !delta) return EA_E_BADARG;
  SM_SET(q, q); SM_SET(k, k); SM_SET(v, v); SM_SET(o, out); SM_SET(dout, dout);
  SM_SET(dq, dq); SM_SET(dk, dk); SM_SET(dv, dv);
  p.mask = mask; p.lse = const_cast<float*>(lse); p.delta = delta;
  return softmax_dispatch(1, p, dtype, D, (hipStream_t)stream);
}

int ea_softmax_sample(int32_t B, int32_t H, int32_t N, int32_t D, int32_t dtype, float scale,
                      const ea_t4* q, const ea_t4* k, const uint64_t* seed, int64_t* index, void* stream) {
  SmP p = {};
  int rc = fill_sm(B, H, N, D, dtype, scale, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, D, 2) || !view_ok(k, D, 2) || !seed || !index) return EA_E_BADARG;
  SM_SET(q, q); SM_SET(k, k);
  p.seed = reinterpret_cast<const unsigned long long*>(seed);
  p.sample_out = reinterpret_cast<long long*>(index);
  return softmax_dispatch(2, p, dtype, D, (hipStream_t)stream);
}

int32_t ea_softmax_tiles(int32_t which, int32_t B, int32_t H, int32_t N, int32_t D, int32_t has_keep, int32_t cus) {
  SmP p = {};
  int rc = fill_sm(B, H, N, D, EA_BF16, 1.f, p);          // (the rule does not depend on the I/O type)
  if (rc != EA_OK) return rc;
  if ((which != 0 && which != 1) || cus < 0) return EA_E_BADARG;
  return softmax_tiles(which, (long)B * H, N, D, has_keep != 0, cus > 0 ? cus : ea_device_cus());
}

}  // extern "C"

// ---- Performer (FAVOR+) on the LARA skeletons ----
static int fill_perf(const ea_perf_geom* g, LaraP& p, bool ypass) {
  if (!g) return EA_E_BADARG;
  ea_lara_geom lg;
  lg.B = g->B; lg.H = g->H; lg.N = g->N; lg.D = g->D; lg.dtype = g->dtype; lg.C = g->M;
  lg.mis = EA_MIS_BH; lg.kappa = 0.f;
  lg.scale = 1.f / sqrtf(sqrtf((float)g->D));            // data_normalizer d^-1/4
  int rc = fill_lara(&lg, p, ypass);
  if (rc != EA_OK) return rc;
  p.w_per_head = 1;
  p.norm_coef2 = 0.5f * lg.scale * lg.scale * LOG2E;      // d^-1/2 |x|^2 / 2
  p.knorm_coef = lg.scale * lg.scale;
  p.ratio = 1.f / sqrtf((float)g->M);
  p.feps = 1e-4f;
  return EA_OK;
}

extern "C" {

int32_t ea_performer_parts(const ea_perf_geom* g) {
  LaraP p = {};
  if (fill_perf(g, p, true) != EA_OK) return EA_E_BADARG;
  return p.nsplit * lara_nsub(p.NCT);
}

int ea_performer_kmax(const ea_perf_geom* g, const ea_t4* k, const float* W, float* p_ml, void* stream) {
  LaraP p = {};
  int rc = fill_perf(g, p, true);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !W || !p_ml) return EA_E_BADARG;
  p.k = mk(k); p.omega = W; p.p_ml = p_ml;
  return lara_y_dispatch(LY_PMAX, p, g->dtype, (hipStream_t)stream);
}

int ea_performer_kv(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                    const float* W, const float* stab, float* p_ml, float* p_kv, void* stream) {
  LaraP p = {};
  int rc = fill_perf(g, p, true);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !W || !stab || !p_ml || !p_kv) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.mask = mask; p.omega = W; p.stab = stab; p.p_ml = p_ml; p.p_acc0 = p_kv;
  return lara_y_dispatch(LY_PKV, p, g->dtype, (hipStream_t)stream);
}

int ea_performer_out(const ea_perf_geom* g, const ea_t4* q, const float* W, const float* kv,
                     const float* ksum, const ea_t4* out, void* stream) {
  LaraP p = {};
  int rc = fill_perf(g, p, false);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(out, g->D, 2) || !W || !kv || !ksum) return EA_E_BADARG;
  p.q = mk(q); p.o = mk(out); p.omega = W; p.kv = kv; p.cst = ksum;
  return lara_x_dispatch(LX_POUT, p, g->dtype, (hipStream_t)stream);
}

int ea_performer_bwd_q(const ea_perf_geom* g, const ea_t4* q, const ea_t4* out, const ea_t4* dout,
                       const float* W, const float* kv, const float* ksum, const ea_t4* dq,
                       float* stabq, float* invden, float* dden, void* stream) {
  LaraP p = {};
  int rc = fill_perf(g, p, false);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(out, g->D, 2) || !view_ok(dout, g->D, 2) || !view_ok(dq, g->D, 2) || !W || !kv ||
      !ksum || !stabq || !invden || !dden) return EA_E_BADARG;
  p.q = mk(q); p.o = mk(out); p.dout = mk(dout); p.dq = mk(dq); p.omega = W; p.kv = kv; p.cst = ksum;
  p.lseZ = stabq; p.tmean = invden; p.rowdot = dden;
  return lara_x_dispatch(LX_PBWDQ, p, g->dtype, (hipStream_t)stream);
}

int ea_performer_bwd_qstats(const ea_perf_geom* g, const ea_t4* q, const ea_t4* dout, const float* W,
                            const float* stabq, const float* invden, const float* dden,
                            float* p_ml, float* p_dkv, void* stream) {
  LaraP p = {};
  int rc = fill_perf(g, p, true);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, g->D, 2) || !view_ok(dout, g->D, 2) || !W || !stabq || !invden || !dden || !p_ml || !p_dkv)
    return EA_E_BADARG;
  p.q = mk(q); p.dout = mk(dout); p.omega = W;
  p.lseZ = const_cast<float*>(stabq); p.tmean = const_cast<float*>(invden); p.rowdot = const_cast<float*>(dden);
  p.p_ml = p_ml; p.p_acc0 = p_dkv;
  return lara_y_dispatch(LY_PBWDQ, p, g->dtype, (hipStream_t)stream);
}

int ea_performer_bwd_k(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                       const float* W, const float* stab, const float* dkv, const float* dksum,
                       const ea_t4* dk, const ea_t4* dv, void* stream) {
  LaraP p = {};
  int rc = fill_perf(g, p, false);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !view_ok(dk, g->D, 2) || !view_ok(dv, g->D, 2) || !W || !stab ||
      !dkv || !dksum) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.dk = mk(dk); p.dv = mk(dv); p.mask = mask; p.omega = W; p.stab = stab;
  p.dkv = dkv; p.rsum = dksum;
  return lara_x_dispatch(LX_PBWDK, p, g->dtype, (hipStream_t)stream);
}

}  // extern "C"

// ---- fused LARA landmark pipeline ----
static int fill_lmk(const ea_lmk_geom* g, LmkP& p) {
  if (!g || g->BH <= 0 || g->L <= 0 || g->C <= 0 || g->D <= 0) return EA_E_BADARG;
  // a geometry outside the second-generation kernels is well-formed but not built for (ea_hip.h; lara_lmk_dispatch says the same)
  if (g->L > 64 || g->C > 64 || (g->D != 32 && g->D != 64)) return EA_E_UNSUPPORTED;
  if (g->C % g->L != 0 || (g->dup == 0 && g->C != g->L) || (g->dup != 0 && g->C != 2 * g->L)) return EA_E_BADARG;
  if (g->mis < 0 || g->mis > 2 || g->dup < 0 || g->dup > 2) return EA_E_BADARG;
  p.BH = g->BH; p.L = g->L; p.C = g->C; p.D = g->D;
  p.has_mlp = g->has_mlp; p.mixed = g->mixed; p.mis = g->mis; p.dup = g->dup; p.scale = g->scale;
  p.eva = g->eva;
  if (g->eva && (g->dup != 0 || !g->has_mlp)) return EA_E_BADARG;
  return EA_OK;
}
#define LMK_PARAMS(p)                                                                        \
  p.Wq = Wq; p.bq = bq; p.gq = gq; p.cq = cq; p.Wk = Wk; p.bk = bk; p.gk = gk; p.ck = ck;
extern "C" {

int ea_lara_landmarks_fwd(const ea_lmk_geom* g, const float* pq, const float* pk,
                          const float* Wq, const float* bq, const float* gq, const float* cq,
                          const float* Wk, const float* bk, const float* gk, const float* ck,
                          const float* noise, float* omega, float* qbar_rows, float* bhv, float* lp,
                          float* saved, void* stream) {
  LmkP p = {};
  int rc = fill_lmk(g, p);
  if (rc != EA_OK) return rc;
  if (!pq || !pk || !omega || (!lp && !g->eva)) return EA_E_BADARG;
  if (g->has_mlp && (!Wq || !bq || !gq || !cq || !Wk || !bk || !gk || !ck)) return EA_E_BADARG;
  if (!g->eva && g->mis == EA_MIS_OPT && (!qbar_rows || !bhv)) return EA_E_BADARG;
  if ((g->eva || g->mis == EA_MIS_BIASED) && !qbar_rows) return EA_E_BADARG;
  if (g->dup != 0 && !noise) return EA_E_BADARG;
  p.pq = pq; p.pk = pk; LMK_PARAMS(p)
  p.noise = noise; p.omega = omega; p.qbar_rows = qbar_rows; p.bhv = bhv; p.lp = lp;
  p.saved = saved;
  return lara_lmk_dispatch(false, p, (hipStream_t)stream);
}

int ea_lara_landmarks_fwd_cb(const ea_lmk_geom* g, const float* pq, const float* pk,
                             const float* Wq, const float* bq, const float* gq, const float* cq,
                             const float* Wk, const float* bk, const float* gk, const float* ck,
                             const float* noise, const float* colbias, float* omega, float* qbar_rows, float* bhv,
                             float* lp, float* saved, void* stream) {
  LmkP p = {};
  int rc = fill_lmk(g, p);
  if (rc != EA_OK) return rc;
  if (!pq || !pk || !omega || !lp || g->eva || !g->mixed || !colbias) return EA_E_BADARG;
  if (g->has_mlp && (!Wq || !bq || !gq || !cq || !Wk || !bk || !gk || !ck)) return EA_E_BADARG;
  if (g->mis == EA_MIS_OPT && (!qbar_rows || !bhv)) return EA_E_BADARG;
  if (g->mis == EA_MIS_BIASED && !qbar_rows) return EA_E_BADARG;
  if (g->dup != 0 && !noise) return EA_E_BADARG;
  p.pq = pq; p.pk = pk; LMK_PARAMS(p)
  p.noise = noise; p.omega = omega; p.qbar_rows = qbar_rows; p.bhv = bhv; p.lp = lp;
  p.saved = saved; p.colbias = colbias;
  return lara_lmk_dispatch(false, p, (hipStream_t)stream);
}

int64_t ea_lara_landmarks_saved_floats(const ea_lmk_geom* g) {
  LmkP p = {};
  if (const int rc = fill_lmk(g, p)) return rc;
  return (int64_t)g->BH * (int64_t)lara_lmk_saved_per_bh(g->L, g->D);
}

// dqr_S > 1 (composite EVA backward, round 6): d_qbar_rows = slice 0 of dqr_S <= 4 slice partials `dqr_stride` floats apart
static int lara_landmarks_bwd_qparts(const ea_lmk_geom* g, const float* pq, const float* pk,
                                     const float* Wq, const float* bq, const float* gq, const float* cq,
                                     const float* Wk, const float* bk, const float* gk, const float* ck,
                                     const float* noise, const float* d_omega, const float* d_qbar_rows, int dqr_S, long dqr_stride,
                                     const float* d_bhv, const float* d_lp, float* dpq, float* dpk,
                                     float* dW_part, float* dvec_part, const float* saved, void* stream) {
  LmkP p = {};
  int rc = fill_lmk(g, p);
  if (rc != EA_OK) return rc;
  if (!pq || !pk || !d_omega || (!d_lp && !g->eva) || !dpq || !dpk) return EA_E_BADARG;
  if (g->eva && !d_qbar_rows) return EA_E_BADARG;
  if (dqr_S < 1 || dqr_S > 4 || (dqr_S > 1 && !g->eva)) return EA_E_BADARG;
  if (g->has_mlp && (!Wq || !bq || !gq || !cq || !Wk || !bk || !gk || !ck || !dW_part || !dvec_part))
    return EA_E_BADARG;
  if (g->dup != 0 && !noise) return EA_E_BADARG;
  p.pq = pq; p.pk = pk; LMK_PARAMS(p)
  p.noise = noise; p.d_omega = d_omega; p.d_qbar_rows = d_qbar_rows; p.d_bhv = d_bhv; p.d_lp = d_lp;
  p.dqr_S = dqr_S; p.dqr_stride = dqr_stride;
  p.dpq = dpq; p.dpk = dpk; p.dW_part = dW_part; p.dvec_part = dvec_part;
  p.saved = const_cast<float*>(saved);
  return lara_lmk_dispatch(true, p, (hipStream_t)stream);
}

int ea_lara_landmarks_bwd(const ea_lmk_geom* g, const float* pq, const float* pk,
                          const float* Wq, const float* bq, const float* gq, const float* cq,
                          const float* Wk, const float* bk, const float* gk, const float* ck,
                          const float* noise, const float* d_omega, const float* d_qbar_rows,
                          const float* d_bhv, const float* d_lp, float* dpq, float* dpk,
                          float* dW_part, float* dvec_part, const float* saved, void* stream) {
  return lara_landmarks_bwd_qparts(g, pq, pk, Wq, bq, gq, cq, Wk, bk, gk, ck, noise, d_omega, d_qbar_rows, 1, 0, d_bhv, d_lp, dpq,
                                   dpk, dW_part, dvec_part, saved, stream);
}

int ea_lara_landmarks_bwd_parts(const ea_lmk_geom* g, const float* pq, const float* pk,
                                const float* Wq, const float* bq, const float* gq, const float* cq,
                                const float* Wk, const float* bk, const float* gk, const float* ck,
                                const float* noise, const float* d_omega, int32_t dom_S, const float* dom_parts, float dom_scale,
                                const float* d_qbar_rows, const float* d_bhv, const float* d_lp, float* dpq, float* dpk,
                                float* dW_part, float* dvec_part, const float* saved, void* stream) {
  LmkP p = {};
  int rc = fill_lmk(g, p);
  if (rc != EA_OK) return rc;
  if (g->eva || !pq || !pk || !d_omega || !d_lp || !dpq || !dpk || !dom_parts || dom_S < 1 || dom_S > 4) return EA_E_BADARG;
  if (g->has_mlp && (!Wq || !bq || !gq || !cq || !Wk || !bk || !gk || !ck || !dW_part || !dvec_part))
    return EA_E_BADARG;
  if (g->dup != 0 && !noise) return EA_E_BADARG;
  p.pq = pq; p.pk = pk; LMK_PARAMS(p)
  p.noise = noise; p.d_omega = d_omega; p.d_qbar_rows = d_qbar_rows; p.d_bhv = d_bhv; p.d_lp = d_lp;
  p.dom_parts = dom_parts; p.dom_S = dom_S; p.dom_scale = dom_scale;
  p.dpq = dpq; p.dpk = dpk; p.dW_part = dW_part; p.dvec_part = dvec_part;
  p.saved = const_cast<float*>(saved);
  return lara_lmk_dispatch(true, p, (hipStream_t)stream);
}

int ea_lara_landmarks_bwd_cb(const ea_lmk_geom* g, const float* pq, const float* pk,
                             const float* Wq, const float* bq, const float* gq, const float* cq,
                             const float* Wk, const float* bk, const float* gk, const float* ck,
                             const float* noise, const float* colbias, const float* d_omega, const float* d_qbar_rows,
                             const float* d_bhv, const float* d_lp, float* dpq, float* dpk,
                             float* dW_part, float* dvec_part, float* d_colbias, const float* saved, void* stream) {
  LmkP p = {};
  int rc = fill_lmk(g, p);
  if (rc != EA_OK) return rc;
  if (!pq || !pk || !d_omega || !d_lp || !dpq || !dpk || g->eva || !g->mixed || !colbias || !d_colbias || !saved)
    return EA_E_BADARG;
  if (g->has_mlp && (!Wq || !bq || !gq || !cq || !Wk || !bk || !gk || !ck || !dW_part || !dvec_part))
    return EA_E_BADARG;
  if (g->dup != 0 && !noise) return EA_E_BADARG;
  p.pq = pq; p.pk = pk; LMK_PARAMS(p)
  p.noise = noise; p.d_omega = d_omega; p.d_qbar_rows = d_qbar_rows; p.d_bhv = d_bhv; p.d_lp = d_lp;
  p.dpq = dpq; p.dpk = dpk; p.dW_part = dW_part; p.dvec_part = dvec_part;
  p.saved = const_cast<float*>(saved); p.colbias = colbias; p.d_colbias = d_colbias;
  return lara_lmk_dispatch(true, p, (hipStream_t)stream);
}

}  // extern "C"

// ---- LARA partial merges ----
extern "C" {

int ea_lara_merge_fwd(int32_t BH, int32_t S, int32_t C, int32_t D, int32_t has_t,
                      const float* p_ml, const float* p_kv, const float* lp,
                      float* kv, float* lse_k, float* lse_t, float* cst, void* stream) {
  if (BH <= 0 || S <= 0 || C <= 0 || D <= 0 || !p_ml || !p_kv || !lp || !kv || !lse_k || !cst ||
      (has_t && !lse_t)) return EA_E_BADARG;
  MergeP p = {};
  p.BH = BH; p.S = S; p.C = C; p.D = D; p.has_t = has_t;
  p.p_ml = p_ml; p.p_kv = p_kv; p.lp = lp; p.kv = kv; p.lse_k = lse_k; p.lse_t = lse_t; p.cst = cst;
  return lara_merge_dispatch(false, p, (hipStream_t)stream);
}

int ea_lara_merge_bwd(int32_t BH, int32_t S, int32_t C, int32_t D, int32_t has_t, float scale,
                      const float* p_ml, const float* p_dkv, const float* p_dom, const float* p_m1,
                      const float* p_m2, const float* kv, const float* qbar,
                      float* r, float* dbh, float* dlp, float* dkk, float* dkv, float* domq,
                      float* dqbar, float* uq, void* stream) {
  if (BH <= 0 || S <= 0 || C <= 0 || D <= 0 || !p_ml || !p_dkv || !p_dom || !kv || !r || !dkk ||
      !dkv || !domq) return EA_E_BADARG;
  if (has_t && (!p_m1 || !p_m2 || !qbar || !dqbar || !uq)) return EA_E_BADARG;
  MergeP p = {};
  p.BH = BH; p.S = S; p.C = C; p.D = D; p.has_t = has_t; p.scale = scale;
  p.p_ml = p_ml; p.acc0 = p_dkv; p.acc1 = p_dom; p.acc2 = p_m1; p.acc3 = p_m2;
  p.kv = const_cast<float*>(kv); p.qbar = qbar;
  p.r = r; p.dbh = dbh; p.dlp = dlp; p.dkk = dkk; p.dkv = dkv; p.domq = domq; p.dqbar = dqbar; p.uq = uq;
  return lara_merge_dispatch(true, p, (hipStream_t)stream);
}

}  // extern "C"

// ---- projection bias gradient ----
extern "C" {

int ea_bias_grad_parts(int32_t rows, int32_t cols) { return ea::colsum_parts(rows, cols); }

int ea_bias_grad(int32_t dtype, int32_t rows, int32_t cols, const void* dy, float* part, float* db, void* stream) {
  if (!dy || !part || !db) return EA_E_BADARG;
  return ea::colsum_dispatch(dtype, dy, part, db, rows, cols, (hipStream_t)stream);
}

int ea_colsum_f32(int32_t rows, int32_t cols, const float* x, float* out, void* stream) {
  if (!x || !out) return EA_E_BADARG;
  return ea::colsum_f32_dispatch(x, out, rows, cols, nullptr, nullptr, 0, (hipStream_t)stream);
}

int ea_colsum2_f32(int32_t rows, int32_t cols1, const float* x1, float* out1, int32_t cols2, const float* x2, float* out2,
                   void* stream) {
  if (!x1 || !out1 || !x2 || !out2 || cols2 <= 0) return EA_E_BADARG;
  return ea::colsum_f32_dispatch(x1, out1, rows, cols1, x2, out2, cols2, (hipStream_t)stream);
}

int ea_gather_sum(int32_t rows, int32_t K, int32_t cols, const float* g, const int32_t* inv, float* out, void* stream) {
  if (!g || !inv || !out) return EA_E_BADARG;
  return ea::gather_sum_dispatch(g, inv, out, rows, K, cols, (hipStream_t)stream);
}

int ea_multi_cast(int32_t dtype, int32_t K, const float* const* src, const int64_t* n, void* const* dst, void* stream) {
  if (!src || !n || !dst) return EA_E_BADARG;
  return ea::multi_cast_dispatch(dtype, K, src, (const long long*)n, dst, (hipStream_t)stream);
}

int ea_table_bias_fwd(int32_t h, int32_t th, int32_t Wq, int32_t Wk, int32_t ld, float scale, const float* table, const int32_t* idx,
                      float* out, void* stream) {
  if (!table || !idx || !out) return EA_E_BADARG;
  return ea::table_bias_fwd_dispatch(table, idx, out, h, th, Wq, Wk, ld, scale, (hipStream_t)stream);
}

int ea_table_bias_bwd(int32_t rows, int32_t K, int32_t h, int32_t Wq, int32_t Wk, int32_t ld, float scale, const float* g,
                      const int32_t* inv, float* dtable, void* stream) {
  if (!g || !inv || !dtable) return EA_E_BADARG;
  return ea::table_bias_bwd_dispatch(g, inv, dtable, rows, K, h, Wq, Wk, ld, scale, (hipStream_t)stream);
}


int ea_stream_copy(const void* src, void* dst, int64_t bytes, void* stream) {
  if (!src || !dst || bytes <= 0 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return EA_E_BADARG;
  return ea::stream_copy_dispatch(src, dst, (size_t)bytes, (hipStream_t)stream);
}

int ea_slice_sum(int32_t BH, int32_t S, int32_t n, float scale, const float* a, const float* parts,
                 float* out, void* stream) {
  if (!parts || !out) return EA_E_BADARG;
  return ea::slice_sum_dispatch(a, parts, out, BH, S, n, scale, (hipStream_t)stream);
}

// ---- LARA 1-D landmark proposals: segment means of (LayerNorm'd) rows ----
static int fill_seg(const ea_geom* g, SegP& p) {
  if (!g || g->B <= 0 || g->H <= 0 || g->N <= 0 || g->L <= 0 || g->D <= 0 ||
      (g->dtype != EA_BF16 && g->dtype != EA_F16 && g->dtype != EA_F32)) return EA_E_BADARG;
  // a well-formed geometry the kernels are not built for (include/ea_hip.h: EA_E_UNSUPPORTED), as lara_segment_dispatch and
  // seglin_dispatch class it themselves
  if ((g->D != 32 && g->D != 64) || g->dtype == EA_F32) return EA_E_UNSUPPORTED;
  if (g->N <= g->L) return EA_E_UNSUPPORTED;            // the reference uses the rows themselves then
  p.B = g->B; p.H = g->H; p.N = g->N; p.L = g->L;
  p.segs = g->N / g->L;
  p.nshort = g->N % g->L == 0 ? g->L : (p.segs + 1) * g->L - g->N;   // lara.py:111-124
  return EA_OK;
}

int ea_lara_segment_fwd(const ea_geom* g, const ea_t4* q2, const ea_t4* k2, const uint8_t* mask,
                        const float* bias_q, const float* bias_k, const float* mbias_q, const float* mbias_k,
                        const float* gq, const float* cq, const float* gk, const float* ck,
                        float* qbar, float* kbar, void* stream) {
  SegP p = {};
  int rc = fill_seg(g, p);
  if (rc != EA_OK) return rc;
  if (!t4_ok32(q2, g->D, g->N) || !t4_ok32(k2, g->D, g->N) || !qbar || !kbar) return EA_E_BADARG;
  if ((gq == nullptr) != (gk == nullptr) || (gq && (!cq || !ck))) return EA_E_BADARG;
  SET3(q, q2); SET3(k, k2);
  p.mask = mask; p.bias_q = bias_q; p.bias_k = bias_k; p.mbias_q = mbias_q; p.mbias_k = mbias_k;
  p.gq = gq; p.cq = cq; p.gk = gk; p.ck = ck; p.qbar = qbar; p.kbar = kbar;
  return lara_segment_dispatch(false, p, g->dtype, g->D, (hipStream_t)stream);
}

int ea_lara_segment_bwd(const ea_geom* g, const ea_t4* q2, const ea_t4* k2, const uint8_t* mask,
                        const float* bias_q, const float* bias_k, const float* mbias_q, const float* mbias_k,
                        const float* gq, const float* cq, const float* gk, const float* ck,
                        const float* d_qbar, const float* d_kbar, const ea_t4* dq2, const ea_t4* dk2,
                        float* part, void* stream) {
  SegP p = {};
  int rc = fill_seg(g, p);
  if (rc != EA_OK) return rc;
  if (!t4_ok32(q2, g->D, g->N) || !t4_ok32(k2, g->D, g->N) || !t4_ok32(dq2, g->D, g->N) ||
      !t4_ok32(dk2, g->D, g->N) || !d_qbar || !d_kbar) return EA_E_BADARG;
  if ((gq == nullptr) != (gk == nullptr) || (gq && (!cq || !ck || !part))) return EA_E_BADARG;
  SET3(q, q2); SET3(k, k2); SET3(dq, dq2); SET3(dk, dk2);
  p.mask = mask; p.bias_q = bias_q; p.bias_k = bias_k; p.mbias_q = mbias_q; p.mbias_k = mbias_k;
  p.gq = gq; p.cq = cq; p.gk = gk; p.ck = ck; p.d_qbar = d_qbar; p.d_kbar = d_kbar; p.part = part;
  return lara_segment_dispatch(true, p, g->dtype, g->D, (hipStream_t)stream);
}

}  // extern "C"

// ---- LARA 'adaptive-1d' with the generator Linear inside the segment kernels (ea_lara_seglin.hip) ----
static int fill_seglin(const ea_geom* g, ea::SegLinP& p) {
  SegP sp = {};
  const int rc = fill_seg(g, sp);
  if (rc != EA_OK) return rc;
  if (g->D != 64) return EA_E_UNSUPPORTED;
  p.B = sp.B; p.H = sp.H; p.N = sp.N; p.L = sp.L; p.segs = sp.segs; p.nshort = sp.nshort;
  return EA_OK;
}

extern "C" {

int32_t ea_lara_seglin_groups(const ea_geom* g) {
  ea::SegLinP p = {};
  const int rc = fill_seglin(g, p);
  return rc != EA_OK ? rc : ea::seglin_groups(p.B * p.H, p.L);
}

int ea_lara_seglin_fwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const float* Gq, const float* gq_b, const float* Gk,
                       const float* gk_b, const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                       float* qbar, float* kbar, void* stream) {
  ea::SegLinP p = {};
  const int rc = fill_seglin(g, p);
  if (rc != EA_OK) return rc;
  if (!t4_ok32(q, 64, g->N) || !t4_ok32(k, 64, g->N) || !Gq || !gq_b || !Gk || !gk_b || !lnq_w || !lnq_b || !lnk_w || !lnk_b ||
      !qbar || !kbar) return EA_E_BADARG;
  SET3(q, q); SET3(k, k);
  p.Gq = Gq; p.gqb = gq_b; p.Gk = Gk; p.gkb = gk_b; p.lnq_w = lnq_w; p.lnq_b = lnq_b; p.lnk_w = lnk_w; p.lnk_b = lnk_b;
  p.qbar = qbar; p.kbar = kbar;
  return ea::seglin_dispatch(0, p, g->dtype, (hipStream_t)stream);
}

static int seglin_bwd_impl(const ea_geom* g, const ea_t4* q, const ea_t4* k, const float* Gq, const float* gq_b, const float* Gk,
                           const float* gk_b, const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                           const float* d_qbar, const float* d_kbar, const ea_t4* dq, const ea_t4* dk, float* part, float* dG_part,
                           float* stats, const float* fin_qbar, const float* fin_uq, const float* fin_lse, int32_t C, float scale,
                           bool fin, void* stream) {
  ea::SegLinP p = {};
  int rc = fill_seglin(g, p);
  if (rc != EA_OK) return rc;
  if (!t4_ok32(q, 64, g->N) || !t4_ok32(k, 64, g->N) || !t4_ok32(dq, 64, g->N) || !t4_ok32(dk, 64, g->N) || !Gq || !gq_b || !Gk ||
      !gk_b || !lnq_w || !lnq_b || !lnk_w || !lnk_b || !d_qbar || !d_kbar || !part || !dG_part || !stats || ((uintptr_t)stats & 15))
    return EA_E_BADARG;
  if (fin) {
    if (!fin_qbar || !fin_uq || !fin_lse || C < 1 || !(scale > 0.f)) return EA_E_BADARG;
    if (C > 64) return EA_E_UNSUPPORTED;
    p.fin_qbar = fin_qbar; p.fin_uq = fin_uq; p.fin_lse = fin_lse; p.C = C;
    p.fin_scale = scale; p.fin_scale_log2 = scale * 1.4426950408889634f;
  }
  SET3(q, q); SET3(k, k); SET3(dq, dq); SET3(dk, dk);
  p.Gq = Gq; p.gqb = gq_b; p.Gk = Gk; p.gkb = gk_b; p.lnq_w = lnq_w; p.lnq_b = lnq_b; p.lnk_w = lnk_w; p.lnk_b = lnk_b;
  p.d_qbar = d_qbar; p.d_kbar = d_kbar; p.part = part; p.dG_part = dG_part; p.stats = reinterpret_cast<f32x4*>(stats);
  rc = ea::seglin_dispatch(fin ? 3 : 1, p, g->dtype, (hipStream_t)stream);
  if (rc != EA_OK) return rc;
  return ea::seglin_dispatch(2, p, g->dtype, (hipStream_t)stream);
}

int ea_lara_seglin_bwd(const ea_geom* g, const ea_t4* q, const ea_t4* k, const float* Gq, const float* gq_b, const float* Gk,
                       const float* gk_b, const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                       const float* d_qbar, const float* d_kbar, const ea_t4* dq, const ea_t4* dk, float* part, float* dG_part,
                       float* stats, void* stream) {
  return seglin_bwd_impl(g, q, k, Gq, gq_b, Gk, gk_b, lnq_w, lnq_b, lnk_w, lnk_b, d_qbar, d_kbar, dq, dk, part, dG_part, stats,
                         nullptr, nullptr, nullptr, 0, 0.f, false, stream);
}

int ea_lara_seglin_bwd_fin(const ea_geom* g, const ea_t4* q, const ea_t4* k, const float* Gq, const float* gq_b, const float* Gk,
                           const float* gk_b, const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                           const float* d_qbar, const float* d_kbar, const ea_t4* dq, const ea_t4* dk, float* part,
                           float* dG_part, float* stats, const float* fin_qbar, const float* fin_uq, const float* fin_lse_t,
                           int32_t C, float scale, void* stream) {
  return seglin_bwd_impl(g, q, k, Gq, gq_b, Gk, gk_b, lnq_w, lnq_b, lnk_w, lnk_b, d_qbar, d_kbar, dq, dk, part, dG_part, stats,
                         fin_qbar, fin_uq, fin_lse_t, C, scale, true, stream);
}

}  // extern "C"

// ---- mu networks: per-row Linear (+ LayerNorm) on the chunk means ----
extern "C" {

int32_t ea_rows_mlp_parts(int32_t R, int32_t D) {
  if (R <= 0 || (D != 32 && D != 64 && D != 128)) return EA_E_BADARG;
  return ea::rows_mlp_blocks(R, D);
}

int ea_rows_mlp_fwd(int32_t R, int32_t D, int32_t sides, int32_t layer_norm,
                    const float* x0, const float* x1, const float* W0, const float* W1,
                    const float* b0, const float* b1, const float* g0, const float* g1,
                    const float* c0, const float* c1, float* y0, float* y1,
                    float* zhat, float* rstd, void* stream) {
  if (R <= 0 || sides < 1 || sides > 2 || !x0 || !W0 || !b0 || !y0) return EA_E_BADARG;
  if (sides == 2 && (!x1 || !W1 || !b1 || !y1)) return EA_E_BADARG;
  if (layer_norm && (!g0 || !c0 || (sides == 2 && (!g1 || !c1)))) return EA_E_BADARG;
  if ((zhat == nullptr) != (rstd == nullptr)) return EA_E_BADARG;
  RowsP p = {};
  p.R = R;
  p.x[0] = x0; p.x[1] = x1; p.W[0] = W0; p.W[1] = W1; p.b[0] = b0; p.b[1] = b1;
  p.g[0] = g0; p.g[1] = g1; p.c[0] = c0; p.c[1] = c1; p.y[0] = y0; p.y[1] = y1;
  p.zhat = zhat; p.rstd = rstd;
  return ea::rows_mlp_dispatch(p, D, sides, layer_norm, false, (hipStream_t)stream);
}

int ea_rows_mlp_bwd(int32_t R, int32_t D, int32_t sides, int32_t layer_norm,
                    const float* dy0, const float* dy1, const float* x0, const float* x1,
                    const float* W0, const float* W1, const float* g0, const float* g1,
                    const float* zhat, const float* rstd, float* dx0, float* dx1,
                    float* feed, float* dW_part, void* stream) {
  if (R <= 0 || sides < 1 || sides > 2 || !dy0 || !x0 || !W0 || !dx0 || !feed || !dW_part) return EA_E_BADARG;
  if (sides == 2 && (!dy1 || !x1 || !W1 || !dx1)) return EA_E_BADARG;
  if (layer_norm && (!g0 || !zhat || !rstd || (sides == 2 && !g1))) return EA_E_BADARG;
  RowsP p = {};
  p.R = R;
  p.dy[0] = dy0; p.dy[1] = dy1; p.x[0] = x0; p.x[1] = x1; p.W[0] = W0; p.W[1] = W1;
  p.g[0] = g0; p.g[1] = g1; p.zhat = const_cast<float*>(zhat); p.rstd = const_cast<float*>(rstd);
  p.dx[0] = dx0; p.dx[1] = dx1; p.feed = feed; p.dW_part = dW_part;
  return ea::rows_mlp_dispatch(p, D, sides, layer_norm, true, (hipStream_t)stream);
}

}  // extern "C"

// ---- projection weight + bias gradient (ea_wgrad.hip) ----
extern "C" {

int32_t ea_wgrad_parts(int32_t rows, int32_t out_features, int32_t in_features) {
  return wgrad_slices(rows, out_features, in_features);
}

int ea_wgrad(int32_t dtype, int32_t rows, int32_t out_features, int32_t in_features, const void* dy, const void* x,
             float* dw_part, float* db_part, int64_t part_ld, void* stream) {
  if (!dy || !x || !dw_part || ((uintptr_t)dy & 15) || ((uintptr_t)x & 15) || ((uintptr_t)dw_part & 15)) return EA_E_BADARG;
  if (part_ld < (int64_t)out_features * in_features || (part_ld & 3)) return EA_E_BADARG;
  return wgrad_dispatch(dtype, dy, x, dw_part, db_part, (long)part_ld, rows, out_features, in_features, (hipStream_t)stream);
}

int32_t ea_wgrad_pair_parts(int32_t rows, int32_t out1, int32_t in1, int32_t out2, int32_t in2) {
  return wgrad_pair_slices(rows, out1, in1, out2, in2);
}

int ea_wgrad_pair(int32_t dtype, int32_t rows, int32_t out1, int32_t in1, const void* dy1, const void* x1, float* dw_part1,
                  float* db_part1, int64_t part_ld1, int32_t out2, int32_t in2, const void* dy2, const void* x2,
                  float* dw_part2, float* db_part2, int64_t part_ld2, void* stream) {
  if ((dtype != EA_BF16 && dtype != EA_F16) || rows <= 0 || !dy1 || !x1 || !dw_part1 || !dy2 || !x2 || !dw_part2) return EA_E_BADARG;
  if (part_ld1 < (int64_t)out1 * in1 || part_ld2 < (int64_t)out2 * in2 || (part_ld1 & 3) || (part_ld2 & 3)) return EA_E_BADARG;
  if (((uintptr_t)dy1 | (uintptr_t)x1 | (uintptr_t)dw_part1 | (uintptr_t)dy2 | (uintptr_t)x2 | (uintptr_t)dw_part2) & 15)
    return EA_E_BADARG;
  return wgrad_pair_dispatch(dtype, rows, dy1, x1, dw_part1, db_part1, (long)part_ld1, out1, in1, dy2, x2, dw_part2, db_part2,
                             (long)part_ld2, out2, in2, (hipStream_t)stream);
}

int ea_part_sum(int32_t S, int32_t n, int64_t ld, const float* parts, float* out, void* stream) {
  if (!parts || !out || ((uintptr_t)parts & 15) || ((uintptr_t)out & 15)) return EA_E_BADARG;
  return part_sum_dispatch(parts, out, S, n, (long)ld, (hipStream_t)stream);
}

int ea_multi_sum(int32_t K, const float* const* parts, const int32_t* S, const int32_t* n, const int64_t* ld, float* const* out,
                 void* stream) {
  if (!parts || !S || !n || !ld || !out) return EA_E_BADARG;
  return multi_sum_dispatch(K, parts, S, n, (const long long*)ld, out, (hipStream_t)stream);
}

}  // extern "C"

// ---- LARA sampling + proposal densities beyond the fused landmark kernels (ea_lara_segment.hip) ----
extern "C" {

int ea_lara_sample_fwd(int32_t BH, int32_t L, int32_t C, int32_t D, int32_t mis, int32_t mode, float scale,
                       const float* qbar, const float* mu, const float* noise, float* omega, float* qbar_rows, float* bhv,
                       float* lp, void* stream) {
  if (!qbar || !mu || !omega || !lp || (mode != 0 && !noise) || mis < 0 || mis > 2) return EA_E_BADARG;
  if (mis == EA_MIS_OPT && (!qbar_rows || !bhv)) return EA_E_BADARG;
  if (mis == EA_MIS_BIASED && !qbar_rows) return EA_E_BADARG;
  if ((mode == 0) != (C == L) || (mode != 0 && C != 2 * L)) return EA_E_BADARG;
  ea::SampP p = {};
  p.qbar = qbar; p.mu = mu; p.noise = noise; p.omega = omega; p.qrows = mis == EA_MIS_BH ? nullptr : qbar_rows;
  p.bhv = mis == EA_MIS_OPT ? bhv : nullptr; p.lp = lp;
  p.BH = BH; p.L = L; p.C = C; p.D = D; p.mis = mis; p.mode = mode; p.scale = scale;
  return ea::lara_sample_dispatch(false, p, (hipStream_t)stream);
}

int ea_lara_sample_bwd(int32_t BH, int32_t L, int32_t C, int32_t D, int32_t mis, int32_t mode, float scale,
                       const float* qbar, const float* mu, const float* noise, const float* d_omega, const float* d_qbar_rows,
                       const float* d_bhv, const float* d_lp, float* d_qbar, float* d_mu, void* stream) {
  if (!qbar || !mu || !d_omega || !d_qbar || !d_mu || (mode != 0 && !noise) || mis < 0 || mis > 2) return EA_E_BADARG;
  if ((mode == 0) != (C == L) || (mode != 0 && C != 2 * L)) return EA_E_BADARG;
  ea::SampP p = {};
  p.qbar = qbar; p.mu = mu; p.noise = noise;
  p.d_omega = d_omega; p.d_qrows = mis == EA_MIS_BH ? nullptr : d_qbar_rows; p.d_bhv = mis == EA_MIS_OPT ? d_bhv : nullptr;
  p.d_lp = d_lp; p.d_qbar = d_qbar; p.d_mu = d_mu;
  p.BH = BH; p.L = L; p.C = C; p.D = D; p.mis = mis; p.mode = mode; p.scale = scale;
  return ea::lara_sample_dispatch(true, p, (hipStream_t)stream);
}

}  // extern "C"

// ---- adaptive 2-D pooling of a token grid that does not divide evenly (ea_lara_segment.hip) ----
extern "C" {

int ea_adaptive_pool2d_fwd(int32_t dtype, int32_t B, int32_t H, int32_t gh, int32_t gw, int32_t side, int32_t D,
                           const ea_t4* x, float* mean, void* stream) {
  if (!x || !x->ptr || !mean) return EA_E_BADARG;
  return pool2d_dispatch(false, dtype, x->ptr, (long)x->sb, (long)x->sh, (long)x->sn, mean, B, H, gh, gw, side, D,
                         (hipStream_t)stream);
}

int ea_adaptive_pool2d_bwd(int32_t dtype, int32_t B, int32_t H, int32_t gh, int32_t gw, int32_t side, int32_t D,
                           const float* dmean, const ea_t4* dx, void* stream) {
  if (!dx || !dx->ptr || !dmean) return EA_E_BADARG;
  return pool2d_dispatch(true, dtype, dx->ptr, (long)dx->sb, (long)dx->sh, (long)dx->sn, const_cast<float*>(dmean), B, H, gh,
                         gw, side, D, (hipStream_t)stream);
}

}  // extern "C"

// ---- LARA 'adaptive-1d': the generators' Linear folded into the qkv projection (ea_fold.hip) ----
extern "C" {

int ea_lara_fold_fwd(int32_t dtype, int32_t C, int32_t heads, const float* W, const float* b, const float* Gq, const float* gq_b,
                     const float* Gk, const float* gk_b, void* w_ext, void* b_ext, float* bias_q, float* bias_k, void* stream) {
  if (!W || !Gq || !Gk || !gq_b || !gk_b || !w_ext || !bias_q || !bias_k || heads <= 0 || C % heads) return EA_E_BADARG;
  ea::FoldP p = {};
  p.W = W; p.b = b; p.Gq = Gq; p.Gk = Gk; p.gqb = gq_b; p.gkb = gk_b; p.w_ext = (char*)w_ext; p.b_ext = (char*)b_ext;
  p.bias_q = bias_q; p.bias_k = bias_k; p.C = C; p.h = heads; p.d = C / heads;
  return ea::fold_dispatch(false, dtype, p, (hipStream_t)stream);
}

int32_t ea_lara_fold_parts(int32_t heads) { return ea::fold_bwd_parts(heads); }

int ea_lara_fold_bwd(int32_t C, int32_t heads, const float* W, const float* b, const float* Gq, const float* Gk,
                     const float* dW_ext, int64_t ldw, const float* db_ext, const float* dbias_q, const float* dbias_k,
                     float* dW, float* db, float* dG, float* dG_part, float* dgq_b, float* dgk_b, void* stream) {
  if (!W || !Gq || !Gk || !dW_ext || !dbias_q || !dbias_k || !dW || !dG || !dG_part || !dgq_b || !dgk_b || heads <= 0 ||
      C % heads || ldw < C) return EA_E_BADARG;
  ea::FoldP p = {};
  p.W = W; p.b = b; p.Gq = Gq; p.Gk = Gk; p.dW_ext = dW_ext; p.ldw = (long)ldw; p.db_ext = db_ext; p.dbias_q = dbias_q;
  p.dbias_k = dbias_k; p.dW = dW; p.db = db; p.dgqb = dgq_b; p.dgkb = dgk_b;
  p.C = C; p.h = heads; p.d = C / heads;
  // the bias part of dG goes to a scratch behind the partials; one slice sum adds everything up into dG [2, d, d]
  const int S = ea::fold_bwd_parts(heads);
  const size_t dd = (size_t)p.d * p.d;
  p.dG_part = dG_part; p.dG_base = dG_part + (size_t)2 * S * dd;
  int rc = ea::fold_dispatch(true, 0, p, (hipStream_t)stream);
  if (rc != EA_OK) return rc;
  return ea_slice_sum(2, S, (int32_t)dd, 1.0f, p.dG_base, dG_part, dG, stream);
}

}  // extern "C"

// ---- Performer in exact fp32 arithmetic (ea_performer_f32.hip) ----
static int pf_fill(const ea_perf_geom* g, Pf32P& p) {
  if (!g || g->B <= 0 || g->H <= 0 || g->N <= 0 || g->dtype < 0 || g->dtype > EA_F32) return EA_E_BADARG;
  if (g->D != 64 || g->M <= 0 || g->M > PF32_MAX_M || (g->M & 15)) return EA_E_UNSUPPORTED;
  p.B = g->B; p.H = g->H; p.N = g->N; p.M = g->M; p.dtype = g->dtype;
  return EA_OK;
}

extern "C" {

int32_t ea_performer_f32_parts(const ea_perf_geom* g) {
  Pf32P p = {};
  const int rc = pf_fill(g, p);
  return rc != EA_OK ? rc : f32tile::plan_slices(g->B * g->H, g->N).S;
}

int ea_performer_f32_kmax(const ea_perf_geom* g, const ea_t4* k, const float* W, float* p_max, void* stream) {
  Pf32P p = {};
  const int rc = pf_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(k, 64, esz) || !W || !p_max) return EA_E_BADARG;
  p.k = mk(k); p.W = W; p.p_max = p_max;
  return pf32_dispatch(0, p, (hipStream_t)stream);
}

int ea_performer_f32_kv(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                        const float* p_max, float* p_kv, float* p_ksum, void* stream) {
  Pf32P p = {};
  const int rc = pf_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(k, 64, esz) || !view_ok(v, 64, esz) || !W || !p_max || !p_kv || !p_ksum) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.mask = mask; p.W = W; p.p_max = const_cast<float*>(p_max); p.p_kv = p_kv; p.p_ks = p_ksum;
  return pf32_dispatch(1, p, (hipStream_t)stream);
}

int ea_performer_f32_out(const ea_perf_geom* g, const ea_t4* q, const float* W, const float* kv, const float* ksum,
                         const ea_t4* out, void* stream) {
  Pf32P p = {};
  const int rc = pf_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(q, 64, esz) || !view_ok(out, 64, esz) || !W || !kv || !ksum) return EA_E_BADARG;
  p.q = mk(q); p.o = mk(out); p.W = W; p.kv = kv; p.ksum = ksum;
  return pf32_dispatch(2, p, (hipStream_t)stream);
}

int ea_performer_f32_bwd_q(const ea_perf_geom* g, const ea_t4* q, const ea_t4* dout, const float* W, const float* kv,
                           const float* ksum, const ea_t4* dq, float* p_dkv, float* p_dksum, void* stream) {
  Pf32P p = {};
  const int rc = pf_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(q, 64, esz) || !view_ok(dout, 64, esz) || !view_ok(dq, 64, esz) || !W || !kv || !ksum || !p_dkv || !p_dksum)
    return EA_E_BADARG;
  p.q = mk(q); p.dout = mk(dout); p.dq = mk(dq); p.W = W; p.kv = kv; p.ksum = ksum; p.p_kv = p_dkv; p.p_ks = p_dksum;
  return pf32_dispatch(3, p, (hipStream_t)stream);
}

int ea_performer_f32_bwd_k(const ea_perf_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                           const float* p_max, const float* dkv, const float* dksum, const ea_t4* dk, const ea_t4* dv,
                           void* stream) {
  Pf32P p = {};
  const int rc = pf_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(k, 64, esz) || !view_ok(v, 64, esz) || !view_ok(dk, 64, esz) || !view_ok(dv, 64, esz) || !W || !p_max ||
      !dkv || !dksum) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.mask = mask; p.W = W; p.p_max = const_cast<float*>(p_max); p.dkv = dkv; p.dksum = dksum;
  p.dk = mk(dk); p.dv = mk(dv);
  return pf32_dispatch(4, p, (hipStream_t)stream);
}

}  // extern "C"

// ---- kernelized attention, every feature map (ea_kernelized.hip) ----
static int kz_fill(const ea_kz_geom* g, KzP& p) {
  if (!g || g->B <= 0 || g->H <= 0 || g->N <= 0 || g->dtype < 0 || g->dtype > EA_F32 || g->map < EA_KZ_FAVORP ||
      g->map > EA_KZ_DPFP || (g->cos != 0 && g->cos != 1)) return EA_E_BADARG;
  const bool w = kz_has_w(g->map);
  if (g->D != 64 || (w && (g->M <= 0 || g->M > KZ_MAX_M || (g->M & 15))) || (g->map == EA_KZ_DPFP && g->nu < 1))
    return EA_E_UNSUPPORTED;
  const int Fb = kz_base_features(g->map, g->M, g->nu);
  if (g->F != Fb * (g->cos ? 2 : 1) || g->F > KZ_MAX_F) return EA_E_UNSUPPORTED;
  p.B = g->B; p.H = g->H; p.N = g->N; p.M = w ? g->M : 16; p.F = g->F; p.Fb = Fb; p.nu = g->nu; p.cos = g->cos;
  p.map = g->map; p.dtype = g->dtype;
  return EA_OK;
}
static bool kz_w_ok(const ea_kz_geom* g, const float* W) { return g->map > EA_KZ_FOURIER || W != nullptr; }
static bool kz_st_ok(const ea_kz_geom* g, const float* p_st) {
  return (g->map != EA_KZ_FAVORP && g->map != EA_KZ_FOURIER) || p_st != nullptr;
}

extern "C" {

int32_t ea_kernelized_parts(const ea_kz_geom* g) {
  KzP p = {};
  const int rc = kz_fill(g, p);
  return rc != EA_OK ? rc : f32tile::plan_slices(g->B * g->H, g->N).S;
}

int ea_kernelized_stats(const ea_kz_geom* g, const ea_t4* q, const ea_t4* k, const float* W, float* p_st, void* stream) {
  KzP p = {};
  const int rc = kz_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (g->map != EA_KZ_FAVORP && g->map != EA_KZ_FOURIER) return EA_E_BADARG;
  if (!view_ok(k, 64, esz) || (g->map == EA_KZ_FOURIER && !view_ok(q, 64, esz)) || !kz_w_ok(g, W) || !p_st)
    return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.W = W; p.p_st = p_st;
  return kz_dispatch(0, p, (hipStream_t)stream);
}

int ea_kernelized_kv(const ea_kz_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                     const float* p_st, float* p_kv, float* p_ksum, void* stream) {
  KzP p = {};
  const int rc = kz_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(k, 64, esz) || !view_ok(v, 64, esz) || !kz_w_ok(g, W) || !kz_st_ok(g, p_st) || !p_kv || !p_ksum)
    return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.mask = mask; p.W = W; p.p_st = const_cast<float*>(p_st); p.p_kv = p_kv; p.p_ks = p_ksum;
  return kz_dispatch(1, p, (hipStream_t)stream);
}

int ea_kernelized_out(const ea_kz_geom* g, const ea_t4* q, const float* W, const float* p_st, const float* kv,
                      const float* ksum, const ea_t4* out, void* stream) {
  KzP p = {};
  const int rc = kz_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(q, 64, esz) || !view_ok(out, 64, esz) || !kz_w_ok(g, W) || !kz_st_ok(g, p_st) || !kv || !ksum)
    return EA_E_BADARG;
  p.q = mk(q); p.o = mk(out); p.W = W; p.p_st = const_cast<float*>(p_st); p.kv = kv; p.ksum = ksum;
  return kz_dispatch(2, p, (hipStream_t)stream);
}

int ea_kernelized_bwd_q(const ea_kz_geom* g, const ea_t4* q, const ea_t4* dout, const float* W, const float* p_st,
                        const float* kv, const float* ksum, const ea_t4* dq, float* p_dkv, float* p_dksum, float* p_dw,
                        void* stream) {
  KzP p = {};
  const int rc = kz_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(q, 64, esz) || !view_ok(dout, 64, esz) || !view_ok(dq, 64, esz) || !kz_w_ok(g, W) || !kz_st_ok(g, p_st) ||
      !kv || !ksum || !p_dkv || !p_dksum || (p_dw && g->map > EA_KZ_FOURIER)) return EA_E_BADARG;
  p.q = mk(q); p.dout = mk(dout); p.dq = mk(dq); p.W = W; p.p_st = const_cast<float*>(p_st); p.kv = kv; p.ksum = ksum;
  p.p_kv = p_dkv; p.p_ks = p_dksum; p.p_dw = p_dw;
  return kz_dispatch(3, p, (hipStream_t)stream);
}

int ea_kernelized_bwd_k(const ea_kz_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                        const float* p_st, const float* dkv, const float* dksum, const ea_t4* dk, const ea_t4* dv,
                        float* p_dw, void* stream) {
  KzP p = {};
  const int rc = kz_fill(g, p);
  if (rc != EA_OK) return rc;
  const int esz = g->dtype == EA_F32 ? 4 : 2;
  if (!view_ok(k, 64, esz) || !view_ok(v, 64, esz) || !view_ok(dk, 64, esz) || !view_ok(dv, 64, esz) ||
      !kz_w_ok(g, W) || !kz_st_ok(g, p_st) || !dkv || !dksum || (p_dw && g->map > EA_KZ_FOURIER)) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.mask = mask; p.W = W; p.p_st = const_cast<float*>(p_st); p.dkv = dkv; p.dksum = dksum;
  p.dk = mk(dk); p.dv = mk(dv); p.p_dw = p_dw;
  return kz_dispatch(4, p, (hipStream_t)stream);
}

}  // extern "C"

// ---- projections as streaming kernels (ea_linear.hip) ----
extern "C" {

int32_t ea_linear_supported(int32_t in_features, int32_t out_features) { return linear_supported(in_features, out_features); }

int ea_linear(int32_t dtype, int32_t rows, int32_t in_features, int32_t out_features, const void* a, int32_t a_f32,
              int64_t lda, const void* w, const float* bias, void* y, int32_t y_f32, int64_t ldy, void* a_cast,
              void* stream) {
  if (!a || !w || !y || ((uintptr_t)a & 15) || ((uintptr_t)w & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15) ||
      ((uintptr_t)a_cast & 15))
    return EA_E_BADARG;
  if (lda < in_features || ldy < out_features || (lda & 7) || (ldy & 7)) return EA_E_BADARG;
  return linear_dispatch(dtype, a, a_f32, w, 0, bias, y, y_f32, a_cast, rows, in_features, out_features, (long)lda,
                         (long)ldy, (hipStream_t)stream);
}

int ea_linear_w32(int32_t dtype, int32_t rows, int32_t in_features, int32_t out_features, const void* a, int32_t a_f32,
                  int64_t lda, const float* w, int32_t w_transposed, const float* bias, void* y, int32_t y_f32, int64_t ldy,
                  void* a_cast, void* stream) {
  if (!a || !w || !y || ((uintptr_t)a & 15) || ((uintptr_t)w & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15) ||
      ((uintptr_t)a_cast & 15))
    return EA_E_BADARG;
  if (lda < in_features || ldy < out_features || (lda & 7) || (ldy & 7)) return EA_E_BADARG;
  // the qkv projection of a 192-wide model: weight resident in registers, activations through LDS once (ea_proj_rs.hip)
  static const bool rs_on = !(getenv("EA_PROJ_RS") && getenv("EA_PROJ_RS")[0] == '0');
  // (a workgroup first loads the whole 576 x 192 weight into its registers: worth it from ~8 token tiles per workgroup on --
  //  at N = 196 x batch 128 the LDS-resident kernel is faster, 25.7 against 30.1 us)
  if (rs_on && !w_transposed && !y_f32 && rows >= 65536 && proj_rs_supported(in_features, out_features))
    return proj_rs_dispatch(dtype, a, a_f32, w, bias, y, a_cast, rows, (long)lda, (long)ldy, (hipStream_t)stream, 0, 0, 0, 0,
                            nullptr, nullptr, nullptr, nullptr);
  return linear_dispatch(dtype, a, a_f32, w, w_transposed ? 2 : 1, bias, y, y_f32, a_cast, rows, in_features, out_features,
                         (long)lda, (long)ldy, (hipStream_t)stream);
}

// input gradient of the 192 -> 576 projection, weight resident in registers (ea_dgrad_rs.hip)
int32_t ea_linear_dgrad_supported(int32_t in_features, int32_t out_features) {
  return dgrad_rs_supported(out_features, in_features);
}

int ea_linear_dgrad(int32_t dtype, int32_t rows, int32_t in_features, int32_t out_features, const void* dy, int64_t ldy,
                    const void* w, int32_t w_f32, void* dx, int32_t dx_f32, int64_t ldx, void* stream) {
  if (!dy || !w || !dx || ((uintptr_t)dy & 15) || ((uintptr_t)w & 15) || ((uintptr_t)dx & 15)) return EA_E_BADARG;
  if (rows < 0 || ldy < out_features || ldx < in_features || (ldy & 7) || (ldx & 3) || (!dx_f32 && (ldx & 7))) return EA_E_BADARG;
  if (!dgrad_rs_supported(out_features, in_features)) return EA_E_UNSUPPORTED;
  if ((int64_t)rows * ldy >= ((int64_t)1 << 40)) return EA_E_BADARG;
  return dgrad_rs_dispatch(dtype, dy, w, w_f32, dx, dx_f32, rows, (long)ldy, (long)ldx, (hipStream_t)stream);
}

// the same product fused with the last corrections of dq / dk (ea_dgrad_rs.hip, dgrad_fin_kernel)
int ea_linear_dgrad_finish(int32_t dtype, int32_t B, int32_t gh, int32_t gw, int32_t pool_r, int32_t C, float scale,
                           void* dqkv, int64_t ldy, const void* qkv, int64_t ldq, const void* w, int32_t w_f32, void* dx,
                           int32_t dx_f32, int64_t ldx, const float* qbar, const float* uq, const float* lse_t,
                           const float* dpq, const float* dpk, void* stream) {
  if (!dqkv || !w || !dx || ((uintptr_t)dqkv & 15) || ((uintptr_t)w & 15) || ((uintptr_t)dx & 15) || ((uintptr_t)qkv & 15))
    return EA_E_BADARG;
  if (B <= 0 || gh <= 0 || gw <= 0 || ldy < 576 || ldx < 192 || (ldy & 7) || (ldx & 3) || (!dx_f32 && (ldx & 7))) return EA_E_BADARG;
  if ((dpq == nullptr) != (dpk == nullptr)) return EA_E_BADARG;
  if (dpq && (pool_r <= 0 || gh % pool_r || gw % pool_r)) return EA_E_BADARG;
  if (uq && (!qkv || !qbar || !lse_t || ldq < 192 || (ldq & 7) || C <= 0)) return EA_E_BADARG;
  if (uq && C > 64) return EA_E_UNSUPPORTED;
  if (!uq && !dpq) return EA_E_BADARG;                        // nothing to correct: ea_linear_dgrad
  if ((int64_t)B * gh * gw >= ((int64_t)1 << 31)) return EA_E_BADARG;
  return dgrad_fin_launch(dtype, dqkv, (long)ldy, qkv, (long)ldq, w, w_f32, dx, dx_f32, (long)ldx, B, gh, gw, pool_r, C, scale,
                          qbar, uq, lse_t, dpq, dpk, (hipStream_t)stream);
}

// qkv projection + pooled q / k rows in one pass (ea_proj_rs.hip, POOL variants)
int32_t ea_linear_pool_supported(int32_t in_features, int32_t out_features, int32_t B, int32_t gh, int32_t gw, int32_t r) {
  return proj_rs_pool_supported(in_features, out_features, B, gh, gw, r);
}

int ea_linear_w32_pool(int32_t dtype, int32_t B, int32_t gh, int32_t gw, int32_t r, int32_t in_features, int32_t out_features,
                       const void* a, int32_t a_f32, int64_t lda, const float* w, const float* bias, void* y, int64_t ldy,
                       void* a_cast, float* pooled_q, float* pooled_k, void* w_cast, void* stream) {
  if (!a || !w || !y || !pooled_q || !pooled_k || ((uintptr_t)a & 15) || ((uintptr_t)w & 15) || ((uintptr_t)y & 15) ||
      ((uintptr_t)bias & 15) || ((uintptr_t)a_cast & 15) || ((uintptr_t)pooled_q & 15) || ((uintptr_t)pooled_k & 15) ||
      ((uintptr_t)w_cast & 15))
    return EA_E_BADARG;
  if (lda < in_features || ldy < out_features || (lda & 7) || (ldy & 7)) return EA_E_BADARG;
  if (!proj_rs_pool_supported(in_features, out_features, B, gh, gw, r)) return EA_E_UNSUPPORTED;
  return proj_rs_dispatch(dtype, a, a_f32, w, bias, y, a_cast, B * gh * gw, (long)lda, (long)ldy, (hipStream_t)stream, B, gh, gw,
                          r, pooled_q, pooled_k, w_cast, nullptr);
}

int ea_linear_w192_prepare(int32_t dtype, const float* wq, const float* wp, void* w16q, void* wq_sw, void* w16p, void* w16pT,
                           void* stream) {
  if (!wq || !w16q || !wq_sw || ((uintptr_t)wq & 15) || ((uintptr_t)wp & 15) || ((uintptr_t)w16q & 15) || ((uintptr_t)wq_sw & 15) ||
      ((uintptr_t)w16p & 15) || ((uintptr_t)w16pT & 15))
    return EA_E_BADARG;
  if (wp && (!w16p || !w16pT)) return EA_E_BADARG;
  return w192_prepare_dispatch(dtype, wq, wp, w16q, wq_sw, w16p, w16pT, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int ea_linear_w192_prepare_t(int32_t dtype, const float* wq, const float* wp, void* w16q, void* wq_sw, void* w16p, void* w16pT,
                             void* wqT_sw, void* stream) {
  if (!wq || !w16q || !wq_sw || !wqT_sw || ((uintptr_t)wq & 15) || ((uintptr_t)wp & 15) || ((uintptr_t)w16q & 15) ||
      ((uintptr_t)wq_sw & 15) || ((uintptr_t)w16p & 15) || ((uintptr_t)w16pT & 15) || ((uintptr_t)wqT_sw & 15))
    return EA_E_BADARG;
  if (wp && (!w16p || !w16pT)) return EA_E_BADARG;
  return w192_prepare_dispatch(dtype, wq, wp, w16q, wq_sw, w16p, w16pT, wqT_sw, nullptr, nullptr, (hipStream_t)stream);
}

// ... and W_proj / W_proj^T in the register order of the 192 -> 192 register-resident kernel (ea_linear_rs192.hip)
int ea_linear_w192_prepare_rs(int32_t dtype, const float* wq, const float* wp, void* w16q, void* wq_sw, void* w16p, void* w16pT,
                              void* wqT_sw, void* wp_rs, void* wpT_rs, void* stream) {
  if (!wq || !wp || !w16q || !wq_sw || !w16p || !w16pT || !wqT_sw || !wp_rs || !wpT_rs) return EA_E_BADARG;
  if (((uintptr_t)wq & 15) || ((uintptr_t)wp & 15) || ((uintptr_t)w16q & 15) || ((uintptr_t)wq_sw & 15) || ((uintptr_t)w16p & 15) ||
      ((uintptr_t)w16pT & 15) || ((uintptr_t)wqT_sw & 15) || ((uintptr_t)wp_rs & 15) || ((uintptr_t)wpT_rs & 15))
    return EA_E_BADARG;
  return w192_prepare_dispatch(dtype, wq, wp, w16q, wq_sw, w16p, w16pT, wqT_sw, wp_rs, wpT_rs, (hipStream_t)stream);
}

// Y = A W^T (+ bias) at 192 -> 192 from such an image, weight resident in registers (ea_linear_rs192.hip)
int ea_linear_rs192(int32_t dtype, const void* a, int64_t lda, const void* image, const float* bias, void* y, int64_t ldy,
                    int32_t rows, void* stream) {
  if (dtype != EA_BF16 && dtype != EA_F16) return EA_E_BADARG;
  if (rows <= 0) return EA_OK;
  if (!a || !image || !y) return EA_E_BADARG;
  if (((uintptr_t)a & 15) || ((uintptr_t)image & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15)) return EA_E_UNSUPPORTED;
  if (!linear_rs192_supported(rows, (long)lda, (long)ldy)) return EA_E_UNSUPPORTED;
  return linear_rs192_dispatch(dtype, a, (long)lda, image, bias, y, (long)ldy, rows, (hipStream_t)stream);
}

int ea_linear_wsw(int32_t dtype, int32_t rows, int32_t B, int32_t gh, int32_t gw, int32_t r, const void* a, int32_t a_f32, int64_t lda,
                  const void* wq_sw, const float* bias, void* y, int64_t ldy, void* a_cast, float* pooled_q, float* pooled_k,
                  void* stream) {
  if (!a || !wq_sw || !y || ((uintptr_t)a & 15) || ((uintptr_t)wq_sw & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15) ||
      ((uintptr_t)a_cast & 15) || ((uintptr_t)pooled_q & 15) || ((uintptr_t)pooled_k & 15))
    return EA_E_BADARG;
  if (lda < 192 || ldy < 576 || (lda & 7) || (ldy & 7) || rows <= 0) return EA_E_BADARG;
  if (r != 0) {
    if (!pooled_q || !pooled_k || rows != B * gh * gw) return EA_E_BADARG;
    if (!proj_rs_pool_supported(192, 576, B, gh, gw, r)) return EA_E_UNSUPPORTED;
  }
  return proj_rs_dispatch(dtype, a, a_f32, nullptr, bias, y, a_cast, rows, (long)lda, (long)ldy, (hipStream_t)stream, B, gh, gw, r,
                          r ? pooled_q : nullptr, r ? pooled_k : nullptr, nullptr, wq_sw);
}

}  // extern "C"

// ---- ScatterBrain feature half (ea_scatter.hip) ----
static int fill_sb(const ea_sb_geom* g, SbP& p) {
  if (!g || g->B <= 0 || g->H <= 0 || g->N <= 0 || g->window <= 0 || (g->dtype != EA_BF16 && g->dtype != EA_F16))
    return EA_E_BADARG;
  if (g->D != 64 || g->M <= 0 || g->M > 64) return EA_E_UNSUPPORTED;
  p.B = g->B; p.H = g->H; p.N = g->N; p.M = g->M; p.w = g->window;
  p.G.N = g->N; p.G.attn2d = g->attn_2d; p.G.gh = g->attn_2d ? g->gh : 1; p.G.gw = g->attn_2d ? g->gw : g->N;
  if (g->attn_2d) {
    if (g->gh % g->window || g->gw % g->window || g->gh * g->gw != g->N) return EA_E_BADARG;
    p.Wq = g->window * g->window;
    p.nwin = (g->gh / g->window) * (g->gw / g->window);
  } else {
    if (g->N % g->window) return EA_E_BADARG;
    p.Wq = g->window;
    p.nwin = g->N / g->window;
  }
  if (p.Wq > 64) return EA_E_UNSUPPORTED;
  p.a = 1.f / sqrtf(sqrtf(64.f));
  p.b = 0.5f / sqrtf(64.f);
  p.lconst = 0.5f * logf((float)g->M);
  p.wpb = 1;
  for (int d = 2; d <= 4; ++d)                      // windows per workgroup of the backward window pass
    if (p.nwin % d == 0) p.wpb = d;
  return EA_OK;
}
static int fill_sb_stats(const ea_sb_geom* g, LaraP& p) {
  ea_perf_geom pg;
  pg.B = g->B; pg.H = g->H; pg.N = g->N; pg.D = g->D; pg.dtype = g->dtype; pg.M = g->M;
  int rc = fill_perf(&pg, p, true);
  if (rc != EA_OK) return rc;
  p.ratio = 1.f; p.feps = 0.f; p.stab_per_feature = 1;
  return EA_OK;
}

extern "C" {

int32_t ea_scatter_parts(const ea_sb_geom* g) {
  LaraP p = {};
  if (!g || fill_sb_stats(g, p) != EA_OK) return EA_E_BADARG;
  return p.nsplit * lara_nsub(p.NCT);
}

int ea_scatter_kmax(const ea_sb_geom* g, const ea_t4* k, const uint8_t* mask, const float* W, float* p_ml, void* stream) {
  LaraP p = {};
  if (!g) return EA_E_BADARG;
  int rc = fill_sb_stats(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !W || !p_ml) return EA_E_BADARG;
  p.k = mk(k); p.mask = mask; p.omega = W; p.p_ml = p_ml;
  return lara_y_dispatch(LY_PMAX, p, g->dtype, (hipStream_t)stream);
}

int ea_scatter_kv(const ea_sb_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                  const float* mx, float* p_ml, float* p_kv, void* stream) {
  LaraP p = {};
  if (!g) return EA_E_BADARG;
  int rc = fill_sb_stats(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, g->D, 2) || !view_ok(v, g->D, 2) || !W || !mx || !p_ml || !p_kv) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.mask = mask; p.omega = W; p.stab = mx; p.p_ml = p_ml; p.p_acc0 = p_kv;
  return lara_y_dispatch(LY_PKV, p, g->dtype, (hipStream_t)stream);
}

int32_t ea_scatter_bwd_parts(const ea_sb_geom* g) {
  SbP p = {};
  if (fill_sb(g, p) != EA_OK) return EA_E_BADARG;
  return p.nwin / p.wpb;
}

int ea_scatter_bwd_window(const ea_sb_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                          const float* W, const float* mx, const float* zall, const float* sall, const ea_t4* oloc,
                          const float* lse_loc, const float* r, const ea_t4* dout, const ea_t4* dq, const ea_t4* dk,
                          const ea_t4* dv, const ea_t4* doloc, float* dlse, float* p_dsall, float* p_dzall,
                          void* stream) {
  SbP p = {};
  int rc = fill_sb(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, 64, 2) || !view_ok(k, 64, 2) || !view_ok(v, 64, 2) || !view_ok(oloc, 64, 2) || !view_ok(dout, 64, 2) || !view_ok(dq, 64, 2) ||
      !view_ok(dk, 64, 2) || !view_ok(dv, 64, 2) || !view_ok(doloc, 64, 2) || !W || !mx || !zall || !sall || !lse_loc || !r || !dlse ||
      !p_dsall || !p_dzall) return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.v = mk(v); p.oloc = mk(oloc); p.dout = mk(dout); p.dq = mk(dq); p.dk = mk(dk);
  p.dv = mk(dv); p.doloc = mk(doloc); p.mask = mask; p.Wf = W; p.mx = mx; p.zall = zall; p.sall = sall;
  p.lse_loc = lse_loc; p.r = const_cast<float*>(r); p.dlse = dlse; p.p_dsall = p_dsall; p.p_dzall = p_dzall;
  return sb_bwd_dispatch(0, p, g->dtype, (hipStream_t)stream);
}

int ea_scatter_bwd_global(const ea_sb_geom* g, const ea_t4* k, const ea_t4* v, const uint8_t* mask, const float* W,
                          const float* mx, const float* dsall, const float* dzall, const ea_t4* dk, const ea_t4* dv,
                          void* stream) {
  SbP p = {};
  int rc = fill_sb(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, 64, 2) || !view_ok(v, 64, 2) || !view_ok(dk, 64, 2) || !view_ok(dv, 64, 2) || !W || !mx || !dsall || !dzall)
    return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.dk = mk(dk); p.dv = mk(dv); p.mask = mask; p.Wf = W; p.mx = mx;
  p.zall = mx; p.sall = dsall;                       // (unused in the global pass; kept valid)
  p.dsall = dsall; p.dzall = dzall;
  p.wpb = 1;
  return sb_bwd_dispatch(1, p, g->dtype, (hipStream_t)stream);
}

int ea_scatter_fwd(const ea_sb_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                   const float* W, const float* mx, const float* zall, const float* sall, const ea_t4* oloc,
                   const float* lse_loc, const ea_t4* out, float* r, void* stream) {
  SbP p = {};
  int rc = fill_sb(g, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, 64, 2) || !view_ok(k, 64, 2) || !view_ok(v, 64, 2) || !view_ok(oloc, 64, 2) || !view_ok(out, 64, 2) || !W || !mx || !zall ||
      !sall || !lse_loc || !r) return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.v = mk(v); p.oloc = mk(oloc); p.out = mk(out); p.mask = mask; p.Wf = W;
  p.mx = mx; p.zall = zall; p.sall = sall; p.lse_loc = lse_loc; p.r = r;
  return sb_fwd_dispatch(p, g->dtype, (hipStream_t)stream);
}

// overlapping windows: the geometry of ea_sb_geom plus the extension of the key patch on every side
static int fill_sb_ov(const ea_sb_geom* g, int32_t ext, SbP& p) {
  int rc = fill_sb(g, p);
  if (rc != EA_OK) return rc;
  if (ext < 0) return EA_E_BADARG;
  if (ext > g->window) return EA_E_UNSUPPORTED;      // the key pass looks at the adjacent windows only
  const int t = g->window + 2 * ext;
  p.ext = ext; p.Wk = g->attn_2d ? t * t : t;
  p.wpb = 1;
  return EA_OK;
}

int32_t ea_scatter_ov_windows(const ea_sb_geom* g, int32_t ext) {
  SbP p = {};
  int rc = fill_sb_ov(g, ext, p);
  return rc != EA_OK ? rc : p.nwin;
}

int ea_scatter_ov_fwd(const ea_sb_geom* g, int32_t ext, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                      const uint8_t* mask, const float* W, const float* mx, const float* zall, const float* sall,
                      const ea_t4* oloc, const float* lse_loc, const ea_t4* out, float* r, void* stream) {
  SbP p = {};
  int rc = fill_sb_ov(g, ext, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, 64, 2) || !view_ok(k, 64, 2) || !view_ok(v, 64, 2) || !view_ok(oloc, 64, 2) || !view_ok(out, 64, 2) || !W || !mx || !zall ||
      !sall || !lse_loc || !r) return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.v = mk(v); p.oloc = mk(oloc); p.out = mk(out); p.mask = mask; p.Wf = W;
  p.mx = mx; p.zall = zall; p.sall = sall; p.lse_loc = lse_loc; p.r = r;
  return sb_ov_dispatch(0, p, g->dtype, (hipStream_t)stream);
}

int ea_scatter_ov_bwd_window(const ea_sb_geom* g, int32_t ext, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                             const uint8_t* mask, const float* W, const float* mx, const float* zall,
                             const float* sall, const ea_t4* oloc, const float* lse_loc, const float* r,
                             const ea_t4* dout, const ea_t4* dq, const ea_t4* doloc, float* dlse, float* w_ds,
                             float* w_dzall, float* w_dzwin, void* stream) {
  SbP p = {};
  int rc = fill_sb_ov(g, ext, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(q, 64, 2) || !view_ok(k, 64, 2) || !view_ok(v, 64, 2) || !view_ok(oloc, 64, 2) || !view_ok(dout, 64, 2) || !view_ok(dq, 64, 2) ||
      !view_ok(doloc, 64, 2) || !W || !mx || !zall || !sall || !lse_loc || !r || !dlse || !w_ds || !w_dzall || !w_dzwin)
    return EA_E_BADARG;
  p.q = mk(q); p.k = mk(k); p.v = mk(v); p.oloc = mk(oloc); p.dout = mk(dout); p.dq = mk(dq);
  p.doloc = mk(doloc); p.mask = mask; p.Wf = W; p.mx = mx; p.zall = zall; p.sall = sall;
  p.lse_loc = lse_loc; p.r = const_cast<float*>(r); p.dlse = dlse; p.p_dsall = w_ds; p.p_dzall = w_dzall;
  p.ws_dz = w_dzwin;
  return sb_ov_dispatch(1, p, g->dtype, (hipStream_t)stream);
}

int ea_scatter_ov_bwd_keys(const ea_sb_geom* g, int32_t ext, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                           const float* W, const float* mx, const float* dsall, const float* dzall, const float* w_ds,
                           const float* w_dzwin, const ea_t4* dk, const ea_t4* dv, void* stream) {
  SbP p = {};
  int rc = fill_sb_ov(g, ext, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(k, 64, 2) || !view_ok(v, 64, 2) || !view_ok(dk, 64, 2) || !view_ok(dv, 64, 2) || !W || !mx || !dsall || !dzall || !w_ds ||
      !w_dzwin) return EA_E_BADARG;
  p.k = mk(k); p.v = mk(v); p.dk = mk(dk); p.dv = mk(dv); p.mask = mask; p.Wf = W; p.mx = mx;
  p.dsall = dsall; p.dzall = dzall; p.p_dsall = const_cast<float*>(w_ds); p.ws_dz = const_cast<float*>(w_dzwin);
  return sb_ov_dispatch(2, p, g->dtype, (hipStream_t)stream);
}

}  // extern "C"

// ---- composite per-module entry points (round 3): one call = the whole LARA core forward, one = the whole backward ----
// The reference's call sites run eagerly (vit/engine.py:47-64); issued from Python the core was ~15 C-ABI calls and ~30
// tensor allocations per step.  Here the launch sequence lives in C++ and every intermediate sits in two caller-owned
// workspaces (`saved`: what the backward needs again; `tmp`: scratch of one direction) whose sizes ea_lara_layer_plan reports.
namespace {
struct LaraLayerPlan {
  ea_geom pg;            // pooling geometry (uniform r x r average pooling of q, k: lara.py:43,48,145-151)
  ea_lmk_geom lg;        // landmark pipeline
  ea_lara_geom g;        // estimator
  int L, C, BH, S_fwd, S_bwd;
  // offsets (floats) into the saved workspace
  size_t o_omega, o_qrows, o_bhv, o_cst, o_kv, o_lsek, o_lset, o_pq, o_pk, o_lmk, o_tok, n_saved;
  // forward scratch: lp, p_ml, p_kv
  size_t f_lp, f_ml, f_kv, n_ftmp;
  // backward scratch: p_ml, p_acc[4], big[4], small[4], d_omega, dpq, dpk, dW, dvec
  size_t b_ml, b_acc, b_big, b_small, b_dom, b_dpq, b_dpk, b_dW, b_dvec, b_domk, n_btmp;
  bool fold_f, fold_b;   // round 5: merge launches folded into their consumers (S <= 4 slices; EA_LARA_FOLD=0 restores them)
};
size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }       // 16-byte aligned sub-buffers
int lara_layer_plan(const ea_lara_layer* c, LaraLayerPlan& P) {
  if (!c || c->B <= 0 || c->H <= 0 || c->gh <= 0 || c->gw <= 0 || c->pool_r <= 0 || c->gh % c->pool_r || c->gw % c->pool_r)
    return EA_E_BADARG;
  const int N = c->gh * c->gw;
  P.L = (c->gh / c->pool_r) * (c->gw / c->pool_r);
  P.C = P.L * (c->dup ? 2 : 1);
  P.BH = c->B * c->H;
  if (P.C > 64 || P.L > 64) return EA_E_UNSUPPORTED;        // larger sample counts: the step-by-step entry points
  ea_geom pg = {};
  pg.B = c->B; pg.H = c->H; pg.N = N; pg.D = c->D; pg.dtype = c->dtype; pg.attn_2d = 1; pg.gh = c->gh; pg.gw = c->gw;
  pg.window = c->pool_r; pg.ext = 0; pg.chunk = c->pool_r; pg.L = P.L; pg.scale = c->scale; pg.causal = 0; pg.lm_base = 0;
  P.pg = pg;
  ea_lmk_geom lg = {};
  lg.BH = P.BH; lg.L = P.L; lg.C = P.C; lg.D = c->D; lg.has_mlp = c->has_mlp; lg.mixed = c->mixed; lg.mis = c->mis;
  lg.dup = c->dup; lg.scale = c->scale; lg.eva = 0;
  P.lg = lg;
  ea_lara_geom g = {};
  g.B = c->B; g.H = c->H; g.N = N; g.D = c->D; g.dtype = c->dtype; g.C = P.C; g.mis = c->mis; g.kappa = c->kappa; g.scale = c->scale;
  P.g = g;
  P.S_fwd = ea_lara_parts(&g);
  P.S_bwd = ea_lara_fused_parts(&g);
  if (P.S_fwd <= 0 || P.S_bwd <= 0) return EA_E_UNSUPPORTED;
  const size_t CD = (size_t)P.BH * P.C * c->D, Cs = (size_t)P.BH * P.C, LD = (size_t)P.BH * P.L * c->D;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al4(n); return at; };
  P.o_omega = take(CD); P.o_qrows = take(CD); P.o_bhv = take(Cs); P.o_cst = take(Cs); P.o_kv = take(CD);
  P.o_lsek = take(Cs); P.o_lset = take(Cs); P.o_pq = take(LD); P.o_pk = take(LD);
  const int64_t ls = ea_lara_landmarks_saved_floats(&lg);
  if (ls < 0) return EA_E_UNSUPPORTED;
  P.o_lmk = take((size_t)ls); P.o_tok = take((size_t)2 * P.BH * N);
  P.n_saved = o;
  o = 0;
  P.f_lp = take(Cs); P.f_ml = take(Cs * P.S_fwd * 4); P.f_kv = take(CD * P.S_fwd);
  P.n_ftmp = o;
  o = 0;
  P.b_ml = take(Cs * P.S_bwd * 4); P.b_acc = take(4 * CD * P.S_bwd); P.b_big = take(4 * CD); P.b_small = take(4 * Cs);
  P.b_dom = take(CD); P.b_dpq = take(LD); P.b_dpk = take(LD);
  P.b_dW = take((size_t)P.BH * 2 * c->D * c->D); P.b_dvec = take((size_t)P.BH * 6 * c->D);
  const char* fold_env = getenv("EA_LARA_FOLD");             // (read per call: the tests switch it inside one process)
  const bool fold_on = !(fold_env && fold_env[0] == '0');
  P.fold_f = fold_on && P.S_fwd <= 4;
  P.fold_b = fold_on && P.S_bwd <= 4;
  // reserved whatever the switch says: the caller memoises the workspace sizes per geometry, and a size that followed the
  // environment would let a later call with the fold ON write p_domk past a buffer sized with it OFF
  P.b_domk = take(P.S_bwd <= 4 ? CD * P.S_bwd : 0);
  P.n_btmp = o;
  return EA_OK;
}
}  // namespace

extern "C" {

int ea_lara_layer_plan(const ea_lara_layer* c, ea_lara_layer_sizes* out) {
  LaraLayerPlan P;
  const int rc = lara_layer_plan(c, P);
  if (rc != EA_OK) return rc;
  if (!out) return EA_E_BADARG;
  // bwd_uq .. saved_lse_t: what ea_linear_dgrad_finish needs after ea_lara_layer_bwd with EA_LARA_DEFER_FINISH -- in the backward
  // scratch u qbar rows (the fourth [B*H, C, D] block of `big`), d(pooled q), d(pooled k); in `saved` the qbar rows and lse_t
  ea_lara_layer_sizes& o = *out;
  o.n_saved = (int64_t)P.n_saved; o.n_fwd_tmp = (int64_t)P.n_ftmp; o.n_bwd_tmp = (int64_t)P.n_btmp;
  o.saved_pq = (int64_t)P.o_pq; o.saved_pk = (int64_t)P.o_pk; o.saved_qrows = (int64_t)P.o_qrows; o.saved_lse_t = (int64_t)P.o_lset;
  o.bwd_dW = (int64_t)P.b_dW; o.bwd_dvec = (int64_t)P.b_dvec; o.bwd_uq = (int64_t)(P.b_big + 3 * (size_t)P.BH * P.C * c->D);
  o.bwd_dpq = (int64_t)P.b_dpq; o.bwd_dpk = (int64_t)P.b_dpk;
  return EA_OK;
}

// proj: the output projection's operands (ea_lara_layer_fwd_proj) or null
static int lara_layer_fwd_impl(const ea_lara_layer* c, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                               const float* noise, const float* const* params, const ea_t4* out, float* saved, float* tmp,
                               int32_t keep_for_backward, const LaraXpP* proj, void* stream) {
  LaraLayerPlan P;
  int rc = lara_layer_plan(c, P);
  if (rc != EA_OK) return rc;
  if (proj) {
    // everything the last launch would refuse is refused here, before the first one
    if (!P.fold_f || !lara_xp_supported(c->H, c->D, P.C, P.S_fwd)) return EA_E_UNSUPPORTED;
    if (!proj->w || ((uintptr_t)proj->w & 15) || !proj->y || ((uintptr_t)proj->y & 7) || proj->ldy < 192 || (proj->ldy & 3) ||
        (proj->bias && ((uintptr_t)proj->bias & 3)) || !view_ok(q, c->D, 2) || !view_ok(out, c->D, 2)) return EA_E_BADARG;
  }
  if (!saved || !tmp || (c->has_mlp && !params)) return EA_E_BADARG;
  const float* pr[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (c->has_mlp) for (int i = 0; i < 8; ++i) pr[i] = params[i];
  const bool opt = c->mis == EA_MIS_OPT;
  float* omega = saved + P.o_omega;
  float* qrows = c->mis != EA_MIS_BH ? saved + P.o_qrows : nullptr;
  float* bhv = opt ? saved + P.o_bhv : nullptr;
  float* lse_t = opt ? saved + P.o_lset : nullptr;
  float* pq = saved + P.o_pq; float* pk = saved + P.o_pk;
  if (!(keep_for_backward & EA_LARA_POOLED_READY)) {
    rc = ea_eva_chunk_mean_fwd(&P.pg, q, k, nullptr, pq, pk, stream);
    if (rc != EA_OK) return rc;
  }
  keep_for_backward &= 1;
  rc = ea_lara_landmarks_fwd(&P.lg, pq, pk, pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6], pr[7], noise, omega, qrows, bhv,
                             tmp + P.f_lp, keep_for_backward ? saved + P.o_lmk : nullptr, stream);
  if (rc != EA_OK) return rc;
  rc = ea_lara_stats_fwd(&P.g, q, k, v, mask, omega, qrows, tmp + P.f_ml, tmp + P.f_kv, stream);
  if (rc != EA_OK) return rc;
  float* tok = keep_for_backward ? saved + P.o_tok : nullptr;
  if (proj)
    return ea_lara_out_proj_fwd_merge(&P.g, q, omega, qrows, bhv, P.S_fwd, tmp + P.f_ml, tmp + P.f_kv, tmp + P.f_lp,
                                      saved + P.o_kv, saved + P.o_lsek, lse_t, saved + P.o_cst, out, tok,
                                      tok ? tok + (size_t)P.BH * P.g.N : nullptr, proj->w, proj->bias, proj->y, proj->ldy, stream);
  if (P.fold_f)
    return ea_lara_out_fwd_merge(&P.g, q, omega, qrows, bhv, P.S_fwd, tmp + P.f_ml, tmp + P.f_kv, tmp + P.f_lp, saved + P.o_kv,
                                 saved + P.o_lsek, lse_t, saved + P.o_cst, out, tok, tok ? tok + (size_t)P.BH * P.g.N : nullptr,
                                 stream);
  rc = ea_lara_merge_fwd(P.BH, P.S_fwd, P.C, c->D, opt ? 1 : 0, tmp + P.f_ml, tmp + P.f_kv, tmp + P.f_lp, saved + P.o_kv,
                         saved + P.o_lsek, lse_t, saved + P.o_cst, stream);
  if (rc != EA_OK) return rc;
  return ea_lara_out_fwd(&P.g, q, omega, qrows, saved + P.o_kv, lse_t, bhv, saved + P.o_cst, out, tok,
                         tok ? tok + (size_t)P.BH * P.g.N : nullptr, stream);
}

int ea_lara_layer_fwd(const ea_lara_layer* c, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                      const float* noise, const float* const* params, const ea_t4* out, float* saved, float* tmp,
                      int32_t keep_for_backward, void* stream) {
  return lara_layer_fwd_impl(c, q, k, v, mask, noise, params, out, saved, tmp, keep_for_backward, nullptr, stream);
}

int ea_lara_layer_fwd_proj(const ea_lara_layer* c, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                           const float* noise, const float* const* params, const ea_t4* out, float* saved, float* tmp,
                           int32_t keep_for_backward, const void* w_proj16, const float* bias, void* y, int64_t ldy,
                           void* stream) {
  LaraXpP xp;
  xp.w = (const char*)w_proj16; xp.bias = bias; xp.y = (char*)y; xp.ldy = (long)ldy;
  return lara_layer_fwd_impl(c, q, k, v, mask, noise, params, out, saved, tmp, keep_for_backward, &xp, stream);
}

int ea_lara_layer_bwd(const ea_lara_layer* c, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* mask,
                      const float* noise, const float* const* params, const ea_t4* dout, const ea_t4* dq, const ea_t4* dk,
                      const ea_t4* dv, const float* saved, float* tmp, float* dparams, int32_t flags, void* stream) {
  const bool defer_finish = (flags & EA_LARA_DEFER_FINISH) != 0;
  LaraLayerPlan P;
  int rc = lara_layer_plan(c, P);
  if (rc != EA_OK) return rc;
  if (!saved || !tmp || (c->has_mlp && !params)) return EA_E_BADARG;
  const float* pr[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (c->has_mlp) for (int i = 0; i < 8; ++i) pr[i] = params[i];
  const bool opt = c->mis == EA_MIS_OPT;
  const int D = c->D;
  const size_t CD = (size_t)P.BH * P.C * D, Cs = (size_t)P.BH * P.C;
  const float* omega = saved + P.o_omega;
  const float* qrows = c->mis != EA_MIS_BH ? saved + P.o_qrows : nullptr;
  const float* bhv = opt ? saved + P.o_bhv : nullptr;
  const float* lse_t = opt ? saved + P.o_lset : nullptr;
  const float* kv = saved + P.o_kv;
  const float* tok = saved + P.o_tok;
  float* p_ml = tmp + P.b_ml;
  float* acc[4];
  for (int i = 0; i < 4; ++i) acc[i] = tmp + P.b_acc + (size_t)i * CD * P.S_bwd;
  float *dkv = tmp + P.b_big, *dom_q = dkv + CD, *dqbar_m = dom_q + CD, *uq = dqbar_m + CD;
  float *r = tmp + P.b_small, *dbh = r + Cs, *dlp_m = dbh + Cs, *dkk = dlp_m + Cs;
  rc = ea_lara_bwd_q_fused(&P.g, q, dout, omega, qrows, kv, lse_t, bhv, saved + P.o_cst, tok, tok + (size_t)P.BH * P.g.N, dq, p_ml,
                           acc[0], acc[1], acc[2], acc[3], stream);
  if (rc != EA_OK) return rc;
  const bool want_dqbar = c->mis == EA_MIS_OPT || c->mis == EA_MIS_BIASED;
  if (P.fold_b) {
    // the key-side pass merges the query side's partials itself and block 0 of each (b,h) writes dbh, dlp, sum dZ q, d qbar
    // rows and u qbar; the landmark backward adds the key side's d omega partials while it loads its strips
    float* domk = tmp + P.b_domk;
    rc = ea_lara_bwd_k_fused_merge(&P.g, k, v, mask, omega, qrows, kv, saved + P.o_lsek, P.S_bwd, p_ml, acc[0], acc[1], acc[2],
                                   acc[3], dk, dv, domk, opt ? dbh : nullptr, dlp_m, dom_q, want_dqbar ? dqbar_m : nullptr,
                                   opt ? uq : nullptr, stream);
    if (rc != EA_OK) return rc;
    float *dpq = tmp + P.b_dpq, *dpk = tmp + P.b_dpk;
    float* dW = c->has_mlp ? tmp + P.b_dW : nullptr;
    float* dvec = c->has_mlp ? tmp + P.b_dvec : nullptr;
    rc = ea_lara_landmarks_bwd_parts(&P.lg, saved + P.o_pq, saved + P.o_pk, pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6], pr[7],
                                     noise, dom_q, P.S_bwd, domk, c->scale, want_dqbar ? dqbar_m : nullptr, opt ? dbh : nullptr,
                                     dlp_m, dpq, dpk, dW, dvec, saved + P.o_lmk, stream);
    if (rc != EA_OK) return rc;
    if (!defer_finish) {
      rc = ea_lara_bwd_finish(&P.g, q, qrows, opt ? uq : nullptr, lse_t, dpq, dpk, c->pool_r, c->gh, c->gw, dq, dk, stream);
      if (rc != EA_OK) return rc;
    }
    if (c->has_mlp && dparams) rc = ea_colsum2_f32(P.BH, 2 * D * D, dW, dparams, 6 * D, dvec, dparams + (size_t)2 * D * D, stream);
    return rc;
  }
  rc = ea_lara_merge_bwd(P.BH, P.S_bwd, P.C, D, opt ? 1 : 0, c->scale, p_ml, acc[0], acc[1], acc[2], acc[3], kv, qrows, r, dbh,
                         dlp_m, dkk, dkv, dom_q, want_dqbar ? dqbar_m : nullptr, opt ? uq : nullptr, stream);
  if (rc != EA_OK) return rc;
  rc = ea_lara_bwd_k_fused(&P.g, k, v, mask, omega, dkv, saved + P.o_lsek, dkk, r, dk, dv, acc[1], stream);
  if (rc != EA_OK) return rc;
  float* d_omega = tmp + P.b_dom;
  rc = ea_slice_sum(P.BH, P.S_bwd, P.C * D, c->scale, dom_q, acc[1], d_omega, stream);
  if (rc != EA_OK) return rc;
  float *dpq = tmp + P.b_dpq, *dpk = tmp + P.b_dpk;
  float* dW = c->has_mlp ? tmp + P.b_dW : nullptr;
  float* dvec = c->has_mlp ? tmp + P.b_dvec : nullptr;
  rc = ea_lara_landmarks_bwd(&P.lg, saved + P.o_pq, saved + P.o_pk, pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6], pr[7], noise,
                             d_omega, want_dqbar ? dqbar_m : nullptr, opt ? dbh : nullptr, dlp_m, dpq, dpk, dW, dvec,
                             saved + P.o_lmk, stream);
  if (rc != EA_OK) return rc;
  if (!defer_finish) {
    rc = ea_lara_bwd_finish(&P.g, q, qrows, opt ? uq : nullptr, lse_t, dpq, dpk, c->pool_r, c->gh, c->gw, dq, dk, stream);
    if (rc != EA_OK) return rc;
  }
  // dparams == NULL: the caller adds the per-(b,h) partials up itself (tmp + bwd_dW / bwd_dvec of the plan: [B*H, 2 D D] and
  // [B*H, 6 D]), e.g. together with other terminal sums of its backward in one ea_multi_sum launch
  if (c->has_mlp && dparams) rc = ea_colsum2_f32(P.BH, 2 * D * D, dW, dparams, 6 * D, dvec, dparams + (size_t)2 * D * D, stream);
  return rc;
}

}  // extern "C"

// ---- composite per-module entry points, EVA (round 4): the 2-D core of eva.py:145-227 in one call each way ----
// chunk means (or the projection kernel's) -> mu networks + omega (fused landmark kernel, eva mode) -> beta -> window
// attention with the control-variate columns; backward: window backward -> landmark-gradient slice sum (+ bias-gradient
// column sum) -> beta backward -> mu-network backward -> chunk-mean backward (-> parameter sums).  Same contract as the
// LARA pair: caller-owned workspaces, sizes from ea_eva_layer_plan.
namespace {
struct EvaLayerPlan {
  ea_geom g;
  ea_lmk_geom lg;
  int L, BH, N, Wq, ld, parts, bparts;
  size_t o_lse, o_qm, o_km, o_omega, o_beta, o_rfk, o_lmk, n_saved;
  size_t b_dlp, b_dl, b_dbp, b_dom, b_dqm, b_dkm, b_dW, b_dvec, n_btmp;
};
int eva_layer_plan(const ea_eva_layer* c, EvaLayerPlan& P) {
  if (!c || c->B <= 0 || c->H <= 0 || c->gh <= 0 || c->gw <= 0 || c->window <= 0 || c->chunk <= 0 ||
      c->gh % c->window || c->gw % c->window || c->gh % c->chunk || c->gw % c->chunk) return EA_E_BADARG;
  if (c->D != 32 && c->D != 64) return EA_E_UNSUPPORTED;
  P.N = c->gh * c->gw;
  P.L = (c->gh / c->chunk) * (c->gw / c->chunk);
  P.BH = c->B * c->H;
  if (P.L > 64) return EA_E_UNSUPPORTED;                    // the fused mu / omega kernel; larger: the step-by-step entries
  ea_geom g = {};
  g.B = c->B; g.H = c->H; g.N = P.N; g.D = c->D; g.dtype = c->dtype; g.attn_2d = 1; g.gh = c->gh; g.gw = c->gw;
  g.window = c->window; g.ext = 0; g.chunk = c->chunk; g.L = P.L; g.scale = c->scale; g.causal = 0; g.lm_base = 0;
  P.g = g;
  ea_lmk_geom lg = {};
  lg.BH = P.BH; lg.L = P.L; lg.C = P.L; lg.D = c->D; lg.has_mlp = 1; lg.mixed = 0; lg.mis = 0; lg.dup = 0;
  lg.scale = c->scale; lg.eva = 1;
  P.lg = lg;
  P.Wq = c->window * c->window;
  P.ld = ea_window_bias_ld(&g);
  P.parts = ea_window_bwd_parts(&g);
  P.bparts = c->has_bias ? ea_window_bwd_bias_parts(&g) : 0;
  if (P.ld <= 0 || P.parts <= 0 || (c->has_bias && P.bparts <= 0)) return EA_E_UNSUPPORTED;
  // geometries whose backward needs scratch slices, several query blocks or the transposed bias copy: step-by-step entries
  if (ea_window_bwd_acc_slices(&g) != 0 || ea_window_bwd_query_blocks(&g) != 1 ||
      (c->has_bias && ea_window_bwd_needs_bias_t(&g) != 0)) return EA_E_UNSUPPORTED;
  const size_t LD = (size_t)P.BH * P.L * c->D;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al4(n); return at; };
  P.o_lse = take((size_t)P.BH * P.N);
  P.o_qm = take(LD); P.o_km = take(LD); P.o_omega = take(LD); P.o_beta = take(LD); P.o_rfk = take(LD);
  const int64_t ls = ea_lara_landmarks_saved_floats(&lg);
  if (ls < 0) return EA_E_UNSUPPORTED;
  P.o_lmk = take((size_t)ls);
  P.n_saved = o;
  o = 0;
  P.b_dlp = take((size_t)2 * P.parts * LD); P.b_dl = take(2 * LD);
  P.b_dbp = take((size_t)P.bparts * c->B * c->H * P.Wq * P.ld);
  P.b_dom = take(LD); P.b_dqm = take(LD); P.b_dkm = take(LD);
  P.b_dW = take((size_t)P.BH * 2 * c->D * c->D); P.b_dvec = take((size_t)P.BH * 6 * c->D);
  P.n_btmp = o;
  return EA_OK;
}
}  // namespace

extern "C" {

int ea_eva_layer_plan(const ea_eva_layer* c, ea_eva_layer_sizes* out) {
  EvaLayerPlan P;
  const int rc = eva_layer_plan(c, P);
  if (rc != EA_OK) return rc;
  if (!out) return EA_E_BADARG;
  // bwd_dqmean / bwd_dkmean: the chunk-mean gradients ea_linear_dgrad_finish adds to dq / dk after EA_EVA_DEFER_CHUNK_MEAN
  ea_eva_layer_sizes& o = *out;
  o.n_saved = (int64_t)P.n_saved; o.n_bwd_tmp = (int64_t)P.n_btmp;
  o.saved_qmean = (int64_t)P.o_qm; o.saved_kmean = (int64_t)P.o_km; o.saved_lse = (int64_t)P.o_lse; o.bias_ld = (int64_t)P.ld;
  o.bwd_dW = (int64_t)P.b_dW; o.bwd_dvec = (int64_t)P.b_dvec; o.bwd_dbias_part = (int64_t)P.b_dbp;
  o.dbias_part_rows = (int64_t)P.bparts * c->B; o.bwd_dqmean = (int64_t)P.b_dqm; o.bwd_dkmean = (int64_t)P.b_dkm;
  return EA_OK;
}

int ea_eva_layer_fwd(const ea_eva_layer* c, const ea_t4* q, const ea_t4* k, const ea_t4* v, const float* bias,
                     const float* noise, const float* const* params, const ea_t4* out, float* saved,
                     int32_t keep_for_backward, void* stream) {
  EvaLayerPlan P;
  int rc = eva_layer_plan(c, P);
  if (rc != EA_OK) return rc;
  if (!saved || !params || (c->has_bias != 0) != (bias != nullptr)) return EA_E_BADARG;
  float *qm = saved + P.o_qm, *km = saved + P.o_km, *omega = saved + P.o_omega, *beta = saved + P.o_beta, *rfk = saved + P.o_rfk;
  if (!(keep_for_backward & EA_LARA_POOLED_READY)) {
    rc = ea_eva_chunk_mean_fwd(&P.g, q, k, nullptr, qm, km, stream);
    if (rc != EA_OK) return rc;
  }
  keep_for_backward &= 1;
  rc = ea_lara_landmarks_fwd(&P.lg, qm, km, params[0], params[1], params[2], params[3], params[4], params[5], params[6],
                             params[7], noise, omega, rfk, nullptr, nullptr, keep_for_backward ? saved + P.o_lmk : nullptr, stream);
  if (rc != EA_OK) return rc;
  rc = ea_eva_beta_fwd(&P.g, k, v, nullptr, omega, beta, stream);
  if (rc != EA_OK) return rc;
  return ea_window_attn_fwd(&P.g, q, k, v, rfk, beta, bias, nullptr, out, saved + P.o_lse, nullptr, 1.f, stream);
}

int ea_eva_layer_bwd(const ea_eva_layer* c, const ea_t4* q, const ea_t4* k, const ea_t4* v, const float* bias,
                     const float* noise, const float* const* params, const ea_t4* out, const ea_t4* dout, const ea_t4* dq,
                     const ea_t4* dk, const ea_t4* dv, const float* saved, float* tmp, float* dbias, float* dparams,
                     int32_t flags, void* stream) {
  EvaLayerPlan P;
  int rc = eva_layer_plan(c, P);
  if (rc != EA_OK) return rc;
  if (!saved || !tmp || !params || (c->has_bias != 0) != (bias != nullptr)) return EA_E_BADARG;
  const int D = c->D;
  const size_t LD = (size_t)P.BH * P.L * D;
  const float *qm = saved + P.o_qm, *km = saved + P.o_km, *omega = saved + P.o_omega, *beta = saved + P.o_beta, *rfk = saved + P.o_rfk;
  float* dl_p = tmp + P.b_dlp;
  float* dl = tmp + P.b_dl;                 // [2][B*H, L, D]: d rf_k_bar, d beta
  float* dbp = c->has_bias ? tmp + P.b_dbp : nullptr;
  rc = ea_window_attn_bwd(&P.g, q, k, v, rfk, beta, bias, nullptr, out, dout, saved + P.o_lse, dq, dk, dv, dl_p,
                          dl_p + (size_t)P.parts * LD, dbp, nullptr, nullptr, nullptr, nullptr, 1.f, nullptr, stream);
  if (rc != EA_OK) return rc;
  // round 6: up to four slice partials are added up by their two consumers while they load them (ea_slice_sum's order of
  // additions: bit-identical) -- one launch less; more slices keep the reduction launch (EA_EVA_FOLD_SLICES=0: always)
  static const bool fold_on = !(getenv("EA_EVA_FOLD_SLICES") && getenv("EA_EVA_FOLD_SLICES")[0] == '0');
  const bool fold = fold_on && P.parts <= 4;
  if (!fold) {
    rc = ea_slice_sum(2, P.parts, (int32_t)LD, 1.f, nullptr, dl_p, dl, stream);
    if (rc != EA_OK) return rc;
  }
  if (c->has_bias && dbias) {        // dbias == NULL: the partials stay in tmp for the caller's reduction (bwd_dbias_part, dbias_part_rows)
    rc = ea_colsum_f32(P.bparts * c->B, c->H * P.Wq * P.ld, dbp, dbias, stream);
    if (rc != EA_OK) return rc;
  }
  float* d_omega = tmp + P.b_dom;
  rc = fold ? eva_beta_bwd_parts(&P.g, k, v, nullptr, omega, beta, dl_p + (size_t)P.parts * LD, P.parts, (long)LD, dk, dv, d_omega, stream)
            : ea_eva_beta_bwd(&P.g, k, v, nullptr, omega, beta, dl + LD, dk, dv, d_omega, stream);
  if (rc != EA_OK) return rc;
  float *dqm = tmp + P.b_dqm, *dkm = tmp + P.b_dkm, *dW = tmp + P.b_dW, *dvec = tmp + P.b_dvec;
  rc = lara_landmarks_bwd_qparts(&P.lg, qm, km, params[0], params[1], params[2], params[3], params[4], params[5], params[6],
                                 params[7], noise, d_omega, fold ? dl_p : dl, fold ? P.parts : 1, fold ? (long)LD : 0, nullptr,
                                 nullptr, dqm, dkm, dW, dvec, saved + P.o_lmk, stream);
  if (rc != EA_OK) return rc;
  if (!(flags & EA_EVA_DEFER_CHUNK_MEAN)) {
    rc = ea_eva_chunk_mean_bwd(&P.g, dqm, dkm, nullptr, dq, dk, stream);
    if (rc != EA_OK) return rc;
  }
  // dparams == NULL: the per-(b,h) partials stay in tmp (offsets bwd_dW / bwd_dvec of the plan) for the caller's own reduction
  if (dparams) rc = ea_colsum2_f32(P.BH, 2 * D * D, dW, dparams, 6 * D, dvec, dparams + (size_t)2 * D * D, stream);
  return rc;
}

}  // extern "C"

// ---- fp32-faithful gathered attention (ea_f32_attn.hip) ----
static F32T f32_mk(const ea_t4* t) {
  F32T r;
  r.p = t ? (const float*)t->ptr : nullptr;
  r.sb = t ? t->sb : 0; r.sh = t ? t->sh : 0; r.sn = t ? t->sn : 0;
  return r;
}
static int fill_ga(const ea_f32_attn* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const ea_t4* ek, const ea_t4* ev,
                   const int32_t* idx_q, const int32_t* idx_k, const float* bias, const uint8_t* kmask, const uint8_t* qmask,
                   const uint8_t* keep, GaP& p) {
  if (!g || g->B <= 0 || g->H <= 0 || g->Nq <= 0 || g->Nk <= 0 || g->G <= 0 || g->Wq <= 0 || g->Wk < 0 || g->L < 0 ||
      g->Wk + g->L <= 0 || !idx_q || (g->Wk > 0 && !idx_k)) return EA_E_BADARG;
  if (g->D != 32 && g->D != 64 && g->D != 128) return EA_E_UNSUPPORTED;
  if (!view_ok(q, g->D, 4) || !view_ok(k, g->D, 4) || !view_ok(v, g->D, 4)) return EA_E_BADARG;
  if (g->L > 0 && (!view_ok(ek, g->D, 4) || !view_ok(ev, g->D, 4))) return EA_E_BADARG;
  if (bias && g->bias_ld < g->Wk) return EA_E_BADARG;
  if (keep && g->keep_ld < g->Wk + g->L) return EA_E_BADARG;
  p.q = f32_mk(q); p.k = f32_mk(k); p.v = f32_mk(v); p.ek = f32_mk(g->L > 0 ? ek : nullptr); p.ev = f32_mk(g->L > 0 ? ev : nullptr);
  p.idx_q = idx_q; p.idx_k = idx_k; p.bias = bias; p.bias_hs = g->bias_hs; p.bias_bs = g->bias_bs; p.bias_ld = g->bias_ld;
  p.kmask = kmask; p.qmask = qmask; p.keep = keep; p.keep_ld = g->keep_ld; p.keep_scale = g->keep_scale;
  p.B = g->B; p.H = g->H; p.Nq = g->Nq; p.Nk = g->Nk; p.D = g->D; p.G = g->G; p.Wq = g->Wq; p.Wk = g->Wk; p.L = g->L;
  p.knorm = g->knorm & 1; p.zero_mv = (g->knorm >> 1) & 1; p.neg_inf = g->neg_inf; p.causal_e = g->causal_e; p.chunk = g->chunk; p.lm_base = g->lm_base;
  p.scale = g->scale;
  return EA_OK;
}

extern "C" {

int ea_f32_attn_fwd(const ea_f32_attn* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const ea_t4* ek, const ea_t4* ev,
                    const int32_t* idx_q, const int32_t* idx_k, const float* bias, const uint8_t* kmask, const uint8_t* qmask,
                    const uint8_t* keep, const ea_t4* out, float* lse, float* stat, void* stream) {
  GaP p = {};
  int rc = fill_ga(g, q, k, v, ek, ev, idx_q, idx_k, bias, kmask, qmask, keep, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(out, g->D, 4)) return EA_E_BADARG;
  p.o = f32_mk(out); p.lse = lse; p.stat = stat;
  return ga_dispatch(false, p, (hipStream_t)stream);
}

int ea_f32_attn_bwd(const ea_f32_attn* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const ea_t4* ek, const ea_t4* ev,
                    const int32_t* idx_q, const int32_t* idx_k, const float* bias, const uint8_t* kmask, const uint8_t* qmask,
                    const uint8_t* keep, const ea_t4* out, const ea_t4* dout, const float* stat, const float* dlse,
                    const ea_t4* dq, float* dk, float* dv, float* dek, float* dev, float* dbias, void* stream) {
  GaP p = {};
  int rc = fill_ga(g, q, k, v, ek, ev, idx_q, idx_k, bias, kmask, qmask, keep, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(out, g->D, 4) || !view_ok(dout, g->D, 4) || !view_ok(dq, g->D, 4) || !stat) return EA_E_BADARG;
  if (dbias && !bias) return EA_E_BADARG;
  p.o = f32_mk(out); p.dout = f32_mk(dout); p.dq = f32_mk(dq); p.stat = const_cast<float*>(stat); p.dlse = dlse;
  p.dk = dk; p.dv = dv; p.dek = g->L > 0 ? dek : nullptr; p.dev = g->L > 0 ? dev : nullptr; p.dbias = dbias;
  return ga_dispatch(true, p, (hipStream_t)stream);
}

int ea_f32_gather_mean_fwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t Cn, int32_t J, const ea_t4* x, const int32_t* idx,
                           const uint8_t* mask, float* mean, void* stream) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0 || (D & 3) || Cn <= 0 || J <= 0 || !view_ok(x, D, 4) || !idx || !mean) return EA_E_BADARG;
  GmP p = {};
  p.x = f32_mk(x); p.idx = idx; p.mask = mask; p.mean = mean; p.B = B; p.H = H; p.N = N; p.D = D; p.Cn = Cn; p.J = J;
  return gm_dispatch(false, p, (hipStream_t)stream);
}

int ea_f32_gather_mean_bwd(int32_t B, int32_t H, int32_t N, int32_t D, int32_t Cn, int32_t J, const int32_t* idx,
                           const uint8_t* mask, const float* dmean, float* dx, void* stream) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0 || (D & 3) || Cn <= 0 || J <= 0 || !idx || !dmean || !dx) return EA_E_BADARG;
  GmP p = {};
  p.idx = idx; p.mask = mask; p.dmean = dmean; p.dx = dx; p.B = B; p.H = H; p.N = N; p.D = D; p.Cn = Cn; p.J = J;
  return gm_dispatch(true, p, (hipStream_t)stream);
}

}  // extern "C"

// ---- row LayerNorm (ea_layernorm.hip) ----
extern "C" {

int32_t ea_layernorm_parts(int32_t rows) { return ea::layernorm_parts(rows); }

int ea_layernorm_fwd(int32_t xtype, int32_t rows, int32_t C, const void* x, const float* gamma, const float* beta, float eps,
                     float* y, float* stats, void* stream) {
  if (!x || !gamma || !beta || !y) return EA_E_BADARG;
  ea::LnP p = {};
  p.x = x; p.gamma = gamma; p.beta = beta; p.y = y; p.stats = stats; p.rows = rows; p.C = C; p.eps = eps;
  return ea::layernorm_dispatch(false, p, xtype, (hipStream_t)stream);
}

int ea_layernorm_bwd(int32_t xtype, int32_t rows, int32_t C, const void* x, const float* gamma, const float* stats,
                     const float* dy, void* dx, float* part, void* stream) {
  if (!x || !gamma || !stats || !dy || !dx || !part) return EA_E_BADARG;
  ea::LnP p = {};
  p.x = x; p.gamma = gamma; p.stats = const_cast<float*>(stats); p.dy = dy; p.dx = dx; p.part = part; p.rows = rows; p.C = C;
  return ea::layernorm_dispatch(true, p, xtype, (hipStream_t)stream);
}

}  // extern "C"

// ---- causal EVA, incremental decoding (ea_ceva_decode.hip) ----
#include "ea_ceva_decode.h"
#include "ea_ceva_decode_linear.h"
#include "ea_ceva_decode_vocab.h"
#include "ea_vocab_score.h"
#include "ea_adaptive_score.h"
#include "ea_adaptive_pick.h"
static ea::DecT dec_mk(const ea_t4* t) {
  ea::DecT r;
  r.p = (const char*)t->ptr; r.sb = t->sb; r.sh = t->sh; r.sn = t->sn;
  return r;
}
// A step's geometry as both families hand it over.  Dynamic (ea_ceva_dec_geom): the host knows t0 and which chunks close.
// Static (ea_ceva_sdec_geom, dev): the count is *pos, so the host can check only that a step fits an empty cache (t0 = 0; the
// kernels check t0 + T <= cap), no chunk range is given, the pad flags are always read, and ring is 0 (cap rows, linear) or
// the rows of a rolling state -- a multiple of window that holds one step's span.  ntok: null, or the per-sequence state's
// [B] token counts of the step (pos and status are [B] then).  l16 (ea_ceva_sdecode_*_l16, a compact state): the landmark
// rows have the geometry's dtype, which is then a 16-bit one.
struct DecG {
  int B, H, D, dtype, window, ext, chunk, t0, T_new, c_first, c_last, cap, adaptive, has_bias, has_mask, ring;
  const int32_t* pos;
  int32_t* status;
  bool dev;
  int32_t* ntok;
  bool l16;
};
static DecG dec_read(const ea_ceva_dec_geom* g) {
  return {g->B, g->H, g->D, g->dtype, g->window, g->ext, g->chunk, g->t0, g->T_new, g->c_first, g->c_last, g->cap,
          g->adaptive, g->has_bias, g->has_mask, 0, nullptr, nullptr, false, nullptr, false};
}
static DecG dec_read(const ea_ceva_sdec_geom* g, bool l16 = false) {
  return {g->B, g->H, g->D, g->dtype, g->window, g->ext, g->chunk, 0, g->T_new, 0, -1, g->cap,
          g->adaptive, g->has_bias, 1, g->ring, g->pos, g->status, true, g->ntok, l16};
}
// What every launch of a step needs; with `windows`, also what close and attn need of the window geometry (append moves
// rows and reads none of it).  Every EA_E_BADARG is decided before the head dim, the static state's own before the rest.
// (reads_pad = false: merge, the one launch of a static step that takes no pad flags.)
static int dec_check(const DecG& g, const uint8_t* pad, bool windows, bool reads_pad = true) {
  if (g.dev && (!g.pos || !g.status || (uintptr_t)g.pos % 4 || (uintptr_t)g.status % 4 || (uintptr_t)g.ntok % 4 ||
                (reads_pad && !pad)))
    return EA_E_BADARG;
  if (windows && (g.window <= 0 || g.chunk <= 0 || g.ext < 0 || (g.dev && (g.cap % g.window || g.window % g.chunk))))
    return EA_E_BADARG;
  if (g.ring != 0 && !(g.ring > 0 && g.window > 0 && g.ring % g.window == 0 && g.ext >= 0 && g.T_new > 0 &&
                       (int64_t)g.ring >= (int64_t)g.window + g.ext + g.T_new)) return EA_E_BADARG;
  if (g.B <= 0 || g.H <= 0 || g.t0 < 0 || g.T_new <= 0 || g.cap < g.t0 + g.T_new ||
      (g.dtype != EA_BF16 && g.dtype != EA_F16 && (g.l16 || g.dtype != EA_F32))) return EA_E_BADARG;
  if (g.D != 32 && g.D != 64 && g.D != 128) return EA_E_UNSUPPORTED;
  return EA_OK;
}
static int dec_fill(const DecG& g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad, const ea_t4* lk,
                    const ea_t4* lv, ea::DecP& p) {
  const int rc = dec_check(g, pad, true);
  if (rc != EA_OK) return rc;
  const int esz = g.dtype == EA_F32 ? 4 : 2;
  if (!view_ok(q, g.D, esz) || !view_ok(k, g.D, esz) || !view_ok(v, g.D, esz)) return EA_E_BADARG;
  const int lsz = g.l16 ? esz : 4;                        // (l16: 16-byte aligned rows of 8-element multiples)
  if (!view_ok(lk, g.D, lsz) || !view_ok(lv, g.D, lsz) || (g.has_mask && !pad)) return EA_E_BADARG;
  p.q = dec_mk(q); p.k = dec_mk(k); p.v = dec_mk(v); p.lk = dec_mk(lk); p.lv = dec_mk(lv);
  p.pad = g.has_mask ? pad : nullptr;
  p.B = g.B; p.H = g.H; p.D = g.D; p.dtype = g.dtype; p.w = g.window; p.e = g.ext; p.r = g.chunk;
  p.t0 = g.t0; p.T = g.T_new; p.c_first = g.c_first; p.c_last = g.c_last; p.cap = g.cap; p.adaptive = g.adaptive ? 1 : 0;
  p.scale = (float)(1.0 / sqrt((double)g.D));
  p.pos = g.pos; p.ring = g.ring; p.ntok = g.ntok;
  return EA_OK;
}
static int dec_close(const DecG& g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                     const float* const* mu_params, const ea_t4* lk, const ea_t4* lv, void* stream) {
  ea::DecP p = {};
  const int rc = dec_fill(g, q, k, v, pad, lk, lv, p);
  if (rc != EA_OK) return rc;
  // dynamic: the chunks must be decoded, rows [c_first r, (c_last + 1) r) lie in [0, t0 + T_new)
  if (!mu_params || (!g.dev && (g.c_first < 0 || g.c_last < g.c_first || (int64_t)(g.c_last + 1) * g.chunk > g.t0 + g.T_new)))
    return EA_E_BADARG;
  const int np = g.adaptive ? 8 : 4;
  for (int i = 0; i < np; ++i) {
    if (!mu_params[i] || (uintptr_t)mu_params[i] % 16) return EA_E_BADARG;
    p.mu[i] = mu_params[i];
  }
  return ea::ceva_decode_launch(ea::DEC_CLOSE, p, (hipStream_t)stream, g.l16);
}
// dec_fill, and what attn and attn_split add to it: the output rows and the bias
static int dec_fill_attn(const DecG& g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad, const float* bias,
                         const ea_t4* lk, const ea_t4* lv, const ea_t4* out, ea::DecP& p) {
  const int rc = dec_fill(g, q, k, v, pad, lk, lv, p);
  if (rc != EA_OK) return rc;
  if (!view_ok(out, g.D, g.dtype == EA_F32 ? 4 : 2) || (g.has_bias && !bias)) return EA_E_BADARG;
  p.o = dec_mk(out);
  p.bias = g.has_bias ? bias : nullptr;
  return EA_OK;
}
static int dec_attn(const DecG& g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad, const float* bias,
                    const ea_t4* lk, const ea_t4* lv, const ea_t4* out, void* stream) {
  ea::DecP p = {};
  const int rc = dec_fill_attn(g, q, k, v, pad, bias, lk, lv, out, p);
  return rc != EA_OK ? rc : ea::ceva_decode_launch(ea::DEC_ATTN, p, (hipStream_t)stream, g.l16);
}
// What the two launches of a split step add to a static step: 2 .. 64 parts, a 16-byte aligned workspace of fp32 partials
// [B, H, 8, parts, D + 4], and a step of at most 8 tokens (one query group per window block).  Decided first, like every
// EA_E_BADARG of the static state.
static int split_check(const ea_ceva_sdec_geom* g, int parts, const void* ws) {
  return g && g->pos && parts >= 2 && parts <= 64 && ws && (uintptr_t)ws % 16 == 0 && g->T_new <= 8 ? EA_OK : EA_E_BADARG;
}
static int dec_attn_split(const ea_ceva_sdec_geom* g, bool l16, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                          const uint8_t* pad, const float* bias, const ea_t4* lk, const ea_t4* lv, const ea_t4* out, int parts,
                          float* ws, void* stream) {
  if (split_check(g, parts, ws) != EA_OK) return EA_E_BADARG;
  ea::DecP p = {};
  const int rc = dec_fill_attn(dec_read(g, l16), q, k, v, pad, bias, lk, lv, out, p);
  return rc != EA_OK ? rc : ea::ceva_sdecode_attn_split(p, parts, ws, (hipStream_t)stream, l16);
}

extern "C" {

int ea_ceva_decode_close(const ea_ceva_dec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                         const float* const* mu_params, const ea_t4* rf_k_bar, const ea_t4* beta, void* stream) {
  return g ? dec_close(dec_read(g), q, k, v, pad, mu_params, rf_k_bar, beta, stream) : EA_E_BADARG;
}

int ea_ceva_decode_attn(const ea_ceva_dec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                        const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, void* stream) {
  return g ? dec_attn(dec_read(g), q, k, v, pad, bias, rf_k_bar, beta, out, stream) : EA_E_BADARG;
}

int ea_ceva_sdecode_append(const ea_ceva_sdec_geom* g, const void* qkv_new, const uint8_t* new_pad, void* qkv, uint8_t* pad,
                           void* stream) {
  if (!g || !qkv_new || !qkv || (uintptr_t)qkv_new % 16 || (uintptr_t)qkv % 16) return EA_E_BADARG;
  const int rc = dec_check(dec_read(g), pad, false);
  if (rc != EA_OK) return rc;
  ea::AppP p = {};
  p.src = (const char*)qkv_new; p.src_pad = new_pad; p.cache = (char*)qkv; p.pad = pad;
  p.pos = g->pos; p.status = g->status; p.ntok = g->ntok;
  p.B = g->B; p.T = g->T_new; p.cap = g->cap; p.ring = g->ring;
  p.row_bytes = 3 * g->H * g->D * (g->dtype == EA_F32 ? 4 : 2);
  return ea::ceva_sdecode_append(p, (hipStream_t)stream);
}

int ea_ceva_sdecode_close(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                          const float* const* mu_params, const ea_t4* rf_k_bar, const ea_t4* beta, void* stream) {
  return g ? dec_close(dec_read(g), q, k, v, pad, mu_params, rf_k_bar, beta, stream) : EA_E_BADARG;
}

int ea_ceva_sdecode_attn(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                         const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, void* stream) {
  return g ? dec_attn(dec_read(g), q, k, v, pad, bias, rf_k_bar, beta, out, stream) : EA_E_BADARG;
}

int ea_ceva_sdecode_attn_split(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                               const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, int32_t parts,
                               float* ws, void* stream) {
  return dec_attn_split(g, false, q, k, v, pad, bias, rf_k_bar, beta, out, parts, ws, stream);
}

// a compact state's close, attn and attn_split: rf_k_bar and beta are rows of g->dtype (bf16 or fp16)
int ea_ceva_sdecode_close_l16(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                              const float* const* mu_params, const ea_t4* rf_k_bar, const ea_t4* beta, void* stream) {
  return g ? dec_close(dec_read(g, true), q, k, v, pad, mu_params, rf_k_bar, beta, stream) : EA_E_BADARG;
}

int ea_ceva_sdecode_attn_l16(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v, const uint8_t* pad,
                             const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta, const ea_t4* out, void* stream) {
  return g ? dec_attn(dec_read(g, true), q, k, v, pad, bias, rf_k_bar, beta, out, stream) : EA_E_BADARG;
}

int ea_ceva_sdecode_attn_split_l16(const ea_ceva_sdec_geom* g, const ea_t4* q, const ea_t4* k, const ea_t4* v,
                                   const uint8_t* pad, const float* bias, const ea_t4* rf_k_bar, const ea_t4* beta,
                                   const ea_t4* out, int32_t parts, float* ws, void* stream) {
  return dec_attn_split(g, true, q, k, v, pad, bias, rf_k_bar, beta, out, parts, ws, stream);
}

int ea_ceva_sdecode_merge(const ea_ceva_sdec_geom* g, const ea_t4* out, int32_t parts, const float* ws, void* stream) {
  if (split_check(g, parts, ws) != EA_OK) return EA_E_BADARG;
  const DecG dg = dec_read(g);
  const int rc = dec_check(dg, nullptr, true, false);
  if (rc != EA_OK) return rc;
  if (!view_ok(out, dg.D, dg.dtype == EA_F32 ? 4 : 2)) return EA_E_BADARG;
  ea::DecMergeP p = {};
  p.o = dec_mk(out); p.ws = ws; p.pos = dg.pos; p.ntok = dg.ntok;
  p.H = dg.H; p.T = dg.T_new; p.cap = dg.cap; p.parts = parts;
  return ea::ceva_sdecode_merge(p, dg.D, dg.dtype, dg.B * dg.H, (hipStream_t)stream);
}

int ea_ceva_sdecode_advance(const ea_ceva_sdec_geom* g, void* stream) {
  if (!g || !g->pos || (uintptr_t)g->pos % 4 || g->T_new <= 0 || g->cap < g->T_new) return EA_E_BADARG;
  if (g->ntok && ((uintptr_t)g->ntok % 4 || g->B <= 0)) return EA_E_BADARG;
  return ea::ceva_sdecode_advance(const_cast<int32_t*>(g->pos), g->ntok, g->B, g->T_new, g->cap, (hipStream_t)stream);
}

}  // extern "C"

// ---- the few-row passes on a held table: what each entry refuses as a bad argument, group by group.  Every entry asks its
// groups first and the geometry (EA_E_UNSUPPORTED) last, so no bad argument is ever reported as an unsupported shape. -------
static int64_t dec_row_bytes(int64_t ld, int dtype) { return ld * (dtype == EA_F32 ? 4 : 2); }

// x [M, ldx] in fp32 or the table's type against the 16-bit table w [., K]
static bool dec_table_ok(int M, int K, const void* x, int x_dtype, int64_t ldx, const void* w, int w_dtype) {
  if (!x || !w || (uintptr_t)x % 16 || (uintptr_t)w % 16) return false;
  if (w_dtype != EA_BF16 && w_dtype != EA_F16) return false;
  if (x_dtype != EA_F32 && x_dtype != w_dtype) return false;
  return M >= 1 && K >= 1 && ldx >= K && dec_row_bytes(ldx, x_dtype) % 16 == 0;
}

// a linear's y [M, ldy] in fp32 or the weight's type, and its optional bias
static bool dec_lin_out_ok(int N, const void* bias, const void* y, int y_dtype, int64_t ldy, int w_dtype) {
  if (!y || (uintptr_t)y % 16 || (uintptr_t)bias % 16) return false;
  if (y_dtype != EA_F32 && y_dtype != w_dtype) return false;
  return N >= 1 && ldy >= N && dec_row_bytes(ldy, y_dtype) % 16 == 0;
}

// a vocab pass's optional logits [M, ldl] in fp32 or the table's type
static bool dec_logits_ok(int V, const void* logits, int logits_dtype, int64_t ldl, int w_dtype) {
  if (!logits) return true;
  if (logits_dtype != EA_F32 && logits_dtype != w_dtype) return false;
  return (uintptr_t)logits % (logits_dtype == EA_F32 ? 4 : 2) == 0 && ldl >= V;
}

// a vocab pass's candidates workspace and what the pick writes (top: optional).  (need < 0: a geometry the entry refuses)
static bool dec_pick_ok(int M, int V, const void* ws, int64_t ws_bytes, const int64_t* token, const float* top) {
  if (!ws || !token || (uintptr_t)ws % 16 || (uintptr_t)token % 8 || (uintptr_t)top % 4) return false;
  const int64_t need = ea::ceva_sdecode_vocab_ws(M, V);
  return need < 0 || ws_bytes >= need;
}

// the sampler's state, optional outputs and arguments but for top_k's upper bound: that one is geometry
static bool dec_sampler_ok(int top_k, float top_p, float temperature, const int64_t* ctr, const int32_t* sid,
                           const int32_t* sel_idx, const float* sel_val, const int32_t* kept) {
  if (!ctr || !sid || (uintptr_t)ctr % 8 || (uintptr_t)sid % 4) return false;
  if ((uintptr_t)sel_idx % 4 || (uintptr_t)sel_val % 4 || (uintptr_t)kept % 4) return false;
  return top_p > 0.f && top_p <= 1.f && std::isfinite(temperature) && temperature > 0.f && top_k >= 1;
}

// the scorer's workspace and outputs (targets: optional)
static bool dec_scorer_ok(int M, int V, const void* lws, int64_t lws_bytes, const int64_t* targets, const float* lse,
                          const float* logp) {
  if (!lws || !lse || !logp || (uintptr_t)lws % 16 || (uintptr_t)lse % 4 || (uintptr_t)logp % 4 || (uintptr_t)targets % 8)
    return false;
  const int64_t need = ea::ceva_sdecode_vocab_lse_ws(M, V);
  return need < 0 || lws_bytes >= need;
}

static bool dec_vocab_geometry_ok(int M, int K, int V) { return M <= EA_CEVA_LINEAR_MAX_ROWS && K % 32 == 0 && V >= 1; }

// the fields DecVocabP and DecLseP share
template <typename P>
static void dec_vocab_fill(P* p, int M, int K, int V, const void* x, int x_dtype, int64_t ldx, const void* w, int w_dtype,
                           void* logits, int logits_dtype, int64_t ldl, void* ws) {
  p->x = (const char*)x; p->w = (const char*)w; p->logits = (char*)logits; p->ws = (ea::VocPick*)ws;
  p->ldx = ldx; p->ldl = logits ? ldl : 0; p->M = M; p->K = K; p->V = V; p->dtype = w_dtype;
  p->x_f32 = x_dtype == EA_F32; p->l_f32 = logits && logits_dtype == EA_F32;
}

// DecLseP's own workspace, behind dec_vocab_fill (M and V are read): lws [M, ceil(V / 16)], then tlogit [M]
static void dec_scorer_fill(ea::DecLseP* p, void* lws, float* lse, float* logp) {
  p->lws = (float*)lws; p->tlogit = p->lws + (int64_t)p->M * ((p->V - 1) / ea::VOC_TILE + 1);
  p->lse = lse; p->logp = logp;
}

static ea::DecSampleP dec_sample_fill(int V, const void* ws, float* logits, int64_t ldl, int top_k, float top_p,
                                      float temperature, uint64_t seed, int64_t* ctr, const int32_t* sid, int64_t* token,
                                      int32_t* sel_idx, float* sel_val, int32_t* kept) {
  ea::DecSampleP s = {};
  s.ws = (const ea::VocPick*)ws; s.logits = logits; s.token = token; s.ctr = ctr; s.sid = sid;
  s.sel_idx = sel_idx; s.sel_val = sel_val; s.kept = kept; s.ldl = ldl; s.V = V; s.top_k = top_k;
  s.top_p = top_p; s.temperature = temperature; s.seed_lo = (uint32_t)seed; s.seed_hi = (uint32_t)(seed >> 32);
  return s;
}

// the state and the outputs of a merge, the optional reports and the scalars but for the envelope: that one is geometry
static bool dec_beam_ok(int W, int eos, int max_new, const float* score, const int32_t* t, const int32_t* nfin,
                        const int32_t* done, const int64_t* token, const int64_t* parent, const int32_t* hist_tok,
                        const int32_t* hist_par, const float* fin_score, const int32_t* fin_len, const int32_t* fin_beam,
                        const int32_t* cand_idx, const float* cand_score, const float* lse, const float* sel_val) {
  if (!score || !t || !nfin || !done || !token || !parent || !hist_tok || !hist_par || !fin_score || !fin_len || !fin_beam)
    return false;
  if ((uintptr_t)token % 8 || (uintptr_t)parent % 8) return false;
  for (const void* q : {(const void*)score, (const void*)t, (const void*)nfin, (const void*)done, (const void*)hist_tok,
                        (const void*)hist_par, (const void*)fin_score, (const void*)fin_len, (const void*)fin_beam,
                        (const void*)cand_idx, (const void*)cand_score, (const void*)lse, (const void*)sel_val})
    if ((uintptr_t)q % 4) return false;
  return W >= 1 && eos >= 0 && max_new >= 1;
}

// the merge's block: what ea_beam_merge reads; ea_ceva_sdecode_vocab_beam adds the row kernel's fields
static ea::DecBeamP dec_beam_fill(int S, int W, int kc, int eos, int max_new, float* score, int32_t* t, int32_t* nfin,
                                  int32_t* done, int64_t* token, int64_t* parent, int32_t* hist_tok, int32_t* hist_par,
                                  float* fin_score, int32_t* fin_len, int32_t* fin_beam, int32_t* cand_idx,
                                  float* cand_score) {
  ea::DecBeamP b = {};
  b.S = S; b.W = W; b.kc = kc; b.eos = eos; b.max_new = max_new; b.score = score; b.t = t; b.nfin = nfin; b.done = done;
  b.token = token; b.parent = parent; b.hist_tok = hist_tok; b.hist_par = hist_par; b.fin_score = fin_score;
  b.fin_len = fin_len; b.fin_beam = fin_beam; b.cand_idx = cand_idx; b.cand_score = cand_score;
  return b;
}

// the constraints of a beam step (ABI 36) -> c but for ban, nban and cap; V < 0: no table to hold the static bans against.
// EA_E_BADARG, or 0
static int dec_bans_fill(ea::BeamBanP* c, int S, int W, int eos, int max_new, int64_t V, int min_len, int ngram,
                         const int32_t* ban_tokens, int n_ban_tokens, const int32_t* prompt_tok, int prompt_cap,
                         const int32_t* prompt_len, const int32_t* t, const int32_t* done, const int32_t* hist_tok,
                         const int32_t* hist_par, int32_t* gen) {
  if (max_new < 1 || min_len < 0 || min_len > max_new - 1 || ngram < 0 || ngram > ea::BAN_MAX_NGRAM || n_ban_tokens < 0 ||
      n_ban_tokens > ea::BAN_MAX_STATIC || (n_ban_tokens > 0 && !ban_tokens) || prompt_cap < 0 ||
      (prompt_cap > 0 && (!prompt_tok || !prompt_len)) || !gen) return EA_E_BADARG;
  if ((uintptr_t)prompt_tok % 4 || (uintptr_t)prompt_len % 4 || (uintptr_t)gen % 4) return EA_E_BADARG;
  *c = ea::BeamBanP{};
  for (int j = 0; j < n_ban_tokens; ++j) {
    if (ban_tokens[j] < 0 || ban_tokens[j] == eos || (V >= 0 && ban_tokens[j] >= V)) return EA_E_BADARG;
    c->static_tok[j] = ban_tokens[j];
  }
  c->t = t; c->done = done; c->hist_tok = hist_tok; c->hist_par = hist_par; c->prompt_tok = prompt_tok;
  c->prompt_len = prompt_len; c->gen = gen; c->S = S; c->W = W; c->eos = eos; c->max_new = max_new; c->min_len = min_len;
  c->ngram = ngram; c->prompt_cap = prompt_cap; c->n_static = n_ban_tokens;
  return 0;
}

extern "C" {

int ea_ceva_sdecode_linear(int32_t M, int32_t K, int32_t N, const void* x, int32_t x_dtype, int64_t ldx,
                           const void* w, int32_t w_dtype, const void* bias, void* y, int32_t y_dtype, int64_t ldy,
                           void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !dec_lin_out_ok(N, bias, y, y_dtype, ldy, w_dtype)) return EA_E_BADARG;
  if (M > EA_CEVA_LINEAR_MAX_ROWS || K % 32 || N % 16) return EA_E_UNSUPPORTED;
  ea::DecLinP p = {};
  p.x = (const char*)x; p.w = (const char*)w; p.bias = (const char*)bias; p.y = (char*)y;
  p.ldx = ldx; p.ldy = ldy; p.M = M; p.K = K; p.N = N; p.dtype = w_dtype;
  p.x_f32 = x_dtype == EA_F32; p.y_f32 = y_dtype == EA_F32;
  return ea::ceva_sdecode_linear(p, (hipStream_t)stream);
}

int ea_ceva_sdecode_linear_fused(int32_t M, int32_t K, int32_t N, const void* x, int32_t x_dtype, int64_t ldx,
                                 const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w, int32_t w_dtype,
                                 const void* bias, int32_t act, const void* res, int32_t res_dtype, int64_t ldr, void* y,
                                 int32_t y_dtype, int64_t ldy, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !dec_lin_out_ok(N, bias, y, y_dtype, ldy, w_dtype)) return EA_E_BADARG;
  // the prologue's and the epilogue's operands
  if ((ln_gamma == nullptr) != (ln_beta == nullptr)) return EA_E_BADARG;
  if ((uintptr_t)ln_gamma % 16 || (uintptr_t)ln_beta % 16 || (uintptr_t)res % 16) return EA_E_BADARG;
  if (ln_gamma && !(std::isfinite(ln_eps) && ln_eps > 0.f)) return EA_E_BADARG;
  if (res) {
    if (res_dtype != EA_F32 && res_dtype != w_dtype) return EA_E_BADARG;
    if (ldr < N || dec_row_bytes(ldr, res_dtype) % 16) return EA_E_BADARG;
  }
  if (x == y) return EA_E_BADARG;
  if (M > EA_CEVA_LINEAR_MAX_ROWS || K % 32 || N % 16) return EA_E_UNSUPPORTED;
  if (act != 0 && act != 1) return EA_E_UNSUPPORTED;
  ea::DecLinFusedP p = {};
  p.x = (const char*)x; p.w = (const char*)w; p.bias = (const char*)bias; p.y = (char*)y;
  p.gamma = ln_gamma; p.beta = ln_beta; p.ln_eps = ln_gamma ? ln_eps : 0.f;
  p.res = (const char*)res; p.res_f32 = res && res_dtype == EA_F32; p.ldr = res ? ldr : 0;
  p.ldx = ldx; p.ldy = ldy; p.M = M; p.K = K; p.N = N; p.dtype = w_dtype; p.act = act;
  p.x_f32 = x_dtype == EA_F32; p.y_f32 = y_dtype == EA_F32;
  return ea::ceva_sdecode_linear_fused(p, (hipStream_t)stream);
}

int64_t ea_ceva_sdecode_vocab_ws(int32_t M, int32_t V) { return ea::ceva_sdecode_vocab_ws(M, V); }

int ea_ceva_sdecode_vocab_argmax(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                 const void* w, int32_t w_dtype, void* logits, int32_t logits_dtype, int64_t ldl,
                                 void* ws, int64_t ws_bytes, int64_t* token, float* top, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !dec_logits_ok(V, logits, logits_dtype, ldl, w_dtype) ||
      !dec_pick_ok(M, V, ws, ws_bytes, token, top)) return EA_E_BADARG;
  if (!dec_vocab_geometry_ok(M, K, V)) return EA_E_UNSUPPORTED;
  ea::DecVocabP p = {};
  dec_vocab_fill(&p, M, K, V, x, x_dtype, ldx, w, w_dtype, logits, logits_dtype, ldl, ws);
  p.token = token; p.top = top;
  return ea::ceva_sdecode_vocab_argmax(p, (hipStream_t)stream);
}

int64_t ea_ceva_sdecode_vocab_sample_ws(int32_t M, int32_t V) { return ea::ceva_sdecode_vocab_ws(M, V); }

// (the logits are required and fp32)
int ea_ceva_sdecode_vocab_sample(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                 const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws, int64_t ws_bytes,
                                 int32_t top_k, float top_p, float temperature, uint64_t seed, int64_t* ctr,
                                 const int32_t* sid, int64_t* token, int32_t* sel_idx, float* sel_val, int32_t* kept,
                                 void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !logits || !dec_logits_ok(V, logits, EA_F32, ldl, w_dtype) ||
      !dec_pick_ok(M, V, ws, ws_bytes, token, nullptr) ||
      !dec_sampler_ok(top_k, top_p, temperature, ctr, sid, sel_idx, sel_val, kept)) return EA_E_BADARG;
  if (top_k > 64 || !dec_vocab_geometry_ok(M, K, V)) return EA_E_UNSUPPORTED;
  ea::DecVocabP p = {};
  dec_vocab_fill(&p, M, K, V, x, x_dtype, ldx, w, w_dtype, logits, EA_F32, ldl, ws);
  const ea::DecSampleP s = dec_sample_fill(V, ws, logits, ldl, top_k, top_p, temperature, seed, ctr, sid, token, sel_idx,
                                           sel_val, kept);
  return ea::ceva_sdecode_vocab_sample(p, s, (hipStream_t)stream);
}

int64_t ea_ceva_sdecode_vocab_lse_ws(int32_t M, int32_t V) { return ea::ceva_sdecode_vocab_lse_ws(M, V); }

int ea_ceva_sdecode_vocab_logprob(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                  const void* w, int32_t w_dtype, void* logits, int32_t logits_dtype, int64_t ldl,
                                  void* ws, int64_t ws_bytes, int64_t* token, float* top, void* lws, int64_t lws_bytes,
                                  const int64_t* targets, float* lse, float* logp, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !dec_logits_ok(V, logits, logits_dtype, ldl, w_dtype) ||
      !dec_pick_ok(M, V, ws, ws_bytes, token, top) || !dec_scorer_ok(M, V, lws, lws_bytes, targets, lse, logp))
    return EA_E_BADARG;
  if (!dec_vocab_geometry_ok(M, K, V)) return EA_E_UNSUPPORTED;
  ea::DecLseP p = {};
  dec_vocab_fill(&p, M, K, V, x, x_dtype, ldx, w, w_dtype, logits, logits_dtype, ldl, ws);
  dec_scorer_fill(&p, lws, lse, logp);
  p.token = token; p.top = top; p.targets = targets;
  return ea::ceva_sdecode_vocab_logprob(p, (hipStream_t)stream);
}

// (the logits are required and fp32; the scorer reads the drawn tokens, not targets)
int ea_ceva_sdecode_vocab_sample_logprob(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                         const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws,
                                         int64_t ws_bytes, int32_t top_k, float top_p, float temperature, uint64_t seed,
                                         int64_t* ctr, const int32_t* sid, int64_t* token, int32_t* sel_idx, float* sel_val,
                                         int32_t* kept, void* lws, int64_t lws_bytes, float* lse, float* logp, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !logits || !dec_logits_ok(V, logits, EA_F32, ldl, w_dtype) ||
      !dec_pick_ok(M, V, ws, ws_bytes, token, nullptr) ||
      !dec_sampler_ok(top_k, top_p, temperature, ctr, sid, sel_idx, sel_val, kept) ||
      !dec_scorer_ok(M, V, lws, lws_bytes, nullptr, lse, logp)) return EA_E_BADARG;
  if (top_k > 64 || !dec_vocab_geometry_ok(M, K, V)) return EA_E_UNSUPPORTED;
  ea::DecLseP p = {};
  dec_vocab_fill(&p, M, K, V, x, x_dtype, ldx, w, w_dtype, logits, EA_F32, ldl, ws);
  dec_scorer_fill(&p, lws, lse, logp);
  p.token_in = token;
  const ea::DecSampleP s = dec_sample_fill(V, ws, logits, ldl, top_k, top_p, temperature, seed, ctr, sid, token, sel_idx,
                                           sel_val, kept);
  return ea::ceva_sdecode_vocab_sample_logprob(p, s, (hipStream_t)stream);
}

// ---- the beam step (ABI 32): the table operands, the logits, the workspace, then the beam's state and outputs; the
// geometry last -------------------------------------------------------------------------------------------------------------
int64_t ea_ceva_sdecode_vocab_beam_ws(int32_t M, int32_t V, int32_t W) { return ea::ceva_sdecode_vocab_beam_ws(M, V, W); }

// (the logits are required and fp32)
int ea_ceva_sdecode_vocab_beam(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                               const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws, int64_t ws_bytes,
                               int32_t W, int32_t eos, int32_t max_new, float* score, int32_t* t, int32_t* nfin,
                               int32_t* done, int64_t* token, int64_t* parent, int32_t* hist_tok, int32_t* hist_par,
                               float* fin_score, int32_t* fin_len, int32_t* fin_beam, int32_t* cand_idx, float* cand_score,
                               float* lse, float* sel_val, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !logits || !dec_logits_ok(V, logits, EA_F32, ldl, w_dtype) ||
      !ws || (uintptr_t)ws % 16 ||
      !dec_beam_ok(W, eos, max_new, score, t, nfin, done, token, parent, hist_tok, hist_par, fin_score, fin_len, fin_beam,
                   cand_idx, cand_score, lse, sel_val) || (V >= 1 && eos >= V)) return EA_E_BADARG;
  const int64_t need = ea::ceva_sdecode_vocab_beam_ws(M, V, W);
  if (need >= 0 && ws_bytes < need) return EA_E_BADARG;
  if (W > 32 || M % W || !dec_vocab_geometry_ok(M, K, V) || need < 0) return EA_E_UNSUPPORTED;
  ea::DecLseP p = {};
  dec_vocab_fill(&p, M, K, V, x, x_dtype, ldx, w, w_dtype, logits, EA_F32, ldl, ws);
  ea::DecBeamP b = dec_beam_fill(M / W, W, 2 * W < V ? 2 * W : V, eos, max_new, score, t, nfin, done, token, parent, hist_tok,
                                 hist_par, fin_score, fin_len, fin_beam, cand_idx, cand_score);
  b.logits = logits; b.ldl = ldl; b.V = V; b.lse = lse; b.sel_val = sel_val;
  ea::ceva_sdecode_vocab_beam_carve(ws, &p, &b);
  p.token = token;                                        // (required by the block; the table pass does not write it)
  return ea::ceva_sdecode_vocab_beam(p, b, (hipStream_t)stream);
}

int ea_beam_merge(int32_t S, int32_t W, int32_t kc, const int32_t* cand_idx, const float* cand_score, int32_t eos,
                  int32_t max_new, float* score, int32_t* t, int32_t* nfin, int32_t* done, int64_t* token, int64_t* parent,
                  int32_t* hist_tok, int32_t* hist_par, float* fin_score, int32_t* fin_len, int32_t* fin_beam, void* stream) {
  if (S < 1 || !cand_idx || !cand_score ||
      !dec_beam_ok(W, eos, max_new, score, t, nfin, done, token, parent, hist_tok, hist_par, fin_score, fin_len, fin_beam,
                   cand_idx, cand_score, nullptr, nullptr) || kc < 1 || kc > 2 * (int64_t)W) return EA_E_BADARG;
  if (W > 32 || (int64_t)S * W > EA_CEVA_LINEAR_MAX_ROWS) return EA_E_UNSUPPORTED;
  const ea::DecBeamP b = dec_beam_fill(S, W, kc, eos, max_new, score, t, nfin, done, token, parent, hist_tok, hist_par,
                                       fin_score, fin_len, fin_beam, (int32_t*)cand_idx, (float*)cand_score);
  return ea::ceva_beam_merge(b, (hipStream_t)stream);
}

// ---- the constrained beam step (ABI 36): the unconstrained entry's groups in their order, then the constraints, the prompt
// and the beams' generated tokens ---------------------------------------------------------------------------------------------
int ea_beam_bans(int32_t S, int32_t W, int32_t eos, int32_t max_new, int32_t min_len, int32_t ngram, const int32_t* ban_tokens,
                 int32_t n_ban_tokens, const int32_t* prompt_tok, int32_t prompt_cap, const int32_t* prompt_len,
                 const int32_t* t, const int32_t* done, const int32_t* hist_tok, const int32_t* hist_par, int32_t* gen,
                 int32_t* ban, int32_t cap, int32_t* nban, void* stream) {
  if (S < 1 || W < 1 || eos < 0 || !t || !done || !hist_tok || !hist_par || !ban || !nban) return EA_E_BADARG;
  for (const void* q : {(const void*)t, (const void*)done, (const void*)hist_tok, (const void*)hist_par, (const void*)ban,
                        (const void*)nban})
    if ((uintptr_t)q % 4) return EA_E_BADARG;
  ea::BeamBanP c;
  if (const int rc = dec_bans_fill(&c, S, W, eos, max_new, -1, min_len, ngram, ban_tokens, n_ban_tokens, prompt_tok, prompt_cap,
                                   prompt_len, t, done, hist_tok, hist_par, gen)) return rc;
  if ((int64_t)cap < ea::beam_ban_cap(prompt_cap, max_new)) return EA_E_BADARG;
  if (W > 32 || (int64_t)S * W > EA_CEVA_LINEAR_MAX_ROWS) return EA_E_UNSUPPORTED;
  c.ban = ban; c.nban = nban; c.cap = cap;
  return ea::ceva_beam_bans(c, (hipStream_t)stream);
}

int64_t ea_ceva_sdecode_vocab_beam_c_ws(int32_t M, int32_t V, int32_t W, int32_t prompt_cap, int32_t max_new) {
  const int64_t base = ea::ceva_sdecode_vocab_beam_ws(M, V, W), more = ea::ceva_beam_bans_ws(M, prompt_cap, max_new);
  return base < 0 || more < 0 ? -1 : base + more;
}

// (the logits are required and fp32)
int ea_ceva_sdecode_vocab_beam_c(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx,
                                 const void* w, int32_t w_dtype, float* logits, int64_t ldl, void* ws, int64_t ws_bytes,
                                 int32_t W, int32_t eos, int32_t max_new, float* score, int32_t* t, int32_t* nfin,
                                 int32_t* done, int64_t* token, int64_t* parent, int32_t* hist_tok, int32_t* hist_par,
                                 float* fin_score, int32_t* fin_len, int32_t* fin_beam, int32_t* cand_idx, float* cand_score,
                                 float* lse, float* sel_val, int32_t min_len, int32_t ngram, const int32_t* ban_tokens,
                                 int32_t n_ban_tokens, const int32_t* prompt_tok, int32_t prompt_cap,
                                 const int32_t* prompt_len, int32_t* gen, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !logits || !dec_logits_ok(V, logits, EA_F32, ldl, w_dtype) ||
      !ws || (uintptr_t)ws % 16 ||
      !dec_beam_ok(W, eos, max_new, score, t, nfin, done, token, parent, hist_tok, hist_par, fin_score, fin_len, fin_beam,
                   cand_idx, cand_score, lse, sel_val) || (V >= 1 && eos >= V)) return EA_E_BADARG;
  ea::BeamBanP c;
  if (const int rc = dec_bans_fill(&c, M / W, W, eos, max_new, V >= 1 ? V : -1, min_len, ngram, ban_tokens, n_ban_tokens,
                                   prompt_tok, prompt_cap, prompt_len, t, done, hist_tok, hist_par, gen)) return rc;
  const int64_t base = ea::ceva_sdecode_vocab_beam_ws(M, V, W);
  const int64_t need = ea_ceva_sdecode_vocab_beam_c_ws(M, V, W, prompt_cap, max_new);
  if (need >= 0 && ws_bytes < need) return EA_E_BADARG;
  if (W > 32 || M % W || !dec_vocab_geometry_ok(M, K, V) || need < 0) return EA_E_UNSUPPORTED;
  ea::DecLseP p = {};
  dec_vocab_fill(&p, M, K, V, x, x_dtype, ldx, w, w_dtype, logits, EA_F32, ldl, ws);
  ea::DecBeamP b = dec_beam_fill(M / W, W, 2 * W < V ? 2 * W : V, eos, max_new, score, t, nfin, done, token, parent, hist_tok,
                                 hist_par, fin_score, fin_len, fin_beam, cand_idx, cand_score);
  b.logits = logits; b.ldl = ldl; b.V = V; b.lse = lse; b.sel_val = sel_val;
  ea::ceva_sdecode_vocab_beam_carve(ws, &p, &b);
  ea::ceva_beam_bans_carve((char*)ws + base, M, &c);
  p.token = token;                                        // (required by the block; the table pass does not write it)
  return ea::ceva_sdecode_vocab_beam_c(p, b, c, (hipStream_t)stream);
}

// ---- the many-row vocabulary pass (ABI 30, ea_vocab_score.hip): the few-row entries' groups in their order -- the table
// operands, the optional logits, then the workspace and the outputs -- and the geometry last ---------------------------------
int64_t ea_vocab_score_ws(int32_t M, int32_t V) { return ea::vocab_score_ws(M, V); }

int32_t ea_vocab_score_tile(int32_t which) {
  switch (which) {
    case 0: return ea::VS_BM;
    case 1: return ea::VS_BN;
    case 2: return ea::VS_SL;
    default: return EA_E_BADARG;
  }
}

int ea_vocab_score(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                   int32_t w_dtype, const int64_t* targets, void* logits, int32_t logits_dtype, int64_t ldl, void* ws,
                   int64_t ws_bytes, int64_t* token, float* top, float* lse, float* logp, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !dec_logits_ok(V, logits, logits_dtype, ldl, w_dtype)) return EA_E_BADARG;
  if (!ws || !token || !lse || !logp) return EA_E_BADARG;
  if ((uintptr_t)ws % 16 || (uintptr_t)token % 8 || (uintptr_t)targets % 8) return EA_E_BADARG;
  if ((uintptr_t)top % 4 || (uintptr_t)lse % 4 || (uintptr_t)logp % 4) return EA_E_BADARG;
  const int64_t need = ea::vocab_score_ws(M, V);       // (< 0: a geometry refused below)
  if (need >= 0 && ws_bytes < need) return EA_E_BADARG;
  if (K % 32 || V < 1 || need < 0) return EA_E_UNSUPPORTED;
  ea::VocabScoreP p = {};
  p.x = (const char*)x; p.w = (const char*)w; p.targets = targets; p.logits = (char*)logits; p.pick = (ea::VsPick*)ws;
  p.token = token; p.top = top; p.lse = lse; p.logp = logp;
  p.ldx = ldx; p.ldl = logits ? ldl : 0; p.M = M; p.K = K; p.V = V; p.dtype = w_dtype;
  p.x_f32 = x_dtype == EA_F32; p.l_f32 = logits && logits_dtype == EA_F32;
  return ea::vocab_score(p, (hipStream_t)stream);
}

// ---- the vocabulary cross-entropy's backward (ABI 38, ea_vocab_nll.hip): the chunk's logit gradient and the plain GEMM ----------
int32_t ea_vocab_nll_chunk(int32_t M, int32_t V) { return ea::vocab_nll_chunk(M, V); }

int64_t ea_vocab_nll_ws(int32_t M, int32_t K, int32_t V, int32_t chunk_cols) { return ea::vocab_nll_ws(M, K, V, chunk_cols); }

int ea_vocab_nll_grad(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                      int32_t w_dtype, const int64_t* targets, const float* lse, const float* d, int32_t v0, int32_t Vc,
                      void* g, int64_t ldg, void* gt, int64_t ldm, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype)) return EA_E_BADARG;
  if (!targets || !lse || !d || !g || !gt) return EA_E_BADARG;
  if ((uintptr_t)targets % 8 || (uintptr_t)lse % 4 || (uintptr_t)d % 4 || (uintptr_t)g % 16 || (uintptr_t)gt % 16) return EA_E_BADARG;
  if (v0 < 0 || Vc < 1 || v0 % ea::VS_SL || (V >= 1 && (int64_t)v0 + Vc > V)) return EA_E_BADARG;
  if (ldg < Vc || ldm < M || ldg % 64 || ldm % 64) return EA_E_BADARG;
  const int64_t grid = (((int64_t)M - 1) / ea::VS_BM + 1) * (((int64_t)Vc - 1) / ea::VS_SL + 1);
  if (K % 32 || V < 1 || grid > ea::VS_MAX_WORKGROUPS) return EA_E_UNSUPPORTED;
  ea::VocabNllGradP p = {};
  p.x = (const char*)x; p.w = (const char*)w; p.targets = targets; p.ldx = ldx; p.M = M; p.K = K; p.V = V; p.dtype = w_dtype;
  p.x_f32 = x_dtype == EA_F32;
  p.lse_in = lse; p.d = d; p.g = (uint16_t*)g; p.gt = (uint16_t*)gt; p.ldg = ldg; p.ldm = ldm; p.v0 = v0; p.Vc = Vc;
  return ea::vocab_nll_grad(p, (hipStream_t)stream);
}

int ea_gemm_nt16(int32_t M, int32_t N, int32_t K, const void* a, int64_t lda, const void* b, int64_t ldb, int32_t dtype,
                 float* out, int64_t ldo, int32_t accumulate, void* stream) {
  if (!a || !b || !out || (uintptr_t)a % 16 || (uintptr_t)b % 16 || (uintptr_t)out % 4) return EA_E_BADARG;
  if (dtype != EA_BF16 && dtype != EA_F16) return EA_E_BADARG;
  if (M < 1 || N < 1 || K < 1 || lda < K || ldb < K || ldo < N || lda % 8 || ldb % 8) return EA_E_BADARG;
  if (accumulate != 0 && accumulate != 1) return EA_E_BADARG;
  const int64_t grid = (((int64_t)M - 1) / ea::VS_BM + 1) * (((int64_t)N - 1) / ea::VS_BN + 1);
  if (K % 32 || grid > ea::VS_MAX_WORKGROUPS) return EA_E_UNSUPPORTED;
  ea::GemmNt16P p = {};
  p.x = (const char*)a; p.w = (const char*)b; p.logits = (char*)out; p.ldx = lda; p.ldw = ldb; p.ldl = ldo;
  p.M = M; p.K = K; p.V = N; p.dtype = dtype; p.l_f32 = 1; p.accumulate = accumulate;
  return ea::gemm_nt16(p, (hipStream_t)stream);
}

// ---- adaptive-softmax scoring (ABI 33, ea_adaptive_score.hip): the routing, the vocabulary pass over a row set, the composite.
// Host arrays (cutoffs, dims, the per-tail operand pointers) are read here, before the first launch --------------------------
static bool adp_cutoffs_ok(int32_t n_tails, const int64_t* cutoffs) {
  if (n_tails < 1 || !cutoffs) return false;
  for (int i = 0; i < n_tails && i < EA_ADAPTIVE_MAX_TAILS; ++i)
    if (cutoffs[i + 1] <= cutoffs[i]) return false;
  return cutoffs[0] >= 1;
}

int ea_adaptive_route(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int64_t* targets, int64_t* head_target,
                      int32_t* rows, int32_t* count, void* stream) {
  if (M < 1 || !adp_cutoffs_ok(n_tails, cutoffs) || !targets || !head_target || !rows || !count) return EA_E_BADARG;
  if ((uintptr_t)targets % 8 || (uintptr_t)head_target % 8 || (uintptr_t)rows % 4 || (uintptr_t)count % 4) return EA_E_BADARG;
  if (n_tails > EA_ADAPTIVE_MAX_TAILS || cutoffs[n_tails] > INT32_MAX) return EA_E_UNSUPPORTED;
  ea::AdaptiveRouteP p = {};
  p.targets = targets; p.head_target = head_target; p.rows = rows; p.count = count; p.M = M; p.n = n_tails;
  for (int i = 0; i <= n_tails; ++i) p.cut[i] = cutoffs[i];
  return ea::adaptive_route(p, (hipStream_t)stream);
}

int64_t ea_vocab_score_rows_ws(int32_t M, int32_t V) { return ea::vocab_score_ws(M, V); }

int ea_vocab_score_rows(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                        int32_t w_dtype, const int64_t* targets, void* logits, int32_t logits_dtype, int64_t ldl, void* ws,
                        int64_t ws_bytes, int64_t* token, float* top, float* lse, float* logp, const int32_t* rows,
                        const int32_t* count, int64_t target_base, int32_t logits_only, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype) || !dec_logits_ok(V, logits, logits_dtype, ldl, w_dtype)) return EA_E_BADARG;
  if (logits_only ? !logits : (!token || !lse || !logp)) return EA_E_BADARG;
  if (!ws || (uintptr_t)ws % 16 || (uintptr_t)token % 8 || (uintptr_t)targets % 8) return EA_E_BADARG;
  if ((uintptr_t)top % 4 || (uintptr_t)lse % 4 || (uintptr_t)logp % 4 || (uintptr_t)rows % 4 || (uintptr_t)count % 4) return EA_E_BADARG;
  if (target_base < 0 || (logits_only != 0 && logits_only != 1)) return EA_E_BADARG;
  const int64_t need = ea::vocab_score_ws(M, V);       // (< 0: a geometry refused below)
  if (need >= 0 && ws_bytes < need) return EA_E_BADARG;
  if (K % 32 || V < 1 || need < 0) return EA_E_UNSUPPORTED;
  ea::VocabScoreRowsP p = {};
  p.x = (const char*)x; p.w = (const char*)w; p.targets = logits_only ? nullptr : targets; p.logits = (char*)logits;
  p.pick = (ea::VsPick*)ws; p.token = token; p.top = top; p.lse = lse; p.logp = logp;
  p.ldx = ldx; p.ldl = logits ? ldl : 0; p.M = M; p.K = K; p.V = V; p.dtype = w_dtype;
  p.x_f32 = x_dtype == EA_F32; p.l_f32 = logits && logits_dtype == EA_F32;
  p.xrows = rows; p.trows = rows; p.count = count; p.target_base = target_base; p.logits_only = logits_only;
  return ea::vocab_score_rows(p, (hipStream_t)stream);
}

int64_t ea_adaptive_score_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims) {
  return ea::adaptive_plan(M, n_tails, cutoffs, dims, nullptr);
}

static int adp_score(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                     int32_t x_dtype, int64_t ldx, const int64_t* targets, const void* head, int32_t w_dtype,
                     const void* const* proj, const void* const* tables, const void* const* hmask, void* ws, int64_t ws_bytes,
                     float* logp, int64_t* token_head, void* stream) {
  if (!adp_cutoffs_ok(n_tails, cutoffs) || !dims || !proj || !tables) return EA_E_BADARG;
  for (int i = 0; hmask && i < n_tails && i < EA_ADAPTIVE_MAX_TAILS; ++i)
    if ((uintptr_t)hmask[i] % 16) return EA_E_BADARG;
  if (!dec_table_ok(M, C, x, x_dtype, ldx, head, w_dtype)) return EA_E_BADARG;
  for (int i = 0; i < n_tails && i < EA_ADAPTIVE_MAX_TAILS; ++i)
    if (dims[i] < 1 || !proj[i] || !tables[i] || (uintptr_t)proj[i] % 16 || (uintptr_t)tables[i] % 16) return EA_E_BADARG;
  if (!targets || !ws || !logp || (uintptr_t)targets % 8 || (uintptr_t)ws % 16 || (uintptr_t)logp % 4 || (uintptr_t)token_head % 8)
    return EA_E_BADARG;
  const int64_t need = n_tails <= EA_ADAPTIVE_MAX_TAILS ? ea::adaptive_plan(M, n_tails, cutoffs, dims, nullptr) : -1;
  if (need >= 0 && ws_bytes < need) return EA_E_BADARG;
  if (n_tails > EA_ADAPTIVE_MAX_TAILS || C % 32 || need < 0) return EA_E_UNSUPPORTED;
  for (int i = 0; i < n_tails; ++i)
    if (dims[i] % 32) return EA_E_UNSUPPORTED;
  ea::AdaptiveScoreP p = {};
  p.x = (const char*)x; p.targets = targets; p.head = (const char*)head; p.ws = (char*)ws; p.logp = logp;
  p.token_head = token_head; p.ldx = ldx; p.M = M; p.C = C; p.n = n_tails; p.dtype = w_dtype; p.x_f32 = x_dtype == EA_F32;
  for (int i = 0; i <= n_tails; ++i) p.cut[i] = cutoffs[i];
  for (int i = 0; i < n_tails; ++i) { p.dims[i] = dims[i]; p.proj[i] = (const char*)proj[i]; p.table[i] = (const char*)tables[i]; }
  for (int i = 0; hmask && i < n_tails; ++i) p.hmask[i] = (const char*)hmask[i];
  return ea::adaptive_score(p, (hipStream_t)stream);
}

int ea_adaptive_score(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                      int32_t x_dtype, int64_t ldx, const int64_t* targets, const void* head, int32_t w_dtype,
                      const void* const* proj, const void* const* tables, void* ws, int64_t ws_bytes, float* logp,
                      int64_t* token_head, void* stream) {
  return adp_score(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, targets, head, w_dtype, proj, tables, nullptr, ws, ws_bytes, logp,
                   token_head, stream);
}

// ---- the adaptive-softmax training loss (ea_adaptive_nll.hip): the masked score, the row-set gradient and GEMM, the gathered
// transpose and the workspace query; additions to ABI 38 ---------------------------------------------------------------------------
int ea_adaptive_score_masked(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                             int32_t x_dtype, int64_t ldx, const int64_t* targets, const void* head, int32_t w_dtype,
                             const void* const* proj, const void* const* tables, const void* const* hmask, void* ws,
                             int64_t ws_bytes, float* logp, int64_t* token_head, void* stream) {
  if (!hmask) return EA_E_BADARG;
  return adp_score(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, targets, head, w_dtype, proj, tables, hmask, ws, ws_bytes, logp,
                   token_head, stream);
}

int64_t ea_adaptive_nll_ws(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, int32_t chunk_cols) {
  return ea::adaptive_nll_ws(M, C, n_tails, cutoffs, dims, chunk_cols);
}

int ea_vocab_nll_grad_rows(int32_t M, int32_t K, int32_t V, const void* x, int32_t x_dtype, int64_t ldx, const void* w,
                           int32_t w_dtype, const int64_t* targets, const float* lse, const float* d, int32_t v0, int32_t Vc,
                           void* g, int64_t ldg, void* gt, int64_t ldm, const int32_t* trows, const int32_t* count,
                           int64_t target_base, void* stream) {
  if (!dec_table_ok(M, K, x, x_dtype, ldx, w, w_dtype)) return EA_E_BADARG;
  if (!targets || !lse || !d || !g || !gt) return EA_E_BADARG;
  if ((uintptr_t)targets % 8 || (uintptr_t)lse % 4 || (uintptr_t)d % 4 || (uintptr_t)g % 16 || (uintptr_t)gt % 16) return EA_E_BADARG;
  if ((uintptr_t)trows % 4 || (uintptr_t)count % 4 || target_base < 0) return EA_E_BADARG;
  if (v0 < 0 || Vc < 1 || v0 % ea::VS_SL || (V >= 1 && (int64_t)v0 + Vc > V)) return EA_E_BADARG;
  if (ldg < Vc || ldm < M || ldg % 64 || ldm % 64) return EA_E_BADARG;
  const int64_t grid = (((int64_t)M - 1) / ea::VS_BM + 1) * (((int64_t)Vc - 1) / ea::VS_SL + 1);
  if (K % 32 || V < 1 || grid > ea::VS_MAX_WORKGROUPS) return EA_E_UNSUPPORTED;
  ea::VocabNllGradRowsP p = {};
  p.x = (const char*)x; p.w = (const char*)w; p.targets = targets; p.ldx = ldx; p.M = M; p.K = K; p.V = V; p.dtype = w_dtype;
  p.x_f32 = x_dtype == EA_F32;
  p.lse_in = lse; p.d = d; p.g = (uint16_t*)g; p.gt = (uint16_t*)gt; p.ldg = ldg; p.ldm = ldm; p.v0 = v0; p.Vc = Vc;
  p.trows = trows; p.count = count; p.target_base = target_base;
  return ea::vocab_nll_grad_rows(p, (hipStream_t)stream);
}

int ea_gemm_nt16_rows(int32_t M, int32_t N, int32_t K, const void* a, int64_t lda, const void* b, int64_t ldb, int32_t dtype,
                      float* out, int64_t ldo, int32_t accumulate, const int32_t* orows, const int32_t* count, void* stream) {
  if (!a || !b || !out || (uintptr_t)a % 16 || (uintptr_t)b % 16 || (uintptr_t)out % 4) return EA_E_BADARG;
  if ((uintptr_t)orows % 4 || (uintptr_t)count % 4) return EA_E_BADARG;
  if (dtype != EA_BF16 && dtype != EA_F16) return EA_E_BADARG;
  if (M < 1 || N < 1 || K < 1 || lda < K || ldb < K || ldo < N || lda % 8 || ldb % 8) return EA_E_BADARG;
  if (accumulate != 0 && accumulate != 1) return EA_E_BADARG;
  const int64_t grid = (((int64_t)M - 1) / ea::VS_BM + 1) * (((int64_t)N - 1) / ea::VS_BN + 1);
  if (K % 32 || grid > ea::VS_MAX_WORKGROUPS) return EA_E_UNSUPPORTED;
  ea::GemmNt16RowsP p = {};
  p.x = (const char*)a; p.w = (const char*)b; p.logits = (char*)out; p.ldx = lda; p.ldw = ldb; p.ldl = ldo;
  p.M = M; p.K = K; p.V = N; p.dtype = dtype; p.l_f32 = 1; p.accumulate = accumulate; p.orows = orows; p.count = count;
  return ea::gemm_nt16_rows(p, (hipStream_t)stream);
}

int ea_rows_transpose16(int32_t M, int32_t K, const void* src, int32_t src_dtype, int64_t ld, const int32_t* rows,
                        const int32_t* count, void* out, int32_t out_dtype, int64_t ldm, void* stream) {
  if (!src || !out || (uintptr_t)src % 4 || (uintptr_t)out % 2 || (uintptr_t)rows % 4 || (uintptr_t)count % 4) return EA_E_BADARG;
  if (out_dtype != EA_BF16 && out_dtype != EA_F16) return EA_E_BADARG;
  if (src_dtype != EA_F32 && src_dtype != out_dtype) return EA_E_BADARG;
  if (M < 1 || K < 1 || ld < K || ldm < M || ldm % 64) return EA_E_BADARG;
  if ((((int64_t)K - 1) / 64 + 1) > 65535 || ldm / 64 > INT32_MAX) return EA_E_UNSUPPORTED;
  ea::RowsTransposeP p = {};
  p.src = (const char*)src; p.rows = rows; p.count = count; p.out = (uint16_t*)out; p.ld = ld; p.ldm = ldm; p.M = M; p.K = K;
  p.dtype = out_dtype; p.src_f32 = src_dtype == EA_F32;
  return ea::rows_transpose16(p, (hipStream_t)stream);
}

// ---- the greedy pick from the adaptive head (ABI 34, ea_adaptive_pick.hip): ea_adaptive_score's groups in their order ----------
int64_t ea_adaptive_pick_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims) {
  return ea::adaptive_pick_plan(M, n_tails, cutoffs, dims, nullptr);
}

int ea_adaptive_pick(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                     int32_t x_dtype, int64_t ldx, const int64_t* targets, const void* head, int32_t w_dtype,
                     const void* const* proj, const void* const* tables, void* ws, int64_t ws_bytes, int64_t* token,
                     float* logp, void* stream) {
  if (!adp_cutoffs_ok(n_tails, cutoffs) || !dims || !proj || !tables) return EA_E_BADARG;
  if (!dec_table_ok(M, C, x, x_dtype, ldx, head, w_dtype)) return EA_E_BADARG;
  for (int i = 0; i < n_tails && i < EA_ADAPTIVE_MAX_TAILS; ++i)
    if (dims[i] < 1 || !proj[i] || !tables[i] || (uintptr_t)proj[i] % 16 || (uintptr_t)tables[i] % 16) return EA_E_BADARG;
  if (!ws || !token || !logp || (uintptr_t)targets % 8 || (uintptr_t)ws % 16 || (uintptr_t)token % 8 || (uintptr_t)logp % 4)
    return EA_E_BADARG;
  const bool envelope = n_tails <= EA_ADAPTIVE_MAX_TAILS && M <= EA_CEVA_LINEAR_MAX_ROWS;
  const int64_t need = envelope ? ea::adaptive_pick_plan(M, n_tails, cutoffs, dims, nullptr) : -1;
  if (need >= 0 && ws_bytes < need) return EA_E_BADARG;
  if (!envelope || C % 32 || need < 0) return EA_E_UNSUPPORTED;
  for (int i = 0; i < n_tails; ++i)
    if (dims[i] % 32) return EA_E_UNSUPPORTED;
  ea::AdaptivePickP p = {};
  p.x = (const char*)x; p.targets = targets; p.head = (const char*)head; p.ws = (char*)ws; p.token = token; p.logp = logp;
  p.ldx = ldx; p.M = M; p.C = C; p.n = n_tails; p.dtype = w_dtype; p.x_f32 = x_dtype == EA_F32;
  for (int i = 0; i <= n_tails; ++i) p.cut[i] = cutoffs[i];
  for (int i = 0; i < n_tails; ++i) { p.dims[i] = dims[i]; p.proj[i] = (const char*)proj[i]; p.table[i] = (const char*)tables[i]; }
  return ea::adaptive_pick(p, (hipStream_t)stream);
}

}  // extern "C"

// ---- the sampled pick and the beam step from the adaptive head (ABI 35, ea_adaptive_pick.hip): ea_adaptive_pick's operands,
// then ea_ceva_sdecode_vocab_sample's / ea_beam_merge's groups in their order --------------------------------------------------
// the operands the three adaptive pick entries share: EA_E_BADARG, or 0
static int adp_operands_ok(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                           int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype, const void* const* proj,
                           const void* const* tables, const void* ws) {
  if (!adp_cutoffs_ok(n_tails, cutoffs) || !dims || !proj || !tables) return EA_E_BADARG;
  if (!dec_table_ok(M, C, x, x_dtype, ldx, head, w_dtype)) return EA_E_BADARG;
  for (int i = 0; i < n_tails && i < EA_ADAPTIVE_MAX_TAILS; ++i)
    if (dims[i] < 1 || !proj[i] || !tables[i] || (uintptr_t)proj[i] % 16 || (uintptr_t)tables[i] % 16) return EA_E_BADARG;
  return !ws || (uintptr_t)ws % 16 ? EA_E_BADARG : 0;
}

// the workspace's size and the geometry, behind the argument checks: EA_E_BADARG, EA_E_UNSUPPORTED, or 0
static int adp_select_geometry(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, int32_t W,
                               int64_t ws_bytes) {
  const bool envelope = n_tails <= EA_ADAPTIVE_MAX_TAILS && M <= EA_CEVA_LINEAR_MAX_ROWS && W <= 32 && (W == 0 || M % W == 0);
  const int64_t need = envelope ? ea::adaptive_select_plan(M, n_tails, cutoffs, dims, W, nullptr) : -1;
  if (need >= 0 && ws_bytes < need) return EA_E_BADARG;
  if (!envelope || C % 32 || need < 0) return EA_E_UNSUPPORTED;
  for (int i = 0; i < n_tails; ++i)
    if (dims[i] % 32) return EA_E_UNSUPPORTED;
  return 0;
}

static ea::AdaptivePickP adp_pick_fill(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims,
                                       const void* x, int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype,
                                       const void* const* proj, const void* const* tables, void* ws) {
  ea::AdaptivePickP p = {};
  p.x = (const char*)x; p.head = (const char*)head; p.ws = (char*)ws;
  p.ldx = ldx; p.M = M; p.C = C; p.n = n_tails; p.dtype = w_dtype; p.x_f32 = x_dtype == EA_F32;
  for (int i = 0; i <= n_tails; ++i) p.cut[i] = cutoffs[i];
  for (int i = 0; i < n_tails; ++i) { p.dims[i] = dims[i]; p.proj[i] = (const char*)proj[i]; p.table[i] = (const char*)tables[i]; }
  return p;
}

extern "C" {

int64_t ea_adaptive_sample_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims) {
  return ea::adaptive_select_plan(M, n_tails, cutoffs, dims, 0, nullptr);
}

int ea_adaptive_sample(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                       int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype, const void* const* proj,
                       const void* const* tables, void* ws, int64_t ws_bytes, int32_t top_k, float top_p, float temperature,
                       uint64_t seed, int64_t* ctr, const int32_t* sid, int64_t* token, float* logp, int32_t* sel_idx,
                       float* sel_val, int32_t* kept, void* stream) {
  if (const int rc = adp_operands_ok(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws)) return rc;
  if (!token || !logp || (uintptr_t)token % 8 || (uintptr_t)logp % 4 ||
      !dec_sampler_ok(top_k, top_p, temperature, ctr, sid, sel_idx, sel_val, kept)) return EA_E_BADARG;
  if (top_k > 64) return EA_E_UNSUPPORTED;
  if (const int rc = adp_select_geometry(M, C, n_tails, cutoffs, dims, 0, ws_bytes)) return rc;
  ea::AdaptivePickP p = adp_pick_fill(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws);
  p.token = token; p.logp = logp;
  ea::AdaptiveJointArgs j = {};
  j.top_k = top_k; j.top_p = top_p; j.temperature = temperature; j.seed_lo = (uint32_t)seed; j.seed_hi = (uint32_t)(seed >> 32);
  j.ctr = ctr; j.sid = sid; j.token = token; j.logp = logp; j.sel_idx = sel_idx; j.sel_val = sel_val; j.kept = kept;
  return ea::adaptive_select(p, j, (hipStream_t)stream);
}

int64_t ea_adaptive_beam_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, int32_t W) {
  return W < 1 ? -1 : ea::adaptive_select_plan(M, n_tails, cutoffs, dims, W, nullptr);
}

int ea_adaptive_beam(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                     int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype, const void* const* proj,
                     const void* const* tables, void* ws, int64_t ws_bytes, int32_t W, int32_t eos, int32_t max_new,
                     float* score, int32_t* t, int32_t* nfin, int32_t* done, int64_t* token, int64_t* parent,
                     int32_t* hist_tok, int32_t* hist_par, float* fin_score, int32_t* fin_len, int32_t* fin_beam,
                     int32_t* cand_idx, float* cand_score, void* stream) {
  if (const int rc = adp_operands_ok(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws)) return rc;
  if (!dec_beam_ok(W, eos, max_new, score, t, nfin, done, token, parent, hist_tok, hist_par, fin_score, fin_len, fin_beam,
                   cand_idx, cand_score, nullptr, nullptr) ||
      (n_tails <= EA_ADAPTIVE_MAX_TAILS && eos >= cutoffs[n_tails])) return EA_E_BADARG;
  if (const int rc = adp_select_geometry(M, C, n_tails, cutoffs, dims, W, ws_bytes)) return rc;
  ea::AdaptivePickP p = adp_pick_fill(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws);
  const int64_t V = cutoffs[n_tails];
  ea::AdaptiveJointArgs j = {};
  j.W = W;
  j.beam = dec_beam_fill(M / W, W, 2 * W < V ? 2 * W : (int)V, eos, max_new, score, t, nfin, done, token, parent, hist_tok,
                         hist_par, fin_score, fin_len, fin_beam, cand_idx, cand_score);
  return ea::adaptive_select(p, j, (hipStream_t)stream);
}

// ---- the constrained beam step from the adaptive head (ABI 36): ea_adaptive_beam's groups, then ea_ceva_sdecode_vocab_beam_c's
// constraints ------------------------------------------------------------------------------------------------------------------
int64_t ea_adaptive_beam_c_ws(int32_t M, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, int32_t W,
                              int32_t prompt_cap, int32_t max_new) {
  const int64_t base = ea_adaptive_beam_ws(M, n_tails, cutoffs, dims, W), more = ea::ceva_beam_bans_ws(M, prompt_cap, max_new);
  return base < 0 || more < 0 ? -1 : base + more;
}

int ea_adaptive_beam_c(int32_t M, int32_t C, int32_t n_tails, const int64_t* cutoffs, const int32_t* dims, const void* x,
                       int32_t x_dtype, int64_t ldx, const void* head, int32_t w_dtype, const void* const* proj,
                       const void* const* tables, void* ws, int64_t ws_bytes, int32_t W, int32_t eos, int32_t max_new,
                       float* score, int32_t* t, int32_t* nfin, int32_t* done, int64_t* token, int64_t* parent,
                       int32_t* hist_tok, int32_t* hist_par, float* fin_score, int32_t* fin_len, int32_t* fin_beam,
                       int32_t* cand_idx, float* cand_score, int32_t min_len, int32_t ngram, const int32_t* ban_tokens,
                       int32_t n_ban_tokens, const int32_t* prompt_tok, int32_t prompt_cap, const int32_t* prompt_len,
                       int32_t* gen, void* stream) {
  if (const int rc = adp_operands_ok(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws)) return rc;
  if (!dec_beam_ok(W, eos, max_new, score, t, nfin, done, token, parent, hist_tok, hist_par, fin_score, fin_len, fin_beam,
                   cand_idx, cand_score, nullptr, nullptr) ||
      (n_tails <= EA_ADAPTIVE_MAX_TAILS && eos >= cutoffs[n_tails])) return EA_E_BADARG;
  ea::BeamBanP c;
  if (const int rc = dec_bans_fill(&c, M / W, W, eos, max_new, n_tails <= EA_ADAPTIVE_MAX_TAILS ? cutoffs[n_tails] : -1, min_len,
                                   ngram, ban_tokens, n_ban_tokens, prompt_tok, prompt_cap, prompt_len, t, done, hist_tok,
                                   hist_par, gen)) return rc;
  const int64_t more = ea::ceva_beam_bans_ws(M, prompt_cap, max_new);
  if (more < 0) return EA_E_UNSUPPORTED;
  if (const int rc = adp_select_geometry(M, C, n_tails, cutoffs, dims, W, ws_bytes - more)) return rc;
  const int64_t base = ea::adaptive_select_plan(M, n_tails, cutoffs, dims, W, nullptr);
  ea::AdaptivePickP p = adp_pick_fill(M, C, n_tails, cutoffs, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws);
  const int64_t V = cutoffs[n_tails];
  ea::AdaptiveJointArgs j = {};
  j.W = W;
  j.beam = dec_beam_fill(M / W, W, 2 * W < V ? 2 * W : (int)V, eos, max_new, score, t, nfin, done, token, parent, hist_tok,
                         hist_par, fin_score, fin_len, fin_beam, cand_idx, cand_score);
  ea::ceva_beam_bans_carve((char*)ws + base, M, &c);
  return ea::adaptive_select(p, j, (hipStream_t)stream, &c);
}

}  // extern "C"
