// ea_adaptive_pick.hip -- the greedy token and its log-probability from a held adaptive softmax (ABI 34), for the <= 64 rows of
// a decoding step, without a [rows, V] tensor
//
//   cutoffs c0 < c1 < .. < c_n = V; a[v], v < c0 + n: the head's logits; b_i[u]: tail i's, on h_i = round_w(x proj_i^T):
//     word  v < c0:    s(v)       = a[v] - lse_h                                  lse_h over ALL c0 + n head columns
//     token c_i + u:   s(c_i + u) = (a[c0 + i] - lse_h) + (b_i[u] - lse_i)        lse_i over tail i
//   token[m] = the vocabulary index of the largest s; logp[m] = s(targets[m]), or s(token[m]) without targets.
//
// Launches: the head's words and the head's classes on the few-row table pass (ceva_rows_kernel on DecLseP: its bits), the
// projections on ea_ceva_sdecode_linear's kernel (its bits), one pass per tail, the pick.
// adaptive_tail_kernel, the tail pass for d_i <= AP_MAX_K: the few-row kernel splits K over its 8 waves -- at d_i = 64 six of
// them idle and a workgroup fetches 2 KB.  Here a workgroup owns AP_SPAN = 16 AP_TPW AP_WAVES columns; a wave owns AP_TPW
// whole 16-column MFMA tiles, the table rows as B operands by one 16-byte global load per lane and k-step, h_i as the A
// operand from an LDS copy the workgroup's waves share (rows >= M are zeros).  A logit is ONE accumulator chained over the
// K / 32 k-steps in ascending order: no cross-wave sum -- this kernel's own order of summation, not ea_ceva_sdecode_linear's.
// The epilogue keeps the vocab epilogue's partial format, per row and WAVE (its 16 AP_TPW columns): a lane folds its own
// column of the wave's tiles in tile order, the 16 lanes of a row reduce once -- the candidate under voc_beats, then
// s = sum exp(logit - its value), a lane's terms in tile order and the xor butterfly (8, 4, 2, 1) over the lanes -- and the
// target's logit is kept (target base c_i).  The workgroup merges its waves' partials in wave order through LDS (ap_merge:
// the better candidate, the sums rescaled to its value; a partial whose maximum is -inf is skipped, never multiplied): one
// (candidate, sum) partial per row and span.  A column >= V_i is
// read from row V_i - 1 (a clamped address) and neither picked nor summed.
// adaptive_pick_kernel, one workgroup per row: per band the candidates' best (the pick's two passes: voc_beats, then the
// sums against the top; the head's sum takes the class tile's partial last), lse by ABI 28's cases, then the n + 1 joint
// scores under voc_beats on (s, vocabulary index).
// ABI 35, the k best joint scores of a row for the sampled pick and the beam step: the same band passes with their fp32
// logits kept (adaptive_tail_kernel on AdaptiveTailKeepP also writes one candidate per 16-column tile), adaptive_select_kernel
// per (row, band) and adaptive_joint_kernel per row, further down.
// Ordinary vector stores only; no atomics on memory (integer LDS atomics in the selection's histograms); no workgroup waits for
// another; launches only.
#include <limits.h>
#include <math.h>
#include <type_traits>
#include "ea_common.h"
#include "ea_ceva_decode_linear.h"
#include "ea_ceva_decode_vocab.h"
#include "ea_adaptive_pick.h"

namespace ea {

namespace {

#include "ea_ceva_decode_rows.h"
#include "ea_voc_select.h"
#include "ea_voc_ban.h"

constexpr int AP_THREADS = AP_WAVES * 64;
constexpr int AP_LDH = AP_MAX_K + 8;                   // elements of a row of h in LDS: 16 bytes of padding
constexpr int APK_THREADS = 256;
constexpr int NB_MAX = AS_MAX_TAILS + 1;

struct AdaptiveTailP {
  const char* h;              // [M, ldh] 16-bit
  const char* w;              // [V, K] 16-bit
  VocPick* cand;              // [M, NP]
  float* sum;                 // [M, NP]
  float* tlogit;              // [M]
  const int64_t* targets;     // [M] or null
  int64_t ldh, target_base;
  int M, K, V, NP;
};

// (a, sa) takes b in: the better candidate, and the sum of both sides' exponentials against its value
EA_DEV void ap_merge(VocPick& a, float& sa, const VocPick b, const float sb) {
  const VocPick c = voc_beats(b, a) ? b : a;
  float s = 0.f;
  if (c.v - c.v == 0.f) {                               // (finite: every value below it is a number or -inf)
    if (a.v != -INFINITY) s = sa * expf(a.v - c.v);
    if (b.v != -INFINITY) s += sb * expf(b.v - c.v);
  }
  a = c;
  sa = s;
}

// the tail pass that keeps its logits (ABI 35): AdaptiveTailP's, the fp32 logits and one candidate per 16-column tile -- what
// voc_select reads of a plain table's pass.  A block of its own: AdaptiveTailP's instance stays what it is.
struct AdaptiveTailKeepP : AdaptiveTailP {
  float* logits;              // [M, V]
  VocPick* tcand;             // [M, NT]
  int NT;                     // ceil(V / 16)
};

template <typename E, int RT, typename P>
__global__ __launch_bounds__(AP_THREADS) void adaptive_tail_kernel(const P p) {
  constexpr bool KEEP = std::is_same<P, AdaptiveTailKeepP>::value;
  static_assert(KEEP || std::is_same<P, AdaptiveTailP>::value, "one of the two blocks");
  __shared__ __attribute__((aligned(16))) uint16_t hs[RT * 16 * AP_LDH];
  __shared__ VocPick wbest[AP_WAVES][RT * 16];
  __shared__ float wsum[AP_WAVES][RT * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int KS = p.K >> 5;
  {                                                     // h -> LDS, 16-byte pieces; a row >= M is zeros
    const int pieces = p.K >> 3;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int e = threadIdx.x; e < RT * 16 * pieces; e += AP_THREADS) {
      const int row = e / pieces, c = e - row * pieces;
      u32x4 v = zero;
      if (row < p.M) v = *reinterpret_cast<const u32x4*>(p.h + ((int64_t)row * p.ldh + 8 * c) * 2);
      *reinterpret_cast<u32x4*>(&hs[row * AP_LDH + 8 * c]) = v;
    }
  }
  __syncthreads();
  const int tile0 = (blockIdx.x * AP_WAVES + wave) * AP_TPW;
  const char* wrow[AP_TPW];
  int live[AP_TPW];                                     // columns of the tile below V: 0 for a tile past the table
#pragma unroll
  for (int t = 0; t < AP_TPW; ++t) {
    const int n0 = (tile0 + t) * VOC_TILE;
    live[t] = max(0, min(VOC_TILE, p.V - n0));
    wrow[t] = p.w + ((int64_t)min(n0 + li, p.V - 1) * p.K + 8 * g) * 2;   // (a column past V: row V - 1 again)
  }
  f32x4 acc[AP_TPW][RT];
#pragma unroll
  for (int t = 0; t < AP_TPW; ++t)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[t][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int s = 0; s < KS; ++s) {
    u32x4 wf[AP_TPW];
#pragma unroll
    for (int t = 0; t < AP_TPW; ++t) wf[t] = ldg16(wrow[t] + (int64_t)s * 64);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(&hs[(rt * 16 + li) * AP_LDH + s * 32 + 8 * g]);
#pragma unroll
      for (int t = 0; t < AP_TPW; ++t) acc[t][rt] = E::mma(as_x8<E>(a), as_x8<E>(wf[t]), acc[t][rt]);
    }
  }
  // D[row = 4 g + r][col = li] of every row tile.  A lane first folds its own column of the wave's AP_TPW tiles, in tile order
  // and without an exchange; then the 16 lanes of a row group reduce ONCE: the candidate under voc_beats, and
  // s = sum exp(logit - its value) over the wave's live columns (a lane's terms in tile order, then the xor butterfly)
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    if (rt * 16 >= p.M) break;                          // (uniform: a row tile of zeros)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = rt * 16 + 4 * g + r;
      int tcol = -1;                                    // the target's column of this table, or none
      if (p.targets && m < p.M) {
        const int64_t t = p.targets[m] - p.target_base;
        if (t >= 0 && t < (int64_t)p.V) tcol = (int)t;
      }
      VocPick c = voc_none();
#pragma unroll
      for (int t = 0; t < AP_TPW; ++t) {
        const float v = acc[t][rt][r];
        const int n = (tile0 + t) * VOC_TILE + li;
        const bool col = li < live[t];
        if (col && n == tcol) p.tlogit[m] = v;
        const VocPick mine = col ? VocPick{v, n} : voc_none();
        if constexpr (KEEP) {                           // the logit, and the tile's candidate: the row group's 16 lanes, before the fold
          if (col && m < p.M) p.logits[(int64_t)m * p.V + n] = v;
          VocPick tc = mine;
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) {
            const VocPick other = voc_exchange(tc, o);
            if (voc_beats(other, tc)) tc = other;
          }
          if (li == 0 && m < p.M && tile0 + t < p.NT) p.tcand[(int64_t)m * p.NT + tile0 + t] = tc;
        }
        if (voc_beats(mine, c)) c = mine;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const VocPick other = voc_exchange(c, o);
        if (voc_beats(other, c)) c = other;
      }
      float s = 0.f;                                    // (c.v NaN or infinite: whatever comes out; not read then)
#pragma unroll
      for (int t = 0; t < AP_TPW; ++t) s += li < live[t] ? expf(acc[t][rt][r] - c.v) : 0.f;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (li == 0) {
        wbest[wave][m] = c;
        wsum[wave][m] = s;
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < p.M) {                         // (M <= 16 RT) the waves' partials of row m, in wave order
    const int m = threadIdx.x;
    VocPick run = wbest[0][m];
    float rs = wsum[0][m];
#pragma unroll
    for (int w = 1; w < AP_WAVES; ++w) ap_merge(run, rs, wbest[w][m], wsum[w][m]);
    p.cand[(int64_t)m * p.NP + blockIdx.x] = run;
    p.sum[(int64_t)m * p.NP + blockIdx.x] = rs;
  }
}

// targets - base -> out: what the few-row table pass compares its columns with
__global__ __launch_bounds__(64) void adaptive_shift_kernel(const int64_t* targets, int64_t base, int64_t* out, int M) {
  const int m = threadIdx.x;
  if (m < M) out[m] = targets[m] - base;
}

struct AdaptivePickFoldP {
  const VocPick* cand[NB_MAX];   // [M][parts[b]]
  const float* sum[NB_MAX];
  const VocPick* cls_cand;       // [M]
  const float* cls_sum;          // [M]
  const float* cls;              // [M][n]
  VocPick* best[NB_MAX];         // [M]
  float* lse[NB_MAX];            // [M]
  const float* tlogit[NB_MAX];   // [M]
  const int64_t* targets;        // [M] or null
  int64_t* token;                // [M]
  float* logp;                   // [M]
  int64_t cut[NB_MAX];
  int parts[NB_MAX];
  int n;
};

// top NaN: NaN; +inf: +inf; -inf (every logit is -inf): -inf
EA_DEV float ap_lse_of(float top, float total) { return top - top == 0.f ? top + logf(total) : top; }

// what ap_band_fold works in
struct ApFold {
  VocPick wbest[APK_THREADS / 64];
  float wpart[APK_THREADS / 64];
  float top_of_band;
};

// One band's fold, the pick's two passes over the band's NP partials (row, srow): the best candidate under voc_beats, then
// S = sum_j s_j expf(m_j - top) -> thread 0's (best, lse).  cls (the head's band alone, else null): the class tile's
// (candidate, sum) -- the head's top is the larger of the two maxima, and its S takes that partial last.  The first
// APK_THREADS threads of the workgroup fold (thread j its partials j, j + APK_THREADS, .. in order, six xor exchanges per
// wave, the waves in wave order), whatever the workgroup's size: the bits do not depend on it (WIDE: a workgroup of more
// threads than those; they idle through it).  Every thread calls it; it ends behind a barrier.
template <bool WIDE>
EA_DEV void ap_band_fold(const VocPick* row, const float* srow, int NP, const VocPick* cls, const float* cls_sum, ApFold& sh,
                         VocPick& best, float& lse) {
  const bool on = !WIDE || threadIdx.x < APK_THREADS;
  // pass 1: the band's best candidate
  VocPick c = voc_none();
  if (on) {
    for (int j = threadIdx.x; j < NP; j += APK_THREADS) {
      const VocPick other = row[j];
      if (voc_beats(other, c)) c = other;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const VocPick other = voc_exchange(c, o);
    if (voc_beats(other, c)) c = other;
  }
  if (on && (threadIdx.x & 63) == 0) sh.wbest[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < APK_THREADS / 64; ++w)
      if (voc_beats(sh.wbest[w], c)) c = sh.wbest[w];
    float top = c.v;
    if (cls && voc_beats(VocPick{cls->v, INT_MAX}, VocPick{top, 0})) top = cls->v;   // the head's top
    sh.top_of_band = top;
  }
  best = c;
  __syncthreads();
  const float top = sh.top_of_band;
  // pass 2: the partial sums against the top
  float s = 0.f;
  if (on && top - top == 0.f) {
    for (int j = threadIdx.x; j < NP; j += APK_THREADS) {
      const float mt = row[j].v;
      if (mt != -INFINITY) s += srow[j] * expf(mt - top);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (on && (threadIdx.x & 63) == 0) sh.wpart[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = sh.wpart[0];
#pragma unroll
    for (int w = 1; w < APK_THREADS / 64; ++w) total += sh.wpart[w];
    if (cls && top - top == 0.f) {                      // the class tile's partial, last
      const float mc = cls->v;
      if (mc != -INFINITY) total += *cls_sum * expf(mc - top);
    }
    lse = ap_lse_of(top, total);
  }
  __syncthreads();                                      // (sh is the next band's)
}

__global__ __launch_bounds__(APK_THREADS) void adaptive_pick_kernel(const AdaptivePickFoldP p) {
  __shared__ ApFold sh;
  const int m = blockIdx.x;
  VocPick best[NB_MAX];                                 // (thread 0's are the bands')
  float lse[NB_MAX];
#pragma unroll
  for (int b = 0; b < NB_MAX; ++b) {
    if (b > p.n) break;                                 // (uniform)
    const int NP = p.parts[b];
    ap_band_fold<false>(p.cand[b] + (int64_t)m * NP, p.sum[b] + (int64_t)m * NP, NP, b == 0 ? p.cls_cand + m : nullptr,
                        p.cls_sum + m, sh, best[b], lse[b]);
    if (threadIdx.x == 0) {
      p.best[b][m] = best[b];
      p.lse[b][m] = lse[b];
    }
  }
  if (threadIdx.x != 0) return;
  const int64_t V = p.cut[p.n];
  const float* a = p.cls + (int64_t)m * p.n;            // a[c0 + i]
  VocPick win = VocPick{best[0].v - lse[0], best[0].i};
#pragma unroll
  for (int i = 0; i < AS_MAX_TAILS; ++i) {
    if (i >= p.n) break;
    const float sc = (a[i] - lse[0]) + (best[i + 1].v - lse[i + 1]);
    const VocPick c = VocPick{sc, (int32_t)(p.cut[i] + best[i + 1].i)};
    if (voc_beats(c, win)) win = c;
  }
  const int64_t tok = min(max((int64_t)win.i, (int64_t)0), V - 1);   // (a token of the vocabulary, come what may)
  float lp = win.v;
  if (p.targets) {
    const int64_t t = p.targets[m];
    lp = NAN;
    if (t >= 0 && t < p.cut[0]) lp = p.tlogit[0][m] - lse[0];
#pragma unroll
    for (int i = 0; i < AS_MAX_TAILS; ++i)
      if (i < p.n && t >= p.cut[i] && t < p.cut[i + 1]) lp = (a[i] - lse[0]) + (p.tlogit[i + 1][m] - lse[i + 1]);
  }
  p.token[m] = tok;
  p.logp[m] = lp;
}

template <typename E, typename P>
int tail_launch(const P& p, hipStream_t st) {
  const dim3 grid((unsigned)p.NP), block(AP_THREADS);
  if (p.M <= 16) hipLaunchKernelGGL((adaptive_tail_kernel<E, 1, P>), grid, block, 0, st, p);
  else if (p.M <= 32) hipLaunchKernelGGL((adaptive_tail_kernel<E, 2, P>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((adaptive_tail_kernel<E, 4, P>), grid, block, 0, st, p);
  return (int)hipGetLastError();
}

// ---- the k best joint log-probabilities of a row (ABI 35) -----------------------------------------------------------------
// Behind band passes that have kept their fp32 logits and one candidate per 16-column tile: adaptive_select_kernel, grid
// (row, band), a band's lse and its min(k, V_b) best RAW logits in order; adaptive_joint_kernel, one workgroup per row, the
// joint scores of those lists as keys, the min(k, V) best in order, then the draw or the beam step's candidates.  The rule is
// spelled out in include/ea_hip.h.
static_assert(SMP_THREADS >= APK_THREADS, "the select kernel's first APK_THREADS threads fold a band as the pick kernel does");
static_assert(NB_MAX * ASEL_MAX_K <= SMP_UNROLL * SMP_THREADS, "voc_threshold and voc_compact walk a row's lists in one iteration");

struct AdaptiveSelectP {
  const VocPick* cand[NB_MAX];   // [M][parts[b]] the passes' partials: what the pick folds
  const float* sum[NB_MAX];
  const VocPick* tile[NB_MAX];   // [M][ceil(vb[b] / 16)] one candidate per 16-column tile
  const float* logits[NB_MAX];   // [M][vb[b]]
  const VocPick* cls_cand;       // [M]
  const float* cls_sum;          // [M]
  float* lse[NB_MAX];            // [M]
  int32_t* list_idx;             // [M][n + 1][ASEL_MAX_K] columns IN the band
  float* list_val;               // [M][n + 1][ASEL_MAX_K] their stored logits
  const int32_t* done;           // [S], rows of a done sentence are skipped; or null
  int parts[NB_MAX], vb[NB_MAX];
  int n, k, W;
};

// the constrained beam step's list (ABI 36) and where a band's columns lie among the tokens
struct AdaptiveBanP {
  BanListP list;
  int64_t base[NB_MAX];          // the token of band b's column 0: 0, then cut[b - 1]
};

// BANS (ABI 36): the listed tokens that fall in band b are applied to the band's stored logits and tile candidates, behind the
// fold (the band's lse is the unconstrained one) and ahead of the selection (ea_voc_ban.h); class columns are no band's.  The
// body of both kernels, inlined: the unconstrained one -- the sampler's too -- keeps its instructions.
template <bool BANS>
EA_DEV void adaptive_select_body(const AdaptiveSelectP& p, const AdaptiveBanP& c, VocSelect& sh, ApFold& fold) {
  const int m = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63;
  if (p.done && p.done[m / p.W]) return;                  // (uniform)
  const int NP = p.parts[b], Vb = p.vb[b], NT = (Vb - 1) / VOC_TILE + 1;
  VocPick best;
  float lse = 0.f;
  ap_band_fold<true>(p.cand[b] + (int64_t)m * NP, p.sum[b] + (int64_t)m * NP, NP, b == 0 ? p.cls_cand + m : nullptr,
                     p.cls_sum + m, fold, best, lse);
  if (threadIdx.x == 0) p.lse[b][m] = lse;
  const float* lrow = p.logits[b] + (int64_t)m * Vb;
  if constexpr (BANS) {                                   // (this workgroup alone reads and writes the band's row from here on)
    const int nb = min(max(c.list.nban[m], 0), c.list.cap);
    voc_apply_bans(const_cast<float*>(lrow), const_cast<VocPick*>(p.tile[b]) + (int64_t)m * NT, Vb,
                   c.list.ban + (int64_t)m * c.list.cap, nb, c.base[b]);
  }
  const int kk = voc_select(p.tile[b] + (int64_t)m * NT, lrow, Vb, NT, p.k, sh);
  if (threadIdx.x >= 64 || lane >= kk) return;
  const int32_t idx = min(max(voc_key_index(sh.sorted[lane]), 0), Vb - 1);   // (a column of the band, come what may)
  const int64_t at = ((int64_t)m * (p.n + 1) + b) * ASEL_MAX_K + lane;
  p.list_idx[at] = idx;
  p.list_val[at] = lrow[idx];                              // (the stored logit's own bits: the key has folded -0 and NaNs)
}

__global__ __launch_bounds__(SMP_THREADS) void adaptive_select_kernel(const AdaptiveSelectP p) {
  __shared__ VocSelect sh;
  __shared__ ApFold fold;
  adaptive_select_body<false>(p, AdaptiveBanP{}, sh, fold);
}

__global__ __launch_bounds__(SMP_THREADS) void adaptive_select_c_kernel(const AdaptiveSelectP p, const AdaptiveBanP c) {
  __shared__ VocSelect sh;
  __shared__ ApFold fold;
  adaptive_select_body<true>(p, c, sh, fold);
}

struct AdaptiveJointP {
  const float* logits[NB_MAX];   // [M][vb[b]]
  const float* lse[NB_MAX];      // [M]
  const float* cls;              // [M][n]
  const int32_t* list_idx;       // [M][n + 1][ASEL_MAX_K]
  const float* list_val;
  int64_t cut[NB_MAX];
  int vb[NB_MAX];
  int n, k;
  AdaptiveJointArgs a;
};

// the joint score of a raw logit of band b: these operations, this order
EA_DEV float asel_score(const AdaptiveJointP& p, int m, int b, float raw) {
  const float lse_h = p.lse[0][m];
  if (b == 0) return raw - lse_h;
  return (p.cls[(int64_t)m * p.n + b - 1] - lse_h) + (raw - p.lse[b][m]);
}

// the band of token v < V and its column there
EA_DEV int asel_band(const AdaptiveJointP& p, int32_t v, int32_t& col) {
  int b = 0;
#pragma unroll
  for (int i = 0; i < AS_MAX_TAILS; ++i)
    if (i < p.n && (int64_t)v >= p.cut[i]) b = i + 1;
  col = b ? (int32_t)(v - p.cut[b - 1]) : v;
  return b;
}

__global__ __launch_bounds__(SMP_THREADS) void adaptive_joint_kernel(const AdaptiveJointP p) {
  __shared__ uint64_t keys[NB_MAX * ASEL_MAX_K];
  __shared__ uint64_t sel[ASEL_MAX_K];
  __shared__ uint64_t sorted[ASEL_MAX_K];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t pass[3];
  __shared__ uint32_t count;
  const int m = blockIdx.x, lane = threadIdx.x & 63;
  const int W = p.a.W;
  const int32_t V = (int32_t)p.cut[p.n];
  float score = 0.f;
  if (W > 0) {                                            // the beam step
    const DecBeamP& bm = p.a.beam;
    const int s = m / W;
    if (bm.done[s]) return;                               // (uniform)
    score = bm.score[m];
    if (bm.t[s] + 1 >= bm.max_new) {                      // (uniform) the forced step: eos alone
      if (threadIdx.x == 0) {
        int32_t col;
        const int b = asel_band(p, bm.eos, col);
        const float raw = p.logits[b][(int64_t)m * p.vb[b] + col];
        bm.cand_idx[(int64_t)m * (2 * W)] = bm.eos;
        bm.cand_score[(int64_t)m * (2 * W)] = score + asel_score(p, m, b, raw);
      }
      return;
    }
  }
  // the bands' lists as keys: (joint score, vocabulary index)
  int off[NB_MAX + 1];
  off[0] = 0;
#pragma unroll
  for (int b = 0; b < NB_MAX; ++b) off[b + 1] = off[b] + (b <= p.n ? min(p.k, p.vb[b]) : 0);
  const int nc = off[NB_MAX], kk = min(p.k, nc);          // (nc >= min(k, V): a band shorter than k is there whole)
  if (threadIdx.x == 0) count = 0u;
  for (int e = threadIdx.x; e < nc; e += SMP_THREADS) {
    int b = 0;
#pragma unroll
    for (int i = 1; i < NB_MAX; ++i)
      if (i <= p.n && e >= off[i]) b = i;
    const int64_t at = ((int64_t)m * (p.n + 1) + b) * ASEL_MAX_K + (e - off[b]);
    const int32_t v = (int32_t)((b ? p.cut[b - 1] : 0) + p.list_idx[at]);
    keys[e] = voc_key(asel_score(p, m, b, p.list_val[at]), v);
  }
  __syncthreads();
  auto key_of = [&](int j) { return keys[j]; };
  const uint64_t t1 = kk < nc ? voc_threshold(key_of, nc, kk, hist, pass) : 0ull;
  __syncthreads();
  voc_compact(key_of, nc, t1, sel, kk, &count);
  __syncthreads();
  voc_rank_sort(sel, sorted, kk);
  if (threadIdx.x >= 64) return;
  // one wave, entry j of the selection in lane j
  const bool live = lane < kk;
  const int32_t tok = live ? min(max(voc_key_index(sorted[lane]), 0), V - 1) : 0;   // (a token of the vocabulary, come what may)
  int32_t col;
  const int b = asel_band(p, tok, col);
  // (the score again, from the stored logit's own bits: the key has folded -0 and NaNs)
  const float sj = live ? asel_score(p, m, b, p.logits[b][(int64_t)m * p.vb[b] + col]) : -INFINITY;
  if (W > 0) {
    if (live) {
      p.a.beam.cand_idx[(int64_t)m * (2 * W) + lane] = tok;
      p.a.beam.cand_score[(int64_t)m * (2 * W) + lane] = score + sj;
    }
    return;
  }
  if (live && p.a.sel_idx) p.a.sel_idx[(int64_t)m * p.k + lane] = tok;
  if (live && p.a.sel_val) p.a.sel_val[(int64_t)m * p.k + lane] = sj;
  const int64_t n = p.a.ctr[m];
  int32_t kept;
  const int drawn = voc_draw(sj, live, kk, p.a.top_p, p.a.temperature, p.a.seed_lo, p.a.seed_hi, n, p.a.sid[m], kept);
  const int32_t token = __shfl(tok, drawn);
  const float lp = __shfl(sj, drawn);
  if (lane == 0) {
    p.a.token[m] = (int64_t)token;
    p.a.logp[m] = lp;
    if (p.a.kept) p.a.kept[m] = kept;
    p.a.ctr[m] = n + 1;                                   // (this workgroup alone reads and writes ctr[m])
  }
}

int64_t r16(int64_t n) { return (n + 15) / 16 * 16; }

}  // namespace

int64_t adaptive_pick_plan(int M, int n, const int64_t* cut, const int32_t* dims, AdaptivePickPlan* plan) {
  if (M < 1 || M > AP_MAX_ROWS || n < 1 || n > AS_MAX_TAILS || !cut || !dims || cut[0] < 1) return -1;
  for (int i = 0; i < n; ++i)
    if (cut[i + 1] <= cut[i] || dims[i] < 1) return -1;
  if (cut[n] > INT_MAX - 2 * AP_SPAN) return -1;
  AdaptivePickPlan pl = {};
  int64_t at = 0, D = 0;
  auto take = [&](int64_t bytes) { const int64_t here = at; at += r16(bytes); return here; };
  for (int i = 0; i < n; ++i) D += dims[i];
  if (D > INT_MAX / 2) return -1;
  pl.D = (int32_t)D;
  pl.cls = take(4 * (int64_t)M * n);
  pl.h = take(2 * (int64_t)M * D);
  for (int b = 0; b <= n; ++b) {
    pl.best[b] = take(8 * (int64_t)M);
    pl.lse[b] = take(4 * (int64_t)M);
    pl.tlogit[b] = take(4 * (int64_t)M);
  }
  for (int i = 0; i < n; ++i) pl.shifted[i] = dims[i] > AP_MAX_K ? take(8 * (int64_t)M) : -1;
  pl.cls_cand = take(8 * (int64_t)M);
  pl.cls_sum = take(4 * (int64_t)M);
  for (int b = 0; b <= n; ++b) {
    const int64_t Vb = b ? cut[b] - cut[b - 1] : cut[0];
    const bool split = b && dims[b - 1] <= AP_MAX_K;
    pl.parts[b] = (int32_t)(split ? (Vb - 1) / AP_SPAN + 1 : (Vb - 1) / VOC_TILE + 1);
    pl.cand[b] = take(8 * (int64_t)M * pl.parts[b]);
    pl.sum[b] = take(4 * (int64_t)M * pl.parts[b]);
  }
  pl.total = at;
  if (plan) *plan = pl;
  return pl.total;
}

// launches 1 .. 4 of the pick: the band passes on the plan `pl`.  keep (ABI 35, or null): every band's fp32 logits are stored
// too, and the column-split tails write one candidate per 16-column tile -- the same kernels' sums, the same partials.
static int adaptive_band_passes(const AdaptivePickP& a, const AdaptivePickPlan& pl, const AdaptiveSelectPlan* keep, hipStream_t st) {
  auto vp = [&](int64_t off) { return reinterpret_cast<VocPick*>(a.ws + off); };
  auto fp = [&](int64_t off) { return reinterpret_cast<float*>(a.ws + off); };
  const int n = a.n, D = pl.D;
  const int64_t c0 = a.cut[0];

  // 1. the head's words: candidates, tile sums and the targets' logits of head[0 .. c0)
  DecLseP hw = {};
  hw.x = a.x; hw.w = a.head; hw.ws = vp(pl.cand[0]); hw.lws = fp(pl.sum[0]); hw.tlogit = fp(pl.tlogit[0]);
  hw.targets = a.targets; hw.token = a.token; hw.lse = fp(pl.lse[0]); hw.logp = a.logp;
  hw.ldx = a.ldx; hw.M = a.M; hw.K = a.C; hw.V = (int)c0; hw.dtype = a.dtype; hw.x_f32 = a.x_f32;
  DecLseP hc = hw;
  if (keep) { hw.logits = a.ws + keep->logits[0]; hw.ldl = c0; hw.l_f32 = 1; }
  if (const int rc = ceva_sdecode_vocab_table_pass(hw, st)) return rc;
  // 2. the head's classes: the n rows behind them, the fp32 logits stored
  hc.w = a.head + c0 * a.C * 2; hc.logits = a.ws + pl.cls; hc.ldl = n; hc.l_f32 = 1; hc.V = n;
  hc.ws = vp(pl.cls_cand); hc.lws = fp(pl.cls_sum); hc.targets = nullptr;
  if (const int rc = ceva_sdecode_vocab_table_pass(hc, st)) return rc;
  // 3. the projections: h [M, D], h_i its columns off_i .. off_i + d_i; one launch where the projections lie in a row
  bool joined = true;
  for (int i = 0; i + 1 < n; ++i) joined = joined && a.proj[i + 1] == a.proj[i] + (int64_t)a.dims[i] * a.C * 2;
  DecLinP lin = {};
  lin.x = a.x; lin.ldx = a.ldx; lin.ldy = D; lin.M = a.M; lin.K = a.C; lin.dtype = a.dtype; lin.x_f32 = a.x_f32;
  int off = 0;
  for (int i = 0; i < n; off += a.dims[i], ++i) {
    lin.w = a.proj[i]; lin.y = a.ws + pl.h + (int64_t)off * 2; lin.N = joined ? D : a.dims[i];
    if (const int rc = ceva_sdecode_linear(lin, st)) return rc;
    if (joined) break;
  }
  // 4. the tails
  off = 0;
  for (int i = 0; i < n; off += a.dims[i], ++i) {
    const int Vi = (int)(a.cut[i + 1] - a.cut[i]);
    const char* hi = a.ws + pl.h + (int64_t)off * 2;
    if (a.dims[i] <= AP_MAX_K) {
      AdaptiveTailP t = {};
      t.h = hi; t.w = a.table[i]; t.cand = vp(pl.cand[i + 1]); t.sum = fp(pl.sum[i + 1]); t.tlogit = fp(pl.tlogit[i + 1]);
      t.targets = a.targets; t.ldh = D; t.target_base = a.cut[i]; t.M = a.M; t.K = a.dims[i]; t.V = Vi; t.NP = pl.parts[i + 1];
      if (keep) {
        AdaptiveTailKeepP tk = {};
        static_cast<AdaptiveTailP&>(tk) = t;
        tk.logits = fp(keep->logits[i + 1]); tk.tcand = vp(keep->tcand[i]); tk.NT = (Vi - 1) / VOC_TILE + 1;
        if (const int rc = a.dtype == EA_BF16 ? tail_launch<BF16>(tk, st) : tail_launch<F16>(tk, st)) return rc;
        continue;
      }
      if (const int rc = a.dtype == EA_BF16 ? tail_launch<BF16>(t, st) : tail_launch<F16>(t, st)) return rc;
    } else {
      int64_t* shifted = reinterpret_cast<int64_t*>(a.ws + pl.shifted[i]);
      if (a.targets) {
        hipLaunchKernelGGL(adaptive_shift_kernel, dim3(1), dim3(64), 0, st, a.targets, a.cut[i], shifted, a.M);
        if (const int rc = (int)hipGetLastError()) return rc;
      }
      DecLseP t = {};
      t.x = hi; t.w = a.table[i]; t.ws = vp(pl.cand[i + 1]); t.lws = fp(pl.sum[i + 1]); t.tlogit = fp(pl.tlogit[i + 1]);
      t.targets = a.targets ? shifted : nullptr; t.token = a.token; t.lse = fp(pl.lse[i + 1]); t.logp = a.logp;
      t.ldx = D; t.M = a.M; t.K = a.dims[i]; t.V = Vi; t.dtype = a.dtype;
      if (keep) { t.logits = a.ws + keep->logits[i + 1]; t.ldl = Vi; t.l_f32 = 1; }
      if (const int rc = ceva_sdecode_vocab_table_pass(t, st)) return rc;
    }
  }
  return 0;
}

int adaptive_pick(const AdaptivePickP& a, hipStream_t st) {
  AdaptivePickPlan pl;
  if (adaptive_pick_plan(a.M, a.n, a.cut, a.dims, &pl) < 0) return EA_E_UNSUPPORTED;
  if (a.dtype != EA_BF16 && a.dtype != EA_F16) return EA_E_BADARG;
  auto vp = [&](int64_t off) { return reinterpret_cast<VocPick*>(a.ws + off); };
  auto fp = [&](int64_t off) { return reinterpret_cast<float*>(a.ws + off); };
  const int n = a.n;
  if (const int rc = adaptive_band_passes(a, pl, nullptr, st)) return rc;
  // 5. the pick
  AdaptivePickFoldP f = {};
  for (int b = 0; b <= n; ++b) {
    f.cand[b] = vp(pl.cand[b]); f.sum[b] = fp(pl.sum[b]); f.best[b] = vp(pl.best[b]); f.lse[b] = fp(pl.lse[b]);
    f.tlogit[b] = fp(pl.tlogit[b]); f.parts[b] = pl.parts[b]; f.cut[b] = a.cut[b];
  }
  f.cls_cand = vp(pl.cls_cand); f.cls_sum = fp(pl.cls_sum); f.cls = fp(pl.cls);
  f.targets = a.targets; f.token = a.token; f.logp = a.logp; f.n = n;
  hipLaunchKernelGGL(adaptive_pick_kernel, dim3((unsigned)a.M), dim3(APK_THREADS), 0, st, f);
  return (int)hipGetLastError();
}

// ---- the sampled pick and the beam step (ABI 35) ----
int64_t adaptive_select_plan(int M, int n, const int64_t* cut, const int32_t* dims, int W, AdaptiveSelectPlan* plan) {
  AdaptiveSelectPlan sp = {};
  int64_t at = adaptive_pick_plan(M, n, cut, dims, &sp.pick);
  if (at < 0 || W < 0 || W > VOC_SAMPLE_MAX_K / 2 || (W && M % W)) return -1;
  auto take = [&](int64_t bytes) { const int64_t here = at; at += r16(bytes); return here; };
  for (int b = 0; b <= n; ++b) sp.logits[b] = take(4 * (int64_t)M * (b ? cut[b] - cut[b - 1] : cut[0]));
  for (int i = 0; i < n; ++i)
    sp.tcand[i] = dims[i] <= AP_MAX_K ? take(8 * (int64_t)M * ((cut[i + 1] - cut[i] - 1) / VOC_TILE + 1)) : -1;
  sp.list_idx = take(4 * (int64_t)M * (n + 1) * ASEL_MAX_K);
  sp.list_val = take(4 * (int64_t)M * (n + 1) * ASEL_MAX_K);
  sp.cand_idx = W ? take(4 * (int64_t)M * 2 * W) : -1;
  sp.cand_score = W ? take(4 * (int64_t)M * 2 * W) : -1;
  sp.total = at;
  if (plan) *plan = sp;
  return sp.total;
}

int adaptive_select(const AdaptivePickP& a0, const AdaptiveJointArgs& j, hipStream_t st, const BeamBanP* bans) {
  if (bans && !j.W) return EA_E_BADARG;
  AdaptiveSelectPlan sp;
  if (adaptive_select_plan(a0.M, a0.n, a0.cut, a0.dims, j.W, &sp) < 0) return EA_E_UNSUPPORTED;
  if (a0.dtype != EA_BF16 && a0.dtype != EA_F16) return EA_E_BADARG;
  const AdaptivePickPlan& pl = sp.pick;
  AdaptivePickP a = a0;
  auto vp = [&](int64_t off) { return reinterpret_cast<VocPick*>(a.ws + off); };
  auto fp = [&](int64_t off) { return reinterpret_cast<float*>(a.ws + off); };
  const int n = a.n, k = j.W ? 2 * j.W : j.top_k;
  if (k < 1 || k > ASEL_MAX_K) return EA_E_UNSUPPORTED;
  a.targets = nullptr;
  if (!a.logp) a.logp = fp(pl.lse[0]);                    // (required by the table pass's block, which writes neither)
  // 1 .. 4: the pick's band passes, their logits kept
  if (const int rc = adaptive_band_passes(a, pl, &sp, st)) return rc;
  // 5. per (row, band): lse and the band's k best raw logits
  AdaptiveSelectP s = {};
  AdaptiveJointP q = {};
  for (int b = 0; b <= n; ++b) {
    const int Vb = (int)(b ? a.cut[b] - a.cut[b - 1] : a.cut[0]);
    const bool split = b && a.dims[b - 1] <= AP_MAX_K;
    s.cand[b] = vp(pl.cand[b]); s.sum[b] = fp(pl.sum[b]); s.tile[b] = split ? vp(sp.tcand[b - 1]) : vp(pl.cand[b]);
    s.logits[b] = q.logits[b] = fp(sp.logits[b]); s.lse[b] = fp(pl.lse[b]); q.lse[b] = fp(pl.lse[b]);
    s.parts[b] = pl.parts[b]; s.vb[b] = q.vb[b] = Vb; q.cut[b] = a.cut[b];
  }
  s.cls_cand = vp(pl.cls_cand); s.cls_sum = fp(pl.cls_sum);
  s.list_idx = reinterpret_cast<int32_t*>(a.ws + sp.list_idx); s.list_val = fp(sp.list_val);
  s.done = j.W ? j.beam.done : nullptr; s.n = n; s.k = k; s.W = j.W;
  if (bans) {                                             // (ABI 36) the ban-list launch, then the selection with the list applied
    if (const int rc = ceva_beam_bans(*bans, st)) return rc;
    AdaptiveBanP c = {};
    c.list = BanListP{bans->ban, bans->nban, bans->cap};
    for (int b = 1; b <= n; ++b) c.base[b] = a.cut[b - 1];
    hipLaunchKernelGGL(adaptive_select_c_kernel, dim3((unsigned)a.M, (unsigned)(n + 1)), dim3(SMP_THREADS), 0, st, s, c);
  } else {
    hipLaunchKernelGGL(adaptive_select_kernel, dim3((unsigned)a.M, (unsigned)(n + 1)), dim3(SMP_THREADS), 0, st, s);
  }
  if (const int rc = (int)hipGetLastError()) return rc;
  // 6. per row: the joint scores, the k best, the draw or the beam's candidates
  q.cls = fp(pl.cls); q.list_idx = s.list_idx; q.list_val = s.list_val; q.n = n; q.k = k; q.a = j;
  if (j.W) {
    if (!q.a.beam.cand_idx) q.a.beam.cand_idx = reinterpret_cast<int32_t*>(a.ws + sp.cand_idx);
    if (!q.a.beam.cand_score) q.a.beam.cand_score = fp(sp.cand_score);
  }
  hipLaunchKernelGGL(adaptive_joint_kernel, dim3((unsigned)a.M), dim3(SMP_THREADS), 0, st, q);
  if (const int rc = (int)hipGetLastError()) return rc;
  // 7. the beam's merge, unchanged
  return j.W ? ceva_beam_merge(q.a.beam, st) : 0;
}

}  // namespace ea
