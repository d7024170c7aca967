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
// Ordinary vector stores only; no atomics; no workgroup waits for another; launches only.
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

template <typename E, int RT>
__global__ __launch_bounds__(AP_THREADS) void adaptive_tail_kernel(const AdaptiveTailP p) {
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

__global__ __launch_bounds__(APK_THREADS) void adaptive_pick_kernel(const AdaptivePickFoldP p) {
  __shared__ VocPick wbest[APK_THREADS / 64];
  __shared__ float wpart[APK_THREADS / 64];
  __shared__ float top_of_band;
  const int m = blockIdx.x;
  VocPick best[NB_MAX];                                 // (thread 0's are the bands')
  float lse[NB_MAX];
#pragma unroll
  for (int b = 0; b < NB_MAX; ++b) {
    if (b > p.n) break;                                 // (uniform)
    const int NP = p.parts[b];
    const VocPick* row = p.cand[b] + (int64_t)m * NP;
    const float* srow = p.sum[b] + (int64_t)m * NP;
    // pass 1: the band's best candidate
    VocPick c = voc_none();
    for (int j = threadIdx.x; j < NP; j += APK_THREADS) {
      const VocPick other = row[j];
      if (voc_beats(other, c)) c = other;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const VocPick other = voc_exchange(c, o);
      if (voc_beats(other, c)) c = other;
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < APK_THREADS / 64; ++w)
        if (voc_beats(wbest[w], c)) c = wbest[w];
      float top = c.v;
      if (b == 0 && voc_beats(VocPick{p.cls_cand[m].v, INT_MAX}, VocPick{top, 0})) top = p.cls_cand[m].v;   // the head's top
      top_of_band = top;
    }
    best[b] = c;
    __syncthreads();
    const float top = top_of_band;
    // pass 2: the partial sums against the top
    float s = 0.f;
    if (top - top == 0.f) {                             // (uniform)
      for (int j = threadIdx.x; j < NP; j += APK_THREADS) {
        const float mt = row[j].v;
        if (mt != -INFINITY) s += srow[j] * expf(mt - top);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      float total = wpart[0];
#pragma unroll
      for (int w = 1; w < APK_THREADS / 64; ++w) total += wpart[w];
      if (b == 0 && top - top == 0.f) {                 // the class tile's partial, last
        const float mc = p.cls_cand[m].v;
        if (mc != -INFINITY) total += p.cls_sum[m] * expf(mc - top);
      }
      lse[b] = ap_lse_of(top, total);
      p.best[b][m] = best[b];
      p.lse[b][m] = lse[b];
    }
    __syncthreads();                                    // (wbest, wpart and top_of_band are the next band's)
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

template <typename E>
int tail_launch(const AdaptiveTailP& p, hipStream_t st) {
  const dim3 grid((unsigned)p.NP), block(AP_THREADS);
  if (p.M <= 16) hipLaunchKernelGGL((adaptive_tail_kernel<E, 1>), grid, block, 0, st, p);
  else if (p.M <= 32) hipLaunchKernelGGL((adaptive_tail_kernel<E, 2>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((adaptive_tail_kernel<E, 4>), grid, block, 0, st, p);
  return (int)hipGetLastError();
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

int adaptive_pick(const AdaptivePickP& a, hipStream_t st) {
  AdaptivePickPlan pl;
  if (adaptive_pick_plan(a.M, a.n, a.cut, a.dims, &pl) < 0) return EA_E_UNSUPPORTED;
  if (a.dtype != EA_BF16 && a.dtype != EA_F16) return EA_E_BADARG;
  auto vp = [&](int64_t off) { return reinterpret_cast<VocPick*>(a.ws + off); };
  auto fp = [&](int64_t off) { return reinterpret_cast<float*>(a.ws + off); };
  const int n = a.n, D = pl.D;
  const int64_t c0 = a.cut[0];

  // 1. the head's words: candidates, tile sums and the targets' logits of head[0 .. c0)
  DecLseP hw = {};
  hw.x = a.x; hw.w = a.head; hw.ws = vp(pl.cand[0]); hw.lws = fp(pl.sum[0]); hw.tlogit = fp(pl.tlogit[0]);
  hw.targets = a.targets; hw.token = a.token; hw.lse = fp(pl.lse[0]); hw.logp = a.logp;
  hw.ldx = a.ldx; hw.M = a.M; hw.K = a.C; hw.V = (int)c0; hw.dtype = a.dtype; hw.x_f32 = a.x_f32;
  if (const int rc = ceva_sdecode_vocab_table_pass(hw, st)) return rc;
  // 2. the head's classes: the n rows behind them, the fp32 logits stored
  DecLseP hc = hw;
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
      if (const int rc = ceva_sdecode_vocab_table_pass(t, st)) return rc;
    }
  }
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

}  // namespace ea
