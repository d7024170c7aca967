// ea_ceva_decode_vocab.hip -- the greedy token pick of a decoding step on a vocabulary table the state holds (ABI 26), the
// sampled one (ABI 27: ceva_vocab_sample_kernel, further down, behind the same first launch) and the token log-probabilities
// (ABI 28: ceva_vocab_lse_kernel and ceva_vocab_lse_pick_kernel, at the end)
//
//   logit[m, v] = sum_k round_w(x[m, k]) w[v, k]            fp32, no bias;  1 <= M <= 64 rows, w [V, K] 16-bit row-major
//   token[m]    = argmax_v logit[m, v]                      the largest value; equal values: the lowest index; a row with NaN
//   top[m]      = logit[m, token[m]]                        logits: the lowest index that holds one (torch.argmax's rule)
//
// The step is bound by reading w once (2 V K bytes: 67 MB at V = 32768, K = 1024).  ceva_vocab_kernel is the tile loop of
// ceva_linear_kernel (ea_ceva_decode_linear.hip, whose instructions are pinned and which is therefore not touched): w is the
// B operand of v_mfma_f32_16x16x32, one 16-byte global load per lane straight into the operand registers; the 8 waves of a
// workgroup split K into contiguous runs of 32-wide k-steps, NS steps in flight; the partial tiles meet in LDS and the
// thread that owns an element adds them in wave order.  An element's sum is formed by the same operations in the same order
// as ceva_linear_kernel forms it: the logits are that kernel's bits.
//
// One workgroup owns VOC_TILE = 16 columns (one column tile) and all row tiles.  The last tile may reach past V: its
// addresses are clamped to row V - 1, and a column >= V is neither stored nor picked.  Epilogue: the thread that holds a summed
// element stores it when logits are asked for; the 16 lanes that hold a row's 16 columns reduce them to one (value, index)
// candidate by lane exchanges and write it to ws[m][workgroup].  ceva_vocab_pick_kernel, one workgroup per row, reduces the
// row's ceil(V / 16) candidates under the same rule and writes token[m] (int64) and top[m].  The rule is a total order on
// (value, index) pairs with distinct indices, so the pick does not depend on the order of the reduction; the order is fixed all
// the same.  No atomics, no workgroup waits for another: a replay repeats the bits.
#include <limits.h>
#include <math.h>
#include "ea_common.h"
#include "ea_ceva_decode_vocab.h"

namespace ea {
namespace {

constexpr int VOC_NW = 8;              // waves per workgroup
constexpr int VOC_NS = 4;              // k-steps a wave loads ahead
constexpr int PICK_THREADS = 512;

static_assert(sizeof(VocPick) == 8, "a candidate is one 8-byte store");

// eight consecutive k of one row of x as they lie in memory, and as the A operand (fp32: rounded to nearest even)
template <bool XF32> struct VocX;
template <> struct VocX<true> {
  f32x4 a, b;
  EA_DEV void load(const char* xrow, int k) {
    a = *reinterpret_cast<const f32x4*>(xrow + (int64_t)k * 4);
    b = *reinterpret_cast<const f32x4*>(xrow + (int64_t)k * 4 + 16);
  }
  template <typename E> EA_DEV u32x4 frag() const {
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return pack8<E>(f);
  }
};
template <> struct VocX<false> {
  u32x4 v;
  EA_DEV void load(const char* xrow, int k) { v = ldg16(xrow + (int64_t)k * 2); }
  template <typename E> EA_DEV u32x4 frag() const { return v; }
};

// a takes b's place: a NaN beats every number, a larger number a smaller one, and of two equals (two NaNs, +0 and -0) the
// lower index
EA_DEV bool voc_beats(const VocPick a, const VocPick b) {
  const bool an = a.v != a.v, bn = b.v != b.v;
  if (an || bn) return an && (!bn || a.i < b.i);
  return a.v > b.v || (a.v == b.v && a.i < b.i);
}

// what every candidate beats: no column
EA_DEV VocPick voc_none() { return VocPick{-INFINITY, INT_MAX}; }

EA_DEV VocPick voc_exchange(const VocPick c, int lane_xor) {
  return VocPick{__shfl_xor(c.v, lane_xor), __shfl_xor(c.i, lane_xor)};
}

template <typename E, bool XF32, int RT>
__global__ __launch_bounds__(VOC_NW * 64) void ceva_vocab_kernel(const DecVocabP p) {
  __shared__ float red[VOC_NW * RT * 256];            // [wave][row tile][16 rows][16 columns]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.x * VOC_TILE;
  const int KS = p.K >> 5;
  const int S = (KS + VOC_NW - 1) / VOC_NW;
  const int s_begin = wave * S, s_end = min(KS, s_begin + S);
  const int live_cols = min(VOC_TILE, p.V - n0);      // columns of this tile below V: at least one
  const char* wrow = p.w + ((int64_t)(n0 + min(li, live_cols - 1)) * p.K + 8 * g) * 2;  // (a column past V: row V - 1 again)
  const char* xrow[RT];
  bool xlive[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int m = rt * 16 + li;
    xlive[rt] = m < p.M;
    xrow[rt] = p.x + (int64_t)min(m, p.M - 1) * p.ldx * (XF32 ? 4 : 2);
  }
  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int s0 = s_begin; s0 < s_end; s0 += VOC_NS) {
    u32x4 wf[VOC_NS];
    VocX<XF32> xr[VOC_NS][RT];
#pragma unroll
    for (int i = 0; i < VOC_NS; ++i) {                 // (a step past the wave's run: a clamped address, a zero operand below)
      const int s = min(s0 + i, KS - 1);
      wf[i] = ldg16(wrow + (int64_t)s * 64);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) xr[i][rt].load(xrow[rt], s * 32 + 8 * g);
    }
    __builtin_amdgcn_sched_barrier(0);                 // every load of the pass is out before the first conversion and MFMA
#pragma unroll
    for (int i = 0; i < VOC_NS; ++i) {
      const bool live = s0 + i < s_end;
      const u32x4 wv = live ? wf[i] : zero;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const u32x4 xc = xr[i][rt].template frag<E>();
        const u32x4 xv = live && xlive[rt] ? xc : zero;
        acc[rt] = E::mma(as_x8<E>(xv), as_x8<E>(wv), acc[rt]);
      }
    }
  }
  // D[row = 4 g + r][col = li] of every row tile -> LDS; then element e of the [16 RT, 16] tile is summed over the waves,
  // in wave order, by one thread
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * RT + rt) * 256 + (4 * g + r) * 16 + li] = acc[rt][r];
  __syncthreads();
  const int NB = (p.V - 1) / VOC_TILE + 1;
  // (whole waves enter or skip an iteration: 256 elements are four waves; a row's 16 columns are 16 lanes in a row)
  for (int e = threadIdx.x; e < RT * 256; e += VOC_NW * 64) {
    const int rt = e >> 8, idx = e & 255, m = rt * 16 + (idx >> 4), n = n0 + (idx & 15);
    const bool col = (idx & 15) < live_cols;
    float v = red[rt * 256 + idx];
#pragma unroll
    for (int w = 1; w < VOC_NW; ++w) v += red[(w * RT + rt) * 256 + idx];
    if (m < p.M && col && p.logits) {
      if (p.l_f32) reinterpret_cast<float*>(p.logits)[(int64_t)m * p.ldl + n] = v;
      else reinterpret_cast<uint16_t*>(p.logits)[(int64_t)m * p.ldl + n] = E::from_f(v);
    }
    VocPick c = col ? VocPick{v, n} : voc_none();
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const VocPick other = voc_exchange(c, o);
      if (voc_beats(other, c)) c = other;
    }
    if (m < p.M && (idx & 15) == 0) p.ws[(int64_t)m * NB + blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(PICK_THREADS) void ceva_vocab_pick_kernel(const DecVocabP p) {
  __shared__ VocPick best[PICK_THREADS / 64];
  const int m = blockIdx.x;
  const int NB = (p.V - 1) / VOC_TILE + 1;
  const VocPick* row = p.ws + (int64_t)m * NB;
  VocPick c = voc_none();
#pragma unroll 4
  for (int j = threadIdx.x; j < NB; j += PICK_THREADS) {
    const VocPick other = row[j];
    if (voc_beats(other, c)) c = other;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const VocPick other = voc_exchange(c, o);
    if (voc_beats(other, c)) c = other;
  }
  if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < PICK_THREADS / 64; ++w)
      if (voc_beats(best[w], c)) c = best[w];
    p.token[m] = (int64_t)c.i;
    if (p.top) p.top[m] = c.v;
  }
}

// ---- the sampled pick (ABI 27) ----------------------------------------------------------------------------------------------
// ceva_vocab_sample_kernel, one workgroup per row of x, behind ceva_vocab_kernel (which has stored the row's fp32 logits and
// one candidate per 16-column tile): the top_k best logits under voc_beats' order, softmax weights at a temperature, the
// nucleus, one Philox4x32-10 draw.  (value, index) pairs are compared as 64-bit keys: the value's order-preserving image in
// the high word -- every NaN one largest key, -0 as +0: what voc_beats calls equal -- and the complement of the index in
// the low word, so a larger key is a pair that beats, and no two keys are equal.
constexpr int SMP_THREADS = 512;
constexpr int SMP_POOL = VOC_SAMPLE_MAX_K * VOC_TILE;   // columns of the selected tiles
constexpr int SMP_UNROLL = 8;                           // keys a thread loads before it counts them

EA_DEV uint64_t voc_key(float v, int32_t i) {
  uint32_t b = __float_as_uint(v), k;
  if (v != v) {
    k = 0xFFFFFFFFu;
  } else {
    if (v == 0.f) b = 0u;
    k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);     // (-inf: 0x007FFFFF, the smallest: key 0 is no pair's)
  }
  return ((uint64_t)k << 32) | (uint32_t)~(uint32_t)i;
}
EA_DEV int32_t voc_key_index(uint64_t key) { return (int32_t)~(uint32_t)key; }

// The `need` largest of n distinct keys key_of(0 .. n - 1), 1 <= need <= n: -> t such that exactly `need` keys are >= t.  A
// radix select, 8 bits a pass from the top: a histogram of the next digit over the keys that match the digits fixed so far,
// then the digit the need-th largest key has.  It stops at the pass whose bucket is taken whole.  Integer LDS atomics: the
// counts do not depend on their order.  Every thread of the workgroup calls it; hist [256], pass [3].
template <typename Load>
EA_DEV uint64_t voc_threshold(Load key_of, int n, int need, uint32_t* hist, uint32_t* pass) {
  const int lane = threadIdx.x & 63;
  uint64_t prefix = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    const uint64_t fixed = shift == 56 ? 0ull : ~0ull << (shift + 8);
    if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += SMP_UNROLL * SMP_THREADS) {   // (whole waves enter an iteration; its loads go out first)
      uint64_t keys[SMP_UNROLL];
#pragma unroll
      for (int u = 0; u < SMP_UNROLL; ++u) {
        const int j = j0 + u * SMP_THREADS + (int)threadIdx.x;
        keys[u] = j < n ? key_of(j) : 0ull;
      }
#pragma unroll
      for (int u = 0; u < SMP_UNROLL; ++u) {
        const bool live = j0 + u * SMP_THREADS + (int)threadIdx.x < n && (keys[u] & fixed) == prefix;
        const uint32_t d = (uint32_t)(keys[u] >> shift) & 255u;
        // the keys of a pass mostly share one digit: the lanes that hold the first live lane's digit add once, together
        const uint64_t act = __ballot(live);
        if (act) {
          const uint32_t d0 = (uint32_t)__shfl((int)d, __ffsll((unsigned long long)act) - 1);
          const uint64_t same = __ballot(live && d == d0);
          if (live) {
            if (d != d0) atomicAdd(&hist[d], 1u);
            else if (lane == __ffsll((unsigned long long)same) - 1) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {                               // lane l: bins 4 l .. 4 l + 3; `above`: the keys of larger digits
      uint32_t h[4], s = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) { h[b] = hist[4 * lane + b]; s += h[b]; }
      uint32_t x = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_down((int)x, o);
        if (lane + o < 64) x += t;
      }
      uint32_t above = x - s;
#pragma unroll
      for (int b = 3; b >= 0; --b) {
        if (above < (uint32_t)need && (uint32_t)need <= above + h[b]) {
          pass[0] = (uint32_t)(4 * lane + b); pass[1] = (uint32_t)need - above; pass[2] = h[b];
        }
        above += h[b];
      }
    }
    __syncthreads();
    prefix |= (uint64_t)pass[0] << shift;
    need = (int)pass[1];
    if (pass[2] == (uint32_t)need) break;                 // (uniform: the whole bucket is taken)
  }
  return prefix;
}

// the keys >= t, in any order -> out[0 .. cap - 1]; *count (zero before) counts them
template <typename Load>
EA_DEV void voc_compact(Load key_of, int n, uint64_t t, uint64_t* out, int cap, uint32_t* count) {
  for (int j0 = 0; j0 < n; j0 += SMP_UNROLL * SMP_THREADS) {
    uint64_t keys[SMP_UNROLL];
#pragma unroll
    for (int u = 0; u < SMP_UNROLL; ++u) {
      const int j = j0 + u * SMP_THREADS + (int)threadIdx.x;
      keys[u] = j < n ? key_of(j) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < SMP_UNROLL; ++u)
      if (j0 + u * SMP_THREADS + (int)threadIdx.x < n && keys[u] >= t) {
        const uint32_t at = atomicAdd(count, 1u);
        if (at < (uint32_t)cap) out[at] = keys[u];
      }
  }
}

// word 0 of Philox4x32-10 (Salmon et al., SC 2011)
EA_DEV uint32_t philox4x32_10_word0(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
  }
  return c0;
}

__global__ __launch_bounds__(SMP_THREADS) void ceva_vocab_sample_kernel(const DecSampleP p) {
  __shared__ uint64_t pool[SMP_POOL];                     // the keys of the selected tiles' columns (0: a column >= V)
  __shared__ uint64_t sel[VOC_SAMPLE_MAX_K];              // the selected tiles' candidates; then the top_k keys, unordered
  __shared__ uint64_t sorted[VOC_SAMPLE_MAX_K];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t pass[3];
  __shared__ uint32_t count[2];
  const int m = blockIdx.x, lane = threadIdx.x & 63;
  const int NB = (p.V - 1) / VOC_TILE + 1;
  const VocPick* cand = p.ws + (int64_t)m * NB;
  const float* lrow = p.logits + (int64_t)m * p.ldl;
  const int kt = min(p.top_k, NB);                        // tiles: a tile that holds one of the k best logits has a maximum
  const int kk = min(p.top_k, p.V);                       // that is among the k best maxima
  if (threadIdx.x < 2) count[threadIdx.x] = 0u;
  // 1. the kt best candidates
  auto cand_key = [&](int j) { const VocPick c = cand[j]; return voc_key(c.v, c.i); };
  const uint64_t t1 = kt < NB ? voc_threshold(cand_key, NB, kt, hist, pass) : 0ull;
  __syncthreads();
  voc_compact(cand_key, NB, t1, sel, kt, &count[0]);
  __syncthreads();
  // 2. their columns' logits, and the kk best of those, in order
  const int np = kt * VOC_TILE;
  for (int e = threadIdx.x; e < np; e += SMP_THREADS) {
    const int col = (voc_key_index(sel[e >> 4]) & ~(VOC_TILE - 1)) + (e & (VOC_TILE - 1));
    pool[e] = (uint32_t)col < (uint32_t)p.V ? voc_key(lrow[col], col) : 0ull;
  }
  __syncthreads();
  auto pool_key = [&](int j) { return pool[j]; };
  const uint64_t t2 = kk < np ? voc_threshold(pool_key, np, kk, hist, pass) : 1ull;
  __syncthreads();
  voc_compact(pool_key, np, t2, sel, kk, &count[1]);
  __syncthreads();
  if ((int)threadIdx.x < kk) {
    const uint64_t key = sel[threadIdx.x];
    int rank = 0;
    for (int i = 0; i < kk; ++i) rank += sel[i] > key;
    sorted[rank] = key;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  // 3 .. 6: one wave, entry j of the selection in lane j
  const bool live = lane < kk;
  const int32_t idx = live ? min(max(voc_key_index(sorted[lane]), 0), p.V - 1) : 0;   // (a column of the row, come what may)
  const float val = live ? lrow[idx] : -INFINITY;        // (the stored logit's own bits: the key has folded -0 and NaNs)
  if (live && p.sel_idx) p.sel_idx[(int64_t)m * p.top_k + lane] = idx;
  if (live && p.sel_val) p.sel_val[(int64_t)m * p.top_k + lane] = val;
  const float v0 = __shfl(val, 0);
  const int64_t n = p.ctr[m];
  int32_t token = __shfl(idx, 0), kept = 0;
  if (v0 - v0 == 0.f) {                                   // (a NaN or an infinite best logit: the greedy pick, kept = 0)
    const float w = live ? expf((val - v0) / p.temperature) : 0.f;
    float run = 0.f, c = 0.f;                             // c_j = ((w_0 + w_1) + ..) + w_j
#pragma unroll
    for (int j = 0; j < VOC_SAMPLE_MAX_K; ++j) {
      run += __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(w), j));
      if (lane == j) c = run;
    }
    const uint64_t in = __ballot(live && c >= p.top_p * run);
    kept = p.top_p >= 1.f || !in ? kk : __ffsll((unsigned long long)in);
    const uint32_t word = philox4x32_10_word0(p.seed_lo, p.seed_hi, (uint32_t)(uint64_t)n, (uint32_t)((uint64_t)n >> 32),
                                              (uint32_t)p.sid[m], 0u);
    const float u = ((float)(word >> 8) + 0.5f) * 0x1p-24f;
    const float r = u * __shfl(c, kept - 1);
    const uint64_t hit = __ballot(lane < kept && c > r);
    token = __shfl(idx, hit ? __ffsll((unsigned long long)hit) - 1 : kept - 1);
  }
  if (lane == 0) {
    p.token[m] = (int64_t)token;
    if (p.kept) p.kept[m] = kept;
    p.ctr[m] = n + 1;                                     // (this workgroup alone reads and writes ctr[m])
  }
}

// ---- token log-probabilities (ABI 28) ---------------------------------------------------------------------------------------
// ceva_vocab_lse_kernel is ceva_vocab_kernel's tile loop, reduction, logits store and candidate written again (the kernels
// above are pinned instruction for instruction: tools/isa_diff.py), with one more epilogue step: behind the candidate exchange
// the 16 lanes of a row group all hold the tile's best (m_t, i_t), and s_t = sum_columns exp(logit - m_t) goes to lws[m][tile].
// ceva_vocab_lse_pick_kernel, one workgroup per row, reduces the candidates as ceva_vocab_pick_kernel does, folds the tile
// sums into lse[m] = top + log(sum_t s_t exp(m_t - top)) and writes logp[m] = (the token's, the target's or the top
// logit) - lse[m]: the log-probability under the model's own distribution at temperature 1, nothing truncated.
template <typename E, bool XF32, int RT>
__global__ __launch_bounds__(VOC_NW * 64) void ceva_vocab_lse_kernel(const DecLseP p) {
  __shared__ float red[VOC_NW * RT * 256];            // [wave][row tile][16 rows][16 columns]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.x * VOC_TILE;
  const int KS = p.K >> 5;
  const int S = (KS + VOC_NW - 1) / VOC_NW;
  const int s_begin = wave * S, s_end = min(KS, s_begin + S);
  const int live_cols = min(VOC_TILE, p.V - n0);      // columns of this tile below V: at least one
  const char* wrow = p.w + ((int64_t)(n0 + min(li, live_cols - 1)) * p.K + 8 * g) * 2;  // (a column past V: row V - 1 again)
  const char* xrow[RT];
  bool xlive[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int m = rt * 16 + li;
    xlive[rt] = m < p.M;
    xrow[rt] = p.x + (int64_t)min(m, p.M - 1) * p.ldx * (XF32 ? 4 : 2);
  }
  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int s0 = s_begin; s0 < s_end; s0 += VOC_NS) {
    u32x4 wf[VOC_NS];
    VocX<XF32> xr[VOC_NS][RT];
#pragma unroll
    for (int i = 0; i < VOC_NS; ++i) {                 // (a step past the wave's run: a clamped address, a zero operand below)
      const int s = min(s0 + i, KS - 1);
      wf[i] = ldg16(wrow + (int64_t)s * 64);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) xr[i][rt].load(xrow[rt], s * 32 + 8 * g);
    }
    __builtin_amdgcn_sched_barrier(0);                 // every load of the pass is out before the first conversion and MFMA
#pragma unroll
    for (int i = 0; i < VOC_NS; ++i) {
      const bool live = s0 + i < s_end;
      const u32x4 wv = live ? wf[i] : zero;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const u32x4 xc = xr[i][rt].template frag<E>();
        const u32x4 xv = live && xlive[rt] ? xc : zero;
        acc[rt] = E::mma(as_x8<E>(xv), as_x8<E>(wv), acc[rt]);
      }
    }
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * RT + rt) * 256 + (4 * g + r) * 16 + li] = acc[rt][r];
  __syncthreads();
  const int NB = (p.V - 1) / VOC_TILE + 1;
  // (whole waves enter or skip an iteration: 256 elements are four waves; a row's 16 columns are 16 lanes in a row)
  for (int e = threadIdx.x; e < RT * 256; e += VOC_NW * 64) {
    const int rt = e >> 8, idx = e & 255, m = rt * 16 + (idx >> 4), n = n0 + (idx & 15);
    const bool col = (idx & 15) < live_cols;
    float v = red[rt * 256 + idx];
#pragma unroll
    for (int w = 1; w < VOC_NW; ++w) v += red[(w * RT + rt) * 256 + idx];
    if (m < p.M && col && p.logits) {
      if (p.l_f32) reinterpret_cast<float*>(p.logits)[(int64_t)m * p.ldl + n] = v;
      else reinterpret_cast<uint16_t*>(p.logits)[(int64_t)m * p.ldl + n] = E::from_f(v);
    }
    if (p.targets && m < p.M && col && p.targets[m] == (int64_t)n) p.tlogit[m] = v;
    VocPick c = col ? VocPick{v, n} : voc_none();
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const VocPick other = voc_exchange(c, o);
      if (voc_beats(other, c)) c = other;
    }
    // every lane of the row group holds (m_t, i_t) now; a column >= V adds nothing.  (m_t NaN or infinite: s_t is whatever
    // comes out -- the second launch does not read it then)
    float s = col ? expf(v - c.v) : 0.f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (m < p.M && (idx & 15) == 0) {
      p.ws[(int64_t)m * NB + blockIdx.x] = c;
      p.lws[(int64_t)m * NB + blockIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__(PICK_THREADS) void ceva_vocab_lse_pick_kernel(const DecLseP p) {
  __shared__ VocPick best[PICK_THREADS / 64];
  __shared__ float part[PICK_THREADS / 64];
  __shared__ float top_of_row;
  const int m = blockIdx.x;
  const int NB = (p.V - 1) / VOC_TILE + 1;
  const VocPick* row = p.ws + (int64_t)m * NB;
  const float* srow = p.lws + (int64_t)m * NB;
  // pass 1: ceva_vocab_pick_kernel's reduction
  VocPick c = voc_none();
#pragma unroll 4
  for (int j = threadIdx.x; j < NB; j += PICK_THREADS) {
    const VocPick other = row[j];
    if (voc_beats(other, c)) c = other;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const VocPick other = voc_exchange(c, o);
    if (voc_beats(other, c)) c = other;
  }
  if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < PICK_THREADS / 64; ++w)
      if (voc_beats(best[w], c)) c = best[w];
    if (!p.token_in) {                                    // (the sampled mode: the token was drawn before this launch)
      p.token[m] = (int64_t)c.i;
      if (p.top) p.top[m] = c.v;
    }
    top_of_row = c.v;
  }
  __syncthreads();
  const float top = top_of_row;
  // pass 2: S = sum_t s_t exp(m_t - top) over the tiles that hold a number (a finite top: every m_t is finite or -inf, every
  // exponent <= 0).  A tile of -inf alone is skipped, never multiplied.
  float s = 0.f;
  if (top - top == 0.f) {                                 // (uniform)
    for (int j = threadIdx.x; j < NB; j += PICK_THREADS) {
      const float mt = row[j].v;
      if (mt != -INFINITY) s += srow[j] * expf(mt - top);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  float total = part[0];
#pragma unroll
  for (int w = 1; w < PICK_THREADS / 64; ++w) total += part[w];
  // top NaN: NaN; +inf: +inf; -inf (every logit is -inf): -inf
  const float lse = top - top == 0.f ? top + logf(total) : top;
  float tl = top;
  if (p.token_in) {
    const int64_t t = p.token_in[m];
    tl = t >= 0 && t < (int64_t)p.V ? reinterpret_cast<const float*>(p.logits)[(int64_t)m * p.ldl + t] : NAN;
  } else if (p.targets) {
    const int64_t t = p.targets[m];
    tl = t >= 0 && t < (int64_t)p.V ? p.tlogit[m] : NAN;   // (no thread of the first launch has written tlogit[m] otherwise)
  }
  p.lse[m] = lse;
  p.logp[m] = tl - lse;
}


using VocKernel = void (*)(const DecVocabP);

template <typename E, bool XF32>
VocKernel voc_of(int M) {
  if (M <= 16) return ceva_vocab_kernel<E, XF32, 1>;
  if (M <= 32) return ceva_vocab_kernel<E, XF32, 2>;
  return ceva_vocab_kernel<E, XF32, 4>;
}

template <typename E>
VocKernel voc_of(bool xf32, int M) { return xf32 ? voc_of<E, true>(M) : voc_of<E, false>(M); }

using LseKernel = void (*)(const DecLseP);

template <typename E, bool XF32>
LseKernel lse_of(int M) {
  if (M <= 16) return ceva_vocab_lse_kernel<E, XF32, 1>;
  if (M <= 32) return ceva_vocab_lse_kernel<E, XF32, 2>;
  return ceva_vocab_lse_kernel<E, XF32, 4>;
}

template <typename E>
LseKernel lse_of(bool xf32, int M) { return xf32 ? lse_of<E, true>(M) : lse_of<E, false>(M); }

}  // namespace

int64_t ceva_sdecode_vocab_ws(int M, int V) {
  if (M < 1 || M > EA_CEVA_LINEAR_MAX_ROWS || V < 1) return -1;
  return (int64_t)M * ((V - 1) / VOC_TILE + 1) * (int64_t)sizeof(VocPick);
}

// (The C entry point has checked pointers, strides, alignment and the size of ws.)
static int voc_kernel_of(const DecVocabP& p, VocKernel* kernel) {
  if (!p.x || !p.w || !p.ws || p.M < 1 || p.ldx < p.K || (p.logits && p.ldl < p.V)) return EA_E_BADARG;
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.V < 1) return EA_E_UNSUPPORTED;
  switch (p.dtype) {
    case EA_BF16: *kernel = voc_of<BF16>(p.x_f32 != 0, p.M); break;
    case EA_F16: *kernel = voc_of<F16>(p.x_f32 != 0, p.M); break;
    default: return EA_E_BADARG;
  }
  return 0;
}

int ceva_sdecode_vocab_argmax(const DecVocabP& p, hipStream_t st) {
  if (!p.token) return EA_E_BADARG;
  VocKernel kernel;
  int rc = voc_kernel_of(p, &kernel);
  if (rc != 0) return rc;
  const unsigned NB = (unsigned)((p.V - 1) / VOC_TILE + 1);
  hipLaunchKernelGGL(kernel, dim3(NB), dim3(VOC_NW * 64), 0, st, p);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ceva_vocab_pick_kernel, dim3((unsigned)p.M), dim3(PICK_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

int ceva_sdecode_vocab_sample(const DecVocabP& p, const DecSampleP& s, hipStream_t st) {
  if (!s.token || !s.ctr || !s.sid || !p.logits || !p.l_f32 || (const char*)s.logits != p.logits || s.ldl != p.ldl ||
      s.ws != p.ws || s.V != p.V) return EA_E_BADARG;
  if (s.top_k < 1 || !(s.top_p > 0.f && s.top_p <= 1.f) || !(s.temperature > 0.f && s.temperature - s.temperature == 0.f))
    return EA_E_BADARG;
  VocKernel kernel;
  int rc = voc_kernel_of(p, &kernel);
  if (rc != 0) return rc;
  if (s.top_k > VOC_SAMPLE_MAX_K) return EA_E_UNSUPPORTED;
  const unsigned NB = (unsigned)((p.V - 1) / VOC_TILE + 1);
  hipLaunchKernelGGL(kernel, dim3(NB), dim3(VOC_NW * 64), 0, st, p);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ceva_vocab_sample_kernel, dim3((unsigned)p.M), dim3(SMP_THREADS), 0, st, s);
  return (int)hipGetLastError();
}

int64_t ceva_sdecode_vocab_lse_ws(int M, int V) {
  if (M < 1 || M > EA_CEVA_LINEAR_MAX_ROWS || V < 1) return -1;
  return (int64_t)M * ((V - 1) / VOC_TILE + 1) * (int64_t)sizeof(float) + (int64_t)M * (int64_t)sizeof(float);
}

// (The C entry point has checked pointers, strides, alignment and the sizes of ws and lws.)
static int lse_kernel_of(const DecLseP& p, LseKernel* kernel) {
  if (!p.x || !p.w || !p.ws || !p.lws || !p.tlogit || !p.lse || !p.logp || p.M < 1 || p.ldx < p.K || (p.logits && p.ldl < p.V))
    return EA_E_BADARG;
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.V < 1) return EA_E_UNSUPPORTED;
  switch (p.dtype) {
    case EA_BF16: *kernel = lse_of<BF16>(p.x_f32 != 0, p.M); break;
    case EA_F16: *kernel = lse_of<F16>(p.x_f32 != 0, p.M); break;
    default: return EA_E_BADARG;
  }
  return 0;
}

int ceva_sdecode_vocab_logprob(const DecLseP& p, hipStream_t st) {
  if (!p.token || p.token_in) return EA_E_BADARG;
  LseKernel kernel;
  int rc = lse_kernel_of(p, &kernel);
  if (rc != 0) return rc;
  const unsigned NB = (unsigned)((p.V - 1) / VOC_TILE + 1);
  hipLaunchKernelGGL(kernel, dim3(NB), dim3(VOC_NW * 64), 0, st, p);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ceva_vocab_lse_pick_kernel, dim3((unsigned)p.M), dim3(PICK_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

int ceva_sdecode_vocab_sample_logprob(const DecLseP& p, const DecSampleP& s, hipStream_t st) {
  if (!s.token || !s.ctr || !s.sid || !p.logits || !p.l_f32 || (const char*)s.logits != p.logits || s.ldl != p.ldl ||
      s.ws != p.ws || s.V != p.V || p.token_in != s.token || p.targets) return EA_E_BADARG;
  if (s.top_k < 1 || !(s.top_p > 0.f && s.top_p <= 1.f) || !(s.temperature > 0.f && s.temperature - s.temperature == 0.f))
    return EA_E_BADARG;
  LseKernel kernel;
  int rc = lse_kernel_of(p, &kernel);
  if (rc != 0) return rc;
  if (s.top_k > VOC_SAMPLE_MAX_K) return EA_E_UNSUPPORTED;
  const unsigned NB = (unsigned)((p.V - 1) / VOC_TILE + 1);
  hipLaunchKernelGGL(kernel, dim3(NB), dim3(VOC_NW * 64), 0, st, p);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ceva_vocab_sample_kernel, dim3((unsigned)p.M), dim3(SMP_THREADS), 0, st, s);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ceva_vocab_lse_pick_kernel, dim3((unsigned)p.M), dim3(PICK_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace ea
