// ea_voc_select.h -- the exact selection of a row's k best (value, index) pairs and the sampler's draw: what the sampled pick
// (ABI 27), the beam step (ABI 32) and the adaptive head's selection (ABI 35) share.  Included by ea_ceva_decode_vocab.hip and
// ea_adaptive_pick.hip, inside their anonymous namespace, behind ea_ceva_decode_rows.h (voc_beats' order is the keys').
// The sampled pick, one workgroup of SMP_THREADS per row behind a table pass that has stored the row's fp32 logits and one
// candidate per 16-column tile: the top_k best logits under voc_beats' order (voc_select), softmax weights at a temperature,
// the nucleus, one Philox4x32-10 draw (voc_draw).  (value, index) pairs are compared as 64-bit keys: the value's
// order-preserving image in the high word -- every NaN one largest key, -0 as +0: what voc_beats calls equal -- and the
// complement of the index in the low word, so a larger key is a pair that beats, and no two keys are equal.
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

// n <= 64 distinct keys sel[0 .. n - 1] -> sorted[0 .. n - 1], the largest first; it ends behind a barrier
EA_DEV void voc_rank_sort(const uint64_t* sel, uint64_t* sorted, int n) {
  if ((int)threadIdx.x < n) {
    const uint64_t key = sel[threadIdx.x];
    int rank = 0;
    for (int i = 0; i < n; ++i) rank += sel[i] > key;
    sorted[rank] = key;
  }
  __syncthreads();
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

// what voc_select works in
struct VocSelect {
  uint64_t pool[SMP_POOL];                                // the keys of the selected tiles' columns (0: a column >= V)
  uint64_t sel[VOC_SAMPLE_MAX_K];                         // the selected tiles' candidates; then the top_k keys, unordered
  uint64_t sorted[VOC_SAMPLE_MAX_K];
  uint32_t hist[256];
  uint32_t pass[3];
  uint32_t count[2];
};

// Steps 1 and 2 of the sampled pick on one row: cand [NB] the table pass's candidates, lrow [V] its fp32 logits ->
// kk = min(top_k, V), and sh.sorted[0 .. kk - 1]: the keys of the row's kk best logits, in order.  Every thread of the
// SMP_THREADS calls it; it ends behind a barrier.
EA_DEV int voc_select(const VocPick* cand, const float* lrow, int V, int NB, int top_k, VocSelect& sh) {
  const int kt = min(top_k, NB);                          // tiles: a tile that holds one of the k best logits has a maximum
  const int kk = min(top_k, V);                           // that is among the k best maxima
  if (threadIdx.x < 2) sh.count[threadIdx.x] = 0u;
  // 1. the kt best candidates
  auto cand_key = [&](int j) { const VocPick c = cand[j]; return voc_key(c.v, c.i); };
  const uint64_t t1 = kt < NB ? voc_threshold(cand_key, NB, kt, sh.hist, sh.pass) : 0ull;
  __syncthreads();
  voc_compact(cand_key, NB, t1, sh.sel, kt, &sh.count[0]);
  __syncthreads();
  // 2. their columns' logits, and the kk best of those, in order
  const int np = kt * VOC_TILE;
  for (int e = threadIdx.x; e < np; e += SMP_THREADS) {
    const int col = (voc_key_index(sh.sel[e >> 4]) & ~(VOC_TILE - 1)) + (e & (VOC_TILE - 1));
    sh.pool[e] = (uint32_t)col < (uint32_t)V ? voc_key(lrow[col], col) : 0ull;
  }
  __syncthreads();
  auto pool_key = [&](int j) { return sh.pool[j]; };
  const uint64_t t2 = kk < np ? voc_threshold(pool_key, np, kk, sh.hist, sh.pass) : 1ull;
  __syncthreads();
  voc_compact(pool_key, np, t2, sh.sel, kk, &sh.count[1]);
  __syncthreads();
  voc_rank_sort(sh.sel, sh.sorted, kk);
  return kk;
}

// Steps 3 .. 6 of the sampled pick, by ONE wave: entry j of a selection of kk in lane j (val: its value, -inf in a lane
// >= kk; live: lane < kk) -> the lane of the drawn entry, the same in every lane; kept: how many entries the nucleus keeps.
// Weights exp((val - val_0) / temperature), c_j = ((w_0 + w_1) + ..) + w_j, the smallest head whose weight reaches top_p of
// the list's, one Philox4x32-10 word at (n, sid) under the seed.  A NaN or an infinite best value: lane 0, kept = 0.
EA_DEV int voc_draw(float val, bool live, int kk, float top_p, float temperature, uint32_t seed_lo, uint32_t seed_hi,
                    int64_t n, int32_t sid, int32_t& kept) {
  const int lane = threadIdx.x & 63;
  const float v0 = __shfl(val, 0);
  int drawn = 0;
  kept = 0;
  if (v0 - v0 == 0.f) {                                   // (a NaN or an infinite best value: the greedy pick, kept = 0)
    const float w = live ? expf((val - v0) / temperature) : 0.f;
    float run = 0.f, c = 0.f;                             // c_j = ((w_0 + w_1) + ..) + w_j
#pragma unroll
    for (int j = 0; j < VOC_SAMPLE_MAX_K; ++j) {
      run += __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(w), j));
      if (lane == j) c = run;
    }
    const uint64_t in = __ballot(live && c >= top_p * run);
    kept = top_p >= 1.f || !in ? kk : __ffsll((unsigned long long)in);
    const uint32_t word = philox4x32_10_word0(seed_lo, seed_hi, (uint32_t)(uint64_t)n, (uint32_t)((uint64_t)n >> 32),
                                              (uint32_t)sid, 0u);
    const float u = ((float)(word >> 8) + 0.5f) * 0x1p-24f;
    const float r = u * __shfl(c, kept - 1);
    const uint64_t hit = __ballot(lane < kept && c > r);
    drawn = hit ? __ffsll((unsigned long long)hit) - 1 : kept - 1;
  }
  return drawn;
}
