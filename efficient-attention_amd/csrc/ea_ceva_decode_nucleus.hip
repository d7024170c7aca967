// ea_ceva_decode_nucleus.hip -- full-vocabulary and nucleus sampling on a row of stored fp32 logits:
// ceva_vocab_nucleus_kernel, the launch behind the table pass of ea_ceva_sdecode_vocab_sample_full (include/ea_hip.h spells
// the contract out; the table pass and the entries' dispatch are ea_ceva_decode_vocab.hip's).  A translation unit of its own:
// build.py compiles it without packed fp32 operations, so that expf and the quotient are the scalar ones in every lane.
//
// One workgroup of NUC_THREADS per row.  Every weight is an INTEGER, q_v = trunc(expf((l_v - val_0) / T) 2^32), so every sum
// below is exact and does not depend on the order of its terms: the LDS atomics are integer atomics, the result is the same
// on every run, for every split of the row, in every batch.  The row (4 V bytes, L2-resident behind the table pass) is
// streamed a small fixed number of times in 16-byte groups, NUC_UNROLL loads of a thread in flight:
//   A  q_v of every column: a histogram of NUC_BUCKETS buckets over floor(16 (val_0 - l_v) / T) -- a monotone image of the
//      total order, 1/16 nat wide; the last bucket takes everything from 23.94 nats down, where q_v = 0 -- with a u64 mass
//      and a u32 count per bucket, and the mass of each of the row's NUC_BLOCKS blocks of columns.  One wave scans the
//      buckets to target = ceil(top_p Z): the boundary bucket, the mass and the count above it.
//   B  (top_p < 1) the boundary bucket's 64-bit keys compacted into an LDS pool of NUC_POOL, and an 8-bit radix select over
//      them with MASS histograms: the exact threshold pair.  A bucket larger than the pool -- a row of equal logits holds all
//      V columns in one -- is selected by the same passes over the streamed row instead.
//   C  (top_p < 1) the KEPT mass of every block.  At top_p = 1 pass A's block masses are the kept ones.
//   D  one wave scans the blocks to the one that holds r; its chunks are walked with workgroup prefix sums down to the
//      thread, and that thread's four columns to the token.
#include <limits.h>
#include <math.h>
#include "ea_common.h"
#include "ea_ceva_decode_vocab.h"

namespace ea {
namespace {

// the keys' order (voc_beats'), Philox4x32-10
#include "ea_voc_select.h"

constexpr int NUC_THREADS = SMP_THREADS;
constexpr int NUC_GROUP = 4;                              // columns of one 16-byte load
constexpr int NUC_CHUNK = NUC_GROUP * NUC_THREADS;        // columns the workgroup loads at once
constexpr int NUC_UNROLL = 4;                             // chunks a thread loads before it works on them
constexpr int NUC_BLOCKS = 128;                           // blocks of a row: ceil(chunks / 128) chunks each
constexpr int NUC_BUCKETS = 384;
constexpr float NUC_PER_NAT = 16.f;
constexpr int NUC_POOL = 4096;                            // keys of the boundary bucket held in LDS
constexpr int NUC_AGGREGATE = 16;                         // lanes that share a bin before they add to it as one
static_assert(NUC_THREADS == 512 && NUC_BUCKETS % 64 == 0 && NUC_BLOCKS == 128, "the wave scans below are written for these");

EA_DEV float nuc_arg(float l, float v0, float temperature) { return (l - v0) / temperature; }   // <= 0, or -0

// q = trunc(expf(x) 2^32): expf(-23) 2^32 < 1/2, so the cut changes no value; the product is exact
EA_DEV uint64_t nuc_mass(float x) { return x < -23.f ? 0ull : (uint64_t)(expf(x) * 0x1p32f); }

EA_DEV int nuc_bucket(float x) {
  const float s = -x * NUC_PER_NAT;
  return s >= (float)(NUC_BUCKETS - 1) ? NUC_BUCKETS - 1 : max((int)s, 0);   // (x <= 0; a bucket of the histogram, come what may)
}

// the value a key was made of (-0 comes back as +0: the same argument but for its sign, the same mass, the same bucket)
EA_DEV float voc_key_value(uint64_t key) {
  const uint32_t k = (uint32_t)(key >> 32);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

EA_DEV uint64_t nuc_wave_sum(uint64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// lane l: x_0 + .. + x_{l-1}; total: the wave's sum
EA_DEV uint64_t nuc_wave_before(uint64_t x, uint64_t& total) {
  const int lane = threadIdx.x & 63;
  uint64_t incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  total = __shfl(incl, 63);
  return incl - x;
}

// The lanes with `on` add (q, 1) to bin b of (mass, count).  Where at least `aggregate` of them hold the first such lane's
// bin they add once, together: a row of equal logits would otherwise queue 64 atomics on one address per instruction.
// Whole waves call it.
EA_DEV void nuc_hist_add(bool on, uint32_t b, uint64_t q, uint64_t* mass, uint32_t* count, int aggregate) {
  const uint64_t act = __ballot(on);
  if (!act) return;                                       // (uniform)
  const int lane = threadIdx.x & 63, first = __ffsll((unsigned long long)act) - 1;
  const uint32_t b0 = (uint32_t)__shfl((int)b, first);
  const bool mine = on && b == b0;
  const uint64_t same = __ballot(mine);
  const bool together = __popcll(same) >= aggregate;      // (uniform)
  if (together) {
    const uint64_t s = nuc_wave_sum(mine ? q : 0ull);
    if (lane == first) {
      if (s) atomicAdd((unsigned long long*)&mass[b0], (unsigned long long)s);
      atomicAdd(&count[b0], (uint32_t)__popcll(same));
    }
  }
  if (on && !(together && mine)) {
    if (q) atomicAdd((unsigned long long*)&mass[b], (unsigned long long)q);
    atomicAdd(&count[b], 1u);
  }
}

// A row as 16-byte groups: group g holds columns 4 g - a .. 4 g - a + 3, a = the floats by which column 0 lies behind a
// 16-byte boundary (ldl and the logits' alignment are the caller's: 4 bytes is all they promise).
struct NucRow {
  const float* base;                                      // 16-byte aligned; column v at base[v + a]
  int a, V, groups, chunks;
};

EA_DEV NucRow nuc_row(const float* lrow, int V) {
  NucRow r;
  r.a = (int)(((uintptr_t)lrow >> 2) & 3);
  r.base = lrow - r.a;
  r.V = V;
  r.groups = (V + r.a + NUC_GROUP - 1) / NUC_GROUP;
  r.chunks = (r.groups + NUC_THREADS - 1) / NUC_THREADS;
  return r;
}

// group g -> its values and the mask of those that are columns of the row (a group off the row: 0).  Only a group that lies
// in the row whole is loaded whole.
EA_DEV uint32_t nuc_load(const NucRow& r, int g, float (&v)[NUC_GROUP]) {
  const int col0 = NUC_GROUP * g - r.a;
  uint32_t ok = 0u;
  if (g < r.groups && col0 >= 0 && col0 + NUC_GROUP <= r.V) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(r.base + (int64_t)NUC_GROUP * g);
#pragma unroll
    for (int e = 0; e < NUC_GROUP; ++e) v[e] = t[e];
    return 15u;
  }
#pragma unroll
  for (int e = 0; e < NUC_GROUP; ++e) {
    const bool in = g < r.groups && (uint32_t)(col0 + e) < (uint32_t)r.V;
    v[e] = in ? r.base[(int64_t)NUC_GROUP * g + e] : 0.f;
    ok |= (uint32_t)in << e;
  }
  return ok;
}

// f(chunk, first column, values, mask) for the thread's group of every chunk in [c_begin, c_end), NUC_UNROLL loads ahead.
// Whole waves enter f, also with an empty mask.
template <typename F>
EA_DEV void nuc_stream(const NucRow& r, int c_begin, int c_end, F f) {
  for (int c = c_begin; c < c_end; c += NUC_UNROLL) {
    float v[NUC_UNROLL][NUC_GROUP];
    uint32_t ok[NUC_UNROLL];
#pragma unroll
    for (int u = 0; u < NUC_UNROLL; ++u) {
      ok[u] = 0u;
      if (c + u < c_end) ok[u] = nuc_load(r, (c + u) * NUC_THREADS + (int)threadIdx.x, v[u]);
    }
#pragma unroll
    for (int u = 0; u < NUC_UNROLL; ++u)
      if (c + u < c_end) f(c + u, NUC_GROUP * ((c + u) * NUC_THREADS + (int)threadIdx.x) - r.a, v[u], ok[u]);   // (uniform)
  }
}

// what the kernel works in: 43 KB
struct NucShared {
  uint64_t pool[NUC_POOL];                                // the boundary bucket's keys
  uint64_t bmass[NUC_BUCKETS];                            // pass A's histogram
  uint32_t bcnt[NUC_BUCKETS];
  uint64_t hmass[256];                                    // the radix select's
  uint32_t hcnt[256];
  uint64_t blk[NUC_BLOCKS];                               // (kept) mass of the row's blocks
  uint64_t wave[NUC_THREADS / 64];                        // a chunk's mass per wave; pass A: the waves' smallest keys
  uint64_t top;                                           // the best candidate's key
  uint64_t Z, need, above, thr, ckept, qthr, rest;        // `need` of the mass behind `above`; rest: r inside its block
  uint32_t nabove, bucket, digit, count, block;
  int32_t token;
};

// The threshold pair of the keys key_of(0 .. n - 1) (0: no key), each of mass nuc_mass of its value: -> the key t with
// mass(keys > t) < need <= mass(keys >= t), 1 <= need <= the keys' mass.  On return sh.above and sh.nabove have grown by the
// mass and the number of the keys > t, and sh.qthr is t's own mass.  voc_threshold's radix select, 8 bits a pass from the
// top, with the digits' masses in place of their counts; all 8 passes run, so t is a key, not a prefix of one.  Every thread
// of the workgroup calls it; it ends behind a barrier.
template <typename Load>
EA_DEV uint64_t nuc_threshold(Load key_of, int n, float v0, float temperature, NucShared& sh) {
  const int lane = threadIdx.x & 63;
  uint64_t prefix = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    const uint64_t fixed = shift == 56 ? 0ull : ~0ull << (shift + 8);
    if (threadIdx.x < 256) { sh.hmass[threadIdx.x] = 0ull; sh.hcnt[threadIdx.x] = 0u; }
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += SMP_UNROLL * NUC_THREADS) {   // (whole waves enter an iteration; its loads go out first)
      uint64_t keys[SMP_UNROLL];
#pragma unroll
      for (int u = 0; u < SMP_UNROLL; ++u) {
        const int j = j0 + u * NUC_THREADS + (int)threadIdx.x;
        keys[u] = j < n ? key_of(j) : 0ull;
      }
#pragma unroll
      for (int u = 0; u < SMP_UNROLL; ++u) {
        const bool live = keys[u] != 0ull && (keys[u] & fixed) == prefix;
        const uint64_t q = live ? nuc_mass(nuc_arg(voc_key_value(keys[u]), v0, temperature)) : 0ull;
        nuc_hist_add(live, (uint32_t)(keys[u] >> shift) & 255u, q, sh.hmass, sh.hcnt, 2);
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {                               // lane l: digits 4 l .. 4 l + 3; above: the mass of larger digits
      uint64_t h[4], s = 0ull;
      uint32_t c[4], cs = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) { h[b] = sh.hmass[4 * lane + b]; c[b] = sh.hcnt[4 * lane + b]; s += h[b]; cs += c[b]; }
      uint64_t x = s;
      uint32_t cx = cs;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_down(x, o);
        const uint32_t ct = (uint32_t)__shfl_down((int)cx, o);
        if (lane + o < 64) { x += t; cx += ct; }
      }
      uint64_t above = x - s;
      uint32_t nabove = cx - cs;
      const uint64_t need = sh.need;
#pragma unroll
      for (int b = 3; b >= 0; --b) {
        if (above < need && need <= above + h[b]) {       // (one digit of one lane: the keys' mass reaches `need`)
          sh.digit = (uint32_t)(4 * lane + b); sh.need = need - above; sh.above += above; sh.nabove += nabove; sh.qthr = h[b];
        }
        above += h[b]; nabove += c[b];
      }
    }
    __syncthreads();
    prefix |= (uint64_t)sh.digit << shift;
  }
  return prefix;
}

// the mass of the chunk's columns that f keeps -> the chunk's block (f(column, value) -> the mass to count); whole waves
template <typename F>
EA_DEV void nuc_block_add(NucShared& sh, int block, int col0, const float (&v)[NUC_GROUP], uint32_t ok, F f) {
  uint64_t s = 0ull;
#pragma unroll
  for (int e = 0; e < NUC_GROUP; ++e)
    if (ok >> e & 1u) s += f(col0 + e, v[e]);
  s = nuc_wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)&sh.blk[block], (unsigned long long)s);
}

__global__ __launch_bounds__(NUC_THREADS) void ceva_vocab_nucleus_kernel(const DecNucleusP p) {
  __shared__ NucShared sh;
  const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int V = p.V, NB = (V - 1) / VOC_TILE + 1;
  const float* lrow = p.logits + (int64_t)m * p.ldl;
  const float T = p.temperature;
  const bool full = p.top_p >= 1.f;
  // 1. the maximum, from the tile candidates: the largest key is the pair that beats every other
  {
    const VocPick* cand = p.ws + (int64_t)m * NB;
    uint64_t best = 0ull;
#pragma unroll 4
    for (int j = threadIdx.x; j < NB; j += NUC_THREADS) {
      const VocPick c = cand[j];
      best = max(best, voc_key(c.v, c.i));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, (uint64_t)__shfl_xor(best, o));
    if (lane == 0) sh.wave[wave] = best;
  }
  for (int j = threadIdx.x; j < NUC_BUCKETS; j += NUC_THREADS) { sh.bmass[j] = 0ull; sh.bcnt[j] = 0u; }
  if (threadIdx.x < NUC_BLOCKS) sh.blk[threadIdx.x] = 0ull;
  if (threadIdx.x == 0) { sh.count = 0u; sh.bucket = 0u; sh.need = 1ull; sh.above = 0ull; sh.nabove = 0u; sh.digit = 0u; }
  __syncthreads();
  uint64_t top = sh.wave[0];
#pragma unroll
  for (int w = 1; w < NUC_THREADS / 64; ++w) top = max(top, sh.wave[w]);
  const int32_t i0 = min(max(voc_key_index(top), 0), V - 1);   // (a column of the row, come what may)
  const float v0 = lrow[i0];                              // (the stored logit's own bits: the candidate's)
  __syncthreads();                                        // (sh.wave is written again)
  if (!(v0 - v0 == 0.f)) {                                // (uniform) NaN or infinite: the greedy pick, kept = 0
    if (threadIdx.x == 0) {
      p.token[m] = (int64_t)i0;
      if (p.kept) p.kept[m] = 0;
      if (p.thr_idx) p.thr_idx[m] = i0;
      if (p.thr_val) p.thr_val[m] = v0;
      if (p.mass) { p.mass[2 * m] = 0; p.mass[2 * m + 1] = 0; }
      p.ctr[m] = p.ctr[m] + 1;                            // (this workgroup alone reads and writes ctr[m])
    }
    return;
  }
  const NucRow row = nuc_row(lrow, V);
  const int cpb = (row.chunks + NUC_BLOCKS - 1) / NUC_BLOCKS;   // chunks of a block
  // 2. pass A: the masses by bucket and by block; at top_p = 1 also the pair every other beats
  uint64_t worst = ~0ull;
  nuc_stream(row, 0, row.chunks, [&](int ch, int col0, const float (&v)[NUC_GROUP], uint32_t ok) {
    uint64_t s = 0ull;
#pragma unroll
    for (int e = 0; e < NUC_GROUP; ++e) {
      const bool on = ok >> e & 1u;
      const float x = nuc_arg(v[e], v0, T);
      const uint64_t q = on ? nuc_mass(x) : 0ull;
      nuc_hist_add(on, (uint32_t)nuc_bucket(x), q, sh.bmass, sh.bcnt, NUC_AGGREGATE);
      s += q;
      if (full && on) worst = min(worst, voc_key(v[e], col0 + e));
    }
    s = nuc_wave_sum(s);
    if (lane == 0 && s) atomicAdd((unsigned long long*)&sh.blk[ch / cpb], (unsigned long long)s);
  });
  if (full) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = min(worst, (uint64_t)__shfl_xor(worst, o));
    if (lane == 0) sh.wave[wave] = worst;
  }
  __syncthreads();
  // 3. Z, the target and the boundary bucket: one wave
  if (threadIdx.x < 64) {
    const uint64_t Z = nuc_wave_sum(sh.blk[2 * lane] + sh.blk[2 * lane + 1]);
    if (full) {
      uint64_t t = sh.wave[lane & 7];
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) t = min(t, (uint64_t)__shfl_xor(t, o));
      if (lane == 0) { sh.Z = Z; sh.ckept = Z; sh.thr = t; sh.nabove = (uint32_t)V - 1u; }
    } else {
      const uint64_t target = (uint64_t)ceil((double)p.top_p * (double)Z);   // 1 .. Z
      constexpr int PER = NUC_BUCKETS / 64;
      uint64_t h[PER], s = 0ull;
      uint32_t n[PER], ns = 0u;
#pragma unroll
      for (int b = 0; b < PER; ++b) { h[b] = sh.bmass[PER * lane + b]; n[b] = sh.bcnt[PER * lane + b]; s += h[b]; ns += n[b]; }
      uint64_t total;
      uint64_t above = nuc_wave_before(s, total), nabove = nuc_wave_before((uint64_t)ns, total);
      if (lane == 0) sh.Z = Z;
#pragma unroll
      for (int b = 0; b < PER; ++b) {
        if (above < target && target <= above + h[b]) {   // (one bucket of one lane)
          sh.bucket = (uint32_t)(PER * lane + b); sh.need = target - above; sh.above = above; sh.nabove = (uint32_t)nabove;
        }
        above += h[b]; nabove += n[b];
      }
    }
  }
  __syncthreads();
  if (!full) {
    // 4. pass B: the threshold pair inside the boundary bucket
    const int bb = (int)sh.bucket, nb = (int)sh.bcnt[bb];
    uint64_t t;
    if (nb <= NUC_POOL) {
      nuc_stream(row, 0, row.chunks, [&](int, int col0, const float (&v)[NUC_GROUP], uint32_t ok) {
#pragma unroll
        for (int e = 0; e < NUC_GROUP; ++e)
          if ((ok >> e & 1u) && nuc_bucket(nuc_arg(v[e], v0, T)) == bb) {
            const uint32_t at = atomicAdd(&sh.count, 1u);
            if (at < (uint32_t)NUC_POOL) sh.pool[at] = voc_key(v[e], col0 + e);
          }
      });
      __syncthreads();
      t = nuc_threshold([&](int j) { return sh.pool[j]; }, nb, v0, T, sh);
    } else {                                              // the bucket does not fit: the same select over the streamed row
      t = nuc_threshold([&](int j) { const float l = lrow[j]; return nuc_bucket(nuc_arg(l, v0, T)) == bb ? voc_key(l, j) : 0ull; },
                        V, v0, T, sh);
    }
    if (threadIdx.x < NUC_BLOCKS) sh.blk[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) { sh.thr = t; sh.ckept = sh.above + sh.qthr; }
    __syncthreads();
    // 5. pass C: the kept mass by block
    nuc_stream(row, 0, row.chunks, [&](int ch, int col0, const float (&v)[NUC_GROUP], uint32_t ok) {
      nuc_block_add(sh, ch / cpb, col0, v, ok,
                    [&](int col, float l) { return voc_key(l, col) >= t ? nuc_mass(nuc_arg(l, v0, T)) : 0ull; });
    });
    __syncthreads();
  }
  // 6. the draw, and the block that holds r: one wave
  const uint64_t thr = sh.thr;
  if (threadIdx.x < 64) {
    const int64_t n = p.ctr[m];
    const uint32_t word = philox4x32_10_word0(p.seed_lo, p.seed_hi, (uint32_t)(uint64_t)n, (uint32_t)((uint64_t)n >> 32),
                                              (uint32_t)p.sid[m], 0u);
    const uint64_t a = 2ull * (word >> 8) + 1ull, C = sh.ckept;
    const uint64_t r = ((a * (C >> 32)) << 7) + ((a * (C & 0xFFFFFFFFull)) >> 25);   // (a C) >> 25 of the 75-bit product: < C
    const uint64_t b0 = sh.blk[2 * lane], b1 = sh.blk[2 * lane + 1];
    uint64_t total;
    const uint64_t before = nuc_wave_before(b0 + b1, total);
    if (before <= r && r < before + b0) { sh.block = (uint32_t)(2 * lane); sh.rest = r - before; }
    else if (before + b0 <= r && r < before + b0 + b1) { sh.block = (uint32_t)(2 * lane + 1); sh.rest = r - before - b0; }
    if (lane == 0) {
      sh.token = voc_key_index(thr);                      // (never the answer: r < C = the blocks' sum)
      if (r >= total) { sh.block = 0u; sh.rest = 0ull; }
    }
  }
  __syncthreads();
  // 7. the walk through that block: the first kept column whose running kept mass exceeds r
  uint64_t rest = sh.rest;
  const int c_begin = (int)sh.block * cpb, c_end = min(c_begin + cpb, row.chunks);
  for (int ch = c_begin; ch < c_end; ++ch) {
    float v[NUC_GROUP];
    const int col0 = NUC_GROUP * (ch * NUC_THREADS + (int)threadIdx.x) - row.a;
    const uint32_t ok = nuc_load(row, ch * NUC_THREADS + (int)threadIdx.x, v);
    uint64_t q[NUC_GROUP], s = 0ull;
#pragma unroll
    for (int e = 0; e < NUC_GROUP; ++e) {
      q[e] = (ok >> e & 1u) && voc_key(v[e], col0 + e) >= thr ? nuc_mass(nuc_arg(v[e], v0, T)) : 0ull;
      s += q[e];
    }
    uint64_t total;
    uint64_t before = nuc_wave_before(s, total);
    if (lane == 0) sh.wave[wave] = total;
    __syncthreads();
    uint64_t chunk = 0ull;
#pragma unroll
    for (int w = 0; w < NUC_THREADS / 64; ++w) {
      if (w < wave) before += sh.wave[w];
      chunk += sh.wave[w];
    }
    if (rest < chunk) {                                   // (uniform) one thread holds it
      if (before <= rest && rest < before + s) {
        int32_t token = col0;
#pragma unroll
        for (int e = NUC_GROUP - 1; e >= 0; --e) {        // the first column whose inclusive mass exceeds rest
          uint64_t upto = before;
#pragma unroll
          for (int i = 0; i <= e; ++i) upto += q[i];
          if (q[e] && upto > rest) token = col0 + e;
        }
        sh.token = token;
      }
      break;
    }
    rest -= chunk;
    __syncthreads();                                      // (sh.wave is written again)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    p.token[m] = (int64_t)min(max(sh.token, 0), V - 1);
    const int32_t ti = min(max(voc_key_index(thr), 0), V - 1);
    if (p.kept) p.kept[m] = (int32_t)(sh.nabove + 1u);
    if (p.thr_idx) p.thr_idx[m] = ti;
    if (p.thr_val) p.thr_val[m] = lrow[ti];               // (the stored logit's own bits: the key has folded -0)
    if (p.mass) { p.mass[2 * m] = (int64_t)sh.ckept; p.mass[2 * m + 1] = (int64_t)sh.Z; }
    p.ctr[m] = p.ctr[m] + 1;                              // (this workgroup alone reads and writes ctr[m])
  }
}

}  // namespace

int ceva_vocab_nucleus_launch(const DecNucleusP& s, int M, hipStream_t st) {
  hipLaunchKernelGGL(ceva_vocab_nucleus_kernel, dim3((unsigned)M), dim3(NUC_THREADS), 0, st, s);
  return (int)hipGetLastError();
}

}  // namespace ea
