// ea_softmax_decode.hip -- decoding steps of causal softmax attention against a static KV cache: append, attn_split, attn_mm.
// (merge and advance are the causal EVA step's launches, ea_ceva_decode.hip: the workspace layout and the counter are shared.)
//
// The cache is k, v [B, H, cap, D] rows of bf16 / fp16 (the two halves of kv [B, 2, H, cap, D]: a head's keys are one
// contiguous stream, its values another), pad [B, cap] flags and the token count *pos in device memory.  A step of T tokens is
//   append      rows *pos .. *pos + T - 1 of k, v and pad from the step's projection buffer
//   attn        out[t] = softmax(s q_t . k_j : j <= *pos + t, j not padded) v,  t < T
//   advance     *pos += T
// and every kernel reads *pos itself, so a captured step replays.  A step with *pos + T > cap writes no cache byte, sets
// *status, delivers NaN rows and leaves *pos alone.  A query whose visible keys are all padded has an empty softmax: NaN.
//
// attn_split (T <= 8: the token step).  The step reads every key and value row of the context once and multiplies each by a
// handful of queries: it is bound by memory, so it runs on the vector ALUs and is shaped for loads in flight.  Grid
// (parts, B H), four waves; wave s of part p owns the 64-key tiles 4 p + s, + 4 parts, .. of [0, *pos + T).  A key row is D / 8
// 16-byte pieces; G = D / 8 adjacent lanes hold one row, so a wave's load instruction fetches 64 / G consecutive rows, 1 KB
// contiguous.  A lane keeps its 8 channels of every query (fp32, times s log2 e) and of every accumulator in registers: a
// score is 8 FMAs and a DPP sum over the G lanes, with no LDS.  Four rows per lane form a batch: one maximum, one rescale,
// four exp2.  The K, V pieces and flags of batch n + 1 are requested before batch n is multiplied.  Each group of G lanes runs
// its own online softmax over the rows it meets; they are folded once at the end, over the wave by DPP / permlane sums and
// over the four waves through LDS.  parts == 1: that result is normalised and stored.  parts > 1: it goes to the workspace
// unnormalised, as (acc[D], max in natural log, sum), and ea_ceva_sdecode_merge's kernel folds the parts.
//
// attn_mm (any T; used above 8: prompts).  One workgroup per 64 step rows, 16 per wave, the heaviest first.  K and V tiles of 64
// keys go through double-buffered LDS, tile j + 1 requested before the MFMAs of tile j.  S^T = K.Q^T and O^T = V^T.P^T on
// mfma_f32_16x16x32, V read with ds_read_b64_tr_b16; the online softmax is fp32, P is rounded to the dtype for P.V and the
// row sum is that of the unrounded weights.  A block's keys are [0, *pos + its last row]; a wave skips the tiles past its own
// last query and compares key against query only in the tiles that pass its first query.  Step rows, not absolute positions,
// are what is grouped by 16, so *pos is free.
//
// Per-sequence counts (SEQ, a compile-time flag of the three kernels, chosen by ntok != null; the shared-count instances are
// the code they were): pos, status and ntok are [B].  Of the step's T positions row b takes the n_b before its first flag in
// the step's pad columns (append finds n_b and writes ntok[b]); nothing is stored for the others and their out rows are zero;
// query t < n_b sees keys j <= pos[b] + t; a row with pos[b] + n_b > cap alone writes nothing, gets status[b] = 1 and NaN rows,
// and keeps pos[b].  Step<true, SEQ> (ea_ceva_decode.h) carries these rules; a workgroup has one b, so every exit is uniform.
// A row's arithmetic is what it is decoded alone: its tiles, its wave and part assignment and its order of summation depend on
// (pos[b], n_b) only.
#include "ea_softmax_decode.h"
#include "ea_lm_frag.h"

namespace ea {

namespace {

constexpr int SD_NT = 256;

EA_DEV const char* sd_row(const DecT& t, int b, int h, int n) {
  return t.p + ((size_t)b * t.sb + (size_t)h * t.sh + (size_t)n * t.sn) * 2;
}

// rows lo .. hi - 1 of the output of (b, h) = x, by the whole workgroup
template <typename E>
EA_DEV void sd_fill(const SdecP& p, int b, int h, int lo, int hi, float x) {
  const uint32_t w = pack2<E>(x, x);
  const int cpr = p.D / 8;
  for (int idx = (int)threadIdx.x; idx < (hi - lo) * cpr; idx += SD_NT) {
    const int i = idx / cpr, c = idx - i * cpr;
    stg16(const_cast<char*>(sd_row(p.o, b, h, lo + i)) + c * 16, u32x4{w, w, w, w});
  }
}

// the T output rows of (b, h) = NaN: a step that does not fit
template <typename E>
EA_DEV void sd_refuse(const SdecP& p, int b, int h) {
  const uint32_t w = pack2<E>(__builtin_nanf(""), __builtin_nanf(""));
  const int cpr = p.D / 8;
  for (int idx = (int)threadIdx.x; idx < p.T * cpr; idx += SD_NT) {
    const int i = idx / cpr, c = idx - i * cpr;
    stg16(const_cast<char*>(sd_row(p.o, b, h, i)) + c * 16, u32x4{w, w, w, w});
  }
}

// The first flagged position of a row of T step flags (T when there is none): n_b.  Wave w takes the 16-byte loads
// w 64 + lane, + 256, .. of the aligned middle of the row -- 1 KB per wave and load -- and stops at its first load with a
// flag in it (a ballot: the exit is uniform over the wave, and what it has not read lies further on); the row's two ends,
// up to 15 bytes each (a row of [B, T] starts at any address), go byte by byte.  Then a minimum over the wave by lane
// exchanges and over the four waves through LDS (red: 4 ints).
EA_DEV int sd_first_flag(const uint8_t* f, int T, int* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = min(T, (int)((16 - ((uintptr_t)f & 15)) & 15));
  const int nvec = (T - head) / 16, tail = head + nvec * 16;
  int first = T;
  if (tid < head && f[tid]) first = tid;
  if (tid < T - tail && f[tail + tid]) first = min(first, tail + tid);
  for (int i0 = wave * 64; i0 < nvec; i0 += SD_NT) {                  // (i0 and nvec are uniform over the wave)
    const int i = i0 + lane;
    int at = 16;
    if (i < nvec) {
      const u32x4 u = ldg16(f + head + (size_t)i * 16);
#pragma unroll
      for (int c = 3; c >= 0; --c)
        if (u[c]) at = c * 4 + (__builtin_ctz(u[c]) >> 3);
    }
    if (at < 16) first = min(first, head + i * 16 + at);
    if (__ballot(at < 16)) break;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
  if (lane == 0) red[wave] = first;
  __syncthreads();
  return min(min(red[0], red[1]), min(red[2], red[3]));
}

// ---- append: one workgroup per (step token, b) ----
// SEQ: every workgroup of row b finds n_b from the row's flags itself (sd_first_flag: one 16-byte load per thread up to 4096
// step tokens), so none waits for another and the step needs no launch in front of it; the one of t = 0 publishes it, also
// when the row does not fit -- the attention kernels and advance decide that from pos[b] + ntok[b] as this kernel does.
// The tokens it stores are unflagged by construction: their pad flag is 0.
template <bool SEQ>
__global__ __launch_bounds__(SD_NT) void sdec_append_kernel(const SdecAppP p) {
  const int t = (int)blockIdx.x, b = (int)blockIdx.y, tid = threadIdx.x;
  int own = p.T;
  if constexpr (SEQ) {
    __shared__ int red[SD_NT / 64];
    if (p.src_pad) own = sd_first_flag(p.src_pad + (size_t)b * p.T, p.T, red);
    if (t == 0 && tid == 0) p.ntok[b] = own;
  }
  const Step<true, SEQ> step(p.pos, b, own);
  const int t0 = step.t0;
  if (!step.fits(p.T, p.cap)) {
    if (t == 0 && (SEQ || b == 0) && tid == 0) p.status[SEQ ? b : 0] = 1;
    return;
  }
  if (SEQ && t >= own) return;                     // (uniform: one b per workgroup)
  const int cpr = p.D / 8, n = p.H * cpr;          // 16-byte pieces of a head's row, of a token's K (or V) row
  const char* src = p.src + ((size_t)t * p.B + b) * 3 * n * 16;
  for (int idx = tid; idx < 2 * n; idx += SD_NT) {
    const int kv = idx / n, hc = idx - kv * n, h = hc / cpr, c = hc - h * cpr;
    const u32x4 x = ldg16(src + ((size_t)(1 + kv) * n + hc) * 16);
    stg16(const_cast<char*>(sd_row(kv ? p.v : p.k, b, h, t0 + t)) + c * 16, x);
  }
  if (tid == 0) p.pad[(size_t)b * p.cap + t0 + t] = !SEQ && p.src_pad ? (p.src_pad[(size_t)b * p.T + t] ? 1 : 0) : 0;
}

// ---- attn_split ----
template <int U> struct SdBatch {                  // U rows of a lane: its 16-byte pieces of K and V, and the rows' pad flags
  u32x4 k[U], v[U];
  uint32_t f[U];
};

// SEQ: t0 = pos[b], the row's nq = ntok[b] queries against its own tiles [0, pos[b] + nq); queries nq .. T - 1 are neither loaded
// nor accumulated (the loops over t end at nq: a uniform branch) and their out rows are zero.  Part 0 writes the zero and the
// NaN rows whatever `parts` is: ceva_merge_kernel leaves both alone and reads the workspace rows of t < nq only, which every
// part writes -- (max = -inf, sum = 0) where it has no tile of this row.
template <typename E, int D, int TQ, bool SEQ>
__global__ __launch_bounds__(SD_NT) void sdec_split_kernel(const SdecP p) {
  constexpr int G = D / 8, R = 64 / G, U = 4, NB = SDEC_TILE / (R * U);      // lanes per row, rows per load, batches per tile
  __shared__ __attribute__((aligned(16))) float mo[4][TQ][D];
  __shared__ float ml[4][TQ][2];
  const int tid = threadIdx.x, lane = tid & 63, c = lane % G, r = lane / G;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int part = (int)blockIdx.x, b = (int)blockIdx.y / p.H, h = (int)blockIdx.y - b * p.H;
  const Step<true, SEQ> step(p.pos, b, SEQ ? p.ntok[b] : 0);
  const int t0 = step.t0, nq = step.n(p.T);        // (one value for every thread of the workgroup: every exit is uniform)
  if (!step.fits(p.T, p.cap)) {
    if (part == 0) sd_refuse<E>(p, b, h);
    return;
  }
  if constexpr (SEQ) {
    if (part == 0) sd_fill<E>(p, b, h, nq, p.T, 0.f);
    if (nq == 0) return;                           // a row that sits the step out
  }
  const int kend = t0 + nq, ntiles = (kend + SDEC_TILE - 1) / SDEC_TILE;
  const float scale2 = p.scale * LOG2E;
  float q[TQ][8], m[TQ], l[TQ], acc[TQ][8];
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
    const bool live = t < nq;
    const u32x4 w = ldg16(sd_row(p.q, b, h, live ? t : 0) + c * 16);
    unpack8<E>(live ? w : u32x4{0u, 0u, 0u, 0u}, q[t]);
    m[t] = -INFINITY; l[t] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { q[t][e] *= scale2; acc[t][e] = 0.f; }
  }
  // the wave's tiles w, w + stride, ..; batch n of them: rows j0 + u R + r, u < U, of tile w + (n / NB) stride
  const int w = part * 4 + wave, stride = 4 * p.parts;
  const int nb = w < ntiles ? (ntiles - w + stride - 1) / stride * NB : 0;
  const char* kb = sd_row(p.k, b, h, 0) + c * 16;
  const char* vb = sd_row(p.v, b, h, 0) + c * 16;
  const uint8_t* fb = p.pad + (size_t)b * p.cap;
  auto first_row = [&](int n) { return (w + (n / NB) * stride) * SDEC_TILE + (n % NB) * (U * R) + r; };
  auto fetch = [&](int n, SdBatch<U>& x) {         // rows past the step's end: the last row's bytes, masked when consumed
    const int j0 = first_row(n);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = min(j0 + u * R, kend - 1);
      x.k[u] = ldg16(kb + (size_t)j * p.k.sn * 2);
      x.v[u] = ldg16(vb + (size_t)j * p.v.sn * 2);
      x.f[u] = fb[j];
    }
  };
  auto consume = [&](int n, const SdBatch<U>& x) {
    const int j0 = first_row(n);
    float s[TQ][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      unpack8<E>(x.k[u], kf);
      const int j = j0 + u * R;
      const bool dead = j >= kend || x.f[u] != 0;
#pragma unroll
      for (int t = 0; t < TQ; ++t) {
        if (SEQ && t >= nq) break;
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(q[t][e], kf[e], d);
        d = group_sum<G>(d);
        s[t][u] = (dead || j > t0 + t) ? -INFINITY : d;
      }
    }
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
      if (SEQ && t >= nq) break;
      float mb = s[t][0];
#pragma unroll
      for (int u = 1; u < U; ++u) mb = fmaxf(mb, s[t][u]);
      const float mnew = fmaxf(m[t], mb);
      const float msafe = mnew == -INFINITY ? 0.f : mnew;
      const float alpha = fast_exp2(m[t] - msafe);
      m[t] = mnew;
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[t][u] = fast_exp2(s[t][u] - msafe);
        ps += s[t][u];
      }
      l[t] = l[t] * alpha + ps;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[t][e] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
      unpack8<E>(x.v[u], vf);
#pragma unroll
      for (int t = 0; t < TQ; ++t) {
        if (SEQ && t >= nq) break;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[t][e] = fmaf(s[t][u], vf[e], acc[t][e]);
      }
    }
  };
  SdBatch<U> xa, xb;
  if (nb > 0) fetch(0, xa);
  for (int n = 0; n < nb; n += 2) {                // (nb is uniform over the wave)
    if (n + 1 < nb) fetch(n + 1, xb);
    consume(n, xa);
    if (n + 1 >= nb) break;
    if (n + 2 < nb) fetch(n + 2, xa);
    consume(n + 1, xb);
  }
  // the wave's R row groups folded: lanes with equal c hold the same channels
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
    const float mx = stride_max<G>(m[t]);
    const float f = fast_exp2(m[t] - (mx == -INFINITY ? 0.f : mx));
    const float lt = stride_sum<G>(l[t] * f);
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = stride_sum<G>(acc[t][e] * f);
    if (r == 0) {
      *reinterpret_cast<f32x4*>(&mo[wave][t][c * 8]) = f32x4{a[0], a[1], a[2], a[3]};
      *reinterpret_cast<f32x4*>(&mo[wave][t][c * 8 + 4]) = f32x4{a[4], a[5], a[6], a[7]};
      if (c == 0) { ml[wave][t][0] = mx; ml[wave][t][1] = lt; }
    }
  }
  __syncthreads();
  // ... and the four waves: thread = (query, four channels)
  constexpr int G4 = D / 4;
  const int t = tid / G4, c4 = (tid - t * G4) * 4;
  if (t >= nq || t >= TQ) return;
  float mx = ml[0][t][0];
#pragma unroll
  for (int v = 1; v < 4; ++v) mx = fmaxf(mx, ml[v][t][0]);
  const float msafe = mx == -INFINITY ? 0.f : mx;
  float lt = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float f = fast_exp2(ml[v][t][0] - msafe);
    lt += f * ml[v][t][1];
    o += f * *reinterpret_cast<const f32x4*>(&mo[v][t][c4]);
  }
  if (p.parts > 1) {
    float* dst = p.ws + (((size_t)blockIdx.y * SDEC_QMAX + t) * p.parts + part) * (D + 4);
    *reinterpret_cast<f32x4*>(dst + c4) = o;
    if (c4 == 0) *reinterpret_cast<f32x4*>(dst + D) = f32x4{mx * LN2, lt, 0.f, 0.f};
  } else {
    const float inv = 1.f / lt;
    const u32x2 w2 = {pack2<E>(o[0] * inv, o[1] * inv), pack2<E>(o[2] * inv, o[3] * inv)};
    *reinterpret_cast<u32x2*>(const_cast<char*>(sd_row(p.o, b, h, t)) + c4 * 2) = w2;
  }
}

// ---- attn_mm ----
// SEQ: t0 = pos[b] and the row has nq = ntok[b] of the step's T rows.  The block first zeroes its rows from nq on -- all of
// them when base >= nq, and then it exits before any tile is staged -- its keys end at pos[b] + min(nq, base + 64), a wave
// whose 16 rows start at or past nq does no MFMA work, and the final store is guarded by i < nq.  The grid stays qt-descending:
// heaviest-first by a row's true work (pos[b] + nq) would need a device-side sort of (qt, b), which is not built.
template <typename E, int D, bool SEQ>
__global__ __launch_bounds__(SD_NT, 2) void sdec_mm_kernel(const SdecP p) {
  constexpr int ROWB = D * 2, KS = D / 32, DT = D / 16, DQ = D / 4, TB = SDEC_TILE * ROWB;
  constexpr int CPR = D / 8, NCH = SDEC_TILE * CPR / SD_NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];          // [2 stages][K tile | V tile], then the key flags
  uint8_t* kflag = reinterpret_cast<uint8_t*>(smem + 4 * TB);          // [2][64]: the key is padded or past the block's range
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  typename LaneOffSel<D>::type lo;
  lo.init(lane);
  const int BH = p.B * p.H, nqt = (p.T + SDEC_TILE - 1) / SDEC_TILE;
  const int qt = nqt - 1 - (int)(blockIdx.x / BH), bh = (int)(blockIdx.x % BH);
  const int b = bh / p.H, h = bh - b * p.H;
  const Step<true, SEQ> step(p.pos, b, SEQ ? p.ntok[b] : 0);
  const int t0 = step.t0, nq = step.n(p.T);                            // (uniform over the workgroup: one b)
  if (!step.fits(p.T, p.cap)) {
    if (qt == 0) sd_refuse<E>(p, b, h);
    return;
  }
  const int base = qt * SDEC_TILE;                                     // the block's first step row
  if constexpr (SEQ) {
    sd_fill<E>(p, b, h, max(base, nq), min(p.T, base + SDEC_TILE), 0.f);
    if (base >= nq) return;
  }
  const int kend = t0 + min(nq, base + SDEC_TILE);                     // its keys are [0, kend)
  const int nt = (kend + SDEC_TILE - 1) / SDEC_TILE;
  const int ia = base + wave * 16;                                     // the wave's 16 step rows
  const bool active = ia < nq;
  const int i = ia + li;
  const bool qv = i < nq;
  const int tq = t0 + i;
  const int wave_lo = t0 + ia, wave_hi = t0 + min(ia + 16, nq) - 1;    // positions of its first and last query
  typename E::x8 qf[KS];
  load_frag<E, KS>(qf, sd_row(p.q, b, h, qv ? i : 0), g, qv);
  const char* kb = sd_row(p.k, b, h, 0);
  const char* vb = sd_row(p.v, b, h, 0);
  const uint8_t* fb = p.pad + (size_t)b * p.cap;
  const float scale2 = p.scale * LOG2E;

  float m = -INFINITY, lsum = 0.f;
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ck[NCH], cv[NCH];
  uint8_t kf = 0;                                  // threads < 64: the flag of key row tid of the tile in flight
  auto fetch_k = [&](int j) {
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      const int idx = tid + n * SD_NT, r = idx / CPR, c = idx - r * CPR, at = j * SDEC_TILE + r;
      const bool ok = at < kend;
      const u32x4 x = ldg16(kb + (size_t)(ok ? at : 0) * p.k.sn * 2 + c * 16);
      ck[n] = ok ? x : u32x4{0u, 0u, 0u, 0u};
    }
    if (tid < SDEC_TILE) {
      const int at = j * SDEC_TILE + tid;
      kf = at >= kend || fb[at < kend ? at : 0];
    }
  };
  auto fetch_v = [&](int j) {
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      const int idx = tid + n * SD_NT, r = idx / CPR, c = idx - r * CPR, at = j * SDEC_TILE + r;
      const bool ok = at < kend;
      const u32x4 x = ldg16(vb + (size_t)(ok ? at : 0) * p.v.sn * 2 + c * 16);
      cv[n] = ok ? x : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto park_k = [&](int j) {
    char* dst = smem + (j & 1) * 2 * TB;
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      const int idx = tid + n * SD_NT, r = idx / CPR, c = idx - r * CPR;
      sts16(dst + TileL<D>::off(r, c), ck[n]);
    }
    if (tid < SDEC_TILE) kflag[(j & 1) * SDEC_TILE + tid] = kf;
  };
  auto park_v = [&](int j) {
    char* dst = smem + (j & 1) * 2 * TB + TB;
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      const int idx = tid + n * SD_NT, r = idx / CPR, c = idx - r * CPR;
      sts16(dst + TileL<D>::off(r, c), cv[n]);
    }
  };
  fetch_k(0);
  fetch_v(0);
  park_k(0);
  park_v(0);
  __syncthreads();
  for (int j = 0; j < nt; ++j) {
    const bool more = j + 1 < nt;
    if (more) {
      fetch_k(j + 1);
      fetch_v(j + 1);
    }
    const char* Ks = smem + (j & 1) * 2 * TB;
    const char* Vs = Ks + TB;
    const int r0 = j * SDEC_TILE;
    const bool work = active && r0 <= wave_hi;                         // (uniform over the wave)
    uint32_t pw[4][2];
    if (work) {                                                        // S^T, masks, online softmax -> P^T rounded to E
      const bool full = r0 + SDEC_TILE - 1 <= wave_lo;                 // every key of the tile is before every query
      f32x4 s[4];
      float mloc = -INFINITY;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc = E::mma(as_x8<E>(lds16(Ks + tt * 16 * ROWB + lo.plain[ks])), qf[ks], acc);
        const int c0 = r0 + tt * 16 + 4 * g;                           // the lane's keys c0 .. c0 + 3
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(kflag + (j & 1) * SDEC_TILE + tt * 16 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool dead = ((f4 >> (8 * r)) & 0xffu) || (!full && c0 + r > tq);
          const float x = dead ? -INFINITY : acc[r] * scale2;
          acc[r] = x;
          mloc = fmaxf(mloc, x);
        }
        s[tt] = acc;
      }
      mloc = quad_max(mloc);
      const float mnew = fmaxf(m, mloc);
      const float msafe = mnew == -INFINITY ? 0.f : mnew;
      const float alpha = fast_exp2(m - msafe);
      m = mnew;
      float psum = 0.f;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        float pv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pv[r] = fast_exp2(s[tt][r] - msafe);
          psum += pv[r];                                               // the normaliser sums the unrounded weights
        }
        pw[tt][0] = pack2<E>(pv[0], pv[1]);
        pw[tt][1] = pack2<E>(pv[2], pv[3]);
      }
      lsum = lsum * alpha + psum;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
    }
    if (more) park_k(j + 1);
    if (work) {                                                        // O^T += V^T.P^T
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const typename E::x8 pf = as_x8<E>(u32x4{pw[2 * kk][0], pw[2 * kk][1], pw[2 * kk + 1][0], pw[2 * kk + 1][1]});
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const u32x2 lo_ = E::tr4(Vs + (2 * kk) * 16 * ROWB + lo.tr[dt]);
          const u32x2 hi_ = E::tr4(Vs + (2 * kk + 1) * 16 * ROWB + lo.tr[dt]);
          o[dt] = E::mma(as_x8<E>(lo_, hi_), pf, o[dt]);
        }
      }
    }
    if (more) park_v(j + 1);
    __syncthreads();
  }

  // lane = query li, channels DQ g .. DQ g + DQ - 1: divided by the row sum, rounded once, 16 bytes per store
  if (!active) return;                                                 // (uniform over the wave)
  const float inv = 1.f / quad_sum(lsum);
  float f[DQ];
  if constexpr (TileL<D>::NEWTR) {
    quad_transpose_f32(o, f);
  } else {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) f[4 * dt + r] = o[dt][r];
  }
  if (qv) {
    char* dst = const_cast<char*>(sd_row(p.o, b, h, i)) + DQ * g * 2;
#pragma unroll
    for (int c = 0; c < DQ / 8; ++c) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = f[8 * c + e] * inv;
      stg16(dst + c * 16, pack8<E>(x));
    }
  }
}

using SdKernel = void (*)(const SdecP);

template <typename E, int D, bool SEQ> SdKernel split_of(int T) {
  return T <= 1   ? sdec_split_kernel<E, D, 1, SEQ>
         : T <= 2 ? sdec_split_kernel<E, D, 2, SEQ>
         : T <= 4 ? sdec_split_kernel<E, D, 4, SEQ>
                  : sdec_split_kernel<E, D, 8, SEQ>;
}
template <typename E, bool SEQ> SdKernel split_of(int D, int T) {
  return D == 32 ? split_of<E, 32, SEQ>(T) : D == 64 ? split_of<E, 64, SEQ>(T) : split_of<E, 128, SEQ>(T);
}
template <typename E> SdKernel split_of(int D, int T, bool seq) { return seq ? split_of<E, true>(D, T) : split_of<E, false>(D, T); }
template <typename E, bool SEQ> SdKernel mm_of(int D) {
  return D == 32 ? sdec_mm_kernel<E, 32, SEQ> : D == 64 ? sdec_mm_kernel<E, 64, SEQ> : sdec_mm_kernel<E, 128, SEQ>;
}
template <typename E> SdKernel mm_of(int D, bool seq) { return seq ? mm_of<E, true>(D) : mm_of<E, false>(D); }

bool sd_geom_ok(const SdecP& p) {
  return (p.dtype == EA_BF16 || p.dtype == EA_F16) && (p.D == 32 || p.D == 64 || p.D == 128);
}

}  // namespace

// (The C entry points have checked the pointers, the views and the geometry.)  SEQ follows the state: p.ntok != null.
int softmax_sdecode_append(const SdecAppP& p, hipStream_t st) {
  void (*kernel)(const SdecAppP) = p.ntok ? sdec_append_kernel<true> : sdec_append_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.T, (unsigned)p.B), dim3(SD_NT), 0, st, p);
  return (int)hipGetLastError();
}

int softmax_sdecode_attn_split(const SdecP& p, hipStream_t st) {
  if (!p.pos || !p.pad || p.parts < 1 || p.parts > 64 || p.T < 1 || p.T > SDEC_QMAX || (p.parts > 1 && !p.ws)) return EA_E_BADARG;
  if (!sd_geom_ok(p)) return EA_E_UNSUPPORTED;
  const SdKernel kernel = p.dtype == EA_BF16 ? split_of<BF16>(p.D, p.T, p.ntok != nullptr) : split_of<F16>(p.D, p.T, p.ntok != nullptr);
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.parts, (unsigned)(p.B * p.H)), dim3(SD_NT), 0, st, p);
  return (int)hipGetLastError();
}

int softmax_sdecode_attn_mm(const SdecP& p, hipStream_t st) {
  if (!p.pos || !p.pad || p.T < 1) return EA_E_BADARG;
  if (!sd_geom_ok(p)) return EA_E_UNSUPPORTED;
  const SdKernel kernel = p.dtype == EA_BF16 ? mm_of<BF16>(p.D, p.ntok != nullptr) : mm_of<F16>(p.D, p.ntok != nullptr);
  const size_t lds = (size_t)4 * SDEC_TILE * p.D * 2 + 2 * SDEC_TILE;
  if (const int e = ea_lds_limit(reinterpret_cast<const void*>(kernel), lds)) return e;
  const int nqt = (p.T + SDEC_TILE - 1) / SDEC_TILE;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(nqt * p.B * p.H)), dim3(SD_NT), lds, st, p);
  return (int)hipGetLastError();
}

}  // namespace ea
