// ea_ceva_decode.hip -- incremental decoding of causal EVA: the landmarks of the chunks a step completes, and the outputs of
// the step's query tokens, each in ONE launch (CausalEVAttention._decode).
//
// Decoding is pinned by prefix consistency with the full-sequence causal path (_f32.causal_eva_core): the output of token t
// equals row t of forward() on tokens 0..t.  Both kernels restate that path's arithmetic row for row, in fp32 throughout,
// on rows of any I/O type (bf16, fp16, fp32); with fp32 rows nothing is rounded to 16 bits.
//
// ceva_close_kernel, one workgroup per (chunk, b, h):
//   qm, km = (1/r) sum of the chunk's unpadded q / k rows                            (GatherMeanFn)
//   rk = mu_k(km), mu = mu_q(qm) + rk; mu_* = Linear [+ LayerNorm(eps 1e-5)]          (the module's mu networks)
//   beta = sum_j softmax_j(s mu.k_j - s |k_j|^2 / 2; padded: -5e4, zero value) v_j  (GatherAttnFn, knorm, zero_masked_v)
// ceva_attn_kernel, one workgroup per (window block touched by the step, b, h); for token t of block bk = t / w:
//   local slot j < w + e is token bk w - e + j: masked (-5e4) when absent, padded, after t, or t itself is padded;
//   otherwise s q.k + bias[t - bk w, j];  landmark c (rf_k_bar, beta) is a column iff c < t / r;
//   out = one softmax over both column sets, times [v ; beta].
// The keys are streamed in 64-column tiles (local tiles first, then landmark tiles), one key per lane for the logits and
// G = D / 4 lanes per value row for P.V.  A wave owns up to QPW queries; when the step holds fewer query groups than
// waves, the waves split the tiles of each group and merge their (max, sum, acc) partials in LDS.
//
// A decoding step is append -> close -> attn -> advance over a state (efficient_attention/_ceva_decode.py), and the state
// sets two switches, both template flags of the kernels, so that every combination compiles to its own straight-line code:
//   DEV  (p.pos != null): where the step starts.  false: t0 is a kernel argument, the host has grown the cache, written the
//        step's rows and decided which chunks close (ea_ceva_decode_*: close and attn only).  true: t0 = *p.pos in device
//        memory, so that a captured step replays at the right position (ea_ceva_sdecode_*): ceva_append_kernel writes the
//        step's rows first, ceva_advance_kernel moves *pos last, the grids hold the most a step of T tokens can need and a
//        workgroup the step does not need exits at once.  `Step` reads the start; nothing else reads *pos.
//   RING (p.ring != 0, with DEV): how a token index becomes a row of q / k / v / pad.  false: token n is row n of cap rows.
//        true: slot n % ring of a ring of p.ring rows, the landmark rows staying linear.  ring is a multiple of w (so of r)
//        and at least w + e + T, so a window block and a chunk never straddle the end of the ring, a local window wraps at
//        most once, and the rows a step appends overwrite only tokens older than the earliest one it reads.  Only addresses
//        change: every test on a token (present, causal, capacity) stays on token indices, and the arithmetic and its order
//        are the linear step's.  `Rows` owns the mapping; no kernel spells it.
#include "ea_common.h"
#include "ea_ceva_decode.h"

namespace ea {

namespace {

constexpr int NT = 256, NW = 4;        // four waves
constexpr int QPW = 8;                 // queries per wave
constexpr int KT = 64;                 // key columns per tile (one per lane)

// element access: 8 or 4 consecutive values of a row as floats; 16-byte loads where the type allows
template <typename E> struct Io;
template <> struct Io<float> {
  static EA_DEV void ld8(const char* p, float* x) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 16);
    x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3]; x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
  }
  static EA_DEV f32x4 ld4(const char* p) { return *reinterpret_cast<const f32x4*>(p); }
  static EA_DEV float ld1(const char* p) { return *reinterpret_cast<const float*>(p); }
  static EA_DEV void st4(char* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
  static constexpr int SZ = 4;
};
template <typename H> struct Io16 {
  static EA_DEV void ld8(const char* p, float* x) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = H::to_f((uint16_t)(u[i] & 0xffffu));
      x[2 * i + 1] = H::to_f((uint16_t)(u[i] >> 16));
    }
  }
  static EA_DEV f32x4 ld4(const char* p) {
    const u32x2 u = *reinterpret_cast<const u32x2*>(p);
    return f32x4{H::to_f((uint16_t)(u[0] & 0xffffu)), H::to_f((uint16_t)(u[0] >> 16)),
                 H::to_f((uint16_t)(u[1] & 0xffffu)), H::to_f((uint16_t)(u[1] >> 16))};
  }
  static EA_DEV float ld1(const char* p) { return H::to_f(*reinterpret_cast<const uint16_t*>(p)); }
  static EA_DEV void st4(char* p, f32x4 v) { *reinterpret_cast<u32x2*>(p) = u32x2{pack2<H>(v[0], v[1]), pack2<H>(v[2], v[3])}; }
  static constexpr int SZ = 2;
};
template <> struct Io<BF16> : Io16<BF16> {};
template <> struct Io<F16> : Io16<F16> {};

template <typename E> EA_DEV const char* row(const DecT& t, int b, int h, int n) {
  return t.p + ((size_t)b * t.sb + (size_t)h * t.sh + (size_t)n * t.sn) * Io<E>::SZ;
}

// Token index -> row of q / k / v / pad.  RING = false: the identity, every member folds away.  RING = true: slot
// n % ring.  A kernel reduces once (`slot` of its first token) and then walks: a run of fewer than `ring` rows that starts
// at a slot passes the end of the ring at most once (`wrap`), and one that starts up to `ring` rows before a slot falls
// before slot 0 at most once (`unwrap`).
template <bool RING> struct Rows {
  int ring;
  EA_DEV int slot(int n) const { return RING ? n % ring : n; }                     // n >= 0
  EA_DEV size_t slot(int n, int j) const { return RING ? (size_t)((n + j) % ring) : (size_t)n + j; }
  EA_DEV int wrap(int s) const { return RING ? s - (s >= ring ? ring : 0) : s; }   // 0 <= s < 2 ring
  EA_DEV int unwrap(int s) const { return RING && s < 0 ? s + ring : s; }          // -ring <= s < ring
  EA_DEV int len(int cap) const { return RING ? ring : cap; }                      // rows per batch element (of pad)
};

// Where the step starts, and whether it fits the cache.  DEV = false: the kernel argument (the host has checked the
// capacity: `fits` is true and folds away).  DEV = true: the token count in device memory -- one value for every thread of
// the step's launches up to advance, so every exit decided from it is uniform.
template <bool DEV> struct Step {
  int t0;
  EA_DEV Step(const int32_t* pos, int arg_t0) : t0(DEV ? *pos : arg_t0) {}
  EA_DEV bool fits(int T, int cap) const { return !DEV || t0 + T <= cap; }
};

EA_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// s[i] += q_i . row over D, the row read by this lane alone (8 values per load), q_i broadcast from LDS
template <typename E, int D>
EA_DEV void dot_rows(const char* rp, const float (*qs)[D], float* s) {
#pragma unroll 4
  for (int c = 0; c < D; c += 8) {
    float x[8];
    Io<E>::ld8(rp + (size_t)c * Io<E>::SZ, x);
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&qs[i][c]), b = *reinterpret_cast<const f32x4*>(&qs[i][c + 4]);
      float acc = s[i];
      acc = fmaf(a[0], x[0], acc); acc = fmaf(a[1], x[1], acc); acc = fmaf(a[2], x[2], acc); acc = fmaf(a[3], x[3], acc);
      acc = fmaf(b[0], x[4], acc); acc = fmaf(b[1], x[5], acc); acc = fmaf(b[2], x[6], acc); acc = fmaf(b[3], x[7], acc);
      s[i] = acc;
    }
  }
}

// acc[i] += sum over the tile rows j = kg, kg + NKG, .. of p[j][i] v_j[dc .. dc + 3], v_j at row rows.wrap(n0 + j)
template <typename E, int D, bool RING>
EA_DEV void pv_rows(Rows<RING> rows, const DecT& t, int b, int h, int n0, int nrows, int kg, int dc, const float (*ps)[QPW],
                    f32x4* acc) {
  constexpr int NKG = 64 / (D / 4);
  for (int j = kg; j < nrows; j += NKG) {
    const f32x4 v = Io<E>::ld4(row<E>(t, b, h, rows.wrap(n0 + j)) + (size_t)dc * Io<E>::SZ);
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(&ps[j][0]), p1 = *reinterpret_cast<const f32x4*>(&ps[j][4]);
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc[i] += p0[i] * v; acc[4 + i] += p1[i] * v; }
  }
}

// every output row of the step is NaN: a static step that would pass the cache's capacity (written by blockIdx.x == 0)
template <typename E, int D>
EA_DEV void refuse_out(const DecP& p, int b, int h) {
  if (blockIdx.x != 0) return;
  const float nan = __builtin_nanf("");
  for (int idx = threadIdx.x; idx < p.T * (D / 4); idx += NT) {
    const int i = idx / (D / 4), c = (idx - i * (D / 4)) * 4;
    Io<E>::st4(const_cast<char*>(row<E>(p.o, b, h, i)) + (size_t)c * Io<E>::SZ, f32x4{nan, nan, nan, nan});
  }
}

// One workgroup per window block of the step.  DEV: the grid holds the most window blocks T tokens can touch, and a block
// this step does not touch exits at once; a step that does not fit writes NaN rows.
template <typename E, int D, bool DEV, bool RING>
__global__ __launch_bounds__(NT) void ceva_attn_kernel(const DecP p) {
  static_assert(QPW == 8, "pv_rows reads the probabilities of a row as two float4");
  static_assert(DEV || !RING, "the ring belongs to the static step");
  constexpr int G = D / 4;                         // lanes per value row in P.V
  __shared__ __attribute__((aligned(16))) float qs[NW][QPW][D];
  __shared__ __attribute__((aligned(16))) float ps[NW][KT][QPW];
  __shared__ __attribute__((aligned(16))) float mo[NW][QPW][D];
  __shared__ float ml[NW][QPW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)blockIdx.y / p.H, h = (int)blockIdx.y - b * p.H;
  const Step<DEV> step(p.pos, p.t0);
  const int t0 = step.t0;
  if (!step.fits(p.T, p.cap)) { refuse_out<E, D>(p, b, h); return; }
  const int bk = t0 / p.w + (int)blockIdx.x;
  if (DEV && bk * p.w >= t0 + p.T) return;
  const int tq0 = max(t0, bk * p.w), tq1 = min(t0 + p.T, (bk + 1) * p.w);
  const int nqg = (tq1 - tq0 + QPW - 1) / QPW;
  const int nsplit = nqg >= NW ? 1 : NW / nqg;     // waves per query group
  const int Wk = p.w + p.e, nlt = (Wk + KT - 1) / KT;
  const int tend = t0 + p.T;                       // cache rows [0, tend) hold tokens
  const int kbase = bk * p.w - p.e;                // token of local slot 0
  // the block's own tokens do not straddle the end of a ring (w divides it): row = token + qs0.  Local slot 0 is row ks0,
  // up to e < ring rows before them, and the window spans w + e < ring rows from there: it wraps at most once.
  const Rows<RING> rows{p.ring};
  const int qs0 = rows.slot(bk * p.w) - bk * p.w;
  const int ks0 = rows.unwrap(kbase + qs0);
  const int pst = rows.len(p.cap);                 // row length of pad
  const int kg = lane / G, dc = (lane % G) * 4;
  for (int g = wave / nsplit; g < nqg; g += NW) {
    const int s = wave % nsplit;
    const int qa = tq0 + g * QPW, nql = min(QPW, tq1 - qa);
    for (int idx = lane; idx < QPW * (D / 8); idx += 64) {
      const int i = idx / (D / 8), c = (idx - i * (D / 8)) * 8;
      float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (i < nql) Io<E>::ld8(row<E>(p.q, b, h, qa + i + qs0) + (size_t)c * Io<E>::SZ, x);
      *reinterpret_cast<f32x4*>(&qs[wave][i][c]) = f32x4{x[0], x[1], x[2], x[3]};
      *reinterpret_cast<f32x4*>(&qs[wave][i][c + 4]) = f32x4{x[4], x[5], x[6], x[7]};
    }
    __builtin_amdgcn_wave_barrier();
    bool qpad[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) qpad[i] = i < nql && p.pad && p.pad[(size_t)b * pst + qa + i + qs0];
    const int lmax = (qa + nql - 1) / p.r;         // landmark columns of the group's last query
    const int ntile = nlt + (lmax + KT - 1) / KT;
    float m[QPW], l[QPW];
    f32x4 acc[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) { m[i] = -INFINITY; l[i] = 0.f; acc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int tile = s; tile < ntile; tile += nsplit) {
      const bool lmk = tile >= nlt;
      const int col = (lmk ? (tile - nlt) * KT : tile * KT) + lane;
      float sc[QPW];
#pragma unroll
      for (int i = 0; i < QPW; ++i) sc[i] = 0.f;
      float x[QPW];
      if (!lmk) {
        const int tok = kbase + col;
        const bool present = col < Wk && tok >= 0 && tok < tend;
        const int sl = rows.wrap(ks0 + col);       // the key's row: reduced once per lane and tile
        if (present) dot_rows<E, D>(row<E>(p.k, b, h, sl), qs[wave], sc);
        const bool kmask = !present || (p.pad && p.pad[(size_t)b * pst + sl]);
#pragma unroll
        for (int i = 0; i < QPW; ++i) {
          const int tq = qa + i;
          if (i >= nql || col >= Wk) x[i] = -INFINITY;
          else if (kmask || qpad[i] || tok > tq) x[i] = MASK_FILL;
          else x[i] = sc[i] * p.scale + (p.bias ? p.bias[(size_t)(tq - bk * p.w) * Wk + col] : 0.f);
        }
      } else {
        if (col < lmax) dot_rows<float, D>(row<float>(p.lk, b, h, col), qs[wave], sc);
#pragma unroll
        for (int i = 0; i < QPW; ++i) x[i] = (i < nql && col < (qa + i) / p.r) ? sc[i] * p.scale : -INFINITY;
      }
#pragma unroll
      for (int i = 0; i < QPW; ++i) {
        const float mn = fmaxf(m[i], wave_max(x[i]));
        const float alpha = mn == -INFINITY ? 1.f : __expf(m[i] - mn);
        const float pv = mn == -INFINITY ? 0.f : __expf(x[i] - mn);
        m[i] = mn;
        l[i] = l[i] * alpha + pv;
        acc[i] *= alpha;
        ps[wave][lane][i] = pv;
      }
      __builtin_amdgcn_wave_barrier();
      if (!lmk) {
        // rows of absent / not yet decoded tokens: p is zero for every live query, their value rows are not read
        const int j0 = max(0, -(kbase + tile * KT)), j1 = min(KT, min(Wk - tile * KT, tend - (kbase + tile * KT)));
        if (j1 > j0) pv_rows<E, D>(rows, p.v, b, h, rows.wrap(ks0 + tile * KT + j0), j1 - j0, kg, dc, &ps[wave][j0], acc);
      } else {
        pv_rows<float, D>(Rows<false>{}, p.lv, b, h, (tile - nlt) * KT, min(KT, lmax - (tile - nlt) * KT), kg, dc, ps[wave], acc);
      }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
      l[i] = wave_sum(l[i]);
#pragma unroll
      for (int o = G; o < 64; o <<= 1)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] += __shfl_xor(acc[i][c], o);
    }
    if (nsplit == 1) {
      if (lane < G) {
#pragma unroll
        for (int i = 0; i < QPW; ++i)
          if (i < nql) Io<E>::st4(const_cast<char*>(row<E>(p.o, b, h, qa + i - t0)) + (size_t)dc * Io<E>::SZ, acc[i] * (1.f / l[i]));
      }
    } else {
      if (lane < G) {
#pragma unroll
        for (int i = 0; i < QPW; ++i) *reinterpret_cast<f32x4*>(&mo[wave][i][dc]) = acc[i];
      }
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < QPW; ++i) { ml[wave][i][0] = m[i]; ml[wave][i][1] = l[i]; }
      }
    }
  }
  if (nsplit == 1) return;                         // (uniform over the workgroup)
  __syncthreads();
  const int g = wave / nsplit;
  if (wave % nsplit != 0 || g >= nqg) return;
  const int qa = tq0 + g * QPW, nql = min(QPW, tq1 - qa);
  for (int idx = lane; idx < nql * G; idx += 64) {
    const int i = idx / G, c = (idx - i * G) * 4;
    float mx = -INFINITY;
    for (int w = wave; w < wave + nsplit; ++w) mx = fmaxf(mx, ml[w][i][0]);
    float lt = 0.f;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    for (int w = wave; w < wave + nsplit; ++w) {
      const float f = ml[w][i][0] == -INFINITY ? 0.f : __expf(ml[w][i][0] - mx);
      lt += f * ml[w][i][1];
      o += f * *reinterpret_cast<const f32x4*>(&mo[w][i][c]);
    }
    Io<E>::st4(const_cast<char*>(row<E>(p.o, b, h, qa + i - t0)) + (size_t)c * Io<E>::SZ, o * (1.f / lt));
  }
}

// block-wide max / sum of one value per thread (red: 2 NW floats of LDS)
EA_DEV float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r = fmaxf(r, red[w]);
  return r;
}

// One workgroup per chunk the step completes: c_first .. c_last of the kernel arguments, or (DEV) the chunks that tokens
// t0 .. t0 + T - 1 complete; then the grid holds ceil(T / r), the most T tokens can complete, and a workgroup whose chunk
// this step does not complete exits at once.  The chunk's rows do not straddle the end of a ring (r divides it); its
// landmark row is row c.
template <typename E, int D, bool DEV, bool RING>
__global__ __launch_bounds__(NT) void ceva_close_kernel(const DecP p) {
  static_assert(DEV || !RING, "the ring belongs to the static step");
  __shared__ __attribute__((aligned(16))) float xm[2][D];      // chunk means of q, k
  __shared__ __attribute__((aligned(16))) float y[2][D];       // after the Linear layers
  __shared__ __attribute__((aligned(16))) float mu[D];
  __shared__ float pt[NT];                                      // probabilities of the current row tile
  __shared__ float red[NW];
  const int tid = threadIdx.x;
  const Step<DEV> step(p.pos, p.t0);
  const int c = (DEV ? step.t0 / p.r : p.c_first) + (int)blockIdx.x;
  if (DEV && (!step.fits(p.T, p.cap) || c > (step.t0 + p.T) / p.r - 1)) return;
  const int b = (int)blockIdx.y / p.H, h = (int)blockIdx.y - b * p.H;
  const Rows<RING> rows{p.ring};
  const int n0 = rows.slot(c * p.r);                           // first row of the chunk
  const uint8_t* pad = p.pad ? p.pad + (size_t)b * rows.len(p.cap) + n0 : nullptr;
  // masked means over the chunk's rows, divided by the chunk length
  if (tid < 2 * D) {
    const int side = tid / D, o = tid - side * D;
    const DecT& t = side ? p.k : p.q;
    float a = 0.f;
    for (int j = 0; j < p.r; ++j) {
      if (pad && pad[j]) continue;
      a += Io<E>::ld1(row<E>(t, b, h, n0 + j) + (size_t)o * Io<E>::SZ);
    }
    xm[side][o] = a * (1.f / (float)p.r);
  }
  __syncthreads();
  // mu networks: y = W x + b per side, then (adaptive) LayerNorm over the D outputs
  const int per = p.adaptive ? 4 : 2;
  if (tid < 2 * D) {
    const int side = tid / D, o = tid - side * D;
    const float* W = p.mu[side * per] + (size_t)o * D;
    float a = p.mu[side * per + 1][o];
    for (int i = 0; i < D; i += 4) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(W + i);
      a = fmaf(w4[0], xm[side][i], a); a = fmaf(w4[1], xm[side][i + 1], a);
      a = fmaf(w4[2], xm[side][i + 2], a); a = fmaf(w4[3], xm[side][i + 3], a);
    }
    y[side][o] = a;
  }
  __syncthreads();
  float z = 0.f;
  if (tid < 2 * D) {
    const int side = tid / D, o = tid - side * D;
    z = y[side][o];
    if (p.adaptive) {
      float mean = 0.f, var = 0.f;
      for (int i = 0; i < D; ++i) mean += y[side][i];
      mean *= 1.f / (float)D;
      for (int i = 0; i < D; ++i) { const float dv = y[side][i] - mean; var = fmaf(dv, dv, var); }
      var *= 1.f / (float)D;
      z = (z - mean) / sqrtf(var + 1e-5f) * p.mu[side * per + 2][o] + p.mu[side * per + 3][o];
    }
  }
  __syncthreads();
  if (tid >= D && tid < 2 * D) {                   // k side: rf_k_bar = rk
    const int o = tid - D;
    xm[1][o] = z;
    const_cast<float*>(reinterpret_cast<const float*>(row<float>(p.lk, b, h, c)))[o] = z;
  }
  __syncthreads();
  if (tid < D) mu[tid] = z + xm[1][tid];           // mu = mu_q(qm) + rk
  __syncthreads();
  // beta = softmax over the chunk rows of (s mu.k_j - s |k_j|^2 / 2), padded rows -5e4 with a zero value row
  float mrun = -INFINITY, lrun = 0.f, acc = 0.f;
  for (int j0 = 0; j0 < p.r; j0 += NT) {
    const int j = j0 + tid;
    float x = -INFINITY;
    if (j < p.r) {
      if (pad && pad[j]) {
        x = MASK_FILL;
      } else {
        const char* rp = row<E>(p.k, b, h, n0 + j);
        float dot = 0.f, nn = 0.f;
        for (int c8 = 0; c8 < D; c8 += 8) {
          float kx[8];
          Io<E>::ld8(rp + (size_t)c8 * Io<E>::SZ, kx);
#pragma unroll
          for (int e = 0; e < 8; ++e) { dot = fmaf(mu[c8 + e], kx[e], dot); nn = fmaf(kx[e], kx[e], nn); }
        }
        x = dot * p.scale - 0.5f * p.scale * nn;
      }
    }
    const float mn = fmaxf(mrun, block_max(x, red));
    pt[tid] = x == -INFINITY ? 0.f : __expf(x - mn);
    __syncthreads();
    if (tid < D) {
      const float alpha = mrun == -INFINITY ? 0.f : __expf(mrun - mn);
      lrun *= alpha;
      acc *= alpha;
      const int nj = min(NT, p.r - j0);
      for (int jj = 0; jj < nj; ++jj) {
        lrun += pt[jj];
        if (pad && pad[j0 + jj]) continue;
        acc = fmaf(pt[jj], Io<E>::ld1(row<E>(p.v, b, h, n0 + j0 + jj) + (size_t)tid * Io<E>::SZ), acc);
      }
    }
    mrun = mn;
    __syncthreads();
  }
  if (tid < D) const_cast<float*>(reinterpret_cast<const float*>(row<float>(p.lv, b, h, c)))[tid] = acc / lrun;
}

// ---- DEV steps: the token count lives in device memory -----------------------------------------------------------------
// A step is append -> close -> attn -> advance on one stream.  Only advance writes *pos, so the three before it read the
// same count, and each decides from it alone whether the step fits the cache.  A step that does not fit writes no cache
// byte: append sets *status, close exits, attn writes NaN rows, advance leaves *pos.

// one workgroup per (token t, element b) of the step: the token's [3, H, D] row, 16 bytes per lane and load, and its pad flag.
// Each token's row is reduced on its own (a step may straddle the end of a ring); the capacity test stays on p.cap, the
// landmark capacity.
template <bool RING>
__global__ __launch_bounds__(NT) void ceva_append_kernel(const AppP p) {
  const Step<true> step(p.pos, 0);
  const int t = (int)blockIdx.x, b = (int)blockIdx.y;
  if (!step.fits(p.T, p.cap)) {
    if (t == 0 && b == 0 && threadIdx.x == 0) *p.status = 1;
    return;
  }
  const u32x4* src = reinterpret_cast<const u32x4*>(p.src + ((size_t)t * p.B + b) * p.row_bytes);
  const Rows<RING> rows{p.ring};
  const size_t at = (size_t)b * rows.len(p.cap) + rows.slot(step.t0, t);
  u32x4* dst = reinterpret_cast<u32x4*>(p.cache + at * p.row_bytes);
  for (int i = threadIdx.x; i < p.row_bytes / 16; i += NT) dst[i] = src[i];
  if (threadIdx.x == 0) p.pad[at] = p.src_pad ? p.src_pad[(size_t)b * p.T + t] : (uint8_t)0;
}

// *pos += T, in a launch of its own after attn on the same stream: stream order puts it behind every read of *pos in the
// step.  (The other way, the last attn workgroup advancing through a completion counter, needs an agent-scope release /
// acquire pair across XCDs and a counter that every replay must find reset; a dependent launch boundary costs about
// 1.5 us, eager or in a graph, and leaves no ordering to get wrong.)
__global__ __launch_bounds__(64) void ceva_advance_kernel(int32_t* pos, int T, int cap) {
  if (threadIdx.x == 0) {
    const Step<true> step(pos, 0);
    if (step.fits(T, cap)) *pos = step.t0 + T;
  }
}

using DecKernel = void (*)(const DecP);

template <typename E, int D>
DecKernel kernel_of(DecKind kind, bool dev, bool ring) {
  if (kind == DEC_CLOSE)
    return !dev ? ceva_close_kernel<E, D, false, false> : ring ? ceva_close_kernel<E, D, true, true> : ceva_close_kernel<E, D, true, false>;
  return !dev ? ceva_attn_kernel<E, D, false, false> : ring ? ceva_attn_kernel<E, D, true, true> : ceva_attn_kernel<E, D, true, false>;
}

template <typename E>
DecKernel kernel_of(int D, DecKind kind, bool dev, bool ring) {
  switch (D) {
    case 32: return kernel_of<E, 32>(kind, dev, ring);
    case 64: return kernel_of<E, 64>(kind, dev, ring);
    default: return kernel_of<E, 128>(kind, dev, ring);
  }
}

}  // namespace

// DEV / RING follow the state: p.pos != null / p.ring != 0.  (The C entry points have checked the ring: a multiple of w
// that holds the span of one step, ea_capi.hip.)
int ceva_decode_launch(DecKind kind, const DecP& p, hipStream_t st) {
  const bool dev = p.pos != nullptr, ring = p.ring != 0;
  if (dev ? !p.pad : ring) return EA_E_BADARG;     // a DEV step always reads the pad flags; a ring belongs to a DEV step
  if (p.D != 32 && p.D != 64 && p.D != 128) return EA_E_UNSUPPORTED;
  DecKernel kernel;
  switch (p.dtype) {
    case EA_BF16: kernel = kernel_of<BF16>(p.D, kind, dev, ring); break;
    case EA_F16: kernel = kernel_of<F16>(p.D, kind, dev, ring); break;
    case EA_F32: kernel = kernel_of<float>(p.D, kind, dev, ring); break;
    default: return EA_E_BADARG;
  }
  // x: the chunks the step closes / the window blocks it touches; DEV: the most T tokens can, wherever they start
  const int nx = kind == DEC_CLOSE ? (dev ? (p.T + p.r - 1) / p.r : p.c_last - p.c_first + 1)
                                   : (dev ? (p.T + p.w - 2) / p.w + 1 : (p.t0 + p.T - 1) / p.w - p.t0 / p.w + 1);
  hipLaunchKernelGGL(kernel, dim3((unsigned)nx, (unsigned)(p.B * p.H)), dim3(NT), 0, st, p);
  return (int)hipGetLastError();
}

int ceva_sdecode_append(const AppP& p, hipStream_t st) {
  hipLaunchKernelGGL(p.ring ? ceva_append_kernel<true> : ceva_append_kernel<false>, dim3((unsigned)p.T, (unsigned)p.B), dim3(NT),
                     0, st, p);
  return (int)hipGetLastError();
}

int ceva_sdecode_advance(int32_t* pos, int T, int cap, hipStream_t st) {
  hipLaunchKernelGGL(ceva_advance_kernel, dim3(1), dim3(64), 0, st, pos, T, cap);
  return (int)hipGetLastError();
}

}  // namespace ea
