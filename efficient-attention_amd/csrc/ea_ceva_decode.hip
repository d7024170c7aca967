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
//   SEQ  (p.ntok != null, with DEV): whose count it is, and how many of the step's T tokens are this batch element's.  false:
//        one count for the batch, every element takes all T.  true: t0 = p.pos[b], and element b takes n_b = p.ntok[b] <= T
//        tokens, the positions before its first flag in the step's pad flags (append finds n_b and publishes it; close, attn
//        and advance read it behind that launch).  Nothing is stored for the other positions, their output rows are zero,
//        and overflow is per element: status[b], NaN rows of b alone.  The grids stay those of T tokens; a workgroup whose
//        element needs less exits at once.  `Step` owns both numbers; no kernel body reads p.T for anything else.
// A fourth template parameter of close, attn and attn_split is no switch of the step but the element type L of the landmark
// rows (rf_k_bar, beta): float, or E on a compact state (16-bit DEV steps only).
// A DEV step of at most QPW tokens can run attn as two launches, attn_split -> merge, with the tiles of a window block shared
// by several workgroups (ea_ceva_decode_split.h).  attn and attn_split are one body: the staging
// of a query group, the tile loop with its online softmax, the stash of a wave's partial and the merge over waves exist
// once, as the helpers below (Group, stage_queries, stream_tiles, stash_partial, merge_waves).  A kernel keeps its Step, its
// refusals and exits, its map from blockIdx to (block, part), which tiles a wave takes and what becomes of the result.
#include "ea_common.h"
#include "ea_ceva_decode.h"
#include <type_traits>

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
  static EA_DEV void st1(char* p, float v) { *reinterpret_cast<float*>(p) = v; }
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
  static EA_DEV void st1(char* p, float v) { *reinterpret_cast<uint16_t*>(p) = H::from_f(v); }   // to nearest even
  static constexpr int SZ = 2;
};
template <> struct Io<BF16> : Io16<BF16> {};
template <> struct Io<F16> : Io16<F16> {};

template <typename E> EA_DEV const char* row(const DecT& t, int b, int h, int n) {
  return t.p + ((size_t)b * t.sb + (size_t)h * t.sh + (size_t)n * t.sn) * Io<E>::SZ;
}

// element o of landmark row c (rf_k_bar, beta) = v: close's two stores.  L = float: the value as it is; a 16-bit L (a compact
// state): rounded once, to nearest even
template <typename L> EA_DEV void store_lmk(const DecT& t, int b, int h, int c, int o, float v) {
  Io<L>::st1(const_cast<char*>(row<L>(t, b, h, c)) + (size_t)o * Io<L>::SZ, v);
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

// Where the step starts, how many tokens of it batch element b has, and whether they fit the cache.  DEV = false: the kernel
// argument (the host has checked the capacity: `fits` is true and folds away).  DEV = true: the token count in device memory
// -- one value for every thread of the step's launches up to advance, so every exit decided from it is uniform.  SEQ: the
// count and the share of element b; a workgroup has one b, so the exits stay uniform.
template <bool DEV, bool SEQ = false> struct Step {
  static_assert(DEV || !SEQ, "per-sequence counts belong to the static step");
  int t0, own;                                     // own: the element's tokens of this step (SEQ; else all T of them)
  EA_DEV Step(const DecP& p, int b) : t0(SEQ ? p.pos[b] : DEV ? *p.pos : p.t0), own(SEQ ? p.ntok[b] : 0) {}
  EA_DEV Step(const int32_t* pos, int b, int n_own) : t0(pos[SEQ ? b : 0]), own(n_own) {}   // append finds n itself
  EA_DEV int n(int T) const { return SEQ ? own : T; }
  EA_DEV bool fits(int T, int cap) const { return !DEV || t0 + n(T) <= cap; }
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

// output rows n .. T - 1 of element b are zero: the step positions that are not its tokens (SEQ; written by blockIdx.x == 0)
template <typename E, int D>
EA_DEV void zero_out(const DecP& p, int b, int h, int n) {
  if (blockIdx.x != 0) return;
  for (int idx = n * (D / 4) + threadIdx.x; idx < p.T * (D / 4); idx += NT) {
    const int i = idx / (D / 4), c = (idx - i * (D / 4)) * 4;
    Io<E>::st4(const_cast<char*>(row<E>(p.o, b, h, i)) + (size_t)c * Io<E>::SZ, f32x4{0.f, 0.f, 0.f, 0.f});
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


// ---- what ceva_attn and ceva_attn_split share: one query group of a window block against a strided list of its tiles -----
// The pad flags of a launch.  OPT: they may be absent (the dynamic step's; null = no position is padded), and every read
// tests the pointer; a launch that always has them (attn_split) reads them outright.
template <bool OPT> struct Pad {
  const uint8_t* f;
  EA_DEV bool at(size_t i) const { return (!OPT || f) && f[i]; }
};

// Where the queries and the local keys of window block bk lie; the kernel sets [qa, qa + nql), the query group, itself.
// The block's own tokens do not straddle the end of a ring (w divides it): row = token + qs0.  Local slot 0 is row ks0, up
// to e < ring rows before them, and the window spans w + e < ring rows from there: it wraps at most once.
struct Group {
  int bk, qa, nql, tend, kbase, qs0, ks0, pst, Wk, nlt;
  template <bool RING>
  EA_DEV Group(const DecP& p, Rows<RING> rows, int bk, int tend)     // tend: cache rows [0, tend) hold tokens
      : bk(bk), qa(0), nql(0), tend(tend),
        kbase(bk * p.w - p.e),                     // token of local slot 0
        qs0(rows.slot(bk * p.w) - bk * p.w), ks0(rows.unwrap(kbase + qs0)),
        pst(rows.len(p.cap)),                      // row length of pad
        Wk(p.w + p.e), nlt((Wk + KT - 1) / KT) {}
};

// the group's query rows -> qs as floats, rows nql .. QPW - 1 zero
template <typename E, int D>
EA_DEV void stage_queries(const DecP& p, int b, int h, const Group& g, float (*qs)[D], int lane) {
  for (int idx = lane; idx < QPW * (D / 8); idx += 64) {
    const int i = idx / (D / 8), c = (idx - i * (D / 8)) * 8;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < g.nql) Io<E>::ld8(row<E>(p.q, b, h, g.qa + i + g.qs0) + (size_t)c * Io<E>::SZ, x);
    *reinterpret_cast<f32x4*>(&qs[i][c]) = f32x4{x[0], x[1], x[2], x[3]};
    *reinterpret_cast<f32x4*>(&qs[i][c + 4]) = f32x4{x[4], x[5], x[6], x[7]};
  }
  __builtin_amdgcn_wave_barrier();
}

// tiles first, first + stride, .. of [local tiles, landmark tiles]: online softmax into (m, l, acc), then l and acc summed
// over the lanes that hold a share of them.  L: the element type of the landmark rows -- float, or E on a compact state
template <typename E, int D, bool RING, bool OPT, typename L>
EA_DEV void stream_tiles(const DecP& p, int b, int h, const Group& g, int first, int stride, const float (*qs)[D],
                         float (*ps)[QPW], int lane, float* m, float* l, f32x4* acc) {
  static_assert(QPW == 8, "pv_rows reads the probabilities of a row as two float4");
  constexpr int G = D / 4;                         // lanes per value row in P.V
  const Rows<RING> rows{p.ring};
  const Pad<OPT> pad{p.pad};
  const int kg = lane / G, dc = (lane % G) * 4;
  const int bk = g.bk, qa = g.qa, nql = g.nql, tend = g.tend, kbase = g.kbase, ks0 = g.ks0, pst = g.pst, Wk = g.Wk, nlt = g.nlt;
  bool qpad[QPW];
#pragma unroll
  for (int i = 0; i < QPW; ++i) qpad[i] = i < nql && pad.at((size_t)b * pst + qa + i + g.qs0);
  const int lmax = (qa + nql - 1) / p.r;           // landmark columns of the group's last query
  const int ntile = nlt + (lmax + KT - 1) / KT;
#pragma unroll
  for (int i = 0; i < QPW; ++i) { m[i] = -INFINITY; l[i] = 0.f; acc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int tile = first; tile < ntile; tile += stride) {
    const bool lmk = tile >= nlt;
    const int col = (lmk ? (tile - nlt) * KT : tile * KT) + lane;
    float sc[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) sc[i] = 0.f;
    float x[QPW];
    if (!lmk) {
      const int tok = kbase + col;
      const bool present = col < Wk && tok >= 0 && tok < tend;
      const int sl = rows.wrap(ks0 + col);         // the key's row: reduced once per lane and tile
      if (present) dot_rows<E, D>(row<E>(p.k, b, h, sl), qs, sc);
      const bool kmask = !present || pad.at((size_t)b * pst + sl);
#pragma unroll
      for (int i = 0; i < QPW; ++i) {
        const int tq = qa + i;
        if (i >= nql || col >= Wk) x[i] = -INFINITY;
        else if (kmask || qpad[i] || tok > tq) x[i] = MASK_FILL;
        else x[i] = sc[i] * p.scale + (p.bias ? p.bias[(size_t)(tq - bk * p.w) * Wk + col] : 0.f);
      }
    } else {
      if (col < lmax) dot_rows<L, D>(row<L>(p.lk, b, h, col), qs, sc);
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
      ps[lane][i] = pv;
    }
    __builtin_amdgcn_wave_barrier();
    if (!lmk) {
      // rows of absent / not yet decoded tokens: p is zero for every live query, their value rows are not read
      const int j0 = max(0, -(kbase + tile * KT)), j1 = min(KT, min(Wk - tile * KT, tend - (kbase + tile * KT)));
      if (j1 > j0) pv_rows<E, D>(rows, p.v, b, h, rows.wrap(ks0 + tile * KT + j0), j1 - j0, kg, dc, &ps[j0], acc);
    } else {
      pv_rows<L, D>(Rows<false>{}, p.lv, b, h, (tile - nlt) * KT, min(KT, lmax - (tile - nlt) * KT), kg, dc, ps, acc);
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
}

// a wave's partial of its group -> LDS, for the merge over the waves that shared the group
template <int D>
EA_DEV void stash_partial(const float* m, const float* l, const f32x4* acc, float (*mo)[D], float (*ml)[2], int lane) {
  constexpr int G = D / 4;
  if (lane < G) {
#pragma unroll
    for (int i = 0; i < QPW; ++i) *reinterpret_cast<f32x4*>(&mo[i][lane * 4]) = acc[i];
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < QPW; ++i) { ml[i][0] = m[i]; ml[i][1] = l[i]; }
  }
}

// columns c .. c + 3 of query i, merged over waves w0 .. w0 + n - 1 in that order: not normalised
template <int D>
EA_DEV f32x4 merge_waves(const float (*mo)[QPW][D], const float (*ml)[QPW][2], int w0, int n, int i, int c, float& mx, float& lt) {
  mx = -INFINITY;
  for (int w = w0; w < w0 + n; ++w) mx = fmaxf(mx, ml[w][i][0]);
  lt = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int w = w0; w < w0 + n; ++w) {
    const float f = ml[w][i][0] == -INFINITY ? 0.f : __expf(ml[w][i][0] - mx);
    lt += f * ml[w][i][1];
    o += f * *reinterpret_cast<const f32x4*>(&mo[w][i][c]);
  }
  return o;
}

// ---- DEV steps: the token count lives in device memory -----------------------------------------------------------------
// A step is append -> close -> attn -> advance on one stream.  Only advance writes *pos, so the three before it read the
// same count, and each decides from it alone whether the step fits the cache.  A step that does not fit writes no cache
// byte: append sets *status, close exits, attn writes NaN rows, advance leaves *pos.

// The first flagged position of a row of T step flags (T when there is none): the element's token count of this step.
// 16 flags per load where the row allows (its ends, up to 15 bytes each, go byte by byte: a row of [B, T] starts at any
// address), the first set byte of a load by its lowest set bit, then a minimum over the workgroup (red: NW ints of LDS).
EA_DEV int first_flag(const uint8_t* f, int T, int* red) {
  const int tid = threadIdx.x;
  const int head = min(T, (int)((16 - ((uintptr_t)f & 15)) & 15));
  const int nvec = (T - head) / 16, tail = head + nvec * 16;
  int first = T;
  if (tid < head && f[tid]) first = tid;
  const u32x4* v = reinterpret_cast<const u32x4*>(f + head);
  for (int i = tid; i < nvec; i += NT) {           // (a thread's later loads lie further on: its first hit is its minimum)
    const u32x4 u = v[i];
    int at = 16;
#pragma unroll
    for (int c = 3; c >= 0; --c)
      if (u[c]) at = c * 4 + (__builtin_ctz(u[c]) >> 3);
    if (at < 16) { first = min(first, head + i * 16 + at); break; }
  }
  if (tid < T - tail && f[tail + tid]) first = min(first, tail + tid);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
  if ((tid & 63) == 0) red[tid >> 6] = first;
  __syncthreads();
  first = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) first = min(first, red[w]);
  return first;
}


// ---- the kernels of a step (ea_ceva_decode_step.h), and of a short step with its landmark range split over workgroups
// (ea_ceva_decode_split.h)
#include "ea_ceva_decode_step.h"
#include "ea_ceva_decode_split.h"

// *pos += T, in a launch of its own after attn on the same stream: stream order puts it behind every read of *pos in the
// step.  (The other way, the last attn workgroup advancing through a completion counter, needs an agent-scope release /
// acquire pair across XCDs and a counter that every replay must find reset; a dependent launch boundary costs about
// 1.5 us, eager or in a graph, and leaves no ordering to get wrong.)
__global__ __launch_bounds__(64) void ceva_advance_kernel(int32_t* pos, int T, int cap) {
  if (threadIdx.x == 0) {
    const Step<true> step(pos, 0, T);
    if (step.fits(T, cap)) *pos = step.t0 + T;
  }
}

// SEQ: pos[b] += ntok[b], one thread per batch element; an element that does not fit keeps its count
__global__ __launch_bounds__(64) void ceva_advance_seq_kernel(int32_t* pos, const int32_t* ntok, int B, int cap) {
  const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (b >= B) return;
  const Step<true, true> step(pos, b, ntok[b]);
  if (step.fits(0, cap)) pos[b] = step.t0 + step.n(0);
}

using DecKernel = void (*)(const DecP);
using SplitKernel = void (*)(const DecSplitP);
using MergeKernel = void (*)(const DecMergeP);

// a run-time flag -> its template argument: f(std::bool_constant<flag>{}), the one place a flag of a step is mapped
template <typename F>
auto with_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }

// L: the landmark element type, float or (a compact state) E; for fp32 rows the two are one instance.  RING, SEQ and a
// 16-bit L belong to a DEV step: null without it (the launchers have refused that)
template <typename E, int D, typename L>
DecKernel kernel_of(DecKind kind, bool dev, bool ring, bool seq) {
  return with_flag(dev, [&](auto dv) {
    return with_flag(ring, [&](auto rg) {
      return with_flag(seq, [&](auto sq) -> DecKernel {
        constexpr bool DEV = decltype(dv)::value, RING = decltype(rg)::value, SEQ = decltype(sq)::value;
        if constexpr (DEV || !(RING || SEQ || Io<L>::SZ == 2))
          return kind == DEC_CLOSE ? ceva_close_kernel<E, D, DEV, RING, SEQ, L> : ceva_attn_kernel<E, D, DEV, RING, SEQ, L>;
        return nullptr;
      });
    });
  });
}

template <typename E, int D, typename L>
SplitKernel split_of(bool ring, bool seq) {
  return with_flag(ring, [&](auto rg) {
    return with_flag(seq, [&](auto sq) -> SplitKernel { return ceva_attn_split_kernel<E, D, decltype(rg)::value, decltype(sq)::value, L>; });
  });
}

template <typename E, int D>
MergeKernel merge_of(bool seq) { return seq ? ceva_merge_kernel<E, D, true> : ceva_merge_kernel<E, D, false>; }

// (dtype, D) -> <E, D>: calls pick(E{}, Dim<D>{}), which chooses its kernel instance.  False for a dtype that is none of the
// three; the callers have refused every D but 32, 64 and 128 before.
template <int D> struct Dim { static constexpr int value = D; };
template <typename F>
bool with_types(int dtype, int D, F&& pick) {
  const auto dims = [&](auto e) {
    switch (D) {
      case 32: pick(e, Dim<32>{}); break;
      case 64: pick(e, Dim<64>{}); break;
      default: pick(e, Dim<128>{}); break;
    }
  };
  switch (dtype) {
    case EA_BF16: dims(BF16{}); return true;
    case EA_F16: dims(F16{}); return true;
    case EA_F32: dims(0.f); return true;
    default: return false;
  }
}

}  // namespace

// DEV / RING / SEQ follow the state: p.pos != null / p.ring != 0 / p.ntok != null.  (The C entry points have checked the
// ring: a multiple of w that holds the span of one step, ea_capi.hip.)  l16: p.lk, p.lv are rows of p.dtype, a 16-bit type.
int ceva_decode_launch(DecKind kind, const DecP& p, hipStream_t st, bool l16) {
  const bool dev = p.pos != nullptr, ring = p.ring != 0, seq = p.ntok != nullptr;
  if (dev ? !p.pad : (ring || seq)) return EA_E_BADARG;   // a DEV step always reads the pad flags; ring, ntok belong to a DEV step
  if (l16 && (!dev || p.dtype == EA_F32)) return EA_E_BADARG;   // compact landmark rows belong to a 16-bit DEV step
  if (p.D != 32 && p.D != 64 && p.D != 128) return EA_E_UNSUPPORTED;
  DecKernel kernel;
  if (!with_types(p.dtype, p.D, [&](auto e, auto d) {
        using E = decltype(e);
        constexpr int D = decltype(d)::value;
        kernel = l16 ? kernel_of<E, D, E>(kind, dev, ring, seq) : kernel_of<E, D, float>(kind, dev, ring, seq);
      }))
    return EA_E_BADARG;
  // x: the chunks the step closes / the window blocks it touches; DEV: the most T tokens can, wherever they start
  const int nx = kind == DEC_CLOSE ? (dev ? (p.T + p.r - 1) / p.r : p.c_last - p.c_first + 1)
                                   : (dev ? (p.T + p.w - 2) / p.w + 1 : (p.t0 + p.T - 1) / p.w - p.t0 / p.w + 1);
  hipLaunchKernelGGL(kernel, dim3((unsigned)nx, (unsigned)(p.B * p.H)), dim3(NT), 0, st, p);
  return (int)hipGetLastError();
}

// (The C entry points have checked parts, the workspace and T <= QPW.)
int ceva_sdecode_attn_split(const DecP& p, int parts, float* ws, hipStream_t st, bool l16) {
  const bool ring = p.ring != 0, seq = p.ntok != nullptr;
  if (!p.pos || !p.pad || !ws || parts < 2 || parts > 64 || p.T > QPW || (l16 && p.dtype == EA_F32)) return EA_E_BADARG;
  if (p.D != 32 && p.D != 64 && p.D != 128) return EA_E_UNSUPPORTED;
  SplitKernel kernel;
  if (!with_types(p.dtype, p.D, [&](auto e, auto d) {
        using E = decltype(e);
        constexpr int D = decltype(d)::value;
        kernel = l16 ? split_of<E, D, E>(ring, seq) : split_of<E, D, float>(ring, seq);
      }))
    return EA_E_BADARG;
  const int nx = (p.T + p.w - 2) / p.w + 1;        // the most window blocks T tokens can touch
  const DecSplitP sp = {p, ws, parts};
  hipLaunchKernelGGL(kernel, dim3((unsigned)(nx * parts), (unsigned)(p.B * p.H)), dim3(NT), 0, st, sp);
  return (int)hipGetLastError();
}

int ceva_sdecode_merge(const DecMergeP& p, int D, int dtype, int BH, hipStream_t st) {
  const bool seq = p.ntok != nullptr;
  if (!p.pos || !p.ws || p.parts < 2 || p.parts > 64 || p.T > QPW) return EA_E_BADARG;
  if (D != 32 && D != 64 && D != 128) return EA_E_UNSUPPORTED;
  MergeKernel kernel;
  if (!with_types(dtype, D, [&](auto e, auto d) { kernel = merge_of<decltype(e), decltype(d)::value>(seq); })) return EA_E_BADARG;
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.T, (unsigned)BH), dim3(64), 0, st, p);
  return (int)hipGetLastError();
}

int ceva_sdecode_append(const AppP& p, hipStream_t st) {
  void (*kernel)(const AppP) = with_flag(p.ring != 0, [&](auto rg) {
    return with_flag(p.ntok != nullptr, [&](auto sq) { return &ceva_append_kernel<decltype(rg)::value, decltype(sq)::value>; });
  });
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.T, (unsigned)p.B), dim3(NT), 0, st, p);
  return (int)hipGetLastError();
}

int ceva_sdecode_advance(int32_t* pos, const int32_t* ntok, int B, int T, int cap, hipStream_t st) {
  if (ntok) hipLaunchKernelGGL(ceva_advance_seq_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, pos, ntok, B, cap);
  else hipLaunchKernelGGL(ceva_advance_kernel, dim3(1), dim3(64), 0, st, pos, T, cap);
  return (int)hipGetLastError();
}

}  // namespace ea
