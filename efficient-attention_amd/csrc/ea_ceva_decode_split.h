// ea_ceva_decode_split.h -- a short decoding step with its landmark range split over workgroups: attn_split, merge.
// Not a header of declarations: ea_ceva_decode.hip includes this text once, inside its anonymous namespace and after the
// kernels of ea_ceva_decode_step.h, whose helpers (Io, row, Rows, Step, dot_rows, pv_rows, refuse_out, zero_out) it uses;
// those kernels keep their symbols and their code (tools/isa_diff.py).
//
// ceva_attn streams every landmark row of a (b, h) through ONE workgroup: at a long context a 1-token step is bound by the
// latency of that one CU, not by bandwidth.  A step of at most QPW tokens has one query group per window block, and there the
// four waves of ceva_attn already share the 64-column tiles of [local tiles, landmark tiles] with stride 4 and merge their
// (max, sum, acc) partials in LDS.  Here `parts` workgroups per window block share them with stride 4 parts:
//   ceva_attn_split_kernel, one workgroup per (window block the step can touch, part, b, h): wave s of part p is virtual
//     wave p 4 + s and takes tiles p 4 + s, + 4 parts, ..  -- balanced at any position, no context length on the host.  After
//     the in-LDS merge of its four waves it does not normalise: for each live query it writes (acc[D], m, l) to the workspace.
//   ceva_merge_kernel, one workgroup per (step token, b, h): combines the parts of a live query as the in-LDS merge does,
//     normalises and stores the output row in the cache's dtype.
// The partials travel through global memory and the launch boundary orders them: no atomics, no completion counter, no
// workgroup waits for another (the decision recorded for advance, ea_ceva_decode.hip).
// Workspace: fp32 [B, H, QPW, parts, D + 4]; row (b, h, t - t0, p) = acc[0 .. D - 1], m, l, two unused floats (rows stay
// 16-byte aligned).  A query belongs to exactly one window block, so every row of a live query is written exactly once per
// step, by ordinary vector stores, and rows of other step positions are not read.  A part whose tile list is empty writes
// m = -inf, l = 0, acc = 0.
// What a step refuses stays with blockIdx.x == 0 of attn_split (block 0, part 0): NaN rows of a step that does not fit, zero
// rows n_b .. T - 1 of a per-sequence element; merge re-evaluates both tests from pos / ntok (advance runs behind it) and leaves
// those rows alone.
#if !defined(CEVA_SPLIT_TEXT)
#error "included by ea_ceva_decode.hip only"
#endif

constexpr int WSX = 4;                             // floats behind acc[D] in a workspace row: m, l, 2 unused

template <typename E, int D, bool RING, bool SEQ>
__global__ __launch_bounds__(NT) void ceva_attn_split_kernel(const DecSplitP sp) {
  static_assert(QPW == 8, "pv_rows reads the probabilities of a row as two float4");
  const DecP& p = sp.d;
  constexpr int G = D / 4;                         // lanes per value row in P.V
  __shared__ __attribute__((aligned(16))) float qs[NW][QPW][D];
  __shared__ __attribute__((aligned(16))) float ps[NW][KT][QPW];
  __shared__ __attribute__((aligned(16))) float mo[NW][QPW][D];
  __shared__ float ml[NW][QPW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)blockIdx.y / p.H, h = (int)blockIdx.y - b * p.H;
  const Step<true, SEQ> step(p, b);
  const int t0 = step.t0;
  if (!step.fits(p.T, p.cap)) { refuse_out<E, D>(p, b, h); return; }
  if (SEQ) {
    zero_out<E, D>(p, b, h, step.n(p.T));
    if (step.n(p.T) == 0) return;                  // an element that sits the step out
  }
  const int blk = (int)blockIdx.x / sp.parts, part = (int)blockIdx.x - blk * sp.parts;
  const int bk = t0 / p.w + blk;
  if (bk * p.w >= t0 + step.n(p.T)) return;
  // the block's queries: at most T <= QPW of them, one query group, shared by all four waves
  const int qa = max(t0, bk * p.w), nql = min(t0 + step.n(p.T), (bk + 1) * p.w) - qa;
  const int Wk = p.w + p.e, nlt = (Wk + KT - 1) / KT;
  const int tend = t0 + step.n(p.T);               // cache rows [0, tend) hold tokens
  const int kbase = bk * p.w - p.e;                // token of local slot 0
  const Rows<RING> rows{p.ring};
  const int qs0 = rows.slot(bk * p.w) - bk * p.w;
  const int ks0 = rows.unwrap(kbase + qs0);
  const int pst = rows.len(p.cap);                 // row length of pad
  const int kg = lane / G, dc = (lane % G) * 4;
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
  for (int i = 0; i < QPW; ++i) qpad[i] = i < nql && p.pad[(size_t)b * pst + qa + i + qs0];
  const int lmax = (qa + nql - 1) / p.r;           // landmark columns of the group's last query
  const int ntile = nlt + (lmax + KT - 1) / KT;
  float m[QPW], l[QPW];
  f32x4 acc[QPW];
#pragma unroll
  for (int i = 0; i < QPW; ++i) { m[i] = -INFINITY; l[i] = 0.f; acc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int tile = part * NW + wave; tile < ntile; tile += sp.parts * NW) {
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
      if (present) dot_rows<E, D>(row<E>(p.k, b, h, sl), qs[wave], sc);
      const bool kmask = !present || p.pad[(size_t)b * pst + sl];
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
  if (lane < G) {
#pragma unroll
    for (int i = 0; i < QPW; ++i) *reinterpret_cast<f32x4*>(&mo[wave][i][dc]) = acc[i];
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < QPW; ++i) { ml[wave][i][0] = m[i]; ml[wave][i][1] = l[i]; }
  }
  __syncthreads();
  if (wave != 0) return;
  // the part's partial of each live query: the four waves merged, not normalised
  float* ws = sp.ws + (((size_t)blockIdx.y * QPW + (qa - t0)) * sp.parts + part) * (D + WSX);
  for (int idx = lane; idx < nql * G; idx += 64) {
    const int i = idx / G, c = (idx - i * G) * 4;
    float mx = -INFINITY;
    for (int w = 0; w < NW; ++w) mx = fmaxf(mx, ml[w][i][0]);
    float lt = 0.f;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < NW; ++w) {
      const float f = ml[w][i][0] == -INFINITY ? 0.f : __expf(ml[w][i][0] - mx);
      lt += f * ml[w][i][1];
      o += f * *reinterpret_cast<const f32x4*>(&mo[w][i][c]);
    }
    float* dst = ws + (size_t)i * sp.parts * (D + WSX);
    *reinterpret_cast<f32x4*>(dst + c) = o;
    if (c == 0) *reinterpret_cast<f32x4*>(dst + D) = f32x4{mx, lt, 0.f, 0.f};
  }
}


// One wave per (step token t, b, h).  Lane p reads (m, l) of part p and the wave finds the common maximum; then G lanes
// add the parts' rows in part order, as the in-LDS merge adds its waves.
template <typename E, int D, bool SEQ>
__global__ __launch_bounds__(64) void ceva_merge_kernel(const DecMergeP p) {
  constexpr int G = D / 4;
  __shared__ float fs[64], ls[64];
  const int t = (int)blockIdx.x, lane = threadIdx.x;
  const int b = (int)blockIdx.y / p.H, h = (int)blockIdx.y - b * p.H;
  const Step<true, SEQ> step(p.pos, b, SEQ ? p.ntok[b] : 0);
  if (!step.fits(p.T, p.cap) || t >= step.n(p.T)) return;     // NaN rows, zero rows: attn_split has written them
  const float* ws = p.ws + ((size_t)blockIdx.y * QPW + t) * p.parts * (D + WSX);
  float m = -INFINITY, l = 0.f;
  if (lane < p.parts) {
    m = ws[(size_t)lane * (D + WSX) + D];
    l = ws[(size_t)lane * (D + WSX) + D + 1];
  }
  const float mx = wave_max(m);
  const float f = m == -INFINITY ? 0.f : __expf(m - mx);
  fs[lane] = f;
  ls[lane] = f * l;
  __syncthreads();
  if (lane >= G) return;
  float lt = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int q = 0; q < p.parts; ++q) {
    lt += ls[q];
    o += fs[q] * *reinterpret_cast<const f32x4*>(ws + (size_t)q * (D + WSX) + lane * 4);
  }
  Io<E>::st4(const_cast<char*>(row<E>(p.o, b, h, t)) + (size_t)lane * 4 * Io<E>::SZ, o * (1.f / lt));
}
