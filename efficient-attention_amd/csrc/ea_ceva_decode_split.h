// ea_ceva_decode_split.h -- a short decoding step with its landmark range split over workgroups: attn_split, merge.
// Included once by ea_ceva_decode.hip, inside its anonymous namespace and after the kernels of ea_ceva_decode_step.h.
//
// ceva_attn streams every landmark row of a (b, h) through ONE workgroup: at a long context a 1-token step is bound by the
// latency of that one CU, not by bandwidth.  A step of at most QPW tokens has one query group per window block, and there the
// four waves of ceva_attn share the tiles of [local tiles, landmark tiles] with stride 4.  Here `parts` workgroups per
// window block share them with stride 4 parts, on the same body (stage_queries, stream_tiles, stash_partial, merge_waves of
// ea_ceva_decode.hip).  What this file adds to it:
//   ceva_attn_split_kernel, one workgroup per (window block the step can touch, part, b, h): wave s of part p is virtual
//     wave p 4 + s and takes tiles p 4 + s, + 4 parts, ..  -- balanced at any position, no context length on the host.  After
//     the in-LDS merge of its four waves it does not normalise: for each live query it writes (acc[D], m, l) to the workspace.
//     A DEV step always has pad flags, so it reads them without testing the pointer (Pad<false>).
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
// L is the element type of the landmark rows attn_split reads: float, or E on a compact state.  The partials are fp32
// either way, so merge and the workspace layout do not depend on it.

constexpr int WSX = 4;                             // floats behind acc[D] in a workspace row: m, l, 2 unused

template <typename E, int D, bool RING, bool SEQ, typename L>
__global__ __launch_bounds__(NT) void ceva_attn_split_kernel(const DecSplitP sp) {
  const DecP& p = sp.d;
  constexpr int G = D / 4;                         // lanes that share a row of the merged partial
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
  Group gr(p, Rows<RING>{p.ring}, bk, t0 + step.n(p.T));
  gr.qa = max(t0, bk * p.w); gr.nql = min(t0 + step.n(p.T), (bk + 1) * p.w) - gr.qa;
  stage_queries<E, D>(p, b, h, gr, qs[wave], lane);
  float m[QPW], l[QPW];
  f32x4 acc[QPW];
  stream_tiles<E, D, RING, false, L>(p, b, h, gr, part * NW + wave, sp.parts * NW, qs[wave], ps[wave], lane, m, l, acc);
  stash_partial<D>(m, l, acc, mo[wave], ml[wave], lane);
  __syncthreads();
  if (wave != 0) return;
  // the part's partial of each live query: the four waves merged, not normalised
  float* ws = sp.ws + (((size_t)blockIdx.y * QPW + (gr.qa - t0)) * sp.parts + part) * (D + WSX);
  for (int idx = lane; idx < gr.nql * G; idx += 64) {
    const int i = idx / G, c = (idx - i * G) * 4;
    float mx, lt;
    const f32x4 o = merge_waves<D>(mo, ml, 0, NW, i, c, mx, lt);
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
