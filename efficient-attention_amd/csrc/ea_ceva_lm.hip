// ea_ceva_lm.hip -- the landmark (control-variate) columns of causal EVA for sequences of more than 64 chunks.
//
// causal_eva.py:716-783 puts a query's local window columns and its visible landmark columns under one softmax.  The window
// kernels (ea_window_*.hip) park every landmark row in LDS and stop at 64 of them; here the two halves are computed apart
// and joined exactly through their log-sum-exps,
//     Z = logaddexp(lse_loc, lse_lm),   out = e^(lse_loc - Z) o_loc + e^(lse_lm - Z) o_lm,
// the window half by the window kernels with L = 0, the landmark half -- block-lower-triangular attention of N queries over
// L = N / r landmark rows (landmark c is visible to token t iff c < lm_base + t / r; every other landmark column holds the
// finite fill -5e4 with zero gradient, ea_f32_attn.hip's logit_of) -- by the kernels of this file:
//   clm_prepare_kernel : 16-bit images of rf_k_bar / beta, zero rows up to a multiple of 64, once per step
//   clm_fwd_kernel     : a 64-query tile per workgroup (4 waves x 16 queries); 64-row landmark tiles stream through
//                        double-buffered LDS, S^T = K.Q^T on MFMA 16x16x32, online softmax in registers, O^T = V^T.P^T with
//                        transposed LDS reads; the epilogue joins with (o_loc, lse_loc) and writes out and (Z, lse_lm)
//   clm_bwd_kernel<Q>  : same tiling; recomputes p = e^(s - Z), dS = p (dout.lv keep - delta), dq = s dS.lk; writes
//                        d o_loc, d lse_loc and delta
//   clm_bwd_kernel<K>  : a 64-landmark tile per workgroup, query tiles stream through LDS; d lk = s dS^T.q and
//                        d lv = P^T.dout accumulate in registers and every row is stored once (no atomics)
// The two backward kernels are one template: the streamed side (rows in LDS) and the resident side (fragments in registers)
// swap roles.  Work per workgroup grows (query side) or shrinks (key side) linearly with its position: the long ones launch
// first.  A fill column weighs e^(-5e4 - Z): nothing, unless the row has only fills (a padded query that sees no landmark);
// tiles that hold such a row (lse_loc < CLM_DEGENERATE) take every landmark, as the reference's softmax does.
#include "ea_ceva_lm.h"

namespace ea {

namespace {

template <typename E, int D>
__global__ __launch_bounds__(256) void clm_prepare_kernel(const CevaLmP p) {
  constexpr int CPR = D / 8;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)p.B * p.H * p.Lp * CPR;
  if (idx >= total) return;
  const int c = (int)(idx % CPR);
  const size_t rowg = idx / CPR;
  const int row = (int)(rowg % p.Lp);
  const size_t bh = rowg / p.Lp;
  u32x4 kw = {0u, 0u, 0u, 0u}, vw = kw;
  if (row < p.L) {
    const size_t off = (bh * p.L + row) * D + c * 8;
    float f[8], f2[8];
    *reinterpret_cast<float4*>(f) = *reinterpret_cast<const float4*>(p.lk + off);
    *reinterpret_cast<float4*>(f + 4) = *reinterpret_cast<const float4*>(p.lk + off + 4);
    *reinterpret_cast<float4*>(f2) = *reinterpret_cast<const float4*>(p.lv + off);
    *reinterpret_cast<float4*>(f2 + 4) = *reinterpret_cast<const float4*>(p.lv + off + 4);
    kw = pack8<E>(f);
    vw = pack8<E>(f2);
  }
  stg16(const_cast<char*>(p.lk16) + idx * 16, kw);
  stg16(const_cast<char*>(p.lv16) + idx * 16, vw);
}

// landmark tiles a query tile walks: up to its last query's limit, or all of them when it holds a degenerate row
EA_DEV int clm_query_tiles(const CevaLmP& p, int qt, bool degenerate) {
  const int all = p.Lp / CLM_TILE;
  if (degenerate) return all;
  const int limmax = p.lm_base + min(qt * CLM_TILE + CLM_TILE - 1, p.N - 1) / p.r;
  return min(all, (limmax + CLM_TILE - 1) / CLM_TILE);
}

template <typename E, int D, bool DR>
__global__ __launch_bounds__(256, 2) void clm_fwd_kernel(const CevaLmP p) {
  constexpr int ROWB = D * 2, KS = D / 32, DT = D / 16, DQ = D / 4, TB = CLM_TILE * ROWB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  typename LaneOffSel<D>::type lo;
  lo.init(lane);
  const int BH = p.B * p.H;
  const int qt = p.nQT - 1 - (int)(blockIdx.x / BH), bh = (int)(blockIdx.x % BH);
  const int b = bh / p.H, h = bh - b * p.H;
  const int tok = qt * CLM_TILE + wave * 16 + li;
  const bool qv = tok < p.N;
  const int64_t tc = qv ? tok : p.N - 1;
  typename E::x8 qf[KS];
  load_frag<E, KS>(qf, p.q.p + (b * p.q.sb + h * p.q.sh + tc * p.q.sn) * 2, g, qv);
  const float ll = p.lse_loc[(size_t)bh * p.N + tc];
  const int lim = qv ? p.lm_base + tok / p.r : 0;
  const int limmin = p.lm_base + qt * CLM_TILE / p.r;
  const int nt = clm_query_tiles(p, qt, __syncthreads_or(qv && ll < CLM_DEGENERATE));
  const char* lkb = p.lk16 + (size_t)bh * p.Lp * ROWB;
  const char* lvb = p.lv16 + (size_t)bh * p.Lp * ROWB;
  const uint8_t* krow = DR ? p.keep + ((size_t)bh * p.N + tc) * p.keep_ld + 4 * g : nullptr;

  float m = -INFINITY, lsum = 0.f;
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  TilePair<D> tp;
  if (nt > 0) {
    tp.load_img(lkb, lvb, 0, tid);
    tp.store(smem, smem + TB, tid);
  }
  __syncthreads();
  for (int j = 0; j < nt; ++j) {
    const char* Ks = smem + (j & 1) * 2 * TB;
    const char* Vs = Ks + TB;
    if (j + 1 < nt) tp.load_img(lkb, lvb, (j + 1) * CLM_TILE, tid);
    const bool full = j * CLM_TILE + CLM_TILE - 1 < limmin && (j + 1) * CLM_TILE <= p.L;
    f32x4 s[4];
    float mloc = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = E::mma(as_x8<E>(lds16(Ks + tt * 16 * ROWB + lo.plain[ks])), qf[ks], acc);
      const int c0 = j * CLM_TILE + tt * 16 + 4 * g;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = acc[r] * p.scale_log2;
        if (!full) x = c0 + r >= p.L ? -INFINITY : (c0 + r >= lim ? MASK_FILL * LOG2E : x);
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
    uint32_t pw[4][2];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      float pv[4];
      uint32_t k4 = 0x01010101u;
      // (the keep mask's landmark columns end at 16 ceil(L / 16): the zero rows of the image past them have no column)
      if (DR) k4 = j * CLM_TILE + tt * 16 + 16 <= p.keep_ld ? *reinterpret_cast<const uint32_t*>(krow + j * CLM_TILE + tt * 16) : 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pv[r] = fast_exp2(s[tt][r] - msafe);
        psum += pv[r];                                   // the normaliser keeps every column
        if (DR) pv[r] = ((k4 >> (8 * r)) & 0xffu) ? pv[r] * p.keep_scale : 0.f;
      }
      pw[tt][0] = pack2<E>(pv[0], pv[1]);
      pw[tt][1] = pack2<E>(pv[2], pv[3]);
    }
    lsum = lsum * alpha + psum;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
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
    if (j + 1 < nt) tp.store(smem + ((j + 1) & 1) * 2 * TB, smem + ((j + 1) & 1) * 2 * TB + TB, tid);
    __syncthreads();
  }

  // ---- join with the window half: lane = query li, channels DQ g .. DQ g + DQ - 1 ----
  const float ltot = quad_sum(lsum);
  const float lse_lm = ltot > 0.f ? (m + fast_log2(ltot)) * LN2 : -INFINITY;
  const float mx = fmaxf(ll, lse_lm);
  const float Z = mx + __logf(__expf(ll - mx) + __expf(lse_lm - mx));
  const float w_loc = __expf(ll - Z), w_lm = ltot > 0.f ? __expf(lse_lm - Z) / ltot : 0.f;
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
    const char* src = p.oloc.p + (b * p.oloc.sb + h * p.oloc.sh + tc * p.oloc.sn + DQ * g) * 2;
    char* dst = p.out.p + (b * p.out.sb + h * p.out.sh + tc * p.out.sn + DQ * g) * 2;
#pragma unroll
    for (int c = 0; c < DQ / 8; ++c) {
      float ol[8];
      unpack8<E>(ldg16(src + c * 16), ol);
#pragma unroll
      for (int i = 0; i < 8; ++i) ol[i] = w_loc * ol[i] + w_lm * f[8 * c + i];
      stg16(dst + c * 16, pack8<E>(ol));
    }
    if (g == 0) *reinterpret_cast<float2*>(p.zl + ((size_t)bh * p.N + tok) * 2) = make_float2(Z, lse_lm);
  }
}

// KSIDE = false: workgroup = 64-query tile, landmark tiles (lk16 | lv16) stream, q / dout fragments resident -> dq, d o_loc,
//                d lse_loc, delta, the degenerate flag.
// KSIDE = true : workgroup = 64-landmark tile, query tiles (q | dout) stream with their (Z, delta, limit), lk16 / lv16
//                fragments resident -> d lk, d lv.
// Streamed row sr and resident column (lane li): score^T[sr][li] and dP^T[sr][li] from the row operands in LDS, then
// acc1^T[ch][li] += A^T[ch][sr] dS[sr][li] (and acc2^T += B^T P on the key side) with the transposed LDS reads.
template <typename E, int D, bool KSIDE, bool DR>
__global__ __launch_bounds__(256, 2) void clm_bwd_kernel(const CevaLmP p) {
  constexpr int ROWB = D * 2, KS = D / 32, DT = D / 16, TB = CLM_TILE * ROWB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* zq = reinterpret_cast<float*>(smem + 4 * TB);     // key side: [2][64] Z log2(e), then delta, then the limits
  float* dq_ = zq + 2 * CLM_TILE;
  int* lq = reinterpret_cast<int*>(dq_ + 2 * CLM_TILE);
  int* incl = lq + 2 * CLM_TILE;                           // key side: [nQT] this landmark tile walks query tile qt
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  typename LaneOffSel<D>::type lo;
  lo.init(lane);
  const int BH = p.B * p.H;
  const int pos = (int)(blockIdx.x / BH), bh = (int)(blockIdx.x % BH);
  const int b = bh / p.H, h = bh - b * p.H;
  const int me = KSIDE ? pos : p.nQT - 1 - pos;            // this workgroup's landmark tile / query tile
  const char* lkb = p.lk16 + (size_t)bh * p.Lp * ROWB;
  const char* lvb = p.lv16 + (size_t)bh * p.Lp * ROWB;
  const char* qb = p.q.p + (b * p.q.sb + h * p.q.sh) * 2;
  const char* dob = p.dout.p + (b * p.dout.sb + h * p.dout.sh) * 2;

  typename E::x8 r1[KS], r2[KS];         // resident fragments: q | lk16 and dout | lv16 of row (lane li)
  float z2 = INFINITY, dlt = 0.f;        // query side: the lane's query
  int lim = 0, first = 0, end = 0;       // streamed tiles [first, end)
  const int rcol = me * CLM_TILE + wave * 16 + li;          // the lane's query token / landmark row
  if constexpr (!KSIDE) {
    const bool qv = rcol < p.N;
    const int64_t tc = qv ? rcol : p.N - 1;
    load_frag<E, KS>(r1, qb + tc * p.q.sn * 2, g, qv);
    load_frag<E, KS>(r2, dob + tc * p.dout.sn * 2, g, qv);
    typename E::x8 of[KS];
    load_frag<E, KS>(of, p.out.p + (b * p.out.sb + h * p.out.sh + tc * p.out.sn) * 2, g, qv);
    dlt = frag_dot<E, KS>(r2, of);
    load_frag<E, KS>(of, p.oloc.p + (b * p.oloc.sb + h * p.oloc.sh + tc * p.oloc.sn) * 2, g, qv);
    const float dol = frag_dot<E, KS>(r2, of);
    const size_t row = (size_t)bh * p.N + tc;
    const float ll = p.lse_loc[row], Z = p.zl[2 * row];
    const float w_loc = __expf(ll - Z);
    const int deg = __syncthreads_or(qv && ll < CLM_DEGENERATE);
    if (qv) {
      z2 = Z * LOG2E;
      lim = p.lm_base + rcol / p.r;
      char* dst = p.doloc.p + (b * p.doloc.sb + h * p.doloc.sh + tc * p.doloc.sn) * 2;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float x[8];
        unpack8<E>(__builtin_bit_cast(u32x4, r2[ks]), x);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] *= w_loc;
        stg16(dst + (g * KS + ks) * 16, pack8<E>(x));
      }
      if (g == 0) {
        p.delta[row] = dlt;
        p.dlse_loc[row] = w_loc * (dol - dlt);
      }
    }
    if (tid == 0) p.flags[(size_t)bh * p.nQT + me] = deg;
    end = clm_query_tiles(p, me, deg != 0);
  } else {
    load_frag<E, KS>(r1, lkb + (size_t)rcol * ROWB, g, true);       // (rows < Lp exist: zero past L)
    load_frag<E, KS>(r2, lvb + (size_t)rcol * ROWB, g, true);
    // the first query tile with a token that sees this tile's first landmark; earlier tiles only when flagged degenerate
    const long long t0 = (long long)p.r * (me * CLM_TILE + 1 - p.lm_base);
    const int qt0 = t0 <= 0 ? 0 : (t0 / CLM_TILE < p.nQT ? (int)(t0 / CLM_TILE) : p.nQT);
    for (int qt = tid; qt < p.nQT; qt += 256) incl[qt] = (qt >= qt0 || p.flags[(size_t)bh * p.nQT + qt]) ? 1 : 0;
    __syncthreads();
    end = p.nQT;
    while (first < end && !incl[first]) ++first;
  }
  auto next_tile = [&](int t) {
    ++t;
    if constexpr (KSIDE) while (t < end && !incl[t]) ++t;
    return t;
  };

  f32x4 acc1[DT], acc2[KSIDE ? DT : 1];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc1[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dt = 0; dt < (KSIDE ? DT : 1); ++dt) acc2[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  TilePair<D> tp;
  float pz = INFINITY, pd = 0.f;         // key side, threads < 64: the staged query's Z log2(e), delta, limit
  int pl = 0;
  auto fetch = [&](int t) {
    if constexpr (KSIDE) {
      tp.load_tok(qb, p.q.sn, dob, p.dout.sn, t * CLM_TILE, p.N, tid);
      const int tk = t * CLM_TILE + tid;
      pz = INFINITY; pd = 0.f; pl = 0;
      if (tid < CLM_TILE && tk < p.N) {
        pz = p.zl[2 * ((size_t)bh * p.N + tk)] * LOG2E;
        pd = p.delta[(size_t)bh * p.N + tk];
        pl = p.lm_base + tk / p.r;
      }
    } else {
      tp.load_img(lkb, lvb, t * CLM_TILE, tid);
    }
  };
  auto park = [&](int buf) {
    tp.store(smem + buf * 2 * TB, smem + buf * 2 * TB + TB, tid);
    if constexpr (KSIDE)
      if (tid < CLM_TILE) { zq[buf * CLM_TILE + tid] = pz; dq_[buf * CLM_TILE + tid] = pd; lq[buf * CLM_TILE + tid] = pl; }
  };
  int cur = first, buf = 0;
  if (cur < end) { fetch(cur); park(0); }
  __syncthreads();
  while (cur < end) {
    const int nxt = next_tile(cur);
    if (nxt < end) fetch(nxt);
    const char* As = smem + buf * 2 * TB;
    const char* Bs = As + TB;
    // no entry of the tile pair is masked: every query exists and sees every landmark row, all of which exist
    const int qtile = KSIDE ? cur : me, ltile = KSIDE ? me : cur;
    const bool full = qtile * CLM_TILE + CLM_TILE <= p.N && (ltile + 1) * CLM_TILE <= p.L &&
                      ltile * CLM_TILE + CLM_TILE - 1 < p.lm_base + qtile * CLM_TILE / p.r;
    uint32_t dsw[4][2], pkw[4][2];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = sc;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        sc = E::mma(as_x8<E>(lds16(As + tt * 16 * ROWB + lo.plain[ks])), r1[ks], sc);
        dp = E::mma(as_x8<E>(lds16(Bs + tt * 16 * ROWB + lo.plain[ks])), r2[ks], dp);
      }
      const int sr0 = tt * 16 + 4 * g;                   // streamed rows sr0 .. sr0 + 3
      float zr[4], dr[4], kf[4] = {1.f, 1.f, 1.f, 1.f};
      int lr[4], cr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (KSIDE) {
          zr[r] = zq[buf * CLM_TILE + sr0 + r]; dr[r] = dq_[buf * CLM_TILE + sr0 + r]; lr[r] = lq[buf * CLM_TILE + sr0 + r];
          cr[r] = rcol;
        } else {
          zr[r] = z2; dr[r] = dlt; lr[r] = lim;
          cr[r] = cur * CLM_TILE + sr0 + r;
        }
      }
      if constexpr (DR) {
        if constexpr (KSIDE) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int tk = min(cur * CLM_TILE + sr0 + r, p.N - 1);
            kf[r] = (rcol < p.keep_ld && p.keep[((size_t)bh * p.N + tk) * p.keep_ld + rcol]) ? p.keep_scale : 0.f;
          }
        } else {
          const int tk = min(rcol, p.N - 1);
          const int c0 = cur * CLM_TILE + tt * 16;
          const uint32_t k4 = c0 + 16 <= p.keep_ld
              ? *reinterpret_cast<const uint32_t*>(p.keep + ((size_t)bh * p.N + tk) * p.keep_ld + c0 + 4 * g) : 0u;
#pragma unroll
          for (int r = 0; r < 4; ++r) kf[r] = ((k4 >> (8 * r)) & 0xffu) ? p.keep_scale : 0.f;
        }
      }
      float pk[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = sc[r] * p.scale_log2;
        bool live = true;
        if (!full) {
          live = cr[r] < p.L && cr[r] < lr[r];
          x = cr[r] >= p.L ? -INFINITY : (live ? x : MASK_FILL * LOG2E);
        }
        const float pr = fast_exp2(x - zr[r]);           // (a query that does not exist carries Z = +inf: 0)
        pk[r] = pr * kf[r];
        ds[r] = live ? pr * (dp[r] * kf[r] - dr[r]) : 0.f;
      }
      dsw[tt][0] = pack2<E>(ds[0], ds[1]); dsw[tt][1] = pack2<E>(ds[2], ds[3]);
      pkw[tt][0] = pack2<E>(pk[0], pk[1]); pkw[tt][1] = pack2<E>(pk[2], pk[3]);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const typename E::x8 dsf = as_x8<E>(u32x4{dsw[2 * kk][0], dsw[2 * kk][1], dsw[2 * kk + 1][0], dsw[2 * kk + 1][1]});
      const typename E::x8 pkf = as_x8<E>(u32x4{pkw[2 * kk][0], pkw[2 * kk][1], pkw[2 * kk + 1][0], pkw[2 * kk + 1][1]});
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int o0 = (2 * kk) * 16 * ROWB + lo.tr[dt], o1 = (2 * kk + 1) * 16 * ROWB + lo.tr[dt];
        acc1[dt] = E::mma(as_x8<E>(E::tr4(As + o0), E::tr4(As + o1)), dsf, acc1[dt]);
        if constexpr (KSIDE) acc2[dt] = E::mma(as_x8<E>(E::tr4(Bs + o0), E::tr4(Bs + o1)), pkf, acc2[dt]);
      }
    }
    if (nxt < end) park(buf ^ 1);
    __syncthreads();
    cur = nxt;
    buf ^= 1;
  }

  // ---- every row leaves once: lane = row rcol, channels acc_chan(dt, g) .. + 3 ----
  if constexpr (KSIDE) {
    if (rcol < p.L) {
      float* dk_ = p.dlk + ((size_t)bh * p.L + rcol) * D;
      float* dv_ = p.dlv + ((size_t)bh * p.L + rcol) * D;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f32x4 a = acc1[dt] * p.scale;
        *reinterpret_cast<f32x4*>(dk_ + acc_chan<D>(dt, g)) = a;
        *reinterpret_cast<f32x4*>(dv_ + acc_chan<D>(dt, g)) = acc2[dt];
      }
    }
  } else if (rcol < p.N) {
    float* d_ = p.dq + (((size_t)b * p.N + rcol) * p.H + h) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const f32x4 a = acc1[dt] * p.scale;
      *reinterpret_cast<f32x4*>(d_ + acc_chan<D>(dt, g)) = a;
    }
  }
}

template <int D> size_t clm_lds(bool kside) {
  return (size_t)4 * CLM_TILE * D * 2 + (kside ? (size_t)6 * CLM_TILE * 4 + CLM_MAX_QT * 4 : 0);
}

template <typename K> int clm_launch(K* kernel, const CevaLmP& p, unsigned grid, size_t lds, hipStream_t st) {
  if (const int e = ea_lds_limit(kernel, lds)) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, p);
  return (int)hipGetLastError();
}

template <typename E, int D>
int clm_run(int which, const CevaLmP& p, hipStream_t st) {
  const unsigned BH = (unsigned)(p.B * p.H);
  if (which == 0) {
    const size_t total = (size_t)BH * p.Lp * (D / 8);
    return clm_launch(&clm_prepare_kernel<E, D>, p, (unsigned)((total + 255) / 256), 0, st);
  }
  const unsigned gq = BH * p.nQT, gk = BH * (p.Lp / CLM_TILE);
  if (which == 1)
    return p.keep ? clm_launch(&clm_fwd_kernel<E, D, true>, p, gq, clm_lds<D>(false), st)
                  : clm_launch(&clm_fwd_kernel<E, D, false>, p, gq, clm_lds<D>(false), st);
  if (which == 2)
    return p.keep ? clm_launch(&clm_bwd_kernel<E, D, false, true>, p, gq, clm_lds<D>(false), st)
                  : clm_launch(&clm_bwd_kernel<E, D, false, false>, p, gq, clm_lds<D>(false), st);
  return p.keep ? clm_launch(&clm_bwd_kernel<E, D, true, true>, p, gk, clm_lds<D>(true), st)
                : clm_launch(&clm_bwd_kernel<E, D, true, false>, p, gk, clm_lds<D>(true), st);
}

}  // namespace

int ceva_lm_dispatch(int which, const CevaLmP& p, int dtype, int D, hipStream_t st) {
  if (which < 0 || which > 3 || p.nQT > CLM_MAX_QT) return EA_E_UNSUPPORTED;
  if (dtype == EA_BF16) {
    if (D == 64) return clm_run<BF16, 64>(which, p, st);
    if (D == 128) return clm_run<BF16, 128>(which, p, st);
  } else if (dtype == EA_F16) {
    if (D == 64) return clm_run<F16, 64>(which, p, st);
    if (D == 128) return clm_run<F16, 128>(which, p, st);
  }
  return EA_E_UNSUPPORTED;
}

}  // namespace ea
