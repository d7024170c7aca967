// ea_eva_lm.hip -- the landmark (control-variate) columns of non-causal EVA for more than 64 landmarks.
//
// eva.py:200-227 puts a query's local window columns and ALL L landmark columns under one softmax.  The window kernels
// (ea_window_*.hip) park every landmark row in LDS and stop at 64 of them; here the two halves are computed apart and joined
// exactly through their log-sum-exps,
//     Z = logaddexp(lse_loc, lse_lm),   out = e^(lse_loc - Z) o_loc + sum_c e^(s_tc - Z) lv_c,   s_tc = scale q_t . lk_c,
// the window half by the window kernels with L = 0, the landmark half -- dense attention of N queries over L landmark rows, no
// visibility rule, no fill columns, no dropout -- by the kernels of this file:
//   elm_prepare_kernel   : 16-bit images of rf_k_bar / beta, zero rows up to a multiple of 64, once per step
//   elm_query_kernel<F>  : a workgroup walks `walk` consecutive 64-query tiles of one (b, h) (4 waves x 16 queries).  Every
//                          query tile needs every landmark tile: where both images fit 128 KB of LDS they are staged ONCE
//                          per workgroup, during the first query tile's pass, and stay; above that 64-row tiles stream
//                          through two slots.  One loop serves both: step (query tile, landmark tile j) reads slot j
//                          (resident) or slot step & 1 (streamed) and stages the next tile while one is still due.
//                          S^T = K.Q^T on MFMA 16x16x32, online softmax in registers, O^T = V^T.P^T with transposed LDS
//                          reads; the epilogue joins with (o_loc, lse_loc) and writes out and (Z, lse_lm)
//   elm_query_kernel<B>  : same walk and staging; recomputes p = e^(s - Z), dS = p (dout.lv - delta), dq = scale dS.lk;
//                          writes d o_loc, d lse_loc and delta
//   elm_key_kernel       : a workgroup owns (query slice, b, h, 64-landmark tile): lk16 / lv16 fragments resident in
//                          registers, the slice's query tiles (q | dout, Z, delta) stream through two LDS slots;
//                          d lk = scale dS^T.q and d lv = P^T.dout accumulate in registers and leave once, into the slice's
//                          plane -- no atomics; the planes are folded in a fixed order (multi_sum_dispatch)
// Tails: queries >= N load as zero rows with Z = +inf (p = 0) and store nothing; image rows >= L are zero, score s = 0 and are
// masked explicitly (p = 0, outside lse_lm).  A row whose window half holds only -5e4 fills has e^(lse_loc - Z) = 0 exactly.
#include "ea_eva_lm.h"
#include "ea_lm_frag.h"

namespace ea {

static_assert(ELM_TILE == CLM_TILE, "TilePair stages 64-row tiles");

namespace {

template <typename E, int D>
__global__ __launch_bounds__(256) void elm_prepare_kernel(const EvaLmP p) {
  constexpr int CPR = D / 8;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)p.B * p.H * p.Lp * CPR) return;
  const int c = (int)(idx % CPR);
  const size_t rowg = idx / CPR;
  const int row = (int)(rowg % p.Lp);
  const size_t bh = rowg / p.Lp;
  u32x4 kw = {0u, 0u, 0u, 0u}, vw = kw;
  if (row < p.L) {
    const size_t off = (bh * p.L + row) * D + c * 8;
    float fk[8], fv[8];
    *reinterpret_cast<float4*>(fk) = *reinterpret_cast<const float4*>(p.lk + off);
    *reinterpret_cast<float4*>(fk + 4) = *reinterpret_cast<const float4*>(p.lk + off + 4);
    *reinterpret_cast<float4*>(fv) = *reinterpret_cast<const float4*>(p.lv + off);
    *reinterpret_cast<float4*>(fv + 4) = *reinterpret_cast<const float4*>(p.lv + off + 4);
    kw = pack8<E>(fk);
    vw = pack8<E>(fv);
  }
  stg16(const_cast<char*>(p.lk16) + idx * 16, kw);
  stg16(const_cast<char*>(p.lv16) + idx * 16, vw);
}

// four 16-column score pieces of a 64-row tile, packed for the MFMA that consumes them as its K = 32 operand
template <typename E> EA_DEV typename E::x8 pack_pair(const uint32_t (&w)[4][2], int kk) {
  return as_x8<E>(u32x4{w[2 * kk][0], w[2 * kk][1], w[2 * kk + 1][0], w[2 * kk + 1][1]});
}

template <typename E, int D, bool BWD>
__global__ __launch_bounds__(256, 2) void elm_query_kernel(const EvaLmP p) {
  constexpr int ROWB = D * 2, KS = D / 32, DT = D / 16, DQ = D / 4, TB = ELM_TILE * ROWB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  typename LaneOffSel<D>::type lo;
  lo.init(lane);
  const int bh = (int)(blockIdx.x / p.nWQ), wq = (int)(blockIdx.x - (unsigned)bh * p.nWQ);
  const int b = bh / p.H, h = bh - b * p.H;
  const int qt0 = wq * p.walk, qt1 = min(qt0 + p.walk, p.nQT);
  if (qt0 >= qt1) return;
  const int nLT = p.nLT;
  const int nstage = p.resident ? nLT : (qt1 - qt0) * nLT;       // landmark tiles this workgroup brings into LDS
  const char* lkb = p.lk16 + (size_t)bh * p.Lp * ROWB;
  const char* lvb = p.lv16 + (size_t)bh * p.Lp * ROWB;
  auto slot = [&](int step, int j) { return smem + (size_t)(p.resident ? j : (step & 1)) * 2 * TB; };

  TilePair<D> tp;
  tp.load_img(lkb, lvb, 0, tid);
  tp.store(smem, smem + TB, tid);
  __syncthreads();
  int step = 0;
  for (int qt = qt0; qt < qt1; ++qt) {
    // ---- the lane's query: token tok, k-chunks g KS .. of its rows ----
    const int tok = qt * ELM_TILE + wave * 16 + li;
    const bool qv = tok < p.N;
    const int64_t tc = qv ? tok : p.N - 1;
    const size_t row = (size_t)bh * p.N + tc;
    typename E::x8 qf[KS], df[BWD ? KS : 1];
    load_frag<E, KS>(qf, p.q.p + (b * p.q.sb + h * p.q.sh + tc * p.q.sn) * 2, g, qv);
    const float ll = p.lse_loc[row];
    float m = -INFINITY, lsum = 0.f;       // forward: online softmax
    float z2 = INFINITY, dlt = 0.f;        // backward: Z log2(e) (+inf: no such query), delta
    if constexpr (BWD) {
      load_frag<E, KS>(df, p.dout.p + (b * p.dout.sb + h * p.dout.sh + tc * p.dout.sn) * 2, g, qv);
      typename E::x8 of[KS];
      load_frag<E, KS>(of, p.out.p + (b * p.out.sb + h * p.out.sh + tc * p.out.sn) * 2, g, qv);
      dlt = frag_dot<E, KS>(df, of);
      load_frag<E, KS>(of, p.oloc.p + (b * p.oloc.sb + h * p.oloc.sh + tc * p.oloc.sn) * 2, g, qv);
      const float dol = frag_dot<E, KS>(df, of);
      const float Z = p.zl[2 * row];
      const float w_loc = __expf(ll - Z);
      if (qv) {
        z2 = Z * LOG2E;
        char* dst = p.doloc.p + (b * p.doloc.sb + h * p.doloc.sh + tc * p.doloc.sn) * 2;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          float x[8];
          unpack8<E>(__builtin_bit_cast(u32x4, df[ks]), x);
#pragma unroll
          for (int i = 0; i < 8; ++i) x[i] *= w_loc;
          stg16(dst + (g * KS + ks) * 16, pack8<E>(x));
        }
        if (g == 0) {
          p.delta[row] = dlt;
          p.dlse_loc[row] = w_loc * (dol - dlt);
        }
      }
    }
    f32x4 acc[DT];                         // forward: O^T; backward: dq^T
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j = 0; j < nLT; ++j, ++step) {
      const bool stage = step + 1 < nstage;
      const int jn = j + 1 < nLT ? j + 1 : 0;
      if (stage) tp.load_img(lkb, lvb, jn * ELM_TILE, tid);
      const char* Ks = slot(step, j);
      const char* Vs = Ks + TB;
      const bool tail = (j + 1) * ELM_TILE > p.L;          // the tile holds image rows >= L: no such column
      uint32_t pw[4][2];
      if constexpr (!BWD) {
        f32x4 s[4];
        float mloc = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) sc = E::mma(as_x8<E>(lds16(Ks + tt * 16 * ROWB + lo.plain[ks])), qf[ks], sc);
          const int c0 = j * ELM_TILE + tt * 16 + 4 * g;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float x = sc[r] * p.scale_log2;
            if (tail && c0 + r >= p.L) x = -INFINITY;
            sc[r] = x;
            mloc = fmaxf(mloc, x);
          }
          s[tt] = sc;
        }
        // (tile 0 is full -- L > 64 --, so the running maximum is finite from the first step on)
        const float mnew = fmaxf(m, quad_max(mloc));
        const float alpha = fast_exp2(m - mnew);
        m = mnew;
        float psum = 0.f;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          float pv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pv[r] = fast_exp2(s[tt][r] - mnew);
            psum += pv[r];
          }
          pw[tt][0] = pack2<E>(pv[0], pv[1]);
          pw[tt][1] = pack2<E>(pv[2], pv[3]);
        }
        lsum = lsum * alpha + psum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] *= alpha;
      } else {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = sc;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            sc = E::mma(as_x8<E>(lds16(Ks + tt * 16 * ROWB + lo.plain[ks])), qf[ks], sc);
            dp = E::mma(as_x8<E>(lds16(Vs + tt * 16 * ROWB + lo.plain[ks])), df[ks], dp);
          }
          const int c0 = j * ELM_TILE + tt * 16 + 4 * g;
          float ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = fast_exp2(sc[r] * p.scale_log2 - z2);
            if (tail && c0 + r >= p.L) pr = 0.f;
            ds[r] = pr * (dp[r] - dlt);
          }
          pw[tt][0] = pack2<E>(ds[0], ds[1]);
          pw[tt][1] = pack2<E>(ds[2], ds[3]);
        }
      }
      // acc^T[ch][query] += A^T[ch][c] . pw[c][query]: A = lv16 (forward: P), lk16 (backward: dS)
      const char* As = BWD ? Ks : Vs;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const typename E::x8 pf = pack_pair<E>(pw, kk);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const u32x2 lo_ = E::tr4(As + (2 * kk) * 16 * ROWB + lo.tr[dt]);
          const u32x2 hi_ = E::tr4(As + (2 * kk + 1) * 16 * ROWB + lo.tr[dt]);
          acc[dt] = E::mma(as_x8<E>(lo_, hi_), pf, acc[dt]);
        }
      }
      if (stage) {
        char* nx = slot(step + 1, jn);
        tp.store(nx, nx + TB, tid);
        __syncthreads();
      }
    }

    if constexpr (BWD) {
      // ---- dq: lane = query tok, channels acc_chan(dt, g) .. + 3 ----
      if (qv) {
        float* d_ = p.dq + (((size_t)b * p.N + tok) * p.H + h) * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(d_ + acc_chan<D>(dt, g)) = acc[dt] * p.scale;
      }
    } else {
      // ---- join with the window half: lane = query tok, channels DQ g .. DQ g + DQ - 1 ----
      const float ltot = quad_sum(lsum);
      const float lse_lm = (m + fast_log2(ltot)) * LN2;
      const float mx = fmaxf(ll, lse_lm);
      const float Z = mx + __logf(__expf(ll - mx) + __expf(lse_lm - mx));
      const float w_loc = __expf(ll - Z), w_lm = __expf(lse_lm - Z) / ltot;
      float f[DQ];
      if constexpr (TileL<D>::NEWTR) {
        quad_transpose_f32(acc, f);
      } else {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) f[4 * dt + r] = acc[dt][r];
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
        if (g == 0) *reinterpret_cast<float2*>(p.zl + row * 2) = make_float2(Z, lse_lm);
      }
    }
  }
}

// Streamed query row sr and the lane's landmark row rcol: score^T[sr][li] and dP^T[sr][li] from the query rows in LDS, then
// dlk^T[ch][li] += q^T[ch][sr] dS[sr][li] and dlv^T[ch][li] += dout^T[ch][sr] P[sr][li] with the transposed LDS reads.
template <typename E, int D>
__global__ __launch_bounds__(256, 2) void elm_key_kernel(const EvaLmP p) {
  constexpr int ROWB = D * 2, KS = D / 32, DT = D / 16, TB = ELM_TILE * ROWB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* zq = reinterpret_cast<float*>(smem + 4 * TB);     // [2][64] Z log2(e) of the staged queries, then their delta
  float* dq_ = zq + 2 * ELM_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  typename LaneOffSel<D>::type lo;
  lo.init(lane);
  const int BH = p.B * p.H;
  const int lt = (int)(blockIdx.x % p.nLT), rest = (int)(blockIdx.x / p.nLT);
  const int bh = rest % BH, sl = rest / BH;
  const int b = bh / p.H, h = bh - b * p.H;
  const char* qb = p.q.p + (b * p.q.sb + h * p.q.sh) * 2;
  const char* dob = p.dout.p + (b * p.dout.sb + h * p.dout.sh) * 2;
  const int rcol = lt * ELM_TILE + wave * 16 + li;          // the lane's landmark row (rows < Lp exist: zero past L)
  const bool colv = rcol < p.L;
  typename E::x8 kf[KS], vf[KS];
  load_frag<E, KS>(kf, p.lk16 + ((size_t)bh * p.Lp + rcol) * ROWB, g, true);
  load_frag<E, KS>(vf, p.lv16 + ((size_t)bh * p.Lp + rcol) * ROWB, g, true);
  const int first = sl * p.per, end = min(first + p.per, p.nQT);       // this slice's query tiles (none: zeros leave)

  f32x4 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  TilePair<D> tp;
  float pz = INFINITY, pd = 0.f;         // threads < 64: the staged query's Z log2(e) (+inf: no such query) and delta
  auto fetch = [&](int t) {
    tp.load_tok(qb, p.q.sn, dob, p.dout.sn, t * ELM_TILE, p.N, tid);
    const int tk = t * ELM_TILE + tid;
    pz = INFINITY; pd = 0.f;
    if (tid < ELM_TILE && tk < p.N) {
      pz = p.zl[2 * ((size_t)bh * p.N + tk)] * LOG2E;
      pd = p.delta[(size_t)bh * p.N + tk];
    }
  };
  auto park = [&](int buf) {
    tp.store(smem + buf * 2 * TB, smem + buf * 2 * TB + TB, tid);
    if (tid < ELM_TILE) { zq[buf * ELM_TILE + tid] = pz; dq_[buf * ELM_TILE + tid] = pd; }
  };
  if (first < end) { fetch(first); park(0); }
  __syncthreads();
  for (int cur = first, buf = 0; cur < end; ++cur, buf ^= 1) {
    if (cur + 1 < end) fetch(cur + 1);
    const char* Qs = smem + buf * 2 * TB;
    const char* Ds = Qs + TB;
    uint32_t dsw[4][2], pkw[4][2];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = sc;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        sc = E::mma(as_x8<E>(lds16(Qs + tt * 16 * ROWB + lo.plain[ks])), kf[ks], sc);
        dp = E::mma(as_x8<E>(lds16(Ds + tt * 16 * ROWB + lo.plain[ks])), vf[ks], dp);
      }
      const int sr0 = buf * ELM_TILE + tt * 16 + 4 * g;    // streamed rows sr0 .. sr0 + 3
      float pk[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = colv ? fast_exp2(sc[r] * p.scale_log2 - zq[sr0 + r]) : 0.f;
        pk[r] = pr;
        ds[r] = pr * (dp[r] - dq_[sr0 + r]);
      }
      dsw[tt][0] = pack2<E>(ds[0], ds[1]); dsw[tt][1] = pack2<E>(ds[2], ds[3]);
      pkw[tt][0] = pack2<E>(pk[0], pk[1]); pkw[tt][1] = pack2<E>(pk[2], pk[3]);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const typename E::x8 dsf = pack_pair<E>(dsw, kk), pkf = pack_pair<E>(pkw, kk);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int o0 = (2 * kk) * 16 * ROWB + lo.tr[dt], o1 = (2 * kk + 1) * 16 * ROWB + lo.tr[dt];
        dk[dt] = E::mma(as_x8<E>(E::tr4(Qs + o0), E::tr4(Qs + o1)), dsf, dk[dt]);
        dv[dt] = E::mma(as_x8<E>(E::tr4(Ds + o0), E::tr4(Ds + o1)), pkf, dv[dt]);
      }
    }
    if (cur + 1 < end) park(buf ^ 1);
    __syncthreads();
  }

  // ---- every row of the slice's plane leaves once: lane = landmark rcol, channels acc_chan(dt, g) .. + 3 ----
  if (colv) {
    const size_t at = (((size_t)sl * BH + bh) * p.L + rcol) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      *reinterpret_cast<f32x4*>(p.dlk + at + acc_chan<D>(dt, g)) = dk[dt] * p.scale;
      *reinterpret_cast<f32x4*>(p.dlv + at + acc_chan<D>(dt, g)) = dv[dt];
    }
  }
}

template <typename K> int elm_launch(K* kernel, const EvaLmP& p, unsigned grid, size_t lds, hipStream_t st) {
  if (const int e = ea_lds_limit(kernel, lds)) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, p);
  return (int)hipGetLastError();
}

template <typename E, int D>
int elm_run(int which, const EvaLmP& p, hipStream_t st) {
  const unsigned BH = (unsigned)(p.B * p.H);
  constexpr size_t PAIR = (size_t)2 * ELM_TILE * D * 2;    // a 64-row tile of each image
  if (which == 0) {
    const size_t total = (size_t)BH * p.Lp * (D / 8);
    return elm_launch(&elm_prepare_kernel<E, D>, p, (unsigned)((total + 255) / 256), 0, st);
  }
  const size_t lq = p.resident ? (size_t)p.nLT * PAIR : 2 * PAIR;
  if (which == 1) return elm_launch(&elm_query_kernel<E, D, false>, p, BH * p.nWQ, lq, st);
  if (which == 2) return elm_launch(&elm_query_kernel<E, D, true>, p, BH * p.nWQ, lq, st);
  return elm_launch(&elm_key_kernel<E, D>, p, (unsigned)p.S * BH * p.nLT, 2 * PAIR + (size_t)4 * ELM_TILE * 4, st);
}

}  // namespace

int eva_lm_dispatch(int which, const EvaLmP& p, int dtype, int D, hipStream_t st) {
  if (which < 0 || which > 3) return EA_E_UNSUPPORTED;
  if (dtype == EA_BF16) {
    if (D == 64) return elm_run<BF16, 64>(which, p, st);
    if (D == 128) return elm_run<BF16, 128>(which, p, st);
  } else if (dtype == EA_F16) {
    if (D == 64) return elm_run<F16, 64>(which, p, st);
    if (D == 128) return elm_run<F16, 128>(which, p, st);
  }
  return EA_E_UNSUPPORTED;
}

}  // namespace ea
