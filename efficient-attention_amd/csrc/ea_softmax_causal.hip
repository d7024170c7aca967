// ea_softmax_causal.hip -- the softmax baseline of the language model (fairseq's causal MultiheadAttention, the attention
// causal EVA is compared against): softmax(s QK^T, -inf above the diagonal and on padded keys) V as streaming kernels with a
// triangular schedule.  The dataflow is ea_softmax.hip's (K/V or Q/dO through LDS in 64-row chunks with the next chunk's loads in
// flight, S^T tiles on MFMA 16x16x32, online softmax in registers, ds_read_b64_tr_b16 fragments for the second product); these
// are templates of their own, so the dense kernels' code does not move.
//
//   fwd     : workgroup = 64 QT queries, a wave owns QT tiles of 16.  It walks the key chunks 0 .. ceil((last query + 1) / 64) - 1.
//             Chunks that end at or below the workgroup's first query run the branch-free bodies (MODE 0: no padding mask,
//             scale folded into the shift; MODE 1: additive -inf from kadd_s).  The QT chunks that cross the diagonal run MODE 2:
//             per wave and per 16-key sub-tile, a sub-tile wholly above a query tile is skipped (both MFMAs, the exponentials,
//             its share of P.V; the test is wave-uniform), the sub-tile on the diagonal gets `key > query -> -inf` per element,
//             sub-tiles below are plain.
//   bwd_dq  : the same walk and bodies; writes delta = dO . O, P from the saved lse, dS^T = P o (keep dP - delta), dQ^T = K^T dS^T
//   bwd_dkv : workgroup = 64 KT keys; (q | dout) chunks with (lse, delta) stream from the chunk that holds the tile's first key
//             to the end of the sequence: the first KT chunks take the diagonal body, the rest the plain one.  dV^T = dO^T P and
//             dK^T = Q^T dS stay in registers, every row is stored once: no atomics, two runs agree bit for bit.
// Work grows linearly with the block's position: the heaviest workgroups come first in the grid (late query blocks, early key
// blocks).  Barriers stay workgroup-wide; waves that skip sub-tiles wait there.
// A query whose visible keys are all padded has an empty softmax: its out is NaN, as in the reference and in the dense kernel
// (this takes left padding; right padding never does it).
#include <type_traits>
#include "ea_softmax_causal.h"

namespace ea {

template <int M> using smc_mode = std::integral_constant<int, M>;

// sub-tiles (of 16 keys, from the chunk's first) a 16-query tile starting at q0 sees of the chunk starting at kc: 0 .. 4
EA_DEV int smc_visible(int q0, int kc) { return min(max((q0 - kc) / 16 + 1, 0), 4); }

template <typename E, int D, bool DR, int QT>
__global__ __launch_bounds__(256, 2) void smc_fwd_kernel(const SmcP p) {
  constexpr int ROWB = D * 2, CPR = D / 8, KS = D / 32, DT = D / 16, DQ = D / 4;
  __shared__ __attribute__((aligned(16))) char Ks[64 * ROWB];
  __shared__ __attribute__((aligned(16))) char Vs[64 * ROWB];
  __shared__ __attribute__((aligned(16))) float kadd_s[64];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int QPB = 64 * QT;                       // queries per workgroup
  const int nqb = (p.N + QPB - 1) / QPB, BH = p.B * p.H;
  const int qb = nqb - 1 - (int)(blockIdx.x / BH), bh = (int)(blockIdx.x % BH);      // heaviest first
  const int b = bh / p.H, h = bh - b * p.H;
  const char* qbase = p.q.p + (b * p.q.sb + h * p.q.sh) * 2;
  const char* kbase = p.k.p + (b * p.k.sb + h * p.k.sh) * 2;
  const char* vbase = p.v.p + (b * p.v.sb + h * p.v.sh) * 2;
  const uint8_t* mrow = p.mask ? p.mask + (size_t)b * p.N : nullptr;
  const int q0 = qb * QPB, kend = min(q0 + QPB, p.N);        // keys [0, kend): nothing beyond the last query
  int qt0[QT], qtok[QT];
  bool qvalid[QT];
  typename E::x8 qf[QT][KS];
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    qt0[u] = q0 + (wave * QT + u) * 16;
    qtok[u] = qt0[u] + li;
    qvalid[u] = qtok[u] < p.N;
    const int tq = min(qtok[u], p.N - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4 w = ldg16(qbase + (tq * p.q.sn + (g * KS + ks) * 8) * 2);
      qf[u][ks] = as_x8<E>(qvalid[u] ? w : u32x4{0u, 0u, 0u, 0u});
    }
  }
  float m[QT], lsum[QT];
  f32x4 o[QT][DT];
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    m[u] = -INFINITY; lsum[u] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // the next chunk's K/V rows are in flight (registers) while this chunk computes; loads are unconditional from clamped rows
  // (the padding bytes are read when the chunk is committed: they would cost NSL more live registers here)
  constexpr int NSL = (64 * CPR + 255) / 256;
  u32x4 nk[NSL], nv[NSL];
  auto issue = [&](int kc_) {
#pragma unroll
    for (int i = 0; i < NSL; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / CPR, c = idx - row * CPR;
      const int tok = min(kc_ + row, p.N - 1);
      nk[i] = ldg16(kbase + (tok * p.k.sn + c * 8) * 2);
      nv[i] = ldg16(vbase + (tok * p.v.sn + c * 8) * 2);
    }
  };
  // One 64-key chunk; MODE is a template tag so that each loop below carries one straight-line body.
  auto chunk = [&](auto mode_tag, int kc) {
    constexpr int MODE = decltype(mode_tag)::value;
    int nt[QT];                                      // (MODE 2) sub-tiles of this chunk the query tile sees
#pragma unroll
    for (int u = 0; u < QT; ++u) nt[u] = MODE == 2 ? smc_visible(qt0[u], kc) : 4;
    const int ntmax = nt[QT - 1];                    // the wave's last tile sees the most
    // Where the accumulators, the query fragments and QT score tiles of 64 keys do not fit 256 VGPRs together (QT D = 256),
    // the chunk goes through the online softmax as two halves of 32 keys: half the score registers, one more rescale test.
    constexpr int NH = QT * D >= 256 ? 2 : 1, TH = 4 / NH;
    // ... and with the keep-mask reads on top, one query tile at a time (the K fragments are read from LDS once per tile)
    constexpr int UG = (DR && QT * D >= 256) ? 1 : QT;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      if (MODE == 2 && hf * TH >= ntmax) continue;
      uint32_t pw[QT][TH][2];
#pragma unroll
      for (int u0 = 0; u0 < QT; u0 += UG) {
        const int ntg = nt[u0 + UG - 1];
        if (MODE == 2 && hf * TH >= ntg) continue;
        f32x4 s[UG][TH];
        float mloc[UG];
#pragma unroll
        for (int u = 0; u < UG; ++u) mloc[u] = -INFINITY;
#pragma unroll
        for (int t = 0; t < TH; ++t) {
          const int tt = hf * TH + t;
          if (MODE == 2 && tt >= ntg) continue;
          const int row = tt * 16 + li;
#pragma unroll
          for (int u = 0; u < UG; ++u) s[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const typename E::x8 kfr = as_x8<E>(lds16(Ks + TileL<D>::off(row, g * KS + ks)));
#pragma unroll
            for (int u = u0; u < u0 + UG; ++u)
              if (MODE != 2 || tt < nt[u]) s[u - u0][t] = E::mma(kfr, qf[u][ks], s[u - u0][t]);
          }
          if constexpr (MODE == 0) {
#pragma unroll
            for (int u = 0; u < UG; ++u)
#pragma unroll
              for (int r = 0; r < 4; ++r) mloc[u] = fmaxf(mloc[u], s[u][t][r]);
          } else {
            const float4 ka4 = *reinterpret_cast<const float4*>(kadd_s + tt * 16 + 4 * g);
            const float kav[4] = {ka4.x, ka4.y, ka4.z, ka4.w};
#pragma unroll
            for (int u = u0; u < u0 + UG; ++u) {
              if (MODE == 2 && tt >= nt[u]) continue;
              const bool diag = MODE == 2 && qt0[u] - kc == tt * 16;        // (wave-uniform) the sub-tile on the diagonal
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float add = (diag && 4 * g + r > li) ? -INFINITY : kav[r];      // key > query
                const float x = fmaf(s[u - u0][t][r], p.scale_log2, add);
                s[u - u0][t][r] = x;
                mloc[u - u0] = fmaxf(mloc[u - u0], x);
              }
            }
          }
        }
#pragma unroll
        for (int u = u0; u < u0 + UG; ++u) {
          if (MODE == 2 && hf * TH >= nt[u]) continue;
          float ml = quad_max(mloc[u - u0]);
          if (MODE == 0) ml *= p.scale_log2;                 // (scale > 0: the maximum commutes with it)
          const float mnew = fmaxf(m[u], ml);
          const float msafe = mnew == -INFINITY ? 0.f : mnew;
          // the rescale of the accumulators is skipped when no lane of the wave needs it -- alpha is exactly 1 there
          const bool moved = mnew != m[u];
          const float alpha = fast_exp2(m[u] - msafe);
          m[u] = mnew;
          float psum = 0.f;
          const uint8_t* krow = DR ? p.keep + ((size_t)bh * p.N + (qvalid[u] ? qtok[u] : 0)) * p.keep_ld + kc + 4 * g : nullptr;
          const float sc = MODE == 0 ? p.scale_log2 : 1.f;
#pragma unroll
          for (int t = 0; t < TH; ++t) {
            const int tt = hf * TH + t;
            if (MODE == 2 && tt >= nt[u]) { pw[u][t][0] = 0u; pw[u][t][1] = 0u; continue; }
            uint32_t k4 = 0;
            if (DR) k4 = *reinterpret_cast<const uint32_t*>(krow + tt * 16);
            float pr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              pr[r] = fast_exp2(fmaf(s[u - u0][t][r], sc, -msafe));
              psum += pr[r];
              if (DR) pr[r] = ((k4 >> (8 * r)) & 0xffu) ? pr[r] * p.keep_scale : 0.f;
            }
            pw[u][t][0] = pack2<E>(pr[0], pr[1]);
            pw[u][t][1] = pack2<E>(pr[2], pr[3]);
          }
          if (__any(moved)) {
            lsum[u] = lsum[u] * alpha + psum;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[u][dt] *= alpha;
          } else {
            lsum[u] += psum;
          }
        }
      }
#pragma unroll
      for (int k2 = 0; k2 < TH / 2; ++k2) {
        const int kk = hf * (TH / 2) + k2;
        if (MODE == 2 && 2 * kk >= ntmax) continue;
        typename E::x8 pf[QT];
#pragma unroll
        for (int u = 0; u < QT; ++u) {
          if (MODE == 2 && 2 * kk >= nt[u]) continue;
          u32x4 pf4;
          pf4[0] = pw[u][2 * k2][0]; pf4[1] = pw[u][2 * k2][1]; pf4[2] = pw[u][2 * k2 + 1][0]; pf4[3] = pw[u][2 * k2 + 1][1];
          pf[u] = as_x8<E>(pf4);
        }
        const int r0 = 32 * kk + 4 * g + (li >> 2), r1 = r0 + 16;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const u32x2 lo = E::tr4(Vs + tile_tr<D>(r0, li, dt));
          const u32x2 hi = E::tr4(Vs + tile_tr<D>(r1, li, dt));
          const typename E::x8 vfr = as_x8<E>(lo, hi);
#pragma unroll
          for (int u = 0; u < QT; ++u)
            if (MODE != 2 || 2 * kk < nt[u]) o[u][dt] = E::mma(vfr, pf[u], o[u][dt]);
        }
      }
    }
  };
  // The chunk loop, once per body.  Rows past the sequence exist only in the last chunk, which is a diagonal one.
  auto run = [&](auto mode_tag, int kc0, int kc1) {
    constexpr int MODE = decltype(mode_tag)::value;
    for (int kc = kc0; kc < kc1; kc += 64) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NSL; ++i) {
        const int idx = tid + i * 256;
        const int row = idx / CPR, c = idx - row * CPR;
        if (64 * CPR % 256 != 0 && idx >= 64 * CPR) continue;
        const bool in = MODE != 2 || kc + row < p.N;
        u32x4 kw = nk[i], vw = nv[i];
        if (MODE == 2) {
          const u32x4 z = {0u, 0u, 0u, 0u};
          kw = in ? kw : z; vw = in ? vw : z;
        }
        sts16(Ks + TileL<D>::off(row, c), kw);
        sts16(Vs + TileL<D>::off(row, c), vw);
        if (MODE != 0 && c == 0) kadd_s[row] = (!in || (mrow && mrow[kc + row])) ? -INFINITY : 0.f;
      }
      __syncthreads();
      if (kc + 64 < kend) issue(kc + 64);
      chunk(mode_tag, kc);
    }
  };
  issue(0);
  if (mrow) run(smc_mode<1>{}, 0, q0); else run(smc_mode<0>{}, 0, q0);
  run(smc_mode<2>{}, q0, kend);
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    const float ltot = quad_sum(lsum[u]);
    const float inv = fast_rcp(ltot);
    float f[DQ];
    if constexpr (TileL<D>::NEWTR) {
      quad_transpose_f32(o[u], f);                // accumulator pieces -> the lane's contiguous channels (all lanes)
#pragma unroll
      for (int j = 0; j < DQ; ++j) f[j] *= inv;
    } else {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) f[4 * dt + r] = o[u][dt][r] * inv;
    }
    if (qvalid[u]) {
      char* dst = p.o.p + (b * p.o.sb + h * p.o.sh + qtok[u] * p.o.sn + DQ * g) * 2;
#pragma unroll
      for (int c = 0; c < DQ / 8; ++c) stg16(dst + c * 16, pack8<E>(f + 8 * c));
      if (g == 0) p.lse[(size_t)bh * p.N + qtok[u]] = (m[u] + fast_log2(ltot)) * LN2;
    }
  }
}

template <typename E, int D, bool DR, int QT>
__global__ __launch_bounds__(256) void smc_bwd_dq_kernel(const SmcP p) {
  constexpr int ROWB = D * 2, CPR = D / 8, KS = D / 32, DT = D / 16, DQ = D / 4;
  __shared__ __attribute__((aligned(16))) char Ks[64 * ROWB];
  __shared__ __attribute__((aligned(16))) char Vs[64 * ROWB];
  __shared__ __attribute__((aligned(16))) float kadd_s[64];     // -inf on padded / out-of-range keys
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int QPB = 64 * QT;
  const int nqb = (p.N + QPB - 1) / QPB, BH = p.B * p.H;
  const int qb = nqb - 1 - (int)(blockIdx.x / BH), bh = (int)(blockIdx.x % BH);      // heaviest first
  const int b = bh / p.H, h = bh - b * p.H;
  const char* kbase = p.k.p + (b * p.k.sb + h * p.k.sh) * 2;
  const char* vbase = p.v.p + (b * p.v.sb + h * p.v.sh) * 2;
  const uint8_t* mrow = p.mask ? p.mask + (size_t)b * p.N : nullptr;
  const int q0 = qb * QPB, kend = min(q0 + QPB, p.N);
  int qt0[QT], qtok[QT];
  bool qvalid[QT];
  typename E::x8 qf[QT][KS], dof[QT][KS];
  float delta[QT], lse2[QT];
  f32x4 dq[QT][DT];
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    qt0[u] = q0 + (wave * QT + u) * 16;
    qtok[u] = qt0[u] + li;
    qvalid[u] = qtok[u] < p.N;
    const int tq = min(qtok[u], p.N - 1);
    delta[u] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int eo = (g * KS + ks) * 8;
      const u32x4 z = {0u, 0u, 0u, 0u};
      u32x4 w = ldg16(p.q.p + (b * p.q.sb + h * p.q.sh + tq * p.q.sn + eo) * 2);
      u32x4 dw = ldg16(p.dout.p + (b * p.dout.sb + h * p.dout.sh + tq * p.dout.sn + eo) * 2);
      u32x4 ow = ldg16(p.o.p + (b * p.o.sb + h * p.o.sh + tq * p.o.sn + eo) * 2);
      w = qvalid[u] ? w : z; dw = qvalid[u] ? dw : z; ow = qvalid[u] ? ow : z;
      qf[u][ks] = as_x8<E>(w);
      dof[u][ks] = as_x8<E>(dw);
      float a8[8], c8[8];
      unpack8<E>(dw, a8);
      unpack8<E>(ow, c8);
#pragma unroll
      for (int i = 0; i < 8; ++i) delta[u] += a8[i] * c8[i];
    }
    delta[u] = quad_sum(delta[u]);
    lse2[u] = qvalid[u] ? p.lse[(size_t)bh * p.N + qtok[u]] * LOG2E : INFINITY;
    if (qvalid[u] && g == 0) p.delta[(size_t)bh * p.N + qtok[u]] = delta[u];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  constexpr int NSL = (64 * CPR + 255) / 256;
  u32x4 nk[NSL], nv[NSL];
  uint8_t nm[NSL];
  auto issue = [&](int kc_) {
#pragma unroll
    for (int i = 0; i < NSL; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / CPR, c = idx - row * CPR;
      const int tok = min(kc_ + row, p.N - 1);
      nk[i] = ldg16(kbase + (tok * p.k.sn + c * 8) * 2);
      nv[i] = ldg16(vbase + (tok * p.v.sn + c * 8) * 2);
      nm[i] = mrow ? mrow[tok] : (uint8_t)0;
    }
  };
  auto chunk = [&](auto mode_tag, int kc) {
    constexpr int MODE = decltype(mode_tag)::value;
    int nt[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) nt[u] = MODE == 2 ? smc_visible(qt0[u], kc) : 4;
    const int ntmax = nt[QT - 1];
    uint32_t dsw[QT][4][2];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      if (MODE == 2 && tt >= ntmax) {
#pragma unroll
        for (int u = 0; u < QT; ++u) { dsw[u][tt][0] = 0u; dsw[u][tt][1] = 0u; }
        continue;
      }
      f32x4 s[QT], dp[QT];
#pragma unroll
      for (int u = 0; u < QT; ++u) { s[u] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[u] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      const int row = tt * 16 + li;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const typename E::x8 kfr = as_x8<E>(lds16(Ks + TileL<D>::off(row, g * KS + ks)));
        const typename E::x8 vfr = as_x8<E>(lds16(Vs + TileL<D>::off(row, g * KS + ks)));
#pragma unroll
        for (int u = 0; u < QT; ++u) {
          if (MODE == 2 && tt >= nt[u]) continue;
          s[u] = E::mma(kfr, qf[u][ks], s[u]);
          dp[u] = E::mma(vfr, dof[u][ks], dp[u]);
        }
      }
      float kav[4] = {0.f, 0.f, 0.f, 0.f};
      if (MODE != 0) {
        const float4 ka4 = *reinterpret_cast<const float4*>(kadd_s + tt * 16 + 4 * g);
        kav[0] = ka4.x; kav[1] = ka4.y; kav[2] = ka4.z; kav[3] = ka4.w;
      }
#pragma unroll
      for (int u = 0; u < QT; ++u) {
        if (MODE == 2 && tt >= nt[u]) { dsw[u][tt][0] = 0u; dsw[u][tt][1] = 0u; continue; }
        const bool diag = MODE == 2 && qt0[u] - kc == tt * 16;
        uint32_t k4 = 0;
        if (DR) k4 = *reinterpret_cast<const uint32_t*>(
                    p.keep + ((size_t)bh * p.N + (qvalid[u] ? qtok[u] : 0)) * p.keep_ld + kc + tt * 16 + 4 * g);
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // (lse2 = +inf on rows past the sequence, kav = -inf on dead keys: either way exp2(-inf) = 0)
          float pr = MODE == 0 ? fast_exp2(fmaf(s[u][r], p.scale_log2, -lse2[u]))
                               : fast_exp2(fmaf(s[u][r], p.scale_log2, kav[r]) - lse2[u]);
          if (diag && 4 * g + r > li) pr = 0.f;                              // key > query
          float dpr = dp[u][r];
          if (DR) dpr = ((k4 >> (8 * r)) & 0xffu) ? dpr * p.keep_scale : 0.f;
          ds[r] = pr * (dpr - delta[u]);
        }
        dsw[u][tt][0] = pack2<E>(ds[0], ds[1]);
        dsw[u][tt][1] = pack2<E>(ds[2], ds[3]);
      }
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (MODE == 2 && 2 * kk >= ntmax) continue;
      typename E::x8 dsf[QT];
#pragma unroll
      for (int u = 0; u < QT; ++u) {
        u32x4 f4v;
        f4v[0] = dsw[u][2 * kk][0]; f4v[1] = dsw[u][2 * kk][1]; f4v[2] = dsw[u][2 * kk + 1][0]; f4v[3] = dsw[u][2 * kk + 1][1];
        dsf[u] = as_x8<E>(f4v);
      }
      const int r0 = 32 * kk + 4 * g + (li >> 2), r1 = r0 + 16;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const u32x2 lo = E::tr4(Ks + tile_tr<D>(r0, li, dt));
        const u32x2 hi = E::tr4(Ks + tile_tr<D>(r1, li, dt));
        const typename E::x8 kt = as_x8<E>(lo, hi);
#pragma unroll
        for (int u = 0; u < QT; ++u)
          if (MODE != 2 || 2 * kk < nt[u]) dq[u][dt] = E::mma(kt, dsf[u], dq[u][dt]);
      }
    }
  };
  auto run = [&](auto mode_tag, int kc0, int kc1) {
    constexpr int MODE = decltype(mode_tag)::value;
    for (int kc = kc0; kc < kc1; kc += 64) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NSL; ++i) {
        const int idx = tid + i * 256;
        const int row = idx / CPR, c = idx - row * CPR;
        if (64 * CPR % 256 != 0 && idx >= 64 * CPR) continue;
        const bool in = MODE != 2 || kc + row < p.N;
        u32x4 kw = nk[i], vw = nv[i];
        if (MODE == 2) {
          const u32x4 z = {0u, 0u, 0u, 0u};
          kw = in ? kw : z; vw = in ? vw : z;
        }
        sts16(Ks + TileL<D>::off(row, c), kw);
        sts16(Vs + TileL<D>::off(row, c), vw);
        if (MODE != 0 && c == 0) kadd_s[row] = (!in || nm[i]) ? -INFINITY : 0.f;
      }
      __syncthreads();
      if (kc + 64 < kend) issue(kc + 64);
      chunk(mode_tag, kc);
    }
  };
  issue(0);
  if (mrow) run(smc_mode<1>{}, 0, q0); else run(smc_mode<0>{}, 0, q0);
  run(smc_mode<2>{}, q0, kend);
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    float f[DQ];
    if constexpr (TileL<D>::NEWTR) {
      quad_transpose_f32(dq[u], f);
#pragma unroll
      for (int j = 0; j < DQ; ++j) f[j] *= p.scale;
    } else {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) f[4 * dt + r] = dq[u][dt][r] * p.scale;
    }
    if (qvalid[u]) {
      char* dst = p.dq.p + (b * p.dq.sb + h * p.dq.sh + qtok[u] * p.dq.sn + DQ * g) * 2;
#pragma unroll
      for (int c = 0; c < DQ / 8; ++c) stg16(dst + c * 16, pack8<E>(f + 8 * c));
    }
  }
}

// KT: 16-key tiles per wave: the Q / dO fragments a wave reads from LDS (plain and transposed) feed KT MFMAs each
template <typename E, int D, bool DR, int KT>
__global__ __launch_bounds__(256) void smc_bwd_dkv_kernel(const SmcP p) {
  constexpr int ROWB = D * 2, CPR = D / 8, KS = D / 32, DT = D / 16, DQ = D / 4;
  __shared__ __attribute__((aligned(16))) char Qs[64 * ROWB];
  __shared__ __attribute__((aligned(16))) char dOs[64 * ROWB];
  __shared__ __attribute__((aligned(16))) float lse_s[64];
  __shared__ __attribute__((aligned(16))) float delta_s[64];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int KPB = 64 * KT;                       // keys per workgroup
  const int BH = p.B * p.H;
  const int kb = (int)(blockIdx.x / BH), bh = (int)(blockIdx.x % BH);      // early key tiles are the long ones: first
  const int b = bh / p.H, h = bh - b * p.H;
  const char* qbase = p.q.p + (b * p.q.sb + h * p.q.sh) * 2;
  const char* dobase = p.dout.p + (b * p.dout.sb + h * p.dout.sh) * 2;
  const int k0 = kb * KPB;
  int kt0[KT], ktok[KT];
  bool kvalid[KT], kdead[KT];
  typename E::x8 kf[KT][KS], vf[KT][KS];
  f32x4 dk[KT][DT], dv[KT][DT];
#pragma unroll
  for (int u = 0; u < KT; ++u) {
    kt0[u] = k0 + (wave * KT + u) * 16;
    ktok[u] = kt0[u] + li;
    kvalid[u] = ktok[u] < p.N;
    const int tk = min(ktok[u], p.N - 1);
    kdead[u] = !kvalid[u] || (p.mask && p.mask[(size_t)b * p.N + tk]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int eo = (g * KS + ks) * 8;
      const u32x4 z = {0u, 0u, 0u, 0u};
      const u32x4 kw = ldg16(p.k.p + (b * p.k.sb + h * p.k.sh + tk * p.k.sn + eo) * 2);
      const u32x4 vw = ldg16(p.v.p + (b * p.v.sb + h * p.v.sh + tk * p.v.sn + eo) * 2);
      kf[u][ks] = as_x8<E>(kvalid[u] ? kw : z);
      vf[u][ks] = as_x8<E>(kvalid[u] ? vw : z);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dk[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }

  constexpr int NSL = (64 * CPR + 255) / 256;
  u32x4 nq[NSL], nd[NSL];
  float nl[NSL], ndl[NSL];
  auto issue = [&](int qc_) {
#pragma unroll
    for (int i = 0; i < NSL; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / CPR, c = idx - row * CPR;
      const int tok = min(qc_ + row, p.N - 1);
      nq[i] = ldg16(qbase + (tok * p.q.sn + c * 8) * 2);
      nd[i] = ldg16(dobase + (tok * p.dout.sn + c * 8) * 2);
      nl[i] = p.lse[(size_t)bh * p.N + tok];
      ndl[i] = p.delta[(size_t)bh * p.N + tok];
    }
  };
  // One 64-query chunk.  DG: the chunk crosses the diagonal of this workgroup's keys -- per wave and per 16-query sub-tile,
  // a sub-tile wholly before a key tile is skipped, the one on the diagonal gets `key > query -> 0` per element.
  auto chunk = [&](auto diag_tag, int qc) {
    constexpr bool DG = decltype(diag_tag)::value;
    int first[KT];                                   // (DG) the first 16-query sub-tile of this chunk that sees the key tile
#pragma unroll
    for (int u = 0; u < KT; ++u) first[u] = DG ? max((kt0[u] - qc) / 16, 0) : 0;
    const int fmin = first[0];                       // the wave's first key tile is seen soonest
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
      if (DG && 2 * qq + 1 < fmin) continue;
      uint32_t pw[KT][2][2], dsw[KT][2][2];
#pragma unroll
      for (int uq = 0; uq < 2; ++uq) {
        const int st = 2 * qq + uq, rq = st * 16;
        if (DG && st < fmin) {
#pragma unroll
          for (int u = 0; u < KT; ++u) { pw[u][uq][0] = pw[u][uq][1] = 0u; dsw[u][uq][0] = dsw[u][uq][1] = 0u; }
          continue;
        }
        f32x4 s[KT], dp[KT];
#pragma unroll
        for (int u = 0; u < KT; ++u) { s[u] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[u] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const typename E::x8 qfr = as_x8<E>(lds16(Qs + TileL<D>::off(rq + li, g * KS + ks)));
          const typename E::x8 dfr = as_x8<E>(lds16(dOs + TileL<D>::off(rq + li, g * KS + ks)));
#pragma unroll
          for (int u = 0; u < KT; ++u) {
            if (DG && st < first[u]) continue;
            s[u] = E::mma(qfr, kf[u][ks], s[u]);
            dp[u] = E::mma(dfr, vf[u][ks], dp[u]);
          }
        }
        const float4 l4 = *reinterpret_cast<const float4*>(lse_s + rq + 4 * g);
        const float4 d4 = *reinterpret_cast<const float4*>(delta_s + rq + 4 * g);
        const float ll[4] = {l4.x, l4.y, l4.z, l4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int u = 0; u < KT; ++u) {
          if (DG && st < first[u]) { pw[u][uq][0] = pw[u][uq][1] = 0u; dsw[u][uq][0] = dsw[u][uq][1] = 0u; continue; }
          const bool diag = DG && kt0[u] - qc == rq;                       // (wave-uniform)
          float pr[4], ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // a dead key's column is computed like any other and zeroed in the epilogue (columns are independent)
            pr[r] = fast_exp2(fmaf(s[u][r], p.scale_log2, ll[r]));
            if (diag && li > 4 * g + r) pr[r] = 0.f;                        // key > query
            float dpr = dp[u][r];
            float km = 1.f;
            if (DR) {
              const int qt = min(qc + rq + 4 * g + r, p.N - 1);
              km = p.keep[((size_t)bh * p.N + qt) * p.keep_ld + (kvalid[u] ? ktok[u] : 0)] ? p.keep_scale : 0.f;
              dpr *= km;
            }
            ds[r] = pr[r] * (dpr - dd[r]);
            if (DR) pr[r] *= km;
          }
          pw[u][uq][0] = pack2<E>(pr[0], pr[1]); pw[u][uq][1] = pack2<E>(pr[2], pr[3]);
          dsw[u][uq][0] = pack2<E>(ds[0], ds[1]); dsw[u][uq][1] = pack2<E>(ds[2], ds[3]);
        }
      }
      typename E::x8 pf[KT], dsf[KT];
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        u32x4 a4, b4;
        a4[0] = pw[u][0][0]; a4[1] = pw[u][0][1]; a4[2] = pw[u][1][0]; a4[3] = pw[u][1][1];
        b4[0] = dsw[u][0][0]; b4[1] = dsw[u][0][1]; b4[2] = dsw[u][1][0]; b4[3] = dsw[u][1][1];
        pf[u] = as_x8<E>(a4); dsf[u] = as_x8<E>(b4);
      }
      const int r0 = 32 * qq + 4 * g + (li >> 2), r1 = r0 + 16;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int o0 = tile_tr<D>(r0, li, dt);
        const int o1 = tile_tr<D>(r1, li, dt);
        const typename E::x8 dot = as_x8<E>(E::tr4(dOs + o0), E::tr4(dOs + o1));
        const typename E::x8 qt_ = as_x8<E>(E::tr4(Qs + o0), E::tr4(Qs + o1));
#pragma unroll
        for (int u = 0; u < KT; ++u) {
          if (DG && 2 * qq + 1 < first[u]) continue;
          dv[u][dt] = E::mma(dot, pf[u], dv[u][dt]);
          dk[u][dt] = E::mma(qt_, dsf[u], dk[u][dt]);
        }
      }
    }
  };
  auto run = [&](auto diag_tag, int qc0, int qc1) {
    for (int qc = qc0; qc < qc1; qc += 64) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NSL; ++i) {
        const int idx = tid + i * 256;
        const int row = idx / CPR, c = idx - row * CPR;
        if (64 * CPR % 256 != 0 && idx >= 64 * CPR) continue;
        const bool in = qc + row < p.N;
        const u32x4 z = {0u, 0u, 0u, 0u};
        sts16(Qs + TileL<D>::off(row, c), in ? nq[i] : z);
        sts16(dOs + TileL<D>::off(row, c), in ? nd[i] : z);
        if (c == 0) {
          lse_s[row] = in ? -nl[i] * LOG2E : -INFINITY;       // MINUS the log2-domain lse: added inside the score fma
          delta_s[row] = in ? ndl[i] : 0.f;
        }
      }
      __syncthreads();
      if (qc + 64 < p.N) issue(qc + 64);
      chunk(diag_tag, qc);
    }
  };
  // queries before the tile's first key see none of its keys: their chunks are never loaded
  const int qdiag = min(k0 + KPB, p.N);
  issue(k0);
  run(std::true_type{}, k0, qdiag);
  run(std::false_type{}, (qdiag + 63) / 64 * 64, p.N);
#pragma unroll
  for (int u = 0; u < KT; ++u) {
    float fk[DQ], fv[DQ];
    if constexpr (TileL<D>::NEWTR) {
      quad_transpose_f32(dk[u], fk);
      quad_transpose_f32(dv[u], fv);
#pragma unroll
      for (int j = 0; j < DQ; ++j) fk[j] *= p.scale;
    } else {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { fk[4 * dt + r] = dk[u][dt][r] * p.scale; fv[4 * dt + r] = dv[u][dt][r]; }
    }
    if (kdead[u]) {
#pragma unroll
      for (int j = 0; j < DQ; ++j) fk[j] = fv[j] = 0.f;
    }
    if (kvalid[u]) {
      char* d1 = p.dk.p + (b * p.dk.sb + h * p.dk.sh + ktok[u] * p.dk.sn + DQ * g) * 2;
      char* d2 = p.dv.p + (b * p.dv.sb + h * p.dv.sh + ktok[u] * p.dv.sn + DQ * g) * 2;
#pragma unroll
      for (int c = 0; c < DQ / 8; ++c) {
        stg16(d1 + c * 16, pack8<E>(fk + 8 * c));
        stg16(d2 + c * 16, pack8<E>(fv + 8 * c));
      }
    }
  }
}

bool softmax_causal_tiles_ok(int which, int tiles, int D, bool has_keep) {
  if (which == 0) return tiles == 1 || tiles == 2 || (tiles == 4 && D <= 64 && !has_keep);
  return tiles == 1 || (tiles == 2 && D <= 64);
}

int softmax_causal_tiles(int which, long bh, int N, int D, bool has_keep, int cus) {
  // t tiles per wave make nb = ceil(N / (64 t)) workgroups per sequence, worth (nb + 1) / 2 of the heaviest one
  auto fills = [&](int t) {
    const long nb = (N + 64 * t - 1) / (64 * t);
    return bh * (nb + 1) >= 4L * cus;                // bh (nb + 1) / 2 >= 2 cus
  };
  for (int t = which == 0 ? 4 : 2; t > 1; t >>= 1)
    if (softmax_causal_tiles_ok(which, t, D, has_keep) && fills(t)) return t;
  return 1;
}

template <typename E, int D, bool DR>
static int launch_smc(int which, const SmcP& p, int qt, hipStream_t st) {
  const dim3 block(256);
  const long bh = (long)p.B * p.H;
  const dim3 gq((unsigned)(bh * ((p.N + 64 * qt - 1) / (64 * qt))));
  if (which == 0) {
    if (qt == 4) { if constexpr (D <= 64 && !DR) hipLaunchKernelGGL((smc_fwd_kernel<E, D, DR, 4>), gq, block, 0, st, p); }
    else if (qt == 2) hipLaunchKernelGGL((smc_fwd_kernel<E, D, DR, 2>), gq, block, 0, st, p);
    else hipLaunchKernelGGL((smc_fwd_kernel<E, D, DR, 1>), gq, block, 0, st, p);
  } else {
    if (qt == 2) {
      if constexpr (D <= 64) {
        hipLaunchKernelGGL((smc_bwd_dq_kernel<E, D, DR, 2>), gq, block, 0, st, p);
        hipLaunchKernelGGL((smc_bwd_dkv_kernel<E, D, DR, 2>), gq, block, 0, st, p);
      }
    } else {
      hipLaunchKernelGGL((smc_bwd_dq_kernel<E, D, DR, 1>), gq, block, 0, st, p);
      hipLaunchKernelGGL((smc_bwd_dkv_kernel<E, D, DR, 1>), gq, block, 0, st, p);
    }
  }
  return (int)hipGetLastError();
}

template <typename E, int D>
static int launch_smc_d(int which, const SmcP& p, int tiles, hipStream_t st) {
  const bool dr = p.keep != nullptr;
  const int qt = tiles > 0 ? tiles : softmax_causal_tiles(which, (long)p.B * p.H, p.N, D, dr, ea_device_cus());
  if (!softmax_causal_tiles_ok(which, qt, D, dr)) return EA_E_BADARG;
  return dr ? launch_smc<E, D, true>(which, p, qt, st) : launch_smc<E, D, false>(which, p, qt, st);
}

int softmax_causal_dispatch(int which, const SmcP& p, int dtype, int D, int tiles, hipStream_t st) {
  if (dtype == EA_BF16) {
    if (D == 64) return launch_smc_d<BF16, 64>(which, p, tiles, st);
    if (D == 32) return launch_smc_d<BF16, 32>(which, p, tiles, st);
    if (D == 128) return launch_smc_d<BF16, 128>(which, p, tiles, st);
  } else if (dtype == EA_F16) {
    if (D == 64) return launch_smc_d<F16, 64>(which, p, tiles, st);
    if (D == 32) return launch_smc_d<F16, 32>(which, p, tiles, st);
    if (D == 128) return launch_smc_d<F16, 128>(which, p, tiles, st);
  }
  return EA_E_UNSUPPORTED;
}

}  // namespace ea
