// ea_lara_lm.hip -- the token-column passes of the LARA estimator for 128 < C <= 512 samples, d = 64.
//
// lara_x_body (ea_lara_x_body.h) keeps every 16-sample tile of a token tile in registers at once, which caps it at C = 128.
// Here the sample axis is a LOOP over 64-sample groups:
//   * a prepare launch writes 16-bit images [BH, Cp, 64] (Cp = 64 ceil(C / 64), zero pad rows) of the landmark matrices and
//     the per-sample scalar columns [BH, 3, Cp] in the log2 domain, with pad values that give a pad slot weight exactly 0
//     (cst2 = -inf, lse_t2 = lse_k2 = +inf), so the passes need no `c < C` test and mean_c t divides by C;
//   * a workgroup of 4 waves owns `tok_per_block` tokens of one (b, h) and takes them in 64-token steps, one 16-token tile per
//     wave; token rows sit in registers as MFMA B operands (layout X of ea_lara.h: scores D[c = 4g + r][n = li]);
//   * RESIDENT plan: the images of the pass are staged once per workgroup and stay; STREAMED plan: 64-row groups go through
//     two LDS slots, the next group's global loads are issued before the current group's MFMAs and committed after them
//     (one barrier per group);
//   * quantities that need every c before any c can be finished take a sweep of their own:
//       LLM_FWD   mis-opt: sweep 1 t -> mean_c t; sweep 2 alpha, z, online softmax over c (running maximum, rescaled
//                 accumulator), W.kv.  mis-biased / mis-bh: the second sweep alone.
//       LLM_BWDQ  re-uses the forward's lseZ / tmean: sweep 1 rowdot = sum_c W dW and sda = sum_c d alpha
//                 (= sum_c e dW - rowdot sum_c e with e = 2^(z - lseZ) where alpha is not clamped); sweep 2 dZ, t dt and
//                 dq = s (omega^T dZ + qbar^T t dt).
//       LLM_BWDK  one sweep: Pk, dB -> dv = dkv^T Pk, dk = s omega^T dB - s k sum_c dB.
//       LLM_QCORR one sweep: dq -= s sum_c t (u qbar)_c.
// Rounding points are lara_x_body's: weights are packed to the element type before their MFMA, normalisers and scalar sums
// add the unrounded values, results are stored in the I/O dtype.
#include "ea_lara.h"
#include "ea_lara_lm.h"

namespace ea {
namespace {

template <int MODE, int MIS> struct LlmUse {
  static constexpr bool U0 = MODE != LLM_QCORR;                                                       // omega
  static constexpr bool U1 = MODE == LLM_QCORR || ((MODE == LLM_FWD || MODE == LLM_BWDQ) && MIS != MIS_BH);   // qbar
  static constexpr int NM = (U0 ? 1 : 0) + (U1 ? 1 : 0) + 1;
  static constexpr int S0 = 0, S1 = U0 ? 1 : 0, S2 = NM - 1;                                          // LDS slots of the three
};

// score tiles of one 64-sample group against the wave's 16 tokens: a = M0 . x1, tt = M1 . x1, dw = M2 . x2
template <typename E, bool UA, bool UT, bool UW>
EA_DEV void llm_scores(const char* m0, const char* m1, const char* m2, const int* plain, const typename E::x8* x1,
                       const typename E::x8* x2, f32x4* a, f32x4* tt, f32x4* dw) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    a[ct] = tt[ct] = dw[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ro = ct * 16 * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (UA) a[ct] = E::mma(as_x8<E>(lds16(m0 + ro + plain[ks])), x1[ks], a[ct]);
      if (UT) tt[ct] = E::mma(as_x8<E>(lds16(m1 + ro + plain[ks])), x1[ks], tt[ct]);
      if (UW) dw[ct] = E::mma(as_x8<E>(lds16(m2 + ro + plain[ks])), x2[ks], dw[ct]);
    }
  }
}

// acc^T[d][n] += M^T . w over the 64 samples of a group (transpose reads of the row-major tile)
template <typename E>
EA_DEV void llm_contract(const char* m, const int* tr, const float (&w)[4][4], f32x4* acc) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    u32x4 pw;
    pw[0] = pack2<E>(w[2 * kk][0], w[2 * kk][1]); pw[1] = pack2<E>(w[2 * kk][2], w[2 * kk][3]);
    pw[2] = pack2<E>(w[2 * kk + 1][0], w[2 * kk + 1][1]); pw[3] = pack2<E>(w[2 * kk + 1][2], w[2 * kk + 1][3]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const char* r = m + 32 * kk * 128 + tr[dt];
      acc[dt] = E::mma(as_x8<E>(E::tr4(r), E::tr4(r + 16 * 128)), as_x8<E>(pw), acc[dt]);
    }
  }
}

template <typename E>
__global__ __launch_bounds__(256) void llm_prepare_kernel(const LaraLmP p) {
  const size_t total = (size_t)p.B * p.H * p.Cp * 8;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c8 = (int)(idx & 7);
  const size_t rr = idx >> 3;
  const int row = (int)(rr % p.Cp);
  const size_t bh = rr / p.Cp;
  const bool ok = row < p.C;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (!p.dst[j]) continue;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p.src[j] && ok) {
      const float* s = p.src[j] + (bh * p.C + row) * 64 + c8 * 8;
      const float4 lo = *reinterpret_cast<const float4*>(s), hi = *reinterpret_cast<const float4*>(s + 4);
      f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
    }
    stg16(p.dst[j] + idx * 16, pack8<E>(f));
  }
  if (c8 == 0 && p.sdst) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      p.sdst[(bh * 3 + j) * p.Cp + row] = (p.ssrc[j] && ok) ? p.ssrc[j][bh * p.C + row] * p.smul[j] : p.spad[j];
  }
}

template <typename E, int MODE, int MIS, bool STREAM>
__global__ __launch_bounds__(256) void llm_kernel(const LaraLmP p) {
  using U = LlmUse<MODE, MIS>;
  constexpr int ROWB = 128, DQ = 16, GB = LLM_GROUP * ROWB;
  constexpr bool OPT = MIS == MIS_OPT, BIASED = MIS == MIS_BIASED;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Cp = p.Cp, NG = p.NG;
  float* SC0 = reinterpret_cast<float*>(smem);
  float* SC1 = SC0 + Cp;
  float* SC2 = SC1 + Cp;
  char* IMG = smem + (size_t)3 * Cp * sizeof(float);
  const int MS = STREAM ? GB : Cp * ROWB;            // bytes between two images in LDS

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int bh = blockIdx.x / p.nsplit, blk = blockIdx.x - bh * p.nsplit;
  const int b = bh / p.H, h = bh - b * p.H;
  const int n0 = blk * p.tok_per_block, n1 = min(p.N, n0 + p.tok_per_block);
  const size_t ioff = (size_t)bh * Cp * ROWB;
  const char* gm0 = U::U0 ? p.img[0] + ioff : nullptr;
  const char* gm1 = U::U1 ? p.img[1] + ioff : nullptr;
  const char* gm2 = p.img[2] + ioff;

  // a 64-row group of every image of the pass on its way to LDS: two 16-byte chunks per thread and image
  u32x4 st[U::NM][2];
  auto load_group = [&](int gi) {
    const size_t o = (size_t)gi * GB + (size_t)tid * 16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (U::U0) st[U::S0][i] = ldg16(gm0 + o + i * 4096);
      if (U::U1) st[U::S1][i] = ldg16(gm1 + o + i * 4096);
      st[U::S2][i] = ldg16(gm2 + o + i * 4096);
    }
  };
  auto store_group = [&](char* base) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256;
      const int off = TileL<64>::off(idx >> 3, idx & 7);
#pragma unroll
      for (int s = 0; s < U::NM; ++s) sts16(base + s * MS + off, st[s][i]);
    }
  };
  for (int c = tid; c < 3 * Cp; c += 256) SC0[c] = p.sc[(size_t)bh * 3 * Cp + c];
  if (STREAM) {
    load_group(0);
    store_group(IMG);
  } else {
    for (int gi = 0; gi < NG; ++gi) {
      load_group(gi);
      store_group(IMG + gi * GB);
    }
  }
  __syncthreads();

  LaneOff2<64> lo;
  lo.init(lane);
  int turn = 0;                                      // STREAMED: groups taken so far (slot = turn & 1)
  // one sweep over the sample groups; body(gi, base): the images of group gi are at base + slot * MS
  auto sweep = [&](auto&& body) {
    for (int gi = 0; gi < NG; ++gi) {
      if constexpr (STREAM) {
        load_group(gi + 1 == NG ? 0 : gi + 1);       // in flight during this group's MFMAs (the last one of a kernel is unused)
        body(gi, IMG + (turn & 1) * U::NM * GB);
        store_group(IMG + ((turn + 1) & 1) * U::NM * GB);   // (read last in the previous turn, before its barrier)
        __syncthreads();
        ++turn;
      } else {
        body(gi, IMG + gi * GB);
      }
    }
  };
  auto v4 = [&](const float* base, int gi, int ct) { return *reinterpret_cast<const float4*>(base + gi * 64 + ct * 16 + 4 * g); };

  constexpr bool KEYS = MODE == LLM_BWDK;
  constexpr bool TWO_TOK = MODE == LLM_BWDQ || MODE == LLM_BWDK;
  const T4& tk1 = KEYS ? p.k : p.q;
  const T4& tk2 = KEYS ? p.v : p.dout;
  const char* t1b = tk1.p + (b * tk1.sb + h * tk1.sh) * 2;
  const char* t2b = TWO_TOK ? tk2.p + (b * tk2.sb + h * tk2.sh) * 2 : nullptr;
  const float s2 = p.scale_log2, kappa = p.kappa, invC = 1.f / (float)p.C;

  // every wave takes every 64-token step (the streamed plan has a barrier per group); a tile past the end works on the
  // clamped last token and stores nothing
  for (int t0 = n0; t0 < n1; t0 += 64) {
    const int tok = t0 + wave * 16 + li;
    const bool valid = tok < n1;
    const int64_t tc = valid ? tok : n1 - 1;
    u32x4 raw1[2];
    typename E::x8 x1[2], x2[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      raw1[ks] = ldg16(t1b + (tc * tk1.sn + (g * 2 + ks) * 8) * 2);
      x1[ks] = as_x8<E>(raw1[ks]);
      x2[ks] = as_x8<E>(TWO_TOK ? ldg16(t2b + (tc * tk2.sn + (g * 2 + ks) * 8) * 2) : raw1[ks]);
    }
    const size_t so = (size_t)bh * p.N + tc;
    f32x4 acc[4], acc2[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = acc2[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 a[4], tt[4], dw[4];

    if constexpr (MODE == LLM_FWD) {
      float tmean = 0.f;
      if constexpr (OPT) {
        float ts = 0.f;
        sweep([&](int gi, const char* base) {
          llm_scores<E, false, true, false>(nullptr, base + U::S1 * MS, nullptr, lo.plain, x1, x2, a, tt, dw);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const float4 ls = v4(SC1, gi, ct);
            ts += fast_exp2(tt[ct][0] * s2 - ls.x) + fast_exp2(tt[ct][1] * s2 - ls.y);
            ts += fast_exp2(tt[ct][2] * s2 - ls.z) + fast_exp2(tt[ct][3] * s2 - ls.w);
          }
        });
        tmean = quad_sum(ts) * invC;
      }
      float mrun = -INFINITY, ssum = 0.f;
      sweep([&](int gi, const char* base) {
        llm_scores<E, true, U::U1, false>(base, base + U::S1 * MS, nullptr, lo.plain, x1, x2, a, tt, dw);
        float z[4][4], gmax = -INFINITY;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float4 cs = v4(SC0, gi, ct);
          const float c4[4] = {cs.x, cs.y, cs.z, cs.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            z[ct][r] = a[ct][r] * s2 + c4[r];
            if (BIASED) z[ct][r] += tt[ct][r] * s2;
            gmax = fmaxf(gmax, z[ct][r]);
          }
        }
        const float mn = fmaxf(mrun, quad_max(gmax));   // finite from the first group on: slot 0 is a real sample
        const float resc = fast_exp2(mrun - mn);
        mrun = mn;
        ssum *= resc;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[dt] = acc[dt] * resc;
        float w[4][4];
        const float kt = -kappa * tmean;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float4 ls = OPT ? v4(SC1, gi, ct) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 bv = OPT ? v4(SC2, gi, ct) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float l4[4] = {ls.x, ls.y, ls.z, ls.w}, b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float wv = fast_exp2(z[ct][r] - mn);
            if (OPT) {
              const float t = fast_exp2(tt[ct][r] * s2 - l4[r]);
              wv *= fmaxf(kappa * t + (b4[r] + kt), 1e-8f);
            }
            w[ct][r] = wv;
            ssum += wv;
          }
        }
        llm_contract<E>(base + U::S2 * MS, lo.tr, w, acc);
      });
      ssum = quad_sum(ssum);
      char* dst = valid ? p.o.p + (b * p.o.sb + h * p.o.sh + tc * p.o.sn + DQ * g) * 2 : ea_trash_line();
      u32x4 o0, o1;
      quad_transpose_pack<E>(acc, fast_rcp(ssum), o0, o1);
      stg16(dst, o0);
      stg16(dst + 16, o1);
      if (p.lseZ && valid && g == 0) {
        p.lseZ[so] = mrun + fast_log2(ssum);
        p.tmean[so] = tmean;
      }
    } else if constexpr (MODE == LLM_BWDQ) {
      const float lz = p.lseZ[so], tm = p.tmean[so];
      const float kt = -kappa * tm;
      // one (c, n) entry: W, and e = 2^(z - lseZ) where alpha is not clamped (d alpha = e (dW - rd)), t
      auto entry = [&](float av, float tv, float cs, float ls, float bv, float& W, float& e, float& t) {
        float x = av * s2 + (cs - lz);
        if (BIASED) x += tv * s2;
        const float wz = fast_exp2(x);
        W = wz; e = 0.f; t = 0.f;
        if (OPT) {
          t = fast_exp2(tv * s2 - ls);
          const float al = kappa * t + (bv + kt);
          W = wz * fmaxf(al, 1e-8f);
          e = al > 1e-8f ? wz : 0.f;
        }
      };
      float rd = 0.f, e1 = 0.f, e0 = 0.f;
      sweep([&](int gi, const char* base) {
        llm_scores<E, true, U::U1, true>(base, base + U::S1 * MS, base + U::S2 * MS, lo.plain, x1, x2, a, tt, dw);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float4 cs = v4(SC0, gi, ct);
          const float4 ls = OPT ? v4(SC1, gi, ct) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 bv = OPT ? v4(SC2, gi, ct) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float c4[4] = {cs.x, cs.y, cs.z, cs.w}, l4[4] = {ls.x, ls.y, ls.z, ls.w}, b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float W, e, t;
            entry(a[ct][r], tt[ct][r], c4[r], l4[r], b4[r], W, e, t);
            rd += W * dw[ct][r];
            e1 += e * dw[ct][r];
            e0 += e;
          }
        }
      });
      rd = quad_sum(rd);
      const float sda = OPT ? quad_sum(e1) - rd * quad_sum(e0) : 0.f;
      const float sdm = sda * invC;
      sweep([&](int gi, const char* base) {
        llm_scores<E, true, U::U1, true>(base, base + U::S1 * MS, base + U::S2 * MS, lo.plain, x1, x2, a, tt, dw);
        float w1[4][4], w2[4][4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float4 cs = v4(SC0, gi, ct);
          const float4 ls = OPT ? v4(SC1, gi, ct) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 bv = OPT ? v4(SC2, gi, ct) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float c4[4] = {cs.x, cs.y, cs.z, cs.w}, l4[4] = {ls.x, ls.y, ls.z, ls.w}, b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float W, e, t;
            entry(a[ct][r], tt[ct][r], c4[r], l4[r], b4[r], W, e, t);
            const float dd = dw[ct][r] - rd;
            w1[ct][r] = W * dd;                                        // dZ
            w2[ct][r] = OPT ? t * kappa * (e * dd - sdm) : w1[ct][r];   // t dt | dT = dZ (mis-biased)
          }
        }
        llm_contract<E>(base, lo.tr, w1, acc);
        if (U::U1) llm_contract<E>(base + U::S1 * MS, lo.tr, w2, acc);
      });
      float f[DQ];
      quad_transpose_f32(acc, f);
      if (valid) {
#pragma unroll
        for (int j = 0; j < DQ; ++j) f[j] *= p.scale;
        char* dst = p.dq.p + (b * p.dq.sb + h * p.dq.sh + tc * p.dq.sn + DQ * g) * 2;
        stg16(dst, pack8<E>(f));
        stg16(dst + 16, pack8<E>(f + 8));
        if (g == 0) {
          p.rowdot[so] = rd;
          p.sda[so] = sda;
        }
      }
    } else if constexpr (MODE == LLM_BWDK) {
      float kf[2][8], nrm = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        unpack8<E>(raw1[ks], kf[ks]);
#pragma unroll
        for (int i = 0; i < 8; ++i) nrm += kf[ks][i] * kf[ks][i];
      }
      nrm = quad_sum(nrm);
      const bool dead = !valid || (p.mask && p.mask[(size_t)b * p.N + tc]);
      const float diag2 = 0.5f * s2 * nrm;
      float sdb = 0.f;
      sweep([&](int gi, const char* base) {
        llm_scores<E, true, false, true>(base, nullptr, base + U::S2 * MS, lo.plain, x1, x2, a, tt, dw);
        float w1[4][4], w2[4][4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float4 lk = v4(SC0, gi, ct), dk4 = v4(SC1, gi, ct), rs = v4(SC2, gi, ct);
          const float l4[4] = {lk.x, lk.y, lk.z, lk.w}, d4[4] = {dk4.x, dk4.y, dk4.z, dk4.w}, r4[4] = {rs.x, rs.y, rs.z, rs.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pk = dead ? 0.f : fast_exp2(a[ct][r] * s2 - diag2 - l4[r]);
            const float db = pk * (dw[ct][r] - d4[r] + r4[r]);
            w1[ct][r] = pk;
            w2[ct][r] = db;
            sdb += db;
          }
        }
        llm_contract<E>(base + U::S2 * MS, lo.tr, w1, acc);     // dv = dkv^T Pk
        llm_contract<E>(base, lo.tr, w2, acc2);                 // omega^T dB
      });
      sdb = quad_sum(sdb);
      float fv[DQ], fk[DQ];
      quad_transpose_f32(acc, fv);
      quad_transpose_f32(acc2, fk);
      if (valid) {
        char* dstv = p.dv.p + (b * p.dv.sb + h * p.dv.sh + tc * p.dv.sn + DQ * g) * 2;
        stg16(dstv, pack8<E>(fv));
        stg16(dstv + 16, pack8<E>(fv + 8));
        char* dstk = p.dk.p + (b * p.dk.sb + h * p.dk.sh + tc * p.dk.sn + DQ * g) * 2;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          float o8[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) o8[i] = p.scale * fk[8 * ks + i] - p.scale * kf[ks][i] * sdb;
          stg16(dstk + ks * 16, pack8<E>(o8));
        }
      }
    } else {   // LLM_QCORR
      sweep([&](int gi, const char* base) {
        llm_scores<E, false, true, false>(nullptr, base + U::S1 * MS, nullptr, lo.plain, x1, x2, a, tt, dw);
        float w[4][4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float4 ls = v4(SC1, gi, ct);
          w[ct][0] = fast_exp2(tt[ct][0] * s2 - ls.x); w[ct][1] = fast_exp2(tt[ct][1] * s2 - ls.y);
          w[ct][2] = fast_exp2(tt[ct][2] * s2 - ls.z); w[ct][3] = fast_exp2(tt[ct][3] * s2 - ls.w);
        }
        llm_contract<E>(base + U::S2 * MS, lo.tr, w, acc);
      });
      float f[DQ];
      quad_transpose_f32(acc, f);
      if (valid) {
        char* dst = p.dq.p + (b * p.dq.sb + h * p.dq.sh + tc * p.dq.sn + DQ * g) * 2;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float old[8];
          unpack8<E>(ldg16(dst + c * 16), old);
#pragma unroll
          for (int i = 0; i < 8; ++i) old[i] -= f[8 * c + i] * p.scale;
          stg16(dst + c * 16, pack8<E>(old));
        }
      }
    }
  }
}

template <typename K> int llm_launch(K* kernel, const LaraLmP& p, size_t grid, size_t lds, hipStream_t st) {
  if (const int e = ea_lds_limit(kernel, lds)) return e;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), lds, st, p);
  return (int)hipGetLastError();
}

template <typename E, int MODE, int MIS>
int llm_run_plan(const LaraLmP& p, hipStream_t st) {
  const size_t grid = (size_t)p.B * p.H * p.nsplit, lds = llm_lds(MODE, p.mis, p.Cp, p.resident != 0);
  if (p.resident) return llm_launch(&llm_kernel<E, MODE, MIS, false>, p, grid, lds, st);
  return llm_launch(&llm_kernel<E, MODE, MIS, true>, p, grid, lds, st);
}

template <typename E>
int llm_run(int which, const LaraLmP& p, hipStream_t st) {
  if (which == -1) {
    const size_t total = (size_t)p.B * p.H * p.Cp * 8;
    return llm_launch(&llm_prepare_kernel<E>, p, (total + 255) / 256, 0, st);
  }
  if (which == LLM_BWDK) return llm_run_plan<E, LLM_BWDK, -1>(p, st);
  if (which == LLM_QCORR) return llm_run_plan<E, LLM_QCORR, -1>(p, st);
  if (which == LLM_FWD) {
    if (p.mis == MIS_OPT) return llm_run_plan<E, LLM_FWD, MIS_OPT>(p, st);
    if (p.mis == MIS_BIASED) return llm_run_plan<E, LLM_FWD, MIS_BIASED>(p, st);
    return llm_run_plan<E, LLM_FWD, MIS_BH>(p, st);
  }
  if (which == LLM_BWDQ) {
    if (p.mis == MIS_OPT) return llm_run_plan<E, LLM_BWDQ, MIS_OPT>(p, st);
    if (p.mis == MIS_BIASED) return llm_run_plan<E, LLM_BWDQ, MIS_BIASED>(p, st);
    return llm_run_plan<E, LLM_BWDQ, MIS_BH>(p, st);
  }
  return EA_E_BADARG;
}

}  // namespace

int lara_lm_dispatch(int which, const LaraLmP& p, int dtype, hipStream_t st) {
  if (dtype == EA_BF16) return llm_run<BF16>(which, p, st);
  if (dtype == EA_F16) return llm_run<F16>(which, p, st);
  return EA_E_UNSUPPORTED;
}

}  // namespace ea
