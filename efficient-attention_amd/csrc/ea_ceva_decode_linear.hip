// ea_ceva_decode_linear.hip -- the two projections of a decoding step on weights a static state holds (ABI 22)
//
//   y[m, n] = round_y( sum_k round_w(x[m, k]) w[n, k] + bias[n] ),   1 <= M <= 64 rows, w [N, K] 16-bit row-major
//
// A step of a handful of rows is bound by reading w once: 6 MB (qkv) and 2 MB (out) at C = 1024 against 8 .. 64 rows of x.
// v_mfma_f32_16x16x32 takes w as its B operand with no staging at all: lane (g = lane >> 4, li = lane & 15) holds
// B[k = 8 g .. 8 g + 7][col = li] = w[n0 + li][k0 + 8 g ..], eight consecutive k of one weight row = one 16-byte global load
// straight into the operand registers.  x is the A operand, read from global memory the same way (row li of a 16-row tile;
// a few KB that every workgroup shares, so L2 serves them), rounded to the weight's type on load when it arrives in fp32.
//
// One workgroup owns 16 output columns and all (up to four) 16-row tiles of x.  Its NW waves split K into contiguous runs of
// 32-wide k-steps (wave s: steps s S .. s S + S - 1, S = ceil(K / 32 / NW)), so that a wave reads S 64-byte pieces in a row of
// every weight row; the body is branch-free (addresses clamped, operands zeroed by select), NS steps unrolled, so all of a
// wave's loads are issued ahead of its first MFMA: K <= 32 NS NW = 1024 is one pass.  The waves' partial tiles meet in LDS
// and are added in wave order by the threads that store them: no atomics, no workgroup waits for another -- a replay
// repeats the sums bit for bit.  Rows >= M of a tile are zero operands and are never stored.
//
// ceva_linear_fused_kernel (ABI 24) is the same product with what a decoder layer's feed-forward puts around it:
//
//   y[m, n] = round_y( act( sum_k round_w(LN(x)[m, k]) w[n, k] + bias[n] ) + res[m, n] )
//
// Prologue (LN): every workgroup computes (mean, rstd) of its M rows over K in fp32 -- two passes, biased variance,
// rsqrt(var + eps), the definition of ea_layernorm_fwd -- one wave per row, rows wave, wave + 8, ..; the statistics go to LDS
// and each lane keeps those of its RT operand rows.  An operand is then (x - mean) rstd gamma + beta in fp32, rounded ONCE
// to the weight's type as it is loaded: where the full path under autocast rounds (fp32 layer_norm output cast by the Linear).
// That costs every workgroup a second read of x (M K elements, L2) and saves a launch and an [M, K] round trip.
// Epilogue: the thread that sums an element over the waves applies bias, ReLU and the residual (fp32 or the weight's type) in
// fp32 and stores it; res may be y itself (the element is read and written by the same thread), x may not be y (other
// workgroups still read it).  The plain kernel above is left as it was: its instructions are pinned (tools/isa_diff.py).
#include "ea_common.h"
#include "ea_ceva_decode_linear.h"

namespace ea {
namespace {

constexpr int LIN_NW = 8;              // waves per workgroup
constexpr int LIN_NS = 4;              // k-steps a wave loads ahead

// eight consecutive k of one row of x as they lie in memory, and as the A operand (fp32: rounded to nearest even)
template <bool XF32> struct LinX;
template <> struct LinX<true> {
  f32x4 a, b;
  EA_DEV void load(const char* xrow, int k) {
    a = *reinterpret_cast<const f32x4*>(xrow + (int64_t)k * 4);
    b = *reinterpret_cast<const f32x4*>(xrow + (int64_t)k * 4 + 16);
  }
  template <typename E> EA_DEV u32x4 frag() const {
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return pack8<E>(f);
  }
};
template <> struct LinX<false> {
  u32x4 v;
  EA_DEV void load(const char* xrow, int k) { v = ldg16(xrow + (int64_t)k * 2); }
  template <typename E> EA_DEV u32x4 frag() const { return v; }
};

template <typename E, bool XF32, bool YF32, int RT>
__global__ __launch_bounds__(LIN_NW * 64) void ceva_linear_kernel(const DecLinP p) {
  __shared__ float red[LIN_NW * RT * 256];            // [wave][row tile][16 rows][16 columns]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.x * 16;
  const int KS = p.K >> 5;
  const int S = (KS + LIN_NW - 1) / LIN_NW;
  const int s_begin = wave * S, s_end = min(KS, s_begin + S);
  const char* wrow = p.w + ((int64_t)(n0 + li) * p.K + 8 * g) * 2;
  const char* xrow[RT];
  bool xlive[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int m = rt * 16 + li;
    xlive[rt] = m < p.M;
    xrow[rt] = p.x + (int64_t)min(m, p.M - 1) * p.ldx * (XF32 ? 4 : 2);
  }
  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int s0 = s_begin; s0 < s_end; s0 += LIN_NS) {
    u32x4 wf[LIN_NS];
    LinX<XF32> xr[LIN_NS][RT];
#pragma unroll
    for (int i = 0; i < LIN_NS; ++i) {                 // (a step past the wave's run: a clamped address, a zero operand below)
      const int s = min(s0 + i, KS - 1);
      wf[i] = ldg16(wrow + (int64_t)s * 64);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) xr[i][rt].load(xrow[rt], s * 32 + 8 * g);
    }
    __builtin_amdgcn_sched_barrier(0);                 // every load of the pass is out before the first conversion and MFMA
#pragma unroll
    for (int i = 0; i < LIN_NS; ++i) {
      const bool live = s0 + i < s_end;
      const u32x4 wv = live ? wf[i] : zero;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const u32x4 xc = xr[i][rt].template frag<E>();
        const u32x4 xv = live && xlive[rt] ? xc : zero;
        acc[rt] = E::mma(as_x8<E>(xv), as_x8<E>(wv), acc[rt]);
      }
    }
  }
  // D[row = 4 g + r][col = li] of every row tile -> LDS; then element e of the [16 RT, 16] tile is summed over the waves,
  // in wave order, by one thread
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * RT + rt) * 256 + (4 * g + r) * 16 + li] = acc[rt][r];
  __syncthreads();
  for (int e = threadIdx.x; e < RT * 256; e += LIN_NW * 64) {
    const int rt = e >> 8, idx = e & 255, m = rt * 16 + (idx >> 4), n = n0 + (idx & 15);
    if (m >= p.M) continue;
    float v = red[rt * 256 + idx];
#pragma unroll
    for (int w = 1; w < LIN_NW; ++w) v += red[(w * RT + rt) * 256 + idx];
    if (p.bias) v += E::to_f(reinterpret_cast<const uint16_t*>(p.bias)[n]);
    if constexpr (YF32) reinterpret_cast<float*>(p.y)[(int64_t)m * p.ldy + n] = v;
    else reinterpret_cast<uint16_t*>(p.y)[(int64_t)m * p.ldy + n] = E::from_f(v);
  }
}

// ---- the fused sibling (ABI 24) ----------------------------------------------------------------------------------------------
// k-steps a wave of the fused kernel loads ahead: four like the plain kernel; the fp32-x, four-row-tile LayerNorm instance
// holds 4 x 8 fp32 of x plus gamma and beta per step and takes two
template <bool XF32, int RT, bool LN> constexpr int fused_ns() { return LN && XF32 && RT == 4 ? 2 : LIN_NS; }

// eight consecutive k of one row of x as floats (the statistics, and the normalised operand)
template <typename E> EA_DEV void lin_floats(const LinX<true>& x, float* f) {
  f[0] = x.a[0]; f[1] = x.a[1]; f[2] = x.a[2]; f[3] = x.a[3]; f[4] = x.b[0]; f[5] = x.b[1]; f[6] = x.b[2]; f[7] = x.b[3];
}
template <typename E> EA_DEV void lin_floats(const LinX<false>& x, float* f) { unpack8<E>(x.v, f); }

template <typename E, bool XF32, bool YF32, int RT, bool LN>
__global__ __launch_bounds__(LIN_NW * 64) void ceva_linear_fused_kernel(const DecLinFusedP p) {
  constexpr int NS = fused_ns<XF32, RT, LN>();
  __shared__ float red[LIN_NW * RT * 256];            // [wave][row tile][16 rows][16 columns]
  __shared__ float stat[LN ? 2 * EA_LIN_MAX_ROWS : 2];  // (mean, rstd) of row m
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.x * 16;
  const int KS = p.K >> 5;
  const int S = (KS + LIN_NW - 1) / LIN_NW;
  const int s_begin = wave * S, s_end = min(KS, s_begin + S);
  const char* wrow = p.w + ((int64_t)(n0 + li) * p.K + 8 * g) * 2;
  const char* xrow[RT];
  bool xlive[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int m = rt * 16 + li;
    xlive[rt] = m < p.M;
    xrow[rt] = p.x + (int64_t)min(m, p.M - 1) * p.ldx * (XF32 ? 4 : 2);
  }
  float mean[RT], rstd[RT];
  if constexpr (LN) {
    // rows wave, wave + 8, ..: 8-element pieces lane, lane + 64, .. of the row, twice
    const int pieces = p.K >> 3;
    const float invK = 1.f / (float)p.K;
    for (int m = wave; m < p.M; m += LIN_NW) {
      const char* row = p.x + (int64_t)m * p.ldx * (XF32 ? 4 : 2);
      float sum = 0.f;
      for (int c = lane; c < pieces; c += 64) {
        LinX<XF32> v;
        float f[8];
        v.load(row, 8 * c);
        lin_floats<E>(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += f[j];
      }
      const float mu = wave_sum(sum) * invK;
      float sq = 0.f;
      for (int c = lane; c < pieces; c += 64) {
        LinX<XF32> v;
        float f[8];
        v.load(row, 8 * c);
        lin_floats<E>(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) sq += (f[j] - mu) * (f[j] - mu);
      }
      const float rs = rsqrtf(wave_sum(sq) * invK + p.ln_eps);
      if (lane == 0) { stat[2 * m] = mu; stat[2 * m + 1] = rs; }
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int m = min(rt * 16 + li, p.M - 1);
      mean[rt] = stat[2 * m];
      rstd[rt] = stat[2 * m + 1];
    }
  }
  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int s0 = s_begin; s0 < s_end; s0 += NS) {
    u32x4 wf[NS];
    LinX<XF32> xr[NS][RT];
    LinX<true> gam[LN ? NS : 1], bet[LN ? NS : 1];
#pragma unroll
    for (int i = 0; i < NS; ++i) {                     // (a step past the wave's run: a clamped address, a zero operand below)
      const int s = min(s0 + i, KS - 1);
      wf[i] = ldg16(wrow + (int64_t)s * 64);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) xr[i][rt].load(xrow[rt], s * 32 + 8 * g);
      if constexpr (LN) {
        gam[i].load(reinterpret_cast<const char*>(p.gamma), s * 32 + 8 * g);
        bet[i].load(reinterpret_cast<const char*>(p.beta), s * 32 + 8 * g);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                 // every load of the pass is out before the first conversion and MFMA
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const bool live = s0 + i < s_end;
      const u32x4 wv = live ? wf[i] : zero;
      float gf[8], bf[8];
      if constexpr (LN) { lin_floats<E>(gam[i], gf); lin_floats<E>(bet[i], bf); }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        u32x4 xc;
        if constexpr (LN) {
          float f[8];
          lin_floats<E>(xr[i][rt], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = (f[j] - mean[rt]) * rstd[rt] * gf[j] + bf[j];
          xc = pack8<E>(f);
        } else {
          xc = xr[i][rt].template frag<E>();
        }
        const u32x4 xv = live && xlive[rt] ? xc : zero;
        acc[rt] = E::mma(as_x8<E>(xv), as_x8<E>(wv), acc[rt]);
      }
    }
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * RT + rt) * 256 + (4 * g + r) * 16 + li] = acc[rt][r];
  __syncthreads();
  for (int e = threadIdx.x; e < RT * 256; e += LIN_NW * 64) {
    const int rt = e >> 8, idx = e & 255, m = rt * 16 + (idx >> 4), n = n0 + (idx & 15);
    if (m >= p.M) continue;
    float v = red[rt * 256 + idx];
#pragma unroll
    for (int w = 1; w < LIN_NW; ++w) v += red[(w * RT + rt) * 256 + idx];
    if (p.bias) v += E::to_f(reinterpret_cast<const uint16_t*>(p.bias)[n]);
    if (p.act == 1) v = v < 0.f ? 0.f : v;             // (a NaN stays one)
    if (p.res) {
      if (p.res_f32) v += reinterpret_cast<const float*>(p.res)[(int64_t)m * p.ldr + n];
      else v += E::to_f(reinterpret_cast<const uint16_t*>(p.res)[(int64_t)m * p.ldr + n]);
    }
    if constexpr (YF32) reinterpret_cast<float*>(p.y)[(int64_t)m * p.ldy + n] = v;
    else reinterpret_cast<uint16_t*>(p.y)[(int64_t)m * p.ldy + n] = E::from_f(v);
  }
}

using LinKernel = void (*)(const DecLinP);

template <typename E, bool XF32, bool YF32>
LinKernel lin_of(int M) {
  if (M <= 16) return ceva_linear_kernel<E, XF32, YF32, 1>;
  if (M <= 32) return ceva_linear_kernel<E, XF32, YF32, 2>;
  return ceva_linear_kernel<E, XF32, YF32, 4>;
}

template <typename E>
LinKernel lin_of(bool xf32, bool yf32, int M) {
  if (xf32) return yf32 ? lin_of<E, true, true>(M) : lin_of<E, true, false>(M);
  return yf32 ? lin_of<E, false, true>(M) : lin_of<E, false, false>(M);
}

using LinFusedKernel = void (*)(const DecLinFusedP);

template <typename E, bool XF32, bool YF32, bool LN>
LinFusedKernel fused_of(int M) {
  if (M <= 16) return ceva_linear_fused_kernel<E, XF32, YF32, 1, LN>;
  if (M <= 32) return ceva_linear_fused_kernel<E, XF32, YF32, 2, LN>;
  return ceva_linear_fused_kernel<E, XF32, YF32, 4, LN>;
}

template <typename E, bool LN>
LinFusedKernel fused_of(bool xf32, bool yf32, int M) {
  if (xf32) return yf32 ? fused_of<E, true, true, LN>(M) : fused_of<E, true, false, LN>(M);
  return yf32 ? fused_of<E, false, true, LN>(M) : fused_of<E, false, false, LN>(M);
}

template <typename E>
LinFusedKernel fused_of(bool ln, bool xf32, bool yf32, int M) {
  return ln ? fused_of<E, true>(xf32, yf32, M) : fused_of<E, false>(xf32, yf32, M);
}

}  // namespace

// (The C entry point has checked pointers, strides and alignment.)
int ceva_sdecode_linear(const DecLinP& p, hipStream_t st) {
  if (!p.x || !p.w || !p.y || p.M < 1 || p.ldx < p.K || p.ldy < p.N) return EA_E_BADARG;
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.N <= 0 || p.N % 16) return EA_E_UNSUPPORTED;
  LinKernel kernel;
  switch (p.dtype) {
    case EA_BF16: kernel = lin_of<BF16>(p.x_f32 != 0, p.y_f32 != 0, p.M); break;
    case EA_F16: kernel = lin_of<F16>(p.x_f32 != 0, p.y_f32 != 0, p.M); break;
    default: return EA_E_BADARG;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(p.N / 16)), dim3(LIN_NW * 64), 0, st, p);
  return (int)hipGetLastError();
}

// (The C entry point has checked pointers, strides, alignment, eps and the aliasing rule.)
int ceva_sdecode_linear_fused(const DecLinFusedP& p, hipStream_t st) {
  if (!p.x || !p.w || !p.y || p.M < 1 || p.ldx < p.K || p.ldy < p.N || (p.res && p.ldr < p.N)) return EA_E_BADARG;
  if ((p.gamma == nullptr) != (p.beta == nullptr) || p.x == p.y) return EA_E_BADARG;
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.N <= 0 || p.N % 16) return EA_E_UNSUPPORTED;
  if (p.act != 0 && p.act != 1) return EA_E_UNSUPPORTED;
  LinFusedKernel kernel;
  switch (p.dtype) {
    case EA_BF16: kernel = fused_of<BF16>(p.gamma != nullptr, p.x_f32 != 0, p.y_f32 != 0, p.M); break;
    case EA_F16: kernel = fused_of<F16>(p.gamma != nullptr, p.x_f32 != 0, p.y_f32 != 0, p.M); break;
    default: return EA_E_BADARG;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(p.N / 16)), dim3(LIN_NW * 64), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace ea
