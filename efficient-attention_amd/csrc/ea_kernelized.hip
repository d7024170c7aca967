// ea_kernelized.hip -- kernelized attention with the reference's feature maps, in EXACT fp32 arithmetic.
//
// KernelizedAttention (kernelized_attention.py) is linear attention over a feature map phi:
//   out_n = phi(q_n) KV / max(phi(q_n).ksum, 1e-2),  KV = sum_n phi(k_n)^T v_n,  ksum = sum_n phi(k_n),  padded keys phi = 0.
// The maps (c = d^-1/4, c2 = d^-1/2 / 2, r = m^-1/2, W [m, d] per head, logits l = c W x):
//   favorp       r exp(l - c2|x|^2 - stab) + 1e-4    stab: row max of l (queries) / max over (tokens, j) of the keys (detached)
//   relu         relu(r l) + 1e-3
//   fourier      r [sin l, cos l] exp(c2|x|^2 - max_n c2|x_n|^2)   (max over the sequence, per side, detached; 2m features)
//   relu-only    relu(x) + 0.1;  sigmoid-only  sigmoid(x) + 0.1    (d features, no W)
//   dpfp         x' = [relu(x), relu(-x)];  phi = concat_{j=1..nu} x' * roll(x', j)   (2 d nu features, no W)
// cos weighting (cosFormer) doubles the features to [phi cos t_n, phi sin t_n], t_n = (pi/2) n / N.
//
// The skeleton is ea_performer_f32.hip's: one 8-wave workgroup per (b,h, sequence slice), 64-token tiles in fp32 LDS, every
// product on v_mfma_f32_16x16x4_f32 (tile_mm), sequence-wide sums as per-slice partials added by ea_slice_sum; what the two
// units share word for word (tile moves, row reductions, constants, slice plan) is ea_f32_tile.h.  What is new
// is that the feature map is a compile-time policy (forward: tile -> phi; backward: d phi -> d logits / dx) and that the
// feature dimension (up to 256) is processed in blocks of fb = 32 or 16 columns: the features of a tile are never whole in
// LDS, only the block being worked on, so every kernel stays within the 160 KB of a CU next to the tiles, W and the logits.
#include "ea_common.h"
#include "ea_kernelized.h"
#include "ea_f32_mm.h"
#include "ea_f32_tile.h"

namespace ea {

using namespace f32tile;

namespace {

constexpr int FBM = 32;           // largest feature block
constexpr int LDF = FBM + 1;      // row stride of the feature-block images
constexpr int FMAX = KZ_MAX_F;    // features
constexpr int NACC = FMAX / 16 * (PD / 16) / NWV;   // [F][64] accumulator tiles per wave (8)
constexpr int DP2 = 2 * PD;       // dpfp's x' width

// LDS image (floats) -- the same function sizes the launch on the host
__host__ __device__ inline int kz_ld_l(int map, int M) { return kz_has_w(map) ? M + 1 : 0; }
__host__ __device__ inline int kz_ld_g(int map, int M) { return kz_has_w(map) ? M + 1 : map == KZ_DPFP ? DP2 + 1 : LDD; }
__host__ __device__ inline size_t kz_lds_floats(int map, int M) {
  const size_t w = kz_has_w(map) ? (size_t)M * LDD : 0, l = (size_t)TB * kz_ld_l(map, M);
  size_t g = (size_t)TB * kz_ld_g(map, M);
  if (g < (size_t)TB * LDD) g = (size_t)TB * LDD;                  // (the bwd_q out tile lives there too)
  return w + 2 * TB * LDD + l + 2 * TB * LDF + FBM * LDD + g + 8 * TB + FMAX;
}

struct Sm {
  float *W, *X, *Y, *L, *P, *D, *KB, *G;
  float *diag, *rs, *den, *dden, *sdl, *cw, *sw, *lv, *vec;
  int ldl, ldg;
};

EA_DEV Sm carve(float* sm, int map, int M) {
  Sm s;
  s.ldl = kz_ld_l(map, M);
  s.ldg = kz_ld_g(map, M);
  size_t g = (size_t)TB * s.ldg;
  if (g < (size_t)TB * LDD) g = (size_t)TB * LDD;
  float* c = sm;
  s.W = c; c += kz_has_w(map) ? M * LDD : 0;
  s.X = c; c += TB * LDD;
  s.Y = c; c += TB * LDD;
  s.L = c; c += TB * s.ldl;
  s.P = c; c += TB * LDF;
  s.D = c; c += TB * LDF;
  s.KB = c; c += FBM * LDD;
  s.G = c; c += g;
  s.diag = c; s.rs = c + TB; s.den = c + 2 * TB; s.dden = c + 3 * TB; s.sdl = c + 4 * TB; s.cw = c + 5 * TB;
  s.sw = c + 6 * TB; s.lv = c + 7 * TB;
  s.vec = c + 8 * TB;
  return s;
}

// c2 |x_n|^2 of the tile in X -> diag (row owners)
EA_DEV void sq_norms(const float* X, float* diag, int tid) {
  const int row = tid / LPR, q4 = tid % LPR;
  float s = 0.f;
  for (int e = q4 * (PD / LPR); e < (q4 + 1) * (PD / LPR); ++e) { const float x = X[row * LDD + e]; s += x * x; }
  s = row8_sum(s);
  if (q4 == 0) diag[row] = s * KC2;
}

// L[n][j] = c W_j . x_n for the tile in X (M logits per token)
EA_DEV void logits(const Sm& s, int M, int tid) {
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int ntn = M / 16;
  for (int t = wave; t < (TB / 16) * ntn; t += NWV) {
    const int m0 = (t / ntn) * 16, n0 = (t % ntn) * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    tile_mm<false, true, PD>(acc, s.X, LDD, s.W, LDD, m0, n0, PD, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) s.L[(m0 + 4 * g + r) * s.ldl + n0 + li] = acc[r] * KC;
  }
}

// the (b,h)'s statistic `side` (0 key side, 1 query side): maximum of the slice maxima
EA_DEV float stat_of(const KzP& p, int bh, int side) {
  float m = -INFINITY;
  for (int s = 0; s < p.S; ++s) m = fmaxf(m, p.p_st[((size_t)bh * p.S + s) * 2 + side]);
  return m;
}

// ---- the feature-map policy ---------------------------------------------------------------------------------------------
// x'[i] of dpfp
EA_DEV float dpfp_xp(const float* X, int n, int i) {
  return i < PD ? fmaxf(X[n * LDD + i], 0.f) : fmaxf(-X[n * LDD + i - PD], 0.f);
}

// base feature fb (before cos weighting) of token row n; needs the per-row prologue (rs) and, for the W maps, the logits
template <int MAP>
EA_DEV float base_feat(const Sm& s, int n, int fb, int M, float r) {
  if (MAP == KZ_FAVORP) return r * __expf(s.L[n * s.ldl + fb] - s.rs[n]) + 1e-4f;
  if (MAP == KZ_RELU) return fmaxf(r * s.L[n * s.ldl + fb], 0.f) + 1e-3f;
  if (MAP == KZ_FOURIER) {
    const bool cs = fb >= M;
    const float a = s.L[n * s.ldl + (cs ? fb - M : fb)];
    return s.rs[n] * (cs ? cosf(a) : sinf(a));
  }
  if (MAP == KZ_RELU_ONLY) return fmaxf(s.X[n * LDD + fb], 0.f) + 0.1f;
  if (MAP == KZ_SIGMOID_ONLY) return 1.f / (1.f + __expf(-s.X[n * LDD + fb])) + 0.1f;
  const int i = fb & (DP2 - 1), j = (fb >> 7) + 1;
  return dpfp_xp(s.X, n, i) * dpfp_xp(s.X, n, (i - j) & (DP2 - 1));
}

// per-tile prologue of the rows: rs (favorp: |x|^2 term + stabiliser; fourier: r exp(c2|x|^2 - max)), the cos / sin weights,
// liveness of the keys; clears the row accumulators.  `stat`: favorp key stabiliser or fourier's sequence maximum.
template <int MAP, bool COS>
EA_DEV void rows_prologue(const Sm& s, const KzP& p, int b, int t0, int n1, bool key, float stat, int M, float r, int tid) {
  const int row = tid / LPR, q4 = tid % LPR;
  float mx = -INFINITY;
  if (MAP == KZ_FAVORP && !key) {
    for (int j = q4 * (M / LPR), je = j + (M / LPR); j < je; ++j) mx = fmaxf(mx, s.L[row * s.ldl + j]);
    mx = row8_max(mx);
  }
  if (q4 == 0) {
    const int tok = t0 + row;
    if (MAP == KZ_FAVORP) s.rs[row] = s.diag[row] + (key ? stat : mx);
    if (MAP == KZ_FOURIER) s.rs[row] = r * __expf(s.diag[row] - stat);
    if (COS) {
      const float th = (1.5707963267948966f * (float)tok) * (1.f / (float)p.N);
      s.cw[row] = cosf(th);
      s.sw[row] = sinf(th);
    }
    s.lv[row] = key ? ((tok < n1 && !(p.mask && p.mask[(size_t)b * p.N + tok])) ? 1.f : 0.f) : 1.f;
    s.den[row] = 0.f;
    s.sdl[row] = 0.f;
  }
}

// P[n][c] = phi(x_n)[f0 + c], c < fb (0 for dead keys)
template <int MAP, bool COS>
EA_DEV void feat_block(const Sm& s, int f0, int fb, int Fb, int M, float r, int tid) {
  const int row = tid / LPR, q4 = tid % LPR, w = fb / LPR;
  const bool hi = COS && f0 >= Fb;
  const float wt = COS ? (hi ? s.sw[row] : s.cw[row]) : 1.f;
  const float lv = s.lv[row];
  for (int c = q4 * w; c < (q4 + 1) * w; ++c) {
    const int f = f0 + c;
    const float v = base_feat<MAP>(s, row, hi ? f - Fb : f, M, r) * wt;
    s.P[row * LDF + c] = lv != 0.f ? v : 0.f;
  }
}

// d phi block (in D) -> d logits (W maps, into G [64][M]) or dx (dx' for dpfp) accumulated in G; the row sums of the |x|^2
// term into sdl.  Blocks never straddle the cos halves, fourier's sin / cos halves or a dpfp roll, so within one block every
// element of G has one writer.
template <int MAP, bool COS>
EA_DEV void feat_bwd_block(const Sm& s, int f0, int fb, int Fb, int M, float r, int tid) {
  const int row = tid / LPR, q4 = tid % LPR, w = fb / LPR;
  const bool hi = COS && f0 >= Fb;
  const float wt = (COS ? (hi ? s.sw[row] : s.cw[row]) : 1.f) * s.lv[row];
  float acc = 0.f;
  for (int c = q4 * w; c < (q4 + 1) * w; ++c) {
    const int fbase = (hi ? f0 - Fb : f0) + c;
    const float g = s.D[row * LDF + c] * wt;
    if (MAP == KZ_FAVORP) {
      const float t = g * (base_feat<MAP>(s, row, fbase, M, r) - 1e-4f);
      s.G[row * s.ldg + fbase] += t;
      acc += t;
    } else if (MAP == KZ_RELU) {
      s.G[row * s.ldg + fbase] += r * s.L[row * s.ldl + fbase] > 0.f ? g * r : 0.f;
    } else if (MAP == KZ_FOURIER) {
      const bool cs = fbase >= M;
      const int j = cs ? fbase - M : fbase;
      const float a = s.L[row * s.ldl + j], sa = sinf(a), ca = cosf(a);
      s.G[row * s.ldg + j] += cs ? -g * s.rs[row] * sa : g * s.rs[row] * ca;
      acc += g * s.rs[row] * (cs ? ca : sa);                // d phi . phi: phi is proportional to exp(c2 |x|^2)
    } else if (MAP == KZ_RELU_ONLY) {
      s.G[row * s.ldg + fbase] += s.X[row * LDD + fbase] > 0.f ? g : 0.f;
    } else if (MAP == KZ_SIGMOID_ONLY) {
      const float sg = 1.f / (1.f + __expf(-s.X[row * LDD + fbase]));
      s.G[row * s.ldg + fbase] += g * sg * (1.f - sg);
    } else {                                                  // dpfp, first factor x'[i]
      const int i = fbase & (DP2 - 1), j = (fbase >> 7) + 1;
      s.G[row * s.ldg + i] += g * dpfp_xp(s.X, row, (i - j) & (DP2 - 1));
    }
  }
  if (MAP == KZ_FAVORP || MAP == KZ_FOURIER) {
    acc = row8_sum(acc);
    if (q4 == 0) s.sdl[row] += acc;
  }
  if (MAP == KZ_DPFP) {                                       // second factor x'[i - j]: its own pass (the indices overlap)
    __syncthreads();
    for (int c = q4 * w; c < (q4 + 1) * w; ++c) {
      const int fbase = (hi ? f0 - Fb : f0) + c;
      const float g = s.D[row * LDF + c] * wt;
      const int i = fbase & (DP2 - 1), j = (fbase >> 7) + 1;
      s.G[row * s.ldg + ((i - j) & (DP2 - 1))] += g * dpfp_xp(s.X, row, i);
    }
  }
}

// the input gradient of the tile -> dst[64][65]: W maps c G W -/+ 2 c2 sdl x; dpfp dx' -> dx; relu / sigmoid-only G itself
template <int MAP>
EA_DEV void input_grad(float* dst, const Sm& s, int M, int tid) {
  if (kz_has_w(MAP)) {
    const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const float sg = MAP == KZ_FAVORP ? -2.f * KC2 : MAP == KZ_FOURIER ? 2.f * KC2 : 0.f;
    for (int t = wave; t < 16; t += NWV) {
      const int m0 = (t >> 2) * 16, n0 = (t & 3) * 16;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      tile_mm<false, false>(acc, s.G, s.ldg, s.W, LDD, m0, n0, M, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = m0 + 4 * g + r, e = n0 + li;
        dst[n * LDD + e] = KC * acc[r] + sg * s.sdl[n] * s.X[n * LDD + e];
      }
    }
  } else {
    const int row = tid / LPR, q4 = tid % LPR;
    for (int e = q4 * (PD / LPR); e < (q4 + 1) * (PD / LPR); ++e) {
      const float x = s.X[row * LDD + e];
      dst[row * LDD + e] = MAP == KZ_DPFP ? (x > 0.f ? s.G[row * s.ldg + e] : 0.f) - (x < 0.f ? s.G[row * s.ldg + e + PD] : 0.f)
                                          : s.G[row * s.ldg + e];
    }
  }
}

EA_DEV void zero_g(const Sm& s, int M, int map, int tid) {
  const int n = TB * s.ldg;
  for (int i = tid; i < n; i += NTH) s.G[i] = 0.f;
}

// per-tile start shared by every kernel: load the x tile (and the second tile), logits, |x|^2, row prologue
template <int MAP, bool COS>
EA_DEV void tile_start(const Sm& s, const KzP& p, const T4& xt, const T4* yt, int ylim, int b, int h, int t0, int n1,
                       bool key, float stat, float r, int tid) {
  __syncthreads();
  load_tile(s.X, xt, b, h, t0, p.N, p.dtype, tid);
  if (yt) load_tile(s.Y, *yt, b, h, t0, ylim, p.dtype, tid);
  __syncthreads();
  if (kz_has_w(MAP)) logits(s, p.M, tid);
  if (MAP == KZ_FAVORP || MAP == KZ_FOURIER) sq_norms(s.X, s.diag, tid);
  __syncthreads();
  rows_prologue<MAP, COS>(s, p, b, t0, n1, key, stat, p.M, r, tid);
  __syncthreads();
}

EA_DEV void load_w(const Sm& s, const KzP& p, int map, int h, int tid) {
  if (kz_has_w(map)) load_mat(s.W, p.W + (size_t)h * p.M * PD, p.M, tid);
}

// does accumulator tile i of this wave ([F][64] tiles t = wave + 8 i: feature tile t / 4, channel tile t % 4) lie in the
// block [f0, f0 + fb)?
EA_DEV bool acc_in_block(int wave, int i, int f0, int fb) {
  const int ft = ((wave + NWV * i) >> 2) * 16;
  return ft >= f0 && ft < f0 + fb;
}

// the slice's partial of dW [M][64] (side 0: query pass, 1: key pass)
EA_DEV float* dw_part(const KzP& p, int b, int h, int side, int sl) {
  return p.p_dw + ((((size_t)h * p.B + b) * 2 + side) * p.S + sl) * p.M * PD;
}

// partial dW += c G^T X, the tile's share (G = d logits).  The slice's partial belongs to this workgroup alone, so it is
// accumulated in place (first tile: written) -- no accumulator registers live across the tile loop
EA_DEV void dw_accumulate(const Sm& s, float* ow, int M, bool first, int wave, int lane) {
  const int g = lane >> 4, li = lane & 15;
  for (int t = wave; t < (M / 16) * 4; t += NWV) {
    const int j0 = (t >> 2) * 16, e0 = (t & 3) * 16;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    tile_mm<true, false>(a, s.G, s.ldg, s.X, LDD, j0, e0, TB, lane);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      float* d = ow + (size_t)(j0 + 4 * g + rr) * PD + e0 + li;
      *d = (first ? 0.f : *d) + KC * a[rr];
    }
  }
}

// an empty slice (n0 >= n1: the slices are whole multiples of tiles) still owns its dW partial: zeros
EA_DEV void dw_zero_if_empty(float* ow, int M, int n0, int n1, int tid) {
  if (n0 < n1) return;
  for (int i = tid; i < M * PD; i += NTH) ow[i] = 0.f;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------
// statistics: favorp -- slice maximum of the key logits over (tokens, features) (padded keys included, as in the reference);
// fourier -- slice maxima of c2 |x|^2 over the keys (side 0) and the queries (side 1)
template <int MAP>
__global__ __launch_bounds__(NTH) void kz_stats_kernel(const KzP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Sm s = carve(sm, MAP, p.M);
  __shared__ float red[2][NWV];
  const int tid = threadIdx.x;
  const int bh = blockIdx.x, sl = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int row = tid / LPR, q4 = tid % LPR;
  load_w(s, p, MAP, h, tid);
  int n0, n1;
  slice_range(p, sl, n0, n1);
  float mk = -INFINITY, mq = -INFINITY;
  for (int t0 = n0; t0 < n1; t0 += TB) {
    __syncthreads();
    load_tile(s.X, p.k, b, h, t0, p.N, p.dtype, tid);
    if (MAP == KZ_FOURIER) load_tile(s.Y, p.q, b, h, t0, p.N, p.dtype, tid);
    __syncthreads();
    if (MAP == KZ_FAVORP) {
      logits(s, p.M, tid);
      __syncthreads();
      if (t0 + row < n1)
        for (int j = q4 * (p.M / LPR), je = j + (p.M / LPR); j < je; ++j) mk = fmaxf(mk, s.L[row * s.ldl + j]);
    } else {
      sq_norms(s.X, s.diag, tid);
      sq_norms(s.Y, s.rs, tid);
      __syncthreads();
      if (q4 == 0 && t0 + row < n1) { mk = fmaxf(mk, s.diag[row]); mq = fmaxf(mq, s.rs[row]); }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mk = fmaxf(mk, __shfl_xor(mk, o)); mq = fmaxf(mq, __shfl_xor(mq, o)); }
  if ((tid & 63) == 0) { red[0][tid >> 6] = mk; red[1][tid >> 6] = mq; }
  __syncthreads();
  if (tid < 2) {
    float m2 = red[tid][0];
    for (int i = 1; i < NWV; ++i) m2 = fmaxf(m2, red[tid][i]);
    p.p_st[((size_t)bh * p.S + sl) * 2 + tid] = m2;
  }
}

// keys: partial KV [F][64] and ksum [F] of the slice
template <int MAP, bool COS>
__global__ __launch_bounds__(NTH) void kz_kv_kernel(const KzP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Sm s = carve(sm, MAP, p.M);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, li = lane & 15;
  const int bh = blockIdx.x, sl = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const float r = rsqrtf((float)p.M);
  load_w(s, p, MAP, h, tid);
  const float stat = MAP == KZ_FAVORP || MAP == KZ_FOURIER ? stat_of(p, bh, 0) : 0.f;
  int n0, n1;
  slice_range(p, sl, n0, n1);
  f32x4 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ks = 0.f;
  for (int t0 = n0; t0 < n1; t0 += TB) {
    tile_start<MAP, COS>(s, p, p.k, &p.v, p.N, b, h, t0, n1, true, stat, r, tid);
    for (int f0 = 0; f0 < p.F; f0 += p.fb) {
      feat_block<MAP, COS>(s, f0, p.fb, p.Fb, p.M, r, tid);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NACC; ++i)
        if (acc_in_block(wave, i, f0, p.fb)) {
          const int t = wave + NWV * i;
          tile_mm<true, false, TB>(acc[i], s.P, LDF, s.Y, LDD, (t >> 2) * 16 - f0, (t & 3) * 16, TB, lane);
        }
      if (tid >= f0 && tid < f0 + p.fb) {
        float a = 0.f;
        for (int n = 0; n < TB; ++n) a += s.P[n * LDF + tid - f0];
        ks += a;
      }
      __syncthreads();
    }
  }
  float* okv = p.p_kv + ((size_t)bh * p.S + sl) * p.F * PD;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int t = wave + NWV * i;
    if ((t >> 2) * 16 < p.F) {
      const int j0 = (t >> 2) * 16, e0 = (t & 3) * 16;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) okv[(size_t)(j0 + 4 * g + rr) * PD + e0 + li] = acc[i][rr];
    }
  }
  if (tid < p.F) p.p_ks[((size_t)bh * p.S + sl) * p.F + tid] = ks;
}

// the block's rows [f0, f0 + fb) of a [BH, F, 64] matrix -> KB
EA_DEV void load_kb(const Sm& s, const float* m, const KzP& p, int bh, int f0, int tid) {
  load_mat(s.KB, m + ((size_t)bh * p.F + f0) * PD, p.fb, tid);
}

// acc2 (this wave's two [64][64] output tiles t = wave, wave + 8) += P KB over the block
EA_DEV void acc_feat_times(f32x4* acc2, const Sm& s, int fb, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int t = wave + NWV * i;
    if (fb == FBM) tile_mm<false, false, FBM>(acc2[i], s.P, LDF, s.KB, LDD, (t >> 2) * 16, (t & 3) * 16, FBM, lane);
    else tile_mm<false, false, 16>(acc2[i], s.P, LDF, s.KB, LDD, (t >> 2) * 16, (t & 3) * 16, 16, lane);
  }
}

// den[n] += P[n] . vec[f0 ..]
EA_DEV void acc_den(const Sm& s, int f0, int fb, int tid) {
  const int row = tid / LPR, q4 = tid % LPR, w = fb / LPR;
  float a = 0.f;
  for (int c = q4 * w; c < (q4 + 1) * w; ++c) a += s.P[row * LDF + c] * s.vec[f0 + c];
  a = row8_sum(a);
  if (q4 == 0) s.den[row] += a;
}

// acc2 * rowscale -> dst[64][65]
template <typename Fn>
EA_DEV void acc_to_tile(float* dst, const f32x4* acc2, int wave, int lane, Fn rowscale) {
  const int g = lane >> 4, li = lane & 15;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int t = wave + NWV * i, m0 = (t >> 2) * 16, n0 = (t & 3) * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(m0 + 4 * g + r) * LDD + n0 + li] = acc2[i][r] * rowscale(m0 + 4 * g + r);
  }
}

// queries, forward: out
template <int MAP, bool COS>
__global__ __launch_bounds__(NTH) void kz_out_kernel(const KzP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Sm s = carve(sm, MAP, p.M);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.x, sl = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const float r = rsqrtf((float)p.M);
  load_w(s, p, MAP, h, tid);
  for (int i = tid; i < p.F; i += NTH) s.vec[i] = p.ksum[(size_t)bh * p.F + i];
  const float stat = MAP == KZ_FOURIER ? stat_of(p, bh, 1) : 0.f;
  int n0, n1;
  slice_range(p, sl, n0, n1);
  for (int t0 = n0; t0 < n1; t0 += TB) {
    tile_start<MAP, COS>(s, p, p.q, nullptr, 0, b, h, t0, n1, false, stat, r, tid);
    f32x4 acc2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int f0 = 0; f0 < p.F; f0 += p.fb) {
      feat_block<MAP, COS>(s, f0, p.fb, p.Fb, p.M, r, tid);
      load_kb(s, p.kv, p, bh, f0, tid);
      __syncthreads();
      acc_feat_times(acc2, s, p.fb, wave, lane);
      acc_den(s, f0, p.fb, tid);
      __syncthreads();
    }
    acc_to_tile(s.Y, acc2, wave, lane, [&](int n) { return 1.f / fmaxf(s.den[n], 1e-2f); });
    __syncthreads();
    store_tile(s.Y, p.o, b, h, t0, n1, p.dtype, tid);
  }
}

// queries, backward: dq, the slice partials of d KV [F][64] and d ksum [F], and (learnable W) of dW [M][64]
template <int MAP, bool COS>
__global__ __launch_bounds__(NTH) void kz_bwd_q_kernel(const KzP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Sm s = carve(sm, MAP, p.M);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, li = lane & 15;
  const int bh = blockIdx.x, sl = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int row = tid / LPR, q4 = tid % LPR;
  const float r = rsqrtf((float)p.M);
  load_w(s, p, MAP, h, tid);
  for (int i = tid; i < p.F; i += NTH) s.vec[i] = p.ksum[(size_t)bh * p.F + i];
  const float stat = MAP == KZ_FOURIER ? stat_of(p, bh, 1) : 0.f;
  int n0, n1;
  slice_range(p, sl, n0, n1);
  if (kz_has_w(MAP) && p.p_dw) dw_zero_if_empty(dw_part(p, b, h, 0, sl), p.M, n0, n1, tid);
  f32x4 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dks = 0.f;
  for (int t0 = n0; t0 < n1; t0 += TB) {
    tile_start<MAP, COS>(s, p, p.q, &p.dout, n1, b, h, t0, n1, false, stat, r, tid);   // dout rows beyond the slice: 0
    // pass A: out = phi(q) KV / max(den, 1e-2)
    f32x4 acc2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int f0 = 0; f0 < p.F; f0 += p.fb) {
      feat_block<MAP, COS>(s, f0, p.fb, p.Fb, p.M, r, tid);
      load_kb(s, p.kv, p, bh, f0, tid);
      __syncthreads();
      acc_feat_times(acc2, s, p.fb, wave, lane);
      acc_den(s, f0, p.fb, tid);
      __syncthreads();
    }
    float* Os = s.G;                                         // the out tile, until G collects the gradients
    acc_to_tile(Os, acc2, wave, lane, [&](int n) { return 1.f / fmaxf(s.den[n], 1e-2f); });
    __syncthreads();
    {
      // d num = dout / max(den, 1e-2);  d den = -(dout . out) / max(den, 1e-2) where the clamp is inactive
      const float inv = 1.f / fmaxf(s.den[row], 1e-2f);
      float rd = 0.f;
      for (int e = q4 * (PD / LPR); e < (q4 + 1) * (PD / LPR); ++e) rd += s.Y[row * LDD + e] * Os[row * LDD + e];
      rd = row8_sum(rd);
      for (int e = q4 * (PD / LPR); e < (q4 + 1) * (PD / LPR); ++e) s.Y[row * LDD + e] *= inv;
      if (q4 == 0) s.dden[row] = s.den[row] >= 1e-2f ? -rd * inv : 0.f;
    }
    __syncthreads();
    zero_g(s, p.M, MAP, tid);
    // pass B: d phi = d num KV^T + d den ksum -> G;  d KV += phi^T d num, d ksum += phi^T d den
    for (int f0 = 0; f0 < p.F; f0 += p.fb) {
      feat_block<MAP, COS>(s, f0, p.fb, p.Fb, p.M, r, tid);
      load_kb(s, p.kv, p, bh, f0, tid);
      __syncthreads();
      if (wave < (p.fb / 16) * 4) {
        const int m0 = (wave & 3) * 16, j0 = (wave >> 2) * 16;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        tile_mm<false, true, PD>(a, s.Y, LDD, s.KB, LDD, m0, j0, PD, lane);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int n = m0 + 4 * g + rr, j = j0 + li;
          s.D[n * LDF + j] = a[rr] + s.dden[n] * s.vec[f0 + j];
        }
      }
#pragma unroll
      for (int i = 0; i < NACC; ++i)
        if (acc_in_block(wave, i, f0, p.fb)) {
          const int t = wave + NWV * i;
          tile_mm<true, false, TB>(acc[i], s.P, LDF, s.Y, LDD, (t >> 2) * 16 - f0, (t & 3) * 16, TB, lane);
        }
      if (tid >= f0 && tid < f0 + p.fb) {
        float a = 0.f;
        for (int n = 0; n < TB; ++n) a += s.P[n * LDF + tid - f0] * s.dden[n];
        dks += a;
      }
      __syncthreads();
      feat_bwd_block<MAP, COS>(s, f0, p.fb, p.Fb, p.M, r, tid);
      __syncthreads();
    }
    if (kz_has_w(MAP) && p.p_dw) dw_accumulate(s, dw_part(p, b, h, 0, sl), p.M, t0 == n0, wave, lane);
    input_grad<MAP>(s.Y, s, p.M, tid);                       // dq tile (d num is dead)
    __syncthreads();
    store_tile(s.Y, p.dq, b, h, t0, n1, p.dtype, tid);
  }
  float* okv = p.p_kv + ((size_t)bh * p.S + sl) * p.F * PD;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int t = wave + NWV * i;
    if ((t >> 2) * 16 < p.F) {
      const int j0 = (t >> 2) * 16, e0 = (t & 3) * 16;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) okv[(size_t)(j0 + 4 * g + rr) * PD + e0 + li] = acc[i][rr];
    }
  }
  if (tid < p.F) p.p_ks[((size_t)bh * p.S + sl) * p.F + tid] = dks;
}

// keys, backward: dk, dv from the summed d KV, d ksum (and, learnable W, the key side's dW partials)
template <int MAP, bool COS>
__global__ __launch_bounds__(NTH) void kz_bwd_k_kernel(const KzP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Sm s = carve(sm, MAP, p.M);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, li = lane & 15;
  const int bh = blockIdx.x, sl = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const float r = rsqrtf((float)p.M);
  load_w(s, p, MAP, h, tid);
  for (int i = tid; i < p.F; i += NTH) s.vec[i] = p.dksum[(size_t)bh * p.F + i];
  const float stat = MAP == KZ_FAVORP || MAP == KZ_FOURIER ? stat_of(p, bh, 0) : 0.f;
  int n0, n1;
  slice_range(p, sl, n0, n1);
  if (kz_has_w(MAP) && p.p_dw) dw_zero_if_empty(dw_part(p, b, h, 1, sl), p.M, n0, n1, tid);
  for (int t0 = n0; t0 < n1; t0 += TB) {
    tile_start<MAP, COS>(s, p, p.k, &p.v, p.N, b, h, t0, n1, true, stat, r, tid);
    zero_g(s, p.M, MAP, tid);
    f32x4 acc2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int f0 = 0; f0 < p.F; f0 += p.fb) {
      feat_block<MAP, COS>(s, f0, p.fb, p.Fb, p.M, r, tid);
      load_kb(s, p.dkv, p, bh, f0, tid);
      __syncthreads();
      // d phi[n][f] = v[n] . dKV[f] + d ksum[f]  (dead keys: zeroed in feat_bwd_block)
      if (wave < (p.fb / 16) * 4) {
        const int m0 = (wave & 3) * 16, j0 = (wave >> 2) * 16;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        tile_mm<false, true, PD>(a, s.Y, LDD, s.KB, LDD, m0, j0, PD, lane);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int n = m0 + 4 * g + rr, j = j0 + li;
          s.D[n * LDF + j] = a[rr] + s.vec[f0 + j];
        }
      }
      acc_feat_times(acc2, s, p.fb, wave, lane);             // dv = phi dKV
      __syncthreads();
      feat_bwd_block<MAP, COS>(s, f0, p.fb, p.Fb, p.M, r, tid);
      __syncthreads();
    }
    if (kz_has_w(MAP) && p.p_dw) dw_accumulate(s, dw_part(p, b, h, 1, sl), p.M, t0 == n0, wave, lane);
    acc_to_tile(s.Y, acc2, wave, lane, [](int) { return 1.f; });     // v is dead: its tile takes dv
    __syncthreads();
    store_tile(s.Y, p.dv, b, h, t0, n1, p.dtype, tid);
    __syncthreads();
    input_grad<MAP>(s.Y, s, p.M, tid);
    __syncthreads();
    store_tile(s.Y, p.dk, b, h, t0, n1, p.dtype, tid);
  }
}

// ------------------------------------------------------------------------------------------------------------------------
namespace {

template <int MAP, bool COS>
int kz_launch(int which, const KzP& p, dim3 grid, size_t lds, hipStream_t st) {
  const dim3 block(NTH);
  switch (which) {
    case 0:
      if constexpr (MAP == KZ_FAVORP || MAP == KZ_FOURIER) {
        if (const int e = ea_lds_limit(&kz_stats_kernel<MAP>, lds)) return e;
        hipLaunchKernelGGL(kz_stats_kernel<MAP>, grid, block, lds, st, p);
      } else {
        return EA_E_BADARG;
      }
      break;
    case 1:
      if (const int e = ea_lds_limit(&kz_kv_kernel<MAP, COS>, lds)) return e;
      hipLaunchKernelGGL((kz_kv_kernel<MAP, COS>), grid, block, lds, st, p);
      break;
    case 2:
      if (const int e = ea_lds_limit(&kz_out_kernel<MAP, COS>, lds)) return e;
      hipLaunchKernelGGL((kz_out_kernel<MAP, COS>), grid, block, lds, st, p);
      break;
    case 3:
      if (const int e = ea_lds_limit(&kz_bwd_q_kernel<MAP, COS>, lds)) return e;
      hipLaunchKernelGGL((kz_bwd_q_kernel<MAP, COS>), grid, block, lds, st, p);
      break;
    case 4:
      if (const int e = ea_lds_limit(&kz_bwd_k_kernel<MAP, COS>, lds)) return e;
      hipLaunchKernelGGL((kz_bwd_k_kernel<MAP, COS>), grid, block, lds, st, p);
      break;
    default:
      return EA_E_BADARG;
  }
  return (int)hipGetLastError();
}

template <int MAP>
int kz_launch_map(int which, const KzP& p, dim3 grid, size_t lds, hipStream_t st) {
  return p.cos ? kz_launch<MAP, true>(which, p, grid, lds, st) : kz_launch<MAP, false>(which, p, grid, lds, st);
}

}  // namespace

int kz_dispatch(int which, const KzP& p0, hipStream_t st) {
  KzP p = p0;
  if (p.map < KZ_FAVORP || p.map > KZ_DPFP || p.dtype < 0 || p.dtype > 2 || p.B <= 0 || p.H <= 0 || p.N <= 0)
    return EA_E_BADARG;
  if (kz_has_w(p.map) && (p.M <= 0 || p.M > KZ_MAX_M || (p.M & 15))) return EA_E_UNSUPPORTED;
  if (!kz_has_w(p.map)) p.M = 16;                       // (unused: only sizes r = M^-1/2, which these maps do not read)
  const int Fb = kz_base_features(p.map, p.M, p.nu);
  if (Fb <= 0 || Fb != p.Fb || p.F != Fb * (p.cos ? 2 : 1) || p.F > FMAX) return EA_E_UNSUPPORTED;
  p.fb = (Fb % FBM == 0 && (p.map != KZ_FOURIER || p.M % FBM == 0)) ? FBM : 16;
  const Slices sl = plan_slices(p.B * p.H, p.N);
  p.S = sl.S;
  p.tps = sl.tps;
  const dim3 grid((unsigned)(p.B * p.H), (unsigned)p.S);
  const size_t lds = kz_lds_floats(p.map, p.M) * sizeof(float);
  switch (p.map) {
    case KZ_FAVORP: return kz_launch_map<KZ_FAVORP>(which, p, grid, lds, st);
    case KZ_RELU: return kz_launch_map<KZ_RELU>(which, p, grid, lds, st);
    case KZ_FOURIER: return kz_launch_map<KZ_FOURIER>(which, p, grid, lds, st);
    case KZ_RELU_ONLY: return kz_launch_map<KZ_RELU_ONLY>(which, p, grid, lds, st);
    case KZ_SIGMOID_ONLY: return kz_launch_map<KZ_SIGMOID_ONLY>(which, p, grid, lds, st);
    default: return kz_launch_map<KZ_DPFP>(which, p, grid, lds, st);
  }
}

}  // namespace ea
