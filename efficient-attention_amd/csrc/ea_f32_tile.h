// ea_f32_tile.h -- the tile layer of the exact-fp32 feature cores (ea_performer_f32.hip, ea_kernelized.hip).
//
// Both units run one 8-wave workgroup per (b,h, sequence slice) over 64-token tiles of head dim 64 held as fp32 LDS images
// with an odd row stride (conflict-free for both operand orientations of tile_mm).  What they share is here: the tile
// constants, the tile / matrix moves, the 8-lane row reductions, d^-1/4 and d^-1/2 / 2, and the slice plan.  The logits, the
// feature stages and the kernels are the units' own.
#pragma once
#include "ea_common.h"
#include "ea_t4.h"

namespace ea {
namespace f32tile {

constexpr int TB = 64;            // tokens per tile
constexpr int PD = 64;            // head dim
constexpr int LDD = PD + 1;       // row stride of the [*][64] images
constexpr int NTH = 512;          // threads per workgroup: 8 waves, two per SIMD (the LDS images allow one workgroup per CU)
constexpr int NWV = NTH / 64;     // waves
constexpr int LPR = NTH / TB;     // lanes per token row in the elementwise stages (8)

constexpr float KC = 0.35355339059327373f;   // 64^-1/4
constexpr float KC2 = 0.0625f;               // 64^-1/2 / 2

// The sequence slices of a (b,h): S workgroups of tps tokens each (whole tiles), about 1024 workgroups in all.
struct Slices {
  int S, tps;
};
inline Slices plan_slices(int BH, int N) {
  const int tiles = (N + TB - 1) / TB;
  int S = (1024 + BH - 1) / BH;
  if (S > tiles) S = tiles;
  if (S < 1) S = 1;
  if (S > 64) S = 64;
  return {S, ((tiles + S - 1) / S) * TB};
}

// the token range of this workgroup (P: a parameter block with N and the planned tps)
template <typename P>
EA_DEV void slice_range(const P& p, int s, int& n0, int& n1) {
  n0 = s * p.tps;
  n1 = min(p.N, n0 + p.tps);
}

// rows n0 .. n0 + 63 of a [B,H,N,64] view -> dst[row][65] fp32 (rows >= N: zeros); thread = (row, 8 channels)
EA_DEV void load_tile(float* dst, const T4& t, int b, int h, int n0, int N, int dtype, int tid) {
  const int row = tid / LPR, c0 = (tid % LPR) * 8;
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = 0.f;
  if (n0 + row < N) {
    const size_t eo = (size_t)b * t.sb + (size_t)h * t.sh + (size_t)(n0 + row) * t.sn + c0;
    if (dtype == 2) {
      const float* s = reinterpret_cast<const float*>(t.p) + eo;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(s), v1 = *reinterpret_cast<const f32x4*>(s + 4);
      f[0] = v0[0]; f[1] = v0[1]; f[2] = v0[2]; f[3] = v0[3]; f[4] = v1[0]; f[5] = v1[1]; f[6] = v1[2]; f[7] = v1[3];
    } else {
      const u32x4 w0 = ldg16(t.p + eo * 2);
      if (dtype == 0) unpack8<BF16>(w0, f);
      else unpack8<F16>(w0, f);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[row * LDD + c0 + i] = f[i];
}

// src[row][65] fp32 -> rows n0 .. of a [B,H,N,64] view in its I/O type (rows >= N dropped)
EA_DEV void store_tile(const float* src, const T4& t, int b, int h, int n0, int N, int dtype, int tid) {
  const int row = tid / LPR, c0 = (tid % LPR) * 8;
  if (n0 + row >= N) return;
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = src[row * LDD + c0 + i];
  const size_t eo = (size_t)b * t.sb + (size_t)h * t.sh + (size_t)(n0 + row) * t.sn + c0;
  if (dtype == 2) {
    float* d = reinterpret_cast<float*>(t.p) + eo;
    *reinterpret_cast<f32x4*>(d) = f32x4{f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(d + 4) = f32x4{f[4], f[5], f[6], f[7]};
  } else {
    char* d = t.p + eo * 2;
    if (dtype == 0) stg16(d, pack8<BF16>(f));
    else stg16(d, pack8<F16>(f));
  }
}

// [rows][64] fp32 global matrix -> dst[rows][65]
EA_DEV void load_mat(float* dst, const float* src, int rows, int tid) {
  for (int idx = tid; idx < rows * (PD / 4); idx += NTH) {
    const int r = idx / (PD / 4), c = (idx - r * (PD / 4)) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)r * PD + c);
    float* d = dst + r * LDD + c;
    d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
  }
}

// over the LPR = 8 lanes that share a row (row = tid / LPR); lane q4 of a row walks the CONTIGUOUS part q4 of it, which with
// the odd row stride keeps the 64 lanes of a wave on distinct LDS banks
EA_DEV float row8_sum(float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); return v; }
EA_DEV float row8_max(float v) { v = fmaxf(v, __shfl_xor(v, 1)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 4)); return v; }

}  // namespace f32tile
}  // namespace ea
