// ea_lm_frag.h -- device helpers shared by the landmark-column kernels (ea_ceva_lm.hip, ea_eva_lm.hip): 64-row tile pairs on
// their way from global memory to LDS through registers, and a lane's operand fragments of one row.
#pragma once
#include "ea_common.h"

namespace ea {

constexpr int CLM_TILE = 64;             // queries per workgroup / landmark rows per streamed tile

// two 64-row tiles on their way from global memory to LDS through registers
template <int D> struct TilePair {
  static constexpr int CPR = D / 8, NCH = CLM_TILE * CPR / 256;
  u32x4 a[NCH], b[NCH];
  // rows row0 .. row0 + 63 of two contiguous [rows][D] 16-bit images
  EA_DEV void load_img(const char* A, const char* B, int row0, int tid) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const size_t off = ((size_t)row0 * CPR + tid + i * 256) * 16;
      a[i] = ldg16(A + off);
      b[i] = ldg16(B + off);
    }
  }
  // tokens tok0 .. tok0 + 63 of two strided views (pointers at their (b, h)); tokens >= N come as zero rows
  EA_DEV void load_tok(const char* A, int64_t sna, const char* B, int64_t snb, int tok0, int N, int tid) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int idx = tid + i * 256, row = idx / CPR, c = idx - row * CPR;
      const bool ok = tok0 + row < N;
      const int64_t tc = ok ? tok0 + row : N - 1;
      const u32x4 x = ldg16(A + (tc * sna + c * 8) * 2), y = ldg16(B + (tc * snb + c * 8) * 2);
      const u32x4 z = {0u, 0u, 0u, 0u};
      a[i] = ok ? x : z;
      b[i] = ok ? y : z;
    }
  }
  EA_DEV void store(char* As, char* Bs, int tid) const {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int idx = tid + i * 256, row = idx / CPR, c = idx - row * CPR;
      sts16(As + TileL<D>::off(row, c), a[i]);
      sts16(Bs + TileL<D>::off(row, c), b[i]);
    }
  }
};

// the lane's B-operand fragments of one row of a strided view / an image: chunk g KS + ks, what LaneOff::plain pairs with
template <typename E, int KS> EA_DEV void load_frag(typename E::x8* f, const char* row, int g, bool ok) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const u32x4 w4 = ldg16(row + (g * KS + ks) * 16);
    f[ks] = as_x8<E>(ok ? w4 : u32x4{0u, 0u, 0u, 0u});
  }
}
template <typename E, int KS> EA_DEV float frag_dot(const typename E::x8* a, const typename E::x8* b) {
  float s = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float x[8], y[8];
    unpack8<E>(__builtin_bit_cast(u32x4, a[ks]), x);
    unpack8<E>(__builtin_bit_cast(u32x4, b[ks]), y);
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(x[i], y[i], s);
  }
  return quad_sum(s);
}

}  // namespace ea
