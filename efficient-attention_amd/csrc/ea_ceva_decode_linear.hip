// ea_ceva_decode_linear.hip -- the projections of a decoding step on weights a static state holds: the plain one (ABI 22) and
// the one with what a decoder layer's feed-forward puts around it (ABI 24)
//
//   y[m, n] = round_y( sum_k round_w(x[m, k]) w[n, k] + bias[n] ),   1 <= M <= 64 rows, w [N, K] 16-bit row-major
//   y[m, n] = round_y( act( sum_k round_w(LN(x)[m, k]) w[n, k] + bias[n] ) + res[m, n] )
//
// Both are instances of ceva_rows_kernel (ea_ceva_decode_rows.h: the tile loop, the LayerNorm prologue and the epilogue), on
// DecLinP and on DecLinFusedP; this file checks a block and launches its instance.
#include <limits.h>
#include <math.h>
#include <type_traits>
#include "ea_common.h"
#include "ea_ceva_decode_linear.h"
#include "ea_ceva_decode_vocab.h"

namespace ea {
namespace {

#include "ea_ceva_decode_rows.h"

template <typename P>
int lin_launch(const P& p, hipStream_t st) {
  const RowsKernel<P> kernel = rows_kernel_of(p);
  return kernel ? rows_launch(kernel, p, p.N, st) : EA_E_BADARG;
}

}  // namespace

// (The C entry point has checked pointers, strides and alignment.)
int ceva_sdecode_linear(const DecLinP& p, hipStream_t st) {
  if (!p.x || !p.w || !p.y || p.M < 1 || p.ldx < p.K || p.ldy < p.N) return EA_E_BADARG;
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.N <= 0 || p.N % 16) return EA_E_UNSUPPORTED;
  return lin_launch(p, st);
}

// (The C entry point has checked pointers, strides, alignment, eps and the aliasing rule.)
int ceva_sdecode_linear_fused(const DecLinFusedP& p, hipStream_t st) {
  if (!p.x || !p.w || !p.y || p.M < 1 || p.ldx < p.K || p.ldy < p.N || (p.res && p.ldr < p.N)) return EA_E_BADARG;
  if ((p.gamma == nullptr) != (p.beta == nullptr) || p.x == p.y) return EA_E_BADARG;
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.N <= 0 || p.N % 16) return EA_E_UNSUPPORTED;
  if (p.act != 0 && p.act != 1) return EA_E_UNSUPPORTED;
  return lin_launch(p, st);
}

}  // namespace ea
