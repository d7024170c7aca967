// ea_adaptive_nll.hip -- the backward of the adaptive-softmax training loss (ea_harness.adaptive_loss.adaptive_nll,
// DecoderStack.adaptive_loss), whose forward is ea_adaptive_score (ea_adaptive_score.hip):
//
//   logp[m] = (a[m, ht_m] - lse_h[m]) + [m in tail i at position j] (b_i[j, t_m - c_i] - lse_i[j]),   h_i = E(x[rows_i] Q_i^T),  b_i = h_i E_i^T
//
// The head is ea_vocab_nll.hip's chunk loop on the head table with head_target and lse_head.  A tail runs the same loop over
// its device-counted list of positions, sized for M of them; nothing is read back:
//   ea_vocab_nll_grad_rows  VS_EPI_GRAD with ROWS = true: x (= h_i) and lse by position, targets and d through the list; the
//                           positions at or beyond the count are WRITTEN as zeros in G and G^T (the GEMMs contract over them)
//   ea_rows_transpose16     x[rows_i]^T and h_i^T as 16-bit [K, ldm] images with zeros beyond the count: h_i is uninitialised
//                           workspace there, and a zero of G^T times a NaN would poison dE_i
//   ea_gemm_nt16            dE_i[chunk] = G^T h_i,  dQ_i = dh_i^T x[rows_i]
//   ea_gemm_nt16_rows       dh_i (+)= G E_i (identity rows, the count: a dead tile runs no k loop) and dX[rows_i] += dh_i Q_i
//                           (the output rows through the list; a row lies in at most one tail and the launches are ordered)
//   rows_mask16             (forward, ea_adaptive_score_masked) h_i = E(h_i mask): the Dropout inside a tail
// Ordinary vector stores only; no atomics; no workgroup waits for another; every output element is written by one thread of
// one launch: bitwise reproducible.
#include "ea_vocab_score_tile.h"
#include "ea_adaptive_score.h"

namespace ea {
namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_TILE = 64;
constexpr int RM_THREADS = 256;

int64_t up64(int64_t n) { return (n + 63) / 64 * 64; }

EA_DEV int rt_live(const int32_t* count, int M) { return count ? max(0, min(*count, M)) : M; }

// a [64 positions][64 k] tile through LDS: read along k, written along the positions
template <typename E>
__global__ __launch_bounds__(RT_THREADS) void rows_transpose16_kernel(const RowsTransposeP p) {
  __shared__ uint16_t tile[RT_TILE][RT_TILE + 2];
  const int tid = threadIdx.x, lo = tid & 63, hi = tid >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * RT_TILE;
  const int k0 = blockIdx.y * RT_TILE;
  const int live = rt_live(p.count, p.M);
  if (j0 < live) {                                     // (uniform; a dead tile loads nothing)
    for (int jj = hi; jj < RT_TILE; jj += RT_THREADS / 64) {
      const int64_t j = j0 + jj;
      const int k = k0 + lo;
      uint16_t v = 0;
      if (j < live && k < p.K) {                       // (a list entry at or beyond the count is never read)
        const int64_t r = p.rows ? (int64_t)p.rows[j] : j;
        if (p.src_f32) v = E::from_f(reinterpret_cast<const float*>(p.src)[r * p.ld + k]);
        else v = reinterpret_cast<const uint16_t*>(p.src)[r * p.ld + k];
      }
      tile[jj][lo] = v;
    }
    __syncthreads();
  }
  for (int kk = hi; kk < RT_TILE; kk += RT_THREADS / 64) {
    const int64_t j = j0 + lo;
    const int k = k0 + kk;
    if (k < p.K && j < p.ldm) p.out[(int64_t)k * p.ldm + j] = j0 < live ? tile[lo][kk] : (uint16_t)0;
  }
}

// eight elements a thread
template <typename E>
__global__ __launch_bounds__(RM_THREADS) void rows_mask16_kernel(const RowsMaskP p) {
  const int per = p.D / 8;
  const int64_t at = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
  const int64_t j = at / per;
  if (j >= rt_live(p.count, p.M)) return;
  float h[8], m[8];
  unpack8<E>(*reinterpret_cast<const u32x4*>(p.h + at * 8), h);
  unpack8<E>(*reinterpret_cast<const u32x4*>(p.mask + at * 8), m);
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] *= m[e];
  *reinterpret_cast<u32x4*>(p.h + at * 8) = pack8<E>(h);
}

}  // namespace

int vocab_nll_grad_rows(VocabNllGradRowsP p, hipStream_t st) {
  p.MT = (p.M - 1) / VS_BM + 1;
  p.NS = (p.Vc - 1) / VS_SL + 1;
  if (p.dtype == EA_BF16)
    return p.x_f32 ? vs_launch<BF16, true, true, VS_EPI_GRAD>(p, st) : vs_launch<BF16, false, true, VS_EPI_GRAD>(p, st);
  return p.x_f32 ? vs_launch<F16, true, true, VS_EPI_GRAD>(p, st) : vs_launch<F16, false, true, VS_EPI_GRAD>(p, st);
}

int gemm_nt16_rows(GemmNt16RowsP p, hipStream_t st) {
  p.MT = (p.M - 1) / VS_BM + 1;
  p.NS = (p.V - 1) / VS_BN + 1;
  return p.dtype == EA_BF16 ? vs_launch<BF16, false, true, VS_EPI_GEMM>(p, st) : vs_launch<F16, false, true, VS_EPI_GEMM>(p, st);
}

int rows_transpose16(const RowsTransposeP& p, hipStream_t st) {
  const dim3 grid((unsigned)(p.ldm / RT_TILE), (unsigned)((p.K - 1) / RT_TILE + 1));
  if (p.dtype == EA_BF16) hipLaunchKernelGGL(rows_transpose16_kernel<BF16>, grid, dim3(RT_THREADS), 0, st, p);
  else hipLaunchKernelGGL(rows_transpose16_kernel<F16>, grid, dim3(RT_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

int rows_mask16(const RowsMaskP& p, hipStream_t st) {
  const int64_t n = (int64_t)p.M * (p.D / 8);
  const dim3 grid((unsigned)((n - 1) / RM_THREADS + 1));
  if (p.dtype == EA_BF16) hipLaunchKernelGGL(rows_mask16_kernel<BF16>, grid, dim3(RM_THREADS), 0, st, p);
  else hipLaunchKernelGGL(rows_mask16_kernel<F16>, grid, dim3(RM_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

// the largest chunk pass + x[rows_i]^T + the largest tail's dh (fp32), dh in 16 bits, its transpose and Q_i^T
int64_t adaptive_nll_ws(int M, int C, int n, const int64_t* cut, const int32_t* dims, int chunk_cols) {
  if (M < 1 || C < 1 || n < 1 || n > AS_MAX_TAILS || !cut || !dims || cut[0] < 1) return -1;
  for (int i = 0; i < n; ++i)
    if (cut[i + 1] <= cut[i] || dims[i] < 1) return -1;
  if (cut[n] > INT_MAX || cut[0] + n > INT_MAX) return -1;
  const int64_t ldm = up64(M);
  int64_t pass = vocab_nll_ws(M, C, (int)(cut[0] + n), chunk_cols), tail = 0;
  if (pass < 0) return -1;
  for (int i = 0; i < n; ++i) {
    const int64_t d = dims[i], w = vocab_nll_ws(M, dims[i], (int)(cut[i + 1] - cut[i]), chunk_cols);
    if (w < 0) return -1;
    pass = w > pass ? w : pass;
    const int64_t t = 6 * (int64_t)M * d + 2 * d * ldm + 2 * (int64_t)C * d;
    tail = t > tail ? t : tail;
  }
  return pass + 2 * (int64_t)C * ldm + tail;
}

}  // namespace ea
