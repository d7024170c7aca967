// ea_vocab_score.hip -- the many-row vocabulary pass (ABI 30): token, top logit, log-sum-exp and a log-probability per row
// of x against a 16-bit vocabulary table, for thousands of rows, without a [rows, V] tensor
//
//   logit[m, v] = sum_k round_w(x[m, k]) w[v, k]            fp32, no bias;  any M >= 1, w [V, K] 16-bit row-major, K % 32 == 0
//   token[m]    = argmax_v logit[m, v], top[m] its value    torch.argmax's rule: equal values: the lowest index; NaN wins
//   lse[m]      = log sum_v exp(logit[m, v])                 by cases on top: NaN, +inf, -inf stay; else top + logf(S)
//   logp[m]     = logit[m, targets[m]] - lse[m]              (no targets: top[m] - lse[m])
//
// The few-row entries (ea_ceva_decode_vocab.hip) stream the whole table for at most 64 rows: bound by 2 V K bytes per call.
// With M in the thousands the work is a GEMM, M x V x K, and both operands are K-contiguous: a lane's eight k of a row of x
// (the MFMA's A operand) and of a row of w (its B operand) are one 16-byte piece of a row, so tiles go through LDS as they
// lie in memory and no transposed read is needed.
//
// Launch one, vocab_score_kernel: workgroup (slice t, row tile) owns VS_BM = 128 rows of x and the VS_SL = 2048 columns
// t VS_SL .. of the table.  It walks the slice in column blocks of VS_BN = 128 and K in stages of VS_BK = 64: eight waves, 4 x 2,
// each a 32 x 64 accumulator acc[2][4] of v_mfma_f32_16x16x32 (with four waves of 64 x 64 the running state of 16 rows per
// lane beside 64 accumulator registers did not fit 256 VGPRs).  A stage is two tiles [128][64] of 16-bit, 128-byte rows whose
// 16-byte chunks are swizzled by psi (ea_lds_swizzle.h: conflict-free for chunk 4 ks + g of row li); the next stage's global
// loads are issued before the MFMAs of this one and stored to the other LDS buffer behind them: one barrier per stage.  fp32
// rows of x are rounded to the table's type as they are stored to LDS.  Rows >= M and table rows >= V are read as row M - 1 /
// the slice's last row (never beyond the allocations); k >= K of the last stage is a zero operand.
// Behind a block's last stage a lane holds, of each of its 8 rows, the four columns 16 j + li of its wave's half: it folds
// them into the row's running (best value, best index, sum of exp(logit - best value)) -- its OWN columns' only, in
// registers, across the blocks of the slice.  A column >= V is -inf with no index: it takes no part.  The sum is rescaled
// only when the best value rises (the factor is exactly 1 otherwise).  The target's logit is stored by the lane that holds it.
// After the slice's last block the 16 lanes of a row merge (xor butterfly 8, 4, 2, 1: the best pair, each lane's sum rescaled
// once to it, the sums added), then the wave pair through LDS, and one partial per (row, slice) goes to ws.
// Launch two, vocab_score_fold_kernel: one thread per row folds the row's slices in slice order.
//
// The order of summation is this kernel's own: the logits need not have the few-row entries' bits.  Slice and block widths
// are compile-time constants, so the partition of the columns depends on V alone: a row's results do not depend on M, on the
// rows beside it or on its place in the batch.  Ordinary vector stores only; no atomics; no workgroup waits for another.
#include <limits.h>
#include <math.h>
#include "ea_common.h"
#include "ea_vocab_score.h"

namespace ea {
namespace {

constexpr int VS_THREADS = 512;                                      // eight waves, 4 x 2: a wave owns 32 rows x 64 columns
constexpr int VS_FOLD_THREADS = 256;
constexpr int VS_TILE_BYTES = VS_BM * VS_BK * 2;                      // one [128][64] 16-bit tile
constexpr int VS_STAGE_BYTES = 2 * VS_TILE_BYTES;                     // x tile, w tile
constexpr int VS_LDS_TGT = 2 * VS_STAGE_BYTES;                        // int32 [VS_BM]: the rows' targets, -1: none
constexpr int VS_LDS_MERGE = VS_LDS_TGT + VS_BM * 4;                  // (value, index, sum) [VS_BM]: the right wave's partials
constexpr int VS_LDS_BYTES = VS_LDS_MERGE + VS_BM * 12;
static_assert(VS_BM == 128 && VS_BN == 128 && VS_BK == 64, "eight waves of 32 x 64 over 128-byte LDS rows");
static_assert(VS_SL % VS_BN == 0, "a slice is whole column blocks");
static_assert(sizeof(VsPick) == 8, "a candidate is one 8-byte store");

// a takes b's place: a NaN beats every number, a larger number a smaller one, and of two equals (two NaNs, +0 and -0) the
// lower index (the few-row entries' voc_beats).  Selects, no branches: the epilogue is straight-line code.
EA_DEV bool vs_beats(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv, lower = ai < bi;
  const bool among_nan = !bn | lower;
  const bool among_numbers = (av > bv) | ((av == bv) & lower);     // (false when b is NaN)
  return an ? among_nan : among_numbers;
}

// a partial sum of exponentials taken against the maximum `from`, against the maximum `to` >= from
EA_DEV float vs_rescale(float s, float from, float to) { return from == to ? s : s * expf(from - to); }

// eight consecutive k of one row of x as they lie in memory, and as 16-bit (fp32: rounded to nearest even)
template <bool XF32> struct VsX;
template <> struct VsX<true> {
  f32x4 a, b;
  EA_DEV void zero() { a = f32x4{0.f, 0.f, 0.f, 0.f}; b = a; }
  EA_DEV void load(const char* row, int k) {
    a = *reinterpret_cast<const f32x4*>(row + (int64_t)k * 4);
    b = *reinterpret_cast<const f32x4*>(row + (int64_t)k * 4 + 16);
  }
  template <typename E> EA_DEV u32x4 frag() const {
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return pack8<E>(f);
  }
};
template <> struct VsX<false> {
  u32x4 v;
  EA_DEV void zero() { v = u32x4{0u, 0u, 0u, 0u}; }
  EA_DEV void load(const char* row, int k) { v = ldg16(row + (int64_t)k * 2); }
  template <typename E> EA_DEV u32x4 frag() const { return v; }
};

template <typename E, bool XF32>
__global__ __launch_bounds__(VS_THREADS) void vocab_score_kernel(const VocabScoreP p) {
  extern __shared__ __attribute__((aligned(16))) char vs_lds[];
  int32_t* tgts = reinterpret_cast<int32_t*>(vs_lds + VS_LDS_TGT);
  float* merge = reinterpret_cast<float*>(vs_lds + VS_LDS_MERGE);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;
  const int slice = blockIdx.x / p.MT;
  const int m0 = (blockIdx.x - slice * p.MT) * VS_BM;
  const int s0 = slice * VS_SL;                        // (< V)
  const int ncols = min(VS_SL, p.V - s0);              // columns of this slice: at least one
  const int nblk = (ncols + VS_BN - 1) / VS_BN;
  const int KT = (p.K + VS_BK - 1) / VS_BK;
  const int IT = nblk * KT;

  // the loads of a stage: chunk lc of rows lr and lr + 64 of both tiles.  The x tile is fetched (from L2: 256 KB a workgroup
  // at K = 1024) and staged again for every column block of the slice: 128 x K 16-bit elements do not fit beside two stages in
  // LDS.  Measured as it stands: 470 TFLOP/s at (9216, 1024, 32768 | 262144); keeping x resident (a smaller
  // row tile, or K split over two passes) is the first thing to try beyond that and is not done here.
  const int lc = tid & 7, lr = tid >> 3;
  const char* xrow[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) xrow[q] = p.x + (int64_t)min(m0 + lr + 64 * q, p.M - 1) * p.ldx * (XF32 ? 4 : 2);
  const char* wslice = p.w + (int64_t)s0 * p.K * 2;
  VsX<XF32> rx[2];
  u32x4 rw[2];
  auto fetch = [&](int blk, int kt) {
    const int k = kt * VS_BK + 8 * lc;
    if (k < p.K) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        rx[q].load(xrow[q], k);
        const int n = min(blk * VS_BN + lr + 64 * q, ncols - 1);   // (a column past V: the slice's last row again)
        rw[q] = ldg16(wslice + ((int64_t)n * p.K + k) * 2);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q) { rx[q].zero(); rw[q] = u32x4{0u, 0u, 0u, 0u}; }
    }
  };
  auto stash = [&](int buf) {
    char* xt = vs_lds + buf * VS_STAGE_BYTES;
    char* wt = xt + VS_TILE_BYTES;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int off = lds_off3<64>(lr + 64 * q, lc);
      sts16(xt + off, rx[q].template frag<E>());
      sts16(wt + off, rw[q]);
    }
  };

  if (tid < VS_BM) {
    const int m = m0 + tid;
    int64_t t = -1;
    if (p.targets && m < p.M) t = p.targets[m];
    tgts[tid] = t >= 0 && t < (int64_t)p.V ? (int32_t)t : -1;
  }

  // the operand reads of a stage: row 16 i + li of the wave's 32 rows / 16 j + li of its 64 columns, chunk 4 ks + g
  int aoff[2], boff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    aoff[ks] = lds_off3<64>(wm * 32 + li, 4 * ks + g);
    boff[ks] = VS_TILE_BYTES + lds_off3<64>(wn * 64 + li, 4 * ks + g);
  }

  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the running state of row 16 i + 4 g + r (of the wave's 32) over this lane's columns: entry 4 i + r
  float bv[8], bs[8], tl[8];
  int32_t bi[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) { bv[q] = -INFINITY; bi[q] = INT_MAX; bs[q] = 0.f; tl[q] = 0.f; }

  fetch(0, 0);
  stash(0);
  __syncthreads();
  int blk = 0, kt = 0;
  for (int it = 0; it < IT; ++it) {
    const bool more = it + 1 < IT;
    const bool last_k = kt + 1 == KT;
    const int blk_next = last_k ? blk + 1 : blk, kt_next = last_k ? 0 : kt + 1;
    if (more) fetch(blk_next, kt_next);
    const char* st = vs_lds + (it & 1) * VS_STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 af[2], bf[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = lds16(st + aoff[ks] + i * 16 * 128);
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = lds16(st + boff[ks] + j * 16 * 128);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = E::mma(as_x8<E>(af[i]), as_x8<E>(bf[j]), acc[i][j]);
    }
    if (more) stash((it + 1) & 1);
    if (last_k) {
      // the block's logits: D[row 16 i + 4 g + r][column 16 j + li] of the wave's 32 x 64
      const int c0 = blk * VS_BN + wn * 64 + li;       // this lane's first column, within the slice
      if (p.logits) {                                  // (uniform; the tests' and a curious caller's path)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * 32 + 16 * i + 4 * g + r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int cs = c0 + 16 * j;
              if (cs < ncols && m < p.M) {
                const float a = acc[i][j][r];
                if (p.l_f32) reinterpret_cast<float*>(p.logits)[(int64_t)m * p.ldl + s0 + cs] = a;
                else reinterpret_cast<uint16_t*>(p.logits)[(int64_t)m * p.ldl + s0 + cs] = E::from_f(a);
              }
            }
          }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = 4 * i + r;
          const int tgt = tgts[wm * 32 + 16 * i + 4 * g + r];
          const float mold = bv[q];
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int cs = c0 + 16 * j;
            const bool live = cs < ncols;
            const int col = s0 + (live ? cs : 0);
            const float a = acc[i][j][r];
            v[j] = live ? a : -INFINITY;
            tl[q] = (live & (col == tgt)) ? a : tl[q];
            const bool take = live & vs_beats(a, col, bv[q], bi[q]);
            bv[q] = take ? a : bv[q];
            bi[q] = take ? col : bi[q];
          }
          const float mnew = bv[q];
          float e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = v[j] == -INFINITY ? 0.f : expf(v[j] - mnew);
          bs[q] = vs_rescale(bs[q], mold, mnew) + ((e[0] + e[1]) + (e[2] + e[3]));
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    blk = blk_next; kt = kt_next;
    __syncthreads();
  }

  // the target's logit: stored by the one lane whose columns hold it
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int row = wm * 32 + 16 * (q >> 2) + 4 * g + (q & 3);
    const int tgt = tgts[row];
    const int cs = tgt - s0;                           // (tgt is -1 or in [0, V))
    if (tgt >= 0 && cs >= 0 && cs < ncols && (cs & 15) == li && ((cs >> 6) & 1) == wn && m0 + row < p.M) p.tlogit[m0 + row] = tl[q];
  }
  // the 16 lanes of a row: the best pair, every lane's sum against it, the sums
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float mv = bv[q];
    int32_t mi = bi[q];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mv, o);
      const int32_t oi = __shfl_xor(mi, o);
      const bool take = vs_beats(ov, oi, mv, mi);
      mv = take ? ov : mv;
      mi = take ? oi : mi;
    }
    float s = vs_rescale(bs[q], bv[q], mv);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    bv[q] = mv; bi[q] = mi; bs[q] = s;
  }
  // the wave pair: the right half's partials through LDS, folded left then right
  if (wn == 1 && li == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = wm * 32 + 16 * (q >> 2) + 4 * g + (q & 3);
      merge[3 * row] = bv[q];
      merge[3 * row + 1] = __int_as_float(bi[q]);
      merge[3 * row + 2] = bs[q];
    }
  }
  __syncthreads();
  if (wn == 0 && li == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = wm * 32 + 16 * (q >> 2) + 4 * g + (q & 3);
      const int m = m0 + row;
      const float ov = merge[3 * row];
      const int32_t oi = __float_as_int(merge[3 * row + 1]);
      const float os = merge[3 * row + 2];
      const bool take = vs_beats(ov, oi, bv[q], bi[q]);
      const float mv = take ? ov : bv[q];
      const int32_t mi = take ? oi : bi[q];
      const float s = vs_rescale(bs[q], bv[q], mv) + vs_rescale(os, ov, mv);
      if (m < p.M) {
        const int64_t at = (int64_t)slice * p.M + m;
        p.pick[at] = VsPick{mv, mi};
        p.sum[at] = s;
      }
    }
  }
}

// launch two: one thread per row folds the row's NS partials in slice order
__global__ __launch_bounds__(VS_FOLD_THREADS) void vocab_score_fold_kernel(const VocabScoreP p) {
  const int64_t m = (int64_t)blockIdx.x * VS_FOLD_THREADS + threadIdx.x;
  if (m >= p.M) return;
  float top = -INFINITY;
  int32_t idx = INT_MAX;
  for (int t = 0; t < p.NS; ++t) {
    const VsPick c = p.pick[(int64_t)t * p.M + m];
    if (vs_beats(c.v, c.i, top, idx)) { top = c.v; idx = c.i; }
  }
  // top NaN: NaN; +inf: +inf; -inf (every logit is -inf): -inf; else top + logf(S), a slice of -inf alone skipped
  float lse = top;
  if (top - top == 0.f) {
    float s = 0.f;
    for (int t = 0; t < p.NS; ++t) {
      const float mt = p.pick[(int64_t)t * p.M + m].v;
      if (mt != -INFINITY) s += vs_rescale(p.sum[(int64_t)t * p.M + m], mt, top);
    }
    lse = top + logf(s);
  }
  float tl = top;
  if (p.targets) {
    const int64_t t = p.targets[m];
    tl = t >= 0 && t < (int64_t)p.V ? p.tlogit[m] : NAN;   // (no thread of the first launch has written tlogit[m] otherwise)
  }
  p.token[m] = (int64_t)idx;
  if (p.top) p.top[m] = top;
  p.lse[m] = lse;
  p.logp[m] = tl - lse;
}

template <typename E, bool XF32>
int vs_launch(const VocabScoreP& p, hipStream_t st) {
  if (const int e = ea_lds_limit(vocab_score_kernel<E, XF32>, VS_LDS_BYTES)) return e;
  hipLaunchKernelGGL((vocab_score_kernel<E, XF32>), dim3((unsigned)(p.MT * p.NS)), dim3(VS_THREADS), VS_LDS_BYTES, st, p);
  return (int)hipGetLastError();
}

}  // namespace

int64_t vocab_score_ws(int M, int V) {
  if (M < 1 || V < 1) return -1;
  const int64_t MT = ((int64_t)M - 1) / VS_BM + 1, NS = ((int64_t)V - 1) / VS_SL + 1;
  if (MT * NS > VS_MAX_WORKGROUPS) return -1;
  const int64_t bytes = (int64_t)M * NS * (int64_t)(sizeof(VsPick) + sizeof(float)) + (int64_t)M * (int64_t)sizeof(float);
  return (bytes + 15) / 16 * 16;
}

// (Every argument has been checked by the one caller, ea_vocab_score in ea_capi.hip: nothing is checked again here.)
int vocab_score(VocabScoreP p, hipStream_t st) {
  p.MT = (p.M - 1) / VS_BM + 1;
  p.NS = (p.V - 1) / VS_SL + 1;
  p.sum = reinterpret_cast<float*>(p.pick + (int64_t)p.M * p.NS);
  p.tlogit = p.sum + (int64_t)p.M * p.NS;
  int rc;
  if (p.dtype == EA_BF16) rc = p.x_f32 ? vs_launch<BF16, true>(p, st) : vs_launch<BF16, false>(p, st);
  else rc = p.x_f32 ? vs_launch<F16, true>(p, st) : vs_launch<F16, false>(p, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(vocab_score_fold_kernel, dim3((unsigned)((p.M - 1) / VS_FOLD_THREADS + 1)), dim3(VS_FOLD_THREADS), 0, st,
                     p);
  return (int)hipGetLastError();
}

}  // namespace ea
