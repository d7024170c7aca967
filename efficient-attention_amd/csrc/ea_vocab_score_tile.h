// ea_vocab_score_tile.h -- the tile loop of the many-row vocabulary pass and its fold, as templates: ONE body behind
// ea_vocab_score (ea_vocab_score.hip, ROWS = false) and ea_vocab_score_rows / ea_adaptive_score (ea_adaptive_score.hip, ROWS =
// true).  The design is described at the head of ea_vocab_score.hip.
//
// ROWS = false takes a VocabScoreP and is the kernel of ABI 30: every `if constexpr (ROWS)` falls away.
// ROWS = true takes a VocabScoreRowsP: the M positions of the call name rows of x (xrows) and of targets (trows) through
// int32 lists, only the first *count of them are live, target_base is taken off a target before the range test, and
// logits_only skips the pick / log-sum-exp bookkeeping (the tile loop as a plain GEMM with a 16-bit store).  A workgroup
// whose row tile starts at or beyond the live count returns before its first operand load; inside the last live tile a
// position >= live is clamped to position live - 1 BEFORE a list is read (the clamp to row M - 1 of ROWS = false), so a list
// entry at or beyond the count is never dereferenced; nothing is written at such a position (VS_EPI_GRAD, below, writes ZEROS
// there, from dead workgroups too: its outputs are contracted over).  With no lists, no count and
// base 0 the arithmetic is that of ROWS = false, operation for operation: the same bits.
//
// EPI picks what stands behind a column block's last k stage (ABI 38, ea_vocab_nll.hip; with ROWS = true: ea_adaptive_nll.hip,
// where VS_EPI_GRAD writes zeros at dead positions and VS_EPI_GEMM sends its output rows through a list):
//   VS_EPI_SCORE  the above: every `if constexpr` on EPI falls away and the kernels of ABI 30 / 33 are what they were.
//   VS_EPI_GRAD   a VocabNllGradP: the logit tiles of the table's columns [v0, v0 + Vc) are formed again -- the same k order
//                 per accumulator, so the same bits -- and G = d ((v == target) - expf(a - lse)) is stored in 16 bits, row-major
//                 and transposed.  The table rows of a block are staged in LDS in a permuted order, so that a lane's four
//                 accumulator tiles are four CONSECUTIVE columns: both images are written with 8-byte stores.
//   VS_EPI_GEMM   a GemmNt16P: the loop as a plain GEMM, out (+)= a b^T in fp32; b has a row stride of its own, and a "slice"
//                 is one column block (there is nothing to fold across blocks, and narrow outputs get a wider grid).
#pragma once
#include <limits.h>
#include <math.h>
#include <type_traits>
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

template <bool ROWS> using VsParams = std::conditional_t<ROWS, VocabScoreRowsP, VocabScoreP>;

constexpr int VS_EPI_SCORE = 0, VS_EPI_GRAD = 1, VS_EPI_GEMM = 2;
template <bool ROWS, int EPI> struct VsEpiParams { using type = VsParams<ROWS>; };
template <> struct VsEpiParams<false, VS_EPI_GRAD> { using type = VocabNllGradP; };
template <> struct VsEpiParams<false, VS_EPI_GEMM> { using type = GemmNt16P; };
template <> struct VsEpiParams<true, VS_EPI_GRAD> { using type = VocabNllGradRowsP; };
template <> struct VsEpiParams<true, VS_EPI_GEMM> { using type = GemmNt16RowsP; };

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

// zeros in rows [r0, r1) x columns [c0, c1) of a 16-bit image of row stride ld, by the workgroup's threads together: the image
// is 16-byte aligned, ld and c1 are multiples of 8; 2-byte stores up to the first multiple of 8, 16-byte stores behind it
EA_DEV void vs_zero_block(uint16_t* img, int64_t ld, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int tid) {
  if (r1 <= r0 || c1 <= c0) return;
  const int64_t a0 = min(c1, (c0 + 7) / 8 * 8);
  const int64_t hn = a0 - c0, per = hn + (c1 - a0) / 8, n = per * (r1 - r0);
  for (int64_t at = tid; at < n; at += VS_THREADS) {
    const int64_t r = at / per, i = at - r * per;
    uint16_t* row = img + (r0 + r) * ld;
    if (i < hn) row[c0 + i] = 0;
    else *reinterpret_cast<u32x4*>(row + a0 + 8 * (i - hn)) = u32x4{0u, 0u, 0u, 0u};
  }
}

// how many of the call's M positions are live: M itself, or the device count, kept inside [0, M]
template <bool ROWS> EA_DEV int vs_live(const VsParams<ROWS>& p) {
  if constexpr (ROWS) {
    if (p.count) return max(0, min(*p.count, p.M));
  }
  return p.M;
}

// the target of live position m, target_base taken off: in [0, V), or -1
template <bool ROWS> EA_DEV int32_t vs_target(const VsParams<ROWS>& p, int m) {
  if constexpr (ROWS) {
    const int64_t t = p.targets[p.trows ? (int64_t)p.trows[m] : (int64_t)m];
    return t >= p.target_base && t - p.target_base < (int64_t)p.V ? (int32_t)(t - p.target_base) : -1;
  } else {
    const int64_t t = p.targets[m];
    return t >= 0 && t < (int64_t)p.V ? (int32_t)t : -1;
  }
}

template <typename E, bool XF32, bool ROWS, int EPI = VS_EPI_SCORE>
__global__ __launch_bounds__(VS_THREADS) void vocab_score_kernel(const typename VsEpiParams<ROWS, EPI>::type p) {
  constexpr int SL = EPI == VS_EPI_GEMM ? VS_BN : VS_SL;   // columns of one workgroup
  extern __shared__ __attribute__((aligned(16))) char vs_lds[];
  int32_t* tgts = reinterpret_cast<int32_t*>(vs_lds + VS_LDS_TGT);
  float* merge = reinterpret_cast<float*>(vs_lds + VS_LDS_MERGE);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;
  const int slice = blockIdx.x / p.MT;
  const int m0 = (blockIdx.x - slice * p.MT) * VS_BM;
  const int live = vs_live<ROWS>(p);                   // (ROWS = false: p.M)
  if constexpr (ROWS && EPI != VS_EPI_GRAD) {
    if (m0 >= live) return;                            // (uniform: the whole workgroup, before its first operand load)
  }
  int s0 = slice * SL;                                 // (< V)
  int ncols = min(SL, p.V - s0);                       // columns of this slice: at least one
  if constexpr (EPI == VS_EPI_GRAD) {                  // (the chunk's slices: s0 < v0 + Vc <= V)
    s0 += p.v0;
    ncols = min(SL, p.v0 + p.Vc - s0);
  }
  // ROWS, VS_EPI_GRAD: what the two GEMMs contract over and no live position fills, as zeros, each element by this workgroup
  // alone: the tile's positions at or beyond the live count (rows of g, columns of gt) over this slice's columns, the pad
  // columns Vc .. ldg - 1 of the tile's live rows (the chunk's last slice) and the pad columns M .. ldm - 1 of gt (the last
  // row tile).  A workgroup whose whole tile is dead does this and returns before its first operand load.
  if constexpr (ROWS && EPI == VS_EPI_GRAD) {
    const int64_t rend = min(m0 + VS_BM, p.M), rl = min((int64_t)max(live, m0), rend);
    const int64_t tile_end = m0 + VS_BM >= p.M ? p.ldm : m0 + VS_BM;
    const int64_t c_lo = (int64_t)slice * SL, c_hi = slice == p.NS - 1 ? p.ldg : c_lo + ncols;
    vs_zero_block(p.g, p.ldg, rl, rend, c_lo, c_hi, tid);
    if (slice == p.NS - 1) vs_zero_block(p.g, p.ldg, m0, rl, p.Vc, p.ldg, tid);
    vs_zero_block(p.gt, p.ldm, c_lo, c_lo + ncols, rl, tile_end, tid);
    if (m0 >= live) return;                            // (uniform)
  }
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
  for (int q = 0; q < 2; ++q) {
    int64_t r = min(m0 + lr + 64 * q, live - 1);       // the position, clamped before a list is read
    if constexpr (ROWS) {
      if (p.xrows) r = p.xrows[r];
    }
    xrow[q] = p.x + r * p.ldx * (XF32 ? 4 : 2);
  }
  int64_t ldw = p.K;                                   // the row stride of w
  if constexpr (EPI == VS_EPI_GEMM) ldw = p.ldw;
  const char* wslice = p.w + (int64_t)s0 * ldw * 2;
  // the table row that tile row lr + 64 q holds: itself, or (VS_EPI_GRAD) tile row 16 j + li of a half holds row 4 li + j
  int wrow[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) wrow[q] = EPI == VS_EPI_GRAD ? 64 * q + 4 * (lr & 15) + (lr >> 4) : lr + 64 * q;
  VsX<XF32> rx[2];
  u32x4 rw[2];
  auto fetch = [&](int blk, int kt) {
    const int k = kt * VS_BK + 8 * lc;
    if (k < p.K) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        rx[q].load(xrow[q], k);
        const int n = min(blk * VS_BN + wrow[q], ncols - 1);       // (a column past V: the slice's last row again)
        rw[q] = ldg16(wslice + ((int64_t)n * ldw + k) * 2);
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
    tgts[tid] = p.targets && m < live ? vs_target<ROWS>(p, m) : -1;
  }
  bool bookkeeping = true;                             // (uniform)
  if constexpr (ROWS) bookkeeping = !p.logits_only;
  if constexpr (EPI != VS_EPI_SCORE) bookkeeping = false;
  // VS_EPI_GRAD: d and lse of row 16 i + 4 g + r (of the wave's 32), entry 4 i + r; a row >= M: d = 0
  float gd[8], gl[8];
  if constexpr (EPI == VS_EPI_GRAD) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int m = m0 + wm * 32 + 16 * (q >> 2) + 4 * g + (q & 3);
      if constexpr (ROWS) gd[q] = m < live ? p.d[p.trows ? (int64_t)p.trows[m] : (int64_t)m] : 0.f;
      else gd[q] = m < live ? p.d[m] : 0.f;
      gl[q] = m < live ? p.lse_in[m] : 0.f;
    }
  }
  // ROWS, VS_EPI_GEMM: the row of out that position 16 i + 4 g + r (of the wave's 32) writes, entry 4 i + r
  [[maybe_unused]] int64_t orow[8];
  if constexpr (ROWS && EPI == VS_EPI_GEMM) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int m = m0 + wm * 32 + 16 * (q >> 2) + 4 * g + (q & 3);
      orow[q] = m < live && p.orows ? (int64_t)p.orows[m] : (int64_t)m;
    }
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
      if constexpr (EPI == VS_EPI_GRAD) {
        // this lane's columns are 4 li + j of its wave's 64; cb: the first of them, within the chunk
        const int cb = slice * SL + blk * VS_BN + wn * 64 + 4 * li;
        uint16_t gv[2][4][4];                          // [i][r][j]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = 4 * i + r;
            const int tgt = tgts[wm * 32 + 16 * i + 4 * g + r];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float hit = p.v0 + cb + j == tgt ? 1.f : 0.f;
              const float gf = gd[q] * (hit - expf(acc[i][j][r] - gl[q]));
              gv[i][r][j] = gd[q] == 0.f ? (uint16_t)0 : E::from_f(gf);   // (a select: such a row's logits may be NaN)
            }
          }
        const int mb = m0 + wm * 32 + 4 * g;           // this lane's first row
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = mb + 16 * i + r;
            if (m >= live) continue;
            uint16_t* at = p.g + (int64_t)m * p.ldg + cb;
            if (cb + 3 < p.Vc) {
              *reinterpret_cast<u32x2*>(at) = u32x2{(uint32_t)gv[i][r][0] | (uint32_t)gv[i][r][1] << 16,
                                                    (uint32_t)gv[i][r][2] | (uint32_t)gv[i][r][3] << 16};
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (cb + j < p.Vc) at[j] = gv[i][r][j];
            }
          }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (cb + j >= p.Vc) continue;
            const int m = mb + 16 * i;
            uint16_t* at = p.gt + (int64_t)(cb + j) * p.ldm + m;
            if (m + 3 < live) {
              *reinterpret_cast<u32x2*>(at) = u32x2{(uint32_t)gv[i][0][j] | (uint32_t)gv[i][1][j] << 16,
                                                    (uint32_t)gv[i][2][j] | (uint32_t)gv[i][3][j] << 16};
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (m + r < live) at[r] = gv[i][r][j];
            }
          }
      } else if constexpr (EPI == VS_EPI_GEMM) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * 32 + 16 * i + 4 * g + r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int cs = c0 + 16 * j;
              if (cs < ncols && m < live) {
                int64_t om = m;
                if constexpr (ROWS) om = orow[4 * i + r];
                float* at = reinterpret_cast<float*>(p.logits) + om * p.ldl + s0 + cs;
                *at = p.accumulate ? *at + acc[i][j][r] : acc[i][j][r];
              }
            }
          }
      } else if (p.logits) {                           // (uniform; the tests' and a curious caller's path)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * 32 + 16 * i + 4 * g + r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int cs = c0 + 16 * j;
              if (cs < ncols && m < live) {
                const float a = acc[i][j][r];
                if (p.l_f32) reinterpret_cast<float*>(p.logits)[(int64_t)m * p.ldl + s0 + cs] = a;
                else reinterpret_cast<uint16_t*>(p.logits)[(int64_t)m * p.ldl + s0 + cs] = E::from_f(a);
              }
            }
          }
      }
      if (bookkeeping) {
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
              const bool live_c = cs < ncols;
              const int col = s0 + (live_c ? cs : 0);
              const float a = acc[i][j][r];
              v[j] = live_c ? a : -INFINITY;
              tl[q] = (live_c & (col == tgt)) ? a : tl[q];
              const bool take = live_c & vs_beats(a, col, bv[q], bi[q]);
              bv[q] = take ? a : bv[q];
              bi[q] = take ? col : bi[q];
            }
            const float mnew = bv[q];
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = v[j] == -INFINITY ? 0.f : expf(v[j] - mnew);
            bs[q] = vs_rescale(bs[q], mold, mnew) + ((e[0] + e[1]) + (e[2] + e[3]));
          }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    blk = blk_next; kt = kt_next;
    __syncthreads();
  }
  if constexpr (EPI == VS_EPI_GRAD && !ROWS) {
    // the pad positions the two GEMMs contract over, as zeros: columns Vc .. ldg - 1 of this tile's rows of G by the
    // workgroups of the chunk's last slice, rows M .. ldm - 1 of this slice's rows of G^T by those of the last row tile
    if (slice == p.NS - 1) {
      const int64_t np = p.ldg - p.Vc, n = np * min(VS_BM, live - m0);
      for (int64_t at = tid; at < n; at += VS_THREADS) {
        const int64_t r = at / np;
        p.g[(m0 + r) * p.ldg + p.Vc + (at - r * np)] = 0;
      }
    }
    if (m0 + VS_BM >= live) {
      const int64_t np = p.ldm - live, n = np * ncols;
      for (int64_t at = tid; at < n; at += VS_THREADS) {
        const int64_t c = at / np;
        p.gt[((int64_t)slice * SL + c) * p.ldm + live + (at - c * np)] = 0;
      }
    }
  }
  if (!bookkeeping) return;                            // (uniform: a plain GEMM has no partials)

  // the target's logit: stored by the one lane whose columns hold it
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int row = wm * 32 + 16 * (q >> 2) + 4 * g + (q & 3);
    const int tgt = tgts[row];
    const int cs = tgt - s0;                           // (tgt is -1 or in [0, V))
    if (tgt >= 0 && cs >= 0 && cs < ncols && (cs & 15) == li && ((cs >> 6) & 1) == wn && m0 + row < live) p.tlogit[m0 + row] = tl[q];
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
      if (m < live) {
        const int64_t at = (int64_t)slice * p.M + m;
        p.pick[at] = VsPick{mv, mi};
        p.sum[at] = s;
      }
    }
  }
}

// launch two: one thread per row folds the row's NS partials in slice order
template <bool ROWS>
__global__ __launch_bounds__(VS_FOLD_THREADS) void vocab_score_fold_kernel(const VsParams<ROWS> p) {
  const int64_t m = (int64_t)blockIdx.x * VS_FOLD_THREADS + threadIdx.x;
  if (m >= vs_live<ROWS>(p)) return;
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
  if (p.targets) tl = vs_target<ROWS>(p, (int)m) >= 0 ? p.tlogit[m] : NAN;   // (no thread of the first launch has written tlogit[m] otherwise)
  p.token[m] = (int64_t)idx;
  if (p.top) p.top[m] = top;
  p.lse[m] = lse;
  p.logp[m] = tl - lse;
}

// the two launches on a filled parameter block (MT, NS, sum, tlogit set by the caller); ROWS with logits_only: the first alone
template <typename E, bool XF32, bool ROWS, int EPI = VS_EPI_SCORE>
int vs_launch(const typename VsEpiParams<ROWS, EPI>::type& p, hipStream_t st) {
  if (const int e = ea_lds_limit(vocab_score_kernel<E, XF32, ROWS, EPI>, VS_LDS_BYTES)) return e;
  hipLaunchKernelGGL((vocab_score_kernel<E, XF32, ROWS, EPI>), dim3((unsigned)(p.MT * p.NS)), dim3(VS_THREADS), VS_LDS_BYTES, st,
                     p);
  return (int)hipGetLastError();
}

template <bool ROWS>
int vs_launch_fold(const VsParams<ROWS>& p, hipStream_t st) {
  hipLaunchKernelGGL(vocab_score_fold_kernel<ROWS>, dim3((unsigned)((p.M - 1) / VS_FOLD_THREADS + 1)), dim3(VS_FOLD_THREADS), 0,
                     st, p);
  return (int)hipGetLastError();
}

template <bool ROWS>
int vs_launch_typed(const VsParams<ROWS>& p, hipStream_t st) {
  if (p.dtype == EA_BF16) return p.x_f32 ? vs_launch<BF16, true, ROWS>(p, st) : vs_launch<BF16, false, ROWS>(p, st);
  return p.x_f32 ? vs_launch<F16, true, ROWS>(p, st) : vs_launch<F16, false, ROWS>(p, st);
}

}  // namespace
}  // namespace ea
