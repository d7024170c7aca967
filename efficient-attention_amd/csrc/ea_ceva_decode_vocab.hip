// ea_ceva_decode_vocab.hip -- the greedy token pick of a decoding step on a vocabulary table the state holds (ABI 26)
//
//   logit[m, v] = sum_k round_w(x[m, k]) w[v, k]            fp32, no bias;  1 <= M <= 64 rows, w [V, K] 16-bit row-major
//   token[m]    = argmax_v logit[m, v]                      the largest value; equal values: the lowest index; a row with NaN
//   top[m]      = logit[m, token[m]]                        logits: the lowest index that holds one (torch.argmax's rule)
//
// The step is bound by reading w once (2 V K bytes: 67 MB at V = 32768, K = 1024).  ceva_vocab_kernel is the tile loop of
// ceva_linear_kernel (ea_ceva_decode_linear.hip, whose instructions are pinned and which is therefore not touched): w is the
// B operand of v_mfma_f32_16x16x32, one 16-byte global load per lane straight into the operand registers; the 8 waves of a
// workgroup split K into contiguous runs of 32-wide k-steps, NS steps in flight; the partial tiles meet in LDS and the
// thread that owns an element adds them in wave order.  An element's sum is formed by the same operations in the same order
// as ceva_linear_kernel forms it: the logits are that kernel's bits.
//
// One workgroup owns VOC_TILE = 16 columns (one column tile) and all row tiles.  The last tile may reach past V: its
// addresses are clamped to row V - 1, and a column >= V is neither stored nor picked.  Epilogue: the thread that holds a summed
// element stores it when logits are asked for; the 16 lanes that hold a row's 16 columns reduce them to one (value, index)
// candidate by lane exchanges and write it to ws[m][workgroup].  ceva_vocab_pick_kernel, one workgroup per row, reduces the
// row's ceil(V / 16) candidates under the same rule and writes token[m] (int64) and top[m].  The rule is a total order on
// (value, index) pairs with distinct indices, so the pick does not depend on the order of the reduction; the order is fixed all
// the same.  No atomics, no workgroup waits for another: a replay repeats the bits.
#include <limits.h>
#include <math.h>
#include "ea_common.h"
#include "ea_ceva_decode_vocab.h"

namespace ea {
namespace {

constexpr int VOC_NW = 8;              // waves per workgroup
constexpr int VOC_NS = 4;              // k-steps a wave loads ahead
constexpr int PICK_THREADS = 512;

static_assert(sizeof(VocPick) == 8, "a candidate is one 8-byte store");

// eight consecutive k of one row of x as they lie in memory, and as the A operand (fp32: rounded to nearest even)
template <bool XF32> struct VocX;
template <> struct VocX<true> {
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
template <> struct VocX<false> {
  u32x4 v;
  EA_DEV void load(const char* xrow, int k) { v = ldg16(xrow + (int64_t)k * 2); }
  template <typename E> EA_DEV u32x4 frag() const { return v; }
};

// a takes b's place: a NaN beats every number, a larger number a smaller one, and of two equals (two NaNs, +0 and -0) the
// lower index
EA_DEV bool voc_beats(const VocPick a, const VocPick b) {
  const bool an = a.v != a.v, bn = b.v != b.v;
  if (an || bn) return an && (!bn || a.i < b.i);
  return a.v > b.v || (a.v == b.v && a.i < b.i);
}

// what every candidate beats: no column
EA_DEV VocPick voc_none() { return VocPick{-INFINITY, INT_MAX}; }

EA_DEV VocPick voc_exchange(const VocPick c, int lane_xor) {
  return VocPick{__shfl_xor(c.v, lane_xor), __shfl_xor(c.i, lane_xor)};
}

template <typename E, bool XF32, int RT>
__global__ __launch_bounds__(VOC_NW * 64) void ceva_vocab_kernel(const DecVocabP p) {
  __shared__ float red[VOC_NW * RT * 256];            // [wave][row tile][16 rows][16 columns]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.x * VOC_TILE;
  const int KS = p.K >> 5;
  const int S = (KS + VOC_NW - 1) / VOC_NW;
  const int s_begin = wave * S, s_end = min(KS, s_begin + S);
  const int live_cols = min(VOC_TILE, p.V - n0);      // columns of this tile below V: at least one
  const char* wrow = p.w + ((int64_t)(n0 + min(li, live_cols - 1)) * p.K + 8 * g) * 2;  // (a column past V: row V - 1 again)
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
  for (int s0 = s_begin; s0 < s_end; s0 += VOC_NS) {
    u32x4 wf[VOC_NS];
    VocX<XF32> xr[VOC_NS][RT];
#pragma unroll
    for (int i = 0; i < VOC_NS; ++i) {                 // (a step past the wave's run: a clamped address, a zero operand below)
      const int s = min(s0 + i, KS - 1);
      wf[i] = ldg16(wrow + (int64_t)s * 64);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) xr[i][rt].load(xrow[rt], s * 32 + 8 * g);
    }
    __builtin_amdgcn_sched_barrier(0);                 // every load of the pass is out before the first conversion and MFMA
#pragma unroll
    for (int i = 0; i < VOC_NS; ++i) {
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
  const int NB = (p.V - 1) / VOC_TILE + 1;
  // (whole waves enter or skip an iteration: 256 elements are four waves; a row's 16 columns are 16 lanes in a row)
  for (int e = threadIdx.x; e < RT * 256; e += VOC_NW * 64) {
    const int rt = e >> 8, idx = e & 255, m = rt * 16 + (idx >> 4), n = n0 + (idx & 15);
    const bool col = (idx & 15) < live_cols;
    float v = red[rt * 256 + idx];
#pragma unroll
    for (int w = 1; w < VOC_NW; ++w) v += red[(w * RT + rt) * 256 + idx];
    if (m < p.M && col && p.logits) {
      if (p.l_f32) reinterpret_cast<float*>(p.logits)[(int64_t)m * p.ldl + n] = v;
      else reinterpret_cast<uint16_t*>(p.logits)[(int64_t)m * p.ldl + n] = E::from_f(v);
    }
    VocPick c = col ? VocPick{v, n} : voc_none();
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const VocPick other = voc_exchange(c, o);
      if (voc_beats(other, c)) c = other;
    }
    if (m < p.M && (idx & 15) == 0) p.ws[(int64_t)m * NB + blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(PICK_THREADS) void ceva_vocab_pick_kernel(const DecVocabP p) {
  __shared__ VocPick best[PICK_THREADS / 64];
  const int m = blockIdx.x;
  const int NB = (p.V - 1) / VOC_TILE + 1;
  const VocPick* row = p.ws + (int64_t)m * NB;
  VocPick c = voc_none();
#pragma unroll 4
  for (int j = threadIdx.x; j < NB; j += PICK_THREADS) {
    const VocPick other = row[j];
    if (voc_beats(other, c)) c = other;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const VocPick other = voc_exchange(c, o);
    if (voc_beats(other, c)) c = other;
  }
  if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < PICK_THREADS / 64; ++w)
      if (voc_beats(best[w], c)) c = best[w];
    p.token[m] = (int64_t)c.i;
    if (p.top) p.top[m] = c.v;
  }
}

using VocKernel = void (*)(const DecVocabP);

template <typename E, bool XF32>
VocKernel voc_of(int M) {
  if (M <= 16) return ceva_vocab_kernel<E, XF32, 1>;
  if (M <= 32) return ceva_vocab_kernel<E, XF32, 2>;
  return ceva_vocab_kernel<E, XF32, 4>;
}

template <typename E>
VocKernel voc_of(bool xf32, int M) { return xf32 ? voc_of<E, true>(M) : voc_of<E, false>(M); }

}  // namespace

int64_t ceva_sdecode_vocab_ws(int M, int V) {
  if (M < 1 || M > EA_CEVA_LINEAR_MAX_ROWS || V < 1) return -1;
  return (int64_t)M * ((V - 1) / VOC_TILE + 1) * (int64_t)sizeof(VocPick);
}

// (The C entry point has checked pointers, strides, alignment and the size of ws.)
int ceva_sdecode_vocab_argmax(const DecVocabP& p, hipStream_t st) {
  if (!p.x || !p.w || !p.ws || !p.token || p.M < 1 || p.ldx < p.K || (p.logits && p.ldl < p.V)) return EA_E_BADARG;
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.V < 1) return EA_E_UNSUPPORTED;
  VocKernel kernel;
  switch (p.dtype) {
    case EA_BF16: kernel = voc_of<BF16>(p.x_f32 != 0, p.M); break;
    case EA_F16: kernel = voc_of<F16>(p.x_f32 != 0, p.M); break;
    default: return EA_E_BADARG;
  }
  const unsigned NB = (unsigned)((p.V - 1) / VOC_TILE + 1);
  hipLaunchKernelGGL(kernel, dim3(NB), dim3(VOC_NW * 64), 0, st, p);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ceva_vocab_pick_kernel, dim3((unsigned)p.M), dim3(PICK_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace ea
