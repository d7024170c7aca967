// ea_ceva_decode_rows.h -- the few-row tile kernel of a decoding step: up to 64 rows of x against a 16-bit table the state holds.
// Included by ea_ceva_decode_linear.hip and ea_ceva_decode_vocab.hip, inside their anonymous namespace, after ea_common.h,
// <type_traits> and the two headers that declare the parameter blocks.
//
//   acc[m, n] = sum_k round_w(x[m, k]) w[n, k]        fp32;  1 <= M <= 64 rows, w [N, K] 16-bit row-major, K % 32 == 0
//
// A step of a handful of rows is bound by reading w once: 6 MB (qkv) and 2 MB (out) at C = 1024, 67 MB for a vocabulary of
// 32768, against 8 .. 64 rows of x.  v_mfma_f32_16x16x32 takes w as its B operand with no staging at all: lane
// (g = lane >> 4, li = lane & 15) holds B[k = 8 g .. 8 g + 7][col = li] = w[n0 + li][k0 + 8 g ..], eight consecutive k of
// one weight row = one 16-byte global load straight into the operand registers.  x is the A operand, read from global memory
// the same way (row li of a 16-row tile; a few KB that every workgroup shares, so L2 serves them), rounded to the weight's
// type on load when it arrives in fp32.
//
// One workgroup owns 16 output columns and all (up to four) 16-row tiles of x.  Its NW waves split K into contiguous runs of
// 32-wide k-steps (wave s: steps s S .. s S + S - 1, S = ceil(K / 32 / NW)), so that a wave reads S 64-byte pieces in a row of
// every weight row; the body is branch-free (addresses clamped, operands zeroed by select), NS steps unrolled, so all of a
// wave's loads are issued ahead of its first MFMA: K <= 32 NS NW = 1024 is one pass.  The waves' partial tiles meet in LDS
// and are added in wave order by the threads that store them: no atomics, no workgroup waits for another -- a replay
// repeats the sums bit for bit, and every variant forms an element's sum by the same operations in the same order.  Rows >= M
// of a tile are zero operands and are never stored.
//
// ceva_rows_kernel is that loop ONCE; the parameter block P it is instantiated on says what stands around it:
//
//   DecLinP       y = round_y(acc + bias)                                                            (ABI 22)
//   DecLinFusedP  y = round_y(act(acc' + bias) + res), acc' on LN(x) when LN                         (ABI 24)
//   DecVocabP     logits = acc (stored when asked for), one (value, index) candidate per row and tile (ABI 26, 27)
//   DecLseP       DecVocabP's, the targets' logits and one sum exp(logit - tile maximum) per row and tile (ABI 28)
//
// Each variant's part is an `if constexpr` inside the one body, NOT a function the kernels call: a called helper, however it
// takes its operands, came out of hipcc with a differently scheduled loop, while this form gives every instance the
// instructions and the descriptor the four separately written kernels had (tools/isa_diff.py --by-code).
//
// LN prologue (DecLinFusedP with gamma and beta): every workgroup computes (mean, rstd) of its M rows over K in fp32 -- two
// passes, biased variance, rsqrt(var + eps), the definition of ea_layernorm_fwd -- one wave per row, rows wave, wave + 8, ..;
// the statistics go to LDS and each lane keeps those of its RT operand rows.  An operand is then (x - mean) rstd gamma + beta
// in fp32, rounded ONCE to the weight's type as it is loaded: where the full path under autocast rounds (fp32 layer_norm
// output cast by the Linear).  That costs every workgroup a second read of x (M K elements, L2) and saves a launch and an
// [M, K] round trip.
//
// Linear epilogue: the thread that sums an element over the waves applies bias and, fused, ReLU and the residual (fp32 or the
// weight's type) in fp32 and stores it; res may be y itself (the element is read and written by the same thread), x may not
// be y (other workgroups still read it).
//
// Vocab epilogue: the last column tile may reach past V: its addresses are clamped to row V - 1, and a column >= V is neither
// stored nor picked.  The thread that holds a summed element stores it when logits are asked for; the 16 lanes that hold a
// row's 16 columns reduce them to one (value, index) candidate by lane exchanges and write it to ws[m][workgroup].  DecLseP:
// behind the exchange the 16 lanes of a row group all hold the tile's best (m_t, i_t), and s_t = sum_columns
// exp(logit - m_t) goes to lws[m][tile].

constexpr int LIN_NW = 8;              // waves per workgroup
constexpr int LIN_NS = 4;              // k-steps a wave loads ahead
static_assert(VOC_TILE == 16, "a workgroup's columns are one MFMA column tile");

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

// k-steps a wave loads ahead: four; the fp32-x, four-row-tile LayerNorm instance holds 4 x 8 fp32 of x plus gamma and beta
// per step and takes two
template <bool XF32, int RT, bool LN> constexpr int fused_ns() { return LN && XF32 && RT == 4 ? 2 : LIN_NS; }

// eight consecutive k of one row of x as floats (the statistics, and the normalised operand)
template <typename E> EA_DEV void lin_floats(const LinX<true>& x, float* f) {
  f[0] = x.a[0]; f[1] = x.a[1]; f[2] = x.a[2]; f[3] = x.a[3]; f[4] = x.b[0]; f[5] = x.b[1]; f[6] = x.b[2]; f[7] = x.b[3];
}
template <typename E> EA_DEV void lin_floats(const LinX<false>& x, float* f) { unpack8<E>(x.v, f); }

// a takes b's place: a NaN beats every number, a larger number a smaller one, and of two equals (two NaNs, +0 and -0) the
// lower index.  A total order on (value, index) pairs with distinct indices, so a pick does not depend on the order of its
// reduction; the order is fixed all the same.
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

template <typename E, bool XF32, bool YF32, int RT, bool LN, typename P>
__global__ __launch_bounds__(LIN_NW * 64) void ceva_rows_kernel(const P p) {
  constexpr bool FUSED = std::is_same<P, DecLinFusedP>::value;
  constexpr bool LSE = std::is_same<P, DecLseP>::value;
  constexpr bool VOCAB = LSE || std::is_same<P, DecVocabP>::value;
  static_assert(FUSED || VOCAB || std::is_same<P, DecLinP>::value, "one of the four parameter blocks");
  static_assert(FUSED || !LN, "the LayerNorm prologue belongs to the fused linear");
  static_assert(!VOCAB || !YF32, "the vocab passes have no y");
  constexpr int NS = fused_ns<XF32, RT, LN>();
  __shared__ float red[LIN_NW * RT * 256];            // [wave][row tile][16 rows][16 columns]
  __shared__ float stat[LN ? 2 * EA_LIN_MAX_ROWS : 2];  // (mean, rstd) of row m
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.x * VOC_TILE;
  const int KS = p.K >> 5;
  const int S = (KS + LIN_NW - 1) / LIN_NW;
  const int s_begin = wave * S, s_end = min(KS, s_begin + S);
  int live_cols = VOC_TILE;                           // columns of this tile below V: at least one
  const char* wrow;
  if constexpr (VOCAB) {
    live_cols = min(VOC_TILE, p.V - n0);
    wrow = p.w + ((int64_t)(n0 + min(li, live_cols - 1)) * p.K + 8 * g) * 2;  // (a column past V: row V - 1 again)
  } else {
    wrow = p.w + ((int64_t)(n0 + li) * p.K + 8 * g) * 2;
  }
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
  // D[row = 4 g + r][col = li] of every row tile -> LDS; then element e of the [16 RT, 16] tile is summed over the waves,
  // in wave order, by one thread
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * RT + rt) * 256 + (4 * g + r) * 16 + li] = acc[rt][r];
  __syncthreads();
  // (vocab: whole waves enter or skip an iteration: 256 elements are four waves; a row's 16 columns are 16 lanes in a row)
  for (int e = threadIdx.x; e < RT * 256; e += LIN_NW * 64) {
    const int rt = e >> 8, idx = e & 255, m = rt * 16 + (idx >> 4), n = n0 + (idx & 15);
    if constexpr (!VOCAB) {
      if (m >= p.M) continue;
    }
    const bool col = (idx & 15) < live_cols;
    float v = red[rt * 256 + idx];
#pragma unroll
    for (int w = 1; w < LIN_NW; ++w) v += red[(w * RT + rt) * 256 + idx];
    if constexpr (VOCAB) {
      const int NB = (p.V - 1) / VOC_TILE + 1;
      if (m < p.M && col && p.logits) {
        if (p.l_f32) reinterpret_cast<float*>(p.logits)[(int64_t)m * p.ldl + n] = v;
        else reinterpret_cast<uint16_t*>(p.logits)[(int64_t)m * p.ldl + n] = E::from_f(v);
      }
      if constexpr (LSE) {
        if (p.targets && m < p.M && col && p.targets[m] == (int64_t)n) p.tlogit[m] = v;
      }
      VocPick c = col ? VocPick{v, n} : voc_none();
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const VocPick other = voc_exchange(c, o);
        if (voc_beats(other, c)) c = other;
      }
      if constexpr (LSE) {
        // every lane of the row group holds (m_t, i_t) now; a column >= V adds nothing.  (m_t NaN or infinite: s_t is
        // whatever comes out -- the second launch does not read it then)
        float s = col ? expf(v - c.v) : 0.f;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (m < p.M && (idx & 15) == 0) {
          p.ws[(int64_t)m * NB + blockIdx.x] = c;
          p.lws[(int64_t)m * NB + blockIdx.x] = s;
        }
      } else {
        if (m < p.M && (idx & 15) == 0) p.ws[(int64_t)m * NB + blockIdx.x] = c;
      }
    } else {
      if (p.bias) v += E::to_f(reinterpret_cast<const uint16_t*>(p.bias)[n]);
      if constexpr (FUSED) {
        if (p.act == 1) v = v < 0.f ? 0.f : v;           // (a NaN stays one)
        if (p.res) {
          if (p.res_f32) v += reinterpret_cast<const float*>(p.res)[(int64_t)m * p.ldr + n];
          else v += E::to_f(reinterpret_cast<const uint16_t*>(p.res)[(int64_t)m * p.ldr + n]);
        }
      }
      if constexpr (YF32) reinterpret_cast<float*>(p.y)[(int64_t)m * p.ldy + n] = v;
      else reinterpret_cast<uint16_t*>(p.y)[(int64_t)m * p.ldy + n] = E::from_f(v);
    }
  }
}

// ---- which instance serves a block ----------------------------------------------------------------------------------------
template <typename P> using RowsKernel = void (*)(const P);

template <typename P, typename E, bool XF32, bool YF32, bool LN>
RowsKernel<P> rows_kernel_of(int M) {
  if (M <= 16) return ceva_rows_kernel<E, XF32, YF32, 1, LN, P>;
  if (M <= 32) return ceva_rows_kernel<E, XF32, YF32, 2, LN, P>;
  return ceva_rows_kernel<E, XF32, YF32, 4, LN, P>;
}

// y and the LayerNorm are the linear blocks' own
template <typename P, typename E, bool XF32>
RowsKernel<P> rows_kernel_of(const P& p) {
  if constexpr (std::is_same<P, DecVocabP>::value || std::is_same<P, DecLseP>::value) {
    return rows_kernel_of<P, E, XF32, false, false>(p.M);
  } else {
    if constexpr (std::is_same<P, DecLinFusedP>::value) {
      if (p.gamma) return p.y_f32 ? rows_kernel_of<P, E, XF32, true, true>(p.M) : rows_kernel_of<P, E, XF32, false, true>(p.M);
    }
    return p.y_f32 ? rows_kernel_of<P, E, XF32, true, false>(p.M) : rows_kernel_of<P, E, XF32, false, false>(p.M);
  }
}

// null: p.dtype is no 16-bit type
template <typename P>
RowsKernel<P> rows_kernel_of(const P& p) {
  switch (p.dtype) {
    case EA_BF16: return p.x_f32 ? rows_kernel_of<P, BF16, true>(p) : rows_kernel_of<P, BF16, false>(p);
    case EA_F16: return p.x_f32 ? rows_kernel_of<P, F16, true>(p) : rows_kernel_of<P, F16, false>(p);
    default: return nullptr;
  }
}

// the launch on `cols` columns of the table: one workgroup per 16
template <typename P>
int rows_launch(RowsKernel<P> kernel, const P& p, int cols, hipStream_t st) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((cols - 1) / VOC_TILE + 1)), dim3(LIN_NW * 64), 0, st, p);
  return (int)hipGetLastError();
}
