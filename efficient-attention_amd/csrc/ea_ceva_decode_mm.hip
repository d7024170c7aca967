// ea_ceva_decode_mm.hip -- attn of a static causal EVA decoding step on the matrix cores: the prompt-step twin of
// ceva_attn_kernel (ea_ceva_decode_step.h), for DEV steps (static and rolling states) on bf16 / fp16 rows of head dim 64 / 128.
//
// The contract is ceva_attn_kernel's.  For token t of window block bk = t / w:
//   local slot j < w + e is token bk w - e + j: the finite fill -5e4 when the slot is absent (before token 0, or not yet
//   decoded), the key is padded, the key is after t, or t itself is padded; otherwise s q.k + bias[t - bk w, j];
//   landmark c (rf_k_bar, beta) is a column iff c < t / r;  out = ONE softmax over both column sets, times [v ; beta].
// `Step` owns where the step starts and how many of its T tokens batch element b has, `Rows` how a token index becomes a
// cache row (ea_ceva_decode.h); a step that does not fit writes NaN rows, the positions of a per-sequence element past its
// own count get zero rows, and a workgroup the step does not need exits at once, uniformly -- all as attn does.
//
// Work split.  One workgroup per (64-query tile, b, h), four waves of 16 queries.  Query groups are aligned to 16 in the
// ABSOLUTE token index (tile 0 starts at 16 floor(t0 / 16)), so with w % 16 == 0 a group never straddles a window block; the
// first and the last group of a step may lie partly outside [t0, t0 + n): those rows are computed masked and never stored.
// The grid holds the most a step of T tokens can need, and the tiles that see the most landmark rows launch first.
//
// Tile walk.  Key and value rows go through double-buffered LDS in tiles of 64 rows, the rows of tile i + 1 requested before
// the MFMAs of tile i.  Local tiles come first: token rows from the first slot of the first group's window to the end of
// the last group's block, addressed through `Rows` (a tile may wrap the ring), rows of absent tokens zero.  With w < 64 the
// four groups lie in different blocks: the workgroup stages the union once and each wave walks the tiles that meet ITS
// block's window, every other column of a tile being no column of its queries (-inf).  Landmark tiles follow, 0 up to the
// one that holds max_t t / r; a wave stops at its own last query's limit, and only the tiles that straddle some query's
// limit take the per-query mask -- those below min_t t / r run unmasked.
//
// Arithmetic and its rounding points.  S^T = K.Q^T accumulates in fp32 on mfma_f32_16x16x32 from 16-bit operands: token rows
// as they are, 16-bit landmark rows (L = E, a compact state) copied, fp32 landmark rows (L = float) rounded to E once, to
// nearest even, while they are stored to LDS -- the one place an operand is rounded; there is no prepare launch and no
// 16-bit image in the state.  Scale, bias, masks and the online softmax (running max and sum) stay in fp32 registers.  P is
// rounded to E for O^T = V^T.P^T (transposed LDS reads, fp32 accumulation); THE ROW SUM IS THE FP32 SUM OF THE UNROUNDED
// WEIGHTS.  The epilogue divides by it and rounds the 16 x D output rows once, stored 16 bytes at a time.
#include "ea_ceva_decode_mm.h"
#include "ea_lm_frag.h"
#include <type_traits>

namespace ea {

namespace {

constexpr int MM_NT = 256;

EA_DEV const char* mm_row(const DecT& t, int b, int h, int n, int esz) {
  return t.p + ((size_t)b * t.sb + (size_t)h * t.sh + (size_t)n * t.sn) * esz;
}

// eight consecutive elements of a row of type X on their way to LDS as elements of E; a row that does not exist comes as zeros
template <typename E, typename X> struct Chunk8 {        // X = E: copied
  u32x4 w;
  static constexpr int BYTES = 16;
  EA_DEV void load(const char* p, bool ok) {
    const u32x4 x = ldg16(p);
    w = ok ? x : u32x4{0u, 0u, 0u, 0u};
  }
  EA_DEV u32x4 bits() const { return w; }
};
template <typename E> struct Chunk8<E, float> {          // fp32 landmark rows: rounded to E, to nearest even, on the way
  f32x4 a, b;
  static constexpr int BYTES = 32;
  EA_DEV void load(const char* p, bool ok) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p), y = *reinterpret_cast<const f32x4*>(p + 16);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    a = ok ? x : z;
    b = ok ? y : z;
  }
  EA_DEV u32x4 bits() const {
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return pack8<E>(f);
  }
};

// output rows r0 .. T - 1 of (b, h) = v in every element: the NaN rows of a step that does not fit, the zero rows of the
// positions that are not the element's tokens
template <typename E, int D>
EA_DEV void mm_fill_rows(const DecP& p, int b, int h, int r0, float v) {
  const uint32_t w = pack2<E>(v, v);
  for (int idx = r0 * (D / 8) + (int)threadIdx.x; idx < p.T * (D / 8); idx += MM_NT) {
    const int i = idx / (D / 8), c = idx - i * (D / 8);
    stg16(const_cast<char*>(mm_row(p.o, b, h, i, 2)) + c * 16, u32x4{w, w, w, w});
  }
}

template <typename E, int D, bool RING, bool SEQ, typename L>
__global__ __launch_bounds__(MM_NT, 2) void ceva_attn_mm_kernel(const DecP p) {
  constexpr int ROWB = D * 2, KS = D / 32, DT = D / 16, DQ = D / 4, TB = DMM_TILE * ROWB;
  constexpr int CPR = D / 8, NCH = DMM_TILE * CPR / MM_NT;
  constexpr float FILL2 = MASK_FILL * LOG2E;
  extern __shared__ __attribute__((aligned(16))) char smem[];          // [2 stages][K tile | V tile], then the key flags
  uint8_t* kflag = reinterpret_cast<uint8_t*>(smem + 4 * TB);          // [2][64]: the row is absent or padded
  constexpr int LSZ = std::is_same<L, float>::value ? 4 : 2;            // bytes of a landmark element
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);           // (a scalar: what follows from it is uniform over the wave)
  typename LaneOffSel<D>::type lo;
  lo.init(lane);
  const int BH = p.B * p.H;
  const int qt = dmm_query_tiles(p.T) - 1 - (int)(blockIdx.x / BH), bh = (int)(blockIdx.x % BH);
  const int b = bh / p.H, h = bh - b * p.H;
  const Step<true, SEQ> step(p, b);
  const int t0 = step.t0, n = step.n(p.T), tend = t0 + n;
  if (!step.fits(p.T, p.cap)) {
    if (qt == 0) mm_fill_rows<E, D>(p, b, h, 0, __builtin_nanf(""));
    return;
  }
  if (SEQ && qt == 0) mm_fill_rows<E, D>(p, b, h, n, 0.f);
  const int base = (t0 / DMM_GROUP) * DMM_GROUP + qt * DMM_TILE;       // the tile's first token
  if (n == 0 || base >= tend) return;                                  // (uniform over the workgroup)

  const Rows<RING> rows{p.ring};
  const int pst = rows.len(p.cap), Wk = p.w + p.e;
  // the wave's query group: one window block; the lane's query
  const int ga = base + wave * DMM_GROUP;
  const bool active = ga < tend;                                       // (ga + 15 >= t0 for every group of the grid)
  const int tq = ga + li;
  const bool qv = tq >= t0 && tq < tend;
  const int bk = ga / p.w, kbase = bk * p.w - p.e;                     // token of the block's local slot 0
  const int qslot = rows.slot(qv ? tq : t0);
  typename E::x8 qf[KS];
  load_frag<E, KS>(qf, mm_row(p.q, b, h, qslot, 2), g, qv);
  const bool qbad = !qv || p.pad[(size_t)b * pst + qslot];             // its local columns are all the fill
  const float* brow = p.bias ? p.bias + (size_t)(tq - bk * p.w) * Wk - kbase : nullptr;      // brow[token]
  const int lim = qv ? tq / p.r : 0;                                   // landmark c is a column iff c < lim
  const int lim_lo = max(ga, t0) / p.r, lim_hi = (min(ga + DMM_GROUP, tend) - 1) / p.r;       // over the wave's queries
  // the workgroup's walk: local tokens [tok_lo, tok_hi) in nloc tiles, then landmark rows [0, lmax) in nlm tiles
  const int wlast = min(3, (tend - 1 - base) / DMM_GROUP);             // its last wave with a query
  const int tok_lo = (base / p.w) * p.w - p.e, tok_hi = ((base + wlast * DMM_GROUP) / p.w + 1) * p.w;
  const int nloc = (tok_hi - tok_lo + DMM_TILE - 1) / DMM_TILE;
  const int lmax = (min(base + DMM_TILE, tend) - 1) / p.r;
  const int nlm = (lmax + DMM_TILE - 1) / DMM_TILE;
  const float scale2 = p.scale * LOG2E;

  float m = -INFINITY, lsum = 0.f;
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // The nt tiles of one kind -- local token rows (LOC) or landmark rows -- through the two LDS stages: tile j + 1 on its way while
  // tile j is multiplied.  A side (K or V) of a tile is fetched into registers and parked in LDS by all 256 threads.  Both sides
  // are in flight over the whole of tile j where the registers allow; fp32 landmark rows at D = 128 are 64 registers a pair, so
  // there (LATE_V) the K side flies over the S^T phase and the V side over the P.V phase.  The first tile of a kind is fetched
  // in the open: once per kind and workgroup.
  auto walk = [&](auto kind, const int nt) {
    constexpr bool LOC = decltype(kind)::value;
    using X = std::conditional_t<LOC, E, L>;
    constexpr bool LATE_V = !LOC && D == 128 && LSZ == 4;
    Chunk8<E, X> ck[NCH], cv[NCH];
    uint8_t kf = 0;                                // LOC, threads < 64: the flag of local row tid
    auto fetch = [&](int j, auto side) {
      constexpr bool V = decltype(side)::value;
      const int r0 = LOC ? tok_lo + j * DMM_TILE : j * DMM_TILE;
      const DecT& src = LOC ? (V ? p.v : p.k) : (V ? p.lv : p.lk);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int idx = tid + i * MM_NT, r = idx / CPR, c = idx - r * CPR, at = r0 + r;
        // a token row that exists, through the ring; a landmark row up to the last visible one (they have been closed)
        const bool ok = LOC ? at >= 0 && at < tend : at < lmax;
        const int rw = LOC ? rows.slot(ok ? at : 0) : (ok ? at : 0);
        const char* ptr = mm_row(src, b, h, rw, LOC ? 2 : LSZ) + c * Chunk8<E, X>::BYTES;
        if constexpr (V) cv[i].load(ptr, ok);
        else ck[i].load(ptr, ok);
      }
      if (LOC && !V && tid < DMM_TILE) {
        const int tok = r0 + tid;
        const bool ok = tok >= 0 && tok < tend;
        kf = !ok || p.pad[(size_t)b * pst + rows.slot(ok ? tok : 0)];
      }
    };
    auto park = [&](int j, auto side) {
      constexpr bool V = decltype(side)::value;
      char* dst = smem + (j & 1) * 2 * TB + (V ? TB : 0);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int idx = tid + i * MM_NT, r = idx / CPR, c = idx - r * CPR;
        if constexpr (V) sts16(dst + TileL<D>::off(r, c), cv[i].bits());
        else sts16(dst + TileL<D>::off(r, c), ck[i].bits());
      }
      if (LOC && !V && tid < DMM_TILE) kflag[(j & 1) * DMM_TILE + tid] = kf;
    };
    constexpr std::false_type KSIDE{};
    constexpr std::true_type VSIDE{};
    if (nt <= 0) return;                           // (uniform over the workgroup)
    fetch(0, KSIDE);
    fetch(0, VSIDE);
    park(0, KSIDE);
    park(0, VSIDE);
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
      const bool more = j + 1 < nt;
      if (more) {
        fetch(j + 1, KSIDE);
        if (!LATE_V) fetch(j + 1, VSIDE);
      }
      const char* Ks = smem + (j & 1) * 2 * TB;
      const char* Vs = Ks + TB;
      const int r0 = LOC ? tok_lo + j * DMM_TILE : j * DMM_TILE;       // the tile's first token / landmark row
      // does the wave have a column in this tile?  (uniform over the wave)
      const bool work = active && (LOC ? (r0 + DMM_TILE > kbase && r0 < kbase + Wk) : r0 < lim_hi);
      uint32_t pw[4][2];
      if (work) {                                  // S^T, masks, online softmax -> P^T rounded to E
        const bool full = !LOC && r0 + DMM_TILE - 1 < lim_lo;          // every row of the tile is every query's column
        f32x4 s[4];
        float mloc = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) acc = E::mma(as_x8<E>(lds16(Ks + tt * 16 * ROWB + lo.plain[ks])), qf[ks], acc);
          const int c0 = r0 + tt * 16 + 4 * g;                         // the lane's rows c0 .. c0 + 3 of the tile
          if constexpr (LOC) {
            const uint32_t f4 = *reinterpret_cast<const uint32_t*>(kflag + (j & 1) * DMM_TILE + tt * 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int tok = c0 + r;
              float x;
              if (tok < kbase || tok >= kbase + Wk) x = -INFINITY;     // no slot of this block's window
              else if (((f4 >> (8 * r)) & 0xffu) || qbad || tok > tq) x = FILL2;
              else x = acc[r] * scale2 + (brow ? brow[tok] * LOG2E : 0.f);
              acc[r] = x;
              mloc = fmaxf(mloc, x);
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float x = acc[r] * scale2;
              if (!full) x = c0 + r < lim ? x : -INFINITY;
              acc[r] = x;
              mloc = fmaxf(mloc, x);
            }
          }
          s[tt] = acc;
        }
        mloc = quad_max(mloc);
        const float mnew = fmaxf(m, mloc);
        const float msafe = mnew == -INFINITY ? 0.f : mnew;
        const float alpha = fast_exp2(m - msafe);
        m = mnew;
        float psum = 0.f;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          float pv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pv[r] = fast_exp2(s[tt][r] - msafe);
            psum += pv[r];                                             // the normaliser sums the unrounded weights
          }
          pw[tt][0] = pack2<E>(pv[0], pv[1]);
          pw[tt][1] = pack2<E>(pv[2], pv[3]);
        }
        lsum = lsum * alpha + psum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
      }
      if (more) {
        park(j + 1, KSIDE);
        if (LATE_V) fetch(j + 1, VSIDE);
      }
      if (work) {                                  // O^T += V^T.P^T
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const typename E::x8 pf = as_x8<E>(u32x4{pw[2 * kk][0], pw[2 * kk][1], pw[2 * kk + 1][0], pw[2 * kk + 1][1]});
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const u32x2 lo_ = E::tr4(Vs + (2 * kk) * 16 * ROWB + lo.tr[dt]);
            const u32x2 hi_ = E::tr4(Vs + (2 * kk + 1) * 16 * ROWB + lo.tr[dt]);
            o[dt] = E::mma(as_x8<E>(lo_, hi_), pf, o[dt]);
          }
        }
      }
      if (more) park(j + 1, VSIDE);
      __syncthreads();
    }
  };
  walk(std::true_type{}, nloc);
  walk(std::false_type{}, nlm);

  // ---- lane = query li, channels DQ g .. DQ g + DQ - 1: divided by the row sum, rounded once, 16 bytes per store ----
  if (!active) return;                                                 // (uniform over the wave)
  const float inv = 1.f / quad_sum(lsum);
  float f[DQ];
  if constexpr (TileL<D>::NEWTR) {
    quad_transpose_f32(o, f);
  } else {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) f[4 * dt + r] = o[dt][r];
  }
  if (qv) {
    char* dst = const_cast<char*>(mm_row(p.o, b, h, tq - t0, 2)) + DQ * g * 2;
#pragma unroll
    for (int c = 0; c < DQ / 8; ++c) {
      float x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = f[8 * c + i] * inv;
      stg16(dst + c * 16, pack8<E>(x));
    }
  }
}

using MmKernel = void (*)(const DecP);

template <typename E, int D, typename L>
MmKernel mm_kernel_of(bool ring, bool seq) {
  if (ring) return seq ? ceva_attn_mm_kernel<E, D, true, true, L> : ceva_attn_mm_kernel<E, D, true, false, L>;
  return seq ? ceva_attn_mm_kernel<E, D, false, true, L> : ceva_attn_mm_kernel<E, D, false, false, L>;
}
template <typename E, int D>
MmKernel mm_kernel_of(bool ring, bool seq, bool l16) {
  return l16 ? mm_kernel_of<E, D, E>(ring, seq) : mm_kernel_of<E, D, float>(ring, seq);
}

}  // namespace

// RING / SEQ follow the state, as in ceva_decode_launch: p.ring != 0 / p.ntok != null.  (The C entry points have checked the
// ring and the views.)
int ceva_sdecode_attn_mm(const DecP& p, hipStream_t st, bool l16) {
  if (!p.pos || !p.pad) return EA_E_BADARG;
  if ((p.dtype != EA_BF16 && p.dtype != EA_F16) || (p.D != 64 && p.D != 128) || p.w % DMM_GROUP) return EA_E_UNSUPPORTED;
  const bool ring = p.ring != 0, seq = p.ntok != nullptr;
  MmKernel kernel;
  if (p.dtype == EA_BF16) kernel = p.D == 64 ? mm_kernel_of<BF16, 64>(ring, seq, l16) : mm_kernel_of<BF16, 128>(ring, seq, l16);
  else kernel = p.D == 64 ? mm_kernel_of<F16, 64>(ring, seq, l16) : mm_kernel_of<F16, 128>(ring, seq, l16);
  const size_t lds = (size_t)4 * DMM_TILE * p.D * 2 + 2 * DMM_TILE;
  if (const int e = ea_lds_limit(reinterpret_cast<const void*>(kernel), lds)) return e;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(dmm_query_tiles(p.T) * p.B * p.H)), dim3(MM_NT), lds, st, p);
  return (int)hipGetLastError();
}

}  // namespace ea
