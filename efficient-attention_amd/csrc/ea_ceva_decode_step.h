// ea_ceva_decode_step.h -- the three kernels of a causal EVA decoding step that read the step's position: attn, close, append.
// Included once by ea_ceva_decode.hip, inside its anonymous namespace and after the helpers it uses.  The state's switches
// (DEV, RING, SEQ) and the landmark element type L -- float, or E on a compact state, where close rounds its two stores and
// attn reads landmark rows as it reads key and value rows -- are template parameters of the kernels themselves: every
// combination is the kernel written out, nothing wrapped and nothing inlined.  append has no landmark row.
// What attn does to a query group it shares with attn_split (ea_ceva_decode_split.h) and takes from the helpers of
// ea_ceva_decode.hip.

// One workgroup per window block of the step.  DEV: the grid holds the most window blocks T tokens can touch, and a block
// this step does not touch exits at once; a step that does not fit writes NaN rows.  SEQ: the block's queries are those of
// element b's own n tokens, so the wave split below is that of a shared-count step of n tokens at the same position.
// Wave s of the nsplit that share a query group takes tiles s, s + nsplit, ..; a group with a wave to itself is normalised
// and stored by that wave, the others by the group's first wave after the in-LDS merge.  The dynamic step may come without
// pad flags, so every read of them tests the pointer (Pad<true>).
template <typename E, int D, bool DEV, bool RING, bool SEQ, typename L>
__global__ __launch_bounds__(NT) void ceva_attn_kernel(const DecP p) {
  static_assert(DEV || !RING, "the ring belongs to the static step");
  constexpr int G = D / 4;                         // lanes per value row in P.V
  __shared__ __attribute__((aligned(16))) float qs[NW][QPW][D];
  __shared__ __attribute__((aligned(16))) float ps[NW][KT][QPW];
  __shared__ __attribute__((aligned(16))) float mo[NW][QPW][D];
  __shared__ float ml[NW][QPW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)blockIdx.y / p.H, h = (int)blockIdx.y - b * p.H;
  const Step<DEV, SEQ> step(p, b);
  const int t0 = step.t0;
  if (!step.fits(p.T, p.cap)) { refuse_out<E, D>(p, b, h); return; }
  if (SEQ) {
    zero_out<E, D>(p, b, h, step.n(p.T));
    if (step.n(p.T) == 0) return;                  // an element that sits the step out: no query, no block to touch
  }
  const int bk = t0 / p.w + (int)blockIdx.x;
  if (DEV && bk * p.w >= t0 + step.n(p.T)) return;
  const int tq0 = max(t0, bk * p.w), tq1 = min(t0 + step.n(p.T), (bk + 1) * p.w);
  const int nqg = (tq1 - tq0 + QPW - 1) / QPW;
  const int nsplit = nqg >= NW ? 1 : NW / nqg;     // waves per query group
  Group gr(p, Rows<RING>{p.ring}, bk, t0 + step.n(p.T));
  const int dc = (lane % G) * 4;
  for (int g = wave / nsplit; g < nqg; g += NW) {
    gr.qa = tq0 + g * QPW; gr.nql = min(QPW, tq1 - gr.qa);
    stage_queries<E, D>(p, b, h, gr, qs[wave], lane);
    float m[QPW], l[QPW];
    f32x4 acc[QPW];
    stream_tiles<E, D, RING, true, L>(p, b, h, gr, wave % nsplit, nsplit, qs[wave], ps[wave], lane, m, l, acc);
    if (nsplit == 1) {
      if (lane < G) {
#pragma unroll
        for (int i = 0; i < QPW; ++i)
          if (i < gr.nql) Io<E>::st4(const_cast<char*>(row<E>(p.o, b, h, gr.qa + i - t0)) + (size_t)dc * Io<E>::SZ, acc[i] * (1.f / l[i]));
      }
    } else {
      stash_partial<D>(m, l, acc, mo[wave], ml[wave], lane);
    }
  }
  if (nsplit == 1) return;                         // (uniform over the workgroup)
  __syncthreads();
  const int g = wave / nsplit;
  if (wave % nsplit != 0 || g >= nqg) return;
  const int qa = tq0 + g * QPW, nql = min(QPW, tq1 - qa);
  for (int idx = lane; idx < nql * G; idx += 64) {
    const int i = idx / G, c = (idx - i * G) * 4;
    float mx, lt;
    const f32x4 o = merge_waves<D>(mo, ml, wave, nsplit, i, c, mx, lt);
    Io<E>::st4(const_cast<char*>(row<E>(p.o, b, h, qa + i - t0)) + (size_t)c * Io<E>::SZ, o * (1.f / lt));
  }
}


// One workgroup per chunk the step completes: c_first .. c_last of the kernel arguments, or (DEV) the chunks that tokens
// t0 .. t0 + T - 1 complete; then the grid holds ceil(T / r), the most T tokens can complete, and a workgroup whose chunk
// this step does not complete exits at once.  The chunk's rows do not straddle the end of a ring (r divides it); its
// landmark row is row c.  SEQ: the chunks that element b's own tokens complete.
template <typename E, int D, bool DEV, bool RING, bool SEQ, typename L>
__global__ __launch_bounds__(NT) void ceva_close_kernel(const DecP p) {
  static_assert(DEV || !RING, "the ring belongs to the static step");
  __shared__ __attribute__((aligned(16))) float xm[2][D];      // chunk means of q, k
  __shared__ __attribute__((aligned(16))) float y[2][D];       // after the Linear layers
  __shared__ __attribute__((aligned(16))) float mu[D];
  __shared__ float pt[NT];                                      // probabilities of the current row tile
  __shared__ float red[NW];
  const int tid = threadIdx.x;
  const Step<DEV, SEQ> step(p, SEQ ? (int)blockIdx.y / p.H : 0);
  const int c = (DEV ? step.t0 / p.r : p.c_first) + (int)blockIdx.x;
  if (DEV && (!step.fits(p.T, p.cap) || c > (step.t0 + step.n(p.T)) / p.r - 1)) return;
  const int b = (int)blockIdx.y / p.H, h = (int)blockIdx.y - b * p.H;
  const Rows<RING> rows{p.ring};
  const int n0 = rows.slot(c * p.r);                           // first row of the chunk
  const uint8_t* pad = p.pad ? p.pad + (size_t)b * rows.len(p.cap) + n0 : nullptr;
  // masked means over the chunk's rows, divided by the chunk length
  if (tid < 2 * D) {
    const int side = tid / D, o = tid - side * D;
    const DecT& t = side ? p.k : p.q;
    float a = 0.f;
    for (int j = 0; j < p.r; ++j) {
      if (pad && pad[j]) continue;
      a += Io<E>::ld1(row<E>(t, b, h, n0 + j) + (size_t)o * Io<E>::SZ);
    }
    xm[side][o] = a * (1.f / (float)p.r);
  }
  __syncthreads();
  // mu networks: y = W x + b per side, then (adaptive) LayerNorm over the D outputs
  const int per = p.adaptive ? 4 : 2;
  if (tid < 2 * D) {
    const int side = tid / D, o = tid - side * D;
    const float* W = p.mu[side * per] + (size_t)o * D;
    float a = p.mu[side * per + 1][o];
    for (int i = 0; i < D; i += 4) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(W + i);
      a = fmaf(w4[0], xm[side][i], a); a = fmaf(w4[1], xm[side][i + 1], a);
      a = fmaf(w4[2], xm[side][i + 2], a); a = fmaf(w4[3], xm[side][i + 3], a);
    }
    y[side][o] = a;
  }
  __syncthreads();
  float z = 0.f;
  if (tid < 2 * D) {
    const int side = tid / D, o = tid - side * D;
    z = y[side][o];
    if (p.adaptive) {
      float mean = 0.f, var = 0.f;
      for (int i = 0; i < D; ++i) mean += y[side][i];
      mean *= 1.f / (float)D;
      for (int i = 0; i < D; ++i) { const float dv = y[side][i] - mean; var = fmaf(dv, dv, var); }
      var *= 1.f / (float)D;
      z = (z - mean) / sqrtf(var + 1e-5f) * p.mu[side * per + 2][o] + p.mu[side * per + 3][o];
    }
  }
  __syncthreads();
  if (tid >= D && tid < 2 * D) {                   // k side: rf_k_bar = rk
    const int o = tid - D;
    xm[1][o] = z;
    store_lmk<L>(p.lk, b, h, c, o, z);
  }
  __syncthreads();
  if (tid < D) mu[tid] = z + xm[1][tid];           // mu = mu_q(qm) + rk
  __syncthreads();
  // beta = softmax over the chunk rows of (s mu.k_j - s |k_j|^2 / 2), padded rows -5e4 with a zero value row
  float mrun = -INFINITY, lrun = 0.f, acc = 0.f;
  for (int j0 = 0; j0 < p.r; j0 += NT) {
    const int j = j0 + tid;
    float x = -INFINITY;
    if (j < p.r) {
      if (pad && pad[j]) {
        x = MASK_FILL;
      } else {
        const char* rp = row<E>(p.k, b, h, n0 + j);
        float dot = 0.f, nn = 0.f;
        for (int c8 = 0; c8 < D; c8 += 8) {
          float kx[8];
          Io<E>::ld8(rp + (size_t)c8 * Io<E>::SZ, kx);
#pragma unroll
          for (int e = 0; e < 8; ++e) { dot = fmaf(mu[c8 + e], kx[e], dot); nn = fmaf(kx[e], kx[e], nn); }
        }
        x = dot * p.scale - 0.5f * p.scale * nn;
      }
    }
    const float mn = fmaxf(mrun, block_max(x, red));
    pt[tid] = x == -INFINITY ? 0.f : __expf(x - mn);
    __syncthreads();
    if (tid < D) {
      const float alpha = mrun == -INFINITY ? 0.f : __expf(mrun - mn);
      lrun *= alpha;
      acc *= alpha;
      const int nj = min(NT, p.r - j0);
      for (int jj = 0; jj < nj; ++jj) {
        lrun += pt[jj];
        if (pad && pad[j0 + jj]) continue;
        acc = fmaf(pt[jj], Io<E>::ld1(row<E>(p.v, b, h, n0 + j0 + jj) + (size_t)tid * Io<E>::SZ), acc);
      }
    }
    mrun = mn;
    __syncthreads();
  }
  if (tid < D) store_lmk<L>(p.lv, b, h, c, tid, acc / lrun);
}

// one workgroup per (token t, element b) of the step: the token's [3, H, D] row, 16 bytes per lane and load, and its pad flag.
// Each token's row is reduced on its own (a step may straddle the end of a ring); the capacity test stays on p.cap, the
// landmark capacity.  SEQ: every workgroup finds n_b from the flags of its own element (one pass of 16-byte loads, a
// 2048-token prefill is 128 of them), so none waits for another; the one of t = 0 publishes it, and also when the element
// does not fit -- close, attn and advance decide that from pos[b] + ntok[b] as this kernel does.  The tokens it stores are
// unflagged by construction: their pad flag is 0.
template <bool RING, bool SEQ>
__global__ __launch_bounds__(NT) void ceva_append_kernel(const AppP p) {
  const int t = (int)blockIdx.x, b = (int)blockIdx.y;
  int n = p.T;
  if (SEQ) {
    __shared__ int red[NW];
    if (p.src_pad) n = first_flag(p.src_pad + (size_t)b * p.T, p.T, red);
    if (t == 0 && threadIdx.x == 0) p.ntok[b] = n;
  }
  const Step<true, SEQ> step(p.pos, b, n);
  if (!step.fits(p.T, p.cap)) {
    if (t == 0 && (SEQ || b == 0) && threadIdx.x == 0) p.status[SEQ ? b : 0] = 1;
    return;
  }
  if (SEQ && t >= step.n(p.T)) return;
  const u32x4* src = reinterpret_cast<const u32x4*>(p.src + ((size_t)t * p.B + b) * p.row_bytes);
  const Rows<RING> rows{p.ring};
  const size_t at = (size_t)b * rows.len(p.cap) + rows.slot(step.t0, t);
  u32x4* dst = reinterpret_cast<u32x4*>(p.cache + at * p.row_bytes);
  for (int i = threadIdx.x; i < p.row_bytes / 16; i += NT) dst[i] = src[i];
  if (threadIdx.x == 0) p.pad[at] = !SEQ && p.src_pad ? p.src_pad[(size_t)b * p.T + t] : (uint8_t)0;
}
