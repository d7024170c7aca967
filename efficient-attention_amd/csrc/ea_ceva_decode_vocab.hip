// ea_ceva_decode_vocab.hip -- the token passes of a decoding step on a vocabulary table the state holds: the greedy pick
// (ABI 26), the sampled one (ABI 27: ceva_vocab_sample_kernel, behind the same first launch) and the token log-probabilities
// (ABI 28: ceva_vocab_pick_kernel on DecLseP)
//
//   logit[m, v] = sum_k round_w(x[m, k]) w[v, k]            fp32, no bias;  1 <= M <= 64 rows, w [V, K] 16-bit row-major
//   token[m]    = argmax_v logit[m, v]                      the largest value; equal values: the lowest index; a row with NaN
//   top[m]      = logit[m, token[m]]                        logits: the lowest index that holds one (torch.argmax's rule)
//
// The step is bound by reading w once (2 V K bytes: 67 MB at V = 32768, K = 1024).  The first launch of every pass here, the
// table pass, is ceva_rows_kernel (ea_ceva_decode_rows.h) on DecVocabP or DecLseP: the tile loop of the held projections, so
// the logits are those kernels' bits, with one (value, index) candidate per row and 16-column tile -- and on DecLseP one
// sum of exponentials -- as its epilogue.  This file holds the launches behind it, one workgroup per row of x:
// ceva_vocab_pick_kernel reduces the row's ceil(V / 16) candidates under voc_beats' rule and writes token[m] (int64) and
// top[m]; ceva_vocab_sample_kernel draws a token instead.  No atomics across workgroups, no workgroup waits for another: a
// replay repeats the bits.
#include <limits.h>
#include <math.h>
#include <type_traits>
#include "ea_common.h"
#include "ea_ceva_decode_linear.h"
#include "ea_ceva_decode_vocab.h"

namespace ea {
namespace {

#include "ea_ceva_decode_rows.h"

constexpr int PICK_THREADS = 512;

static_assert(sizeof(VocPick) == 8, "a candidate is one 8-byte store");

// The best of a row's NB candidates under voc_beats' rule -> thread 0's return value.  Every thread of the PICK_THREADS
// calls it; best [PICK_THREADS / 64].
EA_DEV VocPick voc_row_best(const VocPick* row, int NB, VocPick* best) {
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
  }
  return c;
}

// S = sum_t s_t exp(m_t - top) over the tiles that hold a number (a finite top: every m_t is finite or -inf, every
// exponent <= 0; a tile of -inf alone is skipped, never multiplied) -> thread 0's return value; `top` is uniform.  Every
// thread of the PICK_THREADS calls it; part [PICK_THREADS / 64].
EA_DEV float voc_row_expsum(const VocPick* row, const float* srow, int NB, float top, float* part) {
  float s = 0.f;
  if (top - top == 0.f) {                                 // (uniform)
    for (int j = threadIdx.x; j < NB; j += PICK_THREADS) {
      const float mt = row[j].v;
      if (mt != -INFINITY) s += srow[j] * expf(mt - top);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return 0.f;
  float total = part[0];
#pragma unroll
  for (int w = 1; w < PICK_THREADS / 64; ++w) total += part[w];
  return total;
}

// top NaN: NaN; +inf: +inf; -inf (every logit is -inf): -inf
EA_DEV float voc_lse_of(float top, float total) { return top - top == 0.f ? top + logf(total) : top; }

// The launch behind the table pass that picks: one workgroup per row reduces the row's candidates.  On DecLseP
// (ABI 28; the table pass has also written s_t = sum_columns exp(logit - m_t) of every tile to lws[m][tile]) it goes on: it
// folds the tile sums into lse[m] = top + log(sum_t s_t exp(m_t - top)) and writes logp[m] = (the token's, the target's or
// the top logit) - lse[m]: the log-probability under the model's own distribution at temperature 1, nothing truncated.
template <typename P>
__global__ __launch_bounds__(PICK_THREADS) void ceva_vocab_pick_kernel(const P p) {
  constexpr bool LSE = std::is_same<P, DecLseP>::value;
  static_assert(LSE || std::is_same<P, DecVocabP>::value, "one of the two blocks that pick");
  __shared__ VocPick best[PICK_THREADS / 64];
  __shared__ float part[PICK_THREADS / 64];
  __shared__ float top_of_row;
  const int m = blockIdx.x;
  const int NB = (p.V - 1) / VOC_TILE + 1;
  const VocPick* row = p.ws + (int64_t)m * NB;
  // pass 1: the pick
  const VocPick c = voc_row_best(row, NB, best);
  if (threadIdx.x == 0) {
    if constexpr (LSE) {
      if (!p.token_in) {                                  // (the sampled mode: the token was drawn before this launch)
        p.token[m] = (int64_t)c.i;
        if (p.top) p.top[m] = c.v;
      }
      top_of_row = c.v;
    } else {
      p.token[m] = (int64_t)c.i;
      if (p.top) p.top[m] = c.v;
    }
  }
  if constexpr (LSE) {
    __syncthreads();
    const float top = top_of_row;
    // pass 2: the tile sums against the top
    const float total = voc_row_expsum(row, p.lws + (int64_t)m * NB, NB, top, part);
    if (threadIdx.x != 0) return;
    const float lse = voc_lse_of(top, total);
    float tl = top;
    if (p.token_in) {
      const int64_t t = p.token_in[m];
      tl = t >= 0 && t < (int64_t)p.V ? reinterpret_cast<const float*>(p.logits)[(int64_t)m * p.ldl + t] : NAN;
    } else if (p.targets) {
      const int64_t t = p.targets[m];
      tl = t >= 0 && t < (int64_t)p.V ? p.tlogit[m] : NAN;   // (no thread of the first launch has written tlogit[m] otherwise)
    }
    p.lse[m] = lse;
    p.logp[m] = tl - lse;
  }
}

// ---- the sampled pick (ABI 27) ----------------------------------------------------------------------------------------------
// the selection and the draw: ea_voc_select.h
#include "ea_voc_select.h"

__global__ __launch_bounds__(SMP_THREADS) void ceva_vocab_sample_kernel(const DecSampleP p) {
  __shared__ VocSelect sh;
  const int m = blockIdx.x, lane = threadIdx.x & 63;
  const int NB = (p.V - 1) / VOC_TILE + 1;
  const float* lrow = p.logits + (int64_t)m * p.ldl;
  const int kk = voc_select(p.ws + (int64_t)m * NB, lrow, p.V, NB, p.top_k, sh);
  const uint64_t* sorted = sh.sorted;
  if (threadIdx.x >= 64) return;
  // 3 .. 6: one wave, entry j of the selection in lane j
  const bool live = lane < kk;
  const int32_t idx = live ? min(max(voc_key_index(sorted[lane]), 0), p.V - 1) : 0;   // (a column of the row, come what may)
  const float val = live ? lrow[idx] : -INFINITY;        // (the stored logit's own bits: the key has folded -0 and NaNs)
  if (live && p.sel_idx) p.sel_idx[(int64_t)m * p.top_k + lane] = idx;
  if (live && p.sel_val) p.sel_val[(int64_t)m * p.top_k + lane] = val;
  const int64_t n = p.ctr[m];
  int32_t kept;
  const int drawn = voc_draw(val, live, kk, p.top_p, p.temperature, p.seed_lo, p.seed_hi, n, p.sid[m], kept);
  const int32_t token = __shfl(idx, drawn);
  if (lane == 0) {
    p.token[m] = (int64_t)token;
    if (p.kept) p.kept[m] = kept;
    p.ctr[m] = n + 1;                                     // (this workgroup alone reads and writes ctr[m])
  }
}

// ---- the beam step (ABI 32) --------------------------------------------------------------------------------------------------
// Two launches behind the table pass on DecLseP (fp32 logits, one candidate and one sum of exponentials per tile); the rule
// is spelled out in include/ea_hip.h.  Row m = s W + b is beam b of sentence s.
#include "ea_voc_ban.h"
static_assert(PICK_THREADS == SMP_THREADS, "the beam step's row kernel runs the pick's and the sampler's helpers in one workgroup");
constexpr int BEAM_MAX_W = 32;                            // 2 W <= VOC_SAMPLE_MAX_K: a row's candidates are one selection
constexpr int BEAM_POOL = BEAM_MAX_W * VOC_SAMPLE_MAX_K;  // candidates of one sentence
static_assert(BEAM_POOL <= SMP_UNROLL * SMP_THREADS, "voc_threshold and voc_compact walk a sentence in one iteration");

// One workgroup per row (rule A): lse[m] by ceva_vocab_pick_kernel<DecLseP>'s operations, the k' = min(2 W, V) best logits
// by the sampler's steps 1-2 (the forced step: eos alone), and every candidate's score = score[m] + (value - lse[m]): two fp32
// operations, no product anywhere near them.  The rows of a done sentence are skipped.
// BANS (ABI 36): the row's ban list is applied behind lse and ahead of the selection (ea_voc_ban.h); the forced step's list
// is empty.  The body of both kernels, inlined: the unconstrained one keeps its instructions.
template <bool BANS>
EA_DEV void beam_rows_body(const DecBeamP& p, const BanListP& c_list, VocSelect& sh, VocPick* best, float* part,
                           float& top_of_row, float& lse_of_row) {
  const int m = blockIdx.x, s = m / p.W, lane = threadIdx.x & 63;
  if (p.done[s]) return;                                  // (uniform)
  const bool forced = p.t[s] + 1 >= p.max_new;
  const int NB = (p.V - 1) / VOC_TILE + 1;
  const VocPick* cand = p.ws + (int64_t)m * NB;
  const float* lrow = p.logits + (int64_t)m * p.ldl;
  const VocPick c = voc_row_best(cand, NB, best);
  if (threadIdx.x == 0) top_of_row = c.v;
  __syncthreads();
  const float total = voc_row_expsum(cand, p.lws + (int64_t)m * NB, NB, top_of_row, part);
  if (threadIdx.x == 0) {
    lse_of_row = voc_lse_of(top_of_row, total);
    p.lse[m] = lse_of_row;
  }
  __syncthreads();
  const float lse = lse_of_row, score = p.score[m];
  const int64_t at = (int64_t)m * (2 * p.W);
  if (forced) {
    if (threadIdx.x == 0) {
      const float val = lrow[p.eos];
      p.cand_idx[at] = p.eos;
      p.cand_score[at] = score + (val - lse);
      if (p.sel_val) p.sel_val[at] = val;
    }
    return;
  }
  if constexpr (BANS) {                                   // (this workgroup alone reads and writes the row from here on)
    const int nb = min(max(c_list.nban[m], 0), c_list.cap);
    voc_apply_bans(const_cast<float*>(lrow), const_cast<VocPick*>(cand), p.V, c_list.ban + (int64_t)m * c_list.cap, nb, 0);
  }
  const int kk = voc_select(cand, lrow, p.V, NB, 2 * p.W, sh);
  if (threadIdx.x >= 64 || lane >= kk) return;
  const int32_t idx = min(max(voc_key_index(sh.sorted[lane]), 0), p.V - 1);   // (a column of the row, come what may)
  const float val = lrow[idx];                            // (the stored logit's own bits: the key has folded -0 and NaNs)
  p.cand_idx[at + lane] = idx;
  p.cand_score[at + lane] = score + (val - lse);
  if (p.sel_val) p.sel_val[at + lane] = val;
}

__global__ __launch_bounds__(SMP_THREADS) void ceva_vocab_beam_rows_kernel(const DecBeamP p) {
  __shared__ VocSelect sh;
  __shared__ VocPick best[PICK_THREADS / 64];
  __shared__ float part[PICK_THREADS / 64];
  __shared__ float top_of_row, lse_of_row;
  beam_rows_body<false>(p, BanListP{}, sh, best, part, top_of_row, lse_of_row);
}

__global__ __launch_bounds__(SMP_THREADS) void ceva_vocab_beam_rows_c_kernel(const DecBeamP p, const BanListP c) {
  __shared__ VocSelect sh;
  __shared__ VocPick best[PICK_THREADS / 64];
  __shared__ float part[PICK_THREADS / 64];
  __shared__ float top_of_row, lse_of_row;
  beam_rows_body<true>(p, c, sh, best, part, top_of_row, lse_of_row);
}

// ---- the ban-list launch (ABI 36) ------------------------------------------------------------------------------------------
// One wave per row of a sentence that is not done; the rule is spelled out in include/ea_hip.h.  The row's tokens
// x = prompt ++ generated are read where they lie: the prompt, the parent's row of buffer (t - 1) & 1 and the token the
// previous merge wrote -- while the same lanes copy that row, with the token appended, into the row's own place in buffer
// t & 1.  The list: the static bans, eos while t < min_len, then window i of x in lane i % 64, 64 at a time: a window that
// equals the suffix lists the token behind it, at the slot a ballot counts out, so the list's order is fixed too.  The
// forced step lists nothing.  A workgroup writes its own row alone; ordinary vector stores.
constexpr int BAN_THREADS = 64;

__global__ __launch_bounds__(BAN_THREADS) void beam_bans_kernel(const BeamBanP p) {
  const int m = blockIdx.x, s = m / p.W, lane = threadIdx.x;
  if (p.done[s]) return;                                  // (uniform)
  const int M = p.S * p.W;
  const int t = min(max(p.t[s], 0), p.max_new - 1);       // (otherwise only in a state no step of the merge leaves)
  const int plen = p.prompt_cap > 0 ? min(max(p.prompt_len[s], 0), p.prompt_cap) : 0;
  const int32_t* prompt = p.prompt_tok + (int64_t)s * p.prompt_cap;
  int32_t* dst = p.gen + ((int64_t)(t & 1) * M + m) * p.max_new;
  const int32_t* src = dst;
  int32_t last = 0;
  if (t >= 1) {
    const int par = min(max(p.hist_par[(int64_t)(t - 1) * M + m], 0), p.W - 1);
    src = p.gen + ((int64_t)((t - 1) & 1) * M + s * p.W + par) * p.max_new;
    last = p.hist_tok[(int64_t)(t - 1) * M + m];
    for (int j = lane; j < t - 1; j += BAN_THREADS) dst[j] = src[j];
    if (lane == 0) dst[t - 1] = last;
  }
  const int L = plen + t;
  auto x = [&](int i) { return i < plen ? prompt[i] : (i - plen < t - 1 ? src[i - plen] : last); };   // i < L
  int32_t* ban = p.ban + (int64_t)m * p.cap;
  int n = 0;                                              // (uniform)
  if (t + 1 < p.max_new) {
#pragma unroll
    for (int j = 0; j < BAN_MAX_STATIC; ++j)
      if (lane == j && j < p.n_static) ban[j] = p.static_tok[j];
    n = min(p.n_static, BAN_MAX_STATIC);
    if (t < p.min_len) {
      if (lane == 0) ban[n] = p.eos;
      ++n;
    }
    const int ng = p.ngram;
    if (ng >= 1) {
      const int suffix = L - ng + 1;                      // x[suffix .. L): the ng - 1 tokens a new one would follow
      const uint64_t below = (1ull << lane) - 1ull;
      for (int i0 = 0; i0 + ng <= L; i0 += BAN_THREADS) {  // windows i = 0 .. L - ng
        const int i = i0 + lane;
        bool hit = i + ng <= L;
        for (int j = 0; j < ng - 1 && hit; ++j) hit = x(i + j) == x(suffix + j);
        const uint64_t hits = __ballot(hit);
        const int at = n + __popcll(hits & below);
        if (hit && at < p.cap) ban[at] = x(i + ng - 1);
        n += __popcll(hits);
      }
    }
  }
  if (lane == 0) p.nban[m] = min(n, p.cap);
}

// One workgroup per sentence (rules B and C): the sentence's W k' candidates (k' = kc; the forced step: 1) as keys -- the
// score's image in the high word, the complement of the flat index f = b k' + j in the low one -- the n2 = min(2 W, W k')
// largest in order, then one wave walks them, candidate i in lane i.  Only this workgroup touches t[s], nfin[s], done[s],
// the sentence's records and its W rows of token, parent, score and the history.
__global__ __launch_bounds__(SMP_THREADS) void ceva_vocab_beam_merge_kernel(const DecBeamP p) {
  __shared__ uint64_t keys[BEAM_POOL];
  __shared__ uint64_t sel[VOC_SAMPLE_MAX_K];
  __shared__ uint64_t sorted[VOC_SAMPLE_MAX_K];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t pass[3];
  __shared__ uint32_t count;
  const int s = blockIdx.x, W = p.W, lane = threadIdx.x & 63;
  const int M = p.S * W, row0 = s * W;
  if (p.done[s]) {                                        // (uniform) rule C
    if ((int)threadIdx.x < W) {
      p.token[row0 + threadIdx.x] = (int64_t)p.eos;
      p.parent[row0 + threadIdx.x] = (int64_t)(row0 + threadIdx.x);
    }
    return;
  }
  const int t = p.t[s], nfin = p.nfin[s];
  const bool forced = t + 1 >= p.max_new;
  const int kc = forced ? 1 : p.kc;
  const int n = W * kc, n2 = min(2 * W, n);
  const int32_t* cidx = p.cand_idx + (int64_t)row0 * (2 * W);
  const float* cscore = p.cand_score + (int64_t)row0 * (2 * W);
  if (threadIdx.x == 0) count = 0u;
  for (int f = threadIdx.x; f < n; f += SMP_THREADS) keys[f] = voc_key(cscore[(f / kc) * (2 * W) + f % kc], f);
  __syncthreads();
  auto key_of = [&](int f) { return keys[f]; };
  const uint64_t t1 = n2 < n ? voc_threshold(key_of, n, n2, hist, pass) : 0ull;
  __syncthreads();
  voc_compact(key_of, n, t1, sel, n2, &count);
  __syncthreads();
  voc_rank_sort(sel, sorted, n2);
  if (threadIdx.x >= 64) return;
  // candidate i of the walk in lane i
  const bool live = lane < n2;
  const int f = live ? min(max(voc_key_index(sorted[lane]), 0), n - 1) : 0;
  const int b = f / kc;
  const int32_t tok = live ? cidx[b * (2 * W) + f % kc] : 0;
  const float sc = live ? cscore[b * (2 * W) + f % kc] : 0.f;   // (the stored score's own bits)
  const uint64_t below = (1ull << lane) - 1ull;
  const bool is_eos = live && tok == p.eos;
  // finished hypotheses: an eos among the first W whose score is not -inf, while a slot is free
  const bool ends = is_eos && lane < W && sc != -INFINITY;
  const uint64_t ending = __ballot(ends);
  const int slot = nfin + __popcll(ending & below);
  if (ends && slot < W) {
    p.fin_score[row0 + slot] = sc;
    p.fin_len[row0 + slot] = t + 1;
    p.fin_beam[row0 + slot] = b;
  }
  const int nfin_new = min(W, nfin + __popcll(ending));
  // the next step's beams: the first W candidates that go on; the rest of the W are dead
  const bool goes = live && !is_eos;
  const uint64_t going = __ballot(goes);
  const int r = __popcll(going & below), ngo = min(W, __popcll(going));
  const bool hist_ok = t >= 0 && t < p.max_new;          // (otherwise only in a state no step of this kernel leaves)
  if (goes && r < W) {
    p.token[row0 + r] = (int64_t)tok;
    p.parent[row0 + r] = (int64_t)(row0 + b);
    p.score[row0 + r] = sc;
    if (hist_ok) {
      p.hist_tok[(int64_t)t * M + row0 + r] = tok;
      p.hist_par[(int64_t)t * M + row0 + r] = b;
    }
  }
  if (lane >= ngo && lane < W) {
    p.token[row0 + lane] = (int64_t)p.eos;
    p.parent[row0 + lane] = (int64_t)(row0 + lane);
    p.score[row0 + lane] = -INFINITY;
    if (hist_ok) {
      p.hist_tok[(int64_t)t * M + row0 + lane] = p.eos;
      p.hist_par[(int64_t)t * M + row0 + lane] = lane;
    }
  }
  if (lane == 0) {
    p.t[s] = t + 1;
    p.nfin[s] = nfin_new;
    p.done[s] = nfin_new == W || forced;
  }
}

// the table pass on p: its refusals, the sampler's bound on top_k (0: no sampler behind it), the launch
// (The C entry point has checked pointers, strides, alignment and the sizes of ws and lws.)
template <typename P>
int voc_table_pass(const P& p, int top_k, hipStream_t st) {
  if (!p.x || !p.w || !p.ws || p.M < 1 || p.ldx < p.K || (p.logits && p.ldl < p.V)) return EA_E_BADARG;
  if constexpr (std::is_same<P, DecLseP>::value) {
    if (!p.lws || !p.tlogit || !p.lse || !p.logp) return EA_E_BADARG;
  }
  if (p.M > EA_CEVA_LINEAR_MAX_ROWS || p.K <= 0 || p.K % 32 || p.V < 1) return EA_E_UNSUPPORTED;
  const RowsKernel<P> kernel = rows_kernel_of(p);
  if (!kernel) return EA_E_BADARG;
  if (top_k > VOC_SAMPLE_MAX_K) return EA_E_UNSUPPORTED;
  return rows_launch(kernel, p, p.V, st);
}

// a launch behind the table pass: one workgroup per row
template <typename P>
int voc_row_pass(void (*kernel)(const P), int threads, const P& p, int M, hipStream_t st) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)M), dim3(threads), 0, st, p);
  return (int)hipGetLastError();
}

// s reads what the table pass on p writes (fp32 logits, required), and its own arguments are in range
template <typename P>
bool voc_sampler_ok(const P& p, const DecSampleP& s) {
  if (!s.token || !s.ctr || !s.sid || !p.logits || !p.l_f32 || (const char*)s.logits != p.logits || s.ldl != p.ldl ||
      s.ws != p.ws || s.V != p.V) return false;
  return s.top_k >= 1 && s.top_p > 0.f && s.top_p <= 1.f && s.temperature > 0.f && s.temperature - s.temperature == 0.f;
}

}  // namespace

int64_t ceva_sdecode_vocab_ws(int M, int V) {
  if (M < 1 || M > EA_CEVA_LINEAR_MAX_ROWS || V < 1) return -1;
  return (int64_t)M * ((V - 1) / VOC_TILE + 1) * (int64_t)sizeof(VocPick);
}

int64_t ceva_sdecode_vocab_lse_ws(int M, int V) {
  if (M < 1 || M > EA_CEVA_LINEAR_MAX_ROWS || V < 1) return -1;
  return (int64_t)M * ((V - 1) / VOC_TILE + 1) * (int64_t)sizeof(float) + (int64_t)M * (int64_t)sizeof(float);
}

int ceva_sdecode_vocab_argmax(const DecVocabP& p, hipStream_t st) {
  if (!p.token) return EA_E_BADARG;
  const int rc = voc_table_pass(p, 0, st);
  return rc != 0 ? rc : voc_row_pass(ceva_vocab_pick_kernel<DecVocabP>, PICK_THREADS, p, p.M, st);
}

int ceva_sdecode_vocab_sample(const DecVocabP& p, const DecSampleP& s, hipStream_t st) {
  if (!voc_sampler_ok(p, s)) return EA_E_BADARG;
  const int rc = voc_table_pass(p, s.top_k, st);
  return rc != 0 ? rc : voc_row_pass(ceva_vocab_sample_kernel, SMP_THREADS, s, p.M, st);
}

int ceva_sdecode_vocab_logprob(const DecLseP& p, hipStream_t st) {
  if (!p.token || p.token_in) return EA_E_BADARG;
  const int rc = voc_table_pass(p, 0, st);
  return rc != 0 ? rc : voc_row_pass(ceva_vocab_pick_kernel<DecLseP>, PICK_THREADS, p, p.M, st);
}

int ceva_sdecode_vocab_table_pass(const DecLseP& p, hipStream_t st) {
  if (p.token_in) return EA_E_BADARG;
  return voc_table_pass(p, 0, st);
}

int ceva_sdecode_vocab_sample_logprob(const DecLseP& p, const DecSampleP& s, hipStream_t st) {
  if (!voc_sampler_ok(p, s) || p.token_in != s.token || p.targets) return EA_E_BADARG;
  int rc = voc_table_pass(p, s.top_k, st);
  if (rc == 0) rc = voc_row_pass(ceva_vocab_sample_kernel, SMP_THREADS, s, p.M, st);
  return rc != 0 ? rc : voc_row_pass(ceva_vocab_pick_kernel<DecLseP>, PICK_THREADS, p, p.M, st);
}

// ---- the beam step (ABI 32) ----
static int64_t beam_round16(int64_t n) { return (n + 15) & ~(int64_t)15; }

static bool beam_envelope(int M, int W) { return W >= 1 && W <= BEAM_MAX_W && M >= 1 && M <= EA_CEVA_LINEAR_MAX_ROWS && M % W == 0; }

int64_t ceva_sdecode_vocab_beam_ws(int M, int V, int W) {
  if (V < 1 || !beam_envelope(M, W)) return -1;
  return beam_round16(ceva_sdecode_vocab_ws(M, V)) + beam_round16(ceva_sdecode_vocab_lse_ws(M, V)) +
         2 * beam_round16((int64_t)M * 2 * W * 4) + beam_round16((int64_t)M * 4);
}

void ceva_sdecode_vocab_beam_carve(void* ws, DecLseP* p, DecBeamP* b) {
  const int M = p->M, V = p->V, NB = (V - 1) / VOC_TILE + 1;
  char* at = (char*)ws;
  p->ws = (VocPick*)at; at += beam_round16(ceva_sdecode_vocab_ws(M, V));
  p->lws = (float*)at; p->tlogit = p->lws + (int64_t)M * NB; at += beam_round16(ceva_sdecode_vocab_lse_ws(M, V));
  int32_t* idx = (int32_t*)at; at += beam_round16((int64_t)M * 2 * b->W * 4);
  float* score = (float*)at; at += beam_round16((int64_t)M * 2 * b->W * 4);
  float* lse = (float*)at;
  if (!b->cand_idx) b->cand_idx = idx;
  if (!b->cand_score) b->cand_score = score;
  if (!b->lse) b->lse = lse;
  p->lse = p->logp = lse;                                 // (required by the block; the table pass writes neither)
  b->ws = p->ws; b->lws = p->lws;
}

static bool beam_state_ok(const DecBeamP& b) {
  return b.cand_idx && b.cand_score && b.score && b.t && b.nfin && b.done && b.token && b.parent && b.hist_tok && b.hist_par &&
         b.fin_score && b.fin_len && b.fin_beam && b.eos >= 0 && b.max_new >= 1 && b.kc >= 1 && b.kc <= 2 * b.W;
}

int ceva_beam_merge(const DecBeamP& b, hipStream_t st) {
  if (b.S < 1 || b.W < 1 || !beam_state_ok(b)) return EA_E_BADARG;
  if (!beam_envelope(b.S * b.W, b.W)) return EA_E_UNSUPPORTED;
  return voc_row_pass(ceva_vocab_beam_merge_kernel, SMP_THREADS, b, b.S, st);
}

int ceva_sdecode_vocab_beam(const DecLseP& p, const DecBeamP& b, hipStream_t st) {
  if (b.W < 1 || !beam_state_ok(b) || !p.logits || !p.l_f32 || (const char*)b.logits != p.logits || b.ldl != p.ldl ||
      b.ws != p.ws || b.lws != p.lws || !b.lse || b.V != p.V || b.eos >= p.V || p.targets || p.token_in) return EA_E_BADARG;
  if (!beam_envelope(p.M, b.W) || b.S * b.W != p.M || b.kc != (2 * b.W < p.V ? 2 * b.W : p.V)) return EA_E_UNSUPPORTED;
  int rc = voc_table_pass(p, 0, st);
  if (rc == 0) rc = voc_row_pass(ceva_vocab_beam_rows_kernel, SMP_THREADS, b, p.M, st);
  return rc != 0 ? rc : voc_row_pass(ceva_vocab_beam_merge_kernel, SMP_THREADS, b, b.S, st);
}

// ---- the constrained beam step (ABI 36) ----
int64_t ceva_beam_bans_ws(int M, int prompt_cap, int max_new) {
  if (M < 1 || M > EA_CEVA_LINEAR_MAX_ROWS || prompt_cap < 0 || max_new < 1) return -1;
  const int64_t cap = beam_ban_cap(prompt_cap, max_new);
  if (cap > INT_MAX) return -1;
  return beam_round16((int64_t)M * cap * 4) + beam_round16((int64_t)M * 4);
}

void ceva_beam_bans_carve(void* ws, int M, BeamBanP* b) {
  b->cap = (int)beam_ban_cap(b->prompt_cap, b->max_new);
  b->ban = (int32_t*)ws;
  b->nban = (int32_t*)((char*)ws + beam_round16((int64_t)M * b->cap * 4));
}

static bool beam_bans_ok(const BeamBanP& c) {
  if (!c.t || !c.done || !c.hist_tok || !c.hist_par || !c.gen || !c.ban || !c.nban || c.S < 1 || c.W < 1 || c.eos < 0 ||
      c.max_new < 1 || c.prompt_cap < 0 || (c.prompt_cap > 0 && (!c.prompt_tok || !c.prompt_len))) return false;
  if (c.min_len < 0 || c.min_len > c.max_new - 1 || c.ngram < 0 || c.ngram > BAN_MAX_NGRAM || c.n_static < 0 ||
      c.n_static > BAN_MAX_STATIC || (int64_t)c.cap < beam_ban_cap(c.prompt_cap, c.max_new)) return false;
  for (int j = 0; j < c.n_static; ++j)
    if (c.static_tok[j] < 0 || c.static_tok[j] == c.eos) return false;
  return true;
}

int ceva_beam_bans(const BeamBanP& c, hipStream_t st) {
  if (!beam_bans_ok(c)) return EA_E_BADARG;
  if (!beam_envelope(c.S * c.W, c.W)) return EA_E_UNSUPPORTED;
  return voc_row_pass(beam_bans_kernel, BAN_THREADS, c, c.S * c.W, st);
}

int ceva_sdecode_vocab_beam_c(const DecLseP& p, const DecBeamP& b, const BeamBanP& c, hipStream_t st) {
  if (b.W < 1 || !beam_state_ok(b) || !p.logits || !p.l_f32 || (const char*)b.logits != p.logits || b.ldl != p.ldl ||
      b.ws != p.ws || b.lws != p.lws || !b.lse || b.V != p.V || b.eos >= p.V || p.targets || p.token_in) return EA_E_BADARG;
  if (!beam_bans_ok(c) || c.S != b.S || c.W != b.W || c.eos != b.eos || c.max_new != b.max_new || c.t != b.t ||
      c.done != b.done || c.hist_tok != b.hist_tok || c.hist_par != b.hist_par) return EA_E_BADARG;
  for (int j = 0; j < c.n_static; ++j)
    if (c.static_tok[j] >= p.V) return EA_E_BADARG;
  if (!beam_envelope(p.M, b.W) || b.S * b.W != p.M || b.kc != (2 * b.W < p.V ? 2 * b.W : p.V)) return EA_E_UNSUPPORTED;
  int rc = voc_table_pass(p, 0, st);
  if (rc == 0) rc = voc_row_pass(beam_bans_kernel, BAN_THREADS, c, p.M, st);
  if (rc == 0) {
    const BanListP list = {c.ban, c.nban, c.cap};
    hipLaunchKernelGGL(ceva_vocab_beam_rows_c_kernel, dim3((unsigned)p.M), dim3(SMP_THREADS), 0, st, b, list);
    rc = (int)hipGetLastError();
  }
  return rc != 0 ? rc : voc_row_pass(ceva_vocab_beam_merge_kernel, SMP_THREADS, b, b.S, st);
}

}  // namespace ea
