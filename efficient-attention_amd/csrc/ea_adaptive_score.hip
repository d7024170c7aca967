// ea_adaptive_score.hip -- teacher-forced log-probabilities under an adaptive softmax (ABI 33), for thousands of rows, without a
// [rows, V] or [rows, c0 + n] tensor
//
//   cutoffs c0 < c1 < .. < c_n = V; the head holds the c0 frequent tokens and one class column per tail, tail i the tokens
//   [c_i, c_{i+1}) at width d_i:
//     head target  t < c0:  log p = head_logit[t] - lse_head
//     tail i:               log p = (head_logit[c0 + i] - lse_head) + (tail_logit_i[t - c_i] - lse_tail_i),
//                           tail_logit_i = round16(x proj_i^T) table_i^T, for the rows whose target lies in tail i ONLY
//
// adaptive_route_kernel: one workgroup walks the M targets in strides of 256 with a running offset per band: a row's place in
// its band's list is the offset, plus the rows of that band in the waves before its own, plus those in the lanes before it
// (a ballot).  A stable compaction: rows[i] ascends.  Deterministic; one launch; entries at or beyond count[i] are not written.
// The passes are the tile loop of ea_vocab_score_tile.h with ROWS = true: see there for the clamp that keeps a stale list
// entry from being dereferenced.
// adaptive_combine_kernel: section 0, thread m: a row whose target is in the head (or outside [0, V): NaN from the head
// pass) takes logp_head[m]; section 1 + i, thread j < count[i]: row rows[i][j] takes logp_head[row] + logp_tail_i[j].  Every
// row is written by exactly one thread.
// Ordinary vector stores only; no atomics; no workgroup waits for another; launches only.
#include "ea_vocab_score_tile.h"
#include "ea_adaptive_score.h"

namespace ea {
namespace {

constexpr int AR_THREADS = 256;
constexpr int AR_WAVES = AR_THREADS / 64;
constexpr int AC_THREADS = 256;

__global__ __launch_bounds__(AR_THREADS) void adaptive_route_kernel(const AdaptiveRouteP p) {
  __shared__ int wtot[2][AS_MAX_TAILS][AR_WAVES];      // two buffers in turn: one barrier per stride
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c0 = p.cut[0], V = p.cut[p.n];
  int base[AS_MAX_TAILS];
#pragma unroll
  for (int i = 0; i < AS_MAX_TAILS; ++i) base[i] = 0;
  int buf = 0;
  for (int m0 = 0; m0 < p.M; m0 += AR_THREADS, buf ^= 1) {
    const int m = m0 + tid;
    int band = -1;
    if (m < p.M) {
      const int64_t t = p.targets[m];
      int64_t ht = -1;
      if (t >= 0 && t < V) {
        ht = t;
        if (t >= c0) {
#pragma unroll
          for (int i = 0; i < AS_MAX_TAILS; ++i)
            if (i < p.n && t >= p.cut[i] && t < p.cut[i + 1]) band = i;
          ht = c0 + band;
        }
      }
      p.head_target[m] = ht;
    }
    int rank[AS_MAX_TAILS];
#pragma unroll
    for (int i = 0; i < AS_MAX_TAILS; ++i) {
      const uint64_t in = __ballot(band == i);
      rank[i] = __popcll(in & (((uint64_t)1 << lane) - 1));
      if (lane == 0) wtot[buf][i][wave] = __popcll(in);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < AS_MAX_TAILS; ++i) {
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < AR_WAVES; ++w) {
        const int c = wtot[buf][i][w];
        before += w < wave ? c : 0;
        all += c;
      }
      if (band == i) p.rows[(int64_t)i * p.M + base[i] + before + rank[i]] = m;   // (band < n; the place is < M)
      base[i] += all;
    }
  }
#pragma unroll
  for (int i = 0; i < AS_MAX_TAILS; ++i)
    if (tid == i && i < p.n) p.count[i] = base[i];
}

struct AdaptiveCombineP {
  const int64_t* head_target;
  const int32_t* rows;
  const int32_t* count;
  const float* logp_head;
  const float* logp_tail[AS_MAX_TAILS];
  float* logp;
  int64_t c0;
  int M;
};

__global__ __launch_bounds__(AC_THREADS) void adaptive_combine_kernel(const AdaptiveCombineP p) {
  const int j = blockIdx.x * AC_THREADS + threadIdx.x;
  const int sec = blockIdx.y;
  if (j >= p.M) return;
  if (sec == 0) {
    if (p.head_target[j] < p.c0) p.logp[j] = p.logp_head[j];
    return;
  }
  const int i = sec - 1;
  if (j >= p.count[i]) return;
  const int m = p.rows[(int64_t)i * p.M + j];
  const float* tail = p.logp_tail[0];
#pragma unroll
  for (int k = 1; k < AS_MAX_TAILS; ++k) tail = i == k ? p.logp_tail[k] : tail;
  p.logp[m] = p.logp_head[m] + tail[j];
}

int64_t r16(int64_t n) { return (n + 15) / 16 * 16; }

}  // namespace

int adaptive_route(const AdaptiveRouteP& p, hipStream_t st) {
  hipLaunchKernelGGL(adaptive_route_kernel, dim3(1), dim3(AR_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

// (Every argument has been checked by the callers, ea_vocab_score_rows in ea_capi.hip and adaptive_score below.)
int vocab_score_rows(VocabScoreRowsP p, hipStream_t st) {
  p.MT = (p.M - 1) / VS_BM + 1;
  p.NS = (p.V - 1) / VS_SL + 1;
  p.sum = reinterpret_cast<float*>(p.pick + (int64_t)p.M * p.NS);
  p.tlogit = p.sum + (int64_t)p.M * p.NS;
  if (const int rc = vs_launch_typed<true>(p, st)) return rc;
  return p.logits_only ? 0 : vs_launch_fold<true>(p, st);
}

int64_t adaptive_plan(int M, int n, const int64_t* cut, const int32_t* dims, AdaptivePlan* plan) {
  if (M < 1 || n < 1 || n > AS_MAX_TAILS || !cut || !dims || cut[0] < 1) return -1;
  for (int i = 0; i < n; ++i)
    if (cut[i + 1] <= cut[i] || dims[i] < 1) return -1;
  if (cut[n] > INT_MAX || cut[0] + n > INT_MAX) return -1;
  AdaptivePlan pl = {};
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t here = at; at += r16(bytes); return here; };
  pl.head_target = take(8 * (int64_t)M);
  pl.rows = take(4 * (int64_t)n * M);
  pl.count = take(4 * AS_MAX_TAILS);
  pl.token_head = take(8 * (int64_t)M);
  pl.lse_head = take(4 * (int64_t)M);
  pl.logp_head = take(4 * (int64_t)M);
  int64_t inner = vocab_score_ws(M, (int)(cut[0] + n));
  if (inner < 0) return -1;
  for (int i = 0; i < n; ++i) {
    pl.h[i] = take(2 * (int64_t)M * dims[i]);
    pl.token[i] = take(8 * (int64_t)M);
    pl.lse[i] = take(4 * (int64_t)M);
    pl.logp[i] = take(4 * (int64_t)M);
    const int64_t a = vocab_score_ws(M, dims[i]), b = vocab_score_ws(M, (int)(cut[i + 1] - cut[i]));
    if (a < 0 || b < 0) return -1;
    inner = a > inner ? a : inner;
    inner = b > inner ? b : inner;
  }
  pl.inner = at;
  pl.inner_bytes = inner;
  pl.total = at + inner;
  if (plan) *plan = pl;
  return pl.total;
}

int adaptive_score(const AdaptiveScoreP& a, hipStream_t st) {
  AdaptivePlan pl;
  if (adaptive_plan(a.M, a.n, a.cut, a.dims, &pl) < 0) return EA_E_UNSUPPORTED;
  int64_t* head_target = reinterpret_cast<int64_t*>(a.ws + pl.head_target);
  int32_t* rows = reinterpret_cast<int32_t*>(a.ws + pl.rows);
  int32_t* count = reinterpret_cast<int32_t*>(a.ws + pl.count);
  float* logp_head = reinterpret_cast<float*>(a.ws + pl.logp_head);

  AdaptiveRouteP r = {};
  r.targets = a.targets; r.head_target = head_target; r.rows = rows; r.count = count; r.M = a.M; r.n = a.n;
  for (int i = 0; i <= a.n; ++i) r.cut[i] = a.cut[i];
  if (const int rc = adaptive_route(r, st)) return rc;

  // the head: every row, its head target
  VocabScoreRowsP h = {};
  h.x = a.x; h.w = a.head; h.targets = head_target; h.pick = reinterpret_cast<VsPick*>(a.ws + pl.inner);
  h.token = a.token_head ? a.token_head : reinterpret_cast<int64_t*>(a.ws + pl.token_head);
  h.lse = reinterpret_cast<float*>(a.ws + pl.lse_head); h.logp = logp_head;
  h.ldx = a.ldx; h.M = a.M; h.K = a.C; h.V = (int)(a.cut[0] + a.n); h.dtype = a.dtype; h.x_f32 = a.x_f32;
  if (const int rc = vocab_score_rows(h, st)) return rc;

  AdaptiveCombineP c = {};
  for (int i = 0; i < a.n; ++i) {
    const int32_t* list = rows + (int64_t)i * a.M;
    char* hi = a.ws + pl.h[i];
    // the projection: the tail's rows of x, gathered, against proj_i [d_i, C] -> h_i, compact, 16-bit
    VocabScoreRowsP q = {};
    q.x = a.x; q.w = a.proj[i]; q.logits = hi; q.pick = reinterpret_cast<VsPick*>(a.ws + pl.inner);
    q.ldx = a.ldx; q.ldl = a.dims[i]; q.M = a.M; q.K = a.C; q.V = a.dims[i]; q.dtype = a.dtype; q.x_f32 = a.x_f32;
    q.xrows = list; q.count = count + i; q.logits_only = 1;
    if (const int rc = vocab_score_rows(q, st)) return rc;
    if (a.hmask[i]) {                                  // (ea_adaptive_score_masked: the Dropout inside the tail, one launch)
      RowsMaskP k = {};
      k.h = reinterpret_cast<uint16_t*>(hi); k.mask = reinterpret_cast<const uint16_t*>(a.hmask[i]); k.count = count + i;
      k.M = a.M; k.D = a.dims[i]; k.dtype = a.dtype;
      if (const int rc = rows_mask16(k, st)) return rc;
    }
    // the tail: h_i as it lies, the targets through the list, c_i taken off
    VocabScoreRowsP t = {};
    t.x = hi; t.w = a.table[i]; t.targets = a.targets; t.pick = reinterpret_cast<VsPick*>(a.ws + pl.inner);
    t.token = reinterpret_cast<int64_t*>(a.ws + pl.token[i]); t.lse = reinterpret_cast<float*>(a.ws + pl.lse[i]);
    t.logp = reinterpret_cast<float*>(a.ws + pl.logp[i]);
    t.ldx = a.dims[i]; t.M = a.M; t.K = a.dims[i]; t.V = (int)(a.cut[i + 1] - a.cut[i]); t.dtype = a.dtype;
    t.trows = list; t.count = count + i; t.target_base = a.cut[i];
    if (const int rc = vocab_score_rows(t, st)) return rc;
    c.logp_tail[i] = t.logp;
  }
  for (int i = a.n; i < AS_MAX_TAILS; ++i) c.logp_tail[i] = c.logp_tail[0];
  c.head_target = head_target; c.rows = rows; c.count = count; c.logp_head = logp_head; c.logp = a.logp; c.c0 = a.cut[0];
  c.M = a.M;
  hipLaunchKernelGGL(adaptive_combine_kernel, dim3((unsigned)((a.M - 1) / AC_THREADS + 1), (unsigned)(a.n + 1)), dim3(AC_THREADS),
                     0, st, c);
  return (int)hipGetLastError();
}

}  // namespace ea
