// ea_ceva_decode_vocab.h -- parameter blocks of the greedy and the sampled token pick and of the token log-probabilities on a
// held vocabulary table
// (ea_ceva_decode_vocab.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace ea {

constexpr int VOC_TILE = 16;  // columns of one workgroup: one MFMA column tile, one partial per row

// one candidate of a row: the fp32 sum and its column
struct alignas(8) VocPick {
  float v;
  int32_t i;
};

struct DecVocabP {
  const char* x;              // [M, ldx] rows, fp32 or the table's type
  const char* w;              // [V, K] row-major 16-bit table
  char* logits;               // [M, ldl] rows, fp32 or the table's type, or null: nothing is stored
  VocPick* ws;                // [M, ceil(V / 16)] partial picks
  int64_t* token;             // [M]
  float* top;                 // [M], or null
  int64_t ldx, ldl;           // row strides in elements
  int M, K, V;                // 1 <= M <= 64, K % 32 == 0, V >= 1
  int dtype;                  // EA_BF16 | EA_F16: w
  int x_f32, l_f32;           // 1: fp32 rows (x is rounded to `dtype` on load)
};

constexpr int VOC_SAMPLE_MAX_K = 64;  // top_k of the sampled pick: the selection is sorted by one wave

// the sampled pick's second launch (ceva_vocab_sample_kernel); a block of its own: DecVocabP is the table pass's
// parameter and stays what it is
struct DecSampleP {
  const VocPick* ws;          // [M, ceil(V / 16)] candidates of the first launch
  const float* logits;        // [M, ldl] fp32 logits of the first launch
  int64_t* token;             // [M]
  int64_t* ctr;               // [M] draw counters, read and advanced by one
  const int32_t* sid;         // [M] stream ids
  int32_t* sel_idx;           // [M, top_k] the selection in order, or null
  float* sel_val;             // [M, top_k], or null
  int32_t* kept;              // [M], or null
  int64_t ldl;
  int V, top_k;
  float top_p, temperature;
  uint32_t seed_lo, seed_hi;
};

// token log-probabilities (ABI 28): the parameter block of ceva_rows_kernel as the table pass that also writes one
// sum exp(logit - tile maximum) per tile, and of ceva_vocab_pick_kernel as the pick with the log-sum-exp and the
// log-probability; a block of its own: DecVocabP and DecSampleP stay what they are.
//   lse[m]  = log sum_v exp(logit[m, v]) over the whole row: the RAW distribution, temperature 1, nothing truncated -- in the
//             sampled mode too, whatever temperature, top_k and top_p the draw was made with
//   logp[m] = tl - lse[m]; tl: logits[m, token_in[m]] in the sampled mode (token_in set), else logit[m, targets[m]] when
//             targets are given (a target outside [0, V): NaN), else top[m]
struct DecLseP {
  const char* x;              // [M, ldx] rows, fp32 or the table's type
  const char* w;              // [V, K] row-major 16-bit table
  char* logits;               // [M, ldl] rows, fp32 or the table's type, or null (the sampled mode: fp32, required)
  VocPick* ws;                // [M, ceil(V / 16)] partial picks (m_t, i_t)
  float* lws;                 // [M, ceil(V / 16)] s_t = sum over the tile's columns of exp(logit - m_t)
  float* tlogit;              // [M] the targets' logits
  const int64_t* targets;     // [M], or null
  const int64_t* token_in;    // [M] the tokens drawn before the second launch: the sampled mode; or null
  int64_t* token;             // [M]; not written in the sampled mode
  float* top;                 // [M], or null; not written in the sampled mode
  float* lse;                 // [M]
  float* logp;                // [M]
  int64_t ldx, ldl;           // row strides in elements
  int M, K, V;                // 1 <= M <= 64, K % 32 == 0, V >= 1
  int dtype;                  // EA_BF16 | EA_F16: w
  int x_f32, l_f32;           // 1: fp32 rows (x is rounded to `dtype` on load)
};

// the beam step (ABI 32): the parameter block of ceva_vocab_beam_rows_kernel (one workgroup per row, behind the table pass
// on DecLseP) and of ceva_vocab_beam_merge_kernel (one workgroup per sentence); a block of its own: the others stay what
// they are.  M = S W rows, row s W + b is beam b of sentence s.  The merge alone reads from cand_idx on.
struct DecBeamP {
  const VocPick* ws;          // [M, ceil(V / 16)] candidates of the table pass
  const float* lws;           // [M, ceil(V / 16)] its tile sums
  const float* logits;        // [M, ldl] its fp32 logits
  float* lse;                 // [M]
  float* sel_val;             // [M, 2 W] the selected logits, or null
  int64_t ldl;
  int V;
  int32_t* cand_idx;          // [M, 2 W] a row's candidates in order, kc live (the forced step: 1)
  float* cand_score;          // [M, 2 W] score[m] + (logit - lse[m])
  float* score;               // [M] in / out: the beams' cumulative scores
  int32_t* t;                 // [S] in / out: tokens generated
  int32_t* nfin;              // [S] in / out: finished hypotheses
  int32_t* done;              // [S] in / out
  int64_t* token;             // [M]
  int64_t* parent;            // [M] global rows: reorder_incremental_state's new_order
  int32_t* hist_tok;          // [max_new, M]
  int32_t* hist_par;          // [max_new, M] beams
  float* fin_score;           // [S, W]
  int32_t* fin_len;           // [S, W]
  int32_t* fin_beam;          // [S, W]
  int S, W, kc, eos, max_new;
};

// bytes of the beam step's workspace for (M, V, W); < 0: outside the envelope
int64_t ceva_sdecode_vocab_beam_ws(int M, int V, int W);
// p's and b's workspace pointers from one buffer of that size (p->M, p->V, b->W are read; b's candidate lists and lse stay
// where the caller has put them)
void ceva_sdecode_vocab_beam_carve(void* ws, DecLseP* p, DecBeamP* b);
// the table pass with tile sums on p, then the rows and the merge kernel on b
int ceva_sdecode_vocab_beam(const DecLseP& p, const DecBeamP& b, hipStream_t st);
// the merge kernel alone, on the caller's candidate lists
int ceva_beam_merge(const DecBeamP& b, hipStream_t st);

// ---- the constrained beam step (ABI 36) ----
constexpr int BAN_MAX_STATIC = 16;  // static bans of a capture
constexpr int BAN_MAX_NGRAM = 16;   // no_repeat_ngram_size

// the ban-list launch (beam_bans_kernel, one workgroup per row): it keeps the beams' generated tokens row-major in `gen` and
// writes a row's banned tokens; a block of its own: DecBeamP stays what it is.  Row m = s W + b; t = t[s].
struct BeamBanP {
  const int32_t* t;           // [S] tokens generated (read, never written)
  const int32_t* done;        // [S] the rows of a done sentence are skipped
  const int32_t* hist_tok;    // [max_new, M] row t - 1 is read: what the previous merge wrote
  const int32_t* hist_par;    // [max_new, M]
  const int32_t* prompt_tok;  // [S, prompt_cap] (prompt_cap == 0: not read)
  const int32_t* prompt_len;  // [S] clamped to 0 .. prompt_cap (prompt_cap == 0: not read)
  int32_t* gen;               // [2, M, max_new] buffer t & 1 is written, buffer (t - 1) & 1 read
  int32_t* ban;               // [M, cap] a row's banned tokens, duplicates allowed
  int32_t* nban;              // [M] how many
  int S, W, eos, max_new, min_len, ngram, prompt_cap, cap, n_static;
  int32_t static_tok[BAN_MAX_STATIC];
};

// what the constrained row kernels read of it
struct BanListP {
  const int32_t* ban;         // [M, cap]
  const int32_t* nban;        // [M]
  int cap;
};

// entries of a row's list: prompt_cap + max_new windows at the most, the static bans and eos
inline int64_t beam_ban_cap(int prompt_cap, int max_new) { return (int64_t)prompt_cap + max_new + BAN_MAX_STATIC + 1; }
// bytes of ban and nban behind the unconstrained entry's workspace; < 0: outside the envelope
int64_t ceva_beam_bans_ws(int M, int prompt_cap, int max_new);
// b.ban, b.nban (and b.cap) from a buffer of that size
void ceva_beam_bans_carve(void* ws, int M, BeamBanP* b);
// the ban-list launch alone
int ceva_beam_bans(const BeamBanP& b, hipStream_t st);
// the table pass on p, the ban-list launch on c, the rows kernel with c's list applied behind lse, the merge on b
int ceva_sdecode_vocab_beam_c(const DecLseP& p, const DecBeamP& b, const BeamBanP& c, hipStream_t st);

// bytes of ws for (M, V); < 0: outside the envelope
int64_t ceva_sdecode_vocab_ws(int M, int V);
int ceva_sdecode_vocab_argmax(const DecVocabP& p, hipStream_t st);
// the first launch on p (token and top are not read), the second on s
int ceva_sdecode_vocab_sample(const DecVocabP& p, const DecSampleP& s, hipStream_t st);

// bytes of lws and tlogit together for (M, V); < 0: outside the envelope
int64_t ceva_sdecode_vocab_lse_ws(int M, int V);
// the table pass with tile sums, then the pick with lse and logp
int ceva_sdecode_vocab_logprob(const DecLseP& p, hipStream_t st);
// that entry's first launch alone (candidates, tile sums, the targets' logits; token, top, lse, logp are not written): the
// adaptive pick folds the partials of several tables itself (ea_adaptive_pick.hip)
int ceva_sdecode_vocab_table_pass(const DecLseP& p, hipStream_t st);
// the table pass with tile sums on p, ceva_vocab_sample_kernel on s, then lse and logp of the drawn tokens (p.token_in = s.token)
int ceva_sdecode_vocab_sample_logprob(const DecLseP& p, const DecSampleP& s, hipStream_t st);

}  // namespace ea
