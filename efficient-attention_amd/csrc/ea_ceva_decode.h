// ea_ceva_decode.h -- parameter block of the single-query decoding kernels of causal EVA (ea_ceva_decode.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace ea {

struct DecT {                 // [B,H,N,D] view of any I/O type, element strides
  const char* p;
  int64_t sb, sh, sn;
};

struct DecP {
  DecT q, k, v;               // the cache rows [B,H,cap,D] (dtype); [B,H,ring,D] when ring != 0
  DecT lk, lv;                // rf_k_bar, beta [B,H,Lcap,D] fp32 (the l16 launches: dtype): read by attn, written by close
  DecT o;                     // attn: out [B,H,T_new,D] (dtype), row t - t0
  const uint8_t* pad;         // [B,cap] ([B,ring]) 1 = padded position, or null
  const float* bias;          // [w, w + e] dense single-head bias (natural-log domain), or null
  const float* mu[8];         // close: the mu networks' parameters in _mu_params() order
  int B, H, D, dtype, w, e, r, t0, T, c_first, c_last, cap, adaptive;
  float scale;
  const int32_t* pos;         // static decoding: the token count in device memory (t0, c_first, c_last unused), or null
  int ring;                   // static decoding: q, k, v and pad hold `ring` rows, token n at row n % ring; 0 = cap rows, linear
  const int32_t* ntok;        // per-sequence static decoding: pos is [B] and ntok [B] holds each element's tokens of this step
                              // (written by append); null = one shared count, every element takes all T tokens
};

struct AppP {                 // static decoding, append: the step's rows into the cache at rows *pos ..
  const char* src;            // [T, B, 3, H, D] time-first rows of the step (the cache's dtype)
  const uint8_t* src_pad;     // [B, T] the step's pad flags, or null (zeros)
  char* cache;                // [B, cap, 3, H, D]
  uint8_t* pad;               // [B, cap]
  const int32_t* pos;
  int32_t* status;            // set to 1 when the step would pass cap (nothing is written)
  int B, T, cap, row_bytes;   // row_bytes = 3 H D element bytes, a multiple of 16
  int ring;                   // cache and pad hold `ring` rows, token n at row n % ring (cap bounds the step); 0 = cap rows
  int32_t* ntok;              // per-sequence: [B], element b's tokens of this step = the positions before its first flag in
                              // src_pad; pos and status are [B] then, and nothing is stored for the flagged positions.  null = shared
};

struct DecSplitP {               // attn_split: a DEV step of at most 8 tokens, its tile range shared by `parts` workgroups
  DecP d;                     // the step, as attn takes it (d.pos != null)
  float* ws;                  // [B, H, 8, parts, D + 4] fp32 partials (acc[D], m, l, 2 unused) of the step's tokens
  int parts;
};

struct DecMergeP {               // merge: out row t = the parts of step token t combined and normalised
  DecT o;                     // out [B,H,T_new,D] (dtype)
  const float* ws;
  const int32_t* pos;
  const int32_t* ntok;        // null = shared count
  int H, T, cap, parts;
};

enum DecKind { DEC_CLOSE, DEC_ATTN };
// the step's close or attn launch; p.pos != null: t0 = *p.pos (needs p.pad); p.ring != 0: ring rows (needs p.pos);
// p.ntok != null: t0 = p.pos[b], p.ntok[b] tokens (needs p.pos).  l16 (a compact state; needs p.pos and a 16-bit p.dtype):
// p.lk, p.lv are rows of p.dtype, strides in those elements -- close rounds its two stores, attn reads 16-bit landmark rows
int ceva_decode_launch(DecKind kind, const DecP& p, hipStream_t st, bool l16 = false);
// attn as two launches for a DEV step of T <= 8 tokens (ea_ceva_decode_split.h): `parts` workgroups per window block write
// partials to ws, then one workgroup per token combines them; p as for DEC_ATTN, 2 <= parts <= 64
int ceva_sdecode_attn_split(const DecP& p, int parts, float* ws, hipStream_t st, bool l16 = false);
int ceva_sdecode_merge(const DecMergeP& p, int D, int dtype, int BH, hipStream_t st);
int ceva_sdecode_append(const AppP& p, hipStream_t st);
// *pos += T; ntok != null: pos[b] += ntok[b] for the B elements
int ceva_sdecode_advance(int32_t* pos, const int32_t* ntok, int B, int T, int cap, hipStream_t st);

}  // namespace ea
