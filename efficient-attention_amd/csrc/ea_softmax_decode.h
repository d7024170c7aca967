// ea_softmax_decode.h -- parameter blocks of the KV-cache decoding kernels of causal softmax attention (ea_softmax_decode.hip)
#pragma once
#include "ea_ceva_decode.h"      // DecT, and merge / advance, which a softmax step shares with a causal EVA step

namespace ea {

constexpr int SDEC_TILE = 64;            // keys per tile: what a wave of attn_split owns, what attn_mm streams through LDS
constexpr int SDEC_QMAX = 8;             // the most tokens of a split step (QPW of ea_ceva_decode.hip: the workspace is shared)

struct SdecP {                // a step of T tokens at *pos on the cache k, v [B,H,cap,D]
  DecT q;                     // [B,H,T,D] view of the step's projected rows
  DecT k, v;                  // the cache
  DecT o;                     // out [B,H,T,D], row t - *pos
  const uint8_t* pad;         // [B,cap] 1 = padded key
  const int32_t* pos;         // device: tokens in the cache before this step
  int B, H, D, dtype, T, cap;
  float scale;
  float* ws;                  // attn_split, parts > 1: fp32 [B,H,8,parts,D+4] partials (acc[D], max, sum, 2 unused), natural log
  int parts;
  const int32_t* ntok;        // per-sequence counts: pos is [B] and ntok [B] holds each row's tokens of this step (written by
                              // append); null = one shared count, every row takes all T tokens
};

struct SdecAppP {             // append: the step's K and V rows, and its pad flags, into the cache at rows *pos ..
  const char* src;            // [T, B, 3, H, D] time-first rows of the step
  const uint8_t* src_pad;     // [B, T], or null (zeros)
  DecT k, v;
  uint8_t* pad;
  const int32_t* pos;
  int32_t* status;            // set to 1 when the step would pass cap (nothing is written)
  int B, H, D, T, cap;
  int32_t* ntok;              // per-sequence: [B], row b's tokens of this step = the positions before its first flag in src_pad;
                              // pos and status are [B] then, and nothing is stored for the flagged positions.  null = shared
};

// every launch: ntok != null selects the per-sequence instance of its kernel
int softmax_sdecode_append(const SdecAppP& p, hipStream_t st);
// T <= 8; parts == 1: normalises and writes out itself; parts > 1: partials to ws, ceva_sdecode_merge folds them
int softmax_sdecode_attn_split(const SdecP& p, hipStream_t st);
int softmax_sdecode_attn_mm(const SdecP& p, hipStream_t st);

// The parts a split step takes on a device of `cus` compute units: the smallest P with B H P >= 2 cus, at most one part per
// 64-key tile of a full cache and at most 64.  The factor 2 (two workgroups of four waves per compute unit) was not derived
// from a measurement; the one sweep since (tools/softmax_decode_latency.py, DESIGN.md 4b: one layer, d 128, B 1 / 8) puts it
// within 0 - 13 % of the best part count of every row, half as many parts being a little faster at B = 1.
inline int softmax_sdecode_parts(long bh, int cap, int cus) {
  const long want = (2L * cus + bh - 1) / bh, most = (cap + SDEC_TILE - 1) / SDEC_TILE;
  const long p = want < most ? want : most;
  return (int)(p < 1 ? 1 : p > 64 ? 64 : p);
}

}  // namespace ea
