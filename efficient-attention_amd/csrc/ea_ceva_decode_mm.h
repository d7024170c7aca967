// ea_ceva_decode_mm.h -- the matrix-core attn launch of a static causal EVA decoding step (ea_ceva_decode_mm.hip)
#pragma once
#include "ea_ceva_decode.h"

namespace ea {

constexpr int DMM_TILE = 64;             // queries per workgroup / key rows per streamed tile
constexpr int DMM_GROUP = 16;            // queries per wave: groups are aligned to 16 in the absolute token index

// 64-query tiles a step of T tokens can need, wherever it starts: its first group begins up to 15 tokens before it
inline __host__ __device__ int dmm_query_tiles(int T) { return (T + DMM_GROUP - 1 + DMM_TILE - 1) / DMM_TILE; }

// attn of a DEV step (p.pos != null, p.pad != null) on 16-bit rows, p as ceva_decode_launch(DEC_ATTN, ..) takes it; l16: p.lk,
// p.lv are rows of p.dtype.  EA_E_UNSUPPORTED for fp32 rows, D outside {64, 128} and w % 16 != 0: no instance
int ceva_sdecode_attn_mm(const DecP& p, hipStream_t st, bool l16);

}  // namespace ea
