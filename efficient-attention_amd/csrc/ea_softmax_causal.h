// ea_softmax_causal.h -- parameter block of the causal streaming softmax-attention kernels (ea_softmax_causal.hip).
#pragma once
#include "ea_common.h"

namespace ea {

// One sequence of N queries over the same N keys, query i sees keys j <= i.  The fields are SmP's (ea_softmax.h) without the
// key-norm bias and the sampler, which the causal kernels do not build.
struct SmcP {
  struct { char* p; int64_t sb, sh, sn; } q, k, v, o, dout, dq, dk, dv;
  const uint8_t* mask;             // [B, N], non-zero = padded key (-inf), or nullptr
  // attention dropout: keep mask [B,H,N,keep_ld] u8 over the keys of every query (non-zero = kept), kept probabilities scaled
  // by keep_scale = 1/(1-p); or nullptr.  Entries above the diagonal are never read.
  const uint8_t* keep;
  int keep_ld;
  float keep_scale;
  float* lse;      // [BH, N] natural log
  float* delta;    // [BH, N]
  int B, H, N;
  float scale, scale_log2;
};

// which: 0 forward, 1 backward (the query-side pass, then the key-side pass); tiles: a count softmax_causal_tiles_ok accepts
int softmax_causal_dispatch(int which, const SmcP& p, int dtype, int D, int tiles, hipStream_t st);

// The 16-token tiles a wave works on (QT of smc_fwd_kernel / smc_bwd_dq_kernel, KT of smc_bwd_dkv_kernel) for bh = B H sequences
// of N tokens at head size D on a device of `cus` compute units; which: 0 forward (1, 2 or 4), 1 backward (1 or 2).  A workgroup's
// work grows linearly with its position, so nb = ceil(N / (64 t)) workgroups of a sequence are worth (nb + 1) / 2 of the
// heaviest one: t tiles are taken when bh (nb + 1) / 2 >= 2 cus still holds.  Pure: no environment knob.
int softmax_causal_tiles(int which, long bh, int N, int D, bool has_keep, int cus);

// whether the direction and the geometry have an instantiation with `tiles` tiles per wave (tiles > 0)
bool softmax_causal_tiles_ok(int which, int tiles, int D, bool has_keep);

}  // namespace ea
