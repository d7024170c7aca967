// ea_softmax.h -- parameter block of the streaming softmax-attention kernels (ea_softmax.hip).
#pragma once
#include "ea_common.h"

namespace ea {

struct SmP {
  struct { char* p; int64_t sb, sh, sn; } q, k, v, o, dout, dq, dk, dv;
  const uint8_t* mask;
  // attention dropout (abstract_attention.py:131): keep mask [B,H,N,keep_ld] u8 over the keys of
  // every query (non-zero = kept), kept probabilities scaled by keep_scale = 1/(1-p); or nullptr
  const uint8_t* keep;
  int keep_ld;
  float keep_scale;
  // key_norm_bias: logits s q.k_j - s |k_j|^2 / 2 (randomized_attention.py:44-50, the second softmax of
  // RA: prm_projection's norm term as a per-key bias, differentiated with respect to k)
  int key_norm_bias;
  // sample: instead of out, draw one key index per query from softmax(s q.k) by Gumbel-max
  // (randomized_attention.py:35-37); counter-based noise from `seed`
  long long* sample_out;           // [BH, N]
  const unsigned long long* seed;  // device scalar
  float* lse;      // [BH, N] natural log
  float* delta;    // [BH, N]
  int B, H, N;
  float scale, scale_log2;
};

int softmax_dispatch(int which, const SmP& p, int dtype, int D, hipStream_t st);

// The 16-token tiles a wave of the softmax kernels works on (QT of sm_fwd_kernel / sm_bwd_dq_kernel, KT of sm_bwd_dkv_kernel)
// for bh = B H sequences of N tokens at head size D on a device of `cus` compute units; which: 0 forward (1, 2 or 4),
// 1 backward (1 or 2; both backward kernels); has_keep: a dropout keep mask is passed.  The one statement of the rule:
// launch_sm_dr launches what it answers, ea_softmax_tiles (C ABI) reports it.  Pure but for the dev knobs EA_SM_QT (forward)
// and EA_SM_BQT (backward), read once per process; a knob value that is no tile count of that direction is ignored.
int softmax_tiles(int which, long bh, int N, int D, bool has_keep, int cus);

}  // namespace ea
