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
  DecT q, k, v;               // the cache rows [B,H,cap,D] (dtype)
  DecT lk, lv;                // rf_k_bar, beta [B,H,Lcap,D] fp32: read by attn, written by close
  DecT o;                     // attn: out [B,H,T_new,D] (dtype), row t - t0
  const uint8_t* pad;         // [B,cap] 1 = padded position, or null
  const float* bias;          // [w, w + e] dense single-head bias (natural-log domain), or null
  const float* mu[8];         // close: the mu networks' parameters in _mu_params() order
  int B, H, D, dtype, w, e, r, t0, T, c_first, c_last, cap, adaptive;
  float scale;
};

int ceva_decode_dispatch(bool close, const DecP& p, hipStream_t st);

}  // namespace ea
