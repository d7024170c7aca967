// ea_kernelized.h -- parameter block of the kernelized-attention feature-map family (ea_kernelized.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "ea_performer_f32.h"      // Pf32T: a strided [B,H,N,64] view

namespace ea {

// feature maps of the reference's KernelizedAttention (kernelized_attention.py, `proj_method`)
enum KzMap { KZ_FAVORP = 0, KZ_RELU = 1, KZ_FOURIER = 2, KZ_RELU_ONLY = 3, KZ_SIGMOID_ONLY = 4, KZ_DPFP = 5 };

struct KzP {
  Pf32T q, k, v, o, dout, dq, dk, dv;
  const uint8_t* mask;                       // [B,N] key padding mask or null
  const float* W;                            // [H, M, 64] random features (favorp / relu / fourier), else null
  const float *kv, *ksum, *dkv, *dksum;      // [BH, F, 64], [BH, F]
  float* p_st;                               // [BH, S, 2] slice statistics (key side, query side)
  float *p_kv, *p_ks;                        // slice partials [BH, S, F, 64], [BH, S, F]
  float* p_dw;                               // [H, B, 2, S, M, 64] partials of dW (q side 0, k side 1), or null
  int B, H, N, M, F, Fb, nu, cos, map;       // F = features after cos weighting, Fb = before
  int S, tps, fb, dtype;                     // S, tps, fb (feature block) set by the dispatcher
};

int kz_slices(int BH, int N);
int kz_dispatch(int which, const KzP& p, hipStream_t st);   // 0 stats, 1 kv, 2 out, 3 bwd_q, 4 bwd_k

}  // namespace ea
