// ea_kernelized.h -- parameter block of the kernelized-attention feature-map family (ea_kernelized.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "ea_t4.h"

namespace ea {

// feature maps of the reference's KernelizedAttention (kernelized_attention.py, `proj_method`)
enum KzMap { KZ_FAVORP = 0, KZ_RELU = 1, KZ_FOURIER = 2, KZ_RELU_ONLY = 3, KZ_SIGMOID_ONLY = 4, KZ_DPFP = 5 };

constexpr int KZ_MAX_M = 128;                // rows of W (a multiple of 16)
constexpr int KZ_MAX_F = 256;                // features after cos weighting
constexpr bool kz_has_w(int map) { return map <= KZ_FOURIER; }
// feature count of a map at head dim 64 before cos weighting (0: not a map / geometry the kernels are built for)
inline int kz_base_features(int map, int M, int nu) {
  switch (map) {
    case KZ_FAVORP: case KZ_RELU: return M;
    case KZ_FOURIER: return 2 * M;
    case KZ_RELU_ONLY: case KZ_SIGMOID_ONLY: return 64;
    case KZ_DPFP: return nu >= 1 ? 128 * nu : 0;
    default: return 0;
  }
}

struct KzP {
  T4 q, k, v, o, dout, dq, dk, dv;           // [B,H,N,64] views
  const uint8_t* mask;                       // [B,N] key padding mask or null
  const float* W;                            // [H, M, 64] random features (favorp / relu / fourier), else null
  const float *kv, *ksum, *dkv, *dksum;      // [BH, F, 64], [BH, F]
  float* p_st;                               // [BH, S, 2] slice statistics (key side, query side)
  float *p_kv, *p_ks;                        // slice partials [BH, S, F, 64], [BH, S, F]
  float* p_dw;                               // [H, B, 2, S, M, 64] partials of dW (q side 0, k side 1), or null
  int B, H, N, M, F, Fb, nu, cos, map;       // F = features after cos weighting, Fb = before
  int S, tps, fb, dtype;                     // S, tps, fb (feature block) set by the dispatcher
};

int kz_dispatch(int which, const KzP& p, hipStream_t st);   // 0 stats, 1 kv, 2 out, 3 bwd_q, 4 bwd_k

}  // namespace ea
