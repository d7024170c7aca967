// ea_ceva_decode_linear.h -- parameter block of the few-row projection of a decoding step (ea_ceva_decode_linear.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace ea {

struct DecLinP {
  const char* x;              // [M, ldx] rows, fp32 or the weight's type
  const char* w;              // [N, K] row-major 16-bit weight
  const char* bias;           // [N] in the weight's type, or null
  char* y;                    // [M, ldy] rows, the weight's type or fp32
  int64_t ldx, ldy;           // row strides in elements
  int M, K, N;                // 1 <= M <= 64, K % 32 == 0, N % 16 == 0
  int dtype;                  // EA_BF16 | EA_F16: w, bias
  int x_f32, y_f32;           // 1: fp32 rows (x is rounded to `dtype` on load)
};

int ceva_sdecode_linear(const DecLinP& p, hipStream_t st);

// the fused few-row linear of a decoder layer's feed-forward (ABI 24): a block of its own, so that the plain kernel's
// parameter block and with it its code stay what they were
constexpr int EA_LIN_MAX_ROWS = 64;
struct DecLinFusedP {
  const char* x;              // [M, ldx] rows, fp32 or the weight's type; never y
  const char* w;              // [N, K] row-major 16-bit weight
  const char* bias;           // [N] in the weight's type, or null
  const float* gamma;         // [K] fp32, LayerNorm over K in front of the product; both null: none
  const float* beta;          // [K] fp32
  const char* res;            // [M, ldr] rows added after the activation, fp32 or the weight's type, or null; may be y
  char* y;                    // [M, ldy] rows, the weight's type or fp32
  int64_t ldx, ldr, ldy;      // row strides in elements
  int M, K, N;                // 1 <= M <= 64, K % 32 == 0, N % 16 == 0
  int dtype;                  // EA_BF16 | EA_F16: w, bias
  int x_f32, res_f32, y_f32;  // 1: fp32 rows
  int act;                    // 0 none, 1 relu
  float ln_eps;
};

int ceva_sdecode_linear_fused(const DecLinFusedP& p, hipStream_t st);

}  // namespace ea
