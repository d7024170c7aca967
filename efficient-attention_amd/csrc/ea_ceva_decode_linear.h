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

}  // namespace ea
