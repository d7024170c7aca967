// ea_ceva_decode_vocab.h -- parameter block of the greedy token pick on a held vocabulary table (ea_ceva_decode_vocab.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace ea {

constexpr int VOC_TILE = 16;  // columns of one workgroup: one MFMA column tile, one partial per row

// one candidate of a row: the fp32 sum and its column
struct alignas(8) VocPick {
  float v;
  int32_t i;
};

struct DecVocabP {
  const char* x;              // [M, ldx] rows, fp32 or the table's type
  const char* w;              // [V, K] row-major 16-bit table
  char* logits;               // [M, ldl] rows, fp32 or the table's type, or null: nothing is stored
  VocPick* ws;                // [M, ceil(V / 16)] partial picks
  int64_t* token;             // [M]
  float* top;                 // [M], or null
  int64_t ldx, ldl;           // row strides in elements
  int M, K, V;                // 1 <= M <= 64, K % 32 == 0, V >= 1
  int dtype;                  // EA_BF16 | EA_F16: w
  int x_f32, l_f32;           // 1: fp32 rows (x is rounded to `dtype` on load)
};

// bytes of ws for (M, V); < 0: outside the envelope
int64_t ceva_sdecode_vocab_ws(int M, int V);
int ceva_sdecode_vocab_argmax(const DecVocabP& p, hipStream_t st);

}  // namespace ea
