// ea_proj.h -- dispatchers of the small reductions and copies of ea_proj.hip.
#pragma once
#include "ea_common.h"

namespace ea {

int colsum_parts(int rows, int cols);
int colsum_dispatch(int dtype, const void* x, float* part, float* out, int rows, int cols, hipStream_t st);
int colsum_f32_dispatch(const float* x, float* out, int rows, int cols, const float* x2, float* out2, int cols2, hipStream_t st);
int gather_sum_dispatch(const float* g, const int* inv, float* out, int rows, int K, int cols, hipStream_t st);
int slice_sum_dispatch(const float* a, const float* p, float* out, int BH, int S, int n, float scale, hipStream_t st);
int multi_cast_dispatch(int dtype, int K, const float* const* src, const long long* n, void* const* dst, hipStream_t st);
int table_bias_fwd_dispatch(const float* table, const int* idx, float* out, int h, int th, int Wq, int Wk, int ld, float scale,
                            hipStream_t st);
int table_bias_bwd_dispatch(const float* g, const int* inv, float* dtable, int rows, int K, int h, int Wq, int Wk, int ld,
                            float scale, hipStream_t st);
int stream_copy_dispatch(const void* src, void* dst, size_t bytes, hipStream_t st);

}  // namespace ea
