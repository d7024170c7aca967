// ea_linear.h -- dispatchers of the projection kernels: ea_linear.hip, ea_proj_rs.hip (192-wide, register-resident),
// ea_dgrad_rs.hip (their input gradient) and ea_wgrad.hip (weight gradient, partial sums).
#pragma once
#include "ea_common.h"

namespace ea {

int linear_supported(int K, int NO);
int proj_rs_supported(int K, int NO);
int proj_rs_pool_supported(int K, int NO, int B, int gh, int gw, int r);
int proj_rs_dispatch(int dtype, const void* a, int a_f32, const float* w, const float* bias, void* y, void* a_cast, int rows,
                     long lda, long ldy, hipStream_t st, int B, int gh, int gw, int r, float* pq, float* pk, void* w_cast,
                     const void* wsw);
int w192_prepare_dispatch(int dtype, const float* wq, const float* wp, void* w16q, void* wsw, void* w16p, void* w16pT, void* wtsw,
                          void* wp_rs, void* wpT_rs, hipStream_t st);
// ea_linear_rs192.hip: weight row behind MFMA row li of tile j of column pair `pair` (the image's piece order)
constexpr int rs192_row(int pair, int j, int li) { return 32 * pair + 8 * (li >> 2) + (li & 3) + 4 * j; }
int linear_rs192_supported(int rows, long lda, long ldy);
int linear_rs192_dispatch(int dtype, const void* a, long lda, const void* wimg, const float* bias, void* y, long ldy, int rows,
                          hipStream_t st);
int dgrad_rs_supported(int K, int NO);
int dgrad_fin_launch(int dtype, const void* dqkv, long ldy, const void* qkv, long ldq, const void* w, int w_f32, void* dx, int dx_f32,
                     long ldx, int B, int gh, int gw, int pool_r, int C, float scale, const float* qbar, const float* uq,
                     const float* lse_t, const float* dpq, const float* dpk, hipStream_t st);
int dgrad_rs_dispatch(int dtype, const void* dy, const void* w, int w_f32, void* dx, int dx_f32, int rows, long ldy, long ldx,
                      hipStream_t st);
int linear_dispatch(int dtype, const void* a, int a_f32, const void* w, int w_mode, const float* bias, void* y, int y_f32,
                    void* a_cast, int rows, int K, int NO, long lda, long ldy, hipStream_t st);
int wgrad_slices(int rows, int M, int K);
int wgrad_pair_slices(int rows, int M1, int K1, int M2, int K2);
int wgrad_pair_dispatch(int dtype, int rows, const void* dy1, const void* x1, float* part1, float* db1, long ld1, int M1, int K1,
                        const void* dy2, const void* x2, float* part2, float* db2, long ld2, int M2, int K2, hipStream_t st);
int wgrad_dispatch(int dtype, const void* dy, const void* x, float* part, float* db_part, long part_ld, int rows, int M,
                   int K, hipStream_t st);
int part_sum_dispatch(const float* part, float* out, int S, int n, long ld, hipStream_t st);
int multi_sum_dispatch(int K, const float* const* part, const int* S, const int* n, const long long* ld, float* const* out,
                       hipStream_t st);

}  // namespace ea
