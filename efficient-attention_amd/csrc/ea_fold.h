// ea_fold.h -- parameter block and dispatchers of the folded generator projection (ea_fold.hip).
#pragma once
#include "ea_common.h"

namespace ea {

struct FoldP {
  const float *W, *b, *Gq, *Gk, *gqb, *gkb;     // [3C, C], [3C] | null, [d, d] x 2, [d] x 2
  char* w_ext;                                   // [5C, C] element type
  char* b_ext;                                   // [5C] element type | null
  float *bias_q, *bias_k;                        // [h, d]
  // backward
  const float *dW_ext, *db_ext, *dbias_q, *dbias_k;   // [5C, ldw], [5C] | null, [h, d] x 2
  float *dW, *db, *dGq, *dGk, *dgqb, *dgkb;            // [3C, C], [3C] | null, [d, d] x 2, [d] x 2
  float *dG_part, *dG_base;                            // [2][h FB_SPLIT][64 x 64] partials, [2][64 x 64] bias part
  long ldw;
  int C, h, d;
};

int fold_dispatch(bool bwd, int dtype, const FoldP& p, hipStream_t st);
int fold_bwd_parts(int heads);

}  // namespace ea
