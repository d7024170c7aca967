// ea_t4.h -- the strided [B,H,N,D] view of the kernel parameter blocks, and the one rule a caller's ea_t4 must meet.
#pragma once
#include <stdint.h>
#include "../../include/ea_hip.h"

namespace ea {

struct T4 {
  char* p;
  int64_t sb, sh, sn;       // element strides; D is contiguous
};
inline T4 mk(const ea_t4* t) {
  T4 r;
  r.p = t ? (char*)t->ptr : nullptr;
  r.sb = t ? t->sb : 0; r.sh = t ? t->sh : 0; r.sn = t ? t->sn : 0;
  return r;
}

// 16-byte vector access to rows of D elements of elem_bytes each: the base is 16-byte aligned, every stride is a multiple of
// 16 / elem_bytes elements (8 of a 16-bit type, 4 of fp32), and a token's row holds the head dim
inline bool view_ok(const ea_t4* t, int D, int elem_bytes) {
  const int a = 16 / elem_bytes;
  return t && t->ptr && ((uintptr_t)t->ptr % 16 == 0) && t->sb % a == 0 && t->sh % a == 0 && t->sn % a == 0 && t->sn >= D;
}

}  // namespace ea
