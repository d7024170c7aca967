// ea_lara_xp.hip -- LARA forward combine with the output projection inside (ABI 29).
//
//   out_n = sum_c W[c,n] kv_c   (ea_lara_x.hip, LX_FWDM: the statistics pass's slice partials merged on load)
//   y_n   = W_proj out_n + bias  for the three heads of a token together (model width 192 = 3 x 64)
// `out` still goes to memory (the weight-gradient pass reads it) but is not read back: the separate projection launch, its
// 72 KB weight staging and its pass over `out` are gone.
//
// One 768-thread workgroup per (image, token range): waves 4 h .. 4 h + 3 are the four waves of lara_x_kernel for head h --
// the SAME body (ea_lara_x_body.h), so out, lseZ / tmean and the merged kv / lse_k / cst / lse_t come out bit for bit --
// with the three heads' landmark rows side by side in LDS (3 x 24.75 KB at C <= 64).  After quad_transpose_pack a lane holds
// 16 channels of one head of one token as two 16-byte pieces; they go to memory and to a [3][64][64] exchange tile in LDS
// (24 KB, double-buffered: one barrier per 64-token step).  Wave w then forms y[64 tokens][16 w .. 16 w + 15]: its 16 rows of
// W_proj are six 16-byte A fragments per lane, loaded straight from the [192,192] 16-bit image ea_linear takes, and held in
// registers for the whole range.  The k-slots, the order of the six accumulations and the rounding of the bias are lin_kernel's:
// y has the bits ea_linear[192->192] gives on the same `out`.
#include "ea_lara_x_body.h"

namespace ea {

template <typename E, int NCT, int MIS>
__global__ __launch_bounds__(768, 1) void lara_xp_kernel(const LaraP p, const LaraXpP xp) {
  lara_x_body<E, 64, NCT, LX_FWDM, MIS, true>(p, xp);
}

size_t lara_xp_lds(int NCT) { return (size_t)3 * lara_xp_head_lds(NCT) + 2 * LARA_XP_XB + 192 * sizeof(float); }

template <typename E, int NCT, int MIS>
static int launch_xp1(const LaraP& p, const LaraXpP& xp, hipStream_t st) {
  const size_t lds = lara_xp_lds(NCT);
  if (const int e = ea_lds_limit(&lara_xp_kernel<E, NCT, MIS>, lds)) return e;
  const dim3 grid((unsigned)(p.B * p.nsplit)), block(768);
  hipLaunchKernelGGL((lara_xp_kernel<E, NCT, MIS>), grid, block, lds, st, p, xp);
  return (int)hipGetLastError();
}

template <typename E, int NCT>
static int launch_xp(const LaraP& p, const LaraXpP& xp, hipStream_t st) {
  if (p.mis == MIS_OPT) return launch_xp1<E, NCT, MIS_OPT>(p, xp, st);
  if (p.mis == MIS_BIASED) return launch_xp1<E, NCT, MIS_BIASED>(p, xp, st);
  return launch_xp1<E, NCT, MIS_BH>(p, xp, st);
}

// the geometries the kernel takes (everything else keeps the two launches)
bool lara_xp_supported(int H, int D, int C, int S) { return H == 3 && D == 64 && C >= 1 && C <= 64 && S >= 1 && S <= 4; }

int lara_xp_dispatch(const LaraP& p0, const LaraXpP& xp, int dtype, hipStream_t st) {
  if (!lara_xp_supported(p0.H, p0.D, p0.C, p0.m_S)) return EA_E_UNSUPPORTED;
  LaraP p = p0;
  p.prof = nullptr;
  // one workgroup per CU holds all of its LDS: about one (image, token range) unit per CU, ranges whole 64-token steps
  const int maxblk = (p.N + 63) / 64;
  int nblk = (ea_device_cus() + p.B - 1) / p.B;
  if (nblk > maxblk) nblk = maxblk;
  if (nblk < 1) nblk = 1;
  int tpb = (p.N + nblk - 1) / nblk;
  tpb = (tpb + 63) / 64 * 64;
  p.tok_per_block = tpb;
  p.nsplit = (p.N + tpb - 1) / tpb;
  if (dtype == EA_BF16) return p.NCT <= 2 ? launch_xp<BF16, 2>(p, xp, st) : launch_xp<BF16, 4>(p, xp, st);
  if (dtype == EA_F16) return p.NCT <= 2 ? launch_xp<F16, 2>(p, xp, st) : launch_xp<F16, 4>(p, xp, st);
  return EA_E_UNSUPPORTED;
}

}  // namespace ea
