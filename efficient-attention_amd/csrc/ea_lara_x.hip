// ea_lara_x.hip -- LARA passes in the token-column layout (see ea_lara.h).
//
//   LX_FWD   out_n = sum_c W[c,n] kv_c,  W = softmax_c(log alpha + s w_c.q_n + lse_k - log_prop)
//            (lara.py:201,221-246; the -s|q_n|^2/2 term of log_proj_q is constant in c and cancels)
//   LX_BWDQ  recomputes W, forms dZ / d(alpha) / dt and writes the part of dq that needs no
//            sequence-wide sum, plus the per-token scalars (lse_Z, mean_c t, dout.out, sum_c dalpha)
//            the token-row pass needs
//   LX_BWDK  dk, dv from Pk = softmax_m(log_proj_k) recomputed with the saved lse_k
//   LX_QCORR dq -= s sum_c t[c,n] (u_c qbar_c): the softmax-over-sequence correction of t
// One 16-token tile per wave step: token rows come straight from global memory as MFMA B
// operands; the landmark matrices live in LDS (row-major for the score MFMAs, transposed for
// the contraction over c); each lane ends up owning D/4 contiguous channels of one token.
#include "ea_lara_x_body.h"

namespace ea {


size_t lara_x_lds(int D, int NCT) {
  const int Cp = NCT * 16;
  return (size_t)3 * Cp * D * 2 + (size_t)3 * Cp * sizeof(float);
}

template <typename E, int D, int NCT>
static int launch_x(int mode, const LaraP& p, hipStream_t st) {
  const size_t lds = lara_x_lds(D, NCT);
  const dim3 grid((unsigned)(p.B * p.H * p.nsplit)), block(256);
#define EA_LXM(M, S)                                                                              \
  do {                                                                                            \
    if (const int e = ea_lds_limit(&lara_x_kernel<E, D, NCT, M, S>, lds)) return e;               \
    hipLaunchKernelGGL((lara_x_kernel<E, D, NCT, M, S>), grid, block, lds, st, p);                \
  } while (0)
#define EA_LX(M) EA_LXM(M, -1)
  switch (mode) {
    case LX_FWD:
      if (p.mis == MIS_OPT) EA_LXM(LX_FWD, MIS_OPT);
      else if (p.mis == MIS_BIASED) EA_LXM(LX_FWD, MIS_BIASED);
      else EA_LXM(LX_FWD, MIS_BH);
      break;
    case LX_FWDM:
      if constexpr (NCT <= 4) {
        if (p.mis == MIS_OPT) EA_LXM(LX_FWDM, MIS_OPT);
        else if (p.mis == MIS_BIASED) EA_LXM(LX_FWDM, MIS_BIASED);
        else EA_LXM(LX_FWDM, MIS_BH);
      } else {
        return EA_E_UNSUPPORTED;
      }
      break;
    case LX_BWDQ: EA_LX(LX_BWDQ); break;
    case LX_BWDK: EA_LX(LX_BWDK); break;
    case LX_QCORR: EA_LX(LX_QCORR); break;
    case LX_POUT: EA_LX(LX_POUT); break;
    case LX_PBWDQ: EA_LX(LX_PBWDQ); break;
    case LX_PBWDK: EA_LX(LX_PBWDK); break;
    default: return EA_E_BADARG;
  }
#undef EA_LX
#undef EA_LXM
  return (int)hipGetLastError();
}

template <typename E, int D>
static int launch_x_nct(int mode, const LaraP& p, hipStream_t st) {
  if (p.NCT <= 2) return launch_x<E, D, 2>(mode, p, st);
  if (p.NCT <= 4) return launch_x<E, D, 4>(mode, p, st);
  if (p.NCT <= 8) return launch_x<E, D, 8>(mode, p, st);
  return EA_E_UNSUPPORTED;
}

int lara_x_dispatch(int mode, const LaraP& p0, int dtype, hipStream_t st) {
  LaraP p = p0;
  p.prof = nullptr;
#ifdef EA_PROFILE
  ProfReport rep;
  p.prof = rep.arm(st, "lara_x", mode);
#endif
  if (dtype == EA_BF16) {
    if (p.D == 64) return launch_x_nct<BF16, 64>(mode, p, st);
    if (p.D == 32) return launch_x_nct<BF16, 32>(mode, p, st);
  } else if (dtype == EA_F16) {
    if (p.D == 64) return launch_x_nct<F16, 64>(mode, p, st);
    if (p.D == 32) return launch_x_nct<F16, 32>(mode, p, st);
  }
  return EA_E_UNSUPPORTED;
}

}  // namespace ea
