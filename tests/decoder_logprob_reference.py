"""Host reference of the token log-probabilities (ea_ceva_sdecode_vocab_logprob, C ABI 28): numpy, fp64, on the CPU.

  lse(row)             the log-sum-exp of a row of stored fp32 logits, in fp64, by the kernel's case rule on the row's top
                       (NaN above every number, as the pick orders them): top NaN -> NaN; +inf -> +inf; -inf (every logit is
                       -inf) -> -inf; else top + log(sum_v exp(logit_v - top)), a -inf logit adding nothing.
  logp(row, target)    logit[target] - lse(row) in fp64; a target outside [0, V): NaN.
  spread(row)          D: the largest minus the smallest finite logit of the row (0 where there is none).
  tol(row, lse64)      (2 D + 40 + NB / 512) 2^-24 + 2^-22 max(1, |lse64|), NB = ceil(V / 16): what the GPU test allows between
                       the kernel's fp32 lse and lse(row).  One rounding of each logit - m_t and m_t - top (at most D 2^-24
                       relative in the exponential, twice), expf and logf at 1 ulp, at most 4 + NB / 512 + 6 + 8 additions of
                       positive terms, and the final add, which rounds at the size of lse."""
import numpy as np


def lse(row):
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    if np.isnan(row).any():
        return float("nan")
    top = row.max()
    if np.isinf(top):
        return float(top)
    return float(top + np.log(np.exp(row - top).sum()))


def logp(row, target):
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    if not 0 <= int(target) < row.size:
        return float("nan")
    with np.errstate(invalid="ignore"):
        return float(row[int(target)] - lse(row))


def spread(row):
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    fin = row[np.isfinite(row)]
    return float(fin.max() - fin.min()) if fin.size else 0.0


def tol(row, lse64):
    V = np.asarray(row).size
    NB = (V + 15) // 16
    size = max(1.0, abs(lse64)) if np.isfinite(lse64) else 1.0
    return (2.0 * spread(row) + 40.0 + NB / 512.0) * 2.0 ** -24 + 2.0 ** -22 * size
