"""Host reference of the many-row vocabulary pass (ea_vocab_score, C ABI 30): numpy, fp64, on the CPU.

  constants()              (BM, BN, SL) as include/ea_hip.h defines them (EA_VOCAB_SCORE_BM / _BN / _SL): read from the header, so
                           that test shapes can be formed without the library; the GPU test checks the library's own answer.
  score(row, target=None)  -> (token, top, lse, logp) of one row of logits in fp64: token by torch.argmax's rule (the largest
                           value, the lowest index among equals; in a row with NaN the lowest NaN index), top = row[token],
                           lse by decoder_logprob_reference.lse's case rule, logp = row[target] - lse (a target outside [0, V):
                           NaN), top - lse without a target.
  tol(row, lse64)          what the GPU test allows between the kernel's fp32 lse and the fp64 log-sum-exp of the kernel's own
                           stored fp32 logits.

The tolerance, from the kernel's operation count (csrc/ea_vocab_score.hip).  u = 2^-24, the relative error of one fp32
operation rounded to nearest; nb = min(ceil(V / BN), SL / BN) column blocks per slice, NS = ceil(V / SL) slices, D the spread
of the row's finite logits.  The kernel forms S = sum_v exp(logit_v - top) and lse = top + logf(S); a -inf logit adds an exact
0.  The relative error of S, to first order:

  * exponents.  A term starts as expf(fl(logit - m)), m the running maximum of its lane at that block, and is then multiplied
    by expf(fl(m - m')) each time a maximum rises: in the lane, at the merge of the 16 lanes, of the wave pair and of the
    slices.  Each difference is rounded once, relative u, and the maximum only rises: the differences telescope to
    top - logit <= D, so all exponent errors of a term together are at most D u, and so is their effect on the term.   D
  * expf at 1 ulp = 2 u: the term's own, and one per rescale that changes it.  A factor is applied only where the maximum
    rose (equal maxima: the sum is kept as it is, no expf, no product): at most nb - 1 times in the lane, then once at each
    of the three merges.  Each such rescale is an expf and a product: 3 u.                                    2 + 3 (nb + 2)
  * additions of positive terms, each u, by the depth of the chain a term passes: two inside a block ((e0 + e1) + (e2 + e3)),
    one per block onto the running sum, four butterfly steps over the 16 lanes, one for the wave pair, one per slice in the
    second launch.                                                                                      2 + nb + 4 + 1 + NS
  That is (D + 4 nb + NS + 15) u, and it is the absolute error of log S.  Then logf at 1 ulp of its result, 0 <= log S <=
  log V: 2 u log V.  Then the final addition top + logf(S), rounded at the size of lse: u |lse|.

  tol = (D + 4 nb + NS + 15 + 2 log V) 2^-24 + 2^-24 max(1, |lse64|)

Nothing here compounds with V beyond nb <= SL / BN = 16 and NS: at V = 32768 the constant part is 116 u against the 256 u of
2^-16.  The GPU test requires tol <= 2^-16 max(1, |lse64|) on its shapes: a dropped column at V = 16 shifts lse by about
1 / 16, at V = 5096 by about 2e-4 = 13 * 2^-16."""
import math
import os
import re

import numpy as np

import decoder_logprob_reference as lp

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ea_hip.h")


def constants():
    text = open(_HEADER).read()
    return tuple(int(re.search(r"#define EA_VOCAB_SCORE_%s (\d+)" % n, text).group(1)) for n in ("BM", "BN", "SL"))


def score(row, target=None):
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    nan = np.isnan(row)
    token = int(np.argmax(nan)) if nan.any() else int(np.argmax(row))       # (np.argmax: the first of equals)
    top = float(row[token])
    lse = lp.lse(row)
    if target is None:
        tl = top
    else:
        tl = float(row[int(target)]) if 0 <= int(target) < row.size else float("nan")
    with np.errstate(invalid="ignore"):
        return token, top, lse, tl - lse


def tol(row, lse64):
    BM, BN, SL = constants()
    V = np.asarray(row).size
    nb = min(-(-V // BN), SL // BN)
    NS = -(-V // SL)
    size = max(1.0, abs(lse64)) if np.isfinite(lse64) else 1.0
    return (lp.spread(row) + 4.0 * nb + NS + 15.0 + 2.0 * math.log(V)) * 2.0 ** -24 + 2.0 ** -24 * size
