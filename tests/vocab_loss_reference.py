"""Host reference of the vocabulary cross-entropy's logit gradient (ea_vocab_nll_grad, C ABI 38): numpy, fp64, on the CPU.

  grad(a, lse, d, targets, v0=0, V=None)   -> G [M, Vc] in fp64 from logits a [M, Vc] (the columns v0 .. v0 + Vc - 1 of the
                                           table), lse [M], d [M], targets [M]:
                                               G[m, c] = d[m] * ((v0 + c == targets[m]) - exp(a[m, c] - lse[m]))
                                           a row with d[m] == 0 is zeros whatever a and lse hold; a target outside [0, V) (V
                                           given) matches no column.
  bound(a, lse, d, targets, dtype, v0=0)   -> [M, Vc] fp64: what the GPU test allows between the kernel's 16-bit G and `grad`
                                           evaluated on the kernel's OWN stored fp32 logits, its own fp32 lse and the fp32 d.
  unit(dtype), floor(dtype)                the unit roundoff and the absolute floor of a 16-bit type, as used below.

The bound, from the kernel's operations (csrc/ea_vocab_score_tile.h, VS_EPI_GRAD), every one in fp32 rounded to nearest, with
u = 2^-24, h = (v == target) in {0, 1}, p = exp(a - lse):

  * s = fl(a - lse): relative u on |a - lse|, so |s - (a - lse)| <= u |a - lse|, and exp(s) = p exp(s - (a - lse)): to first
    order a relative error of u |a - lse| on p.
  * expf at 1 ulp = 2 u (the convention of tests/vocab_score_reference.py): p^ = p (1 + e), |e| <= (|a - lse| + 2) u.
  * the subtraction h - p^ and the product with d, u each: relative 2 u on |h - p|.
  Before the rounding to E the value is off by at most
      e32 = |d| (p (|a - lse| + 2) + 2 |h - p|) u (1 + 2^-10),         the last factor for what the first order leaves out,
  * one rounding to E at unit roundoff uE = 2^-8 (bf16) or 2^-11 (fp16), on a value of size at most |G| + e32;
  * the floor: a result below E's normal range is rounded to a multiple of its smallest subnormal -- fp16: at most 2^-25 off;
    bf16 (fp32's exponent range): 2^-134 -- and an fp32 intermediate below 2^-126 (expf of a very negative difference, its
    product with d) may be flushed: |d| 2^-126 and 2^-126.

      bound = e32 + uE (|G| + e32) + floor(E) + (|d| + 1) 2^-126

A function of (a, lse, d, dtype) and of where the target is; no constant is chosen.  It is dominated by uE |G|: a kernel that
dropped the target term, used a 16-bit lse or rounded twice is outside it on the first element it touches."""
import numpy as np
import torch

U = 2.0 ** -24


def unit(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def floor(dtype):
    return {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}[dtype]


def _parts(a, lse, d, targets, v0, V):
    a = np.asarray(a, dtype=np.float64)
    lse = np.asarray(lse, dtype=np.float64).reshape(-1, 1)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 1)
    t = np.asarray(targets, dtype=np.int64).reshape(-1, 1)
    cols = v0 + np.arange(a.shape[1], dtype=np.int64).reshape(1, -1)
    hit = cols == t
    if V is not None:
        hit = hit & (t >= 0) & (t < V)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = a - lse
        p = np.exp(diff)
    return diff, p, hit.astype(np.float64), d


def grad(a, lse, d, targets, v0=0, V=None):
    diff, p, h, d = _parts(a, lse, d, targets, v0, V)
    with np.errstate(invalid="ignore"):
        g = d * (h - p)
    return np.where(d == 0.0, 0.0, g)


def bound(a, lse, d, targets, dtype, v0=0, V=None):
    diff, p, h, d = _parts(a, lse, d, targets, v0, V)
    with np.errstate(invalid="ignore"):
        e32 = np.abs(d) * (p * (np.abs(diff) + 2.0) + 2.0 * np.abs(h - p)) * U * (1.0 + 2.0 ** -10)
        g = np.abs(d * (h - p))
        b = e32 + unit(dtype) * (g + e32) + floor(dtype) + (np.abs(d) + 1.0) * 2.0 ** -126
    return np.where(d == 0.0, 0.0, b)
