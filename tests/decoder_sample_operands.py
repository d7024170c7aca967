"""Operands of the sampled-pick tests (tests/test_gpu_decoder_sample.py runs them on the kernel, tests/test_decoder_sample_cpu.py
checks on the host that they are what they claim to be).  CPU tensors, built on decoder_vocab_operands.

  SHAPES: the six small shapes of decoder_vocab_operands.SHAPES; LM: (1, 1024, 32768), used once.
  one_tile(shape, wdtype, k) -> x32, w, cols    the k best logits of every row lie in ONE 16-column tile (k <= 16, k <= V)
  spread(shape, wdtype, k)   -> x32, w, cols    one of the k best in each of k different tiles, the tail tile among them
                                                (None where the table has fewer than k tiles)
      Both as decoder_vocab_operands.tie builds its pair: one table row r gets a positive product 4 sqrt(K) |r| with every row
      of x, and 4 r (1 + i / 64), i = 1 .. k, is written to `cols`.  STATED PRECONDITION, x rounded to wdtype, in fp64: every
      logit of `cols` > every other logit of its row + 2 bound.
  period3(shape, wdtype)     -> x32, w          w[v] = 4 w0[v mod 3]: every logit occurs at every third column, and the
                                                lowest columns must win"""
import torch

import decoder_vocab_operands as ops

SHAPES = ops.SHAPES[:6]
LM = ops.SHAPES[6]
KS = [1, 5, 16, 40, 64]
TEMPERATURES = [0.7, 1.0]
TOP_PS = [1.0, 0.9]
SEED = 0x9E3779B97F4A7C15                                    # (both words of the key in use)
DRAWS = 64


def _lifted(shape, wdtype, cols):
    M, K, V = shape
    x32, w = ops.operands(shape, wdtype, 0)
    j = next(v for v in range(V) if v not in cols)
    r = w[j].double()
    u = r / r.norm()
    x = x32.double()
    x = x - (x @ u).unsqueeze(1) * u + 4.0 * K ** 0.5 * u       # every row: x . r = 4 sqrt(K) |r| > 0
    x32 = x.float()
    x32[:, 0] = x32[:, 0].abs() + 1.0
    for i, v in enumerate(cols):
        w[v] = (4.0 * r * (1.0 + (i + 1) / 64.0)).to(wdtype)
    return x32, w, cols


def one_tile(shape, wdtype, k):
    V = shape[2]
    if k > 16 or k >= V:
        return None
    tile = ((V - 1) // 16) // 2                                 # a middle tile (the only one of a 16-column table)
    live = min(16, V - 16 * tile)
    if k > live:
        return None
    return _lifted(shape, wdtype, [16 * tile + (3 * i) % live for i in range(k)] if live == 16 else
                   [16 * tile + i for i in range(k)])


def spread(shape, wdtype, k):
    V = shape[2]
    NB = (V - 1) // 16 + 1
    if NB < k or k >= V:
        return None
    tiles = sorted({(i * (NB - 1)) // max(1, k - 1) for i in range(k)}) if k > 1 else [NB - 1]
    if len(tiles) != k:
        return None
    cols = [16 * t + (5 * i) % min(16, V - 16 * t) for i, t in enumerate(tiles)]
    return _lifted(shape, wdtype, cols)


def lifted_margin(x32, w, cols):
    """min over rows of (the smallest logit of `cols` - the largest other logit - 2 bound), fp64, x rounded to w's type."""
    xh = x32.to(w.dtype)
    L = xh.double() @ w.double().t()
    inside = L[:, cols].min(1).values
    others = L.clone()
    others[:, cols] = float("-inf")
    return (inside - others.max(1).values - 2.0 * ops.bound(xh, w)).min().item()


def period3(shape, wdtype):
    x32, w = ops.operands(shape, wdtype, 0)
    V = shape[2]
    w = (4.0 * w[:3].float()).to(wdtype)[torch.arange(V) % 3]
    return x32, w.contiguous()
