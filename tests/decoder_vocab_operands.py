"""Operands of the vocabulary-pick tests (tests/test_gpu_decoder_vocab.py runs them on the kernel, tests/test_decoder_vocab_cpu.py
checks on the host that they are what they claim to be).  Everything here is CPU tensors, seeded by (shape, type, seed).

  operands(shape, wdtype, seed) -> x32 [M, K] fp32, w [V, K] of wdtype
      x ~ N(0, 1), w ~ N(0, 1 / K); x[:, 0] > 1/2 after rounding to wdtype, so that a table row (+inf, 0, 0, ..) gives a
      +inf logit in every row.
  bound(xh, w) -> [M] fp64: (K + 8) 2^-24 max_v sum_k |x_k w_vk|, the worst-case error of K + 8 fp32 additions in any order
      (products of two bf16 or two fp16 values are exact in fp32).
  tie(shape, wdtype, seed, case) -> x32, w, a, b  (or None where the shape has no such pair)
      One table row r = w[j] is given a positive product with every row of x (x gets 4 sqrt(K) r / |r| added to what it has
      across r), and r times 4 -- exact in both types -- is written to the indices a < b.  STATED PRECONDITION, for x rounded to
      wdtype, in fp64: logit[m, a] = logit[m, b] > logit[m, v] + 2 bound[m] for every other v and every row m.
      Cases: "one_tile" (a, b in one 16-column tile), "two_workgroups" (different tiles), "tail" (b in the last tile),
      "ends" (a = 0, b = V - 1).
  nan_rows(shape, wdtype, seed, two) -> x32, w, rows  (or None): table rows `rows` are NaN; 0 < rows[0] (< rows[1]) < V - 1."""
import functools

import torch

# (M, K, V): one k-step and one tile; idle waves and a tail tile of 8 columns; several hundred partials per row and a tail;
# a second row tile holding one row; a second pass over K; the row bound with V % 16 = 8; the LM shapes
SHAPES = [(1, 32, 16), (3, 288, 40), (16, 256, 4808), (17, 256, 64), (33, 1056, 48), (64, 1024, 1000),
          (1, 1024, 32768), (8, 1024, 32768)]
LM = SHAPES[6:]
W_DTYPES = [torch.bfloat16, torch.float16]
TIE_CASES = ["one_tile", "two_workgroups", "tail", "ends"]


def seeds(shape):
    """The seeds the tests use for a shape (the LM shapes: one)."""
    return (0,) if shape in LM else (0, 1)


def _gen(shape, wdtype, seed):
    M, K, V = shape
    return torch.Generator().manual_seed(((M * 4099 + K) * 8191 + V) * 4 + 2 * seed + (wdtype == torch.float16))


@functools.lru_cache(maxsize=4)
def _drawn(shape, wdtype, seed):
    M, K, V = shape
    g = _gen(shape, wdtype, seed)
    x32 = torch.randn(M, K, generator=g)
    x32[:, 0] = x32[:, 0].abs() + 1.0
    w = (torch.randn(V, K, generator=g) / K ** 0.5).to(wdtype)
    return x32, w


def operands(shape, wdtype, seed=0):
    x32, w = _drawn(shape, wdtype, seed)
    return x32.clone(), w.clone()


def bound(xh, w):
    K = xh.shape[1]
    return (K + 8) * 2.0 ** -24 * (xh.double().abs() @ w.double().abs().t()).max(1).values


def tie_indices(V, case):
    """(a, b) with a < b < V, or None where V has no such pair."""
    last = (V - 1) // 16 * 16                                 # first column of the last tile
    if case == "one_tile":
        a, b = (1, min(14, V - 1))
    elif case == "two_workgroups":
        a, b = (3, 16 * max(1, (V // 16) // 2) + 5)
    elif case == "tail":
        a, b = (5, last + (V - 1 - last) // 2)
    elif case == "ends":
        a, b = (0, V - 1)
    else:
        raise ValueError(case)
    if not 0 <= a < b < V or (case in ("two_workgroups", "tail") and a // 16 == b // 16) or (case == "tail" and b < last):
        return None
    return a, b


def tie(shape, wdtype, seed, case):
    M, K, V = shape
    ab = tie_indices(V, case)
    if ab is None or V < 4:
        return None
    a, b = ab
    x32, w = operands(shape, wdtype, seed)
    j = next(v for v in range(V) if v not in (a, b))
    r = w[j].double()
    u = r / r.norm()
    x = x32.double()
    x = x - (x @ u).unsqueeze(1) * u + 4.0 * K ** 0.5 * u       # every row: x . r = 4 sqrt(K) |r| > 0
    x32 = x.float()
    x32[:, 0] = x32[:, 0].abs() + 1.0
    w[a] = w[b] = (4.0 * r).to(wdtype)
    return x32, w, a, b


def tie_margin(x32, w, a, b):
    """min over rows of (logit[m, a] - max other logit - 2 bound[m]) in fp64, x rounded to w's type; and whether the two
    columns are equal in fp64 -> (margin, equal)."""
    xh = x32.to(w.dtype)
    L = xh.double() @ w.double().t()
    others = L.clone()
    others[:, [a, b]] = float("-inf")
    margin = (L[:, a] - others.max(1).values - 2.0 * bound(xh, w)).min().item()
    return margin, bool((L[:, a] == L[:, b]).all())


def nan_rows(shape, wdtype, seed, two):
    M, K, V = shape
    rows = [V // 3, V - 2] if two else [V // 2]
    if not all(0 < v < V - 1 for v in rows) or (two and not rows[0] < rows[1]):
        return None
    x32, w = operands(shape, wdtype, seed)
    for v in rows:
        w[v] = float("nan")
    return x32, w, rows
