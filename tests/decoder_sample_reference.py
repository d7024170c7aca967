"""Host reference of the sampled token pick (ea_ceva_sdecode_vocab_sample, include/ea_hip.h, C ABI 27), numpy on the CPU:
tests/test_decoder_sample_cpu.py checks it against known answers, tests/test_gpu_decoder_sample.py checks the kernel against it.

  philox4x32_10(counter, key) -> [.., 4] uint32          Salmon et al., SC 2011; counter [.., 4], key [.., 2], vectorised
  uniform(seed, ctr, sid)     -> float32                  u = ((word 0 >> 8) + 0.5) 2^-24 of the draw (seed, ctr, sid), formed in
                                                          fp32 as the kernel forms it (25-bit sums round to nearest even)
  topk(row, k)                -> int64 [min(k, V)]        the columns of the k best logits of one fp32 row under the total
                                                          order: NaN above every number, the larger value first, equal values
                                                          (+0 and -0 too) by the lower column
  cumulative(sel_val, T)      -> float64 [k']             c_j = sum_{i <= j} exp((val_i - val_0) / T), in fp64
  eps(c)                      -> k' 2^-20 c_{k'-1}        the absolute error a kernel's fp32 c_j may have (the issue's bound:
                                                          (val_j - val_0) / T contributes at most 2^-22 / e per term, expf at
                                                          2 ulp and k' fp32 additions 3 * 2^-24 per term, all relative to
                                                          w_0 = 1 <= c: under k' 2^-21; eps is twice that)
  admissible_kept(c, top_p)   -> the n the nucleus rule allows when every c_j may move by eps
  admissible_js(c, kept, u)   -> the j with c_{j-1} - eps <= u c_{kept-1} < c_j + eps, j < kept (c_{-1} = 0)
  admissible_mask(c, kept, u) -> the same for many draws of one row at once, as a boolean matrix [draws, k']"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & _MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & _MASK for i in range(2)]
    c = list(np.broadcast_arrays(*c, *k)[:4])
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
    return np.stack(c, -1).astype(np.uint32)


def uniform(seed, ctr, sid):
    seed = int(seed)
    ctr = np.asarray(ctr, dtype=np.int64).astype(np.uint64)
    sid = np.asarray(sid, dtype=np.int64).astype(np.uint64) & _MASK
    ctr, sid = np.broadcast_arrays(ctr, sid)
    counter = np.stack([ctr & _MASK, ctr >> np.uint64(32), sid, np.zeros_like(ctr)], -1)
    word = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))[..., 0]
    return ((word >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def topk(row, k):
    row = np.asarray(row, dtype=np.float32)
    nan = np.isnan(row)
    value = np.where(nan, np.float32(0), row) + np.float32(0)           # (-0 + 0 = +0: the two compare equal anyway)
    order = np.lexsort((np.arange(row.size), -value.astype(np.float64), ~nan))     # the last key decides first
    return order[:min(int(k), row.size)]


def cumulative(sel_val, temperature):
    v = np.asarray(sel_val, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.cumsum(np.exp((v - v[0]) / float(temperature)))


def eps(c):
    return len(c) * 2.0 ** -20 * c[-1]


def admissible_kept(c, top_p):
    """n is allowed iff some C' within eps of c_{k'-1} has c_{n-2} - eps < top_p C' <= c_{n-1} + eps; n = k' needs the left
    half only (c'_{k'-1} is C' itself, and top_p <= 1)."""
    e, k, lo, hi = eps(c), len(c), top_p * (c[-1] - eps(c)), top_p * (c[-1] + eps(c))
    return [n for n in range(1, k + 1)
            if (n == 1 or c[n - 2] - e < hi) and (n == k or c[n - 1] + e >= lo)]


def admissible_mask(c, kept, u):
    """kept [n] (each >= 1), u [n] -> bool [n, k']: entry (i, j) says that j is admissible for draw i."""
    kept, u = np.asarray(kept, dtype=np.int64).reshape(-1), np.asarray(u, dtype=np.float64).reshape(-1)
    e, r = eps(c), (u * c[kept - 1]).reshape(-1, 1)
    lo = np.concatenate([[0.0], c[:-1]]) - e
    return (lo.reshape(1, -1) <= r) & (r < (c + e).reshape(1, -1)) & (np.arange(len(c)).reshape(1, -1) < kept.reshape(-1, 1))


def admissible_js(c, kept, u):
    return np.nonzero(admissible_mask(c, [kept], [u])[0])[0].tolist()
