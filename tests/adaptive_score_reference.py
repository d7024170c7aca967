"""Host reference of adaptive-softmax scoring (ea_adaptive_route, ea_adaptive_score, C ABI 33): numpy, fp64, on the CPU.

  route(targets, cutoffs)   -> (head_target int64 [M], rows: one ascending int32 list per tail, count int32 [n]); cutoffs =
                            [c0, .., c_n = V].  head_target: t in the head, c0 + i for tail i, -1 outside [0, V).
  score(x, head, projs, tables, cutoffs, targets, h=None, round16=None)
                            -> dict(logp_head, logp_tail, logp [M] fp64, band [M] (-1: head or no band), head_rows [M, c0 + n],
                            tail_rows: per row the fp64 tail logits or None, h: per row the width-d_i row used or None).
                            Row m: vocab_score_reference.score of x[m] head^T at head_target[m]; in tail i also of h_m table_i^T
                            at t - c_i, h_m = h[i][j] where given (the kernel's OWN 16-bit h_i, j the row's place in rows[i]),
                            else round16(x[m] proj_i^T); logp = logp_head + logp_tail.  A target outside [0, V): NaN.
  ulp16(v, dtype)           one unit in the last place of the 16-bit type at |v| (bfloat16: 8 bits of precision; float16: 11,
                            subnormal below 2^-14).
  tol_h(bound, h64, dtype)  what a stored h_i entry may differ from the fp64 product of the rounded operands.
  tol_logp(bound, row, lse) what a pass's log-probability may differ from the fp64 one on the same operands.

The tolerances are assembled from functions the project already derives and tests; no constant is new.
  * decoder_vocab_operands.bound(xh, w)[m] = (K + 8) 2^-24 max_v sum_k |x_k w_vk| bounds the error of any fp32 sum of the K
    exact products of a logit of row m, in any order.
  * h_i: the fp32 sum is within `bound` of the fp64 product and is then rounded ONCE to the 16-bit type, to nearest: at most
    half a unit in the last place -- a whole unit is allowed, which also covers a value that `bound` carries across a
    binade.                                                                            tol_h = bound + ulp16(h64)
  * a pass's logp = fl(tlogit - lse).  vocab_score_reference.tol bounds |lse - lse64| with lse64 taken on the logits the
    kernel formed (its derivation: that file), and covers the rounding of the final operations at the size of lse; the
    target's logit is within `bound` of its fp64 value.                                tol_logp = bound + tol(row, lse64)
    The bound is a worst case over signs (it is hundreds of times the observed error of a sum), which is what leaves room
    for the shift of lse under the logits' own errors, itself at most the largest of them and in practice far below it.
  * the final value is one fp32 addition of the two passes' results: the two tolerances summed, and the addition's rounding,
    2^-24 |logp|, is inside vocab_score_reference.tol's last term (taken at max(1, |lse|) for each pass)."""
import math

import numpy as np

import vocab_score_reference as vref


def route(targets, cutoffs):
    t = np.asarray(targets, dtype=np.int64).reshape(-1)
    c0, V, n = int(cutoffs[0]), int(cutoffs[-1]), len(cutoffs) - 1
    head = np.full(t.shape, -1, dtype=np.int64)
    inside = (t >= 0) & (t < V)
    head[inside & (t < c0)] = t[inside & (t < c0)]
    rows = []
    for i in range(n):
        mask = (t >= int(cutoffs[i])) & (t < int(cutoffs[i + 1]))
        head[mask] = c0 + i
        rows.append(np.nonzero(mask)[0].astype(np.int32))          # (ascending)
    return head, rows, np.array([r.size for r in rows], dtype=np.int32)


def band_of(t, cutoffs):
    """-1 for the head and for a target outside [0, V), else the tail."""
    for i in range(len(cutoffs) - 1):
        if int(cutoffs[i]) <= t < int(cutoffs[i + 1]):
            return i
    return -1


def score(x, head, projs, tables, cutoffs, targets, h=None, round16=None):
    x = np.asarray(x, dtype=np.float64)
    head = np.asarray(head, dtype=np.float64)
    t = np.asarray(targets, dtype=np.int64).reshape(-1)
    M = x.shape[0]
    ht, rows, _ = route(t, cutoffs)
    place = {int(m): (i, j) for i, r in enumerate(rows) for j, m in enumerate(r)}
    head_rows = x @ head.T
    out = dict(logp_head=np.zeros(M), logp_tail=np.zeros(M), logp=np.zeros(M), band=np.full(M, -1), head_rows=head_rows,
               tail_rows=[None] * M, h=[None] * M)
    for m in range(M):
        out["logp_head"][m] = vref.score(head_rows[m], int(ht[m]))[3]
        if m in place:
            i, j = place[m]
            if h is not None:
                hm = np.asarray(h[i][j], dtype=np.float64)
            else:
                hm = x[m] @ np.asarray(projs[i], dtype=np.float64).T
                hm = hm if round16 is None else np.asarray(round16(hm), dtype=np.float64)
            row = hm @ np.asarray(tables[i], dtype=np.float64).T
            out["band"][m], out["tail_rows"][m], out["h"][m] = i, row, hm
            out["logp_tail"][m] = vref.score(row, int(t[m]) - int(cutoffs[i]))[3]
    out["logp"] = out["logp_head"] + out["logp_tail"]
    return out


def ulp16(v, dtype):
    bits, emin = {"bfloat16": (8, -126), "float16": (11, -14)}[str(dtype).replace("torch.", "")]
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** emin)))
    return 2.0 ** (e - (bits - 1))


def tol_h(bound, h64, dtype):
    return np.asarray(bound, dtype=np.float64) + ulp16(h64, dtype)


def tol_logp(bound, row, lse64):
    return float(bound) + vref.tol(row, lse64)
