"""Host reference of the greedy pick from the adaptive head (ea_adaptive_pick, C ABI 34): numpy, fp64, on the CPU.

  constants()               (SPAN, MAX_K) as include/ea_hip.h defines them (EA_ADAPTIVE_PICK_SPAN / _MAX_K).
  ws_layout(M, cutoffs, dims)
                            the documented workspace layout -> dict of byte offsets (cls, h, best<b>, lse<b>, tlogit<b>,
                            shifted<i>, cls_cand, cls_sum, cand<b>, sum<b>), `parts` (partials per row and band), `D`, `total`.
  pick(x, head, projs, tables, cutoffs, targets=None, h=None, round16=None)
                            -> dict(token int64 [M], logp [M], joint [M, V] (the whole log-probability row: fairseq's
                            get_log_prob(x, None)), head_rows [M, c0 + n], tail_rows [n][M, V_i], h [n][M, d_i], lse [n + 1][M]
                            (band 0: over ALL c0 + n head columns), best [n + 1][M] (the largest RAW logit of the band; band
                            0: of the words)).  h: the kernel's OWN 16-bit h_i where given, else round16(x proj_i^T) (round16
                            None: unrounded).  token is the first index of the largest joint score (np.argmax: the lowest
                            of equals); logp = joint[m, targets[m]] (a target outside [0, V): NaN), joint[m, token[m]] without
                            targets.
  decided(joint, tol)       -> (token [M], gap [M], decided [M] bool): the fp64 argmax, the gap between the best and the
                            second-best joint score, and gap > 2 tol.

Tolerances are adaptive_score_reference's (tol_h, tol_logp) on decoder_vocab_operands.bound: no constant is new.  A joint
score is the head's part (one logit, lse_h) plus, in a tail, the tail's part (one logit, lse_i): its error is at most
tol_logp(head) + tol_logp(tail i).  Two scores of one row differ from their fp64 values by at most that sum each, so with
tol[m] = tol_logp(head) + max_i tol_logp(tail i) a gap above 2 tol[m] decides the token, and below it the token's fp64 score
is within 2 tol[m] of the best."""
import os
import re

import numpy as np

import decoder_logprob_reference as lref

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ea_hip.h")


def constants():
    text = open(_HEADER).read()
    return tuple(int(re.search(r"#define EA_ADAPTIVE_PICK_%s (\d+)" % n, text).group(1)) for n in ("SPAN", "MAX_K"))


def r16(n):
    return (n + 15) // 16 * 16


def ws_layout(M, cutoffs, dims):
    SPAN, MAX_K = constants()
    n, at, lay = len(dims), 0, {}

    def take(name, nbytes):
        nonlocal at
        lay[name] = at
        at += r16(nbytes)
    D = sum(dims)
    take("cls", 4 * M * n), take("h", 2 * M * D)
    for b in range(n + 1):
        take("best%d" % b, 8 * M), take("lse%d" % b, 4 * M), take("tlogit%d" % b, 4 * M)
    for i, d in enumerate(dims):
        if d > MAX_K:
            take("shifted%d" % i, 8 * M)
    take("cls_cand", 8 * M), take("cls_sum", 4 * M)
    parts = []
    for b in range(n + 1):
        Vb = cutoffs[0] if b == 0 else cutoffs[b] - cutoffs[b - 1]
        P = -(-Vb // SPAN) if b and dims[b - 1] <= MAX_K else -(-Vb // 16)
        parts.append(P)
        take("cand%d" % b, 8 * M * P), take("sum%d" % b, 4 * M * P)
    lay["parts"], lay["D"], lay["total"] = parts, D, at
    return lay


def pick(x, head, projs, tables, cutoffs, targets=None, h=None, round16=None):
    x = np.asarray(x, dtype=np.float64)
    head = np.asarray(head, dtype=np.float64)
    M, c0, n, V = x.shape[0], int(cutoffs[0]), len(cutoffs) - 1, int(cutoffs[-1])
    head_rows = x @ head.T
    lse = [np.array([lref.lse(r) for r in head_rows])]
    best = [head_rows[:, :c0].max(1)]
    with np.errstate(invalid="ignore"):
        parts = [head_rows[:, :c0] - lse[0][:, None]]
        hs, tail_rows = [], []
        for i in range(n):
            if h is not None:
                hi = np.asarray(h[i], dtype=np.float64)
            else:
                hi = x @ np.asarray(projs[i], dtype=np.float64).T
                hi = hi if round16 is None else np.asarray(round16(hi), dtype=np.float64)
            rows = hi @ np.asarray(tables[i], dtype=np.float64).T
            hs.append(hi), tail_rows.append(rows)
            lse.append(np.array([lref.lse(r) for r in rows]))
            best.append(rows.max(1))
            parts.append((head_rows[:, c0 + i] - lse[0])[:, None] + (rows - lse[i + 1][:, None]))
    joint = np.concatenate(parts, 1)
    assert joint.shape == (M, V)
    token = joint.argmax(1).astype(np.int64)
    if targets is None:
        logp = joint[np.arange(M), token]
    else:
        t = np.asarray(targets, dtype=np.int64).reshape(-1)
        inside = (t >= 0) & (t < V)
        logp = np.where(inside, joint[np.arange(M), np.where(inside, t, 0)], np.nan)
    return dict(token=token, logp=logp, joint=joint, head_rows=head_rows, tail_rows=tail_rows, h=hs, lse=lse, best=best)


def decided(joint, tol):
    top2 = np.sort(joint, axis=1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    return joint.argmax(1), gap, gap > 2.0 * np.asarray(tol)
