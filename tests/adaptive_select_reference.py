"""Host reference of the selection behind ea_adaptive_sample / ea_adaptive_beam (include/ea_hip.h, C ABI 35): numpy on the CPU.
tests/test_adaptive_sample_cpu.py checks it against hand-worked answers, tests/test_gpu_adaptive_sample.py checks the kernels
against it ON THE KERNELS' OWN NUMBERS: the stored band logits, cls and lse read out of the workspace.

  ws_layout(M, cutoffs, dims, W=0)    the documented workspace: adaptive_pick_reference.ws_layout's dict from byte 0, then
                                      logits<b>, tcand<i> (tails of the column-split kernel), list_idx, list_val and, W > 0,
                                      cand_idx, cand_score; `total`.
  band_sizes(cutoffs)                 [V_0, .., V_n]
  joint(band_logits, cls, lse)        -> [n + 1] fp32 [M, V_b]: the joint scores by the rule's fp32 operations, in its order:
                                      a word: a[v] - lse_h; a token of tail i: (a[c0 + i] - lse_h) + (b_i[u] - lse_i)
  select_row(band_rows, joint_rows, cutoffs, k)
                                      one row: per band the min(k, V_b) best RAW logits under decoder_sample_reference.topk's
                                      total order, then the min(k, V) best of their joint scores under the same order on
                                      (s, vocabulary index) -> (idx int64 [k'], val fp32 [k'])
  select(band_logits, cls, lse, cutoffs, k)
                                      every row -> (idx int64 [M, k'], val fp32 [M, k'], joint)
  beam_candidates(idx, val, score)    cand_score = score[m] + s_j, one fp32 addition
  eos_score(joint, cutoffs, eos)      the forced step's single candidate: fp32 [M]"""
import numpy as np

import adaptive_pick_reference as pref
import decoder_sample_reference as sref

F32 = np.float32
LIST = 64                                                # entries of a band's list in the workspace


def band_sizes(cutoffs):
    return [int(c - a) for a, c in zip([0] + list(cutoffs[:-1]), cutoffs)]


def ws_layout(M, cutoffs, dims, W=0):
    _, MAX_K = pref.constants()
    lay = pref.ws_layout(M, cutoffs, dims)
    at, n, sizes = lay["total"], len(dims), band_sizes(cutoffs)
    lay["pick_total"] = at

    def take(name, nbytes):
        nonlocal at
        lay[name] = at
        at += pref.r16(nbytes)
    for b, Vb in enumerate(sizes):
        take("logits%d" % b, 4 * M * Vb)
    for i, d in enumerate(dims):
        if d <= MAX_K:
            take("tcand%d" % i, 8 * M * -(-sizes[i + 1] // 16))
    take("list_idx", 4 * M * (n + 1) * LIST), take("list_val", 4 * M * (n + 1) * LIST)
    if W:
        take("cand_idx", 4 * M * 2 * W), take("cand_score", 4 * M * 2 * W)
    lay["total"] = at
    return lay


def joint(band_logits, cls, lse):
    """band_logits [n + 1] fp32 [M, V_b]; cls fp32 [M, n] (a[c0 + i]); lse [n + 1] fp32 [M] -> [n + 1] fp32 [M, V_b]."""
    rows = [np.asarray(r, dtype=F32) for r in band_logits]
    cls = np.asarray(cls, dtype=F32)
    lse = [np.asarray(v, dtype=F32) for v in lse]
    with np.errstate(invalid="ignore", over="ignore"):
        out = [(rows[0] - lse[0][:, None]).astype(F32)]
        for i in range(len(rows) - 1):
            head = (cls[:, i] - lse[0]).astype(F32)
            tail = (rows[i + 1] - lse[i + 1][:, None]).astype(F32)
            out.append((head[:, None] + tail).astype(F32))
    return out


def select_row(band_rows, joint_rows, cutoffs, k):
    base = [0] + [int(c) for c in cutoffs[:-1]]
    tok, val = [], []
    for b, raw in enumerate(band_rows):
        cols = sref.topk(raw, k)                             # the band's RAW order decides who is a candidate
        tok.append(cols + base[b])
        val.append(np.asarray(joint_rows[b], dtype=F32)[cols])
    tok, val = np.concatenate(tok).astype(np.int64), np.concatenate(val).astype(F32)
    by_token = np.argsort(tok, kind="stable")                # (topk breaks ties by position: positions in token order)
    tok, val = tok[by_token], val[by_token]
    order = sref.topk(val, min(int(k), int(cutoffs[-1])))
    return tok[order], val[order]


def select(band_logits, cls, lse, cutoffs, k):
    j = joint(band_logits, cls, lse)
    M = j[0].shape[0]
    got = [select_row([np.asarray(r, dtype=F32)[m] for r in band_logits], [r[m] for r in j], cutoffs, k) for m in range(M)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), j


def beam_candidates(idx, val, score):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(idx).astype(np.int32), (np.asarray(score, dtype=F32)[:, None] + np.asarray(val, dtype=F32)).astype(F32)


def eos_score(joint_rows, cutoffs, eos):
    base = [0] + [int(c) for c in cutoffs[:-1]]
    b = max(i for i in range(len(base)) if eos >= base[i])
    return np.asarray(joint_rows[b], dtype=F32)[:, eos - base[b]]
