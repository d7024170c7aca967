"""Host reference of the beam step (ea_ceva_sdecode_vocab_beam / ea_beam_merge, include/ea_hip.h, C ABI 32), numpy on the CPU:
tests/test_decoder_beam_cpu.py checks it against hand-worked answers, tests/test_gpu_decoder_beam.py checks the kernels and
DecoderStack.beam_search against it.  Scores are np.float32 throughout; a candidate's score is formed by the rule's two fp32
operations, the subtraction first.

  row_candidates(logits_row, lse, score, W, eos, forced) -> (idx int32 [k'], val fp32 [k'], cand fp32 [k'])
      rule A for one row: forced: k' = 1, the eos column; else the k' = min(2 W, V) best logits under
      decoder_sample_reference.topk's total order; cand[j] = score + (val[j] - lse).
  merge(cand_idx, cand_score, kc, W, eos, t, nfin, done, forced) -> dict
      rules B and C for one sentence: cand_idx / cand_score [W, >= kc] (the forced step reads column 0 alone).  Keys: token
      [W], parent [W] (beams of THIS sentence: the kernel adds s W), score fp32 [W] (None: a done sentence leaves it),
      hist_tok / hist_par [W] (None likewise), records (a list of (fp32 score, length, beam)), t, nfin, done (the new state)
      and events, the set of the things that happened: "eos_finished", "eos_late" (an eos at i >= W, dropped), "eos_inf" (an
      eos with -inf among the first W, dropped), "eos_full" (an eos with nfin == W already, dropped), "tie" (two walked
      neighbours, or the last walked and the first left out, of equal score: the flat index decided), "dead_beam",
      "nan_first", "forced", "forced_finished", "went_idle" (nfin reached W on a step that was not the forced one), "idle".
  backtrack(hist_tok, hist_par, fin_len, fin_beam, eos) -> the hypothesis' tokens (a list; hist_* [steps, W] of one sentence)
  finish(records, len_penalty) -> the records as dicts (raw, len, beam, score = raw / len ** len_penalty in fp64), the best
      first: NaN above every number, the larger first, ties by finishing order
  host_beam_search(step_fn, S, W, eos, max_new, len_penalty=1.0) -> (hyps, info)
      step_fn(tokens, parent) -> (logits fp32 [M, V], lse fp32 [M]); the first call gets (None, None) and answers for the
      prompts' last rows; every later one gets the int64 tokens [M] to feed and the global parent rows [M] to reorder by
      first.  hyps: per sentence the finished hypotheses (finish's dicts with `tokens`); info: steps, events, fin_len."""
import numpy as np

import decoder_sample_reference as sref

F32 = np.float32
NEG_INF = F32(-np.inf)


def row_candidates(logits_row, lse, score, W, eos, forced):
    row = np.asarray(logits_row, dtype=F32)
    idx = np.array([eos], dtype=np.int64) if forced else sref.topk(row, 2 * W)
    val = row[idx]
    with np.errstate(invalid="ignore", over="ignore"):
        cand = (F32(score) + (val - F32(lse)).astype(F32)).astype(F32)
    return idx.astype(np.int32), val, cand


def _same(a, b):
    """Equal under the total order: two NaNs, or two equal numbers (+0 and -0 too)."""
    return bool((np.isnan(a) and np.isnan(b)) or a == b)


def merge(cand_idx, cand_score, kc, W, eos, t, nfin, done, forced):
    if done:
        return dict(token=[eos] * W, parent=list(range(W)), score=None, hist_tok=None, hist_par=None, records=[], t=t, nfin=nfin,
                    done=1, events={"idle"})
    k = 1 if forced else int(kc)
    idx = np.asarray(cand_idx)[:W, :k].reshape(-1)
    sc = np.asarray(cand_score, dtype=F32)[:W, :k].reshape(-1)
    n = W * k
    n2 = min(2 * W, n)
    order = sref.topk(sc, n)
    events = set()
    if np.isnan(sc[order[0]]):
        events.add("nan_first")
    if any(_same(sc[order[i]], sc[order[i + 1]]) for i in range(min(n2, n - 1))):
        events.add("tie")
    token, parent, score, records = [], [], [], []
    for i in range(n2):
        f = int(order[i])
        b, tok, s = f // k, int(idx[f]), sc[f]
        if tok == eos:
            if i >= W:
                events.add("eos_late")
            elif s == NEG_INF:
                events.add("eos_inf")
            elif nfin >= W:
                events.add("eos_full")
            else:
                records.append((s, t + 1, b))
                nfin += 1
                events.add("eos_finished")
        elif len(token) < W:
            token.append(tok)
            parent.append(b)
            score.append(s)
    if len(token) < W:
        events.add("dead_beam")
    for r in range(len(token), W):
        token.append(eos)
        parent.append(r)
        score.append(NEG_INF)
    if forced:
        events.add("forced")
        if records:
            events.add("forced_finished")
    elif nfin == W:
        events.add("went_idle")
    return dict(token=token, parent=parent, score=np.array(score, dtype=F32), hist_tok=list(token), hist_par=list(parent),
                records=records, t=t + 1, nfin=nfin, done=int(nfin == W or forced), events=events)


def backtrack(hist_tok, hist_par, fin_len, fin_beam, eos):
    tokens, b = [eos], fin_beam
    for t in range(fin_len - 2, -1, -1):
        tokens.append(int(hist_tok[t][b]))
        b = int(hist_par[t][b])
    return tokens[::-1]


def finish(records, len_penalty):
    out = [dict(raw=F32(s), len=int(n), beam=int(b), score=float(s) / float(n) ** float(len_penalty)) for s, n, b in records]
    order = sorted(range(len(out)), key=lambda i: (0 if np.isnan(out[i]["score"]) else 1,
                                                   0.0 if np.isnan(out[i]["score"]) else -out[i]["score"], i))
    return [out[i] for i in order]


def host_beam_search(step_fn, S, W, eos, max_new, len_penalty=1.0):
    M = S * W
    score = np.full(M, NEG_INF, dtype=F32)
    score[::W] = F32(0)
    t, nfin, done = [0] * S, [0] * S, [0] * S
    hist_tok, hist_par, records = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    events, tokens, parent, steps = set(), None, None, 0
    for _ in range(max_new):
        logits, lse = step_fn(tokens, parent)
        steps += 1
        tokens, parent = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
        for s in range(S):
            rows = range(s * W, s * W + W)
            forced = t[s] + 1 == max_new
            k = 1 if forced else min(2 * W, logits.shape[1])
            ci, cs = np.zeros((W, k), dtype=np.int32), np.zeros((W, k), dtype=F32)
            if not done[s]:
                for b, m in enumerate(rows):
                    ci[b], _, cs[b] = row_candidates(logits[m], lse[m], score[m], W, eos, forced)
            got = merge(ci, cs, k, W, eos, t[s], nfin[s], done[s], forced)
            events |= got["events"]
            tokens[s * W:s * W + W] = got["token"]
            parent[s * W:s * W + W] = [s * W + b for b in got["parent"]]
            if got["score"] is not None:
                score[s * W:s * W + W] = got["score"]
                hist_tok[s].append(got["hist_tok"])
                hist_par[s].append(got["hist_par"])
                records[s] += got["records"]
            t[s], nfin[s], done[s] = got["t"], got["nfin"], got["done"]
        if all(done):
            break
    hyps = []
    for s in range(S):
        out = finish(records[s], len_penalty)
        for h in out:
            h["tokens"] = backtrack(hist_tok[s], hist_par[s], h["len"], h["beam"], eos)
        hyps.append(out)
    return hyps, dict(steps=steps, events=events, fin_len=[[n for _, n, _ in r] for r in records])
