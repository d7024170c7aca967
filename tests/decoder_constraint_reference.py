"""Host reference of the constrained beam step (ea_beam_bans, ea_ceva_sdecode_vocab_beam_c, ea_adaptive_beam_c; include/ea_hip.h,
C ABI 36), numpy on the CPU: tests/test_decoder_constraints_cpu.py checks it against fairseq's recorded masks
(tests/golden/ngram_block.npz) and hand-worked answers, tests/test_gpu_decoder_constraints.py checks the kernels against it.

  banned(x, t, n, min_len, eos, ban_tokens) -> set
      the banned tokens of a row whose sequence is x (prompt ++ generated, L = len(x)) at step t (tokens generated so far):
      the static bans, eos while t < min_len, and for n >= 1 every x[i + n - 1] with x[i .. i + n - 1) == x[L - n + 1 .. L),
      i = 0 .. L - n.  The forced step is the caller's: it bans nothing.
  apply(logits_row, banned) -> the fp32 row with -inf at the banned columns (those outside the row are skipped)
  row_candidates_c(logits_row, lse, score, W, eos, forced, banned) -> decoder_beam_reference.row_candidates on the masked row;
      lse is the UNCONSTRAINED row's; forced: nothing is masked.
  beam_tokens(hist_tok, hist_par, t, W) -> per beam of one sentence the t tokens it has generated, by following hist_par back
  host_beam_search_c(step_fn, S, W, eos, max_new, len_penalty, prompts, n, min_len, ban_tokens) -> (hyps, info)
      decoder_beam_reference.host_beam_search behind a step function that masks every row before the candidates are taken;
      prompts: per sentence the list of its prompt's tokens."""
import numpy as np

import decoder_beam_reference as bref

F32 = np.float32


def banned(x, t, n, min_len, eos, ban_tokens):
    x = [int(v) for v in x]
    out = set(int(v) for v in ban_tokens)
    if t < min_len:
        out.add(int(eos))
    L = len(x)
    if n >= 1:
        suffix = x[L - n + 1:L] if n > 1 else []
        for i in range(0, L - n + 1):
            if x[i:i + n - 1] == suffix:
                out.add(x[i + n - 1])
    return out


def apply(logits_row, banned_set):
    row = np.array(logits_row, dtype=F32, copy=True)
    for v in banned_set:
        if 0 <= v < row.shape[0]:
            row[v] = -np.inf
    return row


def row_candidates_c(logits_row, lse, score, W, eos, forced, banned_set):
    row = np.asarray(logits_row, dtype=F32) if forced else apply(logits_row, banned_set)
    return bref.row_candidates(row, lse, score, W, eos, forced)


def beam_tokens(hist_tok, hist_par, t, W):
    out = []
    for b in range(W):
        toks, at = [], b
        for step in range(t - 1, -1, -1):
            toks.append(int(hist_tok[step][at]))
            at = int(hist_par[step][at])
        out.append(toks[::-1])
    return out


def host_beam_search_c(step_fn, S, W, eos, max_new, len_penalty=1.0, prompts=None, n=0, min_len=0, ban_tokens=()):
    """decoder_beam_reference.host_beam_search on a step function that masks: every call's rows get -inf at their banned columns
    before rule A sees them (lse stays the unconstrained one), but on the forced step.  The wrapper keeps each row's generated
    tokens by the (tokens, parent) pairs the search hands it: row m continues row parent[m] with tokens[m].  All live
    sentences have generated as many tokens as there were calls; the rows of a done sentence are masked too and never read.
    info gets `bans`: (sentence, beam, t, banned set) per row and unforced step."""
    M = S * W
    prompts = [[] for _ in range(S)] if prompts is None else prompts
    gen, bans, calls = [[] for _ in range(M)], [], [0]

    def masking(tokens, parent):
        logits, lse = step_fn(tokens, parent)
        t = calls[0]
        calls[0] += 1
        if tokens is not None:
            gen[:] = [gen[int(parent[m])] + [int(tokens[m])] for m in range(M)]
        if t + 1 >= max_new:
            return logits, lse
        rows = []
        for m in range(M):
            bset = banned(list(prompts[m // W]) + gen[m], t, n, min_len, eos, ban_tokens)
            bans.append((m // W, m % W, t, bset))
            rows.append(apply(logits[m], bset))
        return np.stack(rows), lse
    hyps, info = bref.host_beam_search(masking, S, W, eos, max_new, len_penalty)
    info["bans"] = bans
    return hyps, info


# ---- the properties a constrained search promises, for tests that must not pass vacuously ------------------------------------------
def violations(prompt, tokens, eos, max_new, n, min_len, ban_tokens):
    """The promises a finished hypothesis (tokens: its generated tokens, the closing eos included) breaks -> a set of
    "ngram", "min_len", "ban".  A hypothesis the forced step closed (max_new tokens) is exempt from min_len alone in its
    last token; its n-grams and bans are checked over the tokens before the forced eos."""
    tokens, prompt = [int(v) for v in tokens], [int(v) for v in prompt]
    out = set()
    forced = len(tokens) >= max_new
    body = tokens[:-1] if forced else tokens                 # (the forced eos ignores every constraint)
    if min_len and not forced and len(tokens) - 1 < min_len:
        out.add("min_len")
    if any(v in set(ban_tokens) for v in body):
        out.add("ban")
    if n >= 1:
        x = prompt + body
        seen = set()
        for end in range(n, len(x) + 1):
            gram = tuple(x[end - n:end])
            if gram in seen and end > len(prompt):               # it ends inside the generated part, a second time
                out.add("ngram")
            seen.add(gram)
    return out
