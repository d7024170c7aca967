"""The beam-search step of the decoder stack (ea_ceva_sdecode_vocab_beam, C ABI 32) against its two baselines, timed on the
16-layer wikitext-103 stack (1024 / 4096 / 8 heads, V = 32768, seeded weights), bf16, behind a context of `--context` tokens,
for S sentences of W beams (M = S W rows):
   a. the replayed beam step: decode, beam_step (the table pass, the rows and the merge kernel), reorder_decoding_state by the
      parents the step has just written -- DecoderStack.beam_search's captured step;
   b. the replayed greedy step at the same number of rows M: decode, next_tokens -- DecoderStack.generate's captured step; a - b
      is what beams cost on top of decoding M rows;
   c. the eager framework route a user had to write before ABI 32: decode, next_tokens(return_logits=True), log_softmax, the
      cumulative scores, topk over [S, W V], the two gathers, the reorder -- no capture (its host loop is part of it);
   d. the reorder alone, replayed with a fixed parent index: its share of a;
   e. with --min-len, --no-repeat-ngram-size or --ban-tokens: the replayed CONSTRAINED beam step (ea_ceva_sdecode_vocab_beam_c,
      C ABI 36: one more launch, the ban list, and the row kernel's constrained instance; the prompt counts for the n-grams),
      on a state of its own beside a; e - a is what the constraints cost.
   --adaptive: the recipe's adaptive head (V = 267744, cutoffs 20000 / 60000) in place of the plain table: routes a, d and e
   alone (ea_adaptive_beam, ea_adaptive_beam_c); b and c are tools/adaptive_sample_latency.py's.
   timeout 600 python tools/beam_step_latency.py [--beams 1x4,1x8,8x4] [--context 512] [--rounds 3] [--reps 40]
                                                  [--min-len N] [--no-repeat-ngram-size N] [--ban-tokens 1,3] [--adaptive]   (GPU)
One process, no counters.  Every route is warmed up, then a round times each route once between two device events over `reps`
steps, and the rounds alternate the routes, so that a drift of the machine shows as spread and not as a difference.  One line
per (S x W, route): the median ms per step over the rounds, the smallest and the largest.  eos is the token with the smallest
logit at the first pick, so that beams stay alive; how many sentences were done at the end is printed all the same."""
import argparse
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
from ea_harness.sequence import wikitext103_decoder  # noqa: E402

DTYPE = torch.bfloat16


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def captured(step):
    """Warm `step` up on a side stream, capture it -> the replay.  A graph holds the addresses of the tensors its step read
    and wrote, not the tensors: the replay keeps `step` -- and with it every state and static input the step closes over --
    alive for as long as it is itself."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()

    def replay():
        g.replay()
    replay.step = step
    return replay


def prefilled(m, prompt, M, budget, **kw):
    if m.is_adaptive:
        st = m.init_adaptive_decoding(m.init_decoding(M, prompt.shape[1] + budget, DTYPE, "cuda", **kw))
    else:
        st = m.init_decoding(M, prompt.shape[1] + budget, DTYPE, "cuda", hold_vocab=True, **kw)
    last = m.decode(prompt.expand(M, -1).t().contiguous(), st)[-1:]
    return st, last


def beam_route(m, prompt, S, W, budget, eos, limits=None):
    """-> (the step of a beam search behind its first pick, its state); limits: the constraints' keywords, or None."""
    st, last = prefilled(m, prompt, S * W, budget)
    m.init_beam_search(st, W, eos, budget + 8)
    if limits:
        m.init_beam_constraints(st, prompt_cap=prompt.shape[1], **limits)
        m.set_beam_prompt(st, prompt.expand(S, -1))
    tok, parent = m.beam_step(last, st)
    m.reorder_decoding_state(st, parent)

    def beam():
        m.beam_step(m.decode(tok, st), st, out=tok)
        m.reorder_decoding_state(st, st.beam.parent)
    return beam, st


def routes(m, prompt, S, W, budget, limits=None):
    M = S * W
    base = (torch.arange(S, device="cuda") * W).view(S, 1)
    if m.is_adaptive:
        eos = m.adaptive_softmax.cutoff[-1] - 1             # (the last tail's last token: beams stay alive)
    else:
        V = m.embed_tokens.weight.shape[0]
        st_0, last = prefilled(m, prompt, M, budget)
        _, logits = m.next_tokens(last, st_0, return_logits=True)
        eos = int(logits[0].max(0).values.argmin())
        del st_0
    # a. the beam step; e. the constrained one
    beam, st_a = beam_route(m, prompt, S, W, budget, eos)
    constrained = [("e. constrained beam step, replayed", captured(beam_route(m, prompt, S, W, budget, eos, limits)[0]))] if limits else []
    # d. the reorder alone
    st_d, _ = prefilled(m, prompt, M, budget)
    fixed = (base + torch.randint(0, W, (S, W), device="cuda")).view(M)

    def reorder():
        m.reorder_decoding_state(st_d, fixed)
    if m.is_adaptive:
        return [("a. beam step, replayed", captured(beam)), ("d. reorder alone, replayed", captured(reorder))] + constrained, st_a
    # b. the greedy step at M rows
    st_b, last = prefilled(m, prompt, M, budget)
    tok_b = m.next_tokens(last, st_b)

    def greedy():
        m.next_tokens(m.decode(tok_b, st_b), st_b, out=tok_b)
    # c. the framework route, eager
    st_c, last = prefilled(m, prompt, M, budget)
    score = torch.full((S, W), float("-inf"), device="cuda")
    score[:, 0] = 0.0
    tok_c = m.next_tokens(last, st_c)

    def framework():
        _, logits = m.next_tokens(m.decode(tok_c, st_c), st_c, return_logits=True)
        cand = (torch.log_softmax(logits[0], dim=-1).view(S, W, V) + score.unsqueeze(-1)).view(S, W * V)
        top, flat = torch.topk(cand, 2 * W, dim=1)        # (2 W, as a search that sets eos candidates aside takes them)
        top, flat = top[:, :W], flat[:, :W]
        score.copy_(top)
        tok_c.copy_((flat % V).view(1, M))
        m.reorder_decoding_state(st_c, (base + flat // V).view(M))
    for _ in range(2):
        framework()
    return [("a. beam step, replayed", captured(beam)), ("b. greedy step, replayed", captured(greedy)),
            ("c. framework route, eager", framework), ("d. reorder alone, replayed", captured(reorder))] + constrained, st_a


def measure(m, prompt, beams, budget, rounds, reps, limits=None):
    S, W = (int(s) for s in beams.split("x"))
    with torch.no_grad(), torch.autocast("cuda", dtype=DTYPE, cache_enabled=False), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        todo, st = routes(m, prompt, S, W, budget, limits)
        times = {name: [] for name, _ in todo}
        for _ in range(rounds):
            for name, call in todo:
                times[name].append(timed(call, reps))
    med = {}
    for name, _ in todo:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        print("S x W = %-5s %-28s median %8.3f ms a step (min %8.3f, max %8.3f)" % (beams, name, med[name], t[0], t[-1]), flush=True)
    by_letter = {name[0]: ms for name, ms in med.items()}
    a_ms, d_ms = by_letter["a"], by_letter["d"]
    if "b" in by_letter:
        print("S x W = %-5s beams on top of greedy decoding (a - b) %.3f ms; framework route / beam step (c / a) %.2f"
              % (beams, a_ms - by_letter["b"], by_letter["c"] / a_ms), flush=True)
    if "e" in by_letter:
        print("S x W = %-5s the constraints on top of the beam step (e - a) %.3f ms (%.1f %%)"
              % (beams, by_letter["e"] - a_ms, 100.0 * (by_letter["e"] - a_ms) / a_ms), flush=True)
    print("S x W = %-5s reorder's share of the beam step (d / a) %.0f %%; sentences done at the end: %d of %d"
          % (beams, 100.0 * d_ms / a_ms, int(st.beam.done.ne(0).sum()), S), flush=True)
    if m.decoding_overflowed(st):
        raise SystemExit("the decoding state overflowed: the numbers above are not a decoding step's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="1x4,1x8,8x4")
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--min-len", type=int, default=0)
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0)
    ap.add_argument("--ban-tokens", default="")
    ap.add_argument("--adaptive", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_step_latency.py times GPU kernels: no GPU here, nothing measured")
    torch.manual_seed(3)
    if a.adaptive:
        V = 267744
        m = wikitext103_decoder(vocab=V, adaptive=True).cuda().eval()
    else:
        m = wikitext103_decoder().cuda().eval()
        with torch.no_grad():
            m.embed_tokens.weight.mul_(1.0 / 32)           # (rows of the initial size make a token's own embedding decide the pick)
        V = m.embed_tokens.weight.shape[0]
    bans = tuple(int(v) for v in a.ban_tokens.split(",") if v)
    limits = dict(min_len=a.min_len, no_repeat_ngram_size=a.no_repeat_ngram_size, ban_tokens=bans)
    if not (a.min_len or a.no_repeat_ngram_size or bans):
        limits = None
    prompt = torch.randint(2, V, (1, a.context), generator=torch.Generator().manual_seed(11)).cuda()
    budget = 4 + a.rounds * a.reps + 8
    print("device:", torch.cuda.get_device_name(0), "| context", a.context, "| V", V, "| %d rounds of %d steps" % (a.rounds, a.reps))
    for beams in a.beams.split(","):
        measure(m, prompt, beams, budget, a.rounds, a.reps, limits)   # (its graphs and states end with the call)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
