"""Sampling and the beam step from the adaptive head (ea_adaptive_sample, ea_adaptive_beam, C ABI 35) against their baselines,
timed on the recipe's geometry (16 layers, 1024 / 4096 / 8 heads, V = 267744, cutoffs 20000 / 60000, factor 4; seeded weights),
bf16, behind a context of `--context` tokens (fp32 parameters under autocast, as the other latency tools run the stack; the
held tables are 16-bit copies either way):
   a. the replayed sampled step, top_k = 40, top_p = 0.9: decode, sample_tokens (ea_adaptive_sample) -- DecoderStack.generate's
      captured step on a state made by init_adaptive_decoding and init_sampling;
   b. the same tree's replayed greedy step on an adaptive-pick state: decode, next_tokens (ea_adaptive_pick);
   c. the framework route a user runs without either: decode, `logits` (a [B, V] tensor), topk(40), softmax, multinomial --
      replayed too;
   d. the replayed beam step at S x W: decode, beam_step (ea_adaptive_beam), reorder_decoding_state by the parents;
   e. the framework route of a beam step: decode, `logits`, log_softmax, the scores added, topk(2 W) per sentence, the reorder --
      eager, as tools/beam_step_latency.py times it on the plain table;
   f. the calls alone on the recipe's tables, M rows of 1024 channels: ea_adaptive_sample (f1) against ea_adaptive_pick (f2).
      The two run the same band passes; f1 stores every band's fp32 logits and the tails' tile candidates on top, and ends in
      the select and the joint launch where f2 ends in the pick's fold: f1 - f2 is what sampling costs over the greedy pick.
      The two launches' own times are a kernel trace's (rocprofv3 --kernel-trace --stats on `--only f`: adaptive_select_kernel,
      adaptive_joint_kernel).
   timeout 900 python tools/adaptive_sample_latency.py [--batches 1,8] [--beams 1x4,8x4] [--context 512] [--rounds 3]
                                                       [--reps 40] [--only abc|de|f]                                  (GPU)
One process, no counters.  Every route is warmed up, then a round times each route once between two device events over `reps`
steps, and the rounds alternate the routes, so that a drift of the machine shows as spread and not as a difference.  One line
per route: the median over the rounds, the smallest and the largest."""
import argparse
import ctypes
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
from ea_harness.sequence import wikitext103_decoder  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adaptive_pick_latency import report  # noqa: E402
from beam_step_latency import captured  # noqa: E402

DTYPE = torch.bfloat16
V = 267744
TOP_K, TOP_P = 40, 0.9


def sampled_routes(m, prompt, B, budget):
    P = prompt.shape[1]
    fed = prompt.expand(B, -1).t().contiguous()
    # a. the sampled step
    st_a = m.init_sampling(m.init_adaptive_decoding(m.init_decoding(B, P + budget, DTYPE, "cuda")), 7, TOP_K, TOP_P)
    tok_a = m.sample_tokens(m.decode(fed, st_a)[-1:], st_a)

    def sampled():
        m.sample_tokens(m.decode(tok_a, st_a), st_a, out=tok_a)
    # b. the greedy step
    st_b = m.init_adaptive_decoding(m.init_decoding(B, P + budget, DTYPE, "cuda"))
    tok_b = m.next_tokens(m.decode(fed, st_b)[-1:], st_b)

    def greedy():
        m.next_tokens(m.decode(tok_b, st_b), st_b, out=tok_b)
    # c. the framework route
    st_c = m.init_decoding(B, P + budget, DTYPE, "cuda")
    tok_c = m.logits(m.decode(fed, st_c)[-1:]).argmax(-1)

    def framework():
        top, idx = torch.topk(m.logits(m.decode(tok_c, st_c))[0].float(), TOP_K, dim=-1)
        drawn = torch.multinomial(torch.softmax(top, dim=-1), 1)
        tok_c.copy_(idx.gather(1, drawn).view(1, B))
    try:
        slow = ("c. logits, topk, softmax, multinomial, replayed", captured(framework))
    except RuntimeError:                                       # (a framework whose multinomial cannot be captured)
        torch.cuda.synchronize()
        slow = ("c. logits, topk, softmax, multinomial, eager", framework)
    return [("a. sampled step (ea_adaptive_sample), replayed", captured(sampled)),
            ("b. greedy step (ea_adaptive_pick), replayed", captured(greedy)), slow], (st_a, st_b, st_c)


def beam_routes(m, prompt, S, W, budget):
    M, P = S * W, prompt.shape[1]
    fed = prompt.expand(M, -1).t().contiguous()
    # d. the beam step
    st_d = m.init_adaptive_decoding(m.init_decoding(M, P + budget, DTYPE, "cuda"))
    last = m.decode(fed, st_d)[-1:]
    eos = int(m.logits(last)[0].float().max(0).values.argmin())   # (an unlikely token: the sentences stay live; reported below)
    m.init_beam_search(st_d, W, eos, budget + 8)
    tok_d, parent = m.beam_step(last, st_d)
    m.reorder_decoding_state(st_d, parent)

    def beam():
        m.beam_step(m.decode(tok_d, st_d), st_d, out=tok_d)
        m.reorder_decoding_state(st_d, st_d.beam.parent)
    # e. the framework route, eager
    st_e = m.init_decoding(M, P + budget, DTYPE, "cuda")
    score = torch.full((S, W), float("-inf"), device="cuda")
    score[:, 0] = 0.0
    tok_e = m.logits(m.decode(fed, st_e)[-1:]).argmax(-1)
    base = (torch.arange(S, device="cuda") * W).view(S, 1)

    def framework():
        logp = torch.log_softmax(m.logits(m.decode(tok_e, st_e))[0].float(), dim=-1)
        cand = (logp.view(S, W, V) + score.unsqueeze(-1)).view(S, W * V)
        top, flat = torch.topk(cand, 2 * W, dim=1)            # (2 W, as a search that sets eos candidates aside takes them)
        top, flat = top[:, :W], flat[:, :W]
        score.copy_(top)
        tok_e.copy_((flat % V).view(1, M))
        m.reorder_decoding_state(st_e, (base + flat // V).view(M))
    for _ in range(2):
        framework()
    return [("d. beam step (ea_adaptive_beam), replayed", captured(beam)),
            ("e. logits, log_softmax, topk, reorder, eager", framework)], (st_d, st_e)


def call_routes(M):
    from efficient_attention import _native as nv
    lib = nv.lib()
    g = torch.Generator().manual_seed(7)
    C, cut, dims = 1024, [20000, 60000, V], [256, 64]

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) / shape[-1] ** 0.5).to(DTYPE).cuda()
    x = torch.randn(M, C, generator=g).to(DTYPE).cuda()
    head, proj = rnd(cut[0] + 2, C), rnd(sum(dims), C)
    tables = [rnd(cut[i + 1] - cut[i], d) for i, d in enumerate(dims)]
    token = torch.zeros(M, dtype=torch.long, device="cuda")
    logp = torch.zeros(M, dtype=torch.float32, device="cuda")
    ctr = torch.zeros(M, dtype=torch.long, device="cuda")
    sid = torch.arange(M, dtype=torch.int32, device="cuda")
    hc, hd = nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims)
    ws1 = torch.empty(lib.ea_adaptive_sample_ws(M, 2, hc, hd), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty(lib.ea_adaptive_pick_ws(M, 2, hc, hd), dtype=torch.uint8, device="cuda")
    pj = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in proj.split(dims, 0)])
    tb = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tables])

    def sample():
        nv.call("ea_adaptive_sample", M, C, 2, hc, hd, nv.ptr(x), nv.io_dtype(x), C, nv.ptr(head), nv.io_dtype(head), pj, tb,
                nv.ptr(ws1), ws1.numel(), TOP_K, TOP_P, 1.0, 7, nv.ptr(ctr), nv.ptr(sid), nv.ptr(token), nv.ptr(logp), None, None,
                None, nv.stream())

    def pick():
        nv.call("ea_adaptive_pick", M, C, 2, hc, hd, nv.ptr(x), nv.io_dtype(x), C, None, nv.ptr(head), nv.io_dtype(head), pj, tb,
                nv.ptr(ws2), ws2.numel(), nv.ptr(token), nv.ptr(logp), nv.stream())
    todo = [("f1. ea_adaptive_sample, the recipe's tables", captured(sample)),
            ("f2. ea_adaptive_pick, the recipe's tables", captured(pick))]
    return todo, [x, head, proj, tables, token, logp, ctr, sid, ws1, ws2, ws1.numel()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--beams", default="1x4,8x4")
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--only", default="abcdef")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_sample_latency.py times GPU kernels: no GPU here, nothing measured")
    print("device:", torch.cuda.get_device_name(0), "| context", a.context, "| V", V, "| %d rounds of %d steps" % (a.rounds, a.reps))
    if "f" in a.only:
        for M in (int(v) for v in a.batches.split(",")):
            todo, keep = call_routes(M)
            med = report("M = %d" % M, todo, a.rounds, 4 * a.reps, unit="us", scale=1000.0)
            f1, f2 = (med[name] for name, _ in todo)
            print("M = %-4d workspace %d bytes; sampling over the greedy pick (f1 - f2) %.1f us" % (M, keep[-1], f1 - f2), flush=True)
            del todo, keep
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    if not set("abcde") & set(a.only):
        return
    torch.manual_seed(3)
    m = wikitext103_decoder(vocab=V, adaptive=True).cuda().eval()
    prompt = torch.randint(2, V, (1, a.context), generator=torch.Generator().manual_seed(11)).cuda()
    budget = 4 + a.rounds * a.reps + 8
    if set("abc") & set(a.only):
        for B in (int(v) for v in a.batches.split(",")):
            with torch.no_grad(), torch.autocast("cuda", dtype=DTYPE, cache_enabled=False), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                todo, states = sampled_routes(m, prompt, B, budget)
                med = report("B = %d" % B, todo, a.rounds, a.reps)
            ms = [med[name] for name, _ in todo]
            print("B = %-4d sampling on top of the greedy step (a - b) %.3f ms; framework route / sampled step (c / a) %.2f"
                  % (B, ms[0] - ms[1], ms[2] / ms[0]), flush=True)
            if any(m.decoding_overflowed(st) for st in states):
                raise SystemExit("a decoding state overflowed: the numbers above are not a decoding step's")
            del todo, states
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    if set("de") & set(a.only):
        for beams in a.beams.split(","):
            S, W = (int(s) for s in beams.split("x"))
            with torch.no_grad(), torch.autocast("cuda", dtype=DTYPE, cache_enabled=False), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                todo, states = beam_routes(m, prompt, S, W, budget)
                med = report("S x W = %s" % beams, todo, a.rounds, a.reps)
            ms = [med[name] for name, _ in todo]
            print("S x W = %-5s framework route / beam step (e / d) %.2f; sentences done at the end: %d of %d"
                  % (beams, ms[1] / ms[0], int(states[0].beam.done.ne(0).sum()), S), flush=True)
            if any(m.decoding_overflowed(st) for st in states):
                raise SystemExit("a decoding state overflowed: the numbers above are not a decoding step's")
            del todo, states
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
