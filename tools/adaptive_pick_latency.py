"""The greedy pick from the adaptive head (ea_adaptive_pick, C ABI 34) against its baselines, timed on the recipe's geometry
(16 layers, 1024 / 4096 / 8 heads, V = 267744, cutoffs 20000 / 60000, factor 4; seeded weights), bf16, behind a context of
`--context` tokens, for B rows (fp32 parameters under autocast, as the other latency tools run the stack; the held
tables are 16-bit copies either way):
   a. the replayed greedy step on an adaptive-pick state: decode, next_tokens (ea_adaptive_pick) -- DecoderStack.generate's
      captured step on a state made by init_adaptive_decoding;
   b. the same step on the slow `logits` route (a state without it): decode, AdaptiveSoftmax.get_log_prob -- framework GEMMs,
      three log_softmax, a cat -- and an argmax over [B, V], replayed too;
   c. the same step on a hold_vocab state of the plain 267744-row stand-in (ea_ceva_sdecode_vocab_argmax on a [V, 1024] table);
   d. the widest tail alone, [207744, 64], M rows: ea_adaptive_pick on a geometry whose head is 16 words of 32 channels, so
      that the call is the tail pass and the pick's fold behind four launches of one workgroup each (d1); the same call with
      a tail of 16 tokens: those launches alone (d0); and ea_ceva_sdecode_vocab_logprob at K = 64, V = 207744: the K-split
      instance of the few-row kernel with its own fold (d2).  d1 against d2 is the column-split kernel with everything
      around it against the K-split one; d0 bounds what surrounds the tail (its one workgroup is latency-bound, so d1 - d0 is
      NOT the tail's time: take that from a kernel trace).
   e. the pick alone on the recipe's tables, M rows of 1024 channels: ea_adaptive_pick (e1) against
      ea_ceva_sdecode_vocab_argmax on a plain [267744, 1024] table (e2): the two steps' last stage without the stack in front.
   timeout 900 python tools/adaptive_pick_latency.py [--batches 1,8] [--rows 1,64] [--context 512] [--rounds 3] [--reps 40]
                                                     [--only abc|d|e]                                                 (GPU)
One process, no counters.  Every route is warmed up, then a round times each route once between two device events over `reps`
steps, and the rounds alternate the routes, so that a drift of the machine shows as spread and not as a difference.  One line
per route: the median over the rounds, the smallest and the largest.  EA_HIP_LIB names another build of the library (the
tiles-per-wave A/B of DESIGN.md 4a was taken this way, on part d)."""
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
from beam_step_latency import captured, timed  # noqa: E402

DTYPE = torch.bfloat16
V = 267744


def report(label, todo, rounds, reps, unit="ms", scale=1.0):
    times = {name: [] for name, _ in todo}
    for _ in range(rounds):
        for name, call in todo:
            times[name].append(timed(call, reps) * scale)
    med = {}
    for name, _ in todo:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        print("%-8s %-44s median %9.3f %s (min %9.3f, max %9.3f)" % (label, name, med[name], unit, t[0], t[-1]), flush=True)
    return med


def step_routes(adaptive, plain, prompt, B, budget):
    P = prompt.shape[1]
    fed = prompt.expand(B, -1).t().contiguous()
    # a. the adaptive pick
    st_a = adaptive.init_adaptive_decoding(adaptive.init_decoding(B, P + budget, DTYPE, "cuda"))
    tok_a = adaptive.next_tokens(adaptive.decode(fed, st_a)[-1:], st_a)

    def pick():
        adaptive.next_tokens(adaptive.decode(tok_a, st_a), st_a, out=tok_a)
    # b. the slow route
    st_b = adaptive.init_decoding(B, P + budget, DTYPE, "cuda")
    tok_b = adaptive.logits(adaptive.decode(fed, st_b)[-1:]).argmax(-1)

    def slow():
        tok_b.copy_(adaptive.logits(adaptive.decode(tok_b, st_b)).argmax(-1))
    # c. the plain stand-in's held table
    st_c = plain.init_decoding(B, P + budget, DTYPE, "cuda", hold_vocab=True)
    tok_c = plain.next_tokens(plain.decode(fed, st_c)[-1:], st_c)

    def held():
        plain.next_tokens(plain.decode(tok_c, st_c), st_c, out=tok_c)
    return [("a. adaptive pick, replayed", captured(pick)), ("b. slow `logits` route, replayed", captured(slow)),
            ("c. plain [V, 1024] held table, replayed", captured(held))], (st_a, st_b, st_c)


def tail_routes(M):
    from efficient_attention import _native as nv
    lib = nv.lib()
    g = torch.Generator().manual_seed(5)
    Vt, d, C, c0 = 207744, 64, 32, 16

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) / shape[-1] ** 0.5).to(DTYPE).cuda()
    x = torch.randn(M, C, generator=g).to(DTYPE).cuda()
    head, proj, table = rnd(c0 + 1, C), rnd(d, C), rnd(Vt, d)
    token = torch.zeros(M, dtype=torch.long, device="cuda")
    logp = torch.zeros(M, dtype=torch.float32, device="cuda")
    keep = [x, head, proj, table, token, logp]

    def composite(size):
        cut, dims = nv.host_array(ctypes.c_int64, [c0, c0 + size]), nv.host_array(ctypes.c_int32, [d])
        ws = torch.empty(lib.ea_adaptive_pick_ws(M, 1, cut, dims), dtype=torch.uint8, device="cuda")
        pj, tb = nv.host_array(ctypes.c_void_p, [proj.data_ptr()]), nv.host_array(ctypes.c_void_p, [table.data_ptr()])
        keep.append(ws)

        def call():
            nv.call("ea_adaptive_pick", M, C, 1, cut, dims, nv.ptr(x), nv.io_dtype(x), C, None, nv.ptr(head), nv.io_dtype(head),
                    pj, tb, nv.ptr(ws), ws.numel(), nv.ptr(token), nv.ptr(logp), nv.stream())
        return call
    # d2: the K-split instance on the same table, h as its rows
    h = torch.randn(M, d, generator=g).to(DTYPE).cuda()
    ws2 = torch.empty(lib.ea_ceva_sdecode_vocab_ws(M, Vt), dtype=torch.uint8, device="cuda")
    lws = torch.empty(lib.ea_ceva_sdecode_vocab_lse_ws(M, Vt), dtype=torch.uint8, device="cuda")
    lse = torch.zeros(M, dtype=torch.float32, device="cuda")
    keep += [h, ws2, lws, lse]

    def ksplit():
        nv.call("ea_ceva_sdecode_vocab_logprob", M, d, Vt, nv.ptr(h), nv.io_dtype(h), d, nv.ptr(table), nv.io_dtype(table), None,
                nv.EA_F32, Vt, nv.ptr(ws2), ws2.numel(), nv.ptr(token), None, nv.ptr(lws), lws.numel(), None, nv.ptr(lse),
                nv.ptr(logp), nv.stream())
    todo = [("d1. ea_adaptive_pick, tail [207744, 64]", captured(composite(Vt))),
            ("d0. ea_adaptive_pick, tail [16, 64]", captured(composite(16))),
            ("d2. ea_ceva_sdecode_vocab_logprob, K = 64", captured(ksplit))]
    return todo, keep


def pick_routes(M):
    from efficient_attention import _native as nv
    lib = nv.lib()
    g = torch.Generator().manual_seed(7)
    C, cut, dims = 1024, [20000, 60000, V], [256, 64]

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) / shape[-1] ** 0.5).to(DTYPE).cuda()
    x = torch.randn(M, C, generator=g).to(DTYPE).cuda()
    head, proj = rnd(cut[0] + 2, C), rnd(sum(dims), C)
    tables = [rnd(cut[i + 1] - cut[i], d) for i, d in enumerate(dims)]
    plain = rnd(V, C)
    token = torch.zeros(M, dtype=torch.long, device="cuda")
    logp = torch.zeros(M, dtype=torch.float32, device="cuda")
    hc, hd = nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims)
    ws = torch.empty(lib.ea_adaptive_pick_ws(M, 2, hc, hd), dtype=torch.uint8, device="cuda")
    pj = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in proj.split(dims, 0)])
    tb = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tables])
    ws2 = torch.empty(lib.ea_ceva_sdecode_vocab_ws(M, V), dtype=torch.uint8, device="cuda")

    def adaptive():
        nv.call("ea_adaptive_pick", M, C, 2, hc, hd, nv.ptr(x), nv.io_dtype(x), C, None, nv.ptr(head), nv.io_dtype(head), pj, tb,
                nv.ptr(ws), ws.numel(), nv.ptr(token), nv.ptr(logp), nv.stream())

    def argmax():
        nv.call("ea_ceva_sdecode_vocab_argmax", M, C, V, nv.ptr(x), nv.io_dtype(x), C, nv.ptr(plain), nv.io_dtype(plain), None,
                nv.EA_F32, V, nv.ptr(ws2), ws2.numel(), nv.ptr(token), None, nv.stream())
    todo = [("e1. ea_adaptive_pick, the recipe's tables", captured(adaptive)),
            ("e2. ea_ceva_sdecode_vocab_argmax, [V, 1024]", captured(argmax))]
    return todo, [x, head, proj, tables, plain, token, logp, ws, ws2, ws.numel()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rows", default="1,64")
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--only", default="abcde")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_pick_latency.py times GPU kernels: no GPU here, nothing measured")
    print("device:", torch.cuda.get_device_name(0), "| context", a.context, "| V", V, "| %d rounds of %d steps" % (a.rounds, a.reps))
    if "d" in a.only:
        for M in (int(v) for v in a.rows.split(",")):
            todo, keep = tail_routes(M)
            med = report("M = %d" % M, todo, a.rounds, 4 * a.reps, unit="us", scale=1000.0)
            d1, d0, d2 = (med[name] for name, _ in todo)
            print("M = %-4d the call with the column-split tail (d1) %.1f us, with a one-workgroup tail (d0) %.1f us; K-split pass "
                  "and fold (d2) %.1f us; d2 / d1 %.2f" % (M, d1, d0, d2, d2 / d1), flush=True)
            del todo, keep
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    if "e" in a.only:
        for M in (int(v) for v in a.batches.split(",")):
            todo, keep = pick_routes(M)
            med = report("M = %d" % M, todo, a.rounds, 4 * a.reps, unit="us", scale=1000.0)
            e1, e2 = (med[name] for name, _ in todo)
            print("M = %-4d workspace %d bytes; plain table / adaptive pick (e2 / e1) %.2f" % (M, keep[-1], e2 / e1), flush=True)
            del todo, keep
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    if not set("abc") & set(a.only):
        return
    torch.manual_seed(3)
    adaptive = wikitext103_decoder(vocab=V, adaptive=True).cuda().eval()
    torch.manual_seed(3)
    plain = wikitext103_decoder(vocab=V).cuda().eval()
    with torch.no_grad():
        plain.embed_tokens.weight.mul_(1.0 / 32)
    prompt = torch.randint(2, V, (1, a.context), generator=torch.Generator().manual_seed(11)).cuda()
    budget = 4 + a.rounds * a.reps + 8
    for B in (int(v) for v in a.batches.split(",")):
        with torch.no_grad(), torch.autocast("cuda", dtype=DTYPE, cache_enabled=False), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            todo, states = step_routes(adaptive, plain, prompt, B, budget)
            med = report("B = %d" % B, todo, a.rounds, a.reps)
        ms = [med[name] for name, _ in todo]
        print("B = %-4d slow route / adaptive pick (b / a) %.2f; plain held table / adaptive pick (c / a) %.2f"
              % (B, ms[1] / ms[0], ms[2] / ms[0]), flush=True)
        if any(m.decoding_overflowed(st) for m, st in zip((adaptive, adaptive, plain), states)):
            raise SystemExit("a decoding state overflowed: the numbers above are not a decoding step's")
        del todo, states
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
