"""Decoding latency of causal softmax attention on its KV cache (csrc/ea_softmax_decode.hip), embed 1024, h 8, d 128, bf16:
   layer   one replayed 1-token step of one attention layer (held projections) at a given context, against
             sdpa   F.scaled_dot_product_attention on the same cache rows around the same held projections
             ceva   the causal EVA layer's replayed step on a rolling state at the same context (bench.py's LM arguments)
           and the same step at every kv_splits of --splits around the planner's choice
   stack   one replayed 1-token step of a 16-layer DecoderStack (ffn 4096, vocab 32768), softmax against causal_eva
   prompt  one eager 2048-token prompt step of the layer from an empty cache, against sdpa is_causal
   --per-sequence   instead of the above: the layer's replayed 1-token step on a per-sequence state (pos [B]) at uniform
           contexts, next to two shared-count states of the same geometry measured in the same rounds (`shared`, and its twin
           `shared'`: the distance between the two is the baseline's own run-to-run spread), and one ragged mix at B = 8 -- one
           row at 32768 tokens, seven at 512 -- next to shared-count states with every row at 32768 and at 512
   python tools/softmax_decode_latency.py [--per-sequence] [--contexts 512,4096,32768] [--batches 1,8] [--rounds 7] [--steps 50]      (GPU)
Every step is captured with torch.cuda.graph after a warm-up and replayed; rounds alternate the routes; a round resets the
token count to the context, replays `steps` steps and is timed by the host clock around a device synchronise.  The cache rows
are random: the time does not depend on them.  Prints the median and min .. max over the rounds in microseconds per step."""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import efficient_attention as ea  # noqa: E402
from ea_harness.sequence import DecoderStack  # noqa: E402

warnings.simplefilter("ignore")
EMBED, HEADS, FFN, LAYERS, VOCAB = 1024, 8, 4096, 16, 32768
RECIPE = dict(window_size=128, chunk_size=8, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
              overlap_window=False)
DT = torch.bfloat16


def set_context(m, inc, ctx):
    """The state of attention module `m` as after `ctx` tokens: the device count and its host shadow (rows stay what they are)."""
    m._get_input_buffer(inc)["pos"].fill_(ctx)
    host = inc.get(m._incremental_state_id + ".kv_static") or m.get_incremental_state(inc, "attn_static")
    host["count"] = ctx


def captured(step):
    """step() warmed up on a side stream, then captured -> the graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g


def timed(routes, rounds, steps):
    """routes: name -> (reset(), graph) -> name -> (median, min, max) microseconds per replayed step."""
    times = {n: [] for n in routes}
    for _ in range(rounds):
        for n, (reset, g) in routes.items():
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                g.replay()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e6 / steps)
    return {n: (sorted(t)[len(t) // 2], min(t), max(t)) for n, t in times.items()}


def show(head, res, base):
    print(head + "  ".join("%s %.1f (%.1f .. %.1f) x%.2f" % (n, *res[n], res[n][0] / res[base][0]) for n in res), flush=True)


def kv_route(m, B, ctx, steps, x, splits):
    inc = {}
    m.init_kv_cache(inc, B, ctx + steps + 2, DT, "cuda", kv_splits=splits, hold_projections=True)
    m._get_input_buffer(inc)["kv"].normal_()
    reset = lambda: set_context(m, inc, ctx)                               # noqa: E731
    reset()
    g = captured(lambda: m(x, x, x, incremental_state=inc))
    return (reset, g), inc[m._incremental_state_id + ".kv_static"]["kv_splits"], m._get_input_buffer(inc)


def layer_rows(soft, ceva, B, ctx, a):
    x = 0.5 * torch.randn(1, B, EMBED, device="cuda", dtype=DT)
    d = EMBED // HEADS
    routes = {}
    routes["kv"], planned, buf = kv_route(soft, B, ctx, a.steps, x, 0)
    k, v = buf["kv"][:, 0, :, :ctx + 1], buf["kv"][:, 1, :, :ctx + 1]       # the cache rows a step at `ctx` reads

    def sdpa():
        qkv = F.linear(x.view(B, EMBED), buf["w_qkv"], buf["b_qkv"]).view(B, 3, HEADS, 1, d)
        out = F.scaled_dot_product_attention(qkv[:, 0], k, v)
        return F.linear(out.reshape(1, B, EMBED), buf["w_out"], buf["b_out"])
    routes["sdpa"] = (lambda: None, captured(sdpa))
    inc = {}
    ceva.init_rolling_decoding(inc, B, ctx + a.steps + 130, DT, "cuda", hold_projections=True)
    reset = lambda: set_context(ceva, inc, ctx)                            # noqa: E731
    reset()
    routes["ceva"] = (reset, captured(lambda: ceva(x, x, x, incremental_state=inc)))
    show("layer  B %d ctx %5d (P %2d): " % (B, ctx, planned), timed(routes, a.rounds, a.steps), "kv")
    sweep = {}
    for P in sorted({max(1, planned // 4), max(1, planned // 2), planned, min(64, planned * 2), min(64, planned * 4), 1}):
        sweep["P%d" % P] = kv_route(soft, B, ctx, a.steps, x, P)[0]
    show("         kv_splits sweep:   ", timed(sweep, a.rounds, a.steps), "P%d" % planned)


def stack_rows(B, ctx, a):
    tok = torch.randint(2, VOCAB, (1, B), device="cuda")
    routes = {}
    for name in ("softmax", "causal_eva"):
        torch.manual_seed(0)
        stack = DecoderStack(VOCAB, EMBED, FFN, HEADS, LAYERS, RECIPE, dropout=0.0, attn_name=name,
                             max_positions=ctx + a.steps + 256).cuda().eval()
        st = stack._make_decoding(B, ctx + a.steps + 130, DT, "cuda")
        mods = [layer.self_attn for layer in stack.layers]

        def reset(mods=mods, st=st):
            for m in mods:
                set_context(m, st.incremental, ctx)
        reset()
        with torch.no_grad():
            routes[name] = (reset, captured(lambda: stack.decode(tok, st)))
    show("stack  B %d ctx %5d:        " % (B, ctx), timed(routes, a.rounds, max(a.steps // 5, 4)), "softmax")


def prompt_rows(soft, B, T, rounds):
    x = 0.5 * torch.randn(T, B, EMBED, device="cuda", dtype=DT)
    inc = {}
    soft.init_kv_cache(inc, B, T, DT, "cuda", hold_projections=True)
    buf = soft._get_input_buffer(inc)
    d = EMBED // HEADS

    def kv():
        set_context(soft, inc, 0)
        return soft(x, x, x, incremental_state=inc)

    def sdpa():
        q, k, v = [t.permute(1, 2, 0, 3) for t in F.linear(x, buf["w_qkv"], buf["b_qkv"]).view(T, B, 3, HEADS, d).unbind(2)]
        out = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        return F.linear(out.permute(2, 0, 1, 3).reshape(T, B, EMBED), buf["w_out"], buf["b_out"])
    fns, times = dict(kv=kv, sdpa=sdpa), dict(kv=[], sdpa=[])
    for fn in fns.values():
        fn()
    for _ in range(rounds):
        for n, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e6 / 5)
    show("prompt B %d T %d (eager):   " % (B, T), {n: (sorted(t)[len(t) // 2], min(t), max(t)) for n, t in times.items()}, "kv")


def perseq_rows(soft, a):
    def route(ctxs, seq):
        """The layer's captured step on a state whose rows hold ctxs tokens (a shared-count state: ctxs[0] for all)."""
        B, inc = len(ctxs), {}
        x = 0.5 * torch.randn(1, B, EMBED, device="cuda", dtype=DT)
        soft.init_kv_cache(inc, B, max(ctxs) + a.steps + 2, DT, "cuda", hold_projections=True, per_sequence=seq)
        buf, host = soft._get_input_buffer(inc), inc[soft._incremental_state_id + ".kv_static"]
        buf["kv"].normal_()
        at = torch.tensor(ctxs if seq else ctxs[:1], dtype=torch.int32, device="cuda")

        def reset():
            buf["pos"].copy_(at)
            host["count"] = ctxs[0]
        reset()
        return reset, captured(lambda: soft(x, x, x, incremental_state=inc))
    for B in [int(v) for v in a.batches.split(",")]:
        for ctx in [int(v) for v in a.contexts.split(",")]:
            routes = {"shared": route([ctx] * B, False), "shared'": route([ctx] * B, False), "seq": route([ctx] * B, True)}
            show("per-seq B %d ctx %5d uniform:  " % (B, ctx), timed(routes, a.rounds, a.steps), "shared")
    mix = [32768] + [512] * 7
    routes = {"seq-mix": route(mix, True), "shared-32768": route([32768] * 8, False), "shared-512": route([512] * 8, False)}
    show("per-seq B 8 ragged 1 x 32768 + 7 x 512:  ", timed(routes, a.rounds, a.steps), "seq-mix")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", default="512,4096,32768")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-stack", action="store_true")
    ap.add_argument("--per-sequence", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("softmax_decode_latency.py measures on a GPU: none found")
    torch.manual_seed(0)
    soft = ea.CausalSoftmaxAttention(EMBED, HEADS).cuda().eval()
    ceva = ea.CausalEVAttention(EMBED, HEADS, self_attention=True, dropout=0.0, attn_args=argparse.Namespace(**RECIPE)).cuda().eval()
    print("microseconds per replayed 1-token step, bf16, median (min .. max) of %d rounds of %d steps" % (a.rounds, a.steps))
    if a.per_sequence:
        with torch.no_grad():
            perseq_rows(soft, a)
        return
    with torch.no_grad():
        for B in [int(v) for v in a.batches.split(",")]:
            for ctx in [int(v) for v in a.contexts.split(",")]:
                layer_rows(soft, ceva, B, ctx, a)
        for B in [int(v) for v in a.batches.split(",")]:
            prompt_rows(soft, B, 2048, a.rounds)
    if not a.no_stack:
        for B in [int(v) for v in a.batches.split(",")]:
            for ctx in [int(v) for v in a.contexts.split(",")]:
                stack_rows(B, ctx, a)


if __name__ == "__main__":
    main()
