"""Incremental decoding of CausalEVAttention at the LM layer (embed 1024, h 8, d 128, the wikitext-103 recipe: w = 128, chunks of
8, T5 bias, adaptive 'qk'):
   python tools/time_decode.py   (GPU).  Prints
 - ms per 1-token step at B = 1 and 8 after a context of 512 and 4096 tokens (64 and 512 landmarks), in bf16 autocast and in fp32
   (the position is reset before every step, so the context stays fixed; these steps close no chunk);
 - ms of one 512-token and one 2048-token prefill step on an empty state.
   python tools/time_decode.py --matrix-prompts   (GPU).  Prints the bf16 prefill steps on a STATIC state made without and with
   `matrix_prompts=True`, and a 16384-token prompt fed through a rolling state in pieces of 2048 at B = 1: ms of the whole
   step, and of its attn launches alone (device events around ea_ceva_sdecode_attn / _attn_mm), in alternating rounds.
Eager steps under no_grad, a warm-up, a device synchronise around every block, the median over the blocks."""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
import efficient_attention as ea  # noqa: E402

warnings.simplefilter("ignore")
EMBED, HEADS = 1024, 8
RECIPE = dict(window_size=128, chunk_size=8, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
              overlap_window=False)


def build():
    torch.manual_seed(0)
    m = ea.AttentionFactory.build_attention(
        "causal_eva", dict(embed_dim=EMBED, num_heads=HEADS, self_attention=True, dropout=0.0,
                           attn_args=argparse.Namespace(**RECIPE)))
    return m.cuda().eval()


def ctx(dtype):
    return torch.autocast("cuda", dtype=torch.bfloat16) if dtype == "bf16" else torch.autocast("cuda", enabled=False)


def blocks_ms(fn, per_block, blocks, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(blocks):
        t = time.perf_counter()
        for _ in range(per_block):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3 / per_block)
    return sorted(times)[len(times) // 2]


def step_ms(m, B, context, dtype, steps=50, blocks=5):
    x = torch.randn(context + 1, B, EMBED, device="cuda")
    state = {}
    m.init_incremental_state()
    with torch.no_grad(), ctx(dtype):
        m(x[:context], x[:context], x[:context], incremental_state=state)
        tok = x[context:context + 1]

        def one():
            m.set_incremental_state(state, "attn_pos", context)     # the same position every step: fixed context
            m(tok, tok, tok, incremental_state=state)
        return blocks_ms(one, steps, blocks, warmup=5)


def prefill_ms(m, B, T, dtype, blocks=3):
    x = torch.randn(T, B, EMBED, device="cuda")
    with torch.no_grad(), ctx(dtype):
        def one():
            m.init_incremental_state()
            m(x, x, x, incremental_state={})
        return blocks_ms(one, 1, blocks, warmup=1)


def static_prefill_ms(m, B, T, rolling, rounds=5):
    """(step ms, attn ms) of a T-token bf16 prompt on a static state (rolling: a ring fed in pieces of 2048) without / with
    matrix_prompts: the two states take turns, round by round; medians."""
    from efficient_attention import _native as nv
    x = torch.randn(T, B, EMBED, device="cuda")
    states, got = [], ([], [])
    for on in (False, True):
        st = {}
        if rolling:
            m.init_rolling_decoding(st, B, T, torch.bfloat16, "cuda", max_step_tokens=2048, matrix_prompts=on)
        else:
            m.init_static_decoding(st, B, T, torch.bfloat16, "cuda", matrix_prompts=on)
        states.append(st)
    real, spans = nv.call, []

    def timed(name, *a):
        if "sdecode_attn" not in name:
            return real(name, *a)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        real(name, *a)
        ev[1].record()
        spans.append(ev)
    nv.call = timed
    try:
        with torch.no_grad(), ctx("bf16"):
            for rnd in range(rounds + 1):                         # (round 0 warms up)
                for on, st in enumerate(states):
                    m._get_input_buffer(st)["pos"].zero_()
                    m.get_incremental_state(st, "attn_static")["count"] = 0
                    del spans[:]
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    m(x, x, x, incremental_state=st)
                    torch.cuda.synchronize()
                    if rnd:
                        got[on].append(((time.perf_counter() - t) * 1e3, sum(a.elapsed_time(b) for a, b in spans)))
    finally:
        nv.call = real
    med = lambda v: sorted(v)[len(v) // 2]                        # noqa: E731
    return [(med([g[0] for g in r]), med([g[1] for g in r])) for r in got]


def main_matrix():
    m = build()
    print("bf16 prompt step on a static state, ms: step (attn launches alone), without -> with matrix_prompts")
    for name, B, T, rolling in (("static", 1, 512, False), ("static", 8, 512, False), ("static", 1, 2048, False),
                                ("static", 8, 2048, False), ("rolling, pieces of 2048", 1, 16384, True)):
        (s0, a0), (s1, a1) = static_prefill_ms(m, B, T, rolling)
        print("%-24s B %d T %5d  %9.3f (%8.3f) -> %9.3f (%8.3f)" % (name, B, T, s0, a0, s1, a1), flush=True)


def main():
    if "--matrix-prompts" in sys.argv[1:]:
        return main_matrix()
    m = build()
    print("per-token step, ms (context -> landmarks)")
    print("%-6s %3s %12s %12s" % ("dtype", "B", "ctx 512 (64)", "ctx 4096 (512)"))
    for dtype in ("bf16", "fp32"):
        for B in (1, 8):
            a = step_ms(m, B, 512, dtype)
            b = step_ms(m, B, 4096, dtype)
            print("%-6s %3d %12.3f %12.3f" % (dtype, B, a, b), flush=True)
    print("prefill step on an empty state, ms")
    print("%-6s %3s %10s %10s" % ("dtype", "B", "T = 512", "T = 2048"))
    for dtype in ("bf16", "fp32"):
        for B in (1, 8):
            print("%-6s %3d %10.3f %10.3f" % (dtype, B, prefill_ms(m, B, 512, dtype), prefill_ms(m, B, 2048, dtype)), flush=True)


if __name__ == "__main__":
    main()
