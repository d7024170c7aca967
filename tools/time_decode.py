"""Incremental decoding of CausalEVAttention at the LM layer (embed 1024, h 8, d 128, the wikitext-103 recipe: w = 128, chunks of
8, T5 bias, adaptive 'qk'):
   python tools/time_decode.py   (GPU).  Prints
 - ms per 1-token step at B = 1 and 8 after a context of 512 and 4096 tokens (64 and 512 landmarks), in bf16 autocast and in fp32
   (the position is reset before every step, so the context stays fixed; these steps close no chunk);
 - ms of one 512-token and one 2048-token prefill step on an empty state.
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


def main():
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
