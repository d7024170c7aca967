"""Per-token latency of CausalEVAttention decoding at the wikitext-103 LM geometry (embed 1024, h 8, d 128, w 128, chunks of 8,
T5 bias, adaptive 'qk'), 16 stacked residual attention layers (x + attn(x), no FFN), bf16 autocast, in three modes:
 - dynamic: the incremental state of `_decode` (host token count, two decode launches per layer step);
 - static:  `init_static_decoding`, the same step run eagerly (four decode launches per layer step);
 - graph:   that static step over all 16 layers captured once with torch.cuda.graph and replayed.
   python tools/ceva_decode_latency.py [--context 512] [--steps 64]   (GPU)
A 1-token step after a prefill of `context` tokens; a warm-up, then the median over 5 blocks of `steps` tokens, each block
timed by the host clock around its steps and a device synchronise.  The rows of the three modes are compared (bitwise)."""
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
EMBED, HEADS, LAYERS = 1024, 8, 16
RECIPE = dict(window_size=128, chunk_size=8, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
              overlap_window=False)


def build():
    torch.manual_seed(0)
    return [ea.AttentionFactory.build_attention(
        "causal_eva", dict(embed_dim=EMBED, num_heads=HEADS, self_attention=True, dropout=0.0,
                           attn_args=argparse.Namespace(**RECIPE))).cuda().eval() for _ in range(LAYERS)]


def step(mods, states, x):
    for m, st in zip(mods, states):
        x = x + m(x, x, x, incremental_state=st)[0]
    return x


def run(mods, mode, B, context, steps, blocks=5, warmup=4):
    """-> (median ms per token, the rows of every timed step)."""
    n_tok = context + warmup + 1 + blocks * steps
    torch.manual_seed(1)
    x = 0.5 * torch.randn(n_tok, B, EMBED, device="cuda")
    states = []
    for m in mods:
        st = {}
        m.init_incremental_state()
        if mode != "dynamic":
            m.init_static_decoding(st, B, n_tok, torch.bfloat16, "cuda")
        states.append(st)
    rows, times = [], []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        step(mods, states, x[:context])
        t = context
        xin = x[t:t + 1].clone()
        if mode == "graph":
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step(mods, states, xin)                       # the token at `context`, eager on a side stream
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                yout = step(mods, states, xin)

            def one(tok):
                xin.copy_(x[tok:tok + 1])
                g.replay()
                return yout.clone()
        else:
            step(mods, states, xin)

            def one(tok):
                return step(mods, states, x[tok:tok + 1])
        t += 1
        for _ in range(warmup):
            one(t)
            t += 1
        torch.cuda.synchronize()
        for _ in range(blocks):
            t0 = time.perf_counter()
            for _ in range(steps):
                rows.append(one(t))
                t += 1
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / steps)
    return sorted(times)[len(times) // 2], torch.cat(rows, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--steps", type=int, default=64)
    a = ap.parse_args()
    mods = build()
    print("ms per token, %d layers, bf16, context %d" % (LAYERS, a.context))
    print("%3s %10s %10s %10s  %s" % ("B", "dynamic", "static", "graph", "rows equal (static, graph vs dynamic)"))
    for B in (1, 8):
        res = {mode: run(mods, mode, B, a.context, a.steps) for mode in ("dynamic", "static", "graph")}
        ref = res["dynamic"][1]
        same = [torch.equal(res[mode][1], ref) for mode in ("static", "graph")]
        print("%3d %10.3f %10.3f %10.3f  %s" % (B, res["dynamic"][0], res["static"][0], res["graph"][0], same), flush=True)


if __name__ == "__main__":
    main()
