"""Per-token latency of the causal-EVA decoder stack (ea_harness.sequence.wikitext103_decoder: embed 1024, ffn 4096, 8 heads,
16 pre-norm layers, window 128, chunks of 8, T5 bias, adaptive 'qk'), bf16 autocast: ONE captured single-token `decode` step
(embedding, positions, 16 layers; no logits -- the output projection is the same work in both modes) replayed on rolling states,
   hold_weights=True:  every layer's q/k/v/out projections on ea_ceva_sdecode_linear and its feed-forward on two
                       ea_ceva_sdecode_linear_fused launches, over 16-bit weights the state holds;
   hold_weights=False: the yardstick -- the layer's own nn.Linear modules under autocast (framework kernels that cast the fp32
                       masters on every replay), which is what a user of the attention alone would write around it.
   python tools/decoder_stack_latency.py [--context 512|4096] [--batches 1,8] [--hold 0|1|both] [--steps 64]      (GPU)
After a prefill of `context` tokens fed in pieces of one window: a warm-up step on a side stream, the capture, 4 replays, then
the median over 5 blocks of `steps` replayed tokens, each block timed by the host clock around its replays and a device
synchronise.  One line per (batch, mode): ms per token and ms per token and layer.  With --hold both the two modes run one after the
other in this process and the largest difference of their rows is printed (rounding: 16-bit weights, other summation orders).
For a table, run the modes alternately in processes of their own, at least three times each."""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
from ea_harness.sequence import wikitext103_decoder  # noqa: E402

warnings.simplefilter("ignore")
WINDOW, LAYERS = 128, 16


def run(stack, B, context, hold, steps, blocks=5, warmup=4):
    """-> (median ms per token, rows of the timed steps [blocks * steps, B, C], decoding_state_nbytes)."""
    n_tok = context + 1 + warmup + blocks * steps
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(2, stack.embed_tokens.num_embeddings, (n_tok, B), generator=g).cuda()
    rows, times = [], []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        state = stack.init_decoding(B, n_tok, torch.bfloat16, "cuda", rolling=True, hold_weights=hold)
        for a in range(0, context, WINDOW):
            stack.decode(tokens[a:min(a + WINDOW, context)], state)
        t = context
        xin = tokens[t:t + 1].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            stack.decode(xin, state)                          # the token at `context`, eager on a side stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yout = stack.decode(xin, state)
        t += 1

        def one(tok):
            xin.copy_(tokens[tok:tok + 1])
            graph.replay()
            return yout.clone()
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
        if stack.decoding_overflowed(state):
            raise RuntimeError("the decoding state overflowed")
        nbytes = stack.decoding_state_nbytes(state)
    return sorted(times)[len(times) // 2], torch.cat(rows, 0), nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=512, help="tokens before the timed steps; DESIGN.md 4a uses 512 and 4096")
    ap.add_argument("--batches", default="1,8", help="comma-separated batch sizes")
    ap.add_argument("--hold", default="both", choices=["0", "1", "both"])
    ap.add_argument("--steps", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_stack_latency.py needs a GPU: a latency is measured on one or not at all")
    torch.manual_seed(0)
    stack = wikitext103_decoder(max_positions=a.context + 1024).cuda().eval()
    modes = {"0": [False], "1": [True], "both": [False, True]}[a.hold]
    print("ms per token, wikitext103_decoder (%d layers), bf16, rolling states, context %d, 1-token replayed decode step"
          % (LAYERS, a.context))
    for B in [int(b) for b in a.batches.split(",")]:
        got = {}
        for hold in modes:
            ms, rows, nbytes = run(stack, B, a.context, hold, a.steps)
            got[hold] = rows
            print("B %2d  hold_weights=%-5s  %8.3f ms per token  %7.1f us per layer  state %d bytes"
                  % (B, hold, ms, ms * 1e3 / LAYERS, nbytes), flush=True)
        if len(got) == 2:
            d = (got[True].float() - got[False].float()).abs().max().item()
            print("B %2d  max |rows held - rows plain| %.3e of max |rows| %.3e" % (B, d, got[False].float().abs().max().item()),
                  flush=True)


if __name__ == "__main__":
    main()
