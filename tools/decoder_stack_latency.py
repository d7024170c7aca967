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
For a table, run the modes alternately in processes of their own, at least three times each.

--generate times the whole captured greedy step of `DecoderStack.generate` instead -- embedding, positions, 16 layers, the pick
of the next token and its write-back into the step's static input -- on held weights, replayed with nothing fed from the host:
   --hold-vocab 1: the pick is `next_tokens` (ea_ceva_sdecode_vocab_argmax on the 16-bit table the state holds);
   --hold-vocab 0: the pick is `logits(y).argmax(-1)` and `tok_in.copy_`, the framework's cast, GEMM and argmax.
   python tools/decoder_stack_latency.py --generate --hold-vocab 0|1 [--vocab 32768|262144] [--root CHECKOUT]       (GPU)
One line per batch: the median ms per token over the blocks, their smallest and largest, and the pick alone (a captured graph of
the pick on one row set, replayed) as us and as GB/s on the 2 V C bytes of a 16-bit table.  --root names the checkout whose
package is timed (default: this one; it needs its library built: `python CHECKOUT/efficient-attention_amd/build.py`); where that package does not know `hold_vocab` -- a checkout of an earlier commit --
--hold-vocab 1 is reported as unavailable and the plain pick is timed, so that the same command line serves both.

--generate --sample K,P,T times the captured SAMPLED step (top_k, top_p, temperature) on a held table:
   a package with `DecoderStack.init_sampling`: the pick is `sample_tokens` (ea_ceva_sdecode_vocab_sample; device counters);
   a package without it (--root an earlier checkout): the framework sampler, written with that checkout's interface --
       `next_tokens(rows, state, return_logits=True)`, then torch.topk, torch.softmax at the temperature, torch.multinomial
       and `tok_in.copy_`, all inside the capture (no nucleus cut: fewer launches than a full equivalent, in its favour).
   python tools/decoder_stack_latency.py --generate --sample 40,0.9,1.0 [--vocab 32768|262144] [--root CHECKOUT]   (GPU)

--generate --hold-vocab 1 --logprobs times the captured greedy step that also writes the token's log-probability (ABI 28):
   --logprobs (= --logprobs native): the pick is `token_logprobs` into static buffers (ea_ceva_sdecode_vocab_logprob);
   --logprobs framework: the yardstick on this same tree, inside the capture -- `next_tokens(rows, state, return_logits=True)`,
       torch.logsumexp over the fp32 [B, V] logits, a gather of the token's logit and the subtraction.
   Without --logprobs the same command line times the greedy held step alone: what the feature costs.
   python tools/decoder_stack_latency.py --generate --hold-vocab 1 --logprobs [native|framework] [--vocab 32768|262144]   (GPU)"""
import argparse
import os
import sys
import time
import warnings

_root = argparse.ArgumentParser(add_help=False)           # --root decides where the imports below come from
_root.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(_root.parse_known_args()[0].root)
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
from ea_harness.sequence import DecoderStack, wikitext103_decoder  # noqa: E402

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


def run_generate(stack, B, context, hold_vocab, steps, blocks=5, warmup=4, sample=None, logprobs=None):
    """The captured greedy step (sample = (top_k, top_p, temperature): the sampled step) replayed -> (block times in ms per
    token, pick alone in us, decoding_state_nbytes)."""
    n_tok = context + 2 + warmup + blocks * steps
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(2, stack.embed_tokens.num_embeddings, (context, B), generator=g).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        opt = dict(hold_vocab=True) if hold_vocab else {}
        state = stack.init_decoding(B, n_tok, torch.bfloat16, "cuda", rolling=True, hold_weights=True, **opt)
        for a in range(0, context, WINDOW):
            y = stack.decode(tokens[a:min(a + WINDOW, context)], state)
        y = y[-1:].clone()
        native = sample is not None and hasattr(stack, "init_sampling")
        if native:
            stack.init_sampling(state, 1234, sample[0], sample[1], sample[2])
        lp = torch.zeros((1, B), dtype=torch.float32, device="cuda")
        if logprobs == "native":
            stack.init_logprobs(state)
            if hasattr(state, "pick"):                          # generate's own pick: it writes the scorer's static buffers
                lp_pick = state.pick(stack, B, return_logprobs=True)
            else:                                               # (a --root from before ea_harness/token_pick.py)
                def lp_pick(rows, out):
                    stack._logprob_pick(rows, state, None, out, state.scorer.logp[:B].view(1, B), state.scorer.lse[:B].view(1, B))

        def pick(rows, out):
            if logprobs == "native":
                lp_pick(rows, out)
            elif logprobs == "framework":
                _, logits = stack.next_tokens(rows, state, out=out, return_logits=True)
                lp.copy_(logits.gather(2, out.unsqueeze(2)).squeeze(2) - torch.logsumexp(logits, -1))
            elif native:
                stack.sample_tokens(rows, state, out=out)
            elif sample is not None:                           # the framework sampler on the fp32 logits handed back
                _, logits = stack.next_tokens(rows, state, return_logits=True)
                val, idx = torch.topk(logits[0], sample[0], dim=-1)
                j = torch.multinomial(torch.softmax(val / sample[2], -1), 1)
                out.copy_(idx.gather(1, j).t())
            elif hold_vocab:
                stack.next_tokens(rows, state, out=out)
            else:
                out.copy_(stack.logits(rows).argmax(-1))
        tok_in = torch.zeros((1, B), dtype=torch.long, device="cuda")
        pick(y, tok_in)

        def step():
            pick(stack.decode(tok_in, state), tok_in)

        def captured(fn):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()                                           # eager on a side stream: the warm-up
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            return graph

        def timed(graph):
            for _ in range(warmup):
                graph.replay()
            torch.cuda.synchronize()
            times = []
            for _ in range(blocks):
                t0 = time.perf_counter()
                for _ in range(steps):
                    graph.replay()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3 / steps)
            return times
        times = timed(captured(step))
        if stack.decoding_overflowed(state):
            raise RuntimeError("the decoding state overflowed")
        scratch = torch.zeros_like(tok_in)
        alone = timed(captured(lambda: pick(y, scratch)))
        nbytes = stack.decoding_state_nbytes(state)
    return times, sorted(alone)[len(alone) // 2] * 1e3, nbytes


def main_generate(a):
    known = hasattr(DecoderStack, "next_tokens")
    sample = None
    if a.sample:
        k, p, t = a.sample.split(",")
        sample = (int(k), float(p), float(t))
        if not known:
            raise SystemExit("--sample needs a package with hold_vocab (next_tokens(return_logits=True) is its yardstick)")
        a.hold_vocab = 1
        print("sampled step, top_k %d, top_p %g, temperature %g: %s" % (sample + (
            "sample_tokens (ea_ceva_sdecode_vocab_sample)" if hasattr(DecoderStack, "init_sampling") else
            "the framework sampler (next_tokens(return_logits=True), topk, softmax, multinomial, copy_)",)))
    hold_vocab = a.hold_vocab == 1 and known
    if a.logprobs:
        if sample is not None or not hold_vocab or not hasattr(DecoderStack, "init_logprobs"):
            raise SystemExit("--logprobs times the greedy step on a held table (--hold-vocab 1, no --sample) of a package "
                             "with init_logprobs")
        print("greedy step with the token's log-probability: %s" % (
            "token_logprobs (ea_ceva_sdecode_vocab_logprob)" if a.logprobs == "native" else
            "the framework route (next_tokens(return_logits=True), logsumexp, gather, sub, copy_)"))
    if a.hold_vocab == 1 and not known:
        print("the package under %s does not know hold_vocab: timing its plain pick (logits, argmax, copy_)" % ROOT)
    torch.manual_seed(0)
    stack = wikitext103_decoder(vocab=a.vocab, max_positions=a.context + 1024).cuda().eval()
    V, C = stack.embed_tokens.weight.shape
    print("ms per token, wikitext103_decoder (%d layers, vocab %d), bf16, rolling states, held weights, context %d, the captured "
          "greedy step replayed; package %s" % (LAYERS, V, a.context, ROOT))
    for B in [int(b) for b in a.batches.split(",")]:
        times, pick_us, nbytes = run_generate(stack, B, a.context, hold_vocab, a.steps, sample=sample, logprobs=a.logprobs or None)
        print("B %2d  hold_vocab=%-5s  %8.3f ms per token (blocks %.3f .. %.3f)  pick alone %8.1f us = %7.1f GB/s on 2 V C bytes"
              "  state %d bytes" % (B, hold_vocab, sorted(times)[len(times) // 2], min(times), max(times), pick_us,
                                    2.0 * V * C / (pick_us * 1e-6) / 1e9, nbytes), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=512, help="tokens before the timed steps; DESIGN.md 4a uses 512 and 4096")
    ap.add_argument("--batches", default="1,8", help="comma-separated batch sizes")
    ap.add_argument("--hold", default="both", choices=["0", "1", "both"])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--generate", action="store_true", help="time the whole captured greedy step (see the module docstring)")
    ap.add_argument("--hold-vocab", type=int, default=1, choices=[0, 1], help="with --generate: the pick on the held table")
    ap.add_argument("--vocab", type=int, default=32768, help="with --generate: rows of the vocabulary table")
    ap.add_argument("--sample", default="", help="with --generate: K,P,T -- time the sampled step (see the module docstring)")
    ap.add_argument("--logprobs", nargs="?", const="native", default="", choices=["native", "framework"],
                    help="with --generate --hold-vocab 1: the step also writes the token's log-probability")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is timed (default: this one)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_stack_latency.py needs a GPU: a latency is measured on one or not at all")
    if a.generate:
        return main_generate(a)
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
