"""Forward + backward time of one CausalEVAttention layer trained past 64 chunks (embed 1024, h 8, d 128, w 128, chunks of 8, T5
bias, adaptive 'qk', bf16 autocast), with the landmark columns on the 16-bit kernels of csrc/ea_ceva_lm.hip
(_ops.USE_CEVA_LONG = True) and on the fp32 gathered-attention route they replace (False), on the same module and inputs:
   python tools/ceva_long_latency.py [--shapes 4x2048,2x4096] [--rounds 7] [--steps 10]      (GPU)
Rounds alternate the two routes; a round times `steps` training steps (forward, backward of a fixed dy) by the host clock around
the steps and a device synchronise, after a warm-up of both routes; the module is in eval mode (no omega noise, no dropout) so
that the two routes compute the same function.  Prints per shape the median and the min .. max over the
rounds of each route in ms per step, their ratio, and max |y_on - y_off| / max |y_off| of the two routes' outputs."""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
import efficient_attention as ea  # noqa: E402
from efficient_attention import _ops  # noqa: E402

warnings.simplefilter("ignore")
EMBED, HEADS = 1024, 8
RECIPE = dict(window_size=128, chunk_size=8, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
              overlap_window=False)


def train_step(m, x, dy, on):
    _ops.USE_CEVA_LONG = on
    m.zero_grad(set_to_none=True)
    x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x, x, x)[0]
    y.backward(dy)
    return y.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x2048,2x4096", help="comma-separated BxT")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    torch.manual_seed(0)
    m = ea.AttentionFactory.build_attention(
        "causal_eva", dict(embed_dim=EMBED, num_heads=HEADS, self_attention=True, dropout=0.0,
                           attn_args=argparse.Namespace(**RECIPE))).cuda().eval()
    was = _ops.USE_CEVA_LONG
    print("ms per training step of one layer (forward + backward), bf16 autocast, %d rounds of %d steps" % (a.rounds, a.steps))
    for shape in a.shapes.split(","):
        B, T = [int(v) for v in shape.split("x")]
        x = (0.5 * torch.randn(T, B, EMBED, device="cuda")).requires_grad_(True)
        dy = torch.randn(T, B, EMBED, device="cuda").to(torch.bfloat16)
        ys = {on: train_step(m, x, dy, on) for on in (True, False)}
        for on in (True, False):
            train_step(m, x, dy, on)
        torch.cuda.synchronize()
        times = {True: [], False: []}
        for _ in range(a.rounds):
            for on in (True, False):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    train_step(m, x, dy, on)
                torch.cuda.synchronize()
                times[on].append((time.perf_counter() - t0) * 1e3 / a.steps)
        med = {on: sorted(t)[len(t) // 2] for on, t in times.items()}
        diff = ((ys[True].float() - ys[False].float()).abs().max() / ys[False].float().abs().max()).item()
        print("B %d T %5d (%d chunks): 16-bit %.3f (%.3f .. %.3f)  fp32 route %.3f (%.3f .. %.3f)  ratio %.2f  max|dy|/max|y| %.1e"
              % (B, T, T // RECIPE["chunk_size"], med[True], min(times[True]), max(times[True]), med[False], min(times[False]),
                 max(times[False]), med[False] / med[True], diff), flush=True)
    _ops.USE_CEVA_LONG = was


if __name__ == "__main__":
    main()
