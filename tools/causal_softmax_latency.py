"""Forward + backward time of one causal softmax attention layer (embed 1024, h 8, d 128, bf16 autocast) on the causal streaming
kernels of csrc/ea_softmax_causal.hip, against three things on the same inputs:
   dense   the same layer with the core on the dense ea_softmax_attn_* kernels (the whole square: another function, the cost only)
   sdpa    F.scaled_dot_product_attention(is_causal=True) around the same projections
   ceva    the CausalEVAttention layer of bench.py's LM arguments (window 128, chunks of 8, T5 bias, adaptive 'qk')
   python tools/causal_softmax_latency.py [--shapes 18x512,4x2048,2x4096] [--rounds 7] [--steps 10]      (GPU)
Rounds alternate the four routes; a round times `steps` training steps (forward, backward of a fixed dy) by the host clock around
the steps and a device synchronise, after a warm-up of every route; modules in eval mode (no dropout, no noise).  Prints per
shape the median and the min .. max over the rounds of each route in ms per step and each route's ratio to the causal kernels."""
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
from efficient_attention import _ops  # noqa: E402

warnings.simplefilter("ignore")
EMBED, HEADS = 1024, 8
RECIPE = dict(window_size=128, chunk_size=8, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
              overlap_window=False)
ROUTES = ("causal", "dense", "sdpa", "ceva")


def layer_forward(m, x, route):
    """The softmax module's forward with its core swapped: the causal kernels, the dense kernels, or the framework's SDPA."""
    if route == "causal":
        return m(x, x, x)[0]
    T, B, C = x.shape
    qkv5 = m._project(x).transpose(0, 1)                          # [B, T, 3, h, d]
    if route == "dense":
        out = _ops.SoftmaxAttnFn.apply(qkv5, None)
    else:
        q, k, v = [qkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
        out = F.scaled_dot_product_attention(q, k, v, is_causal=True).permute(0, 2, 1, 3)
    return _ops.linear(out.transpose(0, 1).reshape(T, B, C), m.out_proj)


def train_step(mods, x, dy, route):
    m = mods["ceva" if route == "ceva" else "softmax"]
    m.zero_grad(set_to_none=True)
    x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x, x, x)[0] if route == "ceva" else layer_forward(m, x, route)
    y.backward(dy)


def core_step(fn, qkv5, dout):
    qkv5.grad = None
    fn.apply(qkv5, None).backward(dout)


def core_times(B, T, rounds, steps):
    """The cores alone on one fused qkv tensor: _ops.CausalSoftmaxAttnFn against the dense _ops.SoftmaxAttnFn -> medians (ms)."""
    d = EMBED // HEADS
    qkv5 = torch.randn(B, T, 3, HEADS, d, device="cuda").to(torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B, T, HEADS, d, device="cuda").to(torch.bfloat16)
    fns = dict(causal=_ops.CausalSoftmaxAttnFn, dense=_ops.SoftmaxAttnFn)
    for fn in fns.values():
        core_step(fn, qkv5, dout)
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                core_step(fn, qkv5, dout)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e3 / steps)
    return {n: (sorted(t)[len(t) // 2], min(t), max(t)) for n, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="18x512,4x2048,2x4096", help="comma-separated BxT")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    torch.manual_seed(0)
    mods = dict(softmax=ea.CausalSoftmaxAttention(EMBED, HEADS).cuda().eval(),
                ceva=ea.CausalEVAttention(EMBED, HEADS, self_attention=True, dropout=0.0,
                                          attn_args=argparse.Namespace(**RECIPE)).cuda().eval())
    print("ms per training step of one layer (forward + backward), bf16 autocast, %d rounds of %d steps" % (a.rounds, a.steps))
    for shape in a.shapes.split(","):
        B, T = [int(v) for v in shape.split("x")]
        x = (0.5 * torch.randn(T, B, EMBED, device="cuda")).requires_grad_(True)
        dy = torch.randn(T, B, EMBED, device="cuda").to(torch.bfloat16)
        for _ in range(2):
            for route in ROUTES:
                train_step(mods, x, dy, route)
        torch.cuda.synchronize()
        times = {route: [] for route in ROUTES}
        for _ in range(a.rounds):
            for route in ROUTES:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    train_step(mods, x, dy, route)
                torch.cuda.synchronize()
                times[route].append((time.perf_counter() - t0) * 1e3 / a.steps)
        med = {r: sorted(t)[len(t) // 2] for r, t in times.items()}
        print("B %2d T %5d: " % (B, T) + "  ".join("%s %.3f (%.3f .. %.3f) x%.2f" % (r, med[r], min(times[r]), max(times[r]),
                                                                                  med[r] / med["causal"]) for r in ROUTES), flush=True)
        ct = core_times(B, T, a.rounds, a.steps)
        print("            cores alone: " + "  ".join("%s %.3f (%.3f .. %.3f)" % ((n,) + ct[n]) for n in ct)
              + "  dense / causal %.2f" % (ct["dense"][0] / ct["causal"][0]), flush=True)


if __name__ == "__main__":
    main()
