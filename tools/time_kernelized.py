"""Captured fwd+bwd step of KernelizedAttention's feature maps at the cfg3 geometry (x = [32,28,28,192], h = 3, bf16 autocast)
next to favorp on the exact-fp32 Performer core:
   python tools/time_kernelized.py   (GPU).  Prints F (features after cos weighting), ms per captured step (median of 5
replays x 20 steps) and the ratio to favorp."""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
import efficient_attention as ea  # noqa: E402
from efficient_attention import _kernelized  # noqa: E402

warnings.simplefilter("ignore")
SHAPE = (32, 28, 28, 192)
CASES = [  # (label, proj_method, approx_attn_dim, cos_weighting, sample_scheme)
    ("favorp (Performer f32 core)", "favorp", 64, False, "fixed"),
    ("favorp + cos", "favorp", 64, True, "fixed"),
    ("favorp learnable", "favorp", 64, False, "learnable"),
    ("relu", "relu", 64, False, "fixed"),
    ("relu + cos", "relu", 64, True, "fixed"),
    ("relu learnable", "relu", 64, False, "learnable"),
    ("fourier m=32", "fourier", 32, False, "fixed"),
    ("fourier m=64", "fourier", 64, False, "fixed"),
    ("fourier m=64 + cos", "fourier", 64, True, "fixed"),
    ("relu-only", "relu-only", 64, False, "default"),
    ("sigmoid-only", "sigmoid-only", 64, False, "default"),
    ("relu-only + cos", "relu-only", 64, True, "default"),
    ("dpfp nu=1", "dpfp", 128, False, "default"),
    ("dpfp nu=2", "dpfp", 256, False, "default"),
]


def captured_ms(mod, x, g, steps=20, reps=5):
    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(x)
        y.backward(g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / steps)
    return sorted(times)[len(times) // 2]


def main():
    base = None
    print("%-30s %5s %10s %8s" % ("map", "F", "ms/step", "x favorp"))
    for label, pm, m, cos, scheme in CASES:
        torch.manual_seed(0)
        mod = ea.KernelizedAttention(dim=SHAPE[-1], num_heads=3, approx_attn_dim=m, proj_method=pm, cos_weighting=cos,
                                     sample_scheme=scheme).cuda().train()
        x = torch.randn(*SHAPE, device="cuda", requires_grad=True)
        g = torch.randn(*SHAPE, device="cuda", dtype=torch.bfloat16)
        ms = captured_ms(mod, x, g)
        base = ms if base is None else base
        F = _kernelized.feature_count(pm, m, 64, cos)
        print("%-30s %5d %10.3f %8.2f" % (label, F, ms, ms / base), flush=True)
        del mod, x, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
