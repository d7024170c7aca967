"""The vocabulary cross-entropy as a training loss: forward + backward of two routes from rows x [M, K] and the fp32 master table
w [V, K] to (d x, d w), at the model's own workload (wikitext-103 LM layer: 18 x 512 = 9216 rows, K = 1024):
   1. ea_harness.vocab_loss.vocab_nll (C ABI 38): ea_vocab_score forward; per column chunk one ea_vocab_nll_grad and two
      ea_gemm_nt16 backward; no [M, V] tensor;
   2. the framework: F.linear on the 16-bit operands, .float(), F.cross_entropy, backward -- where it fits in memory.
   python tools/vocab_loss_latency.py [--shapes 9216x1024x32768,9216x1024x262144] [--rounds 3] [--reps 3] [--window-ms 200] [--dtype bf16] [--chunk-cols N]   (GPU)
Operands are seeded normal draws (x ~ N(0, 1), w ~ N(0, 1 / K)), not zeros; both routes get the same sum of the targets'
log-probabilities to differentiate.  Each route is warmed up twice at the shape it is timed at; a round times every route once,
between two device events, over at least `reps` calls and at least `window-ms` of work, and the rounds alternate the routes, so
that a drift of the machine shows as spread and not as a difference.  Per (shape, route): the median ms per forward + backward
over the rounds with the smallest and the largest, 8 M K V / time as TFLOP/s for route 1 (a logit pass forward, a logit pass and
two GEMMs backward) and 6 M K V / time for route 2 (three GEMMs), and the rise of torch.cuda.max_memory_allocated over one
forward + backward above the operands (x, w, targets).  There is no pass or fail on time: the figures go into DESIGN.md 4a."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from efficient_attention import _native as nv  # noqa: E402
from ea_harness.vocab_loss import vocab_nll  # noqa: E402


def operands(M, K, V, dtype):
    g = torch.Generator().manual_seed(M * 31 + V)
    x = torch.randn(M, K, generator=g).to(dtype).cuda().requires_grad_(True)
    w = torch.empty(V, K, dtype=torch.float32, device="cuda")
    for a in range(0, V, 32768):                          # (in pieces: no [V, K] fp32 tensor on the host)
        w[a:a + 32768] = (torch.randn(min(32768, V - a), K, generator=g) / K ** 0.5).cuda()
    targets = torch.randint(0, V, (M,), generator=g).cuda()
    return x, w.requires_grad_(True), targets


def route_ours(x, w, targets, dtype, chunk_cols):
    M, K = x.shape

    def call():
        x.grad = w.grad = None
        with torch.autocast("cuda", dtype=dtype, cache_enabled=False):
            logp = vocab_nll(x.view(M, 1, K), w, targets.view(M, 1), chunk_cols=chunk_cols)
        (-logp.sum()).backward()
    return call


def route_framework(x, w, targets, dtype):
    M, V = x.shape[0], w.shape[0]
    need = M * V * (2 + 4 + 4 + 2) * 1.15                 # the 16-bit logits, their fp32 copy, its gradient, the 16-bit gradient
    if need > torch.cuda.mem_get_info()[0]:
        return None

    def call():
        x.grad = w.grad = None
        F.cross_entropy(F.linear(x, w.to(dtype)).float(), targets, reduction="sum").backward()
    return call


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def peak_rise(call, x, w):
    x.grad = w.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="9216x1024x32768,9216x1024x262144")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--chunk-cols", type=int, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vocab_loss_latency.py times GPU kernels: no GPU here, nothing measured")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    print("BM, BN, SL =", nv.vocab_score_tiles(), "| device:", torch.cuda.get_device_name(0))
    for shape in a.shapes.split(","):
        M, K, V = (int(s) for s in shape.split("x"))
        x, w, targets = operands(M, K, V, dtype)
        cc = nv.lib().ea_vocab_nll_chunk(M, V) if a.chunk_cols is None else a.chunk_cols
        print("%s chunk_cols %d (%d chunks), ea_vocab_nll_ws %.1f MiB, [M, V] in 16 bits %.1f MiB"
              % (shape, cc, -(-V // cc), nv.lib().ea_vocab_nll_ws(M, K, V, cc) / 2 ** 20, M * V * 2 / 2 ** 20))
        routes = [("vocab_nll", route_ours(x, w, targets, dtype, a.chunk_cols), 8.0), ("framework", route_framework(x, w, targets, dtype), 6.0)]
        grads, times = {}, {name: [] for name, _, _ in routes}
        for name, call, _ in routes:
            if call is None:
                print("%s %-10s does not fit in the free device memory: not measured" % (shape, name))
                continue
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            grads[name] = (x.grad.float().clone(), w.grad.clone())
        reps = {name: max(a.reps, min(1000, int(a.window_ms / timed(call, 1)) + 1)) for name, call, _ in routes if call is not None}
        for _ in range(a.rounds):
            for name, call, _ in routes:
                if call is not None:
                    times[name].append(timed(call, reps[name]))
        for name, call, passes in routes:
            if call is None:
                continue
            t = sorted(times[name])
            med = t[len(t) // 2]
            print("%s %-10s fwd+bwd median %9.3f ms (min %9.3f, max %9.3f; %d calls a window) | %6.1f TFLOP/s | peak above the operands %8.1f MiB"
                  % (shape, name, med, t[0], t[-1], reps[name], passes * M * K * V / (med * 1e-3) / 1e12, peak_rise(call, x, w) / 2 ** 20))
        if len(grads) == 2:
            for i, what in enumerate(("d x", "d w")):
                mine, theirs = grads["vocab_nll"][i], grads["framework"][i]
                print("%s %s: |ours - framework| / |framework| = %.3e" % (shape, what, ((mine - theirs).norm() / theirs.norm()).item()))
        del x, w, targets, routes, grads
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
