"""Teacher-forced scoring under the wikitext-103 recipe's adaptive softmax (V = 267744, cutoffs 20000 / 60000, band widths
1024 / 256 / 64), timed at the model's own workload (18 x 512 = 9216 rows of 1024 channels, bf16), three routes to the targets'
log-probabilities:
   1. ea_adaptive_score (C ABI 33): one call -- route, head pass, per tail a gathered projection and a tail pass, combine;
   2. the torch restatement, AdaptiveSoftmax.get_log_prob(x, target) on the same 16-bit operands: what the reference runs;
   3. ea_vocab_score on a plain [V, 1024] table: what the stand-in (a plain tied embedding) costs today.
   python tools/adaptive_score_latency.py [--rows 9216] [--rounds 3] [--reps 5] [--window-ms 200] [--dtype bf16] [--only NAME]   (GPU)
Two target draws: every target in the head, and targets with shares 80 / 12 / 8 % per band.  The timing method is
tools/vocab_score_latency.py's: seeded normal operands, two warm-up calls per route, rounds that alternate the routes, each
window at least `reps` calls and `window-ms` of work between two device events; the median, smallest and largest ms per call.
--only adaptive|torch|plain runs a single route (for a kernel trace of route 1 by itself)."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
from efficient_attention import _native as nv  # noqa: E402
from ea_harness.adaptive import AdaptiveInput, AdaptiveSoftmax  # noqa: E402
from ea_harness.sequence import AdaptiveTables  # noqa: E402
from vocab_score_latency import operands, route_score, timed  # noqa: E402

C, V, CUTOFF, FACTOR = 1024, 267744, [20000, 60000], 4


def targets_for(M, shares, seed):
    g = torch.Generator().manual_seed(seed)
    cut = [0] + CUTOFF + [V]
    band = torch.multinomial(torch.tensor(shares), M, replacement=True, generator=g)
    lo, hi = torch.tensor(cut[:-1])[band], torch.tensor(cut[1:])[band]
    return (lo + (torch.rand(M, generator=g) * (hi - lo)).long()).clamp(max=V - 1).cuda()


def route_adaptive(x, tables, targets):
    M, n = x.shape[0], len(tables.dims)
    cut, dims = nv.host_array(ctypes.c_int64, tables.cutoff), nv.host_array(ctypes.c_int32, tables.dims)
    nbytes = nv.lib().ea_adaptive_score_ws(M, n, cut, dims)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    logp = torch.empty(M, dtype=torch.float32, device="cuda")
    proj = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tables.proj])
    tabs = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tables.tables])

    def call():
        nv.call("ea_adaptive_score", M, C, n, cut, dims, nv.ptr(x), nv.io_dtype(x), C, nv.ptr(targets), nv.ptr(tables.head),
                nv.io_dtype(tables.head), proj, tabs, nv.ptr(ws), nbytes, nv.ptr(logp), None, nv.stream())
        return logp
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=9216)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--only", default=None, choices=["adaptive", "torch", "plain"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_score_latency.py times GPU kernels: no GPU here, nothing measured")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    M = a.rows
    print("BM, BN, SL =", nv.vocab_score_tiles(), "| device:", torch.cuda.get_device_name(0))
    torch.manual_seed(0)
    with torch.device("cuda"):
        inp = AdaptiveInput(V, 1, C, FACTOR, C, list(CUTOFF))
        sm = AdaptiveSoftmax(V, C, list(CUTOFF), 0.0, FACTOR, inp, True).to(dtype).eval()
    tables = AdaptiveTables(sm, dtype, "cuda")
    x, w, _ = operands(M, C, V, dtype)
    for draw, shares in (("all head", [1.0, 0.0, 0.0]), ("80/12/8", [0.80, 0.12, 0.08])):
        targets = targets_for(M, shares, 7)

        def torch_route():
            with torch.no_grad():
                return sm.get_log_prob(x, targets)
        plain = route_score(x, w, targets)
        routes = [("adaptive", "ea_adaptive_score", route_adaptive(x, tables, targets)),
                  ("torch", "torch get_log_prob", torch_route),
                  ("plain", "ea_vocab_score [V, 1024]", lambda: plain()[1])]
        routes = [r for r in routes if a.only in (None, r[0])]
        results, times = {}, {}
        for key, name, call in routes:
            for _ in range(2):
                out = call()
            torch.cuda.synchronize()
            results[key], times[key] = out.float().clone(), []
        reps = {key: max(a.reps, min(1000, int(a.window_ms / timed(call, 1)) + 1)) for key, _, call in routes}
        for _ in range(a.rounds):
            for key, _, call in routes:
                times[key].append(timed(call, reps[key]))
        for key, name, _ in routes:
            t = sorted(times[key])
            print("%d rows, targets %-8s %-26s median %8.3f ms (min %8.3f, max %8.3f; %d calls a window)"
                  % (M, draw, name, t[len(t) // 2], t[0], t[-1], reps[key]))
        if "adaptive" in results and "torch" in results:
            print("%d rows, targets %-8s largest |ea_adaptive_score - torch| %.3e (the torch route keeps h in its own rounding)"
                  % (M, draw, (results["adaptive"] - results["torch"]).abs().max().item()))


if __name__ == "__main__":
    main()
