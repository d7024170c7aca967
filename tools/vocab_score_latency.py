"""Corpus-scale token scoring on a 16-bit vocabulary table: three routes to (greedy token, log-probability of a target) for M
rows of x [M, K] against w [V, K], timed at the model's own workload (wikitext-103 LM layer: 18 x 512 = 9216 rows, K = 1024):
   1. ea_vocab_score (C ABI 30): one call, the tiled GEMM with the pick and the online log-sum-exp as its epilogue;
   2. the 64-row loop of DecoderStack.token_logprobs: ea_ceva_sdecode_vocab_logprob on ceil(M / 64) pieces, each streaming the
      whole table -- the only HIP route before ABI 30, and so the baseline;
   3. the framework: F.linear, float(), log_softmax, gather and argmax on a [M, V] tensor, where it fits in memory.
   python tools/vocab_score_latency.py [--shapes 9216x1024x32768,9216x1024x262144] [--rounds 3] [--reps 5] [--window-ms 200] [--dtype bf16]   (GPU)
Operands are seeded normal draws (x ~ N(0, 1), w ~ N(0, 1 / K)), not zeros.  Each route is warmed up twice at the shape it is
timed at; a round times every route once, between two device events, over at least `reps` calls and at least `window-ms` of
work, and the rounds alternate the routes, so that a drift of the machine shows as spread and not as a difference.  One line
per (shape, route): the median ms per call over the rounds, the smallest and the largest, 2 M K V / time as TFLOP/s, and for
route 2 the table bytes it streams per second; then how far the routes' results are apart (reordered fp32 sums, and in the
framework route logits rounded to 16 bits: tokens may differ where two logits nearly tie)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from efficient_attention import _native as nv  # noqa: E402

FEW_ROWS = 64


def operands(M, K, V, dtype):
    g = torch.Generator().manual_seed(M * 31 + V)
    x = torch.randn(M, K, generator=g).to(dtype).cuda()
    w = torch.empty(V, K, dtype=dtype, device="cuda")
    for a in range(0, V, 32768):                          # (in pieces: no [V, K] fp32 tensor on the host)
        w[a:a + 32768] = (torch.randn(min(32768, V - a), K, generator=g) / K ** 0.5).to(dtype).cuda()
    targets = torch.randint(0, V, (M,), generator=g).cuda()
    return x, w, targets


def route_score(x, w, targets):
    M, K = x.shape
    V = w.shape[0]
    nbytes = nv.lib().ea_vocab_score_ws(M, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tok = torch.empty(M, dtype=torch.long, device="cuda")
    lse = torch.empty(M, dtype=torch.float32, device="cuda")
    logp = torch.empty(M, dtype=torch.float32, device="cuda")

    def call():
        nv.call("ea_vocab_score", M, K, V, nv.ptr(x), nv.io_dtype(x), K, nv.ptr(w), nv.io_dtype(w), nv.ptr(targets), None,
                nv.EA_F32, V, nv.ptr(ws), nbytes, nv.ptr(tok), None, nv.ptr(lse), nv.ptr(logp), nv.stream())
        return tok, logp
    return call


def route_few_rows(x, w, targets):
    M, K = x.shape
    V = w.shape[0]
    nbytes, lbytes = nv.lib().ea_ceva_sdecode_vocab_ws(FEW_ROWS, V), nv.lib().ea_ceva_sdecode_vocab_lse_ws(FEW_ROWS, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    lws = torch.empty(lbytes, dtype=torch.uint8, device="cuda")
    tok = torch.empty(M, dtype=torch.long, device="cuda")
    lse = torch.empty(M, dtype=torch.float32, device="cuda")
    logp = torch.empty(M, dtype=torch.float32, device="cuda")

    def call():
        for a in range(0, M, FEW_ROWS):                   # token_pick.HeldGreedyLogprob.run's loop
            n = min(FEW_ROWS, M - a)
            nv.call("ea_ceva_sdecode_vocab_logprob", n, K, V, nv.ptr(x[a:a + n]), nv.io_dtype(x), K, nv.ptr(w), nv.io_dtype(w),
                    None, nv.EA_F32, V, nv.ptr(ws), nbytes, nv.ptr(tok[a:a + n]), None, nv.ptr(lws), lbytes,
                    nv.ptr(targets[a:a + n]), nv.ptr(lse[a:a + n]), nv.ptr(logp[a:a + n]), nv.stream())
        return tok, logp
    return call


def route_framework(x, w, targets):
    M, V = x.shape[0], w.shape[0]
    need = M * V * (x.element_size() + 4 + 4) * 1.25      # the 16-bit logits, their fp32 copy, the log-softmax
    free = torch.cuda.mem_get_info()[0]
    if need > free:
        return None

    def call():
        logits = F.linear(x, w).float()
        lp = torch.log_softmax(logits, dim=-1)
        return logits.argmax(-1), lp.gather(1, targets.unsqueeze(1)).squeeze(1)
    return call


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="9216x1024x32768,9216x1024x262144")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vocab_score_latency.py times GPU kernels: no GPU here, nothing measured")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    print("BM, BN, SL =", nv.vocab_score_tiles(), "| device:", torch.cuda.get_device_name(0))
    for shape in a.shapes.split(","):
        M, K, V = (int(s) for s in shape.split("x"))
        x, w, targets = operands(M, K, V, dtype)
        routes = [("ea_vocab_score", route_score(x, w, targets)), ("64-row loop", route_few_rows(x, w, targets)),
                  ("framework", route_framework(x, w, targets))]
        results, times = {}, {name: [] for name, _ in routes}
        for name, call in routes:
            if call is None:
                print("%s %-15s does not fit in the free device memory: not measured" % (shape, name))
                continue
            for _ in range(2):
                out = call()
            torch.cuda.synchronize()
            results[name] = tuple(t.clone() for t in out)
        # a timed window is at least `reps` calls and at least --window-ms of work (sized by one timed call after the warm-up)
        reps = {name: max(a.reps, min(1000, int(a.window_ms / timed(call, 1)) + 1)) for name, call in routes if call is not None}
        for _ in range(a.rounds):
            for name, call in routes:
                if call is not None:
                    times[name].append(timed(call, reps[name]))
        flop = 2.0 * M * K * V
        for name, call in routes:
            if call is None:
                continue
            t = sorted(times[name])
            med = t[len(t) // 2]
            extra = ""
            if name == "64-row loop":
                extra = " | table stream %.0f GB/s" % (-(-M // FEW_ROWS) * 2.0 * V * K / (med * 1e-3) / 1e9)
            print("%s %-15s median %9.3f ms (min %9.3f, max %9.3f; %d calls a window) | %7.1f TFLOP/s%s"
                  % (shape, name, med, t[0], t[-1], reps[name], flop / (med * 1e-3) / 1e12, extra))
        base = results["ea_vocab_score"]
        for name in ("64-row loop", "framework"):
            if name in results:
                tok, lp = results[name]
                print("%s ea_vocab_score vs %-12s tokens equal in %d of %d rows; largest |logp difference| %.3e"
                      % (shape, name, int((tok == base[0]).sum()), M, (lp - base[1]).abs().max().item()))
        del x, w, targets, routes, results
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
