"""The adaptive-softmax criterion as a training loss: forward + backward of three routes from rows x [M, C] to the gradients of x
and of every parameter, at the recipe's geometry (wikitext-103: 9216 rows, C = 1024, cutoffs 20000 / 60000 / 267744, factor 4:
tails of width 256 and 64):
   1. ea_harness.adaptive_loss.adaptive_nll: ea_adaptive_score forward; the head's chunk loop and, per tail, the device-counted
      chunk loop (ea_vocab_nll_grad_rows, ea_gemm_nt16_rows, ea_gemm_nt16, ea_rows_transpose16) backward; nothing read back;
   2. the framework: ea_harness.adaptive.AdaptiveSoftmax.get_log_prob(x, target) under autocast (16-bit GEMMs, fp32 softmax) and
      backward -- it reads the per-band row indices back and builds [rows, c0 + n] and [rows_i, V_i] tensors;
   3. ea_harness.vocab_loss.vocab_nll on a plain [V, C] table of the same height, for scale.
   python tools/adaptive_loss_latency.py [--rows 9216] [--channels 1024] [--cutoffs 20000,60000,267744] [--factor 4]
                                         [--mixes head,80/12/8] [--rounds 5] [--reps 3] [--window-ms 200] [--dtype bf16]   (GPU)
Operands are seeded normal draws in the modules' own initialisation, not zeros; every route differentiates the sum of the
targets' log-probabilities.  Two target mixes: every target in the head, and 80 / 12 / 8 % over the bands.  Each route is warmed
up twice at the shape it is timed at; a round times every route once, between two device events, over at least `reps` calls
and at least `window-ms` of work, and the rounds alternate the routes, so that a drift of the machine shows as spread and not as
a difference.  Per (mix, route): the median ms per forward + backward over the rounds with the smallest and the largest, and the
rise of torch.cuda.max_memory_allocated over one forward + backward above the operands (x, the parameters, the targets).  There
is no pass or fail on time: the figures go into DESIGN.md 4a."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
from efficient_attention import _native as nv  # noqa: E402
from ea_harness.adaptive import AdaptiveSoftmax  # noqa: E402
from ea_harness.adaptive_loss import adaptive_nll  # noqa: E402
from ea_harness.vocab_loss import vocab_nll  # noqa: E402


def targets_of(mix, M, cutoffs, g):
    """mix 'head' or percentages 'a/b/c' over the bands -> int64 [M] on the device, the bands' rows interleaved at random."""
    share = [100] + [0] * (len(cutoffs) - 1) if mix == "head" else [float(s) for s in mix.split("/")]
    if len(share) != len(cutoffs) or abs(sum(share) - 100) > 1e-6:
        raise SystemExit("a mix is 'head' or one percentage per band summing to 100, got %r" % mix)
    band = torch.multinomial(torch.tensor(share, dtype=torch.float), M, replacement=True, generator=g)
    lo = torch.tensor([0] + list(cutoffs[:-1]))[band]
    hi = torch.tensor(list(cutoffs))[band]
    return (lo + (torch.rand(M, generator=g) * (hi - lo)).long()).minimum(hi - 1).cuda()


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def peak_rise(call, clear):
    clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=9216)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--cutoffs", default="20000,60000,267744")
    ap.add_argument("--factor", type=float, default=4.0)
    ap.add_argument("--mixes", default="head,80/12/8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_loss_latency.py times GPU kernels: no GPU here, nothing measured")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    M, C = a.rows, a.channels
    cutoffs = [int(c) for c in a.cutoffs.split(",")]
    V = cutoffs[-1]
    g = torch.Generator().manual_seed(M * 31 + V)
    torch.manual_seed(M * 31 + V)
    sm = AdaptiveSoftmax(V, C, cutoffs[:-1], 0.0, factor=a.factor).cuda()
    dims = sm.band_dims()
    plain = torch.empty(V, C, dtype=torch.float32, device="cuda")
    for at in range(0, V, 32768):                          # (in pieces: no [V, C] fp32 tensor on the host)
        plain[at:at + 32768] = (torch.randn(min(32768, V - at), C, generator=g) / C ** 0.5).cuda()
    plain.requires_grad_(True)
    x = torch.randn(M, C, generator=g).to(dtype).cuda().requires_grad_(True)
    cut, hd = nv.host_array(ctypes.c_int64, cutoffs), nv.host_array(ctypes.c_int32, dims)
    print("BM, BN, SL =", nv.vocab_score_tiles(), "| device:", torch.cuda.get_device_name(0))
    print("%d rows x %d, cutoffs %s, widths %s: ea_adaptive_nll_ws %.1f MiB, ea_adaptive_score_ws (saved) %.1f MiB, the last tail's "
          "[M, V_i] in 16 bits %.1f MiB" % (M, C, cutoffs, dims, nv.lib().ea_adaptive_nll_ws(M, C, len(dims), cut, hd, 0) / 2 ** 20,
                                           nv.lib().ea_adaptive_score_ws(M, len(dims), cut, hd) / 2 ** 20,
                                           2 * M * (cutoffs[-1] - cutoffs[-2]) / 2 ** 20))

    def clear():
        x.grad = plain.grad = None
        sm.zero_grad(set_to_none=True)
    for mix in a.mixes.split(","):
        targets = targets_of(mix, M, cutoffs, g)
        counts = [int(((targets >= lo) & (targets < hi)).sum()) for lo, hi in zip([0] + cutoffs[:-1], cutoffs)]

        def ours():
            clear()
            with torch.autocast("cuda", dtype=dtype, cache_enabled=False):
                logp = adaptive_nll(x.view(M, 1, C), sm, targets.view(M, 1))
            (-logp.sum()).backward()

        def framework():
            clear()
            with torch.autocast("cuda", dtype=dtype, cache_enabled=False):
                logp = sm.get_log_prob(x, targets)
            (-logp.float().sum()).backward()

        def plain_table():
            clear()
            with torch.autocast("cuda", dtype=dtype, cache_enabled=False):
                logp = vocab_nll(x.view(M, 1, C), plain, targets.view(M, 1))
            (-logp.sum()).backward()
        routes = [("adaptive_nll", ours), ("framework", framework), ("vocab_nll plain", plain_table)]
        grads, times = {}, {name: [] for name, _ in routes}
        for name, call in routes:
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            grads[name] = [x.grad.float().clone()] + [None if p.grad is None else p.grad.clone() for p in sm.parameters()]
        reps = {name: max(a.reps, min(1000, int(a.window_ms / timed(call, 1)) + 1)) for name, call in routes}
        for _ in range(a.rounds):
            for name, call in routes:
                times[name].append(timed(call, reps[name]))
        print("mix %s: rows per band %s" % (mix, counts))
        for name, call in routes:
            t = sorted(times[name])
            print("mix %-8s %-16s fwd+bwd median %9.3f ms (min %9.3f, max %9.3f; %d rounds of %d calls) | peak above the operands %8.1f MiB"
                  % (mix, name, t[len(t) // 2], t[0], t[-1], len(t), reps[name], peak_rise(call, clear) / 2 ** 20))
        names = ["d x"] + ["d " + k for k, _ in sm.named_parameters()]
        for k, mine, theirs in zip(names, grads["adaptive_nll"], grads["framework"]):
            if theirs is None or theirs.norm().item() == 0.0:
                print("mix %-8s %s: the framework route has no gradient here; ours is %s"
                      % (mix, k, "absent" if mine is None else "all zeros" if mine.abs().max().item() == 0.0 else "NOT zero"))
            else:
                print("mix %-8s %s: |ours - framework| / |framework| = %.3e" % (mix, k, ((mine - theirs).norm() / theirs.norm()).item()))
        clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
