"""Forward + backward time of one LARA layer past 128 samples under bf16 autocast, with the estimator on the 16-bit kernels of
csrc/ea_lara_lm.hip (_ops.USE_LARA_LONG = True) and on the fp32 gathered-attention route they replace (False, what
EA_LARA_LONG=0 selects), on the same module and inputs:
   python tools/lara_long_latency.py [--cases deit,seq] [--rounds 7] [--steps 10]      (GPU)
Cases: deit = x [128, 28, 28, 192], 3 heads, 14 x 14 = 196 pooled landmarks; seq = x [2, 4096, 512], 8 heads, 256 segment
landmarks.  Also prints the plan (resident / streamed) each token-column pass of the 16-bit route takes.  Rounds alternate the two routes; a round times `steps` training steps (forward, backward of a
fixed dy) by the host clock around the steps and a device synchronise, after a warm-up of both routes; the module is in eval
mode (no landmark noise) so that the two routes compute the same function.  Prints per case the median and the min .. max over the
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
CASES = {
    "deit": ((128, 28, 28, 192), dict(dim=192, num_heads=3, num_landmarks=196, proposal_gen="pool-mixed", mis_type="mis-opt")),
    "seq": ((2, 4096, 512), dict(dim=512, num_heads=8, num_landmarks=256, proposal_gen="adaptive-1d", mis_type="mis-opt")),
}


def train_step(m, x, dy, on):
    _ops.USE_LARA_LONG = on
    m.zero_grad(set_to_none=True)
    x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    y.backward(dy)
    return y.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="deit,seq")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    was = _ops.USE_LARA_LONG
    print("ms per training step of one layer (forward + backward), bf16 autocast, %d rounds of %d steps" % (a.rounds, a.steps))
    for name in a.cases.split(","):
        shape, args = CASES[name]
        torch.manual_seed(0)
        m = ea.AttentionFactory.build_attention("lara", dict(args)).cuda().eval()
        x = (0.5 * torch.randn(*shape, device="cuda")).requires_grad_(True)
        dy = torch.randn(*shape, device="cuda").to(torch.bfloat16)
        import ctypes
        from efficient_attention import _native as nv
        N = 1
        for n_ in shape[1:-1]:
            N *= n_
        g = nv.ea_lara_geom(shape[0], args["num_heads"], N, 64, nv.EA_BF16, args["num_landmarks"], 0, 1.0, 0.125)
        plans = [("?", "resident", "streamed")[max(nv.lib().ea_lara_lm_plan(ctypes.byref(g), p_, 0), 0)] for p_ in range(4)]
        print("%-4s plans: out_fwd %s, bwd_q %s, bwd_k %s, bwd_qcorr %s" % ((name,) + tuple(plans)))
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
        print("%-4s x %s (%d landmarks): 16-bit %.3f (%.3f .. %.3f)  fp32 route %.3f (%.3f .. %.3f)  ratio %.2f  max|dy|/max|y| %.1e"
              % (name, list(shape), args["num_landmarks"], med[True], min(times[True]), max(times[True]), med[False],
                 min(times[False]), max(times[False]), med[False] / med[True], diff), flush=True)
    _ops.USE_LARA_LONG = was


if __name__ == "__main__":
    main()
