"""-m gpu: the 16-bit LARA estimator past 128 samples (csrc/ea_lara_lm.hip: the token-column passes as a loop over 64-sample
groups; the token-row kernels and merges behind the ea_lara_lm_* entries).

1. _ops._lara_fwd_core / _lara_bwd_core / _lara_finish, driven as tests/test_gpu_lara_core.py drives them, against the fp64
   evaluation of the same operands under the same bound: a(HIP) <= 4 a(M) + f per tensor, M = the two-pass rounding model of
   tests/lara_reference.py.
2. LinearRA in training under bf16 autocast against the same module on the fp32 route (EA_LARA_LONG=0), entries recorded.
   Measured on an MI355X: every tensor of both cases within (5.2e-3, 4.6e-3) of gpu_checks.MODULE_TOL = (4e-2, 2e-2).  (While
   the [C x C] proposal densities and the softmax mixing still ran as 16-bit GEMMs under autocast, the generators' gradients
   of the [2d] case stood at 2e-2 in rms.)
3. The envelope: d = 32 and C = 128 keep their routes."""
import pytest
import torch

import test_gpu_lara_core as core       # (puts the package and tests/ on sys.path; _run_lara_kernels, _reference)
import lara_reference as lr

KAPPA = core.lc.KAPPA                   # 0.25, what _run_lara_kernels and _reference use
# name: N, C, mis types, B, h, padded tail of batch row 1, time-first qkv5 view, forced plan (0: the planner's, 2: streamed)
CASES = {
    "ninth_tile": dict(N=272, C=129, mis=("opt", "biased", "bh")),
    "padded": dict(N=400, C=200, mask_tail=37),
    "few_tokens": dict(N=100, C=144),
    "edge": dict(N=1024, C=512),
    "streamed": dict(N=400, C=200, plan=2),
    "time_first": dict(N=272, C=256, B=1, h=3, time_first=True),
}
RUNS = [(n_, m) for n_ in sorted(CASES) for m in CASES[n_].get("mis", ("opt",))]


def _operands(name, mis, io):
    """lara_cases.operands' recipe, seeded N + C."""
    k = CASES[name]
    c = dict(B=k.get("B", 2), h=k.get("h", 2), N=k["N"], d=64, C=k["C"], time_first=k.get("time_first", False))
    B, h, N, d, C = c["B"], c["h"], c["N"], c["d"], c["C"]
    g = torch.Generator().manual_seed(N + C)
    r16 = lambda t: t.to(io).float()                                                   # noqa: E731
    o = dict(q=r16(torch.randn(B, h, N, d, generator=g)), k=r16(torch.randn(B, h, N, d, generator=g)),
             v=r16(torch.randn(B, h, N, d, generator=g)), dout=r16(torch.randn(B, h, N, d, generator=g)),
             omega=torch.randn(B, h, C, d, generator=g), qbar=0.5 * torch.randn(B, h, C, d, generator=g),
             bhv=torch.softmax(0.25 * torch.randn(B, h, C, generator=g), -1), lp=torch.randn(B, h, C, generator=g), mask=None)
    if mis == "bh":
        o["qbar"] = None
    if mis != "opt":
        o["bhv"] = None
    if k.get("mask_tail"):
        o["mask"] = torch.zeros(B, N, dtype=torch.bool)
        o["mask"][1, N - k["mask_tail"]:] = True
    return c, o


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(core.DTYPES))
@pytest.mark.parametrize("name,mis", RUNS)
def test_long_passes_match_fp64_same_operand_reference(name, mis, dt, monkeypatch):
    from efficient_attention import _ops
    io = core.DTYPES[dt]
    c, o = _operands(name, mis, io)
    R, M = core._reference(c, o, mis, core.F64, None), core._reference(c, o, mis, torch.float32, io)
    if mis == "opt":       # the clamp at 1e-8 is a discontinuity: the case must keep clear of it in the reference itself
        assert float(lr.lara_alpha(o["q"], o["qbar"], o["bhv"], kappa=KAPPA, scale=c["d"] ** -0.5).min()) > 1e-5
    monkeypatch.setattr(_ops, "LARA_LONG_PLAN", CASES[name].get("plan", 0))
    got = core._run_lara_kernels(c, o, mis, io)              # (fills dqkv5 with NaN first and asserts every element was written)
    if o["mask"] is not None:
        pad = o["mask"][:, None, :, None].expand_as(got["dk"])
        assert bool((got["dk"][pad] == 0).all()) and bool((got["dv"][pad] == 0).all()), "dk / dv of padded keys must be exactly 0"
    if name == "padded":   # fixed summation order over the sequence slices: a second run gives the same bits
        again = core._run_lara_kernels(c, o, mis, io)
        for n_ in ("d_omega", "d_qbar", "d_bhv", "d_lp", "kv"):
            assert torch.equal(got[n_], again[n_]), n_
    assert set(got) == set(R)
    bad, lines = [], []
    for n_ in ("out", "kv", "lse_k", "dq", "dk", "dv", "d_omega", "d_lp", "d_qbar", "d_bhv"):
        if n_ in R:
            ok, txt, _ = lr.bound_report(n_, got[n_], M[n_], R[n_], io)
            lines.append("%s/%s/%s %s" % (name, mis, dt, txt))
            if not ok:
                bad.append(n_)
    print("\n" + "\n".join(lines))
    assert not bad, "%s exceed 4 a(M) + f\n%s" % (bad, "\n".join(lines))


def _lara(**args):
    import efficient_attention as ea
    torch.manual_seed(5)
    return ea.AttentionFactory.build_attention("lara", dict(num_heads=2, mis_type="mis-opt", **args)).cuda().train()


def _train_step(m, x0, dy, noise, mask, long_route):
    """One step under bf16 autocast -> (y, dx and every parameter gradient; the C-ABI entries it called with their geometry's C)."""
    from efficient_attention import _native as nv, _ops
    calls, real, real_like, was = [], nv.call, torch.randn_like, _ops.USE_LARA_LONG
    nv.call = lambda nm, *a: (calls.append((nm, getattr(getattr(a[0], "_obj", None), "C", None))), real(nm, *a))[1]
    torch.randn_like = lambda t, **kw: noise.to(t.dtype)                     # the landmark noise: the same draw on both routes
    _ops.USE_LARA_LONG = long_route
    try:
        m.zero_grad()
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x, mask) if mask is not None else m(x)
        y.backward(dy.to(y.dtype))
    finally:
        nv.call, torch.randn_like, _ops.USE_LARA_LONG = real, real_like, was
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return dict(grads, y=y.detach(), dx=x.grad), calls


MODULES = {
    "2d": ((2, 24, 24, 128), dict(dim=128, proposal_gen="pool-mixed", num_landmarks=144), 144, 0),
    "1d": ((2, 400, 128), dict(dim=128, proposal_gen="adaptive-1d", num_landmarks=100, use_antithetics=True), 100, 41)}


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", sorted(MODULES))
def test_module_trains_past_128_samples_on_the_16_bit_kernels(geometry):
    """C = 144 (2-D) and C = 200 (1-D, antithetic), d = 64: y, dx and every parameter gradient against the same module on the
    route it took before (fp32 up-cast, ea_f32_attn_*), and the new entries ran in place of the fp32 ones."""
    from gpu_checks import MODULE_TOL
    from util import scaled_err
    shape, args, nl, pad = MODULES[geometry]
    m = _lara(**args)
    x0, dy = torch.randn(*shape, device="cuda"), torch.randn(*shape, device="cuda")
    noise = torch.randn(2, 2, nl, 64, device="cuda")
    mask = None
    if pad:
        mask = torch.zeros(shape[0], shape[1], dtype=torch.bool, device="cuda")
        mask[1, shape[1] - pad:] = True
    new, calls = _train_step(m, x0, dy, noise, mask, True)
    old, old_calls = _train_step(m, x0, dy, noise, mask, False)
    names, old_names = {c[0] for c in calls}, {c[0] for c in old_calls}
    assert {"ea_lara_lm_out_fwd", "ea_lara_lm_bwd_q", "ea_lara_lm_bwd_k", "ea_lara_lm_bwd_qcorr", "ea_lara_lm_stats_fwd"} <= names, sorted(names)
    assert not [c for c in names if c.startswith("ea_f32_attn")] and "ea_f32_attn_fwd" in old_names
    assert set(new) == set(old) and len(new) >= 8
    for name in old:
        e = scaled_err(new[name].float().cpu().numpy(), old[name].float().cpu().numpy())
        print(name, e)
        assert e[0] <= MODULE_TOL[0] and e[1] <= MODULE_TOL[1], (name, e)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,args,entry,C", [(64, dict(num_landmarks=144), "ea_f32_attn_fwd", None),
                                              (128, dict(num_landmarks=64, use_antithetics=True), "ea_lara_bwd_q", 128)],
                         ids=["d32_C144", "d64_C128"])
def test_outside_the_envelope_the_routes_stay(dim, args, entry, C):
    """Head dim 32 at 144 landmarks keeps the fp32 route; 128 samples keep the two-pass entries of ea_lara_x.hip."""
    m = _lara(dim=dim, proposal_gen="pool-mixed", **args)
    x0 = torch.randn(2, 24, 24, dim, device="cuda")
    noise = torch.randn(2, 2, args["num_landmarks"], dim // 2, device="cuda")
    _, calls = _train_step(m, x0, torch.randn_like(x0), noise, None, True)
    hit = [c for c in calls if c[0] == entry]
    assert hit and (C is None or hit[0][1] == C) and not [c for c in calls if c[0].startswith("ea_lara_lm")], sorted(set(calls))
