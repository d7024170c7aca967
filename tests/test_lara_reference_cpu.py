"""CPU checks of the same-operand LARA estimator reference (tests/lara_reference.py) that tests/test_gpu_lara_core.py holds the
16-bit token passes to:
  a. the reference equals the oracle (oracle/attention.py: lara_core) in fp64 to 1e-12, output and gradients, and the rounding
     model's hand-written arithmetic with the roundings switched off equals the reference's autograd;
  b. every mis-opt case keeps alpha clear of the clamp (min alpha >= 0.2 / C): a condition on the inputs, not on the kernel;
  c. every case of tests/lara_cases.py still gets the plan it was written for (host queries; no GPU needed), and the geometries
     the library refuses are refused;
  d. the model-relative bound rejects the model with ONE deliberate defect, and accepts the unmutated model."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lara_cases as lc                 # noqa: E402
import lara_reference as lr             # noqa: E402
from oracle import attention as oa      # noqa: E402

F64 = torch.float64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
ORACLE_MIS = {"opt": "mis-opt", "biased": "mis-biased", "bh": "mis-bh"}


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------------
# a. reference against oracle
# ------------------------------------------------------------------------------------------------------------------------
def _landmark_operands(q_bar, mu, noise, mis, mode, scale):
    """omega, qbar rows, bhv, lp of the estimator from q_bar, mu and the noise draw, as lara_core forms them internally."""
    if mode == "antithetic":
        omega, dup = torch.cat([mu + noise, mu - noise], -2), True
    else:
        omega, dup = mu + noise, False
    rep = (lambda t: t.repeat(1, 1, 2, 1)) if dup else (lambda t: t)
    if mis == "opt":
        lpmu = oa.prm_log_features(rep(mu), omega, scale)                       # [B,h,C,C]
        lp = torch.diagonal(lpmu, dim1=-1, dim2=-2)
        return omega, rep(q_bar), torch.exp(lp - torch.logsumexp(lpmu, -1)), lp
    lp = torch.logsumexp(oa.prm_log_features(mu, omega, scale), -1)
    return omega, (rep(mu) if mis == "biased" else None), None, lp


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "tailmask"])
@pytest.mark.parametrize("mode", ["single", "antithetic"])
@pytest.mark.parametrize("mis", ["opt", "biased", "bh"])
def test_reference_equals_lara_core(mis, mode, masked):
    B, h, N, d, L = 2, 2, 40, 16, 6
    g = torch.Generator().manual_seed(5 + len(mis) + len(mode))
    q, k, v = [torch.randn(B, h, N, d, dtype=F64, generator=g).requires_grad_(True) for _ in range(3)]
    q_bar, mu, noise = [0.5 * torch.randn(B, h, L, d, dtype=F64, generator=g) for _ in range(3)]
    gy = torch.randn(B, h, N, d, dtype=F64, generator=g)
    mask = None
    if masked:
        mask = torch.zeros(B, N, dtype=torch.bool)
        mask[1, N - 11:] = True
    scale, kappa = d ** -0.5, 0.7
    ref = oa.lara_core(q, k, v, mask, q_bar, mu, noise, ORACLE_MIS[mis], kappa, mode, scale)
    gr = torch.autograd.grad(ref, [q, k, v], gy)
    omega, qrows, bhv, lp = _landmark_operands(q_bar, mu, noise, mis, mode, scale)
    out, _, _ = lr.lara_estimator(q, k, v, mask, omega, qrows, bhv, lp, mis=mis, kappa=kappa, scale=scale, dtype=F64)
    go = torch.autograd.grad(out, [q, k, v], gy)
    assert _rel(out, ref) <= 1e-12
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(go, gr))


@pytest.mark.parametrize("C", [7, 70], ids=["fused", "two_pass"])
@pytest.mark.parametrize("mis", ["opt", "biased", "bh"])
def test_model_arithmetic_without_roundings_is_the_reference(mis, C):
    """_ModelLara writes the kernels' forward and backward out by hand; with round_to = None it must be the same function."""
    B, h, N, d = 2, 2, 37, 16
    g = torch.Generator().manual_seed(3 + C)
    q, k, v, dout = [torch.randn(B, h, N, d, dtype=F64, generator=g) for _ in range(4)]
    omega, qbar = torch.randn(B, h, C, d, dtype=F64, generator=g), 0.5 * torch.randn(B, h, C, d, dtype=F64, generator=g)
    bhv, lp = torch.softmax(0.25 * torch.randn(B, h, C, dtype=F64, generator=g), -1), torch.randn(B, h, C, dtype=F64, generator=g)
    mask = torch.zeros(B, N, dtype=torch.bool)
    mask[1, N - 9:] = True
    kw = dict(mis=mis, kappa=0.25, scale=d ** -0.5, dtype=F64)
    R = lr.lara_grads(q, k, v, mask, omega, qbar, bhv, lp, dout, **kw)
    X = lr.lara_grads(q, k, v, mask, omega, qbar, bhv, lp, dout, model=True, **kw)
    assert set(X) == set(R)
    for n_ in R:
        assert _rel(X[n_], R[n_]) <= 1e-10, n_
    assert bool((X["dk"][1, :, N - 9:] == 0).all()) and bool((X["dv"][1, :, N - 9:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# b. the alpha margin
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", [n_ for n_, m in lc.RUNS if m == "opt"])
def test_alpha_stays_clear_of_the_clamp(name, dt):
    c, o = lc.operands(name, "opt", DTYPES[dt])
    worst = float("inf")
    for b0 in range(0, c["B"], 16):
        sl = slice(b0, b0 + 16)
        alpha = lr.lara_alpha(o["q"][sl], o["qbar"][sl], o["bhv"][sl], kappa=lc.KAPPA, scale=c["d"] ** -0.5)
        worst = min(worst, float(alpha.min()))
    print("\n%s/%s min alpha * C = %.3f" % (name, dt, worst * c["C"]))
    assert worst >= 0.2 / c["C"]


# ------------------------------------------------------------------------------------------------------------------------
# c. plan pins and refusals
# ------------------------------------------------------------------------------------------------------------------------
def _geom(B, h, N, d, io, C, mis):
    from efficient_attention import _native as nv
    return nv.ea_lara_geom(B, h, N, d, io, C, mis, lc.KAPPA, float(d) ** -0.5)


@pytest.mark.parametrize("io", [0, 1])
@pytest.mark.parametrize("name,mis", lc.RUNS)
def test_plan_pins(name, mis, io, monkeypatch):
    from efficient_attention import _native as nv
    from efficient_attention import _ops
    c = lc.CASES[name]
    monkeypatch.setenv("EA_LARA_FOLD", "1" if c["fold"] else "0")
    geom = _geom(c["B"], c["h"], c["N"], c["d"], io, c["C"], lc.MIS_CODE[mis])
    parts, fused = int(nv.lib().ea_lara_parts(ctypes.byref(geom))), int(nv.lib().ea_lara_fused_parts(ctypes.byref(geom)))
    got = (parts, fused, _ops.lara_fold(c["C"], parts), c["C"] <= 64 and _ops.lara_fold(c["C"], fused), lc.nct(c["C"]), lc.lh1(c["C"]))
    assert got == lc.PINS[name], (name, dict(zip(lc.PIN_NAMES, got)))


def test_pins_say_what_the_case_table_claims():
    P = {n_: dict(zip(lc.PIN_NAMES, v)) for n_, v in lc.PINS.items()}
    C = lc.CASES
    assert set(P) == set(C) and len(lc.RUNS) == 17
    assert P["A1"]["lh1"] and P["A5"]["lh1"] and not P["A6"]["lh1"] and not P["A2"]["lh1"]          # both sides of the LH switch
    assert C["A5"]["C"] - 48 == 2 and C["A6"]["C"] - 48 == 3
    assert {P[n_]["nct"] for n_ in P} == {1, 2, 3, 4, 5, 7}                                          # every landmark-tile template
    assert lc.PINS["A1u"][:2] == lc.PINS["A1"][:2] and not P["A1u"]["fold_fwd"] and not P["A1u"]["fold_bwd"]     # same plan, merges unfolded
    assert P["A7"]["fold_fwd"] and not P["A7"]["fold_bwd"]                                           # folded one way only
    assert not P["A3"]["fold_fwd"] and not P["A3"]["fold_bwd"] and P["A3"]["parts"] > 4
    assert P["A4"]["fused"] == 2 and C["A4"]["N"] <= 64                                              # one slice x two token halves
    assert P["T1"]["fused"] == -2 and P["T2"]["fused"] == -2 and C["T1"]["C"] > 64 and C["T2"]["C"] == 65
    assert P["O1"]["parts"] == 8 and P["O1"]["fused"] == 16 and C["O1"]["time_first"]
    for n_ in ("E1", "E2"):                                                                          # two slices per (b,h), 384 (b,h)
        assert C[n_]["B"] * C[n_]["h"] == 384 and P[n_]["fused"] == 2 and P[n_]["parts"] == 2
    assert C["A1"]["N"] % 16 == 4 and C["A1m"]["mask_tail"] == 37 and C["E2"]["mask_tail"] > 0


def test_unsupported_geometries_are_refused_without_a_launch():
    from efficient_attention import _native as nv
    lib = nv.lib()
    EA_E_BADARG, EA_E_UNSUPPORTED = -1, -2
    assert lib.ea_lara_fused_parts(ctypes.byref(_geom(2, 3, 200, 32, 0, 65, 1))) == EA_E_UNSUPPORTED
    assert lib.ea_lara_parts(ctypes.byref(_geom(2, 3, 200, 32, 0, 65, 1))) > 0
    assert lib.ea_lara_parts(ctypes.byref(_geom(2, 3, 100, 128, 0, 49, 0))) == EA_E_BADARG
    assert lib.ea_lara_parts(ctypes.byref(_geom(2, 3, 100, 64, 0, 129, 0))) == EA_E_UNSUPPORTED
    assert lib.ea_lara_parts(ctypes.byref(_geom(2, 3, 100, 64, 0, 128, 0))) > 0


# ------------------------------------------------------------------------------------------------------------------------
# d. sensitivity of the model-relative bound
# ------------------------------------------------------------------------------------------------------------------------
SENS = {d_: ("A1m" if d_ == "padded_keys_in_lse_k" else "A1") for d_ in lr.DEFECTS}
_SENS = {}
# The correction dq -= s sum_c t[c,n] u_c qbar_c is a small part of dq with these operands (t ~ 1 / N, kappa = 0.25): without it dq
# moves by 1.3 a(M) in bf16 -- 0.4 of the bound -- and by 3.3 times the bound in fp16.  The case is not tuned until it trips.
UNDER_BOUND = {("uq_correction_missing", "bf16")}


def _sens_setup(name, dt):
    key = (name, dt)
    if key not in _SENS:
        io = DTYPES[dt]
        c, o = lc.operands(name, "opt", io)
        ops = (o["q"], o["k"], o["v"], o["mask"], o["omega"], o["qbar"], o["bhv"], o["lp"], o["dout"])
        kw = dict(mis="opt", kappa=lc.KAPPA, scale=c["d"] ** -0.5)
        _SENS[key] = (ops, kw, lr.lara_grads(*ops, dtype=F64, **kw), lr.lara_grads(*ops, dtype=torch.float32, round_to=io, **kw))
    return _SENS[key]


def _excess(name, X, M, R, io):
    """The largest of the three figures of X over its bound FACTOR * figure(M) + f (> 1: the bound rejects X)."""
    f = lr.floor_for(name, io)
    got = (lr.a_err(X, R),) + lr.norm_errs(X, R)
    mod = (lr.a_err(M, R),) + lr.norm_errs(M, R)
    return max(g_ / (lr.FACTOR * m_ + f) for g_, m_ in zip(got, mod))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ["A1", "A1m"])
def test_unmutated_model_passes_at_ratio_one(name, dt):
    ops, kw, R, M = _sens_setup(name, dt)
    for n_ in R:
        ok, txt, ratio = lr.bound_report(n_, M[n_], M[n_], R[n_], DTYPES[dt])
        assert ok and ratio == 1.0, txt
        # and the model is a rounding-level perturbation of the reference, not a different function
        assert lr.a_err(M[n_], R[n_]) <= (0.05 if dt == "bf16" else 0.01), txt


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("defect", lr.DEFECTS)
def test_bound_rejects_single_defect(defect, dt):
    io = DTYPES[dt]
    ops, kw, R, M = _sens_setup(SENS[defect], dt)
    X = lr.lara_grads(*ops, dtype=torch.float32, round_to=io, defect=defect, **kw)
    res = {n_: lr.bound_report(n_, X[n_], M[n_], R[n_], io) for n_ in R}
    exc = {n_: _excess(n_, X[n_], M[n_], R[n_], io) for n_ in R}
    worst = max(exc, key=exc.get)
    print("\n%s/%s exceeds the bound by a factor %.1f (%s); rejected on %s" % (
        defect, dt, exc[worst], worst, sorted(n_ for n_, (ok, _, _) in res.items() if not ok)))
    if (defect, dt) in UNDER_BOUND:
        # known to stay under the bound in this dtype: the other dtype must still reject it
        other = "fp16" if dt == "bf16" else "bf16"
        assert (defect, other) not in UNDER_BOUND
        ops, kw, R, M = _sens_setup(SENS[defect], other)
        X = lr.lara_grads(*ops, dtype=torch.float32, round_to=DTYPES[other], defect=defect, **kw)
        res = {n_: lr.bound_report(n_, X[n_], M[n_], R[n_], DTYPES[other]) for n_ in R}
    assert not all(ok for ok, _, _ in res.values()), "the bound accepts defect %s:\n%s" % (defect, "\n".join(t for _, t, _ in res.values()))
