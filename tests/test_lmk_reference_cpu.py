"""CPU checks of the same-operand landmark-pipeline reference (tests/lmk_reference.py) that tests/test_gpu_lmk_core.py holds
lmk2_kernel (csrc/ea_lmk2.hip) to:
  a. R equals the oracle in fp64 to 1e-12: oracle.attention._mlp; the mixing lines of lara_landmarks_2d (pooling = identity, with
     and without '-vmixed'); omega of lara_core for the three sample modes; and R's omega, qbar_rows, bhv, lp fed into
     lara_reference.lara_estimator reproduce oracle.attention.lara_core for the three estimators;
  b. the model's hand-written arithmetic with the roundings off equals R's autograd to 1e-10, every case;
  c. the conditions on the inputs (properties of R alone): mis-opt cases keep at least half of bhv in [0.05, 0.95], mixed cases keep
     the largest entry of at least half of the rows of A below 0.9;
  d. what the C ABI refuses, it refuses with the documented code before any launch (NULL device pointers; no device needed);
  e. the model-relative bound accepts the unmutated model at ratio one and rejects the model with ONE deliberate defect."""
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

import lara_reference as lar            # noqa: E402
import lmk_cases as lc                  # noqa: E402
import lmk_reference as lr              # noqa: E402
from oracle import attention as oa      # noqa: E402

F64 = torch.float64
EA_E_BADARG, EA_E_UNSUPPORTED = -1, -2
ORACLE_MIS = {"opt": "mis-opt", "biased": "mis-biased", "bh": "mis-bh"}


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-300))


def _geo(D, L, dup=0, has_mlp=0, mixed=0, mis="opt", eva=0, BH=4):
    return dict(D=D, L=L, C=L * (2 if dup else 1), dup=dup, has_mlp=has_mlp, mixed=mixed, mis=mis, eva=eva, BH=BH, scale=float(D) ** -0.5)


def _per_bh(params, BH):
    return {n_: t.unsqueeze(0).expand(BH, *t.shape) for n_, t in params.items()}


def _draw_params(D, g):
    return dict(Wq=torch.randn(D, D, dtype=F64, generator=g) / D ** 0.5, bq=0.1 * torch.randn(D, dtype=F64, generator=g),
                gq=0.7 + 0.1 * torch.randn(D, dtype=F64, generator=g), cq=0.1 * torch.randn(D, dtype=F64, generator=g),
                Wk=torch.randn(D, D, dtype=F64, generator=g) / D ** 0.5, bk=0.1 * torch.randn(D, dtype=F64, generator=g),
                gk=0.6 + 0.1 * torch.randn(D, dtype=F64, generator=g), ck=0.1 * torch.randn(D, dtype=F64, generator=g))


def _oracle_params(P):
    return {"q_bar_gen.2.weight": P["Wq"], "q_bar_gen.2.bias": P["bq"], "q_bar_gen.3.weight": P["gq"], "q_bar_gen.3.bias": P["cq"],
            "k_bar_gen.2.weight": P["Wk"], "k_bar_gen.2.bias": P["bk"], "k_bar_gen.3.weight": P["gk"], "k_bar_gen.3.bias": P["ck"]}


# ------------------------------------------------------------------------------------------------------------------------
# a. reference against oracle
# ------------------------------------------------------------------------------------------------------------------------
def test_mlp_equals_the_oracle():
    g = torch.Generator().manual_seed(11)
    BH, L, D = 5, 9, 32
    P = _draw_params(D, g)
    x = torch.randn(BH, L, D, dtype=F64, generator=g)
    ref = oa._mlp(x, _oracle_params(P), ("q_bar_gen.2", "q_bar_gen.3"))
    Pb = _per_bh(P, BH)
    assert _rel(lr.mlp(x, Pb["Wq"], Pb["bq"], Pb["gq"], Pb["cq"]), ref) <= 1e-12


@pytest.mark.parametrize("gen", ["pool-mixed", "pool-vmixed", "no-param-pool-mixed", "pool"])
@pytest.mark.parametrize("L", [49, 16, 64])
def test_mixing_equals_lara_landmarks_2d(L, gen):
    """q, k on a side x side grid with side^2 = L landmarks: the adaptive pooling is the identity, pq = q, pk = k."""
    B, h, D = 2, 2, 32
    side = int(L ** 0.5)
    g = torch.Generator().manual_seed(13 + L)
    q, k, v = [0.8 * torch.randn(B, h, L, D, dtype=F64, generator=g) for _ in range(3)]
    P = _draw_params(D, g)
    scale = D ** -0.5
    args = dict(num_landmarks=L, proposal_gen=gen, pool_module_type="light")
    q_bar, k_bar = oa.lara_landmarks_2d(q, k, v, side, side, _oracle_params(P), args, scale)
    has_mlp, mixed = int(gen.startswith("pool")), int(gen.endswith("mixed"))
    colbias = torch.log(v.norm(dim=-1) + 1e-4).reshape(B * h, L) if gen.endswith("-vmixed") else None
    c = _geo(D, L, has_mlp=has_mlp, mixed=mixed, mis="bh", BH=B * h)
    f = lr.lmk_forward(q.reshape(B * h, L, D), k.reshape(B * h, L, D), _per_bh(P, B * h) if has_mlp else None, None, colbias, c)
    assert _rel(f["q_bar"], q_bar.reshape(B * h, L, D)) <= 1e-12
    assert _rel(f["k_bar"], k_bar.reshape(B * h, L, D)) <= 1e-12
    assert _rel(f["mu"], (q_bar + k_bar).reshape(B * h, L, D)) <= 1e-12


MODES = {"single": 0, "antithetic": 1, "multisample": 2}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("mis", ["opt", "biased", "bh"])
def test_outputs_feed_the_estimator_like_lara_core(mis, mode):
    """omega against lara_core's own; R's four outputs through lara_reference.lara_estimator give lara_core's result."""
    B, h, N, d, L = 2, 2, 40, 16, 6
    dup = MODES[mode]
    g = torch.Generator().manual_seed(17 + 3 * dup + len(mis))
    q, k, v = [torch.randn(B, h, N, d, dtype=F64, generator=g) for _ in range(3)]
    q_bar, k_bar = [0.5 * torch.randn(B, h, L, d, dtype=F64, generator=g) for _ in range(2)]
    mu = q_bar + k_bar
    noise = 0.5 * torch.randn(B, h, L * (2 if dup == 2 else 1), d, dtype=F64, generator=g)
    scale, kappa = d ** -0.5, 0.7
    ref, aux = oa.lara_core(q, k, v, None, q_bar, mu, noise, ORACLE_MIS[mis], kappa, mode, scale, return_aux=True)
    c = _geo(d, L, dup=dup, mis=mis, BH=B * h)
    f = lr.lmk_forward(q_bar.reshape(B * h, L, d), k_bar.reshape(B * h, L, d), None, noise.reshape(B * h, -1, d), None, c)
    C = c["C"]
    assert _rel(f["omega"].view(B, h, C, d), aux["omega"]) <= 1e-12

    def v4(t, *tail):
        return None if t is None else t.view(B, h, C, *tail)
    out, _, _ = lar.lara_estimator(q, k, v, None, v4(f["omega"], d), v4(f["qbar_rows"], d), v4(f["bhv"]), v4(f["lp"]), mis=mis,
                                   kappa=kappa, scale=scale, dtype=F64)
    assert (f["qbar_rows"] is None) == (mis == "bh") and (f["bhv"] is None) == (mis != "opt")
    assert _rel(out, ref) <= 1e-12


def test_eva_mode_equals_the_oracle_formulas():
    """eva.py:178-190 as oracle.attention.module_forward's mu_fn states it: rf_k_bar = _mlp(k mean), omega = (rf_q_bar + rf_k_bar) / 2 + eps."""
    g = torch.Generator().manual_seed(19)
    BH, L, D = 4, 7, 32
    P = _draw_params(D, g)
    pq, pk, noise = [torch.randn(BH, L, D, dtype=F64, generator=g) for _ in range(3)]
    op = _oracle_params(P)
    rq, rk = oa._mlp(pq, op, ("q_bar_gen.2", "q_bar_gen.3")), oa._mlp(pk, op, ("k_bar_gen.2", "k_bar_gen.3"))
    f = lr.lmk_forward(pq, pk, _per_bh(P, BH), noise, None, _geo(D, L, has_mlp=1, eva=1, BH=BH))
    assert _rel(f["qbar_rows"], rk) <= 1e-12 and _rel(f["omega"], 0.5 * (rq + rk) + noise) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------
# b. the model without its roundings is the reference
# ------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _setup(name):
    """(c, o, R, M) of a case, computed once and shared."""
    if name not in _CACHE:
        c, o = lc.operands(name)
        _CACHE[name] = (c, o, lr.reference(c, o, use=c["use"]), lr.model(c, o, use=c["use"]))
    return _CACHE[name]


@pytest.mark.parametrize("name", lc.NAMES)
def test_model_arithmetic_without_roundings_is_the_reference(name):
    c, o, R, _ = _setup(name)
    X = lr.lmk_grads(c, o, dtype=F64, model=True, round16=False, use=c["use"])
    assert set(X) == set(R)
    for n_ in R:
        assert X[n_].shape == R[n_].shape and _rel(X[n_], R[n_]) <= 1e-10, n_
    BH, D = c["BH"], c["D"]
    if c["has_mlp"]:
        assert tuple(R["dW_part"].shape) == (BH, 2, D, D) and tuple(R["dvec_part"].shape) == (BH, 2, 3, D)
    assert ("d_colbias" in R) == bool(c["cb"]) and ("bhv" in R) == (c["mis"] == "opt" and not c["eva"])
    assert ("qbar_rows" in R) == (c["eva"] or c["mis"] != "bh")


@pytest.mark.parametrize("name", lc.NAMES)
def test_unmutated_model_passes_at_ratio_one(name):
    c, o, R, M = _setup(name)
    for n_ in R:
        ok, txt, ratio = lr.bound_report(n_, M[n_], M[n_], R[n_], lr.H16)
        exact = lr.a_err(M[n_], R[n_]) == 0.0               # (qbar_rows = pq without the MLP: no arithmetic at all)
        assert ok and (ratio == 1.0 or exact), txt
        assert lr.a_err(M[n_], R[n_]) <= 0.01, txt         # a rounding-level perturbation of R, not another function
        assert lr.floor_for(n_, lr.H16) == 2.0 ** -20       # every result is fp32


def test_case_table_says_what_it_claims():
    C = lc.CASES
    assert len(lc.NAMES) == 16 and all(4 <= C[n_]["BH"] <= 6 for n_ in C)
    assert C["G1o"]["L"] % 16 == 1 and {C[n_]["mis"] for n_ in ("G1o", "G1b", "G1h")} == {"opt", "biased", "bh"}
    assert C["G2"]["dup"] == 1 and C["G2"]["C"] == 2 * C["G2"]["L"] and not C["G2"]["mixed"]
    assert C["G3o"]["dup"] == 2 and C["G3o"]["C"] == 64 and not C["G3o"]["has_mlp"] and C["G3o"]["mixed"]
    assert C["G4"]["D"] == 32 and C["G4"]["L"] == 64
    assert not (C["G5"]["has_mlp"] or C["G5"]["mixed"] or C["G5"]["saved_fwd"] or C["G5"]["saved_bwd"]) and C["G5"]["C"] == 14
    assert C["G6"]["cb"] and C["G6"]["L"] == 33 and not C["G7"]["noise"]
    assert [C[n_]["S"] for n_ in ("G8a", "G8b", "G8c")] == [1, 3, 4] and all(C[n_]["dom_scale"] == 0.125 for n_ in ("G8a", "G8b", "G8c"))
    assert C["G9"]["use"] == ("g_omega", "g_lp") and C["E1"]["eva"] and C["E2"]["eva"] and not C["E2"]["noise"]
    a, b = lc.operands("G1o")[1], lc.operands("G8b")[1]
    assert all(a[n_] is None or bool((a[n_] == b[n_]).all()) for n_ in a if n_ != "parts") and b["parts"].shape[1] == 3


# ------------------------------------------------------------------------------------------------------------------------
# c. conditions on the inputs
# ------------------------------------------------------------------------------------------------------------------------
def _forward64(name):
    c, o = lc.operands(name)
    d = lambda t: None if t is None else t.double()                                  # noqa: E731
    P = _per_bh({n_: d(o[n_]) for n_ in lr.PARAMS}, c["BH"]) if c["has_mlp"] else None
    return c, lr.lmk_forward(d(o["pq"]), d(o["pk"]), P, d(o["noise"]), d(o["colbias"]), c)


@pytest.mark.parametrize("name", lc.OPT)
def test_bhv_is_not_saturated(name):
    c, f = _forward64(name)
    b = f["bhv"]
    share = float(((b >= 0.05) & (b <= 0.95)).double().mean())
    print("\n%s: share of bhv in [0.05, 0.95] %.2f (min %.3f, max %.3f); mean s |mu|^2 %.2f" % (
        name, share, float(b.min()), float(b.max()), float(c["scale"] * (f["mu"] ** 2).sum(-1).mean())))
    assert share >= 0.5


@pytest.mark.parametrize("name", lc.MIXED)
def test_mixing_rows_are_not_one_hot(name):
    c, f = _forward64(name)
    top = f["A"].amax(-1)
    share = float((top < 0.9).double().mean())
    print("\n%s: share of the rows of A with largest entry below 0.9: %.2f (largest %.3f)" % (name, share, float(top.max())))
    assert share >= 0.5


# ------------------------------------------------------------------------------------------------------------------------
# d. refusals through the C ABI (every one of them returns before a launch: fill_lmk and the pointer checks of the entries in
#    ea_capi.hip, the `saved` check of lara_lmk_dispatch in ea_lmk2.hip)
# ------------------------------------------------------------------------------------------------------------------------
def _lg(BH=4, L=49, C=None, D=64, has_mlp=1, mixed=1, mis=0, dup=0, eva=0):
    from efficient_attention import _native as nv
    return nv.ea_lmk_geom(BH, L, L if C is None else C, D, has_mlp, mixed, mis, dup, float(max(D, 1)) ** -0.5, eva)


def _entries(g):
    """Every entry on geometry g with NULL device pointers -> {name: code}."""
    from efficient_attention import _native as nv
    lib, gp, N = nv.lib(), ctypes.byref(g), None
    return {
        "fwd": lib.ea_lara_landmarks_fwd(gp, *([N] * 17)),
        "fwd_cb": lib.ea_lara_landmarks_fwd_cb(gp, *([N] * 18)),
        "bwd": lib.ea_lara_landmarks_bwd(gp, *([N] * 21)),
        "bwd_parts": lib.ea_lara_landmarks_bwd_parts(gp, *([N] * 12), 2, N, 0.125, *([N] * 9)),
        "bwd_cb": lib.ea_lara_landmarks_bwd_cb(gp, *([N] * 23)),
        "saved_floats": int(lib.ea_lara_landmarks_saved_floats(gp)),
    }


def test_saved_floats_formula():
    from efficient_attention import _native as nv
    for BH, L, D, dup in ((6, 49, 64, 0), (5, 16, 64, 1), (4, 64, 32, 0), (5, 7, 32, 1), (1, 1, 32, 0)):
        g = _lg(BH=BH, L=L, C=L * (2 if dup else 1), D=D, dup=dup)
        assert int(nv.lib().ea_lara_landmarks_saved_floats(ctypes.byref(g))) == BH * (3 * L * D + 64 * L + 128)


@pytest.mark.parametrize("kw", [dict(L=65, C=65), dict(L=64, C=128, dup=1), dict(D=128), dict(D=16), dict(D=48)],
                         ids=["L65", "C128", "D128", "D16", "D48"])
def test_geometries_outside_the_kernels_are_unsupported(kw):
    """L, C <= 64 and D in {32, 64}: a well-formed geometry outside them is EA_E_UNSUPPORTED from every entry, the size query
    included (include/ea_hip.h; D = 128 used to answer EA_E_BADARG from fill_lmk while the header classed it as unsupported)."""
    got = _entries(_lg(**kw))
    assert got == {n_: EA_E_UNSUPPORTED for n_ in got}, got


@pytest.mark.parametrize("kw", [dict(L=49, C=50), dict(L=16, C=16, dup=1), dict(L=16, C=48, dup=2), dict(mis=3), dict(mis=-1), dict(dup=3, L=16, C=32),
                                dict(eva=1, dup=1, L=16, C=32, mixed=0), dict(eva=1, has_mlp=0, mixed=0), dict(BH=0), dict(D=0)],
                         ids=["C!=L", "dup1_C!=2L", "dup2_C!=2L", "mis3", "mis-1", "dup3", "eva_dup", "eva_no_mlp", "BH0", "D0"])
def test_malformed_geometries_are_bad_arguments(kw):
    """The size query looks at the geometry alone, so its answer is fill_lmk's: EA_E_BADARG here, the formula for the well-formed
    neighbour."""
    got = _entries(_lg(**kw))
    assert got == {n_: EA_E_BADARG for n_ in got}, got
    ok = _lg(L=16, C=32, dup=1)
    assert _entries(ok)["saved_floats"] == 4 * (3 * 16 * 64 + 64 * 16 + 128)


def test_entry_level_refusals_with_null_pointers():
    """A well-formed geometry with NULL device pointers: every entry answers EA_E_BADARG and launches nothing.  (Which of an
    entry's own checks fires cannot be told apart with NULL pointers; tests/test_gpu_lmk_core.py repeats `_cb` without mixed,
    dom_S = 0 and 5, dup with NULL noise and the backward without `saved` on real tensors, next to the accepted call.)"""
    from efficient_attention import _native as nv
    lib, N = nv.lib(), None
    for g in (_lg(), _lg(mixed=0), _lg(L=16, C=32, dup=1), _lg(has_mlp=0, mixed=0, L=7, C=14, D=32, dup=1)):
        got = _entries(g)
        assert got.pop("saved_floats") > 0
        assert got == {n_: EA_E_BADARG for n_ in got}, got
    gp = ctypes.byref(_lg())
    for S in (0, 5):
        assert lib.ea_lara_landmarks_bwd_parts(gp, *([N] * 12), S, N, 0.125, *([N] * 9)) == EA_E_BADARG


def test_entry_level_refusals_one_argument_at_a_time():
    """Each refusal next to the call that differs from it in that one argument.  The other pointers are a non-NULL placeholder, so
    the accepted call gets as far as the launch -- which is why this part runs only where there is no device to launch on (the
    accepted call then answers hipErrorNoDevice, a positive code): with a device, a refusal that got lost would start a kernel on
    placeholder addresses.  tests/test_gpu_lmk_core.py repeats the refusals whose accepted neighbour is harmless on real tensors."""
    if torch.cuda.is_available():
        return
    from efficient_attention import _native as nv
    lib = nv.lib()
    X, N = ctypes.c_void_p(torch.zeros(16).data_ptr()), None
    P8 = [X] * 8

    def fwd(g, noise=X, saved=X):
        return lib.ea_lara_landmarks_fwd(ctypes.byref(g), X, X, *P8, noise, X, X, X, X, saved, N)

    def fwd_cb(g):
        return lib.ea_lara_landmarks_fwd_cb(ctypes.byref(g), X, X, *P8, X, X, X, X, X, X, X, N)

    def bwd(g, noise=X, saved=X):
        return lib.ea_lara_landmarks_bwd(ctypes.byref(g), X, X, *P8, noise, X, X, X, X, X, X, X, X, saved, N)

    def bwd_parts(g, S, saved=X):
        return lib.ea_lara_landmarks_bwd_parts(ctypes.byref(g), X, X, *P8, X, X, S, X, 0.125, X, X, X, X, X, X, X, saved, N)

    def bwd_cb(g, saved=X):
        return lib.ea_lara_landmarks_bwd_cb(ctypes.byref(g), X, X, *P8, X, X, X, X, X, X, X, X, X, X, X, saved, N)
    ran = lambda rc: rc > 0                                                          # noqa: E731  (got to the launch: no device)
    full, anti = _lg(), _lg(L=16, C=32, dup=1, mixed=0)
    assert ran(fwd(full)) and ran(bwd(full)) and ran(fwd_cb(full)) and ran(bwd_cb(full)) and ran(bwd_parts(full, 1)) and ran(bwd_parts(full, 4))
    assert bwd_parts(full, 0) == EA_E_BADARG and bwd_parts(full, 5) == EA_E_BADARG
    assert fwd_cb(_lg(mixed=0)) == EA_E_BADARG and bwd_cb(_lg(mixed=0)) == EA_E_BADARG
    assert ran(fwd(anti)) and ran(bwd(anti)) and fwd(anti, noise=N) == EA_E_BADARG and bwd(anti, noise=N) == EA_E_BADARG
    # the backward of a mixed or parametrised geometry needs the forward's workspace; the plain one does not
    for g in (full, _lg(mixed=0), _lg(has_mlp=0)):
        assert ran(fwd(g, saved=N)) and bwd(g, saved=N) == EA_E_BADARG and bwd_parts(g, 2, saved=N) == EA_E_BADARG
    assert bwd_cb(full, saved=N) == EA_E_BADARG
    plain = _lg(has_mlp=0, mixed=0, L=7, C=14, D=32, dup=1)
    assert ran(bwd(plain, saved=N)) and ran(fwd(plain, saved=N))


# ------------------------------------------------------------------------------------------------------------------------
# e. sensitivity of the model-relative bound
# ------------------------------------------------------------------------------------------------------------------------
SENS = {"antithetic_sign_missing": "G2", "nrep_missing_in_normaliser": "G2", "pad_columns_unmasked": "G1o", "colbias_along_rows": "G6",
        "fold_missing": "G2", "dqs_first_copy_only": "G2", "eva_half_missing": "E1", "dom_scale_on_d_omega_only": "G8b",
        "dgamma_dbeta_swapped": "G1o", "ln_xhat_term_dropped": "G1o"}
# defects that stay under the bound on their case (none observed): reported with their figure, the case is not tuned
UNDER_BOUND = set()


def _excess(name, X, M, R):
    """The largest of the three figures of X over its bound FACTOR * figure(M) + f (> 1: the bound rejects X)."""
    f = lr.floor_for(name, lr.H16)
    got = (lr.a_err(X, R),) + lr.norm_errs(X, R)
    mod = (lr.a_err(M, R),) + lr.norm_errs(M, R)
    return max(g_ / (lr.FACTOR * m_ + f) for g_, m_ in zip(got, mod))


def test_every_defect_has_its_case():
    assert set(SENS) == set(lr.DEFECTS) and len(lr.DEFECTS) == 10


@pytest.mark.parametrize("defect", lr.DEFECTS)
def test_bound_rejects_single_defect(defect):
    c, o, R, M = _setup(SENS[defect])
    X = lr.lmk_grads(c, o, dtype=torch.float32, model=True, round16=True, defect=defect, use=c["use"])
    assert set(X) == set(R)
    exc = {n_: _excess(n_, X[n_], M[n_], R[n_]) for n_ in R}
    worst = max(exc, key=exc.get)
    rejected = sorted(n_ for n_ in R if not lr.bound_report(n_, X[n_], M[n_], R[n_], lr.H16)[0])
    print("\n%s on %s: %.1f times its bound (%s); rejected on %s" % (defect, SENS[defect], exc[worst], worst, rejected))
    if defect in UNDER_BOUND:
        assert not rejected, "defect %s is now rejected: take it out of UNDER_BOUND" % defect
    else:
        assert rejected, "the bound accepts defect %s (largest figure %.2f of its bound, on %s)" % (defect, exc[worst], worst)
