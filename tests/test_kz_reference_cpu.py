"""CPU checks of the same-operand kernelized-attention reference (tests/kz_reference.py, tests/kz_cases.py) that
tests/test_gpu_kz_core.py holds the kernels of csrc/ea_kernelized.hip to:
  a. R reproduces the reference project's stored results: the core of every kz_* fixture through R (q, k, v from the fixture's own
     qkv Linear) gives the fixture's y and dx;
  b. M with its roundings off equals R's autograd to 1e-10 in fp64, every case; two fp32 evaluations of M that differ in the order
     of additions agree on a(.) within a factor 3 on every tensor (the premise of the factor 4: kz_cases.operands, `fourier`);
  c. the conditions on the inputs hold (relu logits and den away from their branch points by 64 times the model's own error, the
     clamp cases on both sides of the clamp, the all-negative key logits, the stabiliser on a padded key);
  d. every case gets the slice plan and the feature block it records (the formula, the dispatcher's rule and the library's own
     ea_kernelized_parts agree);
  e. what the C ABI refuses, it refuses with the recorded code before any launch (NULL device pointers; no device needed);
  f. the model-relative bound accepts M at ratio one and rejects M with ONE deliberate defect, ten of them."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases_kernelized                 # noqa: E402
import kz_cases as kzc                  # noqa: E402
import kz_reference as kr               # noqa: E402
from kz_checks import KzFixture, feature_matrix   # noqa: E402

F64 = torch.float64
EA_E_BADARG, EA_E_UNSUPPORTED = -1, -2
MAP_ID = {"favorp": 0, "relu": 1, "fourier": 2, "relu-only": 3, "sigmoid-only": 4, "dpfp": 5}

_SETUP = {}


def _setup(name, dt="fp32"):
    if (name, dt) not in _SETUP:
        c, o, redrawn = kzc.operands(name, dt)
        _SETUP[(name, dt)] = (c, o, redrawn, kr.reference(c, o), kr.model(c, o))
    return _SETUP[(name, dt)]


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------------
# a. R against the reference project's fixtures
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cases_kernelized.MODES)
@pytest.mark.parametrize("name", sorted(cases_kernelized.CASES))
def test_reference_reproduces_the_fixtures(name, mode):
    fx = KzFixture(name)
    a = fx.case["args"]
    heads, mp, m, cos = a["num_heads"], a["proj_method"], a["approx_attn_dim"], a["cos_weighting"]
    params = {k: torch.from_numpy(v).to(F64) for k, v in fx.params_np.items()}
    W = feature_matrix(fx, mode, params, "cpu", F64)
    x = torch.from_numpy(fx.x_np).to(F64)
    B, C = x.shape[0], x.shape[-1]
    xs = x.reshape(B, -1, C)
    N, d = xs.shape[1], C // heads
    assert d == 64
    qkv = (xs @ params["qkv.weight"].t() + params["qkv.bias"]).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    g = torch.from_numpy(fx.g_np).to(F64).reshape(B, N, C)
    dout = (g @ params["proj.weight"]).reshape(B, N, heads, d).permute(0, 2, 1, 3)
    mask = None if fx.mask_np is None else torch.from_numpy(fx.mask_np).bool()
    c = dict(map=mp, m=m, cos=cos, B=B, h=heads, N=N)
    R = kr.reference(c, dict(q=qkv[0], k=qkv[1], v=qkv[2], dout=dout, W=W, mask=mask))
    y = R["out"].permute(0, 2, 1, 3).reshape(B, N, C) @ params["proj.weight"].t() + params["proj.bias"]
    dqkv = torch.stack([R["dq"], R["dk"], R["dv"]], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * C)
    dx = dqkv @ params["qkv.weight"]

    def close(got, ref, what):
        # the bounds of tests/test_kernelized_cpu.py (the reference ran in fp32)
        got, ref = got.reshape(-1), torch.from_numpy(ref).to(F64).reshape(-1)
        dlt = got - ref
        assert float(dlt.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()) <= 1e-5 and float(dlt.abs().max() / ref.abs().max()) <= 2e-5, (name, mode, what)
    close(y, fx.y(mode), "y")
    close(dx, fx.dx(mode), "dx")
    assert abs(float((R["den"] < 1e-2).double().mean()) - float(fx.z["%s.clamped_fraction" % mode])) < 1e-9


# ------------------------------------------------------------------------------------------------------------------------
# b. the model against the reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kzc.NAMES + sorted(kzc.PERFORMER_ONLY))
def test_model_without_roundings_is_the_reference(name):
    c, o, _, R, _ = _setup(name)
    X = kr.model(c, o, dtype=F64, rounding=False)
    assert set(kr.compared(X)) == set(kr.compared(R))
    for n_ in list(kr.compared(R)) + ["den"]:
        assert X[n_].shape == R[n_].shape and _rel(X[n_], R[n_]) <= 1e-10, n_
    BH, F = c["B"] * c["h"], c["F"]
    assert tuple(R["kv"].shape) == (BH, F, 64) and tuple(R["dksum"].shape) == (BH, F)
    assert ("dW" in R) == (c["map"] in kr.W_MAPS) and ("p_st" in R) == (c["map"] in kr.STAT_SIDES)
    if "p_st" in R:
        assert tuple(R["p_st"].shape) == (BH, kr.STAT_SIDES[c["map"]])


@pytest.mark.parametrize("name,dt", kzc.RUNS)
def test_unmutated_model_passes_at_ratio_one(name, dt):
    c, o, _, R, M = _setup(name, dt)
    io = kzc.DTYPES[dt]
    for n_ in kr.compared(R):
        ok, txt, ratio = kr.bound_report(n_, M[n_], M[n_], R[n_], io)
        assert ok and (ratio == 1.0 or kr.a_err(M[n_], R[n_]) == 0.0), txt
        assert kr.a_err(M[n_], R[n_]) <= 0.01, txt             # a rounding-level perturbation of R, not another function
        want = 2.0 ** -20 if (dt == "fp32" or n_ not in kr.IO_NAMES) else (2.0 ** -9 if dt == "bf16" else 2.0 ** -12)
        assert kr.floor_for(n_, io) == want


@pytest.mark.parametrize("name", [n_ for n_ in kzc.NAMES if kzc.CASES[n_]["map"] in kr.W_MAPS])
def test_two_fp32_evaluations_of_the_model_agree_on_the_figure(name):
    """The premise of a(HIP) <= 4 a(M) + f: another fp32 evaluation of the same function -- here M with the 64 channels of q, k, W
    permuted alike, i.e. another order of additions in every logit -- has an a(.) within a factor 3 of M's on every tensor whose
    bound is not the floor's.  (Without the den gap of the fourier cases the two were up to 31 times apart: kz_cases.operands.)"""
    c, o, _, R, M = _setup(name)
    lo, hi = (1.0, ""), (1.0, "")
    for seed_ in range(3):
        X = kr.model(c, o, reorder=seed_)
        for n_ in kr.compared(R):
            am = kr.a_err(M[n_], R[n_])
            if am < 2.0 ** -20:
                continue
            r = kr.a_err(X[n_], R[n_]) / am
            lo, hi = min(lo, (r, n_)), max(hi, (r, n_))
    print("\n%s: a(M') / a(M) over 3 reorderings and all tensors: %.2f (%s) .. %.2f (%s)" % ((name,) + lo + hi))
    assert hi[0] <= 3.0 and lo[0] >= 1 / 3.0


def test_floor_for_keeps_its_earlier_answers():
    for rt in (torch.bfloat16, torch.float16, None):
        for n_ in ("out", "dq", "dk", "dv"):
            assert kr.floor_for(n_, rt) == (2.0 ** -9 if rt == torch.bfloat16 else 2.0 ** -12)
        for n_ in ("lse", "dbias", "kv", "dW"):
            assert kr.floor_for(n_, rt) == 2.0 ** -20
    assert all(kr.floor_for(n_, torch.float32) == 2.0 ** -20 for n_ in ("out", "dq", "dk", "dv", "kv"))


# ------------------------------------------------------------------------------------------------------------------------
# c. conditions on the inputs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", kzc.RUNS)
def test_den_is_away_from_the_clamp(name, dt):
    """min |den - 1e-2| >= 64 max |den(M) - den(R)|: the clamp decision is the same in fp32 and fp64 for every query."""
    c, o, redrawn, R, M = _setup(name, dt)
    margin = float((R["den"] - 1e-2).abs().min())
    err = float((M["den"].double() - R["den"]).abs().max())
    print("\n%s %s: min |den - 1e-2| %.3e, max |den(M) - den(R)| %.3e (%.0f times), %d tokens redrawn" % (
        name, dt, margin, err, margin / max(err, 1e-300), redrawn))
    assert margin >= 64 * err
    assert bool(((R["den"] < 1e-2) == (M["den"] < 1e-2)).all())


@pytest.mark.parametrize("name", [n_ for n_ in kzc.NAMES if kzc.CASES[n_]["map"] == "relu"])
def test_relu_logits_are_away_from_zero(name):
    """min |l| over all query and key logits >= 64 max |l(M) - l(R)|: relu's branch is the same in fp32 and fp64."""
    c, o, redrawn, R, M = _setup(name)
    cc, Wd = 64 ** -0.25, o["W"].double()
    worst, margin = 0.0, float("inf")
    for x, lm in ((o["q"], M["_lq"]), (o["k"], M["_lk"])):
        l = cc * torch.einsum("bhnd,hjd->bhnj", x.double(), Wd)
        worst, margin = max(worst, float((lm.detach().double() - l).abs().max())), min(margin, float(l.abs().min()))
        assert bool(((l > 0) == (lm > 0)).all())
    print("\n%s: min |l| %.3e, max |l(M) - l(R)| %.3e (%.0f times), %d tokens redrawn" % (name, margin, worst, margin / worst, redrawn))
    assert margin >= 64 * worst and margin >= kzc.RELU_MARGIN


@pytest.mark.parametrize("name", sorted(kzc.CLAMP))
def test_clamp_cases_have_queries_on_both_sides(name):
    c, o, _, R, _ = _setup(name)
    frac = float((R["den"] < 1e-2).double().mean())
    print("\n%s: %.1f %% of the queries clamped" % (name, 100 * frac))
    if kzc.CLAMP[name] is None:
        assert 0.0 < frac < 1.0
    else:
        assert kzc.CLAMP[name][0] <= frac <= kzc.CLAMP[name][1]


def test_fully_padded_row_is_clamped_everywhere():
    for name in ("mask_favorp_m64", "mask_dpfp_nu1"):
        c, o, _, R, _ = _setup(name)
        assert bool(o["mask"][1].all()) and bool((R["den"][1] == 0).all()) and bool((R["out"][1] == 0).all())
        assert bool(o["mask"][0, 70:96].all()) and not bool(o["mask"][0, 64:70].any())       # padding inside a tile
        for n_ in ("dk", "dv"):
            assert bool((R[n_][o["mask"][:, None, :].expand(c["B"], c["h"], c["N"])] == 0).all())


def test_statistics_cases_tell_the_variants_apart():
    """stat_favorp_m16_n70: every key logit is negative and the last tile is ragged, so zero rows would win the key maximum.
    mask_favorp_m64: in some (b,h) the largest key logit belongs to a padded key, so a maximum over the unpadded keys differs."""
    c, o, _, R, _ = _setup("stat_favorp_m16_n70")
    l = 64 ** -0.25 * torch.einsum("bhnd,hjd->bhnj", o["k"].double(), o["W"].double())
    assert float(l.max()) < -0.1 and c["N"] % 64 == 6 and bool((R["p_st"] < -0.1).all())
    c, o, _, R, _ = _setup("mask_favorp_m64")
    l = 64 ** -0.25 * torch.einsum("bhnd,hjd->bhnj", o["k"].double(), o["W"].double())
    live = l.masked_fill(o["mask"][:, None, :, None], -float("inf")).amax((-1, -2))
    assert int((live[[0, 2]] < l.amax((-1, -2))[[0, 2]] - 0.1).sum()) >= 1


# ------------------------------------------------------------------------------------------------------------------------
# d. the plan of every case
# ------------------------------------------------------------------------------------------------------------------------
def _geom(c, dtype=2, **over):
    from efficient_attention import _native as nv
    f = dict(B=c["B"], H=c["h"], N=c["N"], D=64, dtype=dtype, map=MAP_ID[c["map"]], M=c["m"] if c["map"] in kr.W_MAPS else 0, F=c["F"],
             nu=(c["m"] // 64) // 2 if c["map"] == "dpfp" else 0, cos=int(c["cos"]))
    f.update(over)
    return nv.ea_kz_geom(f["B"], f["H"], f["N"], f["D"], f["dtype"], f["map"], f["M"], f["F"], f["nu"], f["cos"])


@pytest.mark.parametrize("name", kzc.NAMES)
def test_every_case_gets_the_plan_it_records(name):
    from efficient_attention import _native as nv
    c = kzc.CASES[name]
    assert kzc.plan(c["B"] * c["h"], c["N"]) == (c["S"], c["tps"])
    assert int(nv.lib().ea_kernelized_parts(ctypes.byref(_geom(c)))) == c["S"]
    assert kzc.feature_block(c["map"], c["m"]) == c["fb"]
    assert c["F"] == kr.base_features(c) * (2 if c["cos"] else 1) <= 256 and c["F"] % c["fb"] == 0


def test_case_table_says_what_it_claims():
    C = kzc.CASES
    pairs = {(C[n_]["map"], C[n_]["cos"]) for n_ in C if C[n_]["fb"] == 32}
    assert len(pairs) == 12                                                      # every (map, cos) instantiation at fb = 32
    assert {(C[n_]["map"], C[n_]["m"]) for n_ in C if C[n_]["fb"] == 16} >= {("favorp", 16), ("favorp", 48), ("relu", 16), ("relu", 112),
                                                                              ("fourier", 16), ("fourier", 48), ("relu", 80)}
    assert sorted(C[n_]["F"] for n_ in ("favorp_m128_cos", "fourier_m128", "fourier_m64_cos", "dpfp_nu2", "dpfp_nu1_cos")) == [256] * 5
    L1, L2 = C["L1_fourier_m32"], C["L2_relu_m48_cos"]
    tok = lambda c, s: max(0, min(c["N"], (s + 1) * c["tps"]) - s * c["tps"])      # noqa: E731
    n1 = [tok(L1, s) for s in range(L1["S"])]
    assert n1[:32] == [128] * 32 and n1[32] == 34 and n1[33:] == [0] * 31
    assert [tok(L2, s) for s in range(L2["S"])] == [128, 128, 44, 0] and L2["B"] * L2["h"] == 258
    assert int(kzc._mask(L2).any(1).sum()) == 4
    assert (C["L3_favorp_m64_n64"]["N"], C["L3_favorp_m64_n1"]["N"]) == (64, 1)
    assert not C["relu_m64_nodw"]["need_dw"] and all(C[n_]["need_dw"] for n_ in C if C[n_]["map"] in kr.W_MAPS and n_ != "relu_m64_nodw")
    a, b = kzc.operands("relu_m64")[1], kzc.operands("relu_m64_nodw")[1]
    assert all(torch.equal(a[n_], b[n_]) for n_ in ("q", "k", "v", "dout", "W"))
    base = C["favorp_m64"]
    assert (base["B"], base["h"], base["N"], base["S"], base["tps"]) == (2, 2, 200, 4, 64) and int(kzc._mask(base)[1].sum()) == 37
    assert len(kzc.RUNS) == len(kzc.NAMES) + 2 * len(kzc.BOTH16)


# ------------------------------------------------------------------------------------------------------------------------
# e. refusals of the C ABI (kz_fill and the pointer checks of the entries in csrc/ea_capi.hip: all before any launch)
# ------------------------------------------------------------------------------------------------------------------------
def _entries(g):
    """Every entry on geometry g with NULL device pointers -> {name: code}."""
    from efficient_attention import _native as nv
    lib, gp, N = nv.lib(), ctypes.byref(g), None
    return {
        "parts": int(lib.ea_kernelized_parts(gp)),
        "stats": lib.ea_kernelized_stats(gp, N, N, N, N, N),
        "kv": lib.ea_kernelized_kv(gp, *([N] * 8)),
        "out": lib.ea_kernelized_out(gp, *([N] * 7)),
        "bwd_q": lib.ea_kernelized_bwd_q(gp, *([N] * 11)),
        "bwd_k": lib.ea_kernelized_bwd_k(gp, *([N] * 11)),
    }


def _kg(mp="relu", m=64, cos=0, F=None, nu=0, raw_cos=None, **over):
    c = dict(map=mp, m=m, cos=bool(cos), B=2, h=2, N=200)
    Fb = {"favorp": m, "relu": m, "fourier": 2 * m, "relu-only": 64, "sigmoid-only": 64, "dpfp": 128 * max(nu, 0)}[mp]
    c["F"] = Fb * (2 if cos else 1) if F is None else F
    if raw_cos is not None:
        over["cos"] = raw_cos
    return _geom(c, nu=nu, **over)


@pytest.mark.parametrize("mp", kr.W_MAPS)
@pytest.mark.parametrize("m", [0, 8, 24, 144])
def test_w_map_sizes_outside_the_kernels_are_unsupported(mp, m):
    got = _entries(_kg(mp, m))
    assert got == {n_: EA_E_UNSUPPORTED for n_ in got}, got


@pytest.mark.parametrize("kw", [dict(mp="fourier", m=128, cos=1), dict(mp="dpfp", nu=0, F=0), dict(mp="dpfp", nu=0, F=128), dict(mp="dpfp", nu=3),
                                dict(mp="relu", m=64, F=128), dict(mp="relu", m=64, cos=1, F=64), dict(mp="fourier", m=32, F=32),
                                dict(mp="relu-only", F=128), dict(mp="relu", D=32), dict(mp="relu", D=128)],
                         ids=["fourier_m128_cos_F512", "dpfp_nu0", "dpfp_nu0_F128", "dpfp_nu3_F384", "F_is_2Fb_without_cos", "F_is_Fb_with_cos",
                              "fourier_F_is_m", "reluonly_F128", "D32", "D128"])
def test_well_formed_geometries_outside_the_kernels_are_unsupported(kw):
    """More than 256 features, dpfp without a roll, F that is not the map's feature count, D != 64: EA_E_UNSUPPORTED from every
    entry, the plan query included (include/ea_hip.h: 'geometry outside what the kernels are built for')."""
    got = _entries(_kg(**kw))
    assert got == {n_: EA_E_UNSUPPORTED for n_ in got}, got


@pytest.mark.parametrize("kw", [dict(B=0), dict(H=0), dict(N=0), dict(dtype=3), dict(dtype=-1), dict(map=6), dict(map=-1), dict(raw_cos=2)],
                         ids=["B0", "H0", "N0", "dtype3", "dtype-1", "map6", "map-1", "cos2"])
def test_malformed_geometries_are_bad_arguments(kw):
    got = _entries(_kg(**kw))
    assert got == {n_: EA_E_BADARG for n_ in got}, got


def test_entry_level_refusals_with_null_pointers():
    """A well-formed geometry with NULL device pointers: the plan query answers, every launch entry answers EA_E_BADARG.  The
    statistics entry refuses a map without statistics with EA_E_BADARG as well (the geometry is one the kernels are built for; the
    CALL is inconsistent), the dW partials likewise for a map without W (tests/test_gpu_kz_core.py, on real tensors)."""
    for g in (_kg("favorp", 64), _kg("fourier", 32, cos=1), _kg("relu", 48, cos=1), _kg("relu-only"), _kg("sigmoid-only", cos=1), _kg("dpfp", nu=2)):
        got = _entries(g)
        assert got.pop("parts") == 4
        assert got == {n_: EA_E_BADARG for n_ in got}, got


def test_stats_entry_refuses_a_map_without_statistics_before_it_looks_at_pointers():
    """With placeholder (non-NULL) pointers: favorp gets as far as the launch where there is no device (a positive hipError_t), the
    maps without statistics are refused -- so this half runs only without a device, where an accepted call cannot start a kernel
    on placeholder addresses."""
    if torch.cuda.is_available():
        return
    from efficient_attention import _native as nv
    lib = nv.lib()
    buf = torch.zeros(64)
    X = ctypes.c_void_p(buf.data_ptr())
    t4 = nv.ea_t4(buf.data_ptr(), 64, 64, 64)
    T = ctypes.byref(t4)
    assert lib.ea_kernelized_stats(ctypes.byref(_kg("favorp", 64)), T, T, X, X, None) > 0
    for g in (_kg("relu", 64), _kg("relu-only"), _kg("sigmoid-only"), _kg("dpfp", nu=1)):
        assert lib.ea_kernelized_stats(ctypes.byref(g), T, T, X, X, None) == EA_E_BADARG


@pytest.mark.parametrize("m,code", [(16, 0), (48, 0), (80, 0), (96, 0), (112, EA_E_UNSUPPORTED), (128, EA_E_UNSUPPORTED), (24, EA_E_UNSUPPORTED),
                                    (0, EA_E_UNSUPPORTED)])
def test_performer_f32_feature_counts(m, code):
    """ea_performer_f32_* takes m <= 96 in multiples of 16: m = 16, 48, 80 are accepted (the plan query answers S), the rest is
    EA_E_UNSUPPORTED from every entry."""
    from efficient_attention import _native as nv
    lib, N = nv.lib(), None
    gp = ctypes.byref(nv.ea_perf_geom(2, 2, 200, 64, 2, m))
    got = dict(parts=int(lib.ea_performer_f32_parts(gp)), kmax=lib.ea_performer_f32_kmax(gp, N, N, N, N), kv=lib.ea_performer_f32_kv(gp, *([N] * 8)),
               out=lib.ea_performer_f32_out(gp, *([N] * 6)), bwd_q=lib.ea_performer_f32_bwd_q(gp, *([N] * 9)),
               bwd_k=lib.ea_performer_f32_bwd_k(gp, *([N] * 10)))
    if code == 0:
        assert got.pop("parts") == 4 and got == {n_: EA_E_BADARG for n_ in got}, got       # (NULL pointers)
    else:
        assert got == {n_: code for n_ in got}, got


# ------------------------------------------------------------------------------------------------------------------------
# f. sensitivity of the model-relative bound
# ------------------------------------------------------------------------------------------------------------------------
SENS = {"second_16_columns_dropped": "relu_m64", "fourier_cos_reads_sin": "fourier_m16", "cos_angle_tile_local": "relu_m64_cos",
        "kv_slice_missing": "dpfp_nu1", "dw_second_tile_overwrites": "L2_relu_m48_cos", "padded_keys_in_ksum": "reluonly",
        "padded_keys_off_stabiliser": "mask_favorp_m64", "zero_rows_in_key_max": "stat_favorp_m16_n70", "dden_not_clamped": "clamp_fourier_m32",
        "dpfp_roll_negated": "dpfp_nu2"}
# defects that stay under the bound on their case: reported with their figure, the case is not tuned (none observed)
UNDER_BOUND = set()


def test_every_defect_has_its_case():
    assert set(SENS) == set(kr.DEFECTS) and len(kr.DEFECTS) == 10


@pytest.mark.parametrize("defect", kr.DEFECTS)
def test_bound_rejects_single_defect(defect):
    name = SENS[defect]
    c, o, _, R, M = _setup(name)
    X = kr.model(c, o, defect=defect)
    io = torch.float32
    names = kr.compared(R)
    exc = {n_: kr.excess(n_, X[n_], M[n_], R[n_], io) for n_ in names}
    worst = max(exc, key=exc.get)
    rejected = sorted(n_ for n_ in names if not kr.bound_report(n_, X[n_], M[n_], R[n_], io)[0])
    print("\n%s on %s: %.3g times its bound (%s); rejected on %s" % (defect, name, exc[worst], worst, rejected))
    if defect in UNDER_BOUND:
        assert not rejected, "defect %s is now rejected: take it out of UNDER_BOUND" % defect
    else:
        assert rejected, "defect %s stays under the bound on %s (%.3g of it)" % (defect, name, exc[worst])
