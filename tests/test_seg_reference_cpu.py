"""CPU checks of the same-operand reference of LARA's 1-D proposals and the overlapping adaptive pool (tests/seg_reference.py) that
tests/test_gpu_seg_core.py holds lara_segment_kernel, seglin_col_kernel, seglin_dg_kernel and pool2d_*_kernel to:
  a. R equals the oracle in fp64 to 1e-12: oracle.attention.lara_landmarks_1d (+ _mlp) on even and uneven splits, with and without
     the generators; the pool against oracle.geometry.adaptive_pool_matrix and torch.nn.AdaptiveAvgPool2d; the module's folded
     construction (bias_q = b_q G^T + g_b, masked rows zeroed then mbias) against the reference's "zero q before the Linear";
  b. the model's hand-written arithmetic with the roundings off equals R's autograd to 1e-10, every case; the unmutated model
     passes its own bound at ratio one;
  c. the case table says what it claims (segment lengths, iterations per pass, ea_lara_seglin_groups, NCT, G1's mask);
  d. the conditions on the inputs (properties of R alone);
  e. what the C ABI refuses, it refuses with the documented code before any launch (no device needed);
  f. the model-relative bound rejects the model with ONE deliberate defect and accepts the control variant (an identity)."""
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

import seg_cases as sc                  # noqa: E402
import seg_reference as sr              # noqa: E402
from oracle import attention as oa      # noqa: E402
from oracle import geometry as og       # noqa: E402

F64 = torch.float64
EA_E_BADARG, EA_E_UNSUPPORTED = -1, -2
EA_BF16, EA_F16, EA_F32 = 0, 1, 2
DT = ("bf16", "fp16")


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------------
# a. reference against oracle
# ------------------------------------------------------------------------------------------------------------------------
def _gen_params(g):
    P = {}
    for sd in ("q", "k"):
        P["G" + sd], P["gb" + sd] = 0.125 * torch.randn(64, 64, dtype=F64, generator=g), 0.1 * torch.randn(64, dtype=F64, generator=g)
        P["lw" + sd], P["lb" + sd] = 1 + 0.2 * torch.randn(64, dtype=F64, generator=g), 0.1 * torch.randn(64, dtype=F64, generator=g)
    return P


def _oracle_params(P):
    out = {}
    for sd in ("q", "k"):
        out["%s_bar_gen.0.weight" % sd], out["%s_bar_gen.0.bias" % sd] = P["G" + sd], P["gb" + sd]
        out["%s_bar_gen.1.weight" % sd], out["%s_bar_gen.1.bias" % sd] = P["lw" + sd], P["lb" + sd]
    return out


@pytest.mark.parametrize("N,L", [(96, 16), (130, 16), (17, 16), (333, 7), (150, 49), (130, 64)])
def test_segment_means_equal_lara_landmarks_1d(N, L):
    B, h = 2, 2
    g = torch.Generator().manual_seed(3 + N + L)
    q, k = [torch.randn(B, h, N, 64, dtype=F64, generator=g) for _ in range(2)]
    P = _gen_params(g)
    zero = torch.zeros(B, h, L, 64, dtype=F64)
    zb = torch.zeros(B, h, N, 64, dtype=F64)
    # with the generators: seglin's R
    rq, rk = oa.lara_landmarks_1d(q, k, L, _oracle_params(P), dict(proposal_gen="adaptive-1d"))
    c = dict(fam="H", B=B, h=h, N=N, L=L, D=64)
    got = sr.seglin_reference(c, dict(P, xq=q, xk=k, d_qbar=zero, d_kbar=zero, base_q=zb, base_k=zb))
    assert _rel(got["qbar"], rq) <= 1e-12 and _rel(got["kbar"], rk) <= 1e-12
    # without: the segment kernel's plain means
    rq, rk = oa.lara_landmarks_1d(q, k, L, {}, dict(proposal_gen="pool-1d"))
    none = dict(mask=None, bias_q=None, bias_k=None, mbias_q=None, mbias_k=None, gq=None, cq=None, gk=None, ck=None)
    got = sr.segment_reference(dict(c, ln=False), dict(none, xq=q, xk=k, d_qbar=zero, d_kbar=zero))
    assert _rel(got["qbar"], rq) <= 1e-12 and _rel(got["kbar"], rk) <= 1e-12
    assert sum(sr.seg_sizes(N, L)) == N and sorted(sr.seg_sizes(N, L)) == sr.seg_sizes(N, L)          # short segments first


def test_folded_construction_equals_zeroing_q_before_the_linear():
    """The module's folded form: stored rows = G (x W_head^T) without any bias, zeroed for masked tokens; bias_q = b_q G^T + g_b for
    ordinary tokens, mbias = g_b for masked ones.  The reference zeroes q (= x W^T + b_q) of masked tokens before the Linear."""
    B, h, N, L, Cm = 2, 3, 50, 8, 24
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, N, Cm, dtype=F64, generator=g)
    Wq, Wk = [torch.randn(h, 64, Cm, dtype=F64, generator=g) / Cm ** 0.5 for _ in range(2)]
    bq, bk = [0.3 * torch.randn(h, 64, dtype=F64, generator=g) for _ in range(2)]
    P = _gen_params(g)
    mask = torch.zeros(B, N, dtype=torch.bool)
    mask[0, 9:21] = True
    mask[1, 44:] = True
    keep = (~mask)[:, None, :, None].to(F64)
    q = (torch.einsum("bnc,hdc->bhnd", x, Wq) + bq[None, :, None]) * keep
    k = (torch.einsum("bnc,hdc->bhnd", x, Wk) + bk[None, :, None]) * keep
    rq, rk = oa.lara_landmarks_1d(q, k, L, _oracle_params(P), dict(proposal_gen="adaptive-1d"))
    o = dict(xq=torch.einsum("bnc,hdc,ed->bhne", x, Wq, P["Gq"]) * keep, xk=torch.einsum("bnc,hdc,ed->bhne", x, Wk, P["Gk"]) * keep,
             bias_q=bq @ P["Gq"].t() + P["gbq"], bias_k=bk @ P["Gk"].t() + P["gbk"], mbias_q=P["gbq"], mbias_k=P["gbk"],
             gq=P["lwq"], cq=P["lbq"], gk=P["lwk"], ck=P["lbk"], mask=mask,
             d_qbar=torch.zeros(B, h, L, 64, dtype=F64), d_kbar=torch.zeros(B, h, L, 64, dtype=F64))
    got = sr.segment_reference(dict(fam="G", B=B, h=h, N=N, L=L, D=64, ln=True), o)
    assert _rel(got["qbar"], rq) <= 1e-12 and _rel(got["kbar"], rk) <= 1e-12


@pytest.mark.parametrize("name", sc.P_NAMES)
def test_pool_equals_the_oracle_and_torch(name):
    c, o = sc.operands(name, "bf16")
    gh, gw, side, D = c["gh"], c["gw"], c["side"], c["D"]
    R = sr.pool_reference(c, o)
    K = torch.kron(og.adaptive_pool_matrix(gh, side, F64), og.adaptive_pool_matrix(gw, side, F64))
    x = o["x"].double()
    assert _rel(R["mean"], torch.einsum("ln,bhnd->bhld", K, x)) <= 1e-12
    img = x.permute(0, 1, 3, 2).reshape(c["B"] * c["h"], D, gh, gw)
    ref = torch.nn.AdaptiveAvgPool2d(side)(img).reshape(c["B"], c["h"], D, side * side).permute(0, 1, 3, 2)
    assert _rel(R["mean"], ref) <= 1e-12
    assert _rel(R["dx_inc"], torch.einsum("ln,bhld->bhnd", K, o["d_mean"].double())) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------
# b. the model without its roundings is the reference
# ------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _setup(name, dt):
    """(c, o, R, M) of a case in a dtype, computed once and shared."""
    if (name, dt) not in _CACHE:
        c, o = sc.operands(name, dt)
        _CACHE[name, dt] = (c, o, sr.reference(c, o), sr.model(c, o, sc.DTYPES[dt]))
    return _CACHE[name, dt]


@pytest.mark.parametrize("name", sc.NAMES)
def test_model_arithmetic_without_roundings_is_the_reference(name):
    c, o, R, _ = _setup(name, "bf16")
    X = sr.model_exact(c, o)
    assert set(X) == set(R)
    for n_ in R:
        assert X[n_].shape == R[n_].shape and _rel(X[n_], R[n_]) <= 1e-10, n_


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.NAMES)
def test_unmutated_model_passes_at_ratio_one(name, dt):
    c, o, R, M = _setup(name, dt)
    for n_ in R:
        ok, txt, ratio = sr.bound_report(n_, M[n_], M[n_], R[n_], sc.DTYPES[dt])
        assert ok and (ratio == 1.0 or sr.a_err(M[n_], R[n_]) == 0.0), txt
        assert sr.a_err(M[n_], R[n_]) <= 0.02, txt         # a rounding-level perturbation of R, not another function
    fp32 = [n_ for n_ in R if n_ not in ("dq", "dk", "dx", "dq_inc", "dk_inc", "dx_inc", "dG")]
    if not c.get("raw_G"):
        for n_ in fp32:                                     # fp32 outputs of same-operand arithmetic: fp32-level model error
            assert sr.a_err(M[n_], R[n_]) <= 2e-5, (n_, sr.a_err(M[n_], R[n_]))
    assert sr.floor_for("dq", sc.DTYPES[dt]) == (2.0 ** -9 if dt == "bf16" else 2.0 ** -12) and sr.floor_for("part", sc.DTYPES[dt]) == 2.0 ** -20


# ------------------------------------------------------------------------------------------------------------------------
# c. the case table
# ------------------------------------------------------------------------------------------------------------------------
def _geom(B, h, N, L, D=64, dtype=EA_BF16):
    from efficient_attention import _native as nv
    return nv.ea_geom(B, h, N, D, dtype, 0, 1, N, 0, 0, 0, L, float(max(D, 1)) ** -0.5, 0, 0)        # (nv.make_geom's fields; D = 0 allowed)


def _split(name):
    s = sr.seg_sizes(sc.CASES[name]["N"], sc.CASES[name]["L"])
    lo = min(s)
    return lo, s.count(lo), len(s) - s.count(lo)


def test_case_table_says_what_it_claims():
    C = sc.CASES
    assert len(sc.NAMES) == 23 and len(sc.G_NAMES) == 6 and len(sc.H_NAMES) == 8 and len(sc.F_NAMES) == 5 and len(sc.P_NAMES) == 4
    assert all(C[n_]["what"] for n_ in C)
    assert {n_: _split(n_) for n_ in ("G1", "G2", "G3", "G4", "G5", "G6")} == {
        "G1": (8, 14, 2), "G2": (14, 5, 2), "G3": (1, 15, 1), "G4": (85, 3, 1), "G5": (62, 8, 8), "G6": (8, 14, 2)}
    assert {n_: _split(n_) for n_ in sc.H_NAMES} == {"H1": (8, 14, 2), "H2": (1, 15, 1), "H3": (47, 3, 4), "H4": (3, 46, 3),
                                                      "H5": (275, 3, 1), "H6": (2, 62, 2), "H7": (8, 14, 2), "H8": (8, 14, 2)}
    assert all(_split(n_) == (47, 3, 4) for n_ in sc.F_NAMES)
    # lara_segment_kernel: RPI = 8 rows per iteration at D 64, 16 at D 32; two iterations per trip
    assert sc.steps(9, 8) == 2 and sc.steps(8, 8) == 1                                   # G1: 9 > 8 rows
    assert sc.steps(14, 16) == 1 and sc.steps(15, 16) == 1 and C["G2"]["B"] * C["G2"]["h"] * C["G2"]["L"] * 2 == 14
    assert sc.steps(85, 8) == 11 and sc.steps(86, 8) == 11                               # G4: odd count, second row of the last trip idle
    assert sc.steps(62, 16) == 4 and sc.steps(63, 16) == 4 and C["G5"]["D"] == 32 and C["G5"]["ln"] and not C["G5"]["mbias"]
    assert not C["G6"]["ln"] and C["G6"]["bias"] and not C["G6"]["part"] and not C["G2"]["ln"] and not C["G2"]["bias"]
    # seglin: 16 tokens per column step, 32 per dG step
    assert [sc.steps(n_, 16) for n_ in (8, 9)] == [1, 1] and [sc.steps(n_, 32) for n_ in (8, 9)] == [1, 1]
    assert (47 // 16, 47 % 16, 48 // 16, 48 % 16) == (2, 15, 3, 0) and (47 // 32, 47 % 32, 48 % 32) == (1, 15, 16)
    assert (sc.steps(275, 16), 275 % 16, 276 % 16) == (18, 3, 4) and (sc.steps(275, 32), 275 % 32, 276 % 32) == (9, 19, 20)
    assert max(sr.seg_sizes(17, 16)) == 2 and C["H6"]["L"] == 64 and C["H7"]["raw_G"] and C["H7"]["like"] == "H1"
    # the fused finish
    assert [(C[n_]["C"], sc.nct(C[n_]["C"])) for n_ in sc.F_NAMES] == [(49, 4), (16, 2), (32, 2), (33, 4), (64, 4)]
    assert all(C[n_]["like"] == "H3" and C[n_]["scale"] == 64 ** -0.5 for n_ in sc.F_NAMES)
    a, b = sc.operands("H3", "bf16")[1], sc.operands("F1", "bf16")[1]
    assert all(torch.equal(a[n_], b[n_]) for n_ in a)
    # H4: more waves' worth of segments than the column passes hold on any device of up to 304 CUs; 7 segments per dG wave
    h4 = C["H4"]
    assert h4["B"] * h4["h"] * 2 * h4["L"] == 6272 and 6272 > 12 * 304 and h4["B"] * h4["h"] * 4 * h4["L"] == 12544
    for cus in (64, 256, 304):
        for bwd in (False, True):
            per, cg, spg = sr.col_groups(h4["B"], h4["h"], h4["L"], cus, bwd)
            assert per >= 2 and h4["L"] - (cg - 1) * spg < spg, (cus, bwd, per, cg, spg)         # a shorter last group
    assert sr.seglin_groups(64, 49) == (7, 7)
    # the largest tensor
    assert max(C[n_]["B"] * C[n_]["h"] * C[n_]["N"] * C[n_]["D"] for n_ in C) == 64 * 150 * 64


@pytest.mark.parametrize("name", sc.H_NAMES + sc.F_NAMES)
def test_seglin_groups_query_matches_the_restated_formula(name):
    from efficient_attention import _native as nv
    c = sc.CASES[name]
    g = _geom(c["B"], c["h"], c["N"], c["L"])
    got = int(nv.lib().ea_lara_seglin_groups(ctypes.byref(g)))
    assert got == sr.seglin_groups(c["B"] * c["h"], c["L"])[0], got
    if name == "H4":
        assert got == 7
    else:
        assert got == c["L"]                              # one segment per dG wave everywhere else


def test_mask_of_g1_covers_a_whole_segment_and_part_of_another():
    c = sc.CASES["G1"]
    m = sc.mask_of(c)
    sizes = sr.seg_sizes(c["N"], c["L"])
    pos, cover = 0, []
    for sz in sizes:
        cover.append(float(m[0, pos:pos + sz].double().mean()))
        pos += sz
    assert cover[3] == 1.0 and cover[2] == 0.5 and sum(1 for v in cover if v > 0) == 2
    assert 0 < float(m[1].double().sum()) < 8 and bool(m[1, 100:104].all())
    m5 = sc.mask_of(sc.CASES["G5"])
    assert bool(m5[0, 490:530].all()) and int(m5.sum()) == 40 and sc.mask_of(sc.CASES["G2"]) is None


# ------------------------------------------------------------------------------------------------------------------------
# d. conditions on the inputs
# ------------------------------------------------------------------------------------------------------------------------
def _row_variances(c, o):
    out = []
    for sd in ("q", "k"):
        x = o["x" + sd].double()
        if c["fam"] == "G":
            B, h, N, D = x.shape
            add = torch.zeros(B, h, N, D, dtype=F64) if o["bias_" + sd] is None else o["bias_" + sd].double()[None, :, None].expand(B, h, N, D)
            if o["mask"] is not None and o["mbias_" + sd] is not None:
                add = torch.where(o["mask"][:, None, :, None], o["mbias_" + sd].double().expand(B, h, N, D), add)
            elif o["mask"] is not None:
                add = torch.where(o["mask"][:, None, :, None], torch.zeros((), dtype=F64), add)
            z = x + add
        else:
            z = x @ o["G" + sd].double().t() + o["gb" + sd].double()
        out.append(z.var(-1, unbiased=False))
    return torch.stack(out)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.G_NAMES + sc.H_NAMES)
def test_layernorm_rows_have_the_variance_the_case_claims(name, dt):
    c, o = sc.operands(name, dt)
    if c["fam"] == "G" and not c["ln"]:
        return
    v = _row_variances(c, o)
    print("\n%s %s: per-row variance %.4g .. %.4g" % (name, dt, float(v.min()), float(v.max())))
    if name == "H8":
        assert 1e-3 <= float(v.min()) and float(v.max()) <= 1e-2
    else:
        assert float(v.min()) >= 0.05


def test_eps_is_visible_on_h8():
    """eps = 1e-6 in place of 1e-5 moves qbar of H8 by more than 1e-4 relative."""
    c, o = sc.operands("H8", "bf16")
    a, b = sr.model_exact(c, o), sr.seglin_model(c, o, F64, None, "eps_1e6")
    assert _rel(b["qbar"] - o["lbq"].double(), a["qbar"] - o["lbq"].double()) > 1e-4


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.H_NAMES + sc.F_NAMES + sc.P_NAMES)
def test_gradient_base_is_no_larger_than_the_gradient(name, dt):
    c, o, R, _ = _setup(name, dt)
    rms = lambda t: float(t.double().pow(2).mean().sqrt())                           # noqa: E731
    pairs = [("base", "dx_inc")] if c["fam"] == "P" else [("base_q", "dq_inc"), ("base_k", "dk_inc")]
    for b_, g_ in pairs:
        print("\n%s %s: rms(%s) %.3e, rms(%s) %.3e" % (name, dt, b_, rms(o[b_]), g_, rms(R[g_])))
        assert 0 < rms(o[b_]) <= rms(R[g_])
        assert not bool(((o[b_] == 0) & torch.signbit(o[b_])).any())                 # no negative zero (bit identity of base + 0)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.F_NAMES)
def test_finish_softmax_is_not_one_hot(name, dt):
    c, o = sc.operands(name, dt)
    t = sr._finish_t(o["fin_qbar"].double(), o["xq"].double(), o["fin_lse"].double(), c["scale"])
    print("\n%s %s: max t %.4f, sum_n t in %.6f .. %.6f" % (name, dt, float(t.max()), float(t.sum(-1).min()), float(t.sum(-1).max())))
    assert float(t.max()) < 0.5
    assert float((t.sum(-1) - 1).abs().max()) < 1e-5                                  # lse_t is the log-sum-exp over the sequence (fp32-stored)


# ------------------------------------------------------------------------------------------------------------------------
# e. refusals through the C ABI (every one returns before a launch: fill_seg / fill_seglin and the checks of the entries in
#    ea_capi.hip, pool2d_dispatch and seglin_dispatch)
# ------------------------------------------------------------------------------------------------------------------------
def _entries(g):
    """Every segment / seglin entry on geometry g with NULL device pointers -> {name: code}."""
    from efficient_attention import _native as nv
    lib, gp, N = nv.lib(), ctypes.byref(g), None
    return {
        "segment_fwd": lib.ea_lara_segment_fwd(gp, *([N] * 14)),
        "segment_bwd": lib.ea_lara_segment_bwd(gp, *([N] * 17)),
        "seglin_groups": int(lib.ea_lara_seglin_groups(gp)),
        "seglin_fwd": lib.ea_lara_seglin_fwd(gp, *([N] * 13)),
        "seglin_bwd": lib.ea_lara_seglin_bwd(gp, *([N] * 18)),
        "seglin_bwd_fin": lib.ea_lara_seglin_bwd_fin(gp, *([N] * 20), 49, 0.125, N),
    }


SEGMENT = ("segment_fwd", "segment_bwd")


def test_well_formed_geometry_with_null_pointers_is_a_bad_argument():
    for D in (64, 32):
        got = _entries(_geom(2, 3, 130, 16, D=D))
        want = {n_: EA_E_BADARG for n_ in got}
        if D == 64:
            want["seglin_groups"] = 16
        else:
            want.update({n_: EA_E_UNSUPPORTED for n_ in got if n_.startswith("seglin")})    # seglin is D = 64 only
        assert got == want, (D, got)


@pytest.mark.parametrize("N,L", [(16, 16), (15, 16), (1, 1)])
def test_no_more_tokens_than_segments_is_unsupported(N, L):
    got = _entries(_geom(2, 3, N, L))
    assert got == {n_: EA_E_UNSUPPORTED for n_ in got}, got


def test_fp32_and_d128_are_unsupported_by_the_segment_entries():
    """include/ea_hip.h classes a well-formed geometry outside the kernels as EA_E_UNSUPPORTED (D = 128, L = 65 of the landmark
    block; `dtype EA_F32 ... accepted by the ea_performer_f32_* entry points only`).  fill_seg answered EA_E_BADARG for both
    (lara_segment_dispatch and seglin_dispatch, one call later, EA_E_UNSUPPORTED); it now answers the header's code.  Callers
    test != EA_OK.  Malformed geometries stay EA_E_BADARG."""
    for kw in (dict(dtype=EA_F32), dict(D=128), dict(D=16), dict(D=48)):
        got = _entries(_geom(2, 3, 130, 16, **kw))
        assert got == {n_: EA_E_UNSUPPORTED for n_ in got}, (kw, got)
    for g in (_geom(0, 3, 130, 16), _geom(2, 0, 130, 16), _geom(2, 3, 0, 16), _geom(2, 3, 130, 0), _geom(2, 3, 130, 16, D=0),
              _geom(2, 3, 130, 16, dtype=3), _geom(2, 3, 130, 16, dtype=-1)):
        got = _entries(g)
        assert got == {n_: EA_E_BADARG for n_ in got}, got


def test_fused_finish_refusals_with_null_pointers():
    from efficient_attention import _native as nv
    lib, N = nv.lib(), None
    gp = ctypes.byref(_geom(2, 3, 333, 7))
    for C, s in ((0, 0.125), (49, 0.0), (49, -1.0), (49, float("nan")), (65, 0.125)):
        assert lib.ea_lara_seglin_bwd_fin(gp, *([N] * 20), C, s, N) == EA_E_BADARG          # (NULL pointers are decided first)


def test_pool_refusals_with_null_pointers():
    from efficient_attention import _native as nv
    lib, N = nv.lib(), None
    assert lib.ea_adaptive_pool2d_fwd(EA_BF16, 2, 2, 28, 28, 6, 64, N, N, N) == EA_E_BADARG
    assert lib.ea_adaptive_pool2d_bwd(EA_BF16, 2, 2, 28, 28, 6, 64, N, N, N) == EA_E_BADARG


def test_entry_level_refusals_one_argument_at_a_time():
    """Each refusal next to the call that differs from it in that one argument.  The other pointers are a non-NULL placeholder, so
    the accepted call gets as far as the launch -- which is why this part runs only where there is no device to launch on (the
    accepted call then answers a positive HIP code): with a device, a refusal that got lost would start a kernel on placeholder
    addresses."""
    if torch.cuda.is_available():
        return
    from efficient_attention import _native as nv
    lib = nv.lib()
    buf = torch.zeros(64)
    X, N = ctypes.c_void_p(buf.data_ptr()), None
    assert buf.data_ptr() % 16 == 0
    T = ctypes.byref(nv.ea_t4(buf.data_ptr(), 64 * 130 * 3, 64, 64 * 3))
    ran = lambda rc: rc > 0                                                          # noqa: E731  (got to the launch: no device)
    g = _geom(2, 3, 130, 16)
    gp = ctypes.byref(g)

    def seg_fwd(gq=X, cq=X, gk=X, ck=X, qbar=X, mask=X, bias=X, mbias=X, geom=gp):
        return lib.ea_lara_segment_fwd(geom, T, T, mask, bias, bias, mbias, mbias, gq, cq, gk, ck, qbar, X, N)

    def seg_bwd(gq=X, cq=X, gk=X, ck=X, part=X, dbar=X, tdq=T):
        return lib.ea_lara_segment_bwd(gp, T, T, X, X, X, X, X, gq, cq, gk, ck, dbar, X, tdq, T, part, N)
    assert ran(seg_fwd()) and ran(seg_bwd())
    assert ran(seg_fwd(gq=N, cq=N, gk=N, ck=N, mask=N, bias=N, mbias=N))             # plain means, everything optional NULL
    assert ran(seg_bwd(gq=N, cq=N, gk=N, ck=N, part=N))                              # plain means: part may be NULL (ea_capi.hip)
    assert ran(seg_fwd(geom=ctypes.byref(_geom(2, 3, 130, 16, D=32, dtype=EA_F16))))
    for fn in (seg_fwd, seg_bwd):
        assert fn(gk=N) == EA_E_BADARG and fn(gq=N) == EA_E_BADARG                   # gq without gk and the reverse
        assert fn(cq=N) == EA_E_BADARG and fn(ck=N) == EA_E_BADARG                   # gq without cq / ck
    assert seg_bwd(part=N) == EA_E_BADARG                                            # LayerNorm without part
    assert seg_fwd(qbar=N) == EA_E_BADARG and seg_bwd(dbar=N) == EA_E_BADARG and seg_bwd(tdq=None) == EA_E_BADARG

    P8 = [X] * 8

    def lin_fwd(qbar=X, G=X):
        return lib.ea_lara_seglin_fwd(gp, T, T, G, *P8[1:], qbar, X, N)

    def lin_bwd(stats=X, part=X, dG=X):
        return lib.ea_lara_seglin_bwd(gp, T, T, *P8, X, X, T, T, part, dG, stats, N)

    def lin_fin(C=49, s=0.125, stats=X, fq=X, fu=X, fl=X):
        return lib.ea_lara_seglin_bwd_fin(gp, T, T, *P8, X, X, T, T, X, X, stats, fq, fu, fl, C, s, N)
    assert ran(lin_fwd()) and ran(lin_bwd()) and ran(lin_fin()) and ran(lin_fin(C=64)) and ran(lin_fin(C=1))
    assert lin_fwd(qbar=N) == EA_E_BADARG and lin_fwd(G=N) == EA_E_BADARG
    mis = ctypes.c_void_p(buf.data_ptr() + 4)
    assert lin_bwd(stats=mis) == EA_E_BADARG and lin_fin(stats=mis) == EA_E_BADARG and lin_bwd(stats=N) == EA_E_BADARG
    assert lin_bwd(part=N) == EA_E_BADARG and lin_bwd(dG=N) == EA_E_BADARG
    assert lin_fin(C=0) == EA_E_BADARG and lin_fin(s=0.0) == EA_E_BADARG and lin_fin(s=-0.125) == EA_E_BADARG
    assert lin_fin(C=65) == EA_E_UNSUPPORTED
    assert lin_fin(fq=N) == EA_E_BADARG and lin_fin(fu=N) == EA_E_BADARG and lin_fin(fl=N) == EA_E_BADARG

    def pool(bwd=False, dtype=EA_BF16, gh=28, gw=28, side=6, B=2, D=64):
        if bwd:
            return lib.ea_adaptive_pool2d_bwd(dtype, B, 2, gh, gw, side, D, X, T, N)
        return lib.ea_adaptive_pool2d_fwd(dtype, B, 2, gh, gw, side, D, T, X, N)
    for bwd in (False, True):
        assert ran(pool(bwd)) and ran(pool(bwd, gh=6)) and ran(pool(bwd, dtype=EA_F16))
        assert pool(bwd, gh=5) == EA_E_BADARG and pool(bwd, gw=5) == EA_E_BADARG     # side > gh, side > gw
        assert pool(bwd, side=0) == EA_E_BADARG and pool(bwd, B=0) == EA_E_BADARG and pool(bwd, D=0) == EA_E_BADARG
        assert pool(bwd, dtype=EA_F32) == EA_E_BADARG                                # (pool2d_dispatch's own wording; the header names no code)


# ------------------------------------------------------------------------------------------------------------------------
# f. sensitivity of the model-relative bound
# ------------------------------------------------------------------------------------------------------------------------
SENS = {"short_segments_last": "G1", "long_segments_div_by_segs": "H3", "last_token_dropped": "H5", "row_past_end_counted": "G1",
        "eps_1e6": "H8", "masked_rows_get_bias": "G1", "bias_of_head0": "G1", "dmbias_dbias_swapped": "G1", "dlnb_without_len": "H3",
        "last_segment_of_dg_group_missing": "H4", "lse_natural_units": "F1", "padded_rows_t1": "F1", "finish_on_dk_too": "F3",
        "pool_floor_upper_edge": "P1", "pool_bwd_wrong_count": "P2"}
# (defect, dtype) pairs that stay under the bound on their case (none observed): reported with their figure, the case is
# not tuned
UNDER_BOUND = set()


def _excess(name, X, M, R, td):
    """The largest of the three figures of X over its bound FACTOR * figure(M) + f (> 1: the bound rejects X)."""
    f = sr.floor_for(name, td)
    got = (sr.a_err(X, R),) + sr.norm_errs(X, R)
    mod = (sr.a_err(M, R),) + sr.norm_errs(M, R)
    return max(g_ / (sr.FACTOR * m_ + f) for g_, m_ in zip(got, mod))


def test_every_defect_has_its_case():
    assert set(SENS) == set(sr.DEFECTS) and len(sr.DEFECTS) == 15 and sr.CONTROL not in sr.DEFECTS


def _play(defect, case, dt):
    c, o, R, M = _setup(case, dt)
    td = sc.DTYPES[dt]
    X = sr.model(c, o, td, defect)
    assert set(X) == set(R)
    exc = {n_: _excess(n_, X[n_], M[n_], R[n_], td) for n_ in R}
    worst = max(exc, key=exc.get)
    rejected = sorted(n_ for n_ in R if not sr.bound_report(n_, X[n_], M[n_], R[n_], td)[0])
    print("\n%s on %s %s: %.3g times its bound (%s); rejected on %s" % (defect, case, dt, exc[worst], worst, rejected))
    return rejected, exc[worst], worst


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("defect", sr.DEFECTS)
def test_bound_rejects_single_defect(defect, dt):
    rejected, fig, worst = _play(defect, SENS[defect], dt)
    if (defect, dt) in UNDER_BOUND:
        assert not rejected, "defect %s is now rejected in %s: take it out of UNDER_BOUND" % (defect, dt)
        other = "fp16" if dt == "bf16" else "bf16"
        assert (defect, other) not in UNDER_BOUND
    else:
        assert rejected, "the bound accepts defect %s in %s (largest figure %.2f of its bound, on %s)" % (defect, dt, fig, worst)


@pytest.mark.parametrize("dt", DT)
def test_bound_accepts_the_control_variant(dt):
    """mean(a xhat) with a instead of a - mean(a): the normalised row sums to zero, so this is the same function with another
    rounding pattern.  A harness that rejected it would reject everything."""
    rejected, fig, worst = _play(sr.CONTROL, "H1", dt)
    assert not rejected and fig < 1.0, (rejected, fig, worst)
