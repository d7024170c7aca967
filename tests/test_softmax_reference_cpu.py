"""CPU checks of the same-operand softmax reference (tests/softmax_reference.py) that tests/test_gpu_softmax_core.py holds the
16-bit softmax kernels to:
  a. the reference equals the oracle (oracle/attention.py: softmax_core with a mask and with dropout; the second softmax of
     ra_core for the key-norm term) in fp64 to 1e-12, outputs and gradients, and the rounding model with its roundings switched
     off equals the reference's autograd to 1e-10;
  b. every case of tests/softmax_cases.py gets the tile count it was written for (ea_softmax_tiles at 256 compute units; no GPU
     needed), the dev knobs EA_SM_QT / EA_SM_BQT are sanitised (one fresh process per value: they are read once), and the
     geometries the library refuses are refused without a device;
  c. the model-relative bound rejects the model with ONE deliberate defect, and accepts the unmutated model;
  d. an fp32 emulation of the sampler's formula meets the two shares tests/test_gpu_softmax_core.py demands of the kernel."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import softmax_cases as sc              # noqa: E402
import softmax_reference as sr          # noqa: E402
from oracle import attention as oa      # noqa: E402

F64 = torch.float64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
EA_E_BADARG, EA_E_UNSUPPORTED = -1, -2
LIB = os.path.join(ROOT, "efficient-attention_amd", "lib", "libea_hip.so")


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-300))


def _small(seed, B=2, h=2, N=75, d=16):
    g = torch.Generator().manual_seed(seed)
    q, k, v, dout = [torch.randn(B, h, N, d, dtype=F64, generator=g) for _ in range(4)]
    mask = torch.zeros(B, N, dtype=torch.bool)
    mask[0, N - 9:] = True
    mask[1, :66] = True                                          # a dead leading 64-key chunk
    keep = (torch.rand(B, h, N, N, generator=g) >= 0.3).to(torch.uint8)
    return q, k, v, dout, mask, keep


# ------------------------------------------------------------------------------------------------------------------------
# a. reference against oracle, model arithmetic against reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "mask", "keep", "mask_keep"])
def test_reference_equals_oracle_softmax_core(variant):
    q, k, v, dout, mask, keep = _small(11)
    mask = mask if "mask" in variant else None
    keep = keep if "keep" in variant else None
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ref = oa.softmax_core(*leaves, mask=mask, drop_keep=keep, p_drop=0.3)
    gr = torch.autograd.grad(ref, leaves, dout)
    R = sr.softmax_grads(q, k, v, dout, mask=mask, keep=keep, keep_scale=1.0 / 0.7, dtype=F64, round_to=None, batch_step=1)
    assert _rel(R["out"], ref) <= 1e-12
    for n_, g in zip(("dq", "dk", "dv"), gr):
        assert _rel(R[n_], g) <= 1e-12, n_
    s = q.shape[-1] ** -0.5 * torch.einsum("bhid,bhjd->bhij", q, k)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    assert _rel(R["lse"], torch.logsumexp(s, -1)) <= 1e-12 and _rel(R["delta"], (dout * ref).sum(-1)) <= 1e-12
    if mask is not None:
        pad = mask[:, None, :, None].expand_as(R["dk"])
        assert bool((R["dk"][pad] == 0).all()) and bool((R["dv"][pad] == 0).all())


def test_reference_equals_second_softmax_of_ra_core():
    """ra_core(num_samples = 0): w = q + mean_j k_j + noise, out = softmax_j(s w.k_j - s |k_j|^2 / 2) v_j.  The gradient with
    respect to the noise is the dq of that softmax, dv is direct, and dk is the total less what arrives through the mean."""
    q, k, v, dout, _, _ = _small(12)
    N = q.shape[2]
    noise = torch.zeros_like(q).requires_grad_(True)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ref = oa.ra_core(*leaves, num_samples=0, noise=noise)
    gq, gk, gv, gn = torch.autograd.grad(ref, leaves + [noise], dout)
    w = (q + k.mean(-2, keepdim=True)).detach()
    R = sr.softmax_grads(w, k, v, dout, key_norm_bias=True, dtype=F64, round_to=None)
    assert _rel(R["out"], ref) <= 1e-12 and _rel(R["dq"], gn) <= 1e-12 and _rel(R["dv"], gv) <= 1e-12
    assert _rel(R["dk"], gk - gn.sum(-2, keepdim=True) / N) <= 1e-12


@pytest.mark.parametrize("variant", ["plain", "mask", "keep", "mask_keep", "kb"])
def test_model_arithmetic_without_roundings_is_the_reference(variant):
    """M is window_reference._ModelAttn on this file's logits; with round_to = None it must be the same function as R."""
    q, k, v, dout, mask, keep = _small(13)
    kw = dict(mask=mask if "mask" in variant else None, keep=keep if "keep" in variant else None,
              keep_scale=1.0 / 0.7 if "keep" in variant else 1.0, key_norm_bias=variant == "kb", dtype=F64, round_to=None)
    R = sr.softmax_grads(q, k, v, dout, **kw)
    X = sr.softmax_grads(q, k, v, dout, model=True, **kw)
    assert set(X) == set(R) == set(sr.NAMES)
    for n_ in R:
        assert _rel(X[n_], R[n_]) <= 1e-10, n_


# ------------------------------------------------------------------------------------------------------------------------
# b. plan pins, knobs, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_knobs_are_unset():
    """EA_SM_QT / EA_SM_BQT are read once per process: with either set, the pins below and the GPU file would test another variant."""
    assert "EA_SM_QT" not in os.environ and "EA_SM_BQT" not in os.environ


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_plan_pins(name):
    from efficient_attention import _native as nv
    c = sc.CASES[name]
    got = tuple(int(nv.lib().ea_softmax_tiles(which, c["B"], c["h"], c["N"], c["d"], int(c["keep"]), sc.CUS)) for which in (0, 1))
    assert got == sc.PINS[name], (name, got)


def test_pins_say_what_the_case_table_claims():
    C, P = sc.CASES, sc.PINS
    assert set(C) == set(P) and len(C) == 24
    assert {P[n_][0] for n_ in P} == {1, 2, 4} and {P[n_][1] for n_ in P} == {1, 2}                 # every tile-count template
    for d in (32, 64, 128):                                                                          # every head size, masked, with dropout, with KB
        assert any(C[n_]["d"] == d and C[n_]["mask"] for n_ in C) and any(C[n_]["d"] == d and C[n_]["keep"] for n_ in C)
        assert any(C[n_]["d"] == d and C[n_]["kb"] for n_ in C)
    assert C["S1"]["N"] % 64 == 8 and C["S2"]["N"] % 64 == 0 and C["S3"]["N"] < 64 and C["S6"]["N"] % 64 == 2
    assert bool(sc.case_mask(C["S4"])[1, :64].all()) and not bool(sc.case_mask(C["S4"])[0, :64].any())   # the dead leading chunk
    assert P["Q4"][0] == 4 and C["Q4"]["N"] - 256 == 44 and P["Q2"] == (2, 2) and C["Q2"]["N"] - 128 == 72
    assert P["Q4s"][0] == 4 and C["Q4s"]["d"] == 32 and C["Q4s"]["N"] < 256
    assert P["Q2w"] == (2, 1) and C["Q2w"]["d"] == 128
    assert any(P[n_][0] == 2 and C[n_]["mask"] for n_ in C) and any(P[n_][0] == 4 and C[n_]["mask"] for n_ in C)
    assert P["Q2d"] == (2, 2) and C["Q2d"]["keep"] and P["Q2c"][0] == 2 and C["Q2c"]["keep"]
    # Q2c is the 4 -> 2 clamp: the same geometry without a keep mask gets four tiles
    from efficient_attention import _native as nv
    c = C["Q2c"]
    assert nv.lib().ea_softmax_tiles(0, c["B"], c["h"], c["N"], c["d"], 0, sc.CUS) == 4
    assert P["K2"] == (2, 2) and P["K4"][0] == 4 and all(C[n_]["kb"] and C[n_]["views"] == "separate" for n_ in ("K1", "K1s", "K1w", "K2", "K4"))
    assert all(not (C[n_]["kb"] and C[n_]["keep"]) for n_ in C)
    assert C["V1"]["v_is_k"] and not C["V1"]["kb"] and C["V1"]["views"] == "separate"
    for n_ in C:                                                                                     # keep_ld = 64 ceil(N / 64) > N
        assert not C[n_]["keep"] or C[n_]["N"] % 64 != 0


_CHILD = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
L.ea_softmax_tiles.argtypes = [ctypes.c_int32] * 7
L.ea_softmax_tiles.restype = ctypes.c_int32
# (which, B, H, N, D, has_keep): S1 fwd / bwd, Q4 fwd, Q2 fwd / bwd, D2 (d = 128) fwd / bwd, D1 (keep) fwd
G = [(0, 2, 3, 200, 64, 0), (1, 2, 3, 200, 64, 0), (0, 64, 4, 300, 64, 0), (0, 64, 4, 200, 64, 0), (1, 64, 4, 200, 64, 0),
     (0, 1, 2, 100, 128, 1), (1, 1, 2, 100, 128, 1), (0, 2, 2, 200, 64, 1)]
print(" ".join(str(L.ea_softmax_tiles(*g, 256)) for g in G))
"""
_UNSET = [1, 1, 4, 2, 2, 1, 1, 1]
_KNOBS = [
    ("EA_SM_QT", "3", _UNSET),                                   # no forward template has three tiles: ignored
    ("EA_SM_QT", "8", _UNSET),
    ("EA_SM_QT", "4", [4, 1, 4, 4, 2, 2, 1, 2]),                 # taken; still clamped to two at d = 128 and with a keep mask
    ("EA_SM_BQT", "3", _UNSET),                                  # the backward has one and two tiles only: ignored
    ("EA_SM_BQT", "2", [1, 2, 4, 2, 2, 1, 1, 1]),                # taken; still one tile at d = 128
    ("EA_SM_QT", "-2", _UNSET),
]


@pytest.mark.parametrize("knob,value,want", _KNOBS, ids=["%s=%s" % (k_, v_) for k_, v_, _ in _KNOBS])
def test_knob_values_are_sanitised(knob, value, want):
    """A fresh process per value (the knobs are read once into a static).  A count no kernel template has must not reach the
    launcher: it would size the grid for that many tiles per wave and launch the one-tile kernel, leaving most queries unwritten
    without an error."""
    from efficient_attention import _native as nv
    nv.lib()                                                      # (built)
    env = {k_: v_ for k_, v_ in os.environ.items() if k_ not in ("EA_SM_QT", "EA_SM_BQT")}
    env[knob] = value
    r = subprocess.run([sys.executable, "-c", _CHILD, LIB], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split()] == want, (knob, value, r.stdout)


def test_unsupported_calls_are_refused_without_a_device():
    from efficient_attention import _native as nv
    lib = nv.lib()
    assert lib.ea_softmax_tiles(0, 2, 3, 200, 48, 0, sc.CUS) == EA_E_BADARG
    assert lib.ea_softmax_tiles(1, 2, 3, 0, 64, 0, sc.CUS) == EA_E_BADARG
    assert lib.ea_softmax_tiles(2, 2, 3, 200, 64, 0, sc.CUS) == EA_E_BADARG and lib.ea_softmax_tiles(0, 2, 3, 200, 64, 0, -1) == EA_E_BADARG
    # the entry points themselves: a refused call returns before any HIP call, the rows are never dereferenced
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    t = ctypes.byref(nv.ea_t4(base, 200 * 3 * 64, 64, 3 * 64))
    p = ctypes.c_void_p(base)

    def fwd(N, D, keep, kb):
        return lib.ea_softmax_attn_fwd(2, 3, N, D, nv.EA_BF16, 0.125, t, t, t, None, t, p, keep, 1.25, kb, None)

    def bwd(N, D, keep, kb):
        return lib.ea_softmax_attn_bwd(2, 3, N, D, nv.EA_BF16, 0.125, t, t, t, None, t, t, p, p, t, t, t, keep, 1.25, kb, None)
    for call in (fwd, bwd):
        assert call(200, 64, p, 1) == EA_E_UNSUPPORTED            # the key-norm term with a keep mask
        assert call(200, 48, None, 0) == EA_E_BADARG
        assert call(0, 64, None, 0) == EA_E_BADARG


# ------------------------------------------------------------------------------------------------------------------------
# c. sensitivity of the model-relative bound
# ------------------------------------------------------------------------------------------------------------------------
SENS = {"padded_keys_in_normaliser": "S4", "tail_keys_missing": "S1", "last_query_tile_unwritten": "S1",
        "dp_without_keep_scale": "D1", "dropout_in_normaliser": "D1", "kb_missing_in_forward": "K1", "kb_grad_missing_in_dk": "K1",
        "delta_without_keep_scale": "D1"}
_SENS = {}
# (defect, dtype) known to stay under the bound; the other dtype must reject it.  Cases are not tuned until a
# defect trips.
UNDER_BOUND = set()


def _sens_setup(name, dt):
    key = (name, dt)
    if key not in _SENS:
        io = DTYPES[dt]
        c, o = sc.operands(name, io)
        ops, kw = (o["q"], o["k"], o["v"], o["dout"]), sc.reference_kw(c, o)
        _SENS[key] = (ops, kw, sr.softmax_grads(*ops, dtype=F64, round_to=None, **kw),
                      sr.softmax_grads(*ops, dtype=torch.float32, round_to=io, **kw))
    return _SENS[key]


def _excess(name, X, M, R, io):
    """The largest of the three figures of X over its bound FACTOR * figure(M) + f (> 1: the bound rejects X)."""
    f = sr.floor_for(name, io)
    got = (sr.a_err(X, R),) + sr.norm_errs(X, R)
    mod = (sr.a_err(M, R),) + sr.norm_errs(M, R)
    return max(g_ / (sr.FACTOR * m_ + f) for g_, m_ in zip(got, mod))


def test_defect_table_is_complete():
    assert set(SENS) == set(sr.DEFECTS) and len(sr.DEFECTS) == 8


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(set(SENS.values())))
def test_unmutated_model_passes_at_ratio_one(name, dt):
    ops, kw, R, M = _sens_setup(name, dt)
    for n_ in R:
        ok, txt, ratio = sr.bound_report(n_, M[n_], M[n_], R[n_], DTYPES[dt])
        assert ok and ratio == 1.0, txt
        # and the model is a rounding-level perturbation of the reference, not a different function
        assert sr.a_err(M[n_], R[n_]) <= (0.05 if dt == "bf16" else 0.01), txt


def _verdict(defect, dt):
    io = DTYPES[dt]
    ops, kw, R, M = _sens_setup(SENS[defect], dt)
    X = sr.softmax_grads(*ops, dtype=torch.float32, round_to=io, defect=defect, **kw)
    res = {n_: sr.bound_report(n_, X[n_], M[n_], R[n_], io) for n_ in R}
    exc = {n_: _excess(n_, X[n_], M[n_], R[n_], io) for n_ in R}
    return res, exc


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("defect", sr.DEFECTS)
def test_bound_rejects_single_defect(defect, dt):
    res, exc = _verdict(defect, dt)
    worst = max(exc, key=exc.get)
    print("\n%s/%s exceeds the bound by a factor %.3g (%s); rejected on %s" % (
        defect, dt, exc[worst], worst, sorted(n_ for n_, (ok, _, _) in res.items() if not ok)))
    if (defect, dt) in UNDER_BOUND:
        other = "fp16" if dt == "bf16" else "bf16"
        assert (defect, other) not in UNDER_BOUND
        assert all(ok for ok, _, _ in res.values()), "%s/%s is listed as under the bound and is not" % (defect, dt)
        res, exc = _verdict(defect, other)
    assert not all(ok for ok, _, _ in res.values()), "the bound accepts defect %s:\n%s" % (defect, "\n".join(t for _, t, _ in res.values()))


# ------------------------------------------------------------------------------------------------------------------------
# d. the sampler's shares are attainable: an fp32 emulation of the kernel's formula meets them on the test's inputs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", sc.SAMPLER_SHAPES, ids=["x".join(map(str, s)) for s in sc.SAMPLER_SHAPES])
@pytest.mark.parametrize("seed", sc.SAMPLER_SEEDS, ids=["seed32", "seed64"])
def test_fp32_emulation_of_the_sampler_meets_the_shares(seed, shape, dt):
    q, k = sr.sampler_operands(shape, DTYPES[dt])
    score = sr.gumbel_scores(q, k, seed)                          # fp64 [B,h,N,N]
    draw = sr.fp32_emulated_draw(q, k, seed)                      # the kernel's formula in float32
    assert int(draw.min()) >= 0 and int(draw.max()) < shape[2]
    near, exact = sr.sampler_shares(score, draw)
    print("\nfp32 emulation %s %s seed %#x: near %.4f exact %.4f" % (shape, dt, seed, near, exact))
    assert near >= sr.NEAR_SHARE and exact >= sr.EXACT_SHARE
