"""-m "not gpu": the vocabulary cross-entropy's backward (ea_vocab_nll_grad, ea_gemm_nt16, ea_vocab_nll_ws, C ABI 38) and
DecoderStack.loss: the header, the binding, the workspace formula, what the entries refuse before any launch (no pointer is
dereferenced), the interface, and the host reference (tests/vocab_loss_reference.py) on hand-computed values."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import vocab_loss_reference as ref
import vocab_score_reference as sref

ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
BM, BN, SL = sref.constants()
_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_GRAD_ARGS = ["int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
              "int32_t w_dtype", "const int64_t* targets", "const float* lse", "const float* d", "int32_t v0", "int32_t Vc",
              "void* g", "int64_t ldg", "void* gt", "int64_t ldm", "void* stream"]
_GEMM_ARGS = ["int32_t M", "int32_t N", "int32_t K", "const void* a", "int64_t lda", "const void* b", "int64_t ldb",
              "int32_t dtype", "float* out", "int64_t ldo", "int32_t accumulate", "void* stream"]


def _up64(n):
    return (n + 63) // 64 * 64


# ---- C ABI 38 -------------------------------------------------------------------------------------------------------------------
def test_abi_38_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION == 38
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def declared(ret, name):
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (ret, name), text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("int32_t", "ea_vocab_nll_chunk") == ["int32_t M", "int32_t V"]
    assert declared("int64_t", "ea_vocab_nll_ws") == ["int32_t M", "int32_t K", "int32_t V", "int32_t chunk_cols"]
    assert declared("int", "ea_vocab_nll_grad") == _GRAD_ARGS
    assert declared("int", "ea_gemm_nt16") == _GEMM_ARGS
    I, L, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    S = _native.SIGNATURES
    assert S["ea_vocab_nll_chunk"] == [I, I] and S["ea_vocab_nll_ws"] == [I, I, I, I]
    assert S["ea_vocab_nll_grad"] == [I, I, I, P, I, L, P, I, P, P, P, I, I, P, L, P, L, P]
    assert S["ea_gemm_nt16"] == [I, I, I, P, L, P, L, I, P, L, I, P]
    assert _native.lib().ea_vocab_nll_ws.restype is ctypes.c_int64
    assert set(S) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]
    doc = open(HEADER).read()
    assert "ABI 38" in doc and "EA_VOCAB_NLL_BUDGET" in doc and "a guess" in doc
    assert int(re.search(r"#define EA_VOCAB_NLL_BUDGET (\d+)", doc).group(1)) == 256 << 20


def test_the_workspace_is_its_documented_formula(lib):  # noqa: F811
    from efficient_attention import _native
    ws, chunk = _native.lib().ea_vocab_nll_ws, _native.lib().ea_vocab_nll_chunk

    def formula(M, K, V, cc):
        Vc, ldm = min(cc, V), _up64(M)
        ldg = _up64(Vc)
        return 2 * (M * ldg + Vc * ldm + K * ldg + K * ldm)
    for M, K, V, cc in ((1, 32, 16, SL), (BM + 1, 288, 40, SL), (130, 64, SL + 8, SL), (BM, 1056, 2 * SL + BN + 8, SL),
                        (2048, 256, 32768, 2 * SL), (9216, 1024, 32768, 3 * SL), (9216, 1024, 262144, 3 * SL), (7, 96, 5000, 4 * SL)):
        assert ws(M, K, V, cc) == formula(M, K, V, cc), (M, K, V, cc)
    # the default chunk: the widest whole number of slices whose two G images fit the budget; never below one slice, never
    # beyond the table rounded up to slices
    budget = 256 << 20
    for M, V in ((1, 16), (256, 32768), (2048, 32768), (9216, 32768), (9216, 262144), (100000, 262144), (1 << 20, 262144)):
        cc = chunk(M, V)
        want = max(SL, min(budget // (2 * (M + _up64(M))) // SL * SL, -(-V // SL) * SL))
        assert cc == want and cc % SL == 0 and cc >= SL, (M, V, cc, want)
        if cc > SL:
            assert 2 * (M * cc + cc * _up64(M)) <= budget
        assert ws(M, 1024, V, 0) == ws(M, 1024, V, cc) == formula(M, 1024, V, cc)
    assert chunk(9216, 262144) == 3 * SL and chunk(1 << 20, 262144) == SL
    # it does not grow with M V: at a fixed chunk the table's height is gone from it
    assert ws(9216, 1024, 32768, 2 * SL) == ws(9216, 1024, 262144, 2 * SL) == ws(9216, 1024, 1 << 24, 2 * SL)
    for bad in ((0, 32, 16, SL), (-1, 32, 16, SL), (1, 0, 16, SL), (1, 32, 0, SL), (1, 32, -4, SL), (1, 32, 16, -SL),
                (1, 32, 16, SL + 1), (1, 32, 16, SL // 2), (1, 32, 16, BN), ((1 << 31) - 1, 32, 1 << 24, 1 << 24)):
        assert ws(*bad) < 0, bad
    assert chunk(0, 16) < 0 and chunk(4, 0) < 0


_GRAD_REFUSED = (
    [({p: None}, _BADARG) for p in ("x", "w", "targets", "lse", "d", "g", "gt")]
    + [({p: off}, _BADARG) for p in ("x", "w", "g", "gt") for off in (2, 4, 8, 24)]
    + [({"targets": off}, _BADARG) for off in (1, 2, 4, 12)] + [({p: off}, _BADARG) for p in ("lse", "d") for off in (1, 2, 3)]
    + [({"M": n}, _BADARG) for n in (0, -1)] + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, 260, 257)] + [({"ldx": 258, "x_dtype": _F32}, _BADARG)]
    + [({"w_dtype": t, "x_dtype": t}, _BADARG) for t in (_F32, 3, -1)] + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG)]
    + [({"v0": n}, _BADARG) for n in (-SL, -1, 1, BN, SL - 1)] + [({"Vc": n}, _BADARG) for n in (0, -1)]
    + [({"v0": 2 * SL, "Vc": 5000 - 2 * SL + 1}, _BADARG), ({"v0": 4 * SL, "Vc": 8}, _BADARG), ({"Vc": 5001, "ldg": 5056}, _BADARG)]
    + [({"ldg": n}, _BADARG) for n in (2047, 2048 + 32, 2048 + 8, 1024, 0, -64)]
    + [({"ldm": n}, _BADARG) for n in (199, 200, 192, 224, 0, -64)]
    # the geometry
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [({"V": 0}, _UNSUPPORTED), ({"V": -7}, _UNSUPPORTED)]
    # a bad argument is decided before the geometry
    + [(dict(bad, K=48, ldx=1024), _BADARG) for bad in ({"g": None}, {"lse": 2}, {"ldg": 100}, {"v0": 5}, {"d": None})]
)


def _grad_call(nv, bad):
    buf = ctypes.create_string_buffer(2048)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    a = dict(M=200, K=256, V=5000, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, targets=176, lse=184, d=188, v0=0, Vc=2048,
             g=32, ldg=2048, gt=64, ldm=256)
    a.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    return nv.lib().ea_vocab_nll_grad(a["M"], a["K"], a["V"], p(a["x"]), a["x_dtype"], a["ldx"], p(a["w"]), a["w_dtype"],
                                      p(a["targets"]), p(a["lse"]), p(a["d"]), a["v0"], a["Vc"], p(a["g"]), a["ldg"], p(a["gt"]),
                                      a["ldm"], None)


_GEMM_REFUSED = (
    [({p: None}, _BADARG) for p in ("a", "b", "out")] + [({p: off}, _BADARG) for p in ("a", "b") for off in (2, 4, 8, 24)]
    + [({"out": off}, _BADARG) for off in (1, 2, 3)] + [({"dtype": t}, _BADARG) for t in (_F32, 3, -1)]
    + [({n: v}, _BADARG) for n in ("M", "N", "K") for v in (0, -1)]
    + [({"lda": n}, _BADARG) for n in (255, 0, 260, 257)] + [({"ldb": n}, _BADARG) for n in (255, 0, 260, 257)]
    + [({"ldo": n}, _BADARG) for n in (99, 0, -100)] + [({"accumulate": n}, _BADARG) for n in (2, -1, 7)]
    + [({"K": n, "lda": 1024, "ldb": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [(dict(bad, K=48, lda=1024, ldb=1024), _BADARG) for bad in ({"out": None}, {"a": 8}, {"accumulate": 3}, {"ldo": 5})]
)


def _gemm_call(nv, bad):
    buf = ctypes.create_string_buffer(2048)
    base = (ctypes.addressof(buf) + 15) & ~15
    a = dict(M=200, N=100, K=256, a=0, lda=256, b=16, ldb=256, dtype=_BF16, out=36, ldo=100, accumulate=0)
    a.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    return nv.lib().ea_gemm_nt16(a["M"], a["N"], a["K"], p(a["a"]), a["lda"], p(a["b"]), a["ldb"], a["dtype"], p(a["out"]),
                                 a["ldo"], a["accumulate"], None)


def test_the_entries_refuse_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _grad_call(_native, bad)) for bad, want in _GRAD_REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 70 and not wrong, wrong
    got = [(bad, want, _gemm_call(_native, bad)) for bad, want in _GEMM_REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 40 and not wrong, wrong
    # what passes every check but the last one made (K % 32): fp32 rows, fp16, a ragged last chunk, a wider ldg
    for ok in ({}, {"x_dtype": _F32, "ldx": 1028}, {"w_dtype": _F16, "x_dtype": _F16}, {"v0": 2 * SL, "Vc": 5000 - 2 * SL},
               {"Vc": 8, "ldg": 64}, {"ldg": 4096}, {"ldm": 320}):
        assert _grad_call(_native, dict(ok, K=48, ldx=max(1024, ok.get("ldx", 0)))) == _UNSUPPORTED, ok
    for ok in ({}, {"accumulate": 1}, {"dtype": _F16}, {"ldo": 1 << 20}):
        assert _gemm_call(_native, dict(ok, K=48, lda=1024, ldb=1024)) == _UNSUPPORTED, ok


# ---- the interface --------------------------------------------------------------------------------------------------------------
def test_interface_of_loss_and_vocab_nll():
    from ea_harness import sequence as sq
    from ea_harness import vocab_loss as vl
    sig = inspect.signature(sq.DecoderStack.loss).parameters
    assert list(sig) == ["self", "tokens", "key_padding_mask", "reduction"]
    assert sig["key_padding_mask"].default is None and sig["reduction"].default == "mean"
    sig = inspect.signature(vl.vocab_nll).parameters
    assert list(sig) == ["rows", "weight", "targets", "chunk_cols"]
    assert sig["chunk_cols"].kind is inspect.Parameter.KEYWORD_ONLY and sig["chunk_cols"].default is None
    assert issubclass(vl._VocabNll, torch.autograd.Function)
    src = inspect.getsource(vl)
    assert ".item()" not in src.replace("`.item()`", "") and "synchronize" not in src and ".cpu()" not in src


def test_loss_argument_errors_and_the_adaptive_stack_raises():
    from ea_harness.sequence import DecoderStack
    stack = DecoderStack(50, 128, 256, 2, 2, ATTN)
    with pytest.raises(ValueError, match="reduction"):
        stack.loss(torch.zeros(3, 4, dtype=torch.long), reduction="average")
    with pytest.raises(ValueError, match="at least two tokens"):
        stack.loss(torch.zeros(3, 1, dtype=torch.long))
    adaptive = DecoderStack(333, 128, 256, 2, 1, ATTN, adaptive=dict(cutoff=[96, 200], factor=2))
    assert adaptive.is_adaptive
    with pytest.raises(NotImplementedError, match="adaptive-softmax training loss is a follow-up"):
        adaptive.loss(torch.zeros(3, 4, dtype=torch.long))


def test_vocab_nll_argument_errors_and_no_fall_back():
    from ea_harness.vocab_loss import vocab_nll
    rows = torch.zeros(2, 3, 128, requires_grad=True)
    w = torch.zeros(50, 128, requires_grad=True)
    tg = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="table"):
        vocab_nll(rows, torch.zeros(50, 128, dtype=torch.float64), tg)
    with pytest.raises(ValueError, match="channels"):
        vocab_nll(torch.zeros(2, 3, 64), w, tg)
    with pytest.raises(ValueError, match="targets"):
        vocab_nll(rows, w, None)
    with pytest.raises(ValueError, match="targets"):
        vocab_nll(rows, w, tg.int())
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):          # a missing device is an error, never a fall-back
        vocab_nll(rows, w, tg)


# ---- the host reference ---------------------------------------------------------------------------------------------------------
def test_reference_on_hand_computed_values():
    a = np.log(np.array([[1.0, 2.0, 5.0], [4.0, 2.0, 2.0]]))
    lse = np.log(np.array([8.0, 8.0]))
    g = ref.grad(a, lse, [2.0, -1.0], [2, 0])
    want = np.array([[-0.25, -0.5, 2.0 * (1 - 0.625)], [-(1 - 0.5), 0.25, 0.25]])
    assert np.abs(g - want).max() < 1e-15
    assert abs(g[0].sum()) < 1e-15 and abs(g[1].sum()) < 1e-15           # a row of d (onehot - softmax) sums to 0
    # a chunk: the columns are v0 + c
    assert np.array_equal(ref.grad(a[:, 1:], lse, [2.0, -1.0], [2, 0], v0=1), g[:, 1:])
    # a target outside [0, V): no onehot term; d == 0: zeros, whatever the row holds
    out = ref.grad(a, lse, [2.0, -1.0], [3, -1], V=3)
    assert np.abs(out - np.array([[-0.25, -0.5, -1.25], [0.5, 0.25, 0.25]])).max() < 1e-15
    nan = np.full((1, 3), np.nan)
    assert np.array_equal(ref.grad(nan, [np.nan], [0.0], [1]), np.zeros((1, 3)))
    assert np.array_equal(ref.bound(nan, [np.nan], [0.0], [1], torch.bfloat16), np.zeros((1, 3)))


def test_the_bound_is_the_written_count():
    u = 2.0 ** -24
    a, lse, d, t = np.array([[0.5, -3.0, 2.0]]), [2.25], [-1.5], [2]
    for dtype, uE, fl in ((torch.bfloat16, 2.0 ** -8, 2.0 ** -134), (torch.float16, 2.0 ** -11, 2.0 ** -25)):
        assert ref.unit(dtype) == uE and ref.floor(dtype) == fl
        got = ref.bound(a, lse, d, t, dtype)
        for c in range(3):
            diff = a[0, c] - 2.25
            p, h = math.exp(diff), float(c == 2)
            e32 = 1.5 * (p * (abs(diff) + 2) + 2 * abs(h - p)) * u * (1 + 2.0 ** -10)
            want = e32 + uE * (1.5 * abs(h - p) + e32) + fl + 2.5 * 2.0 ** -126
            assert abs(got[0, c] - want) <= 1e-12 * want
        # dominated by the one rounding to E
        g = np.abs(ref.grad(a, lse, d, t))
        assert (got < 1.01 * uE * g + 2.0 ** -24).all() and (got > uE * g).all()
