"""-m "not gpu": the adaptive-softmax training loss (ea_vocab_nll_grad_rows, ea_gemm_nt16_rows, ea_rows_transpose16,
ea_adaptive_score_masked, ea_adaptive_nll_ws -- additions to C ABI 38 -- ea_harness.adaptive_loss.adaptive_nll and
DecoderStack.adaptive_loss): the header, the binding, the workspace formula, what the entries refuse before any launch (no
pointer is dereferenced), the interfaces, and the host reference (tests/adaptive_loss_reference.py) on hand-computed values
and against fp64 autograd of the framework route."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import adaptive_loss_reference as ref
import vocab_score_reference as sref

ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
BM, BN, SL = sref.constants()
_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_GRAD_ARGS = ["int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
              "int32_t w_dtype", "const int64_t* targets", "const float* lse", "const float* d", "int32_t v0", "int32_t Vc",
              "void* g", "int64_t ldg", "void* gt", "int64_t ldm", "const int32_t* trows", "const int32_t* count",
              "int64_t target_base", "void* stream"]
_GEMM_ARGS = ["int32_t M", "int32_t N", "int32_t K", "const void* a", "int64_t lda", "const void* b", "int64_t ldb",
              "int32_t dtype", "float* out", "int64_t ldo", "int32_t accumulate", "const int32_t* orows", "const int32_t* count",
              "void* stream"]
_TRANSPOSE_ARGS = ["int32_t M", "int32_t K", "const void* src", "int32_t src_dtype", "int64_t ld", "const int32_t* rows",
                   "const int32_t* count", "void* out", "int32_t out_dtype", "int64_t ldm", "void* stream"]
_MASKED_ARGS = ["int32_t M", "int32_t C", "int32_t n_tails", "const int64_t* cutoffs", "const int32_t* dims", "const void* x",
                "int32_t x_dtype", "int64_t ldx", "const int64_t* targets", "const void* head", "int32_t w_dtype",
                "const void* const* proj", "const void* const* tables", "const void* const* hmask", "void* ws", "int64_t ws_bytes",
                "float* logp", "int64_t* token_head", "void* stream"]
_WS_ARGS = ["int32_t M", "int32_t C", "int32_t n_tails", "const int64_t* cutoffs", "const int32_t* dims", "int32_t chunk_cols"]


def _up64(n):
    return (n + 63) // 64 * 64


# ---- the C ABI: additions to 38 -------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree_and_the_abi_is_still_38(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION == 38
    doc = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)

    def declared(ret, name):
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (ret, name), text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("int64_t", "ea_adaptive_nll_ws") == _WS_ARGS
    assert declared("int", "ea_vocab_nll_grad_rows") == _GRAD_ARGS
    assert declared("int", "ea_gemm_nt16_rows") == _GEMM_ARGS
    assert declared("int", "ea_rows_transpose16") == _TRANSPOSE_ARGS
    assert declared("int", "ea_adaptive_score_masked") == _MASKED_ARGS
    # the masked score is the score with one more host array; the row-set entries are their plain ones with a tail of lists
    plain = declared("int", "ea_adaptive_score")
    assert [a for a in _MASKED_ARGS if a != "const void* const* hmask"] == plain
    assert _GRAD_ARGS[:17] + ["void* stream"] == declared("int", "ea_vocab_nll_grad")
    assert _GEMM_ARGS[:11] + ["void* stream"] == declared("int", "ea_gemm_nt16")
    I, L, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    S = _native.SIGNATURES
    code = {"int32_t": I, "int64_t": L}
    for name, args in (("ea_adaptive_nll_ws", _WS_ARGS), ("ea_vocab_nll_grad_rows", _GRAD_ARGS), ("ea_gemm_nt16_rows", _GEMM_ARGS),
                       ("ea_rows_transpose16", _TRANSPOSE_ARGS), ("ea_adaptive_score_masked", _MASKED_ARGS)):
        assert S[name] == [code.get(a.rsplit(" ", 1)[0], P) for a in args], name
    assert _native.lib().ea_adaptive_nll_ws.restype is ctypes.c_int64
    assert set(S) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]
    assert "ADDITIONS TO ABI 38" in doc and "the ABI number stays 38" in doc


def _host(nv, cutoffs, dims):
    return nv.host_array(ctypes.c_int64, cutoffs), nv.host_array(ctypes.c_int32, dims)


def test_the_workspace_is_its_documented_formula(lib):  # noqa: F811
    from efficient_attention import _native as nv
    ws, pass_ws = nv.lib().ea_adaptive_nll_ws, nv.lib().ea_vocab_nll_ws

    def query(M, C, cutoffs, dims, cc):
        return ws(M, C, len(dims), *_host(nv, cutoffs, dims), cc)

    def formula(M, C, cutoffs, dims, cc):
        n, ldm = len(dims), _up64(M)
        passes = [pass_ws(M, C, cutoffs[0] + n, cc)] + [pass_ws(M, d, cutoffs[i + 1] - cutoffs[i], cc) for i, d in enumerate(dims)]
        assert min(passes) > 0
        return max(passes) + 2 * C * ldm + max(6 * M * d + 2 * d * ldm + 2 * C * d for d in dims)
    cases = [(1, 128, [96, 200, 333], [64, 32], SL), (BM + 1, 128, [96, 200, 333], [64, 32], 0),
             (2 * BM + 3, 128, [96, 200, 200 + SL + 8], [64, 32], SL), (9216, 1024, [20000, 60000, 267744], [256, 64], 0),
             (9216, 1024, [20000, 60000, 267744], [256, 64], 2 * SL), (2048, 256, [1000, 3000, 63000], [64, 32], SL),
             (7, 96, [5, 6, 7, 8, 5000], [32, 64, 96, 32], 4 * SL)]
    for M, C, cutoffs, dims, cc in cases:
        assert query(M, C, cutoffs, dims, cc) == formula(M, C, cutoffs, dims, cc), (M, C, cutoffs, dims, cc)
    # it does not grow with M V: at a fixed chunk the last tail's height is gone from it
    a = query(9216, 1024, [20000, 60000, 267744], [256, 64], SL)
    assert a == query(9216, 1024, [20000, 60000, 1 << 24], [256, 64], SL)
    assert a < 2 * 9216 * (267744 - 60000)
    for bad in ((0, 128, [96, 200, 333], [64, 32], SL), (4, 0, [96, 200, 333], [64, 32], SL), (4, 128, [96, 96, 333], [64, 32], SL),
                (4, 128, [0, 200, 333], [64, 32], SL), (4, 128, [96, 200, 333], [64, 0], SL), (4, 128, [96, 200, 333], [64, 32], SL + 1),
                (4, 128, [96, 200, 333], [64, 32], -SL), (4, 128, [96, 200, 1 << 31], [64, 32], SL),
                (4, 128, [1, 2, 3, 4, 5, 6], [32] * 5, SL)):
        assert query(*bad) < 0, bad
    assert ws(4, 128, 2, None, None, SL) < 0


def _ptr(base, off):
    return None if off is None else ctypes.c_void_p(base + off)


def _base():
    buf = ctypes.create_string_buffer(4096)
    return buf, (ctypes.addressof(buf) + 15) & ~15       # never dereferenced: a refused call returns before any HIP call


_GRAD_REFUSED = (
    [({p: None}, _BADARG) for p in ("x", "w", "targets", "lse", "d", "g", "gt")]
    + [({p: off}, _BADARG) for p in ("x", "w", "g", "gt") for off in (2, 4, 8, 24)]
    + [({"targets": off}, _BADARG) for off in (1, 2, 4, 12)] + [({p: off}, _BADARG) for p in ("lse", "d") for off in (1, 2, 3)]
    + [({p: off}, _BADARG) for p in ("trows", "count") for off in (1, 2, 3, 6)]
    + [({"target_base": n}, _BADARG) for n in (-1, -(1 << 40))]
    + [({"M": n}, _BADARG) for n in (0, -1)] + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, 260, 257)] + [({"ldx": 258, "x_dtype": _F32}, _BADARG)]
    + [({"w_dtype": t, "x_dtype": t}, _BADARG) for t in (_F32, 3, -1)] + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG)]
    + [({"v0": n}, _BADARG) for n in (-SL, -1, 1, BN, SL - 1)] + [({"Vc": n}, _BADARG) for n in (0, -1)]
    + [({"v0": 2 * SL, "Vc": 5000 - 2 * SL + 1}, _BADARG), ({"v0": 4 * SL, "Vc": 8}, _BADARG), ({"Vc": 5001, "ldg": 5056}, _BADARG)]
    + [({"ldg": n}, _BADARG) for n in (2047, 2048 + 32, 2048 + 8, 1024, 0, -64)]
    + [({"ldm": n}, _BADARG) for n in (199, 200, 192, 224, 0, -64)]
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [({"V": 0}, _UNSUPPORTED), ({"V": -7}, _UNSUPPORTED)]
    + [(dict(bad, K=48, ldx=1024), _BADARG) for bad in ({"g": None}, {"count": 2}, {"trows": 1}, {"target_base": -5}, {"ldg": 100})]
)


def _grad_call(nv, bad):
    buf, base = _base()
    a = dict(M=200, K=256, V=5000, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, targets=176, lse=184, d=188, v0=0, Vc=2048,
             g=32, ldg=2048, gt=64, ldm=256, trows=192, count=196, target_base=20000)
    a.update(bad)
    return nv.lib().ea_vocab_nll_grad_rows(a["M"], a["K"], a["V"], _ptr(base, a["x"]), a["x_dtype"], a["ldx"], _ptr(base, a["w"]),
                                           a["w_dtype"], _ptr(base, a["targets"]), _ptr(base, a["lse"]), _ptr(base, a["d"]), a["v0"],
                                           a["Vc"], _ptr(base, a["g"]), a["ldg"], _ptr(base, a["gt"]), a["ldm"],
                                           _ptr(base, a["trows"]), _ptr(base, a["count"]), a["target_base"], None)


_GEMM_REFUSED = (
    [({p: None}, _BADARG) for p in ("a", "b", "out")] + [({p: off}, _BADARG) for p in ("a", "b") for off in (2, 4, 8, 24)]
    + [({p: off}, _BADARG) for p in ("out", "orows", "count") for off in (1, 2, 3)] + [({"dtype": t}, _BADARG) for t in (_F32, 3, -1)]
    + [({n: v}, _BADARG) for n in ("M", "N", "K") for v in (0, -1)]
    + [({"lda": n}, _BADARG) for n in (255, 0, 260, 257)] + [({"ldb": n}, _BADARG) for n in (255, 0, 260, 257)]
    + [({"ldo": n}, _BADARG) for n in (99, 0, -100)] + [({"accumulate": n}, _BADARG) for n in (2, -1, 7)]
    + [({"K": n, "lda": 1024, "ldb": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [(dict(bad, K=48, lda=1024, ldb=1024), _BADARG) for bad in ({"out": None}, {"orows": 2}, {"count": 1}, {"ldo": 5})]
)


def _gemm_call(nv, bad):
    buf, base = _base()
    a = dict(M=200, N=100, K=256, a=0, lda=256, b=16, ldb=256, dtype=_BF16, out=36, ldo=100, accumulate=1, orows=40, count=44)
    a.update(bad)
    return nv.lib().ea_gemm_nt16_rows(a["M"], a["N"], a["K"], _ptr(base, a["a"]), a["lda"], _ptr(base, a["b"]), a["ldb"], a["dtype"],
                                      _ptr(base, a["out"]), a["ldo"], a["accumulate"], _ptr(base, a["orows"]),
                                      _ptr(base, a["count"]), None)


_TRANSPOSE_REFUSED = (
    [({p: None}, _BADARG) for p in ("src", "out")] + [({p: off}, _BADARG) for p in ("src", "rows", "count") for off in (1, 2, 3)]
    + [({"out": off}, _BADARG) for off in (1, 3)] + [({"out_dtype": t, "src_dtype": t}, _BADARG) for t in (_F32, 3, -1)]
    + [({"src_dtype": t}, _BADARG) for t in (_F16, 3, -1)] + [({n: v}, _BADARG) for n in ("M", "K") for v in (0, -1)]
    + [({"ld": n}, _BADARG) for n in (255, 0, -256)] + [({"ldm": n}, _BADARG) for n in (199, 192, 200, 224, 0, -64)]
    + [({"K": 64 * 65535 + 1, "ld": 1 << 23}, _UNSUPPORTED)]
    + [({"K": 64 * 65535 + 1, "ld": 1 << 23, "out": None}, _BADARG), ({"K": 64 * 65535 + 1, "ld": 1 << 23, "ldm": 100}, _BADARG)]
)


def _transpose_call(nv, bad):
    buf, base = _base()
    a = dict(M=200, K=256, src=0, src_dtype=_BF16, ld=256, rows=16, count=20, out=34, out_dtype=_BF16, ldm=256)
    a.update(bad)
    return nv.lib().ea_rows_transpose16(a["M"], a["K"], _ptr(base, a["src"]), a["src_dtype"], a["ld"], _ptr(base, a["rows"]),
                                        _ptr(base, a["count"]), _ptr(base, a["out"]), a["out_dtype"], a["ldm"], None)


def _masked_call(nv, bad):
    buf, base = _base()
    a = dict(M=50, C=128, cutoffs=[96, 200, 333], dims=[64, 32], x=0, x_dtype=_BF16, ldx=128, targets=16, head=32, w_dtype=_BF16,
             proj=[48, 64], tables=[80, 96], hmask=[112, None], ws=128, ws_bytes=1 << 40, logp=144, token_head=None)
    a.update(bad)

    def arr(offs):
        return None if offs is None else nv.host_array(ctypes.c_void_p, [None if o is None else base + o for o in offs])
    cut = None if a["cutoffs"] is None else nv.host_array(ctypes.c_int64, a["cutoffs"])
    dims = None if a["dims"] is None else nv.host_array(ctypes.c_int32, a["dims"])
    return nv.lib().ea_adaptive_score_masked(a["M"], a["C"], len(a["dims"] or [0, 0]), cut, dims, _ptr(base, a["x"]), a["x_dtype"],
                                             a["ldx"], _ptr(base, a["targets"]), _ptr(base, a["head"]), a["w_dtype"], arr(a["proj"]),
                                             arr(a["tables"]), arr(a["hmask"]), _ptr(base, a["ws"]), a["ws_bytes"],
                                             _ptr(base, a["logp"]), _ptr(base, a["token_head"]), None)


_MASKED_REFUSED = (
    [({p: None}, _BADARG) for p in ("hmask", "cutoffs", "dims", "proj", "tables", "x", "targets", "head", "ws", "logp")]
    + [({"hmask": [off, None]}, _BADARG) for off in (2, 4, 8, 24)] + [({"hmask": [None, off]}, _BADARG) for off in (2, 8)]
    + [({"proj": [48, None]}, _BADARG), ({"tables": [80, 98]}, _BADARG), ({"ws_bytes": 64}, _BADARG), ({"M": 0}, _BADARG)]
    + [({"cutoffs": [96, 96, 333]}, _BADARG), ({"w_dtype": _F32}, _BADARG), ({"ldx": 120}, _BADARG), ({"dims": [64, 0]}, _BADARG)]
    + [({"C": 48, "ldx": 128}, _UNSUPPORTED), ({"dims": [64, 48]}, _UNSUPPORTED)]
    + [({"C": 48, "ldx": 128, "hmask": [2, None]}, _BADARG), ({"C": 48, "ldx": 128, "hmask": None}, _BADARG)]
)


def test_every_new_entry_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    for call, table, least in ((_grad_call, _GRAD_REFUSED, 80), (_gemm_call, _GEMM_REFUSED, 45),
                               (_transpose_call, _TRANSPOSE_REFUSED, 30), (_masked_call, _MASKED_REFUSED, 25)):
        got = [(bad, want, call(_native, bad)) for bad, want in table]
        wrong = [row for row in got if row[1] != row[2]]
        assert len(got) >= least and not wrong, (call.__name__, len(got), wrong)
    # what passes every check but the last one made (K % 32, C % 32): NULL lists, fp32 rows, fp16, a ragged last chunk
    for ok in ({}, {"trows": None}, {"count": None}, {"trows": None, "count": None, "target_base": 0}, {"x_dtype": _F32, "ldx": 1028},
               {"w_dtype": _F16, "x_dtype": _F16}, {"v0": 2 * SL, "Vc": 5000 - 2 * SL}, {"Vc": 8, "ldg": 64}, {"ldm": 320}):
        assert _grad_call(_native, dict(ok, K=48, ldx=max(1024, ok.get("ldx", 0)))) == _UNSUPPORTED, ok
    for ok in ({}, {"accumulate": 0}, {"dtype": _F16}, {"orows": None}, {"count": None}, {"orows": None, "count": None}):
        assert _gemm_call(_native, dict(ok, K=48, lda=1024, ldb=1024)) == _UNSUPPORTED, ok
    for ok in ({}, {"rows": None}, {"count": None}, {"src_dtype": _F32}, {"src_dtype": _F16, "out_dtype": _F16}, {"ldm": 320}):
        assert _transpose_call(_native, dict(ok, K=64 * 65535 + 1, ld=1 << 23)) == _UNSUPPORTED, ok
    for ok in ({}, {"hmask": [None, None]}, {"hmask": [112, 160]}, {"x_dtype": _F32, "ldx": 128}):
        assert _masked_call(_native, dict(ok, C=48)) == _UNSUPPORTED, ok


# ---- the interfaces -------------------------------------------------------------------------------------------------------------
def test_interface_of_adaptive_loss_and_adaptive_nll():
    from ea_harness import sequence as sq
    from ea_harness import adaptive_loss as al
    sig = inspect.signature(sq.DecoderStack.adaptive_loss).parameters
    assert list(sig) == ["self", "tokens", "key_padding_mask", "reduction"]
    assert sig["key_padding_mask"].default is None and sig["reduction"].default == "mean"
    sig = inspect.signature(al.adaptive_nll).parameters
    assert list(sig) == ["rows", "softmax", "targets", "chunk_cols", "tail_masks"]
    for name in ("chunk_cols", "tail_masks"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None
    assert issubclass(al._AdaptiveNll, torch.autograd.Function)
    src = inspect.getsource(al)
    for banned in (".item()", ".cpu()", "nonzero", "synchronize"):
        assert banned not in src, banned
    src = inspect.getsource(sq.DecoderStack.adaptive_loss)
    for banned in (".item()", ".cpu()", "nonzero", "synchronize"):
        assert banned not in src, banned


def test_the_workspace_plan_is_the_headers_layout(lib):  # noqa: F811
    from efficient_attention import _native as nv
    from ea_harness.adaptive_loss import workspace_plan
    r16 = lambda n: (n + 15) // 16 * 16                                              # noqa: E731
    for M, cutoffs, dims in ((1, [96, 200, 333], [64, 32]), (131, [96, 200, 333], [64, 32]), (9216, [20000, 60000, 267744], [256, 64]),
                             (7, [5, 6, 7, 8, 5000], [32, 64, 96, 32])):
        plan, n = workspace_plan(M, dims), len(dims)
        assert plan["head_target"] == 0 and plan["rows"] == r16(8 * M) and plan["count"] == plan["rows"] + r16(4 * n * M)
        assert plan["lse_head"] == plan["count"] + 16 + r16(8 * M)
        at = plan["lse_head"] + 2 * r16(4 * M)
        for i, d in enumerate(dims):
            assert plan["h"][i] == at and plan["lse"][i] == at + r16(2 * M * d) + r16(8 * M)
            at = plan["lse"][i] + 2 * r16(4 * M)
        assert plan["end"] == at
        inner = max([nv.lib().ea_vocab_score_ws(M, cutoffs[0] + n)]
                    + [max(nv.lib().ea_vocab_score_ws(M, d), nv.lib().ea_vocab_score_ws(M, cutoffs[i + 1] - cutoffs[i]))
                       for i, d in enumerate(dims)])
        assert nv.lib().ea_adaptive_score_ws(M, n, *_host(nv, cutoffs, dims)) == at + inner


def test_loss_points_to_adaptive_loss_and_adaptive_loss_wants_an_adaptive_stack():
    from ea_harness.sequence import DecoderStack
    adaptive = DecoderStack(333, 128, 256, 2, 1, ATTN, adaptive=dict(cutoff=[96, 200], factor=2))
    assert adaptive.is_adaptive and adaptive.adaptive_softmax.band_dims() == [64, 32]
    with pytest.raises(NotImplementedError, match="adaptive-softmax training loss is a follow-up") as info:
        adaptive.loss(torch.zeros(3, 4, dtype=torch.long))
    assert "adaptive_loss" in str(info.value)
    with pytest.raises(ValueError, match="reduction"):
        adaptive.adaptive_loss(torch.zeros(3, 4, dtype=torch.long), reduction="average")
    with pytest.raises(ValueError, match="at least two tokens"):
        adaptive.adaptive_loss(torch.zeros(3, 1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):          # a missing device is an error, never a fall-back
        adaptive.adaptive_loss(torch.zeros(3, 4, dtype=torch.long))
    plain = DecoderStack(50, 128, 256, 2, 1, ATTN)
    with pytest.raises(RuntimeError, match="adaptive=dict"):
        plain.adaptive_loss(torch.zeros(3, 4, dtype=torch.long))


def test_adaptive_nll_argument_errors_and_no_fall_back():
    from ea_harness.adaptive import AdaptiveInput, AdaptiveSoftmax
    from ea_harness.adaptive_loss import adaptive_nll
    inp = AdaptiveInput(333, 1, 128, 2, 128, [96, 200, 333])
    sm = AdaptiveSoftmax(333, 128, [96, 200], 0.0, factor=2, adaptive_inputs=inp, tie_proj=True)
    rows = torch.zeros(2, 3, 128, requires_grad=True)
    tg = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="AdaptiveSoftmax"):
        adaptive_nll(rows, torch.zeros(333, 128), tg)
    with pytest.raises(ValueError, match="channels"):
        adaptive_nll(torch.zeros(2, 3, 64), sm, tg)
    with pytest.raises(ValueError, match="targets"):
        adaptive_nll(rows, sm, None)
    with pytest.raises(ValueError, match="targets"):
        adaptive_nll(rows, sm, tg.int())
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        adaptive_nll(rows, sm, tg)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):          # (an untied softmax with a head of its own too)
        adaptive_nll(rows, AdaptiveSoftmax(333, 128, [96, 200], 0.0, factor=2), tg)


# ---- the host reference ---------------------------------------------------------------------------------------------------------
def test_reference_on_hand_computed_values():
    # C = 1, x = 1: the head's logits are its table; c0 = 2 and one tail of 2 tokens at width 1 with Q = 1, so h = x = 1
    ln = math.log
    head = np.array([[ln(1.0)], [ln(2.0)], [ln(5.0)]])                  # softmax (1, 2, 5) / 8; column 2 is the tail's class
    tab = np.array([[ln(1.0)], [ln(3.0)]])                               # softmax (1, 3) / 4
    x = np.ones((3, 1))
    cutoff, tg, d = [2, 4], [1, 3, 7], [2.0, -1.0, 0.0]
    f = ref.forward(x, head, [np.ones((1, 1))], [tab], cutoff, tg)
    assert list(f["head_target"]) == [1, 2, -1] and [list(r) for r in f["rows"]] == [[1]]
    assert abs(f["logp"][0] - ln(2.0 / 8)) < 1e-15 and abs(f["logp"][1] - ln(5.0 / 8 * 3.0 / 4)) < 1e-15 and np.isnan(f["logp"][2])
    out = ref.grads(x, head, [np.ones((1, 1))], [tab], cutoff, tg, d)
    gh = np.array([[-0.25, 2 * 0.75, -1.25], [0.125, 0.25, -0.375], [0.0, 0.0, 0.0]])
    gt = np.array([[0.25, -0.25]])                                       # -1 ((u == 1) - (1, 3) / 4)
    assert np.abs(out["dhead"] - gh.sum(0).reshape(3, 1)).max() < 1e-15
    assert np.abs(out["dtab"][0] - gt.T).max() < 1e-15
    dh = (gt @ tab).item()                                               # -ln(3) / 4
    assert abs(dh + ln(3.0) / 4) < 1e-15 and abs(out["dproj"][0].item() - dh) < 1e-15
    want_dx = gh @ head
    want_dx[1] += dh
    assert np.abs(out["dx"] - want_dx).max() < 1e-15
    # a mask scales h and dh alike
    out2 = ref.grads(x, head, [np.ones((1, 1))], [tab], cutoff, tg, d, masks=[np.array([[1.25]])])
    assert abs(out2["forward"]["h"][0].item() - 1.25) < 1e-15
    p = np.exp(1.25 * tab[:, 0]) / np.exp(1.25 * tab[:, 0]).sum()
    g2 = -1.0 * (np.array([0.0, 1.0]) - p)
    assert np.abs(out2["dtab"][0][:, 0] - 1.25 * g2).max() < 1e-15 and abs(out2["dproj"][0].item() - 1.25 * (g2 @ tab[:, 0])) < 1e-15


def test_reference_against_fp64_autograd_of_the_framework_route():
    from ea_harness.adaptive import AdaptiveInput, AdaptiveSoftmax
    torch.manual_seed(3)
    inp = AdaptiveInput(333, 1, 128, 2, 128, [96, 200, 333]).double()
    sm = AdaptiveSoftmax(333, 128, [96, 200], 0.0, factor=2, adaptive_inputs=inp, tie_proj=True).double()
    M = 37
    x = torch.randn(M, 128, dtype=torch.float64, requires_grad=True)
    tg = torch.randint(0, 333, (M,))
    tg[:4] = torch.tensor([0, 95, 96, 332])
    d = torch.randn(M, dtype=torch.float64)
    logp = sm.get_log_prob(x, tg)
    logp.backward(d)
    num = lambda t: t.detach().numpy()                                               # noqa: E731
    projs = [num(sm.tail_projection(i)) for i in range(2)]
    tabs = [num(sm.tail_table(i)) for i in range(2)]
    out = ref.grads(num(x), num(sm.head_table()), projs, tabs, sm.cutoff, num(tg), num(d))
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())    # noqa: E731
    assert close(out["forward"]["logp"], num(logp)) and close(out["dx"], num(x.grad))
    assert close(out["dhead"][96:], num(sm.head.class_proj.weight.grad))
    assert close(out["dhead"][:96], num(sm.head.word_proj.weight.grad))
    for i in range(2):
        assert close(out["dtab"][i], num(sm.tail[i][2].weight.grad))
        assert close(out["dproj"][i].T, num(sm.tail[i][0].weight.grad))               # (tied: stored [C, d_i])
