"""-m "not gpu": the many-row vocabulary pass (ea_vocab_score, C ABI 30) and DecoderStack.rows_logprobs / evaluate: the header,
the binding, the workspace query, what the entry point refuses before any launch (no pointer is dereferenced), the interface,
and the host reference (tests/vocab_score_reference.py) against hand-computed rows."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import vocab_score_reference as ref

ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
WS, TILE, SCORE = "ea_vocab_score_ws", "ea_vocab_score_tile", "ea_vocab_score"
_ARGS = ["int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
         "int32_t w_dtype", "const int64_t* targets", "void* logits", "int32_t logits_dtype", "int64_t ldl", "void* ws",
         "int64_t ws_bytes", "int64_t* token", "float* top", "float* lse", "float* logp", "void* stream"]


# ---- C ABI 30 -------------------------------------------------------------------------------------------------------------------
def test_abi_30_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 30
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def declared(ret, name):
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (ret, name), text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("int64_t", WS) == ["int32_t M", "int32_t V"]
    assert declared("int32_t", TILE) == ["int32_t which"]
    assert declared("int", SCORE) == _ARGS
    I, L, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _native.SIGNATURES[WS] == [I, I] and _native.SIGNATURES[TILE] == [I]
    assert _native.SIGNATURES[SCORE] == [I, I, I, P, I, L, P, I, P, P, I, L, P, L, P, P, P, P, P]
    assert len(_native.SIGNATURES[SCORE]) == len(_ARGS)
    assert _native.lib().ea_vocab_score_ws.restype is ctypes.c_int64
    assert all(hasattr(lib, s) for s in (WS, TILE, SCORE))
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]
    doc = open(HEADER).read()
    assert "ABI 30" in doc and "need NOT have the bits" in doc and "skipped, never multiplied" in doc


def test_the_tile_constants_are_the_headers(lib):  # noqa: F811
    from efficient_attention import _native
    BM, BN, SL = _native.vocab_score_tiles()
    assert (BM, BN, SL) == ref.constants()
    assert BM % 16 == 0 and BN % 16 == 0 and SL % BN == 0 and BM > 64
    assert [_native.lib().ea_vocab_score_tile(i) for i in (-1, 3, 99)] == [-1, -1, -1]


def test_the_workspace_query(lib):  # noqa: F811
    from efficient_attention import _native
    ws = _native.lib().ea_vocab_score_ws
    BM, BN, SL = ref.constants()
    for M, V in ((1, 1), (65, 16), (BM + 1, 40), (3, 2 * SL + 1000), (9216, 32768), (9216, 262144), (7, 7)):
        NS = -(-V // SL)
        assert ws(M, V) == (12 * M * NS + 4 * M + 15) // 16 * 16, (M, V)
    for M, V in ((0, 16), (-1, 16), (1, 0), (1, -5), (-3, -3), ((1 << 31) - 1, 1), (1 << 30, SL + 1), (BM * 4096 + 1, SL * 2048)):
        assert ws(M, V) < 0, (M, V)
    # grows with M and with V
    sizes_m = [ws(M, 5000) for M in (1, 2, 64, 65, BM, BM + 1, 9216, 100000)]
    sizes_v = [ws(100, V) for V in (1, SL + 1, 2 * SL + 1, 32768, 262144, 1 << 24)]        # (with V: by whole slices)
    assert all(a < b for a, b in zip(sizes_m, sizes_m[1:])), sizes_m
    assert all(a < b for a, b in zip(sizes_v, sizes_v[1:])), sizes_v
    assert ws(100, 1) == ws(100, SL) < ws(100, SL + 1) == ws(100, 2 * SL)
    assert ws(BM * 4096, SL * 2048) > 0                  # the largest grid: 2^23 workgroups


_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_WS_200_5000 = (12 * 200 * 3 + 4 * 200 + 15) // 16 * 16
_BIG = (1 << 31) - 1

_REFUSED = (
    [({p: None}, _BADARG) for p in ("x", "w", "ws", "token", "lse", "logp")]                         # null
    + [({p: off}, _BADARG) for p in ("x", "w", "ws") for off in (2, 4, 8, 24)]                     # not 16-byte aligned
    + [({"token": off}, _BADARG) for off in (2, 4, 12)] + [({"targets": off}, _BADARG) for off in (1, 2, 4, 12)]
    + [({p: off}, _BADARG) for p in ("top", "lse", "logp") for off in (1, 2, 3)]
    + [({"logits": 33, "logits_dtype": _BF16}, _BADARG), ({"logits": 34, "logits_dtype": _F32}, _BADARG)]
    + [({"logits_dtype": t}, _BADARG) for t in (_F16, 3, -1)]
    + [({"M": n}, _BADARG) for n in (0, -1, -64)]
    + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, -256)] + [({"ldl": n}, _BADARG) for n in (4999, 0, -5000)]
    + [({"ldx": 260}, _BADARG), ({"ldx": 257}, _BADARG), ({"ldx": 258, "x_dtype": _F32}, _BADARG)]   # row stride % 16 bytes
    + [({"ws_bytes": n}, _BADARG) for n in (_WS_200_5000 - 1, 8, 0, -1)]
    + [({"w_dtype": t, "x_dtype": t}, _BADARG) for t in (_F32, 3, -1)] + [({"x_dtype": 3}, _BADARG)]
    + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _BF16}, _BADARG)]
    # the geometry
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [({"V": 0, "ldl": 5000}, _UNSUPPORTED), ({"V": -7, "ldl": 5000}, _UNSUPPORTED)]
    + [({"M": _BIG, "ws_bytes": 1 << 50}, _UNSUPPORTED), ({"M": 1 << 30, "ws_bytes": 1 << 50}, _UNSUPPORTED)]
    + [({"M": _BIG, "ws_bytes": 0}, _UNSUPPORTED)]      # (no workspace size to hold it against: the geometry answers)
    # where two faults meet: a bad argument is decided before the geometry
    + [(dict(bad, K=48, ldx=1024), _BADARG) for bad in ({"ws": None}, {"lse": None}, {"logp": None}, {"ws": 8}, {"lse": 2},
                                                        {"token": None}, {"targets": 4}, {"ws_bytes": 0}, {"top": 1},
                                                        {"logits_dtype": 3}, {"x_dtype": 3})]
    + [(dict(bad, M=_BIG), _BADARG) for bad in ({"x": None}, {"logp": 3}, {"ldx": 255})]
    + [({"V": 0, "ldl": -1}, _BADARG), ({"V": 0, "ws": None}, _BADARG)]
    # and among bad arguments the table operands come first: all of these are EA_E_BADARG either way, pinned as such
    + [({"x": None, "ws_bytes": 0}, _BADARG), ({"M": 0, "K": 48}, _BADARG)]
)
# null optional arguments get past every check but the last one made here (K % 32)
_PASSED = [{}, {"logits": None}, {"top": None}, {"targets": None}, {"logits": None, "logits_dtype": 7, "ldl": 0},
           {"ws_bytes": 1 << 40}, {"x_dtype": _F32, "ldx": 1028}, {"w_dtype": _F16, "x_dtype": _F16, "logits_dtype": _F16}]


def _call(nv, bad):
    buf = ctypes.create_string_buffer(2048)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    a = dict(M=200, K=256, V=5000, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, targets=176, logits=32, logits_dtype=_F32,
             ldl=5000, ws=64, ws_bytes=_WS_200_5000, token=112, top=140, lse=184, logp=188)
    a.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    return nv.lib().ea_vocab_score(a["M"], a["K"], a["V"], p(a["x"]), a["x_dtype"], a["ldx"], p(a["w"]), a["w_dtype"],
                                   p(a["targets"]), p(a["logits"]), a["logits_dtype"], a["ldl"], p(a["ws"]), a["ws_bytes"],
                                   p(a["token"]), p(a["top"]), p(a["lse"]), p(a["logp"]), None)


def test_the_entry_point_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_vocab_score_ws(200, 5000) == _WS_200_5000
    got = [(bad, want, _call(_native, bad)) for bad, want in _REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 90 and not wrong, wrong
    passed = [(bad, _call(_native, dict(bad, K=48, ldx=1024))) for bad in _PASSED]
    assert all(rc == _UNSUPPORTED for _, rc in passed), passed


# ---- the interface --------------------------------------------------------------------------------------------------------------
def _stack():
    from ea_harness.sequence import DecoderStack
    return DecoderStack(50, 128, 256, 2, 2, ATTN).eval()


def test_interface_of_rows_logprobs_and_evaluate():
    from ea_harness import sequence as sq
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    par = lambda f: inspect.signature(f).parameters                     # noqa: E731
    D = sq.DecoderStack
    assert names(D.rows_logprobs) == ["self", "rows", "table", "targets", "return_lse"]
    p = par(D.rows_logprobs)
    assert p["table"].default is inspect.Parameter.empty and p["targets"].default is None and p["return_lse"].default is False
    assert names(D.evaluate) == ["self", "tokens", "table", "key_padding_mask", "return_tokens"]
    p = par(D.evaluate)
    assert p["table"].default is None and p["key_padding_mask"].default is None and p["return_tokens"].default is False
    doc = " ".join(D.evaluate.__doc__.split())
    assert "FULL path" in doc and "ceil(rows / 128)" in doc and "ceil(rows / 64)" in doc and "`score`" in doc
    assert "ea_vocab_score" in " ".join(D.rows_logprobs.__doc__.split())
    # what stays
    assert names(D.score) == ["self", "tokens", "state"] and par(D.score)["state"].default is None
    assert "re-streamed once per 64 rows" in " ".join(D.score.__doc__.split())
    assert names(D.token_logprobs) == ["self", "rows", "state", "targets", "out", "return_lse"]


def test_evaluate_refuses_training_mode_and_a_single_token():
    stack = _stack()
    with pytest.raises(ValueError, match="at least two tokens"):
        stack.evaluate(torch.zeros(3, 1, dtype=torch.long))
    stack.train()
    with pytest.raises(NotImplementedError, match="training mode"):
        stack.evaluate(torch.zeros(3, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="training mode"):    # (decided first)
        stack.evaluate(torch.zeros(3, 1, dtype=torch.long))


def test_rows_logprobs_argument_errors():
    stack = _stack()
    rows = torch.zeros(2, 3, 128)
    table = torch.zeros(50, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="16-bit"):
        stack.rows_logprobs(rows, table.float())
    with pytest.raises(ValueError, match="16-bit"):
        stack.rows_logprobs(rows, torch.zeros(50, 256, dtype=torch.float16)[:, ::2])     # not contiguous
    with pytest.raises(ValueError, match="16-bit"):
        stack.rows_logprobs(rows, torch.zeros(50 * 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="channels"):
        stack.rows_logprobs(torch.zeros(2, 3, 64), table)
    with pytest.raises(ValueError, match="at least one row"):
        stack.rows_logprobs(torch.zeros(0, 3, 128), table)
    with pytest.raises(ValueError, match="targets"):
        stack.rows_logprobs(rows, table, targets=torch.zeros(3, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="targets"):
        stack.rows_logprobs(rows, table, targets=torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):          # a missing device is an error, never a fall-back
        stack.rows_logprobs(rows, table)


# ---- the host reference ---------------------------------------------------------------------------------------------------------
def test_reference_on_hand_computed_rows():
    inf, nan = float("inf"), float("nan")
    tok, top, lse, logp = ref.score([0.0, 0.0])
    assert (tok, top) == (0, 0.0) and abs(lse - math.log(2.0)) < 1e-15 and abs(logp + math.log(2.0)) < 1e-15
    tok, top, lse, logp = ref.score([1.0, 3.0, 3.0, -inf], target=0)
    want = 3.0 + math.log(2.0 + math.exp(-2.0))
    assert (tok, top) == (1, 3.0) and abs(lse - want) < 1e-15 and abs(logp - (1.0 - want)) < 1e-15
    assert ref.score([1.0, 3.0, 3.0, -inf], target=3)[3] == -inf
    assert all(math.isnan(ref.score([1.0, 3.0], target=t)[3]) for t in (-1, 2, 1 << 40, -(1 << 40)))
    tok, top, lse, logp = ref.score([5.0, nan, 7.0, nan])
    assert tok == 1 and math.isnan(top) and math.isnan(lse) and math.isnan(logp)
    tok, top, lse, logp = ref.score([-inf, -inf, -inf])
    assert (tok, top, lse) == (0, -inf, -inf) and math.isnan(logp)
    tok, top, lse, logp = ref.score([2.0, inf, inf], target=0)
    assert (tok, top, lse, logp) == (1, inf, inf, -inf)
    tok, top, lse, _ = ref.score([-300.0, -301.0])
    assert tok == 0 and abs(lse - (-300.0 + math.log1p(math.exp(-1.0)))) < 1e-12
    row = np.linspace(-4.0, 4.0, 1000)
    assert abs(ref.score(row)[2] - torch.logsumexp(torch.from_numpy(row), 0).item()) < 1e-12


def test_the_tolerance_is_the_written_count():
    BM, BN, SL = ref.constants()
    for V, lse64 in ((16, 0.5), (40, -3.0), (BN + 24, 2.0), (SL + BN + 8, 300.0), (2 * SL + 1000, -300.0), (32768, 11.0)):
        row = np.linspace(-3.0, 4.5, V)
        nb, NS = min(-(-V // BN), SL // BN), -(-V // SL)
        want = (7.5 + 4 * nb + NS + 15 + 2 * math.log(V)) * 2.0 ** -24 + 2.0 ** -24 * max(1.0, abs(lse64))
        assert abs(ref.tol(row, lse64) - want) < 1e-18
        assert ref.tol(row, lse64) <= 2.0 ** -16 * max(1.0, abs(lse64))
    row = np.full(40, -np.inf)
    assert np.isfinite(ref.tol(row, -np.inf))
