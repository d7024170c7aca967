"""-m "not gpu": the greedy token pick on a held vocabulary table (ea_ceva_sdecode_vocab_argmax, C ABI 26) and the
`hold_vocab` option of ea_harness.sequence.DecoderStack: the header, the binding, what the entry point refuses before any
launch, the workspace query, the refusals of `init_decoding` / `next_tokens` that need no device, and the preconditions of the
operands the GPU tests (tests/test_gpu_decoder_vocab.py) run on the kernel."""
import ctypes
import inspect
import re

import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import decoder_vocab_operands as ops

ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
WS, ARGMAX = "ea_ceva_sdecode_vocab_ws", "ea_ceva_sdecode_vocab_argmax"


def _stack(**kw):
    from ea_harness.sequence import DecoderStack
    return DecoderStack(50, 128, 256, 2, 2, ATTN, **kw)


# ---- C ABI 26 -------------------------------------------------------------------------------------------------------------------
def test_abi_26_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 26
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def declared(ret, name):
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (ret, name), text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("int64_t", WS) == ["int32_t M", "int32_t V"]
    assert declared("int", ARGMAX) == [
        "int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
        "int32_t w_dtype", "void* logits", "int32_t logits_dtype", "int64_t ldl", "void* ws", "int64_t ws_bytes",
        "int64_t* token", "float* top", "void* stream"]
    I, L, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _native.SIGNATURES[WS] == [I, I]
    assert _native.SIGNATURES[ARGMAX] == [I, I, I, P, I, L, P, I, P, I, L, P, L, P, P, P]
    assert _native.lib().ea_ceva_sdecode_vocab_ws.restype is ctypes.c_int64
    assert hasattr(lib, WS) and hasattr(lib, ARGMAX)
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]


_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_WS_8_1000 = 8 * 8 * 63                                      # 8 bytes x 8 rows x ceil(1000 / 16) candidates
# (what is wrong, expected return).  Pointers are offsets from a 16-byte aligned base (or None).  Only refused calls: an
# accepted one launches.
_REFUSED = (
    [({p: None}, _BADARG) for p in ("x", "w", "ws", "token")]                           # null
    + [({p: off}, _BADARG) for p in ("x", "w", "ws") for off in (2, 4, 8, 24)]          # not 16-byte aligned
    + [({"token": off}, _BADARG) for off in (2, 4, 12)] + [({"top": off}, _BADARG) for off in (1, 2, 6)]
    + [({"logits": 50, "logits_dtype": _F32}, _BADARG), ({"logits": 49}, _BADARG)]      # logits: not aligned to its element
    + [({"M": n}, _BADARG) for n in (0, -1, -64)]
    + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, -256)]                                   # ldx < K
    + [({"ldl": n}, _BADARG) for n in (999, 0, -1000)]                                  # ldl < V with logits set
    + [({"ldx": 260}, _BADARG), ({"ldx": 257}, _BADARG), ({"ldx": 258, "x_dtype": _F32}, _BADARG)]   # unaligned rows
    + [({"ws_bytes": n}, _BADARG) for n in (_WS_8_1000 - 1, 8, 0, -1)]                  # ws too small
    + [({"M": 64, "ws_bytes": 8 * 64 * 63 - 8}, _BADARG), ({"V": 1009, "ldl": 1016}, _BADARG)]
    + [({"w_dtype": t, "x_dtype": t, "logits_dtype": t}, _BADARG) for t in (_F32, 3, -1)]            # a bad dtype code
    + [({"x_dtype": 3}, _BADARG), ({"logits_dtype": 3}, _BADARG), ({"logits_dtype": -1}, _BADARG)]
    + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _BF16, "logits_dtype": _F16}, _BADARG)]
    + [({"w_dtype": _BF16, "logits_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _F16, "logits_dtype": _BF16}, _BADARG)]
    + [({"M": n, "ws_bytes": 1 << 40}, _UNSUPPORTED) for n in (65, 128, 1 << 20)]
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [({"V": n, "logits": None}, _UNSUPPORTED) for n in (0, -1, -1000)] + [({"V": 0, "ldl": 0}, _UNSUPPORTED)]
    # a bad argument is decided before the geometry
    + [(dict(bad, M=65), _BADARG) for bad in ({"x": None}, {"ws": 8}, {"token": None}, {"ldx": 255}, {"x_dtype": 3}, {"ldl": 999})]
    + [(dict(bad, K=48, ldx=1024), _BADARG) for bad in ({"w": None}, {"ws_bytes": 0}, {"logits_dtype": 3})]
    + [({"M": 65, "K": 48, "V": 0, "ldx": 1024, "logits": None}, _UNSUPPORTED)]
)
# ... and what is NOT read: logits_dtype / ldl without logits, top when null.  These calls get past every check but the last
# one made here (K % 32), which stands in for the launch.
_NOT_READ = [{"logits": None, "logits_dtype": 3}, {"logits": None, "ldl": 0}, {"logits": None, "ldl": -5}, {"top": None},
             {"ws_bytes": _WS_8_1000}, {"ws_bytes": 1 << 40}]


def _call(nv, bad):
    buf = ctypes.create_string_buffer(512)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    arg = dict(M=8, K=256, V=1000, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, logits=32, logits_dtype=_BF16, ldl=1000,
               ws=64, ws_bytes=_WS_8_1000, token=80, top=96)
    arg.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    return nv.lib().ea_ceva_sdecode_vocab_argmax(
        arg["M"], arg["K"], arg["V"], p(arg["x"]), arg["x_dtype"], arg["ldx"], p(arg["w"]), arg["w_dtype"], p(arg["logits"]),
        arg["logits_dtype"], arg["ldl"], p(arg["ws"]), arg["ws_bytes"], p(arg["token"]), p(arg["top"]), None)


def test_vocab_entry_point_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _call(_native, bad)) for bad, want in _REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 70 and not wrong, wrong
    unread = [(bad, _call(_native, dict(bad, K=48, ldx=1024))) for bad in _NOT_READ]
    assert all(rc == _UNSUPPORTED for _, rc in unread), unread


def test_workspace_query_is_monotone_and_refuses(lib):  # noqa: F811
    from efficient_attention import _native
    ws = _native.lib().ea_ceva_sdecode_vocab_ws
    Ms = [1, 2, 15, 16, 17, 32, 33, 63, 64]
    Vs = [1, 2, 15, 16, 17, 40, 1000, 4808, 32768, 267744, (1 << 31) - 1]
    table = [[ws(M, V) for V in Vs] for M in Ms]
    assert all(n > 0 for row in table for n in row)
    assert all(a <= b for row in table for a, b in zip(row, row[1:]))                    # in V
    assert all(a < b for r0, r1 in zip(table, table[1:]) for a, b in zip(r0, r1))      # in M
    assert ws(1, 1) == ws(1, 16) == 8 and ws(1, 17) == 16 and ws(64, 32768) == 8 * 64 * 2048
    assert ws(64, (1 << 31) - 1) == 8 * 64 * (1 << 27)                                   # (no 32-bit overflow)
    for M, V in ((0, 16), (-1, 16), (65, 16), (1 << 20, 16), (1, 0), (1, -1), (64, -(1 << 31)), (0, 0)):
        assert ws(M, V) < 0, (M, V)


# ---- the stack ------------------------------------------------------------------------------------------------------------------
def test_hold_vocab_refuses_fp32_with_hold_weights_error():
    stack = _stack().eval()
    for rolling in (True, False):
        for hold_weights in (False, True):
            with pytest.raises(ValueError, match="holds 16-bit projection weights"):
                stack.init_decoding(2, 16, torch.float32, "cpu", rolling=rolling, hold_weights=hold_weights, hold_vocab=True)
            with pytest.raises(ValueError, match="holds 16-bit projection weights"):
                stack.init_decoding(batch_size=2, max_tokens=16, device="cpu", rolling=rolling, hold_weights=hold_weights,
                                    hold_vocab=True, dtype=torch.float32)
    with pytest.raises(ValueError, match="hold_vocab=True"):
        stack.init_decoding(2, 16, torch.float32, "cpu", hold_weights=False, hold_vocab=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a 16-bit one goes on to the device check
        stack.init_decoding(2, 16, torch.bfloat16, "cpu", hold_weights=False, hold_vocab=True)


def test_interface_of_the_option():
    from ea_harness import sequence as sq
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    assert names(sq.DecodingState.__init__) == ["self", "incremental", "ffn", "options", "vocab"]
    assert inspect.signature(sq.DecodingState.__init__).parameters["vocab"].default is None
    st = sq.DecodingState({}, None, {"dtype": torch.bfloat16})          # the three-argument form
    assert st.vocab is None and st.vocab_ws is None and not st.hold_vocab and not st.hold_weights
    a, b = torch.zeros(2, 2), torch.zeros(8, dtype=torch.uint8)
    st = sq.DecodingState({}, None, {}, (a, b))
    assert st.vocab is a and st.vocab_ws is b and st.hold_vocab
    assert names(sq.DecoderStack.next_tokens) == ["self", "rows", "state", "out", "return_logits"]
    nt = inspect.signature(sq.DecoderStack.next_tokens).parameters
    assert nt["out"].default is None and nt["return_logits"].default is False
    assert names(sq.DecoderStack.generate)[:5] == ["self", "prompt", "n_new", "state", "graph"]
    doc = " ".join(sq.DecoderStack.next_tokens.__doc__.split())
    assert "FP32 SUMS" in doc and "rounded to 16 bits" in doc


def test_next_tokens_without_the_table_names_the_option():
    from ea_harness import sequence as sq
    stack = _stack().eval()
    st = sq.DecodingState({}, None, {})
    with pytest.raises(RuntimeError, match=r"hold_vocab=True"):
        stack.next_tokens(torch.zeros(1, 2, 128), st)
    assert stack.decoding_state_nbytes(st) == 0


# ---- the operands of the GPU tests ----------------------------------------------------------------------------------------------
def _cases():
    return [(shape, wdtype, seed) for shape in ops.SHAPES for wdtype in ops.W_DTYPES for seed in ops.seeds(shape)]


def test_operands_are_finite_and_give_inf_past_the_table():
    for shape, wdtype, seed in _cases():
        M, K, V = shape
        x32, w = ops.operands(shape, wdtype, seed)
        assert tuple(x32.shape) == (M, K) and x32.dtype == torch.float32 and tuple(w.shape) == (V, K) and w.dtype == wdtype
        assert torch.isfinite(x32).all() and torch.isfinite(w.float()).all()
        assert (x32.to(wdtype).float()[:, 0] > 0.5).all()
        x2, w2 = ops.operands(shape, wdtype, seed)
        assert torch.equal(x32, x2) and torch.equal(w, w2)               # seeded
        assert (ops.bound(x32.to(wdtype), w) > 0).all()


def test_tie_operands_meet_their_precondition():
    seen = {case: 0 for case in ops.TIE_CASES}
    for shape, wdtype, seed in _cases():
        M, K, V = shape
        for case in ops.TIE_CASES:
            got = ops.tie(shape, wdtype, seed, case)
            if got is None:
                assert ops.tie_indices(V, case) is None or V < 4, (shape, case)
                continue
            x32, w, a, b = got
            seen[case] += 1
            assert 0 <= a < b < V and torch.equal(w[a], w[b]) and torch.isfinite(w.float()).all()
            if case == "one_tile":
                assert a // 16 == b // 16
            if case in ("two_workgroups", "tail"):
                assert a // 16 != b // 16
            if case == "tail":
                assert b // 16 == (V - 1) // 16
            if case == "ends":
                assert (a, b) == (0, V - 1)
            assert (x32.to(wdtype).float()[:, 0] > 0.5).all()
            margin, equal = ops.tie_margin(x32, w, a, b)
            assert equal and margin > 0.0, (shape, wdtype, seed, case, margin)
    # every case is met by several shapes; only the single-tile shape has no pair in two tiles
    assert all(n >= 2 * 7 for n in seen.values()), seen
    assert [c for c in ops.TIE_CASES if ops.tie_indices(16, c) is None] == ["two_workgroups", "tail"]


def test_nan_operands_meet_their_precondition():
    n = 0
    for shape, wdtype, seed in _cases():
        M, K, V = shape
        for two in (False, True):
            got = ops.nan_rows(shape, wdtype, seed, two)
            assert got is not None, (shape, two)
            x32, w, rows = got
            n += 1
            assert len(rows) == (2 if two else 1) and all(0 < v < V - 1 for v in rows) and rows == sorted(set(rows))
            bad = torch.isnan(w.float())
            assert bad[rows].all() and int(bad.any(1).sum()) == len(rows)
    assert n >= 2 * 2 * 8
