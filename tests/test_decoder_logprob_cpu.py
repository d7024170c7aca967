"""-m "not gpu": token log-probabilities on a held vocabulary table (ea_ceva_sdecode_vocab_logprob,
ea_ceva_sdecode_vocab_sample_logprob, C ABI 28) and DecoderStack.init_logprobs / token_logprobs / sample_tokens_logprobs /
score / generate(return_logprobs=True): the header, the binding, the workspace query, what the two entry points refuse before
any launch, the interface, and the host reference (tests/decoder_logprob_reference.py) against torch.logsumexp in fp64."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import decoder_logprob_reference as ref

ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
WS, LOGPROB, SAMPLE_LOGPROB = ("ea_ceva_sdecode_vocab_lse_ws", "ea_ceva_sdecode_vocab_logprob",
                               "ea_ceva_sdecode_vocab_sample_logprob")
_ARGMAX_ARGS = ["int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
                "int32_t w_dtype", "void* logits", "int32_t logits_dtype", "int64_t ldl", "void* ws", "int64_t ws_bytes",
                "int64_t* token", "float* top"]
_SAMPLE_ARGS = ["int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
                "int32_t w_dtype", "float* logits", "int64_t ldl", "void* ws", "int64_t ws_bytes", "int32_t top_k",
                "float top_p", "float temperature", "uint64_t seed", "int64_t* ctr", "const int32_t* sid", "int64_t* token",
                "int32_t* sel_idx", "float* sel_val", "int32_t* kept"]


# ---- C ABI 28 -------------------------------------------------------------------------------------------------------------------
def test_abi_28_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 28
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def declared(ret, name):
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (ret, name), text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("int64_t", WS) == ["int32_t M", "int32_t V"]
    # the two existing entries' lists, and behind them the new arguments
    assert declared("int", "ea_ceva_sdecode_vocab_argmax") == _ARGMAX_ARGS + ["void* stream"]
    assert declared("int", "ea_ceva_sdecode_vocab_sample") == _SAMPLE_ARGS + ["void* stream"]
    assert declared("int", LOGPROB) == _ARGMAX_ARGS + ["void* lws", "int64_t lws_bytes", "const int64_t* targets",
                                                       "float* lse", "float* logp", "void* stream"]
    assert declared("int", SAMPLE_LOGPROB) == _SAMPLE_ARGS + ["void* lws", "int64_t lws_bytes", "float* lse", "float* logp",
                                                              "void* stream"]
    I, L, P, F, U = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64
    assert _native.SIGNATURES[WS] == [I, I]
    assert _native.SIGNATURES[LOGPROB] == _native.SIGNATURES["ea_ceva_sdecode_vocab_argmax"][:-1] + [P, L, P, P, P, P]
    assert _native.SIGNATURES[SAMPLE_LOGPROB] == _native.SIGNATURES["ea_ceva_sdecode_vocab_sample"][:-1] + [P, L, P, P, P]
    assert _native.SIGNATURES[SAMPLE_LOGPROB][12:16] == [I, F, F, U]
    assert _native.lib().ea_ceva_sdecode_vocab_lse_ws.restype is ctypes.c_int64
    assert all(hasattr(lib, s) for s in (WS, LOGPROB, SAMPLE_LOGPROB))
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]
    doc = open(HEADER).read()
    assert "ABI 28" in doc and "temperature 1" in doc and "untruncated" in doc


def test_the_workspace_query(lib):  # noqa: F811
    from efficient_attention import _native
    ws = _native.lib().ea_ceva_sdecode_vocab_lse_ws
    for M, V in ((1, 1), (1, 16), (1, 17), (3, 40), (8, 1000), (64, 32768), (64, 262144)):
        assert ws(M, V) == 4 * M * ((V + 15) // 16) + 4 * M, (M, V)
    for M, V in ((0, 16), (-1, 16), (65, 16), (1, 0), (1, -5), (1 << 20, 16)):
        assert ws(M, V) < 0, (M, V)


_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_WS_8_1000 = 8 * 8 * 63
_LWS_8_1000 = 4 * 8 * 63 + 4 * 8
_NAN, _INF = float("nan"), float("inf")

_COMMON = (
    [({p: None}, _BADARG) for p in ("x", "w", "ws", "token", "lws", "lse", "logp")]                   # null
    + [({p: off}, _BADARG) for p in ("x", "w", "ws", "lws") for off in (2, 4, 8, 24)]              # not 16-byte aligned
    + [({"token": off}, _BADARG) for off in (2, 4, 12)]
    + [({p: off}, _BADARG) for p in ("lse", "logp") for off in (1, 2, 3)]
    + [({"M": n}, _BADARG) for n in (0, -1, -64)]
    + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, -256)] + [({"ldl": n}, _BADARG) for n in (999, 0, -1000)]
    + [({"ldx": 260}, _BADARG), ({"ldx": 257}, _BADARG), ({"ldx": 258, "x_dtype": _F32}, _BADARG)]
    + [({"ws_bytes": n}, _BADARG) for n in (_WS_8_1000 - 1, 8, 0, -1)]
    + [({"lws_bytes": n}, _BADARG) for n in (_LWS_8_1000 - 1, 4 * 8 * 63, 4, 0, -1)]
    + [({"w_dtype": t, "x_dtype": t}, _BADARG) for t in (_F32, 3, -1)] + [({"x_dtype": 3}, _BADARG)]
    + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _BF16}, _BADARG)]
    + [({"M": n, "ws_bytes": 1 << 40, "lws_bytes": 1 << 40}, _UNSUPPORTED) for n in (65, 128)]
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [({"V": 0, "ldl": 1000}, _UNSUPPORTED)]
    # a bad argument is decided before the geometry
    + [(dict(bad, M=65, K=48, ldx=1024), _BADARG) for bad in ({"lws": None}, {"lse": None}, {"logp": None}, {"lws": 8},
                                                             {"lse": 2}, {"token": None})]
    + [(dict(bad, K=48, ldx=1024), _BADARG) for bad in ({"lws_bytes": 0}, {"ws_bytes": 0})]
)
_GREEDY = _COMMON + (
    [({"top": off}, _BADARG) for off in (1, 2, 3)] + [({"targets": off}, _BADARG) for off in (1, 2, 4, 12)]
    + [({"logits": 33, "logits_dtype": _BF16}, _BADARG), ({"logits": 34, "logits_dtype": _F32}, _BADARG)]
    + [({"logits_dtype": t}, _BADARG) for t in (_F16, 3, -1)]
    + [(dict(bad, K=48, ldx=1024), _BADARG) for bad in ({"targets": 4},)]
)
_SAMPLED = _COMMON + (
    [({p: None}, _BADARG) for p in ("logits", "ctr", "sid")]
    + [({"ctr": off}, _BADARG) for off in (1, 4, 12)] + [({"logits": off}, _BADARG) for off in (33, 34)]
    + [({"top_p": v}, _BADARG) for v in (0.0, -0.5, 1.0000001, 2.0, _NAN, _INF)]
    + [({"temperature": v}, _BADARG) for v in (0.0, -1.0, _NAN, _INF, -_INF)]
    + [({"top_k": n}, _BADARG) for n in (0, -1, -64)]
    + [({"top_k": n}, _UNSUPPORTED) for n in (65, 128, 1 << 20)]
    + [(dict(bad, top_k=65), _BADARG) for bad in ({"ctr": None}, {"sid": None}, {"logits": None}, {"top_p": 0.0},
                                                  {"temperature": 0.0}, {"lws": None}, {"lws_bytes": 0}, {"logp": 2})]
)
# null optional arguments get past every check but the last one made here (K % 32)
_GREEDY_OK = [{}, {"logits": None}, {"top": None}, {"targets": None}, {"logits": None, "logits_dtype": 7, "ldl": 0},
              {"lws_bytes": 1 << 30}]
_SAMPLED_OK = [{}, {"sel_idx": None, "sel_val": None, "kept": None}, {"top_k": 64}, {"top_p": 1.0}, {"seed": (1 << 64) - 1}]


def _call(nv, bad, sampled):
    buf = ctypes.create_string_buffer(2048)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    arg = dict(M=8, K=256, V=1000, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, logits=32, logits_dtype=_F32, ldl=1000,
               ws=64, ws_bytes=_WS_8_1000, top_k=8, top_p=0.9, temperature=0.8, seed=5, ctr=80, sid=96, token=112,
               sel_idx=128, sel_val=132, kept=136, top=140, lws=160, lws_bytes=_LWS_8_1000, targets=176, lse=184, logp=188)
    arg.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    a = arg
    if sampled:
        return nv.lib().ea_ceva_sdecode_vocab_sample_logprob(
            a["M"], a["K"], a["V"], p(a["x"]), a["x_dtype"], a["ldx"], p(a["w"]), a["w_dtype"], p(a["logits"]), a["ldl"],
            p(a["ws"]), a["ws_bytes"], a["top_k"], a["top_p"], a["temperature"], a["seed"], p(a["ctr"]), p(a["sid"]),
            p(a["token"]), p(a["sel_idx"]), p(a["sel_val"]), p(a["kept"]), p(a["lws"]), a["lws_bytes"], p(a["lse"]),
            p(a["logp"]), None)
    return nv.lib().ea_ceva_sdecode_vocab_logprob(
        a["M"], a["K"], a["V"], p(a["x"]), a["x_dtype"], a["ldx"], p(a["w"]), a["w_dtype"], p(a["logits"]), a["logits_dtype"],
        a["ldl"], p(a["ws"]), a["ws_bytes"], p(a["token"]), p(a["top"]), p(a["lws"]), a["lws_bytes"], p(a["targets"]),
        p(a["lse"]), p(a["logp"]), None)


@pytest.mark.parametrize("sampled", [False, True], ids=["logprob", "sample_logprob"])
def test_the_entry_points_refuse_before_any_launch(lib, sampled):  # noqa: F811
    from efficient_attention import _native
    cases = _SAMPLED if sampled else _GREEDY
    got = [(bad, want, _call(_native, bad, sampled)) for bad, want in cases]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 80 and not wrong, wrong
    passed = [(bad, _call(_native, dict(bad, K=48, ldx=1024), sampled)) for bad in (_SAMPLED_OK if sampled else _GREEDY_OK)]
    assert all(rc == _UNSUPPORTED for _, rc in passed), passed


# ---- the interface --------------------------------------------------------------------------------------------------------------
def _stack():
    from ea_harness.sequence import DecoderStack
    return DecoderStack(50, 128, 256, 2, 2, ATTN).eval()


def _held_state(B=3, V=50, C=128):
    """A DecodingState as hold_vocab leaves it, on the CPU (init_logprobs and the byte count need no device)."""
    from ea_harness import sequence as sq
    return sq.DecodingState({}, None, {"batch_size": B, "dtype": torch.bfloat16},
                            (torch.zeros(V, C, dtype=torch.bfloat16), torch.zeros(8 * 64 * 4, dtype=torch.uint8)))


def test_interface_of_the_scorer():
    from ea_harness import sequence as sq
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    par = lambda f: inspect.signature(f).parameters                     # noqa: E731
    D = sq.DecoderStack
    assert names(D.init_logprobs) == ["self", "state"]
    assert names(D.token_logprobs) == ["self", "rows", "state", "targets", "out", "return_lse"]
    p = par(D.token_logprobs)
    assert p["targets"].default is None and p["out"].default is None and p["return_lse"].default is False
    assert names(D.sample_tokens_logprobs) == ["self", "rows", "state", "out"] and par(D.sample_tokens_logprobs)["out"].default is None
    assert names(D.score) == ["self", "tokens", "state"] and par(D.score)["state"].default is None
    doc = " ".join(D.score.__doc__.split())
    assert "re-streamed once per 64 rows" in doc and "corpus" in doc
    assert names(D.generate) == ["self", "prompt", "n_new", "state", "graph", "return_rows", "return_logprobs"]
    assert names(D.generate)[:5] == ["self", "prompt", "n_new", "state", "graph"]
    assert par(D.generate)["return_rows"].default is False and par(D.generate)["return_logprobs"].default is False
    # what stays
    assert names(sq.DecodingState.__init__) == ["self", "incremental", "ffn", "options", "vocab"]
    assert names(D.next_tokens) == ["self", "rows", "state", "out", "return_logits"]
    assert names(D.sample_tokens) == ["self", "rows", "state", "out", "return_details"]
    assert names(D.init_sampling) == ["self", "state", "seed", "top_k", "top_p", "temperature"]
    st = sq.DecodingState({}, None, {})
    assert st.scorer is None and "scorer" not in vars(st) and st.sampler is None and "sampler" not in vars(st)
    assert sorted(vars(st)) == ["ffn", "incremental", "options", "vocab", "vocab_ws"]


def test_init_logprobs_needs_the_table_and_the_rest_a_scorer():
    from ea_harness import sequence as sq
    stack = _stack()
    with pytest.raises(RuntimeError, match=r"hold_vocab=True"):
        stack.init_logprobs(sq.DecodingState({}, None, {"batch_size": 2}))
    for st in (sq.DecodingState({}, None, {}), _held_state()):
        with pytest.raises(RuntimeError, match=r"init_logprobs"):
            stack.token_logprobs(torch.zeros(1, 3, 128), st)
        with pytest.raises(RuntimeError, match=r"init_logprobs"):
            stack.sample_tokens_logprobs(torch.zeros(1, 3, 128), st)
        with pytest.raises(RuntimeError, match=r"init_logprobs"):      # before the prefill: nothing here is on a device
            stack.generate(torch.zeros(3, 4, dtype=torch.long), 2, st, return_logprobs=True)
        with pytest.raises(RuntimeError, match=r"init_logprobs"):
            stack.score(torch.zeros(3, 4, dtype=torch.long), st)
    with pytest.raises(RuntimeError, match=r"init_logprobs"):
        stack.generate(torch.zeros(3, 4, dtype=torch.long), 2, None, return_logprobs=True)
    scored = stack.init_logprobs(_held_state())
    with pytest.raises(RuntimeError, match=r"init_sampling"):          # a scorer alone does not sample
        stack.sample_tokens_logprobs(torch.zeros(1, 3, 128), scored)


def test_the_scorer_and_its_bytes(lib):  # noqa: F811
    stack = _stack()
    B, V = 3, 50
    st = _held_state(B, V)
    before = stack.decoding_state_nbytes(st)
    assert stack.init_logprobs(st) is st and "scorer" in vars(st)
    sc = st.scorer
    assert sc.ws.dtype == torch.uint8 and sc.ws.numel() == 4 * 64 * ((V + 15) // 16) + 4 * 64
    for t in (sc.lse, sc.logp):
        assert t.dtype == torch.float32 and tuple(t.shape) == (B,)
    assert stack.decoding_state_nbytes(st) - before == sc.ws.numel() + 8 * B
    stack.init_sampling(st, 11, 8, 0.9, 0.8)
    assert stack.decoding_state_nbytes(st) - before == sc.ws.numel() + 8 * B + 4 * B * V + 12 * B
    # a reorder and a reset move the sampler's streams and nothing of the scorer
    kept = (sc.ws.data_ptr(), sc.lse.data_ptr(), sc.logp.data_ptr())
    stack.layers = torch.nn.ModuleList()
    stack.reorder_decoding_state(st, torch.tensor([2, 0, 0]))
    stack.reset_decoding_rows(st, [1])
    assert st.scorer is sc and kept == (sc.ws.data_ptr(), sc.lse.data_ptr(), sc.logp.data_ptr())
    with pytest.raises(ValueError, match="channels"):
        stack.token_logprobs(torch.zeros(1, 3, 64), st)
    with pytest.raises(ValueError, match="targets"):
        stack.token_logprobs(torch.zeros(2, 3, 128), st, targets=torch.zeros(3, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="single-token step"):
        stack.sample_tokens_logprobs(torch.zeros(2, 3, 128), st)


# ---- the host reference ---------------------------------------------------------------------------------------------------------
def test_reference_against_torch_logsumexp_on_random_rows():
    g = torch.Generator().manual_seed(28)
    for V in (1, 16, 17, 40, 1000, 4808):
        for sigma, shift in ((1.0, 0.0), (0.01, 0.0), (20.0, 0.0), (5.0, -300.0), (5.0, 300.0)):
            row = (torch.randn(V, generator=g) * sigma + shift).float()
            want = torch.logsumexp(row.double(), 0).item()
            got = ref.lse(row.numpy())
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (V, sigma, shift, got, want)
            lsm = torch.log_softmax(row.double(), 0)
            for t in (0, V - 1, int(row.argmax())):
                assert abs(ref.logp(row.numpy(), t) - lsm[t].item()) <= 1e-12 * max(1.0, abs(want))
            assert math.isnan(ref.logp(row.numpy(), -1)) and math.isnan(ref.logp(row.numpy(), V))
            assert ref.spread(row.numpy()) == (row.max().double() - row.min().double()).item()
            NB = (V + 15) // 16
            assert ref.tol(row.numpy(), want) == (2 * ref.spread(row.numpy()) + 40 + NB / 512) * 2.0 ** -24 \
                + 2.0 ** -22 * max(1.0, abs(want))


def test_reference_on_special_rows():
    inf, nan = float("inf"), float("nan")
    base = np.linspace(-3.0, 2.0, 40).astype(np.float32)

    def same(a, b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    for name, edit in (("nan", {7: nan}), ("nan_and_inf", {7: nan, 9: inf}), ("inf", {9: inf}), ("minus_inf", {5: -inf}),
                       ("tile_of_minus_inf", {i: -inf for i in range(16, 32)}), ("all_minus_inf", {i: -inf for i in range(40)})):
        row = base.copy()
        for i, v in edit.items():
            row[i] = v
        want = torch.logsumexp(torch.from_numpy(row).double(), 0).item()
        got = ref.lse(row)
        assert same(got, want) or abs(got - want) <= 1e-12, (name, got, want)
        assert np.isfinite(ref.tol(row, got))
    row = base.copy()
    row[5] = -inf
    assert ref.logp(row, 5) == -inf and ref.spread(row) == 5.0
    row[:] = -inf
    assert ref.lse(row) == -inf and ref.spread(row) == 0.0 and math.isnan(ref.logp(row, 3))
    row = base.copy()
    row[9] = inf
    assert ref.lse(row) == inf and ref.logp(row, 0) == -inf and math.isnan(ref.logp(row, 9))
