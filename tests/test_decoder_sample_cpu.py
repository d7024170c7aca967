"""-m "not gpu": the sampled token pick on a held vocabulary table (ea_ceva_sdecode_vocab_sample, C ABI 27) and
DecoderStack.init_sampling / sample_tokens: the host reference against known answers, the header, the binding, what the entry
point refuses before any launch, the interface, and the preconditions of the operands the GPU tests
(tests/test_gpu_decoder_sample.py) run on the kernel -- among them that at least 95 % of the draws of every case are decided
uniquely under the error bound the GPU test allows."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import decoder_sample_operands as sops
import decoder_sample_reference as ref
import decoder_vocab_operands as ops

ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
WS, SAMPLE = "ea_ceva_sdecode_vocab_sample_ws", "ea_ceva_sdecode_vocab_sample"


# ---- the host reference ---------------------------------------------------------------------------------------------------------
def _philox_scalar(counter, key):
    """Philox4x32-10 in plain Python integers, written apart from the vectorised one."""
    c, k = list(counter), list(key)
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
    return c


_KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
          ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
          ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
           (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for counter, key, want in _KNOWN:
        assert tuple(_philox_scalar(counter, key)) == want
        assert tuple(int(x) for x in ref.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))) == want
    got = ref.philox4x32_10(np.array([k[0] for k in _KNOWN], dtype=np.uint64), np.array([k[1] for k in _KNOWN], dtype=np.uint64))
    assert got.shape == (3, 4) and [tuple(int(x) for x in row) for row in got] == [k[2] for k in _KNOWN]


def test_uniform_is_the_first_word_of_the_draws_counter():
    seed = sops.SEED
    ctr = np.array([0, 1, (1 << 32) + 5, (1 << 40) - 1], dtype=np.int64)
    sid = np.array([0, 7, 3, 2 ** 31 - 1], dtype=np.int64)
    u = ref.uniform(seed, ctr, sid)
    assert u.dtype == np.float32
    for n, s, got in zip(ctr.tolist(), sid.tolist(), u.tolist()):
        word = _philox_scalar((n & 0xFFFFFFFF, n >> 32, s, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
        exact = ((word >> 8) + 0.5) * 2.0 ** -24
        assert abs(got - exact) <= 2.0 ** -25 and 0.0 < got <= 1.0
        if word >> 8 < 1 << 23:
            assert got == exact                                           # 24 bits: exact in fp32
    grid = ref.uniform(seed, np.arange(64).reshape(64, 1), np.arange(3).reshape(1, 3))
    assert grid.shape == (64, 3) and len(set(grid.reshape(-1).tolist())) > 180          # streams and counters differ
    assert grid[5, 2] == ref.uniform(seed, 5, 2)


def test_total_order_topk():
    inf, nan = float("inf"), float("nan")
    row = np.array([1.0, nan, 3.0, -0.0, 3.0, inf, 0.0, nan, -inf, 2.0], dtype=np.float32)
    assert ref.topk(row, 64).tolist() == [1, 7, 5, 2, 4, 9, 0, 3, 6, 8]
    assert ref.topk(row, 3).tolist() == [1, 7, 5] and ref.topk(row, 1).tolist() == [1]
    assert ref.topk(np.tile(np.array([2.0, 5.0, 1.0], dtype=np.float32), 5), 7).tolist() == [1, 4, 7, 10, 13, 0, 3]


def test_admissible_sets():
    c = ref.cumulative(np.array([2.0, 1.0, 0.0, -np.inf]), 1.0)
    assert np.allclose(c, [1.0, 1.0 + np.exp(-1.0), 1.0 + np.exp(-1.0) + np.exp(-2.0)] + [1.0 + np.exp(-1.0) + np.exp(-2.0)])
    assert ref.eps(c) == 4 * 2.0 ** -20 * c[-1]
    assert ref.admissible_kept(c, 0.5) == [1] and ref.admissible_kept(c, 0.9) == [2]
    assert ref.admissible_kept(c, 1.0) == [3, 4]                        # (a weight of 0: both heads reach the whole)
    assert ref.admissible_kept(c, c[0] / c[-1]) == [1, 2]               # on the boundary: either
    assert ref.admissible_js(c, 3, 0.5) == [0] and ref.admissible_js(c, 3, 0.99) == [2]
    assert ref.admissible_js(c, 3, c[0] / c[2]) == [0, 1] and ref.admissible_js(c, 2, 1.0) == [1]
    assert np.allclose(ref.cumulative(np.array([1.0, 0.3]), 0.7), [1.0, 1.0 + np.exp(-1.0)])


# ---- C ABI 27 -------------------------------------------------------------------------------------------------------------------
def test_abi_27_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 27
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def declared(ret, name):
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (ret, name), text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("int64_t", WS) == ["int32_t M", "int32_t V"]
    assert declared("int", SAMPLE) == [
        "int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
        "int32_t w_dtype", "float* logits", "int64_t ldl", "void* ws", "int64_t ws_bytes", "int32_t top_k", "float top_p",
        "float temperature", "uint64_t seed", "int64_t* ctr", "const int32_t* sid", "int64_t* token", "int32_t* sel_idx",
        "float* sel_val", "int32_t* kept", "void* stream"]
    I, L, P, F, U = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64
    assert _native.SIGNATURES[WS] == [I, I]
    assert _native.SIGNATURES[SAMPLE] == [I, I, I, P, I, L, P, I, P, L, P, L, I, F, F, U, P, P, P, P, P, P, P]
    assert _native.lib().ea_ceva_sdecode_vocab_sample_ws.restype is ctypes.c_int64
    assert hasattr(lib, WS) and hasattr(lib, SAMPLE)
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]
    ws, ws26 = _native.lib().ea_ceva_sdecode_vocab_sample_ws, _native.lib().ea_ceva_sdecode_vocab_ws
    for M, V in ((1, 1), (1, 17), (8, 1000), (64, 32768), (64, 262144), (0, 16), (65, 16), (1, 0)):
        assert ws(M, V) == ws26(M, V) and (ws(M, V) > 0) == (1 <= M <= 64 and V >= 1)        # one workspace serves both


_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_WS_8_1000 = 8 * 8 * 63
_NAN, _INF = float("nan"), float("inf")
_REFUSED = (
    [({p: None}, _BADARG) for p in ("x", "w", "ws", "token", "logits", "ctr", "sid")]                 # null
    + [({p: off}, _BADARG) for p in ("x", "w", "ws") for off in (2, 4, 8, 24)]                      # not 16-byte aligned
    + [({"token": off}, _BADARG) for off in (2, 4, 12)] + [({"ctr": off}, _BADARG) for off in (1, 4, 12)]
    + [({"logits": off}, _BADARG) for off in (33, 34)]
    + [({"M": n}, _BADARG) for n in (0, -1, -64)]
    + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, -256)] + [({"ldl": n}, _BADARG) for n in (999, 0, -1000)]
    + [({"ldx": 260}, _BADARG), ({"ldx": 257}, _BADARG), ({"ldx": 258, "x_dtype": _F32}, _BADARG)]
    + [({"ws_bytes": n}, _BADARG) for n in (_WS_8_1000 - 1, 8, 0, -1)]
    + [({"w_dtype": t, "x_dtype": t}, _BADARG) for t in (_F32, 3, -1)] + [({"x_dtype": 3}, _BADARG)]
    + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _BF16}, _BADARG)]
    + [({"top_p": v}, _BADARG) for v in (0.0, -0.5, 1.0000001, 2.0, _NAN, _INF)]
    + [({"temperature": v}, _BADARG) for v in (0.0, -1.0, _NAN, _INF, -_INF)]
    + [({"top_k": n}, _BADARG) for n in (0, -1, -64)]
    + [({"top_k": n}, _UNSUPPORTED) for n in (65, 128, 1 << 20)]
    + [({"M": n, "ws_bytes": 1 << 40}, _UNSUPPORTED) for n in (65, 128)]
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    # a bad argument is decided before the geometry
    + [(dict(bad, top_k=65), _BADARG) for bad in ({"ctr": None}, {"sid": None}, {"logits": None}, {"top_p": 0.0},
                                                  {"temperature": 0.0}, {"ctr": 4}, {"ws_bytes": 0})]
    + [(dict(bad, M=65, K=48, ldx=1024), _BADARG) for bad in ({"top_k": 0}, {"top_p": 1.5}, {"temperature": _NAN})]
)
# accepted values of the scalars and null optional outputs get past every check but the last one made here (K % 32)
_NOT_REFUSED = [{"top_p": 1.0}, {"top_p": 1e-6}, {"temperature": 1e-3}, {"temperature": 100.0}, {"top_k": 1}, {"top_k": 64},
                {"sel_idx": None, "sel_val": None, "kept": None}, {"seed": (1 << 64) - 1}]


def _call(nv, bad):
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    arg = dict(M=8, K=256, V=1000, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, logits=32, ldl=1000, ws=64,
               ws_bytes=_WS_8_1000, top_k=8, top_p=0.9, temperature=0.8, seed=5, ctr=80, sid=96, token=112, sel_idx=128,
               sel_val=132, kept=136)
    arg.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    return nv.lib().ea_ceva_sdecode_vocab_sample(
        arg["M"], arg["K"], arg["V"], p(arg["x"]), arg["x_dtype"], arg["ldx"], p(arg["w"]), arg["w_dtype"], p(arg["logits"]),
        arg["ldl"], p(arg["ws"]), arg["ws_bytes"], arg["top_k"], arg["top_p"], arg["temperature"], arg["seed"], p(arg["ctr"]),
        p(arg["sid"]), p(arg["token"]), p(arg["sel_idx"]), p(arg["sel_val"]), p(arg["kept"]), None)


def test_sample_entry_point_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _call(_native, bad)) for bad, want in _REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 80 and not wrong, wrong
    passed = [(bad, _call(_native, dict(bad, K=48, ldx=1024))) for bad in _NOT_REFUSED]
    assert all(rc == _UNSUPPORTED for _, rc in passed), passed


# ---- the stack ------------------------------------------------------------------------------------------------------------------
def _stack():
    from ea_harness.sequence import DecoderStack
    return DecoderStack(50, 128, 256, 2, 2, ATTN).eval()


def _held_state(B=3, V=50, C=128):
    """A DecodingState as hold_vocab leaves it, on the CPU (init_sampling and the byte count need no device)."""
    from ea_harness import sequence as sq
    return sq.DecodingState({}, None, {"batch_size": B, "dtype": torch.bfloat16},
                            (torch.zeros(V, C, dtype=torch.bfloat16), torch.zeros(8 * 64 * 4, dtype=torch.uint8)))


def test_interface_of_the_sampler():
    from ea_harness import sequence as sq
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    assert names(sq.DecodingState.__init__) == ["self", "incremental", "ffn", "options", "vocab"]
    assert names(sq.DecoderStack.init_sampling) == ["self", "state", "seed", "top_k", "top_p", "temperature"]
    par = inspect.signature(sq.DecoderStack.init_sampling).parameters
    assert par["top_p"].default == 1.0 and par["temperature"].default == 1.0
    assert names(sq.DecoderStack.sample_tokens) == ["self", "rows", "state", "out", "return_details"]
    par = inspect.signature(sq.DecoderStack.sample_tokens).parameters
    assert par["out"].default is None and par["return_details"].default is False
    assert names(sq.DecoderStack.next_tokens) == ["self", "rows", "state", "out", "return_logits"]
    assert names(sq.DecoderStack.generate)[:5] == ["self", "prompt", "n_new", "state", "graph"]
    st = sq.DecodingState({}, None, {})
    assert st.sampler is None and "sampler" not in vars(st)             # (the attributes of a state are what they were)


def test_init_sampling_needs_the_table_and_sample_tokens_a_sampler():
    from ea_harness import sequence as sq
    stack = _stack()
    with pytest.raises(RuntimeError, match=r"hold_vocab=True"):
        stack.init_sampling(sq.DecodingState({}, None, {"batch_size": 2}), 1, 8)
    with pytest.raises(RuntimeError, match=r"init_sampling"):
        stack.sample_tokens(torch.zeros(1, 2, 128), sq.DecodingState({}, None, {}))
    with pytest.raises(RuntimeError, match=r"init_sampling"):
        stack.sample_tokens(torch.zeros(1, 3, 128), _held_state())


@pytest.mark.parametrize("bad", [dict(top_k=0), dict(top_k=65), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
                                 dict(top_p=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
                                 dict(temperature=float("inf")), dict(temperature=float("nan")), dict(seed=-1),
                                 dict(seed=1 << 64)], ids=str)
def test_values_outside_the_envelope_raise_before_anything_is_allocated(bad, monkeypatch):
    stack, st = _stack(), _held_state()
    arg = dict(seed=3, top_k=8, top_p=0.9, temperature=0.8)
    arg.update(bad)

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the check")
    for name in ("empty", "zeros", "arange"):
        monkeypatch.setattr(torch, name, no_alloc)
    with pytest.raises(ValueError, match=next(iter(bad)) if "seed" not in bad else "seed"):
        stack.init_sampling(st, **arg)
    assert st.sampler is None


def test_the_sampler_and_its_bytes():
    stack = _stack()
    B, V = 3, 50
    st = _held_state(B, V)
    before = stack.decoding_state_nbytes(st)
    assert stack.init_sampling(st, 11, 8, 0.9, 0.8) is st
    sm = st.sampler
    assert (sm.seed, sm.top_k, sm.top_p, sm.temperature, sm.next_sid) == (11, 8, 0.9, 0.8, B)
    assert sm.logits.dtype == torch.float32 and tuple(sm.logits.shape) == (B, V)
    assert sm.ctr.dtype == torch.long and sm.ctr.tolist() == [0] * B
    assert sm.sid.dtype == torch.int32 and sm.sid.tolist() == list(range(B))
    assert stack.decoding_state_nbytes(st) - before == 4 * B * V + 8 * B + 4 * B
    assert stack.refresh_decoding_weights.__doc__ and st.vocab_ws.numel() == 8 * 64 * 4      # the workspace is vocab_ws
    for bad in (torch.zeros(2, 3, 128), torch.zeros(1, 4, 128)):         # T = 1, and no more rows than the state has
        with pytest.raises(ValueError, match="single-token step"):
            stack.sample_tokens(bad, st)
    with pytest.raises(ValueError, match="channels"):
        stack.sample_tokens(torch.zeros(1, 3, 64), st)


# ---- the operands of the GPU tests ----------------------------------------------------------------------------------------------
def _host_logits(x32, w):
    return (x32.to(w.dtype).double() @ w.double().t()).float().numpy()


def unique_share(logits, k, temperature, top_p, seed, draws):
    """Of draws ctr = 0 .. draws - 1 of every row (sid = the row), the share with exactly one admissible j."""
    M = logits.shape[0]
    u = ref.uniform(seed, np.arange(draws).reshape(draws, 1), np.arange(M).reshape(1, M))
    one = 0
    for m in range(M):
        c = ref.cumulative(logits[m][ref.topk(logits[m], k)], temperature)
        kept = ref.admissible_kept(c, top_p)[0]
        one += int((ref.admissible_mask(c, np.full(draws, kept), u[:, m]).sum(1) == 1).sum())
    return one / (draws * M)


def test_at_least_95_percent_of_the_draws_are_decided_uniquely():
    worst = 1.0
    cases = [(shape, wd) for shape in sops.SHAPES for wd in ops.W_DTYPES] + [(sops.LM, torch.bfloat16)]
    for shape, wdtype in cases:
        x32, w = ops.operands(shape, wdtype, 0)
        L = _host_logits(x32, w)
        assert np.isfinite(L).all()
        for k in sops.KS:
            for T in sops.TEMPERATURES:
                for p in sops.TOP_PS:
                    share = unique_share(L, k, T, p, sops.SEED, sops.DRAWS)
                    worst = min(worst, share)
                    assert share >= 0.95, (shape, wdtype, k, T, p, share)
    print("smallest share of uniquely decided draws: %.4f" % worst)


def test_constructed_tables_meet_their_preconditions():
    seen = {"one_tile": 0, "spread": 0}
    for shape in sops.SHAPES:
        M, K, V = shape
        for wdtype in ops.W_DTYPES:
            for k in sops.KS:
                for name, make in (("one_tile", sops.one_tile), ("spread", sops.spread)):
                    got = make(shape, wdtype, k)
                    if got is None:
                        continue
                    x32, w, cols = got
                    seen[name] += 1
                    assert len(set(cols)) == k and all(0 <= v < V for v in cols) and torch.isfinite(w.float()).all()
                    tiles = {v // 16 for v in cols}
                    if name == "one_tile":
                        assert len(tiles) == 1
                    else:
                        assert len(tiles) == k and (V - 1) // 16 in tiles
                    assert sops.lifted_margin(x32, w, cols) > 0.0, (name, shape, wdtype, k)
                    L = _host_logits(x32, w)
                    assert all(set(ref.topk(L[m], k).tolist()) == set(cols) for m in range(M))
            x32, w = sops.period3(shape, wdtype)
            assert torch.equal(w, w[torch.arange(V) % 3]) and len({tuple(r.tolist()) for r in w[:3].float()}) == 3
            L = _host_logits(x32, w)
            for m in range(M):                                            # the best class, lowest columns first
                best = int(np.argmax(L[m, :3]))
                n = min(5, len(range(best, V, 3)))
                assert ref.topk(L[m], n).tolist() == list(range(best, V, 3))[:n]
    # one_tile: k = 1, 5 (and 16 where a tile of 16 is live); spread: every k on the 4808-column table, 40 on 1000
    assert seen["one_tile"] >= 2 * 12 and seen["spread"] >= 2 * 12, seen
    assert sops.spread((16, 256, 4808), torch.bfloat16, 64) is not None and sops.spread((64, 1024, 1000), torch.float16, 40) is not None
