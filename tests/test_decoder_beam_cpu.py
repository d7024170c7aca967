"""-m "not gpu": the beam step on a held vocabulary table (ea_ceva_sdecode_vocab_beam, ea_beam_merge, C ABI 32) and
DecoderStack.init_beam_search / beam_step / beam_search: the header, the binding, the workspace query, what the two entries
refuse before any launch, the host reference (tests/decoder_beam_reference.py) against hand-worked answers -- every event the
rule names occurs in them, and the test says so -- and the interface.  tests/test_gpu_decoder_beam.py runs the kernels and the
stack against the same reference."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import decoder_beam_reference as ref

WS, BEAM, MERGE = "ea_ceva_sdecode_vocab_beam_ws", "ea_ceva_sdecode_vocab_beam", "ea_beam_merge"
ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
F32 = np.float32
INF, NAN = float("inf"), float("nan")


# ---- C ABI 32 -------------------------------------------------------------------------------------------------------------------
def test_abi_32_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 32
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def declared(ret, name):
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (ret, name), text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("int64_t", WS) == ["int32_t M", "int32_t V", "int32_t W"]
    assert declared("int", BEAM) == [
        "int32_t M", "int32_t K", "int32_t V", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
        "int32_t w_dtype", "float* logits", "int64_t ldl", "void* ws", "int64_t ws_bytes", "int32_t W", "int32_t eos",
        "int32_t max_new", "float* score", "int32_t* t", "int32_t* nfin", "int32_t* done", "int64_t* token", "int64_t* parent",
        "int32_t* hist_tok", "int32_t* hist_par", "float* fin_score", "int32_t* fin_len", "int32_t* fin_beam",
        "int32_t* cand_idx", "float* cand_score", "float* lse", "float* sel_val", "void* stream"]
    assert declared("int", MERGE) == [
        "int32_t S", "int32_t W", "int32_t kc", "const int32_t* cand_idx", "const float* cand_score", "int32_t eos",
        "int32_t max_new", "float* score", "int32_t* t", "int32_t* nfin", "int32_t* done", "int64_t* token", "int64_t* parent",
        "int32_t* hist_tok", "int32_t* hist_par", "float* fin_score", "int32_t* fin_len", "int32_t* fin_beam", "void* stream"]
    I, L, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _native.SIGNATURES[WS] == [I, I, I]
    assert _native.SIGNATURES[BEAM] == [I, I, I, P, I, L, P, I, P, L, P, L, I, I, I] + [P] * 16 and len(_native.SIGNATURES[BEAM]) == 31
    assert _native.SIGNATURES[MERGE] == [I, I, I, P, P, I, I] + [P] * 12 and len(_native.SIGNATURES[MERGE]) == 19
    assert _native.lib().ea_ceva_sdecode_vocab_beam_ws.restype is ctypes.c_int64
    assert all(hasattr(lib, name) for name in (WS, BEAM, MERGE))
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]


def _r16(n):
    return (n + 15) // 16 * 16


def _ws_formula(M, V, W):
    """The header's: r16(8 M NB) + r16(4 M NB + 4 M) + 2 r16(8 M W) + r16(4 M), NB = ceil(V / 16)."""
    NB = (V + 15) // 16
    return _r16(8 * M * NB) + _r16(4 * M * NB + 4 * M) + 2 * _r16(8 * M * W) + _r16(4 * M)


def test_the_workspace_query():
    from efficient_attention import _native
    ws = _native.lib().ea_ceva_sdecode_vocab_beam_ws
    assert "r16(8 M NB) + r16(4 M NB + 4 M) + 2 r16(8 M W) + r16(4 M)" in open(HEADER).read()
    for M, V, W in ((1, 1, 1), (12, 1000, 4), (64, 32768, 32), (3, 40, 3), (17, 64, 17)):
        assert ws(M, V, W) == _ws_formula(M, V, W) > 0, (M, V, W)
    assert ws(12, 1000, 4) == 6048 + 3072 + 2 * 384 + 48
    for M, V, W in ((0, 16, 1), (-4, 16, 2), (65, 16, 1), (66, 16, 33), (8, 0, 2), (8, -1, 2), (8, 16, 0), (8, 16, -2), (33, 16, 33),
                    (8, 16, 3), (64, 16, 24)):
        assert ws(M, V, W) < 0, (M, V, W)


_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_WS_8_1000_4 = _ws_formula(8, 1000, 4)
_STATE = ("score", "t", "nfin", "done", "token", "parent", "hist_tok", "hist_par", "fin_score", "fin_len", "fin_beam")
_REPORTS = ("cand_idx", "cand_score", "lse", "sel_val")
_REFUSED = (
    [({p: None}, _BADARG) for p in ("x", "w", "ws", "logits") + _STATE]                                   # null
    + [({p: off}, _BADARG) for p in ("x", "w", "ws") for off in (2, 4, 8, 24)]                            # not 16-byte aligned
    + [({p: off}, _BADARG) for p in ("token", "parent") for off in (2, 4, 12)]
    + [({p: off}, _BADARG) for p in _STATE[:4] + _STATE[6:] + _REPORTS for off in (1, 2)]
    + [({"logits": off}, _BADARG) for off in (33, 34)]
    + [({"M": n}, _BADARG) for n in (0, -1, -64)]
    + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, -256)] + [({"ldl": n}, _BADARG) for n in (999, 0, -1000)]
    + [({"ldx": 260}, _BADARG), ({"ldx": 257}, _BADARG), ({"ldx": 258, "x_dtype": _F32}, _BADARG)]
    + [({"ws_bytes": n}, _BADARG) for n in (_WS_8_1000_4 - 1, 8, 0, -1)]
    + [({"w_dtype": t, "x_dtype": t}, _BADARG) for t in (_F32, 3, -1)] + [({"x_dtype": 3}, _BADARG)]
    + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _BF16}, _BADARG)]
    + [({"eos": n}, _BADARG) for n in (-1, 1000, 1 << 20)]
    + [({"max_new": n}, _BADARG) for n in (0, -1)]
    + [({"W": n}, _BADARG) for n in (0, -1, -4)]
    + [({"W": n, "ws_bytes": 1 << 40}, _UNSUPPORTED) for n in (33, 64, 3, 5)]                             # W > 32, M % W != 0
    + [({"M": n, "ws_bytes": 1 << 40}, _UNSUPPORTED) for n in (68, 128)]
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [({"V": n, "eos": 0, "ws_bytes": 1 << 40}, _UNSUPPORTED) for n in (0, -5)]
    # a bad argument is decided before the geometry
    + [(dict(bad, W=33, K=48, ldx=1024), _BADARG) for bad in ({"score": None}, {"done": None}, {"logits": None}, {"eos": -1},
                                                             {"max_new": 0}, {"parent": 4}, {"ws": None})]
    + [(dict(bad, M=68, ws_bytes=1 << 40), _BADARG) for bad in ({"eos": 1000}, {"fin_beam": None}, {"lse": 2})]
)
_NOT_REFUSED = [{"eos": 0}, {"eos": 999}, {"max_new": 1}, {"W": 1}, {"W": 8, "ws_bytes": 1 << 40}, {"W": 2, "M": 64, "ws_bytes": 1 << 40},
                {"cand_idx": None, "cand_score": None, "lse": None, "sel_val": None}, {"x_dtype": _F32, "ldx": 256}]


def _p(base, off):
    return None if off is None else ctypes.c_void_p(base + off)


def _call(nv, bad):
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    arg = dict(M=8, K=256, V=1000, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, logits=32, ldl=1000, ws=64,
               ws_bytes=_WS_8_1000_4, W=4, eos=2, max_new=12, score=80, t=84, nfin=88, done=92, token=96, parent=104,
               hist_tok=112, hist_par=116, fin_score=120, fin_len=124, fin_beam=128, cand_idx=132, cand_score=136, lse=140,
               sel_val=144)
    arg.update(bad)
    return nv.lib().ea_ceva_sdecode_vocab_beam(
        arg["M"], arg["K"], arg["V"], _p(base, arg["x"]), arg["x_dtype"], arg["ldx"], _p(base, arg["w"]), arg["w_dtype"],
        _p(base, arg["logits"]), arg["ldl"], _p(base, arg["ws"]), arg["ws_bytes"], arg["W"], arg["eos"], arg["max_new"],
        *[_p(base, arg[k]) for k in _STATE + _REPORTS], None)


def test_beam_entry_point_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _call(_native, bad)) for bad, want in _REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 100 and not wrong, wrong
    passed = [(bad, _call(_native, dict(bad, K=48, ldx=1024))) for bad in _NOT_REFUSED]
    assert all(rc == _UNSUPPORTED for _, rc in passed), passed


_MERGE_REFUSED = (
    [({p: None}, _BADARG) for p in ("cand_idx", "cand_score") + _STATE]
    + [({p: off}, _BADARG) for p in ("token", "parent") for off in (2, 4, 12)]
    + [({p: off}, _BADARG) for p in ("cand_idx", "cand_score") + _STATE[:4] + _STATE[6:] for off in (1, 2)]
    + [({"S": n}, _BADARG) for n in (0, -1)] + [({"W": n}, _BADARG) for n in (0, -3)]
    + [({"kc": n}, _BADARG) for n in (0, -1, 9, 64)] + [({"eos": -1}, _BADARG)] + [({"max_new": n}, _BADARG) for n in (0, -7)]
    + [({"W": 33, "kc": 66}, _UNSUPPORTED), ({"W": 40, "kc": 1}, _UNSUPPORTED), ({"S": 17}, _UNSUPPORTED), ({"S": 65, "W": 1, "kc": 2}, _UNSUPPORTED)]
    + [(dict(bad, S=17), _BADARG) for bad in ({"kc": 9}, {"t": None}, {"eos": -1})]
)


def _call_merge(nv, bad):
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 15) & ~15
    arg = dict(S=2, W=4, kc=8, cand_idx=0, cand_score=4, eos=2, max_new=12, score=80, t=84, nfin=88, done=92, token=96,
               parent=104, hist_tok=112, hist_par=116, fin_score=120, fin_len=124, fin_beam=128)
    arg.update(bad)
    return nv.lib().ea_beam_merge(arg["S"], arg["W"], arg["kc"], _p(base, arg["cand_idx"]), _p(base, arg["cand_score"]),
                                  arg["eos"], arg["max_new"], *[_p(base, arg[k]) for k in _STATE], None)


def test_merge_entry_point_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _call_merge(_native, bad)) for bad, want in _MERGE_REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 50 and not wrong, wrong


# ---- the host reference against hand-worked answers -------------------------------------------------------------------------------
EOS = 9


def known_cases():
    """(name, arguments of ref.merge, the expected result's fields, the events that must occur).  Worked by hand from the
    rule in include/ea_hip.h."""
    f = lambda *v: np.array(v, dtype=F32)                                # noqa: E731
    return [
        # W = 2, k' = 4: sorted -1 (f0, eos: finishes), -2 (f1) = -2 (f4): the lower flat index first, -2.5 (f5, eos at i = 3 >= W)
        ("finish_tie_late", dict(cand_idx=[[EOS, 3, 4, 5], [6, EOS, 7, 8]], cand_score=[f(-1, -2, -3, -4), f(-2, -2.5, -5, -6)],
                                 kc=4, W=2, eos=EOS, t=3, nfin=0, done=0, forced=False),
         dict(token=[3, 6], parent=[0, 1], score=[-2.0, -2.0], records=[(-1.0, 4, 0)], t=4, nfin=1, done=0),
         {"eos_finished", "tie", "eos_late"}),
        # W = 2, k' = 2: NaN first (f0 goes on), then three -inf eos in flat order: i = 1 is dropped for its score, i = 2, 3 for
        # their place; one beam is left to fill
        ("nan_inf_dead", dict(cand_idx=[[5, EOS], [EOS, EOS]], cand_score=[f(NAN, -INF), f(-INF, -INF)], kc=2, W=2, eos=EOS,
                              t=0, nfin=0, done=0, forced=False),
         dict(token=[5, EOS], parent=[0, 1], score=[NAN, -INF], records=[], t=1, nfin=0, done=0),
         {"nan_first", "eos_inf", "eos_late", "tie", "dead_beam"}),
        # W = 2 with one hypothesis finished: the eos at i = 0 is the second: the sentence goes idle before max_new
        ("goes_idle", dict(cand_idx=[[EOS, 1], [2, 3]], cand_score=[f(-0.5, -0.75), f(-1, -2)], kc=2, W=2, eos=EOS, t=2, nfin=1,
                           done=0, forced=False),
         dict(token=[1, 2], parent=[0, 1], score=[-0.75, -1.0], records=[(-0.5, 3, 0)], t=3, nfin=2, done=1), {"eos_finished", "went_idle"}),
        # .. and a done sentence: eos, its own rows, nothing else moves
        ("idle", dict(cand_idx=[[1, 2], [3, 4]], cand_score=[f(0, -1), f(-2, -3)], kc=2, W=2, eos=EOS, t=3, nfin=2, done=1,
                      forced=False),
         dict(token=[EOS, EOS], parent=[0, 1], score=None, records=[], t=3, nfin=2, done=1), {"idle"}),
        # W = 3, forced, nfin = 1: column 0 alone (k' = 1): -1 (beam 1) and -3 (beam 0) finish, W - nfin = 2 of them; -inf is dropped
        ("forced", dict(cand_idx=[[EOS, 1, 1, 1, 1, 1], [EOS, 2, 2, 2, 2, 2], [EOS, 3, 3, 3, 3, 3]],
                        cand_score=[f(-3, 0, 0, 0, 0, 0), f(-1, 0, 0, 0, 0, 0), f(-INF, 0, 0, 0, 0, 0)], kc=6, W=3, eos=EOS, t=6,
                        nfin=1, done=0, forced=True),
         dict(token=[EOS] * 3, parent=[0, 1, 2], score=[-INF] * 3, records=[(-1.0, 7, 1), (-3.0, 7, 0)], t=7, nfin=3, done=1),
         {"forced", "forced_finished", "eos_inf", "dead_beam", "eos_finished"}),
        # W = 2, nfin = 1, two eos among the first W: the second finds no slot
        ("full", dict(cand_idx=[[EOS, 4], [EOS, 5]], cand_score=[f(-1, -3), f(-2, -4)], kc=2, W=2, eos=EOS, t=1, nfin=1, done=0,
                      forced=False),
         dict(token=[4, 5], parent=[0, 1], score=[-3.0, -4.0], records=[(-1.0, 2, 0)], t=2, nfin=2, done=1),
         {"eos_finished", "eos_full", "went_idle"}),
        # +0 and -0 are equal: the flat index decides (f1 = -0 of beam 0 before f2 = +0 of beam 1)
        ("zeros", dict(cand_idx=[[1, 2], [3, 4]], cand_score=[f(-1, -0.0), f(0.0, -2)], kc=2, W=2, eos=EOS, t=0, nfin=0, done=0,
                       forced=False),
         dict(token=[2, 3], parent=[0, 1], score=[-0.0, 0.0], records=[], t=1, nfin=0, done=0), {"tie"}),
    ]


def _check_known(got, want):
    for key in ("token", "parent", "t", "nfin", "done"):
        assert got[key] == want[key], (key, got[key], want[key])
    if want["score"] is None:
        assert got["score"] is None and got["hist_tok"] is None and got["hist_par"] is None
    else:
        assert np.array_equal(got["score"].view(np.int32), np.array(want["score"], dtype=F32).view(np.int32))  # (-0 is not +0)
        assert got["hist_tok"] == want["token"] and got["hist_par"] == want["parent"]
    assert [(float(s), n, b) for s, n, b in got["records"]] == want["records"]


def test_the_host_merge_against_hand_worked_answers():
    seen = set()
    for name, arg, want, events in known_cases():
        got = ref.merge(**arg)
        _check_known(got, want)
        assert events <= got["events"], (name, events, got["events"])
        seen |= got["events"]
    # every event the rule names occurred
    assert {"eos_finished", "eos_late", "eos_inf", "tie", "went_idle", "idle", "forced_finished", "dead_beam", "nan_first"} <= seen


def test_row_candidates_and_the_two_operations():
    row = np.array([1.0, NAN, 3.0, -0.0, 3.0, INF, 0.0, -INF], dtype=F32)
    idx, val, cand = ref.row_candidates(row, F32(0.25), F32(-1.5), 2, 6, False)
    assert idx.tolist() == [1, 5, 2, 4] and idx.dtype == np.int32 and cand.dtype == F32
    assert np.isnan(val[0]) and val[1:].tolist() == [INF, 3.0, 3.0]
    assert np.isnan(cand[0]) and cand[1:].tolist() == [INF, 1.25, 1.25]
    idx, val, cand = ref.row_candidates(row, F32(0.25), F32(-1.5), 8, 6, False)
    assert idx.tolist() == [1, 5, 2, 4, 0, 3, 6, 7]                     # k' = min(2 W, V)
    idx, val, cand = ref.row_candidates(row, F32(0.25), F32(-1.5), 2, 6, True)
    assert idx.tolist() == [6] and val.tolist() == [0.0] and cand.tolist() == [-1.75]
    # the subtraction first: score + (val - lse), not (score + val) - lse
    s, v, l = F32(1.0), F32(2.0 ** -24), F32(-(2.0 ** -24))
    _, _, cand = ref.row_candidates(np.array([v], dtype=F32), l, s, 1, 0, False)
    assert cand[0] == F32(s + F32(v - l)) and cand[0] != F32(F32(s + v) - l)
    assert ref.row_candidates(np.array([1.0, 2.0], dtype=F32), F32(0.0), F32(-INF), 1, 0, False)[2].tolist() == [-INF, -INF]   # (a dead beam)


def test_backtrack_finish_and_the_host_search():
    hist_tok, hist_par = [[4, 5], [6, 7], [8, 3]], [[0, 0], [1, 0], [1, 1]]
    assert ref.backtrack(hist_tok, hist_par, 4, 0, EOS) == [4, 7, 8, EOS]      # beam 0 at step 2 <- 1 at step 1 <- 0 at step 0
    assert ref.backtrack(hist_tok, hist_par, 3, 0, EOS) == [5, 6, EOS] and ref.backtrack(hist_tok, hist_par, 1, 1, EOS) == [EOS]
    out = ref.finish([(F32(-2.0), 4, 0), (F32(-1.0), 1, 1), (F32(-2.0), 4, 1), (F32(NAN), 2, 0)], 1.0)
    assert [(h["beam"], h["len"]) for h in out] == [(0, 2), (0, 4), (1, 4), (1, 1)]   # NaN, -0.5 twice in finishing order, -1
    assert [h["beam"] for h in ref.finish([(F32(-2.0), 4, 0), (F32(-1.0), 1, 1)], 0.0)] == [1, 0]

    # a three-token model whose logits do not depend on the history: V = 3, eos = 2, log-probabilities log(.5, .3, .2)
    logp = np.log(np.array([0.5, 0.3, 0.2])).astype(F32)
    fed = []

    def step_fn(tokens, parent):
        fed.append((tokens, parent))
        return np.tile(logp, (2, 1)), np.zeros(2, dtype=F32)
    hyps, info = ref.host_beam_search(step_fn, 1, 2, 2, 3)
    # step 0: beam 0 alone: 0 (-.69), 1 (-1.20) go on, eos at i = 2 is late.  step 1: 00 (-1.39), 01 (-1.90) | 10 (-1.90), 02
    # (-2.30): eos, late.  step 2, forced: 00 eos, 01 eos
    assert fed[0] == (None, None) and fed[1][0].tolist() == [0, 1] and fed[1][1].tolist() == [0, 0]
    assert info["steps"] == 3 and {"eos_late", "forced_finished"} <= info["events"]
    assert [h["tokens"] for h in hyps[0]] == [[0, 0, 2], [0, 1, 2]]
    assert hyps[0][0]["raw"] == F32(F32(logp[0] + logp[0]) + logp[2]) and hyps[0][0]["len"] == 3


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def _stack():
    from ea_harness.sequence import DecoderStack
    return DecoderStack(50, 128, 256, 2, 2, ATTN).eval()


def _held_state(B=12, V=50, C=128):
    """A DecodingState as hold_vocab leaves it, on the CPU (init_beam_search and the byte count need no device)."""
    from ea_harness import sequence as sq
    return sq.DecodingState({}, None, {"batch_size": B, "dtype": torch.bfloat16},
                            (torch.zeros(V, C, dtype=torch.bfloat16), torch.zeros(8 * 64 * 4, dtype=torch.uint8)))


def test_interface_of_the_beam_search():
    from ea_harness import sequence as sq
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    assert names(sq.DecoderStack.init_beam_search) == ["self", "state", "beam_size", "eos_idx", "max_new", "len_penalty"]
    assert inspect.signature(sq.DecoderStack.init_beam_search).parameters["len_penalty"].default == 1.0
    assert names(sq.DecoderStack.reset_beam_search) == ["self", "state"]
    assert names(sq.DecoderStack.beam_step) == ["self", "rows", "state", "out", "return_details"]
    assert names(sq.DecoderStack.beam_search) == ["self", "prompt", "state", "beam_size", "eos_idx", "max_new", "len_penalty",
                                                  "graph", "poll"]
    par = inspect.signature(sq.DecoderStack.beam_search).parameters
    assert par["state"].default is None and par["graph"].default is True and par["poll"].default == 16
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("beam_size", "eos_idx", "max_new", "len_penalty", "graph", "poll"))
    st = sq.DecodingState({}, None, {})
    assert st.beam is None and st.sampler is None and "beam" not in vars(st)   # (the attributes of a state are what they were)
    assert names(sq.DecodingState.__init__) == ["self", "incremental", "ffn", "options", "vocab"]


def test_init_beam_search_needs_the_table_and_no_sampler():
    from ea_harness import sequence as sq
    stack = _stack()
    with pytest.raises(RuntimeError, match=r"hold_vocab=True"):
        stack.init_beam_search(sq.DecodingState({}, None, {"batch_size": 4}), 2, 3, 8)
    st = _held_state()
    stack.init_sampling(st, 1, 8)
    with pytest.raises(RuntimeError, match=r"sampler"):
        stack.init_beam_search(st, 2, 3, 8)
    assert st.beam is None
    with pytest.raises(RuntimeError, match=r"init_beam_search"):
        stack.beam_step(torch.zeros(1, 12, 128), _held_state())
    with pytest.raises(RuntimeError, match=r"init_beam_search"):
        stack.reset_beam_search(_held_state())


@pytest.mark.parametrize("bad, message", [
    (dict(beam_size=0), "beam_size"), (dict(beam_size=33), "beam_size"), (dict(beam_size=-1), "beam_size"),
    (dict(beam_size=5), "batch size"), (dict(beam_size=8), "batch size"), (dict(B=66, beam_size=2), "batch size"),
    (dict(B=128, beam_size=32), "batch size"), (dict(eos_idx=-1), "eos_idx"), (dict(eos_idx=50), "eos_idx"),
    (dict(max_new=0), "max_new"), (dict(max_new=-3), "max_new"), (dict(len_penalty=float("nan")), "len_penalty")], ids=str)
def test_values_outside_the_envelope_raise_before_anything_is_allocated(bad, message, monkeypatch):
    bad = dict(bad)
    stack, st = _stack(), _held_state(bad.pop("B", 12))
    arg = dict(beam_size=4, eos_idx=3, max_new=8, len_penalty=1.0)
    arg.update(bad)

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the check")
    for name in ("empty", "zeros", "full", "arange"):
        monkeypatch.setattr(torch, name, no_alloc)
    with pytest.raises(ValueError, match=message):
        stack.init_beam_search(st, **arg)
    assert st.beam is None


def test_the_beam_and_its_bytes():
    from efficient_attention import _native
    stack = _stack()
    M, V, W, max_new = 12, 50, 4, 7
    S = M // W
    st = _held_state(M, V)
    before = stack.decoding_state_nbytes(st)
    assert stack.init_beam_search(st, W, 3, max_new, 0.5) is st
    bm = st.beam
    assert (bm.beam_size, bm.eos_idx, bm.max_new, bm.len_penalty) == (W, 3, max_new, 0.5)
    ws = _native.lib().ea_ceva_sdecode_vocab_beam_ws(M, V, W)
    assert ws == _ws_formula(M, V, W) == bm.ws.numel() and bm.ws.dtype == torch.uint8
    # the documented bytes
    assert "4 M V (logits) + ea_ceva_sdecode_vocab_beam_ws(M, V, W)" in stack.decoding_state_nbytes.__doc__
    assert stack.decoding_state_nbytes(st) - before == 4 * M * V + ws + 4 * M + 12 * S + 8 * M + 8 * max_new * M + 12 * S * W
    assert bm.logits.dtype == torch.float32 and tuple(bm.logits.shape) == (M, V)
    assert bm.score.tolist() == [0.0, -INF, -INF, -INF] * S and bm.score.dtype == torch.float32
    for t in (bm.t, bm.nfin, bm.done):
        assert t.dtype == torch.int32 and t.tolist() == [0] * S
    assert bm.parent.dtype == torch.long and tuple(bm.parent.shape) == (M,)
    assert tuple(bm.hist_tok.shape) == tuple(bm.hist_par.shape) == (max_new, M) and bm.hist_tok.dtype == bm.hist_par.dtype == torch.int32
    assert tuple(bm.fin_score.shape) == tuple(bm.fin_len.shape) == tuple(bm.fin_beam.shape) == (S, W)
    # reset: in place
    ptrs = [t.data_ptr() for t in bm.buffers()]
    bm.score.fill_(3.0), bm.t.fill_(2), bm.done.fill_(1), bm.hist_tok.fill_(5), bm.fin_len.fill_(4)
    assert stack.reset_beam_search(st) is st and [t.data_ptr() for t in bm.buffers()] == ptrs
    assert bm.score.tolist() == [0.0, -INF, -INF, -INF] * S and not bm.t.any() and not bm.done.any()
    assert not bm.hist_tok.any() and not bm.fin_len.any()
    for bad in (torch.zeros(2, 12, 128), torch.zeros(1, 4, 128)):        # one step of the whole state
        with pytest.raises(ValueError, match="single-token step"):
            stack.beam_step(bad, st)
    with pytest.raises(ValueError, match="channels"):
        stack.beam_step(torch.zeros(1, 12, 64), st)
