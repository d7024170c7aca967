"""-m "not gpu": the constrained beam step (C ABI 36: ea_beam_bans, ea_ceva_sdecode_vocab_beam_c, ea_adaptive_beam_c) and
DecoderStack.init_beam_constraints / set_beam_prompt / constrained_beam_search: the host reference against fairseq's recorded
masks and hand-worked answers, the header, the binding, the workspace queries, what the entries refuse, the host methods'
argument checks.  The kernels: tests/test_gpu_decoder_constraints.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
import decoder_constraint_reference as cref
import test_decoder_beam_cpu as tb

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
BANS, BEAM_C, BEAM_C_WS = "ea_beam_bans", "ea_ceva_sdecode_vocab_beam_c", "ea_ceva_sdecode_vocab_beam_c_ws"
ADP_C, ADP_C_WS = "ea_adaptive_beam_c", "ea_adaptive_beam_c_ws"
_BADARG, _UNSUPPORTED = -1, -2


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_banned_equals_the_recorded_masks_of_the_reference():
    z = np.load(os.path.join(HERE, "golden", "ngram_block.npz"))
    meta = z["meta"]
    assert len(meta) >= 24
    signs, total = set(), 0
    for i, (rows, step, n, vocab) in enumerate(meta.tolist()):
        tokens, mask = z["tokens%d" % i], z["mask%d" % i]
        assert tokens.shape == (rows, step + 1) and mask.shape == (rows, vocab) and 12 <= vocab <= 40 and 1 <= n <= 4
        signs.add(int(np.sign(step + 2 - n)))
        for r in range(rows):
            got = cref.banned(tokens[r].tolist(), step, n, 0, -1, ())
            assert got == set(np.nonzero(mask[r])[0].tolist()), (i, r, step, n)
            assert np.array_equal(np.isinf(cref.apply(np.zeros(vocab, dtype=F32), got)), mask[r])
            total += len(got)
    assert signs == {-1, 0, 1} and total > 100


def test_banned_on_hand_worked_cases():
    b = cref.banned
    # n = 1: every token of x
    assert b([5, 3, 5, 7], 4, 1, 0, 0, ()) == {3, 5, 7} and b([], 0, 1, 0, 0, ()) == set()
    # n = 3: L = n - 2 and L = n - 1 have no window to compare (i runs over 0 .. L - n); L = n holds the first one
    assert b([4], 1, 3, 0, 0, ()) == set() and b([4, 4], 2, 3, 0, 0, ()) == set()
    assert b([4, 4, 9], 3, 3, 0, 0, ()) == set()                  # window (4, 4) against the suffix (4, 9)
    assert b([4, 4, 4], 3, 3, 0, 0, ()) == {4}                    # window (4, 4) equals the suffix: its continuation
    assert b([6, 2], 2, 2, 0, 0, ()) == set() and b([2, 6, 2], 3, 2, 0, 0, ()) == {6}
    # a suffix that occurs three times, with three continuations (the last occurrence is the suffix itself)
    x = [1, 2, 7, 0, 1, 2, 8, 1, 2, 9, 3, 1, 2]
    assert b(x, len(x), 3, 0, 0, ()) == {7, 8, 9}
    assert b(x, len(x), 2, 0, 0, ()) == {7, 8, 9} and b(x, len(x), 4, 0, 0, ()) == set()
    # the prompt counts: the caller hands prompt ++ generated; t counts the generated tokens alone
    assert b([1, 2, 7] + [1, 2], 2, 3, 0, 0, ()) == {7}
    # min_len: eos is banned at t = min_len - 1 and free at t = min_len
    assert b([3], 2, 0, 3, 11, ()) == {11} and b([3], 3, 0, 3, 11, ()) == set()
    assert b([], 0, 0, 0, 11, ()) == set() and b([], 0, 0, 1, 11, ()) == {11}
    # static bans come on top
    assert b([2, 6, 2], 3, 2, 4, 11, (1, 30)) == {6, 11, 1, 30}


def test_apply_and_row_candidates_c():
    row = np.array([0.5, 3.0, -1.0, 3.0, 2.0, np.nan, 0.0], dtype=F32)
    got = cref.apply(row, {1, 5, 99, -3})
    assert got[1] == -np.inf and got[5] == -np.inf and np.array_equal(got[[0, 2, 3, 4, 6]], row[[0, 2, 3, 4, 6]])
    assert np.isnan(row[5])                                       # (the caller's row is not written)
    lse, score = F32(4.0), F32(-1.0)
    idx, val, cand = cref.row_candidates_c(row, lse, score, 2, 6, False, {1, 5})
    assert idx.tolist() == [3, 4, 0, 6] and val.tolist() == [3.0, 2.0, 0.5, 0.0]
    assert np.array_equal(cand, (score + (val - lse)).astype(F32))
    # fewer than k' unbanned: the banned ones follow at -inf, the lower index first
    idx, val, cand = cref.row_candidates_c(row, lse, score, 3, 6, False, {0, 1, 2, 5, 6})
    assert idx.tolist() == [3, 4, 0, 1, 2, 5] and (cand[2:] == -np.inf).all()
    # the forced step ignores the set
    idx, val, cand = cref.row_candidates_c(row, lse, score, 2, 1, True, {1})
    assert idx.tolist() == [1] and val.tolist() == [3.0]


def test_beam_tokens_follow_the_parents():
    hist_tok = [[5, 6, 7], [8, 9, 10], [11, 12, 13]]
    hist_par = [[0, 1, 2], [2, 0, 0], [1, 1, 0]]
    assert cref.beam_tokens(hist_tok, hist_par, 0, 3) == [[], [], []]
    assert cref.beam_tokens(hist_tok, hist_par, 2, 3) == [[7, 8], [5, 9], [5, 10]]
    assert cref.beam_tokens(hist_tok, hist_par, 3, 3) == [[5, 9, 11], [5, 9, 12], [7, 8, 13]]


def test_the_constrained_host_search_keeps_its_promises_where_the_plain_one_breaks_them():
    """A model that loves token 4 and, behind it, eos: unconstrained it ends at once; constrained it must go on, may not repeat
    a bigram and never picks token 1."""
    V, W, eos, max_new = 9, 2, 0, 8
    base = np.array([2.0, 1.5, 0.1, 0.2, 3.0, 0.3, 0.4, 0.0, -1.0], dtype=F32)

    def step_fn(tokens, parent):
        logits = np.tile(base, (W, 1))
        lse = np.log(np.exp(logits.astype(np.float64)).sum(1)).astype(F32)
        return logits, lse
    plain, _ = cref.host_beam_search_c(step_fn, 1, W, eos, max_new)
    assert any(cref.violations([4, 1], h["tokens"], eos, max_new, 2, 3, (1,)) for h in plain[0])
    hyps, info = cref.host_beam_search_c(step_fn, 1, W, eos, max_new, prompts=[[4, 1]], n=2, min_len=3, ban_tokens=(1,))
    assert hyps[0] and all(not cref.violations([4, 1], h["tokens"], eos, max_new, 2, 3, (1,)) for h in hyps[0])
    assert all(len(h["tokens"]) - 1 >= 3 for h in hyps[0])
    assert any(bset for _, _, _, bset in info["bans"])


# ---- C ABI 36 -----------------------------------------------------------------------------------------------------------------------
def test_abi_36_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 36
    for name in (BANS, BEAM_C, BEAM_C_WS, ADP_C, ADP_C_WS):
        assert hasattr(lib, name) and name in _native.SIGNATURES and name in declared_symbols(), name
    I, L, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    tail = [I, I, P, I, P, I, P, P, P]                                # min_len .. gen, stream
    assert _native.SIGNATURES[BEAM_C] == _native.SIGNATURES["ea_ceva_sdecode_vocab_beam"][:-1] + tail
    assert _native.SIGNATURES[ADP_C] == _native.SIGNATURES["ea_adaptive_beam"][:-1] + tail
    assert _native.SIGNATURES[BEAM_C_WS] == [I] * 5 and _native.SIGNATURES[ADP_C_WS] == [I, I, P, P, I, I, I]
    assert len(_native.SIGNATURES[BANS]) == 20
    assert _native.lib().ea_ceva_sdecode_vocab_beam_c_ws.restype is ctypes.c_int64
    assert _native.lib().ea_adaptive_beam_c_ws.restype is ctypes.c_int64
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    text = open(HEADER).read()
    for phrase in ("ABI 36", "THE FORCED STEP IGNORES EVERY CONSTRAINT", "prompt_cap + max_new + 17", "UNCONSTRAINED logits"):
        assert phrase in text, phrase


def _ban_bytes(M, prompt_cap, max_new):
    return tb._r16(4 * M * (prompt_cap + max_new + 17)) + tb._r16(4 * M)


def test_the_workspace_queries():
    from efficient_attention import _native as nv
    ws, ws0 = nv.lib().ea_ceva_sdecode_vocab_beam_c_ws, nv.lib().ea_ceva_sdecode_vocab_beam_ws
    for M, V, W, pc, mn in ((1, 17, 1, 0, 1), (8, 50, 4, 5, 12), (64, 333, 32, 512, 128), (12, 1000, 4, 0, 7)):
        assert ws(M, V, W, pc, mn) == ws0(M, V, W) + _ban_bytes(M, pc, mn) > 0, (M, V, W, pc, mn)
    for bad in ((0, 50, 1, 0, 4), (65, 50, 1, 0, 4), (8, 0, 4, 0, 4), (8, 50, 3, 0, 4), (8, 50, 33, 0, 4), (8, 50, 4, -1, 4),
                (8, 50, 4, 0, 0), (8, 50, 4, 0, -2), (8, 50, 4, 2 ** 31 - 8, 100)):
        assert ws(*bad) < 0, bad
    cut, dims = nv.host_array(ctypes.c_int64, [96, 200, 333]), nv.host_array(ctypes.c_int32, [64, 32])
    aws, aws0 = nv.lib().ea_adaptive_beam_c_ws, nv.lib().ea_adaptive_beam_ws
    assert aws(8, 2, cut, dims, 4, 5, 12) == aws0(8, 2, cut, dims, 4) + _ban_bytes(8, 5, 12) > 0
    for bad in ((8, 2, cut, dims, 4, -1, 12), (8, 2, cut, dims, 4, 5, 0), (8, 2, cut, dims, 3, 5, 12), (8, 2, cut, dims, 0, 5, 12),
                (65, 2, cut, dims, 1, 5, 12)):
        assert aws(*bad) < 0, bad[0:1] + bad[4:]


_STATE, _REPORTS = tb._STATE, tb._REPORTS
_C_WS = None


def _call_c(nv, bad):
    """ea_ceva_sdecode_vocab_beam_c on addresses that are never dereferenced: a refused call returns before any HIP call."""
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 15) & ~15
    arg = dict(M=8, K=256, V=1000, x=0, x_dtype=0, ldx=256, w=16, w_dtype=0, logits=32, ldl=1000, ws=64,
               ws_bytes=nv.lib().ea_ceva_sdecode_vocab_beam_c_ws(8, 1000, 4, 6, 12), W=4, eos=2, max_new=12, score=80, t=84, nfin=88,
               done=92, token=96, parent=104, hist_tok=112, hist_par=116, fin_score=120, fin_len=124, fin_beam=128, cand_idx=132,
               cand_score=136, lse=140, sel_val=144, min_len=3, ngram=2, ban_tokens=[1, 7], prompt_tok=148, prompt_cap=6,
               prompt_len=152, gen=156)
    arg.update(bad)
    bans = arg["ban_tokens"]
    n_ban = arg.get("n_ban_tokens", 0 if bans is None else len(bans))
    arr = None if bans is None else nv.host_array(ctypes.c_int32, bans + [0])
    return nv.lib().ea_ceva_sdecode_vocab_beam_c(
        arg["M"], arg["K"], arg["V"], tb._p(base, arg["x"]), arg["x_dtype"], arg["ldx"], tb._p(base, arg["w"]), arg["w_dtype"],
        tb._p(base, arg["logits"]), arg["ldl"], tb._p(base, arg["ws"]), arg["ws_bytes"], arg["W"], arg["eos"], arg["max_new"],
        *[tb._p(base, arg[k]) for k in _STATE + _REPORTS], arg["min_len"], arg["ngram"], arr, n_ban, tb._p(base, arg["prompt_tok"]),
        arg["prompt_cap"], tb._p(base, arg["prompt_len"]), tb._p(base, arg["gen"]), None)


_C_REFUSED = (
    [({"min_len": n}, _BADARG) for n in (-1, 12, 13, 100)] + [({"ngram": n}, _BADARG) for n in (-1, 17, 64)]
    + [({"ban_tokens": list(range(3, 20))}, _BADARG), ({"ban_tokens": [2]}, _BADARG), ({"ban_tokens": [5, 2]}, _BADARG),
       ({"ban_tokens": [-1]}, _BADARG), ({"ban_tokens": [1000]}, _BADARG), ({"ban_tokens": None, "n_ban_tokens": 2}, _BADARG),
       ({"n_ban_tokens": -1}, _BADARG), ({"n_ban_tokens": 17}, _BADARG)]
    + [({"prompt_cap": -1}, _BADARG), ({"prompt_tok": None}, _BADARG), ({"prompt_len": None}, _BADARG), ({"gen": None}, _BADARG)]
    + [({p: off}, _BADARG) for p in ("prompt_tok", "prompt_len", "gen") for off in (149, 150)]
    + [({"ws_bytes": tb._WS_8_1000_4}, _BADARG), ({"score": None}, _BADARG), ({"eos": 1000}, _BADARG), ({"max_new": 0}, _BADARG)]
    + [({"W": 33, "ws_bytes": 1 << 40}, _UNSUPPORTED), ({"K": 48, "ldx": 1024}, _UNSUPPORTED), ({"W": 3, "ws_bytes": 1 << 40}, _UNSUPPORTED)]
    # a bad argument is decided before the geometry
    + [(dict(bad, W=33, K=48, ldx=1024), _BADARG) for bad in ({"min_len": 12}, {"ngram": 17}, {"ban_tokens": [2]}, {"gen": None})]
)
_C_NOT_REFUSED = [{}, {"min_len": 0}, {"min_len": 11}, {"ngram": 0}, {"ngram": 16}, {"ban_tokens": None}, {"ban_tokens": list(range(3, 19))},
                  {"prompt_cap": 0, "prompt_tok": None, "prompt_len": None, "ws_bytes": 1 << 40}, {"ban_tokens": [999, 0]}]


def test_the_constrained_entry_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _call_c(_native, bad)) for bad, want in _C_REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 35 and not wrong, wrong
    passed = [(bad, _call_c(_native, dict(bad, K=48, ldx=1024))) for bad in _C_NOT_REFUSED]
    assert all(rc == _UNSUPPORTED for _, rc in passed), passed


def _call_bans(nv, bad):
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 15) & ~15
    arg = dict(S=2, W=4, eos=2, max_new=12, min_len=3, ngram=2, ban_tokens=[1, 7], prompt_tok=0, prompt_cap=6, prompt_len=4, t=8,
               done=12, hist_tok=16, hist_par=20, gen=24, ban=28, cap=6 + 12 + 17, nban=32)
    arg.update(bad)
    bans = arg["ban_tokens"]
    arr = None if bans is None else nv.host_array(ctypes.c_int32, bans + [0])
    p = lambda k: tb._p(base, arg[k])                                  # noqa: E731
    return nv.lib().ea_beam_bans(arg["S"], arg["W"], arg["eos"], arg["max_new"], arg["min_len"], arg["ngram"], arr,
                                 0 if bans is None else len(bans), p("prompt_tok"), arg["prompt_cap"], p("prompt_len"), p("t"),
                                 p("done"), p("hist_tok"), p("hist_par"), p("gen"), p("ban"), arg["cap"], p("nban"), None)


def test_the_ban_list_entry_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native as nv
    refused = ([({k: None}, _BADARG) for k in ("t", "done", "hist_tok", "hist_par", "gen", "ban", "nban", "prompt_tok", "prompt_len")]
               + [({k: 2}, _BADARG) for k in ("t", "gen", "ban", "nban", "prompt_tok")]
               + [({"S": 0}, _BADARG), ({"W": 0}, _BADARG), ({"eos": -1}, _BADARG), ({"max_new": 0}, _BADARG), ({"min_len": 12}, _BADARG),
                  ({"min_len": -1}, _BADARG), ({"ngram": 17}, _BADARG), ({"ban_tokens": [2]}, _BADARG), ({"ban_tokens": [-4]}, _BADARG),
                  ({"ban_tokens": list(range(3, 20))}, _BADARG), ({"cap": 34}, _BADARG), ({"prompt_cap": -1}, _BADARG),
                  ({"W": 33, "S": 1}, _UNSUPPORTED), ({"S": 17}, _UNSUPPORTED), ({"S": 17, "ngram": 17}, _BADARG)])
    got = [(bad, want, _call_bans(nv, bad)) for bad, want in refused]
    wrong = [row for row in got if row[1] != row[2]]
    assert not wrong, wrong


# ---- the host methods -------------------------------------------------------------------------------------------------------------
def test_interface_of_the_constraints():
    from ea_harness import sequence as sq, token_pick as tp
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    assert names(sq.DecoderStack.init_beam_constraints) == ["self", "state", "min_len", "no_repeat_ngram_size", "ban_tokens", "prompt_cap"]
    par = inspect.signature(sq.DecoderStack.init_beam_constraints).parameters
    assert [par[k].default for k in ("min_len", "no_repeat_ngram_size", "ban_tokens", "prompt_cap")] == [0, 0, (), 0]
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("min_len", "no_repeat_ngram_size", "ban_tokens", "prompt_cap"))
    assert names(sq.DecoderStack.set_beam_prompt) == ["self", "state", "prompt", "lengths"]
    assert names(sq.DecoderStack.constrained_beam_search) == names(sq.DecoderStack.beam_search) + ["min_len", "no_repeat_ngram_size",
                                                                                                  "ban_tokens"]
    assert tp.Beam(1, 0, 1, 1.0, *[None] * 12).constraint is None
    assert "not built" not in (sq.DecoderStack.beam_search.__doc__ + sq.DecoderStack.constrained_beam_search.__doc__).replace(
        "Not built: prefix tokens", "")


def _beam_state(M=12, V=50, W=4, eos=3, max_new=7):
    stack, st = tb._stack(), tb._held_state(M, V)
    stack.init_beam_search(st, W, eos, max_new, 0.5)
    return stack, st


@pytest.mark.parametrize("bad, message", [
    (dict(min_len=7), "min_len"), (dict(min_len=8), "min_len"), (dict(min_len=-1), "min_len"),
    (dict(no_repeat_ngram_size=17), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
    (dict(ban_tokens=tuple(range(4, 21))), "at most 16"), (dict(ban_tokens=(1, 3)), "eos_idx"), (dict(ban_tokens=(50,)), "ban_tokens"),
    (dict(ban_tokens=(-1,)), "ban_tokens"), (dict(prompt_cap=-1), "prompt_cap")], ids=str)
def test_constraints_outside_the_envelope_raise_before_anything_is_allocated(bad, message, monkeypatch):
    stack, st = _beam_state()
    ws = st.beam.ws

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the check")
    for name in ("empty", "zeros", "full", "arange"):
        monkeypatch.setattr(torch, name, no_alloc)
    with pytest.raises(ValueError, match=message):
        stack.init_beam_constraints(st, **bad)
    assert st.beam.constraint is None and st.beam.ws is ws


def test_the_constraint_its_bytes_the_prompt_and_reset():
    from efficient_attention import _native
    from ea_harness import sequence as sq
    M, V, W, max_new, pc = 12, 50, 4, 7, 5
    S = M // W
    stack, st = _beam_state(M, V, W, 3, max_new)
    with pytest.raises(RuntimeError, match="init_beam_search"):
        stack.init_beam_constraints(tb._held_state(M, V), min_len=2)
    with pytest.raises(RuntimeError, match="init_beam_constraints|prompt_cap"):
        stack.set_beam_prompt(st, torch.zeros(S, 2, dtype=torch.long))
    plain = stack.decoding_state_nbytes(st)
    ws0 = st.beam.ws
    # all defaults: nothing attached, the state is what it was
    assert stack.init_beam_constraints(st) is st and st.beam.constraint is None and st.beam.ws is ws0
    assert stack.init_beam_constraints(st, min_len=2, no_repeat_ngram_size=3, ban_tokens=[1, 9], prompt_cap=pc) is st
    c = st.beam.constraint
    assert c.scalars() == (2, 3, (1, 9)) and c.prompt_cap == pc
    assert tuple(c.gen.shape) == (2, M, max_new) and c.gen.dtype == torch.int32
    assert tuple(c.prompt_tok.shape) == (S, pc) and tuple(c.prompt_len.shape) == (S,) and c.prompt_len.dtype == torch.int32
    need = _native.lib().ea_ceva_sdecode_vocab_beam_c_ws(M, V, W, pc, max_new)
    assert st.beam.ws.numel() == need == ws0.numel() + _ban_bytes(M, pc, max_new)
    assert stack.decoding_state_nbytes(st) - plain == _ban_bytes(M, pc, max_new) + 4 * S * pc + 4 * S + 8 * M * max_new
    # the prompt
    prompt = torch.tensor([[4, 5, 6], [7, 8, 1], [9, 1, 1]])
    assert stack.set_beam_prompt(st, prompt) is st
    assert c.prompt_tok[:, :3].tolist() == prompt.tolist() and not c.prompt_tok[:, 3:].any() and c.prompt_len.tolist() == [3, 3, 3]
    stack.set_beam_prompt(st, prompt, torch.tensor([3, 2, 9]))
    assert c.prompt_len.tolist() == [3, 2, 3]                          # (clamped to P)
    with pytest.raises(ValueError, match="prompt_cap"):
        stack.set_beam_prompt(st, torch.zeros(S, pc + 1, dtype=torch.long))
    with pytest.raises(ValueError, match="prompt must be"):
        stack.set_beam_prompt(st, torch.zeros(S + 1, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="lengths"):
        stack.set_beam_prompt(st, prompt, torch.zeros(S + 1, dtype=torch.long))
    # reset clears the generated tokens and keeps the prompt, in place
    c.gen.fill_(5)
    ptrs = [t.data_ptr() for t in st.beam.buffers()]
    stack.reset_beam_search(st)
    assert not c.gen.any() and c.prompt_len.tolist() == [3, 2, 3] and [t.data_ptr() for t in st.beam.buffers()] == ptrs
    assert set(t.data_ptr() for t in c.tensors()) <= set(ptrs)
    # a search with other constraints on this state is refused before anything runs; so is a longer prompt
    for kw, message in ((dict(min_len=1), "min_len, no_repeat_ngram_size, ban_tokens"),
                        (dict(min_len=2, no_repeat_ngram_size=3, ban_tokens=(1, 9)), "prompt_cap")):
        with pytest.raises(ValueError, match=message):
            stack.constrained_beam_search(torch.zeros(S, pc + 1, dtype=torch.long), st, beam_size=W, eos_idx=3, max_new=max_new,
                                          len_penalty=0.5, **kw)
    # the constraint comes off again
    stack.init_beam_constraints(st)
    assert st.beam.constraint is None and st.beam.ws.numel() == ws0.numel() and stack.decoding_state_nbytes(st) == plain
    assert isinstance(st, sq.DecodingState)
