"""-m "not gpu": full-vocabulary and nucleus sampling on a held vocabulary table (ea_ceva_sdecode_vocab_sample_full, _logprob,
_ws) and DecoderStack.init_nucleus_sampling: the host reference against known answers, header and binding, what the entry
points refuse before any launch, the interface's errors, and the precondition of tests/test_gpu_decoder_nucleus.py's check 4
-- that at least 0.95 of the draws are decided uniquely under the bound it allows -- on host-side logits of its shapes."""
import ctypes

import numpy as np
import pytest
import torch

from test_cabi import declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
from test_decoder_sample_cpu import _held_state, _stack
import decoder_nucleus_reference as ref
import decoder_vocab_operands as ops

FULL, FULL_LOGPROB, WS = ("ea_ceva_sdecode_vocab_sample_full", "ea_ceva_sdecode_vocab_sample_full_logprob",
                          "ea_ceva_sdecode_vocab_sample_full_ws")


def test_the_reference_on_known_answers():
    row = np.zeros(1000, dtype=np.float32)                                   # the constant row: every q = 2^32
    assert ref.masses(row, 0.7).tolist() == [1 << 32] * 1000 and ref.order(row).tolist() == list(range(1000))
    assert (ref.target(0.5, 10), ref.target(0.3, 10), ref.target(1.0, 12345)) == (5, 4, 12345)      # (float32(0.3) > 0.3)
    assert [ref.nucleus(ref.masses(row, 1.0), ref.order(row), p) for p in (1.0, 0.9, 0.3, 1e-6)] == [1000, 900, 301, 1]
    row = np.array([0.0, np.log(2.0), -np.inf, np.log(2.0), -100.0], dtype=np.float32)
    q = ref.masses(row, 1.0)
    assert ref.order(row).tolist() == [1, 3, 0, 4, 2] and q[[1, 3, 2, 4]].tolist() == [1 << 32, 1 << 32, 0, 0]
    assert abs(int(q[0]) - (1 << 31)) <= 1 << 9                              # (log(2) rounded to fp32)
    assert [ref.nucleus(q, ref.order(row), p) for p in (0.3, 0.5, 0.7, 0.81, 1.0)] == [1, 2, 2, 3, 5]
    assert ref.masses(row, 0.5)[0] in range((1 << 30) - (1 << 9), (1 << 30) + (1 << 9))
    # r = ((2 U + 1) C) >> 25 < C, and 0 for U = 0 below C = 2^25
    assert ref.draw(0, 1 << 32) == 1 << 7 and ref.draw((1 << 24) - 1, 12345) == 12344 and ref.draw(0, (1 << 25) - 1) == 0
    assert ref.word(0, 0, 0) == 0x6627e8d5 >> 8 and ref.eps(1 << 19, 3) == 4.0


def test_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    I, L, P, F, U = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64
    head = [I, I, I, P, I, L, P, I, P, L, P, L, F, F, U, P, P, P, P, P, P, P]
    assert _native.SIGNATURES[FULL] == head + [P] and _native.SIGNATURES[FULL_LOGPROB] == head + [P, L, P, P, P]
    assert _native.SIGNATURES[WS] == [I, I] and _native.lib().ea_ceva_sdecode_vocab_sample_full_ws.restype is ctypes.c_int64
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert all(hasattr(lib, s) for s in (FULL, FULL_LOGPROB, WS)) and _native.lib().ea_abi_version() == 38
    ws, ws26 = _native.lib().ea_ceva_sdecode_vocab_sample_full_ws, _native.lib().ea_ceva_sdecode_vocab_ws
    for M, V in ((1, 1), (8, 1000), (64, 262144), (64, 1 << 24), (0, 16), (65, 16), (1, 0)):
        assert ws(M, V) == ws26(M, V) and (ws(M, V) > 0) == (1 <= M <= 64 and V >= 1)
    assert ws(1, (1 << 24) + 1) < 0


_BADARG, _UNSUPPORTED = -1, -2
_NAN, _INF = float("nan"), float("inf")
_WS, _LWS = 8 * 8 * 63, 4 * 8 * 63 + 4 * 8
_REFUSED = (
    [({p: None}, _BADARG) for p in ("x", "w", "ws", "token", "logits", "ctr", "sid")]
    + [({p: off}, _BADARG) for p in ("x", "w", "ws") for off in (4, 8)]
    + [({"token": 4}, _BADARG), ({"ctr": 4}, _BADARG), ({"mass": 4}, _BADARG), ({"logits": 34}, _BADARG)]
    + [({p: 2}, _BADARG) for p in ("sid", "kept", "thr_idx", "thr_val")]
    + [({"top_p": v}, _BADARG) for v in (0.0, -0.5, 1.0000001, _NAN, _INF)]
    + [({"temperature": v}, _BADARG) for v in (0.0, -1.0, _NAN, _INF)]
    + [({"ws_bytes": _WS - 1}, _BADARG), ({"ldl": 999}, _BADARG), ({"M": 0}, _BADARG)]
    + [({"M": 65, "ws_bytes": 1 << 40, "lws_bytes": 1 << 40}, _UNSUPPORTED), ({"K": 48, "ldx": 1024}, _UNSUPPORTED)]
    + [(dict(bad, M=65, K=48, ldx=1024), _BADARG) for bad in ({"top_p": 1.5}, {"temperature": _NAN}, {"ctr": None})]
)
_REFUSED_LOGPROB = [({p: None}, _BADARG) for p in ("lws", "lse", "logp")] + [({"lws": 8}, _BADARG), ({"lws_bytes": _LWS - 1}, _BADARG)]
_NOT_REFUSED = [{"top_p": 1.0}, {"top_p": 1e-6}, {"temperature": 100.0}, {"seed": (1 << 64) - 1},
                {"kept": None, "thr_idx": None, "thr_val": None, "mass": None}]


def _call(nv, bad, logprob):
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    arg = dict(M=8, K=256, V=1000, x=0, x_dtype=0, ldx=256, w=16, w_dtype=0, logits=32, ldl=1000, ws=64, ws_bytes=_WS, top_p=0.9,
               temperature=0.8, seed=5, ctr=80, sid=96, token=112, kept=128, thr_idx=132, thr_val=136, mass=144, lws=160,
               lws_bytes=_LWS, lse=176, logp=180)
    arg.update(bad)
    p = lambda k: None if arg[k] is None else ctypes.c_void_p(base + arg[k])    # noqa: E731
    tail = [p("lws"), arg["lws_bytes"], p("lse"), p("logp")] if logprob else []
    return getattr(nv.lib(), FULL_LOGPROB if logprob else FULL)(
        arg["M"], arg["K"], arg["V"], p("x"), arg["x_dtype"], arg["ldx"], p("w"), arg["w_dtype"], p("logits"), arg["ldl"], p("ws"),
        arg["ws_bytes"], arg["top_p"], arg["temperature"], arg["seed"], p("ctr"), p("sid"), p("token"), p("kept"), p("thr_idx"),
        p("thr_val"), p("mass"), *tail, None)


@pytest.mark.parametrize("logprob", [False, True])
def test_the_entry_points_refuse_before_any_launch(lib, logprob):  # noqa: F811
    from efficient_attention import _native
    cases = _REFUSED + (_REFUSED_LOGPROB if logprob else [])
    wrong = [(bad, want, got) for bad, want in cases for got in [_call(_native, bad, logprob)] if got != want]
    assert not wrong, wrong
    passed = [(bad, _call(_native, dict(bad, K=48, ldx=1024), logprob)) for bad in _NOT_REFUSED]   # (past every check but K % 32)
    assert all(rc == _UNSUPPORTED for _, rc in passed), passed


@pytest.mark.parametrize("bad", [dict(top_p=0.0), dict(top_p=1.5), dict(top_p=_NAN), dict(temperature=0.0), dict(temperature=_INF),
                                 dict(temperature=_NAN), dict(seed=-1), dict(seed=1 << 64)], ids=str)
def test_values_outside_the_envelope_raise_before_anything_is_allocated(bad, monkeypatch):
    stack, st = _stack(), _held_state()
    for name in ("empty", "zeros", "arange"):
        monkeypatch.setattr(torch, name, lambda *a, **k: pytest.fail("allocated before the check"))
    with pytest.raises(ValueError, match=next(iter(bad))):
        stack.init_nucleus_sampling(st, **dict(dict(seed=3, top_p=0.9, temperature=0.8), **bad))
    assert st.sampler is None


def test_the_sampler_it_attaches_and_the_states_it_refuses(lib):  # noqa: F811
    from ea_harness import sequence as sq
    from ea_harness import token_pick as tp
    stack, st = _stack(), _held_state()
    assert stack.init_nucleus_sampling(st, 11, 0.9, 0.8) is st
    sm = st.sampler
    assert (sm.seed, sm.top_k, sm.top_p, sm.temperature, sm.next_sid, sm.ws) == (11, 0, 0.9, 0.8, 3, None)
    assert tuple(sm.logits.shape) == (3, 50) and sm.ctr.tolist() == [0] * 3 and sm.sid.tolist() == [0, 1, 2]
    assert type(tp.select_pick(stack, st, 3)) is tp.HeldNucleus
    with pytest.raises(ValueError, match="top_k"):                          # (init_sampling keeps refusing the whole vocabulary)
        stack.init_sampling(_held_state(), 11, 0)
    with pytest.raises(RuntimeError, match="hold_vocab=True"):
        stack.init_nucleus_sampling(sq.DecodingState({}, None, {"batch_size": 2}), 1)
    adaptive = sq.DecodingState({}, None, {"batch_size": 2})
    adaptive.adaptive = object()
    with pytest.raises(NotImplementedError, match="adaptive"):
        stack.init_nucleus_sampling(adaptive, 1)


@pytest.mark.parametrize("shape", [(3, 64, 16), (17, 64, 64), (2, 128, 1000), (1, 64, 2048)], ids=str)
def test_nearly_every_draw_is_decided_uniquely_under_the_bound(shape):
    M, K, V = shape
    x32, w = ops.operands(shape, torch.bfloat16, 0)
    L = (x32.to(torch.bfloat16).float() @ w.float().t()).numpy()
    for temperature in (0.7, 1.0):
        for top_p in (1.0, 0.9, 0.3):
            one = 0
            for m in range(M):
                q, ordr = ref.masses(L[m], temperature), ref.order(L[m])
                Kept = np.sort(ordr[:ref.nucleus(q, ordr, top_p)])
                P = np.cumsum(q[Kept]).astype(np.float64)
                e = ref.eps(P[-1], Kept.size)
                lo = np.concatenate([[0.0], P[:-1]]) - e
                r = np.array([ref.draw(ref.word(5, i, m), int(P[-1])) for i in range(64)], dtype=np.float64).reshape(-1, 1)
                one += int((((lo <= r) & (r < P + e)).sum(1) == 1).sum())
            assert one >= 0.95 * 64 * M, (shape, temperature, top_p, one / (64 * M))
