"""-m "not gpu": sampling and the beam step from the adaptive head (csrc/ea_adaptive_pick.hip, C ABI 35: ea_adaptive_sample_ws,
ea_adaptive_sample, ea_adaptive_beam_ws, ea_adaptive_beam; DecoderStack.init_sampling / init_beam_search on a state with an
adaptive pick): the header, the binding table and the version, both workspace queries against the host restatement of the
documented layout (tests/adaptive_select_reference.py), every argument error's code without a device, the host reference of
the selection rule against hand-worked answers, and the stack's errors and attachments."""
import ctypes
import re

import numpy as np
import pytest
import torch

import adaptive_pick_reference as pref
import adaptive_select_reference as sel
from test_adaptive_cpu import ATTN
from test_cabi import HEADER, declared_symbols

NEW = {"ea_adaptive_sample_ws": 4, "ea_adaptive_sample": 26, "ea_adaptive_beam_ws": 5, "ea_adaptive_beam": 31}
F32 = np.float32


def test_s0_header_binding_and_version():
    from efficient_attention import _native
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counts = {m.group(1): m.group(2).count(",") + 1
              for m in re.finditer(r"\b(ea_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    for name, n in NEW.items():
        assert name in declared_symbols() and counts[name] == n and len(_native.SIGNATURES[name]) == n, name
        assert hasattr(_native.lib(), name)
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 35
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert _native.lib().ea_adaptive_sample_ws.restype is ctypes.c_int64
    assert _native.lib().ea_adaptive_beam_ws.restype is ctypes.c_int64


def _arrays(cutoffs, dims):
    from efficient_attention import _native as nv
    return nv.host_array(ctypes.c_int64, cutoffs), nv.host_array(ctypes.c_int32, dims)


def _sample_ws(M, cutoffs, dims):
    from efficient_attention import _native as nv
    return nv.lib().ea_adaptive_sample_ws(M, len(dims), *_arrays(cutoffs, dims))


def _beam_ws(M, cutoffs, dims, W):
    from efficient_attention import _native as nv
    return nv.lib().ea_adaptive_beam_ws(M, len(dims), *_arrays(cutoffs, dims), W)


def test_s0_the_workspace_queries_equal_the_documented_layout():
    from efficient_attention import _native as nv
    SPAN, MAX_K = pref.constants()
    r16 = pref.r16
    cases = ((1, [96, 200, 333], [64, 32]), (64, [96, 200, 333], [64, 32]), (17, [37, 187, 257], [64, 32]),
             (8, [20000, 60000, 267744], [256, 64]), (33, [48, 48 + 3 * SPAN + 5], [256]),
             (64, [40, 100, 160, 300, 500], [64, 32, 32, MAX_K + 32]), (1, [1, 2], [32]))
    for M, cutoffs, dims in cases:
        lay = sel.ws_layout(M, cutoffs, dims)
        pick = nv.lib().ea_adaptive_pick_ws(M, len(dims), *_arrays(cutoffs, dims))
        assert lay["pick_total"] == pick == pref.ws_layout(M, cutoffs, dims)["total"], "the pick's workspace is the prefix"
        assert _sample_ws(M, cutoffs, dims) == lay["total"], (M, cutoffs, dims)
        n, sizes = len(dims), sel.band_sizes(cutoffs)
        formula = pick + sum(r16(4 * M * v) for v in sizes) \
            + sum(r16(8 * M * -(-sizes[i + 1] // 16)) for i, d in enumerate(dims) if d <= MAX_K) + 2 * r16(256 * M * (n + 1))
        assert lay["total"] == formula
        for W in (w for w in (1, 4, 32) if M % w == 0):
            blay = sel.ws_layout(M, cutoffs, dims, W)
            assert _beam_ws(M, cutoffs, dims, W) == blay["total"] == formula + 2 * r16(8 * M * W), (M, W)
            assert blay["cand_idx"] == formula and all(blay[k] == lay[k] for k in lay if k != "total")
    # the recipe's geometry at 8 rows: about 4 M V bytes on top of the pick's
    assert 4 * 8 * 267744 <= _sample_ws(8, [20000, 60000, 267744], [256, 64]) <= 5 * 8 * 267744
    good = ([96, 200, 333], [64, 32])
    assert _sample_ws(0, *good) < 0 and _sample_ws(65, *good) < 0
    assert _sample_ws(8, [96, 96, 333], [64, 32]) < 0 and _sample_ws(8, [0, 200, 333], [64, 32]) < 0
    assert _sample_ws(8, [96, 200, 333], [64, 0]) < 0 and _sample_ws(8, [96, 200, 2 ** 31], [64, 32]) < 0
    assert _sample_ws(8, [1, 2, 3, 4, 5, 6], [32] * 5) < 0
    assert nv.lib().ea_adaptive_sample_ws(8, 2, None, None) < 0
    assert _beam_ws(8, *good, 0) < 0 and _beam_ws(8, *good, 33) < 0 and _beam_ws(8, *good, 3) < 0 and _beam_ws(64, *good, 32) > 0
    assert _beam_ws(0, *good, 1) < 0 and _beam_ws(65, *good, 5) < 0


BAD, UNS = -1, -2


def _common_errors(call):
    from efficient_attention import _native as nv
    odd = ctypes.c_void_p(4096 + 4)
    for kw in (dict(cut=None), dict(dims=None), dict(proj=None), dict(tables=None), dict(x=None), dict(head=None),
               dict(ws=None), dict(token=None), dict(M=0), dict(C=0), dict(n=0), dict(ldx=64),
               dict(cut=nv.host_array(ctypes.c_int64, [96, 96, 333])), dict(cut=nv.host_array(ctypes.c_int64, [0, 200, 333])),
               dict(dims=nv.host_array(ctypes.c_int32, [64, 0])), dict(w_dtype=2), dict(x_dtype=1),
               dict(proj=nv.host_array(ctypes.c_void_p, [4096, None])), dict(tables=nv.host_array(ctypes.c_void_p, [4096 + 8, 4096])),
               dict(x=odd), dict(head=odd), dict(ws=odd), dict(token=odd), dict(x_dtype=0, ldx=132), dict(ws_bytes=64)):
        assert call(**kw) == BAD, kw
    for kw in (dict(M=65), dict(C=144, ldx=144), dict(dims=nv.host_array(ctypes.c_int32, [64, 40])),
               dict(n=5, cut=nv.host_array(ctypes.c_int64, [1, 2, 3, 4, 5, 6]), dims=nv.host_array(ctypes.c_int32, [32] * 5),
                    proj=nv.host_array(ctypes.c_void_p, [4096] * 5), tables=nv.host_array(ctypes.c_void_p, [4096] * 5)),
               dict(cut=nv.host_array(ctypes.c_int64, [96, 200, 2 ** 31]))):
        assert call(**kw) == UNS, kw


def test_s0_sample_argument_errors_are_decided_before_any_launch():
    """Every refusal has its code with no device present: a launch would fail differently."""
    from efficient_attention import _native as nv
    lib = nv.lib()
    cut, dims = _arrays([96, 200, 333], [64, 32])
    fake, big = ctypes.c_void_p(4096), 1 << 40                       # (aligned, never dereferenced: the call stops before)
    ptrs = nv.host_array(ctypes.c_void_p, [4096, 4096])

    def call(M=10, C=128, n=2, cut=cut, dims=dims, x=fake, x_dtype=2, ldx=128, head=fake, w_dtype=0, proj=ptrs, tables=ptrs,
             ws=fake, ws_bytes=big, top_k=5, top_p=0.9, temperature=1.0, seed=1, ctr=fake, sid=fake, token=fake, logp=fake,
             sel_idx=None, sel_val=None, kept=None):
        return lib.ea_adaptive_sample(M, C, n, cut, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws, ws_bytes, top_k,
                                      top_p, temperature, seed, ctr, sid, token, logp, sel_idx, sel_val, kept, None)
    _common_errors(call)
    odd, odd2 = ctypes.c_void_p(4096 + 4), ctypes.c_void_p(4098)
    for kw in (dict(logp=None), dict(logp=odd2), dict(ctr=None), dict(sid=None), dict(ctr=odd), dict(sid=odd2),
               dict(sel_idx=odd2), dict(sel_val=odd2), dict(kept=odd2), dict(top_k=0), dict(top_p=0.0), dict(top_p=1.5),
               dict(top_p=float("nan")), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
               dict(temperature=float("nan"))):
        assert call(**kw) == BAD, kw
    assert call(top_k=65) == UNS
    assert call(top_k=65, ws=None) == BAD                            # (bad arguments are decided before the geometry)


def test_s0_beam_argument_errors_are_decided_before_any_launch():
    from efficient_attention import _native as nv
    lib = nv.lib()
    cut, dims = _arrays([96, 200, 333], [64, 32])
    fake, big = ctypes.c_void_p(4096), 1 << 40
    ptrs = nv.host_array(ctypes.c_void_p, [4096, 4096])
    state = ("score", "t", "nfin", "done", "token", "parent", "hist_tok", "hist_par", "fin_score", "fin_len", "fin_beam")

    def call(M=12, C=128, n=2, cut=cut, dims=dims, x=fake, x_dtype=2, ldx=128, head=fake, w_dtype=0, proj=ptrs, tables=ptrs,
             ws=fake, ws_bytes=big, W=4, eos=2, max_new=5, cand_idx=None, cand_score=None, **kw):
        ptr = {k: kw.get(k, fake) for k in state}
        return lib.ea_adaptive_beam(M, C, n, cut, dims, x, x_dtype, ldx, head, w_dtype, proj, tables, ws, ws_bytes, W, eos,
                                    max_new, *[ptr[k] for k in state], cand_idx, cand_score, None)
    _common_errors(call)
    odd2 = ctypes.c_void_p(4098)
    for k in state:
        assert call(**{k: None}) == BAD, k
        assert call(**{k: ctypes.c_void_p(4096 + 4) if k in ("token", "parent") else odd2}) == BAD, k
    for kw in (dict(cand_idx=odd2), dict(cand_score=odd2), dict(W=0), dict(eos=-1), dict(eos=333), dict(max_new=0)):
        assert call(**kw) == BAD, kw
    for kw in (dict(W=33, M=33), dict(W=5), dict(M=68, W=4)):
        assert call(**kw) == UNS, kw


# ---- the host reference against hand-worked answers ---------------------------------------------------------------------------
def test_s0_the_reference_forms_the_joint_scores_by_the_rules_operations():
    head = np.array([[1.0, 3.0, 2.0]], dtype=F32)                    # c0 = 3
    tail = np.array([[0.5, 4.0]], dtype=F32)                         # one tail of two tokens
    cls = np.array([[2.5]], dtype=F32)
    lse = [np.array([3.75], dtype=F32), np.array([4.25], dtype=F32)]
    j = sel.joint([head, tail], cls, lse)
    assert j[0].dtype == F32 and j[0].tolist() == [[-2.75, -0.75, -1.75]]
    assert j[1].tolist() == [[(2.5 - 3.75) + (0.5 - 4.25), (2.5 - 3.75) + (4.0 - 4.25)]] == [[-5.0, -1.5]]
    idx, val, _ = sel.select([head, tail], cls, lse, [3, 5], 3)
    assert idx.tolist() == [[1, 4, 2]] and val.tolist() == [[-0.75, -1.5, -1.75]]
    # k > V_b and k > V: a band shorter than k is there whole, the selection is the vocabulary in order
    idx, val, _ = sel.select([head, tail], cls, lse, [3, 5], 64)
    assert idx.tolist() == [[1, 4, 2, 0, 3]] and val.tolist() == [[-0.75, -1.5, -1.75, -2.75, -5.0]]
    idx, _, _ = sel.select([head, tail], cls, lse, [3, 5], 1)
    assert idx.tolist() == [[1]]
    assert sel.eos_score(j, [3, 5], 4).tolist() == [-1.5] and sel.eos_score(j, [3, 5], 2).tolist() == [-1.75]
    ci, cs = sel.beam_candidates(idx, np.array([[-0.75]], dtype=F32), np.array([-1.0], dtype=F32))
    assert ci.dtype == np.int32 and cs.tolist() == [[-1.75]]


def test_s0_the_reference_decides_ties():
    # a tie inside a band: the lower column first; +0 and -0 are equal
    head = np.array([[2.0, 5.0, 5.0, -0.0, 0.0]], dtype=F32)
    tail = np.array([[1.0, 1.0, 7.0]], dtype=F32)
    cls = np.array([[0.0]], dtype=F32)
    lse = [np.array([0.0], dtype=F32), np.array([2.0], dtype=F32)]
    idx, val, j = sel.select([head, tail], cls, lse, [5, 8], 8)
    # joint: words 2 5 5 -0 0; tail tokens 5, 6, 7: -1 -1 5
    assert j[1].tolist() == [[-1.0, -1.0, 5.0]]
    assert idx.tolist() == [[1, 2, 7, 0, 3, 4, 5, 6]]                # the tie across bands (5 = 5 = 5): by vocabulary index
    assert val[0, :3].tolist() == [5.0, 5.0, 5.0]
    # the band's RAW order decides who is a candidate: k = 1 takes column 1 of the head and token 7, nothing else
    idx, _, _ = sel.select([head, tail], cls, lse, [5, 8], 1)
    assert idx.tolist() == [[1]]
    idx, _, _ = sel.select([head, tail], cls, lse, [5, 8], 2)
    assert idx.tolist() == [[1, 2]]                                  # candidates 1, 2 | 7, 5: the best two of (5, 5, 5, -1)
    # two raw logits of a band that differ but round to one joint score: the raw order picks the candidate at the k-th place
    big = F32(2.0 ** 26)
    head2 = np.array([[1.0, 1.5]], dtype=F32)                        # 1 - 2^26 and 1.5 - 2^26 both round to -2^26
    lse2 = [np.array([big], dtype=F32), np.array([0.0], dtype=F32)]
    j2 = sel.joint([head2, np.array([[-big * 4]], dtype=F32)], np.array([[0.0]], dtype=F32), lse2)
    assert j2[0][0, 0] == j2[0][0, 1], "fp32 rounding has made the two joint scores equal"
    idx, _, _ = sel.select([head2, np.array([[-big * 4]], dtype=F32)], np.array([[0.0]], dtype=F32), lse2, [2, 3], 1)
    assert idx.tolist() == [[1]], "the larger RAW logit is the band's candidate"
    idx, _, _ = sel.select([head2, np.array([[-big * 4]], dtype=F32)], np.array([[0.0]], dtype=F32), lse2, [2, 3], 2)
    assert idx.tolist() == [[0, 1]], "both are candidates: equal joint scores by vocabulary index"


def test_s0_the_reference_on_a_nan_row():
    head = np.array([[1.0, np.nan, 3.0], [1.0, 2.0, 3.0]], dtype=F32)
    tail = np.array([[0.0, 1.0], [0.0, 1.0]], dtype=F32)
    cls = np.array([[0.5], [0.5]], dtype=F32)
    lse = [np.array([np.nan, 3.5], dtype=F32), np.array([1.25, 1.25], dtype=F32)]     # (ABI 34's case: a NaN maximum, a NaN lse)
    idx, val, _ = sel.select([head, tail], cls, lse, [3, 5], 3)
    assert np.isnan(val[0]).all() and idx[0].tolist() == [0, 1, 2], "every score is NaN: equal, by vocabulary index"
    assert idx[1].tolist() == [2, 1, 0] and val[1].tolist() == [-0.5, -1.5, -2.5], "the row beside it is what it is alone"
    alone = sel.select([head[1:], tail[1:]], cls[1:], [v[1:] for v in lse], [3, 5], 3)
    assert alone[0].tolist() == idx[1:].tolist() and alone[1].tobytes() == val[1:].tobytes()


# ---- the stack ----------------------------------------------------------------------------------------------------------------
def _state(dtype, B=2):
    from ea_harness import sequence as sq
    return sq.DecodingState({}, None, dict(batch_size=B, max_tokens=16, dtype=dtype, device="cpu"))


def test_s0_stack_errors_and_attachments():
    from ea_harness import sequence as sq
    from ea_harness import token_pick as tp
    plain = sq.DecoderStack(333, 128, 256, 2, 1, ATTN).eval()
    stack = sq.DecoderStack(333, 128, 256, 2, 1, ATTN, adaptive=dict(cutoff=[96, 200], factor=2)).eval()
    cut, dims = [96, 200, 333], [64, 32]
    # states with neither a held table nor an adaptive pick keep their error texts
    bare = _state(torch.bfloat16)
    with pytest.raises(RuntimeError, match="init_sampling needs a decoding state that holds the vocabulary table"):
        plain.init_sampling(bare, 1, 5)
    with pytest.raises(RuntimeError, match="init_beam_search needs a decoding state that holds the vocabulary table"):
        plain.init_beam_search(bare, 2, 1, 4)
    with pytest.raises(NotImplementedError, match="adaptive.*init_adaptive_decoding") as err:
        stack.init_decoding(2, 16, torch.bfloat16, "cpu", hold_vocab=True)
    assert "init_sampling" in str(err.value) and "init_beam_search" in str(err.value) and "not built" not in str(err.value)
    # a sampler on an adaptive state: the new workspace for the state's batch size, ctr, sid
    state = stack.init_adaptive_decoding(_state(torch.bfloat16, B=4))
    for bad in (dict(top_k=0), dict(top_k=65), dict(top_p=0.0), dict(temperature=0.0), dict(seed=-1)):
        with pytest.raises(ValueError):
            stack.init_sampling(state, **dict(dict(seed=3, top_k=5), **bad))
        assert state.sampler is None
    assert stack.init_sampling(state, 3, 40, 0.9, 0.7) is state
    sm = state.sampler
    assert isinstance(sm, sq.Sampler) and sm.logits is None and sm.ws.dtype == torch.uint8
    assert sm.ws.numel() == sel.ws_layout(4, cut, dims)["total"], "sized for the state's batch size, not 64"
    assert sm.ctr.tolist() == [0] * 4 and sm.sid.tolist() == [0, 1, 2, 3] and sm.next_sid == 4
    assert (sm.seed, sm.top_k, sm.top_p, sm.temperature) == (3, 40, 0.9, 0.7)
    assert sum(t.numel() * t.element_size() for t in sm.tensors()) == sm.ws.numel() + 12 * 4
    assert isinstance(tp.select_pick(stack, state, 4), tp.AdaptiveSampled)
    assert isinstance(tp.select_pick(stack, state, 4, True), tp.AdaptiveSampled), "no scorer is required"
    with pytest.raises(ValueError, match="a prompt of 5 rows"):
        tp.select_pick(stack, state, 5)
    # the plain sampler's reorder / reset behaviour
    sm.ctr.copy_(torch.tensor([5, 6, 7, 8]))
    sm.reorder(torch.tensor([2, 2, 0, 1]))
    assert sm.ctr.tolist() == [7, 7, 5, 6] and sm.sid.tolist() == [2, 2, 0, 1]
    sm.reset_rows([1, 3])
    assert sm.ctr.tolist() == [7, 0, 5, 0] and sm.sid.tolist() == [2, 4, 0, 5] and sm.next_sid == 6
    with pytest.raises(RuntimeError, match="a beam search draws nothing"):
        stack.init_beam_search(state, 2, 1, 4)
    rows = torch.zeros(1, 4, 128)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):               # (a missing device is an error, never a fall-back)
        stack.sample_tokens(rows, state)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        stack.sample_tokens_logprobs(rows, state)
    with pytest.raises(ValueError, match="single-token step"):
        stack.sample_tokens(torch.zeros(2, 4, 128), state)
    # a beam on an adaptive state
    state = stack.init_adaptive_decoding(_state(torch.bfloat16, B=6))
    assert isinstance(tp.select_pick(stack, state, 6), tp.AdaptiveGreedy)
    for bad in (dict(beam_size=0), dict(beam_size=4), dict(eos_idx=333), dict(eos_idx=-1), dict(max_new=0)):
        with pytest.raises(ValueError):
            stack.init_beam_search(state, **dict(dict(beam_size=3, eos_idx=2, max_new=5), **bad))
        assert state.beam is None
    assert stack.init_beam_search(state, 3, 332, 5, 0.5) is state
    bm = state.beam
    assert isinstance(bm, sq.Beam) and bm.logits is None and bm.ws.numel() == sel.ws_layout(6, cut, dims, 3)["total"]
    assert (bm.beam_size, bm.eos_idx, bm.max_new, bm.len_penalty) == (3, 332, 5, 0.5)
    assert bm.score.tolist() == [0.0, float("-inf"), float("-inf")] * 2 and bm.t.tolist() == [0, 0]
    assert tuple(bm.hist_tok.shape) == (5, 6) and tuple(bm.fin_score.shape) == (2, 3) and bm.parent.dtype == torch.long
    assert all(t is not None for t in bm.tensors()) and len(bm.tensors()) == 11
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        stack.beam_step(torch.zeros(1, 6, 128), state)
    with pytest.raises(ValueError, match="single-token step of the whole state"):
        stack.beam_step(torch.zeros(1, 5, 128), state)
