"""-m gpu: static incremental decoding of CausalEVAttention (init_static_decoding), the step that can be captured into a graph.

A static step is ea_ceva_sdecode_append / _close / _attn / _advance with the token count in device memory.  Checked here: it
equals the dynamic step bit for bit (same arithmetic), a captured 1-token step replayed across window boundaries and chunk
closes equals static eager decoding bit for bit and the full forward at the usual tolerances, two stacked layers in one graph,
the in-place beam reorder (eager and captured), the launch budget of a step, and both overflow cases."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

from test_gpu_causal_eva import RECIPE, _build                               # noqa: E402
from ceva_decoding import (DTYPES, IDS, OLD, STATIC, _Calls, _captured_run, _check_full, _ctx, _decode,   # noqa: E402
                           _geometry, _skip_f32, _stack_step)

# ---- 1. static eager == dynamic, bit for bit --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["recipe_d64", "recipe_d128", "overlap_d64", "no_rpe_noln", "many_chunks"])
@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "leftpad"])
def test_static_eager_equals_dynamic(dtype, variant, padded):
    _skip_f32(dtype)
    aa, embed, heads, T, B = _geometry(variant)
    w = aa["window_size"]
    T = max(T, 3 * w + 11)                                     # past at least 3 window boundaries
    m = _build(embed, heads, aa)
    torch.manual_seed(31)
    x = torch.randn(T, B, embed, device="cuda")
    pad = None
    if padded:
        pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        pad[1, :2 * aa["chunk_size"] + 3] = True              # element 1: a left-padded prompt
    steps = (37, 1, 1, 5)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dyn, _ = _decode(m, x, steps, "dynamic", dtype, pad)
        with _Calls() as calls:
            sta, state = _decode(m, x, steps, "static", dtype, pad, calls=calls)
    assert len(dyn) == len(sta)
    for i, (a, b) in enumerate(zip(dyn, sta)):
        assert a.dtype == b.dtype and torch.equal(a, b), (variant, i)
    assert m._get_input_buffer(state)["qkv"].dtype == dtype
    got = calls.all()
    assert not [c for c in got if c in OLD or c.startswith("ea_ceva_decode")], sorted(set(got))
    assert not m.static_decoding_overflowed(state)
    assert int(m._get_input_buffer(state)["pos"].item()) == T


# ---- 2. a captured 1-token step, replayed ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_captured_step_replays_equal_static_eager(dtype):
    """Prefill 23 tokens, then 96 replays of one captured 1-token step: 3 window boundaries (w = 32) and 24 chunk closes
    (r = 4).  Bit for bit equal to static eager decoding; against the full forward at the fp32 / 16-bit tolerances."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(41)
    T, B, P = 120, 2, 23
    x = torch.randn(T, B, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x)
        eager, _ = _decode(m, x, (P,), "static", dtype)
        eager = torch.cat(eager, 0)
        got, states = _captured_run([m], x, P, dtype, "static")           # (one residual layer: the rows are x + attn(x))
    assert torch.equal(got, eager[P:] + x[P:]), (got.float() - (eager[P:] + x[P:]).float()).abs().max().item()
    _check_full(eager[P:], full[P:], dtype)
    assert not m.static_decoding_overflowed(states[0])
    assert int(m._get_input_buffer(states[0])["pos"].item()) == T


# ---- 3. two stacked layers in one graph ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_two_stacked_layers_in_one_graph(dtype):
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=8)
    mods = [_build(256, 4, aa, seed=s) for s in (3, 4)]
    torch.manual_seed(43)
    T, B, P = 90, 2, 9
    x = torch.randn(T, B, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        states = [{} for _ in mods]
        for m, st in zip(mods, states):
            m.init_incremental_state()
            m.init_static_decoding(st, B, T, dtype, "cuda")
        eager = [_stack_step(mods, states, x[:P])] + [_stack_step(mods, states, x[t:t + 1]) for t in range(P, T)]
        eager = torch.cat(eager, 0)
        got, _ = _captured_run(mods, x, P, dtype, "static")
        h = x
        for m in mods:                                         # the stack on the full forward
            h = h + m(h, h, h)[0]
    assert torch.equal(got, eager[P:]), (got.float() - eager[P:].float()).abs().max().item()
    _check_full(got, h[P:], dtype)


# ---- 4. beam reorder ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("graph_reorder", [False, True], ids=["eager_reorder", "captured_reorder"])
def test_beam_reorder_between_replays(dtype, graph_reorder):
    """reorder_incremental_state on a static state permutes its buffers in place, outside or inside a graph; the replays
    that follow equal the dynamic path given the same reorder, bit for bit."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(47)
    T, B, P, R = 80, 3, 11, 45
    x = torch.randn(T, B, 256, device="cuda")
    order = torch.tensor([2, 0, 0], device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = {}
        m.init_incremental_state()
        ref = [m(x[:P], x[:P], x[:P], incremental_state=st)[0]]
        for t in range(P, T):
            if t == R:
                m.reorder_incremental_state(st, order)
            src = x if t < R else x[:, order]
            ref.append(m(src[t:t + 1], src[t:t + 1], src[t:t + 1], incremental_state=st)[0])
        ref = torch.cat(ref, 0)
        xr = torch.cat([x[:R], x[R:, order]], 0)
        got, states = _captured_run([m], x, P, dtype, "static", reorder=R, order=order, graph_reorder=graph_reorder)
    assert torch.equal(got, ref[P:] + xr[P:]), (got.float() - (ref[P:] + xr[P:]).float()).abs().max().item()
    buf = m._get_input_buffer(states[0])
    assert int(buf["pos"].item()) == T


# ---- 5. launch budget ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_static_step_launches(dtype):
    """A static step calls the four ea_ceva_sdecode_* entry points once each, in order, and otherwise only the projections;
    none of the training-path or dynamic decoding entries.  The same holds for the captured step (capture raises on a
    synchronisation, so that it succeeds shows the step never synchronises)."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(53)
    T, B = 40, 2
    x = torch.randn(T, B, 256, device="cuda")
    st = {}
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings(), _Calls() as calls:
        warnings.simplefilter("ignore")
        m.init_incremental_state()
        m.init_static_decoding(st, B, T, dtype, "cuda")
        for t, n in ((0, 7), (7, 1), (8, 1)):
            calls.step()
            m(x[t:t + n], x[t:t + n], x[t:t + n], incremental_state=st)
        xin = x[9:10].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        calls.step()
        with torch.cuda.stream(s):
            m(xin, xin, xin, incremental_state=st)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        calls.step()
        with torch.cuda.graph(g):
            m(xin, xin, xin, incremental_state=st)
    for got in calls.steps:
        core = [c for c in got if not (c.startswith("ea_linear") or c == "ea_multi_cast")]
        assert core == list(STATIC), got
    g.replay()
    torch.cuda.synchronize()
    assert int(m._get_input_buffer(st)["pos"].item()) == 11


# ---- 6. overflow -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eager_overflow_raises_before_launching():
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    T, B = 64, 2                                               # a multiple of w: cap == max_tokens
    x = torch.randn(T + 1, B, 256, device="cuda")
    st = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), _Calls() as calls:
        m.init_incremental_state()
        m.init_static_decoding(st, B, T, torch.bfloat16, "cuda")
        m(x[:T], x[:T], x[:T], incremental_state=st)
        calls.step()
        with pytest.raises(RuntimeError, match="static decoding state is full"):
            m(x[T:], x[T:], x[T:], incremental_state=st)
    assert calls.steps[-1] == []
    assert int(m._get_input_buffer(st)["pos"].item()) == T and not m.static_decoding_overflowed(st)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_replay_overflow_sets_the_flag_and_writes_nothing(dtype):
    """A replay cannot raise: the step that would pass cap sets `status`, writes NaN outputs and no byte of the state --
    the buffers are placed in arenas with a canary region right after each, and every byte is compared."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(59)
    T, B = 64, 2
    x = torch.randn(T + 2, B, 256, device="cuda")
    st = {}
    arenas = {}
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.init_incremental_state()
        m.init_static_decoding(st, B, T, dtype, "cuda")
        buf = m._get_input_buffer(st)
        for k in ("qkv", "pad", "rf_k_bar", "beta"):
            t = buf[k]
            nbytes = t.numel() * t.element_size()
            arena = torch.full((nbytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
            view = arena[:nbytes].view(t.dtype).view(t.shape)
            view.copy_(t)
            buf[k] = view
            arenas[k] = arena
        m(x[:T - 2], x[:T - 2], x[:T - 2], incremental_state=st)
        xin = x[T - 2:T - 1].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(xin, xin, xin, incremental_state=st)                # token T - 2
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y, _ = m(xin, xin, xin, incremental_state=st)
        xin.copy_(x[T - 1:T])
        g.replay()                                                # token T - 1: the cache is full
        torch.cuda.synchronize()
        assert int(buf["pos"].item()) == T and not m.static_decoding_overflowed(st)
        assert torch.isfinite(y).all()
        before = {k: a.clone() for k, a in arenas.items()}
        xin.copy_(x[T:T + 1])
        g.replay()                                                # token T: past cap
        torch.cuda.synchronize()
    assert m.static_decoding_overflowed(st)
    assert int(buf["pos"].item()) == T
    assert torch.isnan(y).all()
    for k, a in arenas.items():
        assert torch.equal(a, before[k]), k
        assert (a[-4096:] == 0x5A).all(), k
