"""-m gpu: rolling incremental decoding of CausalEVAttention (init_rolling_decoding): the static step on a state whose token
rows live in a ring of R slots (token n in slot n % R), the landmark rows staying linear.

The main handle is bit-for-bit equality with the static state for one sequence of step sizes (the ring changes addresses, not
arithmetic), over runs that lap the ring at least twice.  Also here: nothing older than the live window is read (dead slots
poisoned between steps), token-by-token decoding against the full forward, the module's own splitting of a prompt longer
than max_step_tokens, capture and replay across ring wraps, two stacked layers in one graph, the beam reorder, the launch
budget of a step, both overflow cases, and the size of the state."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

from test_gpu_causal_eva import RECIPE, _build                               # noqa: E402
from ceva_decoding import (DTYPES, IDS, OLD, STATIC, _Calls, _captured_run, _check_full, _ctx, _decode,   # noqa: E402
                           _geometry, _init, _skip_f32, _stack_step)

VARIANTS = ["recipe_d64", "recipe_d128", "overlap_d64", "no_rpe_noln", "many_chunks"]


def _ring(m, S=None):
    """The issue's formula: the smallest multiple of w with R >= w + e + S, S = max_step_tokens (default w)."""
    w, e = m.window_size, m.ext_size
    S = w if S is None else S
    return -(-(w + e + S) // w) * w


def _case(variant, padded, smode):
    """-> module, x, pad, steps, S, R for a run that laps its ring at least twice."""
    aa, embed, heads, T, B = _geometry(variant)
    w = aa["window_size"]
    m = _build(embed, heads, aa)
    S = 37 if smode == "S37" else None
    steps = (37, 1, 1, 5) if smode == "S37" else (w - 3, 1, 1, 5)
    R = _ring(m, S)
    T = max(T, 2 * R + w + 11)
    torch.manual_seed(31)
    x = torch.randn(T, B, embed, device="cuda")
    pad = None
    if padded:
        pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        pad[1, :2 * aa["chunk_size"] + 3] = True              # element 1: a left-padded prompt
    return m, x, pad, steps, S, R


# ---- 3. rolling == static, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "leftpad"])
@pytest.mark.parametrize("smode", ["S37", "Sw"])
def test_rolling_equals_static(dtype, variant, padded, smode):
    """Same module, inputs and step sizes (all <= S; S = 37 < w and S = w) on a static and a rolling state, T >= 2 R + w + 11
    tokens: outputs equal step by step, landmarks / pos / status equal at the end, and ring slot n % R holds what row n of
    the static cache holds for the last R tokens, rows and pad flags."""
    _skip_f32(dtype)
    m, x, pad, steps, S, R = _case(variant, padded, smode)
    T = x.shape[0]
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sta, sstate = _decode(m, x, steps, "static", dtype, pad)
        with _Calls() as calls:
            rol, rstate = _decode(m, x, steps, "rolling", dtype, pad, S=S, calls=calls)
    assert len(sta) == len(rol)
    for i, (a, b) in enumerate(zip(sta, rol)):
        assert a.dtype == b.dtype and torch.equal(a, b), (variant, i)
    sb, rb = m._get_input_buffer(sstate), m._get_input_buffer(rstate)
    assert rb["qkv"].dtype == dtype and rb["qkv"].shape[1] == R and rb["pad"].shape == (x.shape[1], R)
    assert T >= 2 * R and sb["qkv"].shape[1] > R                # the run lapped a real ring at least twice
    for k in ("rf_k_bar", "beta", "pos", "status"):
        assert rb[k].shape == sb[k].shape and torch.equal(rb[k], sb[k]), k
    n = torch.arange(T - R, T, device="cuda")
    assert torch.equal(rb["qkv"][:, n % R], sb["qkv"][:, n])
    assert torch.equal(rb["pad"][:, n % R], sb["pad"][:, n])
    got = calls.all()
    assert not [c for c in got if c in OLD or c.startswith("ea_ceva_decode")], sorted(set(got))
    assert not m.static_decoding_overflowed(rstate)
    assert int(rb["pos"].item()) == T


# ---- 4. nothing dead is read -----------------------------------------------------------------------------------------------------
def _poison_dead(m, R):
    """before(state, t): NaN rows / pad flag 1 in every ring slot whose token is older than floor(t / w) w - e, or that was
    never written."""
    w, e = m.window_size, m.ext_size

    def before(state, t):
        buf = m._get_input_buffer(state)
        s = torch.arange(R, device="cuda")
        tok = s + R * torch.div(t - 1 - s, R, rounding_mode="floor")      # the newest token < t of slot s; < 0: none yet
        dead = (tok < 0) | (tok < (t // w) * w - e)
        buf["qkv"][:, dead] = float("nan")
        buf["pad"][:, dead] = 1
    return before


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "leftpad"])
def test_nothing_dead_is_read(dtype, variant, padded):
    """The run of test_rolling_equals_static (S = 37) with every dead or never-written slot overwritten before every step:
    the outputs stay equal to the static state's, bit for bit."""
    _skip_f32(dtype)
    m, x, pad, steps, S, R = _case(variant, padded, "S37")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sta, _ = _decode(m, x, steps, "static", dtype, pad)
        rol, rstate = _decode(m, x, steps, "rolling", dtype, pad, S=S, before=_poison_dead(m, R))
    assert m._get_input_buffer(rstate)["qkv"].shape[1] == R
    for i, (a, b) in enumerate(zip(sta, rol)):
        assert torch.equal(a, b), (variant, i)


# ---- 5. against the full forward -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["recipe_d64", "many_chunks"])
@pytest.mark.parametrize("padded", [False, True], ids=["nopad", "leftpad"])
def test_token_by_token_rolling_equals_full_forward(dtype, variant, padded):
    """Single-token rolling steps from the first token on, over two laps of the ring, against the causal full forward given
    the same mask; padded rows excluded (and finite)."""
    _skip_f32(dtype)
    aa, embed, heads, T, _ = _geometry(variant)
    B = 3
    m = _build(embed, heads, aa)
    R = _ring(m)
    T = max(T, 2 * R + 11)
    r = aa["chunk_size"]
    torch.manual_seed(13)
    x = torch.randn(T, B, embed, device="cuda")
    pad, live = None, None
    if padded:
        pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        pad[1, :2 * r + 3] = True
        pad[2, :3] = True
        live = (~pad).t().unsqueeze(-1).double()
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x, key_padding_mask=pad)
        rol, rstate = _decode(m, x, (), "rolling", dtype, pad)
    got = torch.cat(rol, 0)
    assert m._get_input_buffer(rstate)["qkv"].shape[1] == R and got.shape == full.shape
    assert torch.isfinite(got).all()
    _check_full(got, full, dtype, live)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_long_context_rolling_equals_full_forward(dtype):
    """embed 128, 2 heads, w = 128, r = 8, T = 8192: the prompt (T - 64 tokens) fed as ONE call, which the module splits into
    pieces of max_step_tokens = w itself, then 64 single tokens; every row against the full forward's."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=128, chunk_size=8)
    m = _build(128, 2, aa)
    T, B, tail = 8192, 1, 64
    torch.manual_seed(17)
    x = torch.randn(T, B, 128, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x)
        with _Calls() as calls:
            rol, rstate = _decode(m, x, (T - tail,), "rolling", dtype, calls=calls)
    assert len(rol) == 1 + tail and rol[0].shape[0] == T - tail
    assert calls.steps[0].count("ea_ceva_sdecode_attn") == (T - tail + 127) // 128       # the module fed the pieces
    buf = m._get_input_buffer(rstate)
    assert buf["qkv"].shape[1] == 256 and int(buf["pos"].item()) == T
    _check_full(torch.cat(rol, 0), full, dtype)


# ---- 6. prompt splitting ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mask", ["nomask", "new_columns", "all_columns"])
def test_prompt_in_one_call_equals_caller_fed_pieces(dtype, mask):
    """A prompt of P > S tokens in one call == the caller feeding pieces of S (the last one shorter), bit for bit, outputs and
    state, and == a static state fed those pieces; with the pad flags in both of fairseq's shapes ([B, T_new] and
    [B, t0 + T_new])."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(61)
    T, B, P0, P, S = 200, 2, 5, 150, 20                         # 5 tokens first, so the prompt starts inside a chunk
    x = torch.randn(T, B, 256, device="cuda")
    pad = None
    if mask != "nomask":
        pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        pad[1, :11] = True
        pad[0, 40:43] = True

    def kpm(a, b):
        if pad is None:
            return None
        return pad[:, a:b] if mask == "new_columns" else pad[:, :b]

    def run(pieces, kind="rolling"):
        st = _init(m, kind, B, T, dtype, S)
        rows, t = [], 0
        for n in [P0] + pieces + [1] * (T - P0 - P):
            rows.append(m(x[t:t + n], x[t:t + n], x[t:t + n], key_padding_mask=kpm(t, t + n), incremental_state=st)[0])
            t += n
        return torch.cat(rows, 0), m._get_input_buffer(st)

    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one, b1 = run([P])
        fed, b2 = run([S] * (P // S) + ([P % S] if P % S else []))
        sta, b3 = run([S] * (P // S) + ([P % S] if P % S else []), kind="static")
    assert one.shape == fed.shape and torch.equal(one, fed)
    # the values: the same pieces on a static state -- 20-token steps that cross window boundaries and straddle the end of
    # the ring (R = 64) after it has wrapped
    assert torch.equal(one, sta)
    for k in ("rf_k_bar", "beta", "pos", "status"):
        assert torch.equal(b1[k], b3[k]), k
    for k in ("qkv", "pad", "rf_k_bar", "beta", "pos", "status"):
        assert torch.equal(b1[k], b2[k]), k
    assert b1["qkv"].shape[1] == 64 and int(b1["pos"].item()) == T       # R = ceil((32 + 0 + 20) / 32) 32


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_oversized_step_under_capture_raises_before_any_launch(dtype):
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    T, B, S = 200, 2, 8
    x = torch.randn(T, B, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings(), _Calls() as calls:
        warnings.simplefilter("ignore")
        st = _init(m, "rolling", B, T, dtype, S)
        m(x[:5], x[:5], x[:5], incremental_state=st)
        xin = x[5:5 + S + 1].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(x[5:6], x[5:6], x[5:6], incremental_state=st)                # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        calls.step()
        with pytest.raises(RuntimeError, match="max_step_tokens"):
            with torch.cuda.graph(g):
                xin.mul_(1.0)                                              # (so that the abandoned capture is not empty)
                m(xin, xin, xin, incremental_state=st)
    assert calls.steps[-1] == [], calls.steps[-1]
    torch.cuda.synchronize()
    assert int(m._get_input_buffer(st)["pos"].item()) == 6


# ---- 7. capture --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_captured_rolling_step_replays_equal_rolling_eager(dtype):
    """Prefill 23 tokens, then 176 replays of one captured 1-token step on a ring of R = 64 slots (w = 32, r = 4): three ring
    wraps, 6 window boundaries, 44 chunk closes.  Bit for bit equal to rolling eager decoding and to the static state."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(41)
    T, B, P = 200, 2, 23
    x = torch.randn(T, B, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x)
        eager = torch.cat(_decode(m, x, (P,), "rolling", dtype)[0], 0)
        static = torch.cat(_decode(m, x, (P,), "static", dtype)[0], 0)
        got, states = _captured_run([m], x, P, dtype)           # (one residual layer: the rows are x + attn(x))
    buf = m._get_input_buffer(states[0])
    assert buf["qkv"].shape[1] == 64 and T - P >= 2 * 64
    assert torch.equal(eager, static)
    assert torch.equal(got, eager[P:] + x[P:]), (got.float() - (eager[P:] + x[P:]).float()).abs().max().item()
    _check_full(eager[P:], full[P:], dtype)
    assert not m.static_decoding_overflowed(states[0])
    assert int(buf["pos"].item()) == T


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_stacked_rolling_layers_in_one_graph(dtype):
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=8)
    mods = [_build(256, 4, aa, seed=s) for s in (3, 4)]
    torch.manual_seed(43)
    T, B, P = 170, 2, 9
    x = torch.randn(T, B, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        states = [_init(m, "rolling", B, T, dtype) for m in mods]
        eager = [_stack_step(mods, states, x[:P])] + [_stack_step(mods, states, x[t:t + 1]) for t in range(P, T)]
        eager = torch.cat(eager, 0)
        got, gstates = _captured_run(mods, x, P, dtype)
        h = x
        for m in mods:                                         # the stack on the full forward
            h = h + m(h, h, h)[0]
    assert all(m._get_input_buffer(st)["qkv"].shape[1] == 64 for m, st in zip(mods, gstates))
    assert torch.equal(got, eager[P:]), (got.float() - eager[P:].float()).abs().max().item()
    _check_full(got, h[P:], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("graph_reorder", [False, True], ids=["eager_reorder", "captured_reorder"])
def test_beam_reorder_between_rolling_replays(dtype, graph_reorder):
    """reorder_incremental_state on a rolling state permutes its buffers in place, outside or inside a graph, after the ring
    has wrapped; the replays that follow equal the same run (capture, reorder, replays) on the static state, bit for bit."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(47)
    T, B, P, at = 180, 3, 11, 109
    x = torch.randn(T, B, 256, device="cuda")
    order = torch.tensor([2, 0, 0], device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref, sstates = _captured_run([m], x, P, dtype, kind="static", reorder=at, order=order, graph_reorder=graph_reorder)
        sbuf = {k: v.clone() for k, v in m._get_input_buffer(sstates[0]).items() if torch.is_tensor(v)}
        got, states = _captured_run([m], x, P, dtype, reorder=at, order=order, graph_reorder=graph_reorder)
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max().item()
    buf = m._get_input_buffer(states[0])
    R = buf["qkv"].shape[1]
    assert R == 64 and int(buf["pos"].item()) == T
    n = torch.arange(T - R, T, device="cuda")
    assert torch.equal(buf["qkv"][:, n % R], sbuf["qkv"][:, n]) and torch.equal(buf["pad"][:, n % R], sbuf["pad"][:, n])
    assert torch.equal(buf["rf_k_bar"], sbuf["rf_k_bar"]) and torch.equal(buf["beta"], sbuf["beta"])


# ---- 8. launch budget ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_rolling_step_launches(dtype, masked):
    """A rolling step of T <= S tokens calls the four ea_ceva_sdecode_* entry points once each, in order, and otherwise only
    the projections -- eager (before and after the ring wraps) and captured."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(53)
    T, B = 120, 2
    x = torch.randn(T, B, 256, device="cuda")
    pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    pad[1, :6] = True

    def kpm(a, b):
        return pad[:, a:b] if masked else None

    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings(), _Calls() as calls:
        warnings.simplefilter("ignore")
        st = _init(m, "rolling", B, T, dtype)
        t = 0
        for n in (7, 1, 32, 30, 1, 1):                          # (S = 32; the ring of 64 wraps inside the fourth step)
            calls.step()
            m(x[t:t + n], x[t:t + n], x[t:t + n], key_padding_mask=kpm(t, t + n), incremental_state=st)
            t += n
        xin, pin = x[t:t + 1].clone(), kpm(t, t + 1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        calls.step()
        with torch.cuda.stream(s):
            m(xin, xin, xin, key_padding_mask=pin, incremental_state=st)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        calls.step()
        with torch.cuda.graph(g):
            m(xin, xin, xin, key_padding_mask=pin, incremental_state=st)
    assert len(calls.steps) == 8
    for got in calls.steps:
        assert not [c for c in got if c in OLD], got
        core = [c for c in got if not (c.startswith("ea_linear") or c == "ea_multi_cast")]
        assert core == list(STATIC), got
    g.replay()
    torch.cuda.synchronize()
    assert int(m._get_input_buffer(st)["pos"].item()) == 74


# ---- 9. overflow -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eager_overflow_raises_at_cap_before_launching(dtype):
    """cap, the landmark capacity, bounds the rolling state (not its ring of 64 slots); a prompt that would pass it raises
    before its first piece is launched."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    T, B = 160, 2                                              # a multiple of w: cap == max_tokens
    x = torch.randn(T + 40, B, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings(), _Calls() as calls:
        warnings.simplefilter("ignore")
        st = _init(m, "rolling", B, T, dtype)
        assert m._get_input_buffer(st)["qkv"].shape[1] == 64
        m(x[:T - 3], x[:T - 3], x[:T - 3], incremental_state=st)
        calls.step()
        with pytest.raises(RuntimeError, match="static decoding state is full"):
            m(x[T - 3:T + 37], x[T - 3:T + 37], x[T - 3:T + 37], incremental_state=st)      # 40 tokens > S: would be split
        assert calls.steps[-1] == []
        m(x[T - 3:T], x[T - 3:T], x[T - 3:T], incremental_state=st)                       # up to cap: fine
        calls.step()
        with pytest.raises(RuntimeError, match="static decoding state is full"):
            m(x[T:T + 1], x[T:T + 1], x[T:T + 1], incremental_state=st)
    assert calls.steps[-1] == []
    assert int(m._get_input_buffer(st)["pos"].item()) == T and not m.static_decoding_overflowed(st)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_replay_overflow_sets_the_flag_and_writes_nothing(dtype):
    """A replay cannot raise: the step that would pass cap sets `status`, writes NaN outputs and no byte of the ring, the pad
    flags, the landmarks or pos -- the buffers are placed in arenas with a canary region right after each, and every byte
    is compared."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(59)
    T, B = 160, 2
    x = torch.randn(T + 2, B, 256, device="cuda")
    arenas = {}
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _init(m, "rolling", B, T, dtype)
        buf = m._get_input_buffer(st)
        assert buf["qkv"].shape[1] == 64
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
        g.replay()                                                # token T - 1: the landmark rows are full
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


# ---- 10. memory --------------------------------------------------------------------------------------------------------------
def _shape_bytes(m, buf, B, rows, cap, dtype):
    """The state's bytes from its shapes alone."""
    h, d, r, w, e = m.num_heads, m.head_dim, m.chunk_size, m.window_size, m.ext_size
    esz = torch.empty((), dtype=dtype).element_size()
    n = B * rows * 3 * h * d * esz + B * rows                  # qkv, pad
    n += 2 * B * h * (cap // r) * d * 4                          # rf_k_bar, beta
    n += 4 + 4                                                  # pos, status
    n += (w * (w + e) * 4 if m.use_t5_rpe else 0)               # the dense [w, w + e] bias table
    n += sum(p.numel() * 4 for p in m._mu_params())             # fp32 mu parameters
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("variant,S", [("recipe_d64", None), ("recipe_d64", 37), ("recipe_d64", 300), ("many_chunks", None),
                                       ("many_chunks", 5), ("no_rpe_noln", None)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ring_length_and_state_bytes(variant, S, dtype):
    _skip_f32(dtype)
    aa, embed, heads, _, B = _geometry(variant)
    m = _build(embed, heads, aa)
    w, e = m.window_size, m.ext_size
    R = _ring(m, S)
    assert R % w == 0 and R >= w + e + (S or w) and R - w < w + e + (S or w)
    sizes = {}
    for T in (4096, 65536):
        st = _init(m, "rolling", B, T, dtype, S)
        buf = m._get_input_buffer(st)
        cap = -(-T // w) * w
        assert buf["qkv"].shape == (B, R, 3, heads, embed // heads) and buf["pad"].shape == (B, R)
        assert buf["rf_k_bar"].shape == buf["beta"].shape == (B, heads, cap // aa["chunk_size"], embed // heads)
        assert m.decoding_state_nbytes(st) == _shape_bytes(m, buf, B, R, cap, dtype)
        sizes[T] = buf["qkv"].shape[1]
    assert sizes[4096] == sizes[65536] == R
    sst = _init(m, "static", B, 4096, dtype)
    assert m.decoding_state_nbytes(sst) == _shape_bytes(m, None, B, 4096, 4096, dtype)
    assert m.decoding_state_nbytes(sst) > m.decoding_state_nbytes(_init(m, "rolling", B, 4096, dtype, S))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_short_max_tokens_gives_the_linear_state(dtype):
    """cap <= R: the rolling state is the linear one (no wrap), no larger than init_static_decoding's, and decodes the same
    bits -- its max_step_tokens still splits a longer prompt."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(67)
    T, B = 60, 2                                               # cap = 64 = R
    x = torch.randn(T, B, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sta, sstate = _decode(m, x, (30, 1, 1, 5), "static", dtype)
        rol, rstate = _decode(m, x, (30, 1, 1, 5), "rolling", dtype)
        st_small = _init(m, "rolling", B, 20, dtype)           # cap = 32 < R
    sb, rb = m._get_input_buffer(sstate), m._get_input_buffer(rstate)
    assert rb["qkv"].shape == sb["qkv"].shape and rb["qkv"].shape[1] == 64
    assert m.decoding_state_nbytes(rstate) <= m.decoding_state_nbytes(sstate)
    assert m._get_input_buffer(st_small)["qkv"].shape[1] == 32
    assert m.decoding_state_nbytes(st_small) == m.decoding_state_nbytes(_init(m, "static", B, 20, dtype))
    for i, (a, b) in enumerate(zip(sta, rol)):
        assert torch.equal(a, b), i
    for k in ("qkv", "pad", "rf_k_bar", "beta", "pos", "status"):
        assert torch.equal(rb[k], sb[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dynamic_state_bytes(dtype):
    """decoding_state_nbytes on the dynamic state of _decode: the sum over its tensors."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    x = torch.randn(40, 2, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype):
        _, st = _decode(m, x, (40,), "dynamic", dtype)
    buf = m._get_input_buffer(st)
    assert m.decoding_state_nbytes(st) == sum(v.numel() * v.element_size() for v in buf.values() if torch.is_tensor(v)) > 0
