"""-m gpu: `hold_projections=True` of static / rolling incremental decoding (csrc/ea_ceva_decode_linear.hip).

A state made with the option holds 16-bit copies of the module's two projections; a step of at most 64 rows (T_new B) runs
them on ea_ceva_sdecode_linear, in front of append and behind advance, and touches no weight with a framework kernel.
Checked here: the kernel against fp64 under a derived bound, prefix consistency of the module on held states, the launches of
a step (eager, warm-up, capture) with the framework's weight ops banned, capture and replay against eager decoding bit for
bit, that the weights a step reads are the state's (and follow `refresh_decoding_weights` without a new capture), the bytes,
and overflow.

The bound of the kernel (and of the cache rows a held step writes), element-wise, with x^ = x rounded to the weight's type:
    |got - ref| <= u_y |ref| + 2 K 2^-24 (|x^| |w|^T + |bias|)
-- one unit in the last place of y (2^-7 bf16, 2^-10 fp16, 2^-23 fp32) for the one rounding of the result, and twice the
fp32 dot-product bound K u |x|.|w| (u = 2^-24) for the fp32 sums, whatever their order."""
import os
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

from test_gpu_causal_eva import RECIPE, _build                               # noqa: E402
from test_gpu_ceva_decode import _io                                         # noqa: E402
from test_gpu_ceva_split_decode import SPLIT, STATE_ROWS, _bits, _decode, _init   # noqa: E402
from ceva_decoding import STATIC, _Calls, _check_full, _ctx, _geometry      # noqa: E402

LINEAR = "ea_ceva_sdecode_linear"
HELD = (LINEAR,) + STATIC + (LINEAR,)
HELD_SPLIT = (LINEAR,) + SPLIT + (LINEAR,)
HELD_KEYS = ("w_qkv", "b_qkv", "w_out", "b_out", "proj_rows")
KINDS = ["static", "rolling"]
U = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}
W_DTYPES = [torch.bfloat16, torch.float16]
W_IDS = ["bf16", "fp16"]


def _excess(got, xh, w, bias, u_y):
    """max over the elements of |got - ref| / bound, ref in fp64 from the rounded operands (on the device)."""
    xd, wd = xh.double(), w.double()
    ref, mag = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    bound = u_y * ref.abs() + 2.0 * xh.shape[1] * 2.0 ** -24 * mag
    assert torch.isfinite(got).all()
    return ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


# ---- 1. the kernel against fp64 ---------------------------------------------------------------------------------------------
# (M, K, N, strided): (1, 96, 288): three k-steps over the waves, the others idle; 16 / 17: one row tile, and a second one
# holding one row; 64: the row bound; the last two: the LM shapes
LINEAR_SHAPES = [(1, 96, 288, False), (2, 256, 768, False), (16, 256, 256, False), (17, 256, 256, True),
                 (64, 512, 1536, False), (8, 1024, 3072, False), (8, 1024, 1024, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=["%dx%dx%d" % s[:3] for s in LINEAR_SHAPES])
def test_linear_kernel_against_fp64(wdtype, shape):
    from efficient_attention import _native as nv
    M, K, N, strided = shape
    g = torch.Generator().manual_seed(M * 1000 + K + N)
    x32 = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(wdtype).cuda()
    b = torch.randn(N, generator=g).to(wdtype).cuda()
    xh = x32.to(wdtype)                                          # round to nearest even, as the kernel's load does
    ldx, ldy = (K + 8, N + 8) if strided else (K, N)
    worst = 0.0
    for xdtype in (torch.float32, wdtype):
        xbuf = torch.full((M + 1, ldx), float("nan"), dtype=xdtype, device="cuda")      # (what lies beside x is not read)
        xbuf[:M, :K] = x32 if xdtype == torch.float32 else xh
        for ydtype in (wdtype, torch.float32):
            for bias in (b, None):
                y = torch.full((M + 3, ldy), 7.0, dtype=ydtype, device="cuda")
                nv.call(LINEAR, M, K, N, nv.ptr(xbuf), _io(xdtype), ldx, nv.ptr(w), _io(wdtype), nv.ptr(bias), nv.ptr(y),
                        _io(ydtype), ldy, nv.stream())
                torch.cuda.synchronize()
                assert (y[M:] == 7.0).all() and (y[:, N:] == 7.0).all(), (xdtype, ydtype)       # rows >= M, columns >= N
                e = _excess(y[:M, :N], xh, w, bias, U[ydtype])
                print(shape, wdtype, "x", xdtype, "y", ydtype, "bias" if bias is not None else "no bias", "|d| / bound: %.3f" % e)
                assert e <= 1.0, (shape, wdtype, xdtype, ydtype, bias is not None, e)
                worst = max(worst, e)
                y2 = torch.full_like(y, 7.0)                     # the same launch again: the same bits
                nv.call(LINEAR, M, K, N, nv.ptr(xbuf), _io(xdtype), ldx, nv.ptr(w), _io(wdtype), nv.ptr(bias), nv.ptr(y2),
                        _io(ydtype), ldy, nv.stream())
                assert _bits(y, y2)
    print(shape, wdtype, "worst |d| / bound: %.3f" % worst)


# ---- 2. the module: prefix consistency ----------------------------------------------------------------------------------------
def _held_geometry(name):
    if name == "d32":
        return dict(RECIPE, window_size=32, chunk_size=4), 96, 3, 110, 2
    return _geometry(name)


def _cache_rows_excess(m, st, x, dtype):
    """The qkv rows the state still holds against the fp64 projection of the same inputs with the held weights."""
    buf = m._get_input_buffer(st)
    T, B, C = x.shape
    rows = buf["qkv"].shape[1]
    n = torch.arange(max(T - rows, 0), T, device="cuda")
    got = buf["qkv"][:, n % rows].reshape(B, n.numel(), 3 * C)
    worst = 0.0
    for b in range(B):
        worst = max(worst, _excess(got[b], x[n, b].to(dtype), buf["w_qkv"], buf["b_qkv"], U[dtype]))
    return worst


# (the d = 128 recipe geometry, the large one, in bf16 only)
PREFIX_CASES = [("overlap_d64", torch.bfloat16), ("overlap_d64", torch.float16), ("recipe_d128", torch.bfloat16),
                ("d32", torch.bfloat16), ("d32", torch.float16)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geometry,dtype", PREFIX_CASES, ids=["%s-%s" % (g, str(d)[6:]) for g, d in PREFIX_CASES])
def test_held_decoding_equals_full_forward(dtype, kind, geometry):
    """Short steps (the new kernel: 14, 2, 2 and 16 rows, then 2 per token) and a long one (80 rows: the library GEMM on the
    held operands) mixed."""
    aa, embed, heads, T, B = _held_geometry(geometry)
    m = _build(embed, heads, aa)
    torch.manual_seed(83)
    x = torch.randn(T, B, embed, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x)
        with _Calls() as calls:
            rows, st = _decode(m, x, (7, 1, 1, 8, 40, 1), kind, dtype, calls=calls, hold_projections=True)
    got = torch.cat(rows, 0)
    assert got.dtype == full.dtype and got.shape == full.shape
    _check_full(got, full, dtype)
    assert [s.count(LINEAR) for s in calls.steps[:6]] == [2, 2, 2, 2, 0, 2]
    assert int(m._get_input_buffer(st)["pos"].item()) == T and not m.static_decoding_overflowed(st)
    e = _cache_rows_excess(m, st, x, dtype)
    print(geometry, kind, dtype, "cache rows |d| / bound: %.3f" % e)
    assert e <= 1.0


@pytest.mark.gpu
def test_held_step_output_dtype_and_rounding_warning():
    """The dtype of y is the plain step's: the autocast dtype under autocast, query.dtype outside it; an fp32 query outside
    autocast is rounded with the one-time warning of the attention cores."""
    from efficient_attention import _ops
    m = _build(256, 4, dict(RECIPE, window_size=32, chunk_size=4))
    x = torch.randn(3, 2, 256, device="cuda")
    with torch.no_grad():
        for cache in W_DTYPES:
            for ctx, q, want in ((_ctx(torch.bfloat16), x, torch.bfloat16), (_ctx(torch.float16), x, torch.float16),
                                 (_ctx(torch.float32), x.to(cache), cache), (_ctx(torch.float32), x, torch.float32)):
                held, plain = _init(m, "static", 2, 8, cache, hold_projections=True), _init(m, "static", 2, 8, cache)
                _ops._FP32_WARNED[0] = False
                with ctx, warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    y = m(q, q, q, incremental_state=held)[0]
                    told = [w for w in seen if "outside torch.autocast" in str(w.message)]
                    yp = m(q, q, q, incremental_state=plain)[0]
                assert y.dtype == yp.dtype == want and y.is_contiguous()
                assert len(told) == (1 if (q.dtype == torch.float32 and want == torch.float32) else 0)
                assert (y.float() - yp.float()).abs().max().item() <= 2e-2 * yp.float().abs().max().item()


# ---- 3. launches ------------------------------------------------------------------------------------------------------------
def _ban(monkeypatch, names):
    from efficient_attention import _ops

    def banned(name):
        def f(*a, **k):
            raise AssertionError("%s reached in a step on a state that holds its projections" % name)
        return f
    where = {"torch.cat": (torch, "cat"), "F.linear": (F, "linear"), "_ops.multi_cast": (_ops, "multi_cast"),
             "_ops.linear": (_ops, "linear"), "_ops.linear_wb": (_ops, "linear_wb")}
    for n in names:
        monkeypatch.setattr(*where[n], banned(n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("opt", [{}, dict(landmark_splits=4, per_sequence=True)], ids=["plain", "split_per_seq"])
def test_held_step_launches(kind, opt, monkeypatch):
    """Steps of 1 and of 8 tokens (B = 2): exactly linear, append, close, attn (attn_split, merge), advance, linear -- eagerly,
    in the warm-up on a side stream and under capture -- with the framework's weight ops replaced by functions that raise.
    35 tokens (70 rows): append, close, attn, advance, with torch.cat and multi_cast still banned."""
    dtype = torch.bfloat16
    m = _build(256, 4, dict(RECIPE, window_size=32, chunk_size=4))
    torch.manual_seed(89)
    B = 2
    x = torch.randn(64, B, 256, device="cuda")
    want = list(HELD_SPLIT if opt else HELD)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _init(m, kind, B, 128, dtype, S=64, hold_projections=True, **opt)
        st2 = _init(m, kind, B, 128, dtype, S=64, hold_projections=True, **opt)
        every = ("torch.cat", "F.linear", "_ops.multi_cast", "_ops.linear", "_ops.linear_wb")
        with _Calls() as calls:
            with monkeypatch.context() as mp:
                _ban(mp, every)
                for a, n in ((0, 1), (1, 8), (9, 1)):
                    calls.step()
                    m(x[a:a + n], x[a:a + n], x[a:a + n], incremental_state=st)
                graphs = []
                for n in (1, 8):                                 # warm-up on a side stream, then the capture
                    xin = x[:n].clone()
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    calls.step()
                    with torch.cuda.stream(s):
                        m(xin, xin, xin, incremental_state=st2)
                    torch.cuda.current_stream().wait_stream(s)
                    g = torch.cuda.CUDAGraph()
                    calls.step()
                    with torch.cuda.graph(g):
                        m(xin, xin, xin, incremental_state=st2)
                    graphs.append(g)
            assert calls.steps == [want] * 7, calls.steps
            with monkeypatch.context() as mp:
                _ban(mp, ("torch.cat", "_ops.multi_cast"))
                calls.step()
                m(x[10:45], x[10:45], x[10:45], incremental_state=st)
            assert calls.steps[-1] == list(STATIC), calls.steps[-1]
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
    assert m.decoding_positions(st).tolist() == [45] * B
    assert m.decoding_positions(st2).tolist() == [1 + 8 + 1 + 8] * B                 # the warm-ups, then one replay each


# ---- 4. capture and replay ----------------------------------------------------------------------------------------------------
def _stack_run(mods, x, P0, dtype, how, kind="rolling", reorder=None, order=None, idle=None, before=None, **opt):
    """A residual stack y = h + attn(h) on fresh states of `kind`: P0 tokens in one eager call, then single tokens, eagerly
    (how = "eager") or as one captured step replayed (a warm-up token on a side stream, the capture, replays).  reorder:
    before token `reorder` the states are permuted by `order` and the inputs from there on are x[:, order].  idle: a batch row
    flagged in every single-token step (per-sequence states).  before(states, t): called ahead of single token t, from the
    first one that a replay would produce.  -> rows [T - P0, B, C], states."""
    T, B = x.shape[:2]
    states = [_init(m, kind, B, T, dtype, **opt) for m in mods]
    mask = None
    if idle is not None:
        mask = torch.zeros(B, 1, dtype=torch.bool, device="cuda")
        mask[idle] = True

    def f(a, kpm=mask):
        h = a
        for m, st in zip(mods, states):
            h = h + m(h, h, h, key_padding_mask=kpm, incremental_state=st)[0]
        return h
    f(x[:P0], None)
    xr = x if order is None else x[:, order]
    xin = x[P0:P0 + 1].clone()
    rows, g = [], None
    if how == "eager":
        rows.append(f(xin).clone())
        t0 = P0 + 1
    else:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            rows.append(f(xin).clone())
        torch.cuda.current_stream().wait_stream(s)
        xin.copy_(x[P0 + 1:P0 + 2])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            yout = f(xin)
        g.replay()
        rows.append(yout.clone())
        t0 = P0 + 2
    for t in range(t0, T):
        if before is not None and t >= P0 + 2:
            before(states, t)
        if reorder is not None and t == reorder:
            for m, st in zip(mods, states):
                m.reorder_incremental_state(st, order)
        xin.copy_((xr if reorder is not None and t >= reorder else x)[t:t + 1])
        if g is None:
            rows.append(f(xin).clone())
        else:
            g.replay()
            rows.append(yout.clone())
    torch.cuda.synchronize()
    return torch.cat(rows, 0), states


def _two_layers():
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    return [_build(256, 4, aa, seed=3), _build(256, 4, aa, seed=4)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("mode", ["plain", "reorder", "per_seq_idle", "split"])
def test_captured_held_step_replays_equal_held_eager(dtype, mode):
    """Two layers, 23 tokens of prompt (69 rows: the library GEMM), then 97 replays of one captured 1-token held step on rings
    of 64 slots (lapped): bit for bit the eagerly decoded held rows and state; with a beam reorder at token 77; with
    per-sequence counts and a row that sits every replay out; with landmark splits."""
    mods = _two_layers()
    torch.manual_seed(97)
    T, B, P0 = 120, 3, 23
    x = torch.randn(T, B, 256, device="cuda")
    kw = dict(hold_projections=True)
    if mode == "reorder":
        kw.update(reorder=77, order=torch.tensor([2, 0, 0], device="cuda"))
    elif mode == "per_seq_idle":
        kw.update(per_sequence=True, idle=1)
    elif mode == "split":
        kw.update(landmark_splits=3)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eager, est = _stack_run(mods, x, P0, dtype, "eager", **kw)
        got, gst = _stack_run(mods, x, P0, dtype, "replay", **kw)
    assert _bits(got, eager), (got.float() - eager.float()).abs().max().item()
    for m, e, g in zip(mods, est, gst):
        eb, gb = m._get_input_buffer(e), m._get_input_buffer(g)
        assert gb["qkv"].shape[1] == 64
        for k in STATE_ROWS + ("w_qkv", "w_out"):
            assert _bits(eb[k], gb[k]), k
        assert not m.static_decoding_overflowed(g)
        assert m.decoding_positions(g).tolist() == ([T, P0, T] if mode == "per_seq_idle" else [T] * B)


# ---- 5. the weights are the state's ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_a_held_state_keeps_the_weights_it_was_made_with(kind):
    dtype = torch.bfloat16
    m = _build(256, 4, dict(RECIPE, window_size=32, chunk_size=4))
    torch.manual_seed(101)
    x = torch.randn(60, 2, 256, device="cuda")
    steps = (9, 1, 33)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        before, _ = _decode(m, x, steps, kind, dtype, hold_projections=True)
        st = _init(m, kind, 2, 60, dtype, hold_projections=True)
        m.q_proj.weight.data.mul_(1.5)
        m.out_proj.bias.data.add_(0.25)
        rows, t = [], 0
        for n in list(steps) + [1] * 60:
            if t >= 60:
                break
            rows.append(m(x[t:t + n], x[t:t + n], x[t:t + n], incremental_state=st)[0])
            t += n
        after, _ = _decode(m, x, steps, kind, dtype, hold_projections=True)
    assert all(_bits(a, b) for a, b in zip(before, rows))
    assert not _bits(torch.cat(after, 0), torch.cat(before, 0))          # (a state made after the change sees it)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [{}, dict(per_sequence=True, landmark_splits=2)], ids=["plain", "split_per_seq"])
def test_refresh_decoding_weights_reaches_a_captured_step(opt):
    """refresh on a fresh state = a state made after the change, bit for bit; a graph captured before the refresh replays
    with the new weights (equal to eager decoding that refreshed at the same token); every held pointer stays."""
    dtype = torch.bfloat16
    mods = _two_layers()
    torch.manual_seed(103)
    T, B, P0, change = 70, 2, 9, 40
    x = torch.randn(T, B, 256, device="cuda")
    saved = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in mods]

    def new_weights():
        for m in mods:
            m.q_proj.weight.data.mul_(1.25)
            m.v_proj.bias.data.add_(0.5)
            m.out_proj.weight.data.mul_(0.5)
            m.adaptive_mu_k[0].bias.data.add_(0.125)
            m.rel_pos_bias.relative_attention_bias.weight.data.mul_(0.5)

    def old_weights():
        for m, sd in zip(mods, saved):
            for k, v in m.state_dict().items():
                v.copy_(sd[k])

    ptrs = []

    def at_change(states, t):
        if t != change:
            return
        held = [[(k, v.data_ptr()) for k, v in m._get_input_buffer(st).items() if torch.is_tensor(v)] for m, st in zip(mods, states)]
        new_weights()
        for m, st in zip(mods, states):
            assert m.refresh_decoding_weights(st) is st
        now = [[(k, v.data_ptr()) for k, v in m._get_input_buffer(st).items() if torch.is_tensor(v)] for m, st in zip(mods, states)]
        assert now == held
        ptrs.append(now)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        old, _ = _stack_run(mods, x, P0, dtype, "eager", hold_projections=True, **opt)
        eager, _ = _stack_run(mods, x, P0, dtype, "eager", before=at_change, hold_projections=True, **opt)
        old_weights()
        got, gst = _stack_run(mods, x, P0, dtype, "replay", before=at_change, hold_projections=True, **opt)
        # ... and a refreshed fresh state next to one made after the change (the parameters are the new ones here)
        m = mods[0]
        old_weights()
        fresh = _init(m, "static", B, T, dtype, hold_projections=True, **opt)
        new_weights()
        m.refresh_decoding_weights(fresh)
        a = [m(x[t:t + n], x[t:t + n], x[t:t + n], incremental_state=fresh)[0] for t, n in ((0, 9), (9, 1), (10, 40), (50, 1))]
        b, _ = _decode(m, x[:51], (9, 1, 40, 1), "static", dtype, hold_projections=True, **opt)
    assert len(ptrs) == 2
    assert _bits(got, eager)
    k = change - P0                                              # rows of the tokens from `change` on
    assert _bits(eager[:k], old[:k]) and not _bits(eager[k:k + 1], old[k:k + 1])
    assert all(_bits(u, v) for u, v in zip(a, b))
    for mm, st in zip(mods, gst):
        buf = mm._get_input_buffer(st)
        assert torch.equal(buf["w_qkv"][:256], mm.q_proj.weight.detach().to(dtype))
        assert torch.equal(buf["b_out"], mm.out_proj.bias.detach().to(dtype))


# ---- 6. bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("opt", [{}, dict(per_sequence=True, landmark_splits=5)], ids=["plain", "split_per_seq"])
def test_a_held_state_is_the_plain_state_plus_its_projections(kind, opt):
    C = 256
    m = _build(C, 4, dict(RECIPE, window_size=32, chunk_size=4))
    B, T = 3, 500
    plain = _init(m, kind, B, T, torch.float16, **opt)
    off = _init(m, kind, B, T, torch.float16, hold_projections=False, **opt)
    held = _init(m, kind, B, T, torch.float16, hold_projections=True, **opt)
    pb, ob, hb = [m._get_input_buffer(s) for s in (plain, off, held)]
    assert set(ob) == set(pb) and set(hb) == set(pb) | set(HELD_KEYS)
    assert {k: (v.shape, v.dtype) for k, v in ob.items() if torch.is_tensor(v)} == {k: (v.shape, v.dtype) for k, v in pb.items() if torch.is_tensor(v)}
    assert m.get_incremental_state(off, "attn_static") == m.get_incremental_state(plain, "attn_static")
    assert m.get_incremental_state(held, "attn_static") == dict(m.get_incremental_state(plain, "attn_static"), hold_projections=True)
    assert m.decoding_state_nbytes(off) == m.decoding_state_nbytes(plain)
    assert m.decoding_state_nbytes(held) - m.decoding_state_nbytes(plain) == 2 * (3 * C * C + 3 * C + C * C + C) + 2 * 64 * 3 * C
    for k in HELD_KEYS:
        assert hb[k].dtype == torch.float16 and hb[k].is_contiguous() and hb[k].data_ptr() % 16 == 0 and not hb[k].requires_grad
    assert hb["proj_rows"].shape == (64, 3 * C)
    # a beam reorder and a row reset leave them alone
    kept = {k: hb[k].clone() for k in HELD_KEYS}
    m.reorder_incremental_state(held, torch.tensor([2, 0, 0], device="cuda"))
    if opt:
        m.reset_decoding_rows(held, [1])
    assert all(torch.equal(hb[k], kept[k]) for k in HELD_KEYS)


# ---- 7. overflow ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_held_per_sequence_overflow_is_per_row(kind):
    """cap = 64; rows 0 and 1 took 30 tokens of the right-padded prompt, row 2 all 60: a held step of 8 tokens overflows row
    2 alone -- NaN rows, status 1, its count kept -- and rows 0, 1 stay prefix consistent."""
    dtype = torch.bfloat16
    m = _build(256, 4, dict(RECIPE, window_size=32, chunk_size=4))
    torch.manual_seed(107)
    B, C = 3, 256
    x, xn = torch.randn(60, B, C, device="cuda"), torch.randn(8, B, C, device="cuda")
    mask = torch.zeros(B, 60, dtype=torch.bool, device="cuda")
    mask[:2, 30:] = True
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _init(m, kind, B, 64, dtype, S=64, per_sequence=True, hold_projections=True)
        m(x, x, x, key_padding_mask=mask, incremental_state=st)
        with _Calls() as calls:
            calls.step()
            y = m(xn, xn, xn, incremental_state=st)[0]
        seq = torch.cat([x[:30, :2], xn[:, :2]], 0)
        full, _ = m(seq, seq, seq)
    assert calls.steps == [list(HELD)]
    assert torch.isnan(y[:, 2]).all() and torch.isfinite(y[:, :2]).all()
    assert m.static_decoding_overflowed_rows(st).tolist() == [False, False, True]
    assert m._get_input_buffer(st)["status"].tolist() == [0, 0, 1]
    assert m.decoding_positions(st).tolist() == [38, 38, 60]
    _check_full(y[:, :2], full[30:], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_held_shared_count_overflow_raises_before_the_first_launch(kind):
    dtype = torch.bfloat16
    m = _build(256, 4, dict(RECIPE, window_size=32, chunk_size=4))
    x = torch.randn(60, 2, 256, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _init(m, kind, 2, 64, dtype, S=64, hold_projections=True)
        m(x, x, x, incremental_state=st)
        with _Calls() as calls:
            calls.step()
            with pytest.raises(RuntimeError, match="static decoding state is full"):
                m(x[:8], x[:8], x[:8], incremental_state=st)
            assert calls.steps == [[]]                           # the projection included
            calls.step()
            m(x[:4], x[:4], x[:4], incremental_state=st)
        assert calls.steps[-1] == list(HELD)
    assert m.decoding_positions(st).tolist() == [64, 64] and not m.static_decoding_overflowed(st)
