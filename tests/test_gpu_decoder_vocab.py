"""-m gpu: the greedy token pick on a held vocabulary table (csrc/ea_ceva_decode_vocab.hip, ea_ceva_sdecode_vocab_argmax,
C ABI 26) and the `hold_vocab` option of ea_harness.sequence.DecoderStack (`next_tokens`, `generate`).

Kernel, at the shapes of decoder_vocab_operands.SHAPES, bf16 and fp16 tables, x in fp32 and in the table's type; x sits in a
NaN-framed buffer with a row stride of K + 8, the table in a buffer whose rows behind V are NaN rows and rows (+inf, 0, 0, ..)
-- a +inf logit in every row of x, were they read -- and the logits in a buffer of sevens with a row stride of V + 8:

 1. logits: the bits of ea_ceva_sdecode_linear (no bias) on the same x and the table padded with zero rows to a multiple of
    16, as fp32 and as the table's type; nothing outside [M, V] is written.
 2. the pick: token[m] == torch.argmax(ref32[m, :V]) and top[m] has the bits of ref32[m, token[m]], ref32 being 1's fp32
    reference, for every row of every shape; the same tokens with logits = NULL.
 3. ties (decoder_vocab_operands.tie; its precondition is checked in fp64 by tests/test_decoder_vocab_cpu.py): token == a in every
    row, logit[:, a] bit-equal to logit[:, b].
 4. NaN: a NaN table row v* is picked in every row; of two, the lower.
 5. fp64 at the LM shapes: L64[m, token[m]] >= max_v L64[m, v] - 2 bound[m], L64 = x^ w^T in fp64 on the host from the rounded
    operands, bound[m] = (K + 8) 2^-24 max_v sum_k |x^_k w_vk| (K + 8 fp32 additions in any order; the products of two bf16
    or two fp16 values are exact in fp32).  The largest |logit - L64| / bound is printed.

Stack (vocab 1000, embed 128, 2 heads of 64, ffn 256, 2 layers, window 16, chunks of 4 -- the geometry of
tests/test_gpu_decoder_stack.py with a vocabulary that is no multiple of 16; B = 3, a 17-token prompt, 28 new tokens):
 6a. generate by capture and replay == generate eagerly, tokens and rows bit for bit, on a state with hold_vocab;
 6b. every generated token satisfies 5's inequality against fp64 logits of the row it was picked from and the held table;
 6c. the captured step runs with F.linear, torch.addmm, torch.matmul, torch.argmax and Tensor.argmax replaced by functions
     that raise -- written out as generate writes it, and generate(graph=True) itself from the end of its prefill on; 6d. an in-place change of embed_tokens.weight reaches a captured pick only after refresh_decoding_weights;
 6e. next_tokens on 130 rows == row-wise calls; 6f. the bytes of the option; 6g. a state made without it."""
import functools
import os
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import decoder_vocab_operands as ops                                                # noqa: E402
from ceva_decoding import _Calls, _ctx                                              # noqa: E402

LINEAR, VOCAB_FN = "ea_ceva_sdecode_linear", "ea_ceva_sdecode_vocab_argmax"
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
SHAPES = ops.SHAPES
_ids = lambda shapes: ["%dx%dx%d" % s for s in shapes]                              # noqa: E731


def _bits(a, b):
    """Equal bit for bit (an integer view of the same width: any strides, a NaN equals itself, -0 differs from +0)."""
    as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int))


def _code(t):
    from efficient_attention import _native as nv
    return nv.EA_F32 if t.dtype == torch.float32 else nv.io_dtype(t)


def _rows(M, K, ld, dtype, values):
    """[M + 1, ld] of NaN with `values` [M, K] in front: what lies beside and below the operand is not read."""
    buf = torch.full((M + 1, ld), float("nan"), dtype=dtype, device="cuda")
    buf[:M, :K] = values
    return buf


def _table(w):
    """[V + 18, K]: w, and behind it NaN rows and rows (+inf, 0, 0, ..) in turn -- a column tile that reaches past V must
    neither read them (it would pick them: x[:, 0] > 0) nor pick the columns they stand for."""
    V, K = w.shape
    buf = torch.zeros((V + 18, K), dtype=w.dtype, device="cuda")
    buf[:V] = w
    buf[V::2] = float("nan")
    buf[V + 1::2, 0] = float("inf")
    return buf


def _pick(M, K, V, xbuf, wbuf, logits=None, top=True):
    """-> token [M] int64, top [M] fp32 (or None); xbuf, logits: 2-D buffers whose row stride is the leading dimension."""
    from efficient_attention import _native as nv
    nbytes = nv.lib().ea_ceva_sdecode_vocab_ws(M, V)
    assert nbytes == 8 * M * ((V + 15) // 16)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")                # (stale candidates would be NaNs)
    token = torch.full((M + 1,), -7, dtype=torch.long, device="cuda")
    t = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda") if top else None
    nv.call(VOCAB_FN, M, K, V, nv.ptr(xbuf), _code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf), nv.ptr(logits),
            0 if logits is None else _code(logits), 0 if logits is None else logits.stride(0), nv.ptr(ws), nbytes,
            nv.ptr(token), nv.ptr(t), nv.stream())
    torch.cuda.synchronize()
    assert token[M].item() == -7 and (t is None or t[M].item() == 7.0)
    return token[:M], (None if t is None else t[:M])


def _logit_buffer(M, V, dtype):
    return torch.full((M + 3, V + 8), 7.0, dtype=dtype, device="cuda")


def _reference(M, K, V, xbuf, w):
    """ea_ceva_sdecode_linear, no bias, on the table padded with zero rows -> (fp32 [M, V], the table's type [M, V])."""
    from efficient_attention import _native as nv
    Vp = (V + 15) // 16 * 16
    wp = torch.zeros((Vp, K), dtype=w.dtype, device="cuda")
    wp[:V] = w
    out = []
    for ydtype in (torch.float32, w.dtype):
        y = torch.empty((M, Vp), dtype=ydtype, device="cuda")
        nv.call(LINEAR, M, K, Vp, nv.ptr(xbuf), _code(xbuf), xbuf.stride(0), nv.ptr(wp), nv.io_dtype(wp), None, nv.ptr(y),
                _code(y), Vp, nv.stream())
        out.append(y[:, :V])
    torch.cuda.synchronize()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _case(shape, wdtype, x_f32):
    """The operands of a shape on the device and the plain kernel's logits, computed once and shared (never written)."""
    M, K, V = shape
    x32, w = ops.operands(shape, wdtype, 0)
    xbuf = _rows(M, K, K + 8, torch.float32 if x_f32 else wdtype, x32.cuda() if x_f32 else x32.to(wdtype).cuda())
    w = w.cuda()
    ref32, ref16 = _reference(M, K, V, xbuf, w)
    return xbuf, _table(w), ref32, ref16


# ---- 1. the logits are the plain kernel's bits ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_logits_are_the_plain_kernels_bits(wdtype, shape):
    M, K, V = shape
    for x_f32 in (True, False):
        xbuf, wbuf, ref32, ref16 = _case(shape, wdtype, x_f32)
        assert torch.isfinite(ref32).all()
        for ref in (ref32, ref16):
            logits = _logit_buffer(M, V, ref.dtype)
            _pick(M, K, V, xbuf, wbuf, logits)
            assert _bits(logits[:M, :V], ref), (shape, wdtype, x_f32, ref.dtype)
            assert (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()


# ---- 2. the pick is exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_the_pick_is_argmax_of_the_fp32_logits_in_every_row(wdtype, shape):
    M, K, V = shape
    for x_f32 in (True, False):
        xbuf, wbuf, ref32, _ = _case(shape, wdtype, x_f32)
        want = torch.argmax(ref32, dim=1)
        for logits in (_logit_buffer(M, V, torch.float32), _logit_buffer(M, V, wdtype), None):
            token, top = _pick(M, K, V, xbuf, wbuf, logits)
            assert torch.equal(token, want), (shape, wdtype, x_f32, token.tolist(), want.tolist())
            assert _bits(top, ref32.gather(1, want.unsqueeze(1)).squeeze(1)), (shape, wdtype, x_f32)
        token, top = _pick(M, K, V, xbuf, wbuf, None, top=False)
        assert top is None and torch.equal(token, want)


# ---- 3. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_of_two_equal_logits_the_lower_index_wins(wdtype, shape):
    M, K, V = shape
    ran = []
    for case in ops.TIE_CASES:
        got = ops.tie(shape, wdtype, 0, case)
        if got is None:                              # (the single-tile shape has no pair in two tiles)
            continue
        x32, w, a, b = got
        ran.append(case)
        wbuf = _table(w.cuda())
        for x_f32 in (True, False):
            xbuf = _rows(M, K, K + 8, torch.float32 if x_f32 else wdtype, x32.cuda() if x_f32 else x32.to(wdtype).cuda())
            logits = _logit_buffer(M, V, torch.float32)
            token, top = _pick(M, K, V, xbuf, wbuf, logits)
            assert token.tolist() == [a] * M, (shape, wdtype, case, x_f32, a, b, token.tolist())
            assert _bits(logits[:M, a], logits[:M, b]) and _bits(top, logits[:M, a])
            token, _ = _pick(M, K, V, xbuf, wbuf, None)
            assert token.tolist() == [a] * M
    assert ran == ops.TIE_CASES or (V == 16 and ran == ["one_tile", "ends"]), ran


# ---- 4. NaN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_a_nan_logit_is_picked_and_of_two_the_lower_index(wdtype, shape):
    M, K, V = shape
    for two in (False, True):
        _, w, rows = ops.nan_rows(shape, wdtype, 0, two)
        wbuf = _table(w.cuda())
        for x_f32 in (True, False):
            xbuf = _case(shape, wdtype, x_f32)[0]
            for logits in (_logit_buffer(M, V, torch.float32), None):
                token, top = _pick(M, K, V, xbuf, wbuf, logits)
                assert token.tolist() == [rows[0]] * M, (shape, wdtype, x_f32, rows, token.tolist())
                assert torch.isnan(top).all()
                if logits is not None:
                    assert torch.equal(torch.isnan(logits[:M, :V]).nonzero()[:, 1].unique().cpu(), torch.tensor(rows))
                    assert torch.equal(torch.argmax(logits[:M, :V].cpu(), dim=1), token.cpu())   # torch.argmax's own rule


# ---- 5. fp64 at the LM shapes -----------------------------------------------------------------------------------------------------
def _excess_and_slack(xh, table, token, logits=None):
    """-> (min over rows of L64[m, token] - max L64[m] + 2 bound[m], max |logits - L64| / bound or None); fp64 on the host."""
    xh, table = xh.cpu(), table.cpu()
    L = xh.double() @ table.double().t()
    bound = ops.bound(xh, table)
    picked = L.gather(1, token.cpu().view(-1, 1)).squeeze(1)
    slack = (picked - L.max(1).values + 2.0 * bound).min().item()
    worst = None if logits is None else ((logits.cpu().double() - L).abs() / bound.unsqueeze(1)).max().item()
    return slack, worst


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", ops.LM, ids=_ids(ops.LM))
def test_pick_against_fp64_at_the_lm_shapes(wdtype, shape):
    M, K, V = shape
    for x_f32 in (True, False):
        xbuf, wbuf, _, _ = _case(shape, wdtype, x_f32)
        logits = _logit_buffer(M, V, torch.float32)
        token, _ = _pick(M, K, V, xbuf, wbuf, logits)
        slack, worst = _excess_and_slack(xbuf[:M, :K].to(wdtype), wbuf[:V], token, logits[:M, :V])
        print(shape, wdtype, "x fp32" if x_f32 else "x 16-bit",
              "largest |logit - L64| / bound: %.4f; min (L64[token] - max L64 + 2 bound): %.3e" % (worst, slack))
        assert slack >= 0.0, (shape, wdtype, x_f32, slack)
        assert worst <= 1.0, (shape, wdtype, x_f32, worst)          # (the bound itself: K + 8 fp32 additions)


# ---- 6. the stack -----------------------------------------------------------------------------------------------------------------
ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
C, FFN, HEADS, LAYERS, VOCAB, B, T, P0 = 128, 256, 2, 2, 1000, 3, 45, 17
WS_BYTES = 8 * 64 * ((VOCAB + 15) // 16)


@functools.lru_cache(maxsize=None)
def _stack():
    """Embedding rows scaled by 1 / 32, as tests/test_gpu_decoder_stack.py's _lively_stack: with rows of the initial size a
    token's own embedding decides the tied logits and greedy decoding repeats one token for ever."""
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(7)
    m = DecoderStack(VOCAB, C, FFN, HEADS, LAYERS, ATTN).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        for layer in m.layers:
            layer.self_attn.rel_pos_bias.relative_attention_bias.weight.mul_(20.0)
        m.embed_tokens.weight.mul_(1.0 / 32)
    return m.eval()


@functools.lru_cache(maxsize=None)
def _tokens():
    g = torch.Generator().manual_seed(11)
    return torch.randint(2, VOCAB, (B, T), generator=g).cuda()


def _ban(monkeypatch):
    """tests/test_gpu_decoder_stack.py's _ban, and the two spellings of argmax."""
    def banned(name):
        def f(*a, **k):
            raise AssertionError("%s reached in a held step of at most 64 rows" % name)
        return f
    for mod, name in ((F, "linear"), (torch, "addmm"), (torch, "matmul"), (torch, "argmax"), (torch.Tensor, "argmax")):
        monkeypatch.setattr(mod, name, banned(name))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "static", "per_sequence_ragged"])
def test_generate_on_a_held_table_replayed_equals_eager_and_picks_within_the_bound(case):
    dtype = torch.bfloat16
    m = _stack()
    prompt = _tokens()[:, :P0].clone()
    opt = dict(rolling=case != "static", hold_vocab=True)
    if case == "per_sequence_ragged":
        opt["per_sequence"] = True
        for b, n in enumerate([17, 9, 1]):
            prompt[b, n:] = m.pad_idx
    n_new = T - P0
    out = {}
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for graph in (False, True):
            st = m.init_decoding(B, T, dtype, "cuda", **opt)
            assert st.hold_vocab and st.hold_weights and torch.equal(st.vocab, m.embed_tokens.weight.detach().to(dtype))
            with _Calls() as calls:
                calls.step()
                out[graph] = m.generate(prompt, n_new, st, graph=graph, return_rows=True) + (st,)
            # the first token, then eagerly one pick per step; captured: the warm-up and the capture
            assert calls.all().count(VOCAB_FN) == (3 if graph else n_new), calls.all().count(VOCAB_FN)
    (tok_e, rows_e, _), (tok_g, rows_g, st) = out[False], out[True]
    assert tuple(tok_g.shape) == (B, n_new) and tok_g.dtype == torch.long and tuple(rows_g.shape) == (n_new, B, C)
    assert torch.equal(tok_g, tok_e) and _bits(rows_g, rows_e)                                        # 6a
    print(case, "tokens", tok_g.tolist())
    assert (tok_g[:, 1:] != tok_g[:, :-1]).any()                        # (a stale input token would show)
    assert int(tok_g.min()) >= 0 and int(tok_g.max()) < VOCAB
    # 6b: token [b, i] was picked from rows[i, b]
    xh = rows_g.reshape(n_new * B, C).to(dtype)
    slack, _ = _excess_and_slack(xh, st.vocab, tok_g.t().reshape(-1))
    print(case, "min (L64[token] - max L64 + 2 bound) over %d picks: %.3e" % (n_new * B, slack))
    assert slack >= 0.0, slack


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_the_captured_generate_step_launches_no_framework_gemm_and_no_argmax(kind, monkeypatch):
    """generate's step -- decode, the pick, the token written into the step's input -- eagerly, on a side stream and under
    capture, with F.linear, torch.addmm, torch.matmul, torch.argmax and Tensor.argmax replaced by functions that raise; the
    replays give the tokens of the eager loop."""
    dtype = torch.bfloat16
    m = _stack()
    tokens = _tokens().t()

    def fed(n_steps, capture):
        st = m.init_decoding(B, T, dtype, "cuda", rolling=kind == "rolling", hold_weights=True, hold_vocab=True)
        picked = []
        with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            last = m.decode(tokens[:P0], st)[-1:]
            with _Calls() as calls, monkeypatch.context() as mp:
                _ban(mp)
                calls.step()
                tok_in = m.next_tokens(last, st)
                assert calls.steps[-1] == [VOCAB_FN]
                picked.append(tok_in.clone())

                def step():
                    m.next_tokens(m.decode(tok_in, st), st, out=tok_in)

                def launched():                      # one step: every layer's two projections, and the pick last
                    names = calls.steps[-1]
                    assert names[-1] == VOCAB_FN and names.count(VOCAB_FN) == 1 and names.count(LINEAR) == 2 * LAYERS, names
                if capture:
                    s = torch.cuda.Stream()          # the first step eagerly on a side stream: the warm-up
                    s.wait_stream(torch.cuda.current_stream())
                    calls.step()
                    with torch.cuda.stream(s):
                        step()
                    torch.cuda.current_stream().wait_stream(s)
                    launched()
                    picked.append(tok_in.clone())
                    g = torch.cuda.CUDAGraph()
                    calls.step()
                    with torch.cuda.graph(g):
                        step()
                    launched()
                    for _ in range(1, n_steps):
                        g.replay()
                        picked.append(tok_in.clone())
                else:
                    for _ in range(n_steps):
                        calls.step()
                        step()
                        launched()
                        picked.append(tok_in.clone())
            torch.cuda.synchronize()
        return torch.cat(picked, 0)
    eager, replayed = fed(8, False), fed(8, True)
    assert torch.equal(eager, replayed), (eager.tolist(), replayed.tolist())
    assert (eager[1:] != eager[:-1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_generate_itself_runs_its_steps_under_the_ban(kind, monkeypatch):
    """`DecoderStack.generate(graph=True)` on held weights and a held table, its own code: the five functions raise from the
    moment the prompt's prefill is over -- `generate` calls `next_tokens` for the first token right behind it, and that call
    arms the ban -- through the first pick, the scratch state, the warm-up, the capture and every replay.  (A prompt of 51
    rows may run library GEMMs in the attention's prefill, as in tests/test_gpu_decoder_stack.py.)"""
    dtype = torch.bfloat16
    m = _stack()
    prompt = _tokens()[:, :P0].clone()
    n_new = 8
    armed = []
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = m.init_decoding(B, T, dtype, "cuda", rolling=kind == "rolling", hold_weights=True, hold_vocab=True)
        want = m.generate(prompt, n_new, st, graph=True)
        st = m.init_decoding(B, T, dtype, "cuda", rolling=kind == "rolling", hold_weights=True, hold_vocab=True)

        def gated(name, real):
            def f(*a, **k):
                if armed:
                    raise AssertionError("%s reached in generate behind the prefill" % name)
                return real(*a, **k)
            return f
        for mod, name in ((F, "linear"), (torch, "addmm"), (torch, "matmul"), (torch, "argmax"), (torch.Tensor, "argmax")):
            monkeypatch.setattr(mod, name, gated(name, getattr(mod, name)))
        real_next = m.next_tokens

        def arming(*a, **k):
            armed.append(True)
            return real_next(*a, **k)
        monkeypatch.setattr(m, "next_tokens", arming)
        try:
            got = m.generate(prompt, n_new, st, graph=True)
            torch.cuda.synchronize()
        finally:
            n_calls = len(armed)
            del armed[:]
    assert n_calls == 3                                  # the first token, the warm-up, the capture
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_refresh_reaches_a_captured_pick_and_only_refresh_does():
    dtype = torch.bfloat16
    m = _stack()
    w = m.embed_tokens.weight
    saved = w.detach().clone()
    g0 = torch.Generator().manual_seed(3)
    fixed = torch.randn(1, B, C, generator=g0).cuda()
    try:
        with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            st = m.init_decoding(B, T, dtype, "cuda", hold_vocab=True)
            m.decode(_tokens().t()[:P0], st)
            xin = _tokens().t()[P0:P0 + 1].clone()
            tok_in = torch.zeros_like(xin)

            def step():
                m.next_tokens(m.decode(xin, st), st, out=tok_in)
                return m.next_tokens(fixed, st, return_logits=True)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step()
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                tok, logits = step()
            ptr = st.vocab.data_ptr()
            g.replay()
            old = (tok.clone(), logits.clone())
            assert tuple(logits.shape) == (1, B, VOCAB) and logits.dtype == torch.float32
            assert torch.equal(old[0], old[1].argmax(-1))
            w.copy_(saved.flip(0))                                      # every row moves: the picks move with them
            g.replay()
            kept = (tok.clone(), logits.clone())
            assert torch.equal(kept[0], old[0]) and _bits(kept[1], old[1])           # no refresh: the old table
            assert m.refresh_decoding_weights(st) is st and st.vocab.data_ptr() == ptr
            assert torch.equal(st.vocab, saved.flip(0).to(dtype))
            g.replay()
            new = (tok.clone(), logits.clone())
            torch.cuda.synchronize()
            assert not _bits(new[1], old[1]) and _bits(new[1], old[1].flip(-1))       # the same sums at the mirrored indices
            assert torch.equal(new[0], new[1].argmax(-1)) and not torch.equal(new[0], old[0])
            eager = m.next_tokens(fixed, st, return_logits=True)
            assert torch.equal(eager[0], new[0]) and _bits(eager[1], new[1])
    finally:
        with torch.no_grad():
            w.copy_(saved)


@pytest.mark.gpu
def test_next_tokens_on_130_rows_equals_row_wise_calls():
    dtype = torch.float16
    m = _stack()
    st = m.init_decoding(2, 8, dtype, "cuda", hold_weights=False, hold_vocab=True)
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(65, 2, C, generator=g).cuda()
    for r in (rows, rows.to(dtype), rows.to(torch.bfloat16)):             # (bf16 rows on an fp16 table: widened to fp32)
        tok, logits = m.next_tokens(r, st, return_logits=True)
        assert tuple(tok.shape) == (65, 2) and tok.dtype == torch.long and tuple(logits.shape) == (65, 2, VOCAB)
        out = torch.full((65, 2), -1, dtype=torch.long, device="cuda")
        assert m.next_tokens(r, st, out=out) is out and torch.equal(out, tok)
        assert torch.equal(tok, logits.argmax(-1))
        for t in range(65):
            for b in range(2):
                one, l1 = m.next_tokens(r[t:t + 1, b:b + 1], st, return_logits=True)
                assert one.item() == tok[t, b].item() and _bits(l1[0, 0], logits[t, b]), (t, b)
    with pytest.raises(ValueError, match="contiguous int64"):
        m.next_tokens(rows, st, out=torch.zeros(65, 2, dtype=torch.int32, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
@pytest.mark.parametrize("hold_weights", [False, True], ids=["plain", "held_weights"])
def test_the_option_adds_the_table_and_the_workspace_and_nothing_else(kind, hold_weights):
    m = _stack()
    dtype = torch.float16
    opt = dict(rolling=kind == "rolling", hold_weights=hold_weights, per_sequence=True, landmark_splits=3)
    without = m.init_decoding(B, 500, dtype, "cuda", **opt)
    explicit = m.init_decoding(B, 500, dtype, "cuda", hold_vocab=False, **opt)
    held = m.init_decoding(B, 500, dtype, "cuda", hold_vocab=True, **opt)
    # 6g: a state made without the option
    for st in (without, explicit):
        assert st.vocab is None and st.vocab_ws is None and not st.hold_vocab and st.hold_weights == hold_weights
        assert m.decoding_state_nbytes(st) == m.decoding_state_nbytes(without)
        with pytest.raises(RuntimeError, match="hold_vocab=True"):
            m.next_tokens(torch.zeros(1, B, C, device="cuda"), st)
    assert sorted(vars(without)) == sorted(vars(held)) == ["ffn", "incremental", "options", "vocab", "vocab_ws"]
    attention = sum(layer.self_attn.decoding_state_nbytes(without.incremental) for layer in m.layers)
    ffn = LAYERS * 2 * (C * FFN + FFN + FFN * C + C) if hold_weights else 0
    assert m.decoding_state_nbytes(without) == attention + ffn                                       # what it is today
    # 6f
    assert m.decoding_state_nbytes(held) - m.decoding_state_nbytes(without) == 2 * VOCAB * C + WS_BYTES
    assert held.vocab.dtype == dtype and tuple(held.vocab.shape) == (VOCAB, C) and held.vocab.is_contiguous()
    assert held.vocab.data_ptr() % 16 == 0 and held.vocab_ws.data_ptr() % 16 == 0 and not held.vocab.requires_grad
    assert held.vocab_ws.numel() * held.vocab_ws.element_size() == WS_BYTES
    assert torch.equal(held.vocab, m.embed_tokens.weight.detach().to(dtype))
    # a beam reorder and a row reset have nothing of the table to move
    kept = held.vocab.clone()
    m.reorder_decoding_state(held, torch.tensor([2, 0, 0], device="cuda"))
    m.reset_decoding_rows(held, [1])
    assert torch.equal(kept, held.vocab)
