"""-m gpu: the sampled token pick on a held vocabulary table (csrc/ea_ceva_decode_vocab.hip, ea_ceva_sdecode_vocab_sample,
C ABI 27) and DecoderStack.init_sampling / sample_tokens / generate on a state with a sampler.

Kernel, at the six small shapes of decoder_vocab_operands.SHAPES and (1, 1024, 32768) once, bf16 and fp16 tables, x in fp32
and in the table's type, top_k in {1, 5, 16, 40, 64}; the operands sit in the framed buffers of tests/test_gpu_decoder_vocab.py
(a NaN-framed x, a table followed by NaN and +inf rows, logits in a buffer of sevens):

 1. logits: bit-equal to ea_ceva_sdecode_vocab_argmax's fp32 logits on the same operands; nothing outside [M, V] is written.
 2. selection: sel_idx / sel_val equal the host's top-k' of those stored logits under the total order
    (decoder_sample_reference.topk), sel_val with the stored logit's bits, k' = min(k, V); entries from k' on are not written.
    On the plain operands and on constructed tables: all k best in one tile, one in each of k tiles (the tail tile among
    them), a table of three rows repeated (the lowest columns win), the `tie` operands with k = 1 (index a wins).
 3. k = 1 is greedy: token == ea_ceva_sdecode_vocab_argmax's token in every row, whatever top_p and the temperature are.
 4. the draw: T in {0.7, 1.0}, top_p in {1.0, 0.9}, 64 consecutive counters per row (64 calls on one ctr buffer): from the
    kernel's own sel_val the host forms c_j in fp64 and allows eps = k' 2^-20 c_{k'-1} (decoder_sample_reference); kept must
    be an n the rule allows, the token sel_idx[j] of a j with c_{j-1} - eps <= u c_{kept-1} < c_j + eps, u from (seed, ctr, sid)
    on the host; ctr ends 64 higher; at least 95 % of a case's draws have exactly one admissible j.
 5. a NaN table row, and a +inf logit: that index, kept = 0, the counter advances.
 6. independence: a batch of 3 rows == three single-row calls with the same (sid, ctr); two rows with one x and sid and ctr
    one apart give each other's stream shifted by one.
 7. the stack (the geometry of tests/test_gpu_decoder_vocab.py, k = 8, top_p = 0.9, T = 0.8; rolling, static, ragged
    per-sequence): generate replayed == eager, tokens and rows bit for bit; every token passes 4 against its row; the same seed
    reproduces, another differs; the steps run with the framework's GEMMs, argmax, multinomial, topk and softmax banned;
    reorder_decoding_state and reset_decoding_rows move and restart the streams; a state without a sampler is greedy as before."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_decoder_vocab as tv                    # the framed buffers, the shared operands, the stack
import decoder_sample_operands as sops
import decoder_sample_reference as ref
import decoder_vocab_operands as ops
from ceva_decoding import _Calls, _ctx

SAMPLE_FN = "ea_ceva_sdecode_vocab_sample"
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
SHAPES = sops.SHAPES
_ids = tv._ids
SEED = sops.SEED


def _sample(M, K, V, xbuf, wbuf, k, top_p=1.0, temperature=1.0, seed=SEED, ctr=None, sid=None, logits=None, calls=1,
            details=True):
    """`calls` consecutive calls on one ctr buffer -> dict(token [calls, M], kept [calls, M], sel_idx / sel_val [M, k] (of
    the last call), logits (the framed buffer), ctr).  Every output has a guard row or frame that must stay what it was."""
    from efficient_attention import _native as nv
    nbytes = nv.lib().ea_ceva_sdecode_vocab_sample_ws(M, V)
    assert nbytes == 8 * M * ((V + 15) // 16)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    logits = tv._logit_buffer(M, V, torch.float32) if logits is None else logits
    ctr = torch.zeros(M, dtype=torch.long, device="cuda") if ctr is None else ctr
    sid = torch.arange(M, dtype=torch.int32, device="cuda") if sid is None else sid
    cbuf = torch.cat([ctr, torch.full((1,), -7, dtype=torch.long, device="cuda")])
    token = torch.full((calls, M + 1), -7, dtype=torch.long, device="cuda")
    kept = torch.full((calls, M + 1), -7, dtype=torch.int32, device="cuda")
    sel_idx = torch.full((M + 1, k), -7, dtype=torch.int32, device="cuda")
    sel_val = torch.full((M + 1, k), 7.0, dtype=torch.float32, device="cuda")
    for i in range(calls):
        nv.call(SAMPLE_FN, M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf),
                nv.ptr(logits), logits.stride(0), nv.ptr(ws), nbytes, k, top_p, temperature, seed, nv.ptr(cbuf), nv.ptr(sid),
                nv.ptr(token[i]), nv.ptr(sel_idx) if details else None, nv.ptr(sel_val) if details else None,
                nv.ptr(kept[i]) if details else None, nv.stream())
    torch.cuda.synchronize()
    assert (token[:, M] == -7).all() and (kept[:, M] == -7).all() and cbuf[M].item() == -7
    assert (sel_idx[M] == -7).all() and (sel_val[M] == 7.0).all()
    assert (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()
    kk = min(k, V)
    assert (sel_idx[:M, kk:] == -7).all() and (sel_val[:M, kk:] == 7.0).all()          # entries from k' on are not written
    if not details:
        assert (sel_idx == -7).all() and (kept == -7).all()
    return dict(token=token[:, :M], kept=kept[:, :M], sel_idx=sel_idx[:M, :kk], sel_val=sel_val[:M, :kk], logits=logits,
                ctr=cbuf[:M])


def _xbuf(x32, wdtype, x_f32):
    M, K = x32.shape
    return tv._rows(M, K, K + 8, torch.float32 if x_f32 else wdtype, x32.cuda() if x_f32 else x32.to(wdtype).cuda())


def _check_selection(got, M, V, k, what):
    """sel_idx / sel_val against the host's top-k' of the stored logits; sel_val has the stored logit's bits."""
    L = got["logits"][:M, :V].cpu()
    Ln = L.numpy()
    sel_idx, sel_val = got["sel_idx"].cpu(), got["sel_val"].cpu()
    for m in range(M):
        want = ref.topk(Ln[m], k)
        assert sel_idx[m].tolist() == want.tolist(), (what, m, sel_idx[m].tolist(), want.tolist())
        assert tv._bits(sel_val[m], L[m][torch.from_numpy(want)]), (what, m)


def _check_draws(got, M, k, top_p, temperature, seed, ctr0, sid, what):
    """4: every draw of every call; -> the share of draws with exactly one admissible j."""
    token, kept = got["token"].cpu().numpy(), got["kept"].cpu().numpy()
    sel_idx, sel_val = got["sel_idx"].cpu().numpy(), got["sel_val"].cpu().numpy()
    calls = token.shape[0]
    ctr0, sid = np.asarray(ctr0, dtype=np.int64), np.asarray(sid, dtype=np.int64)
    u = ref.uniform(seed, ctr0.reshape(1, M) + np.arange(calls).reshape(calls, 1), sid.reshape(1, M))
    one = 0
    for m in range(M):
        c = ref.cumulative(sel_val[m], temperature)
        allowed = ref.admissible_kept(c, top_p)
        assert np.isin(kept[:, m], allowed).all(), (what, m, kept[:, m].tolist(), allowed)
        ok = ref.admissible_mask(c, kept[:, m], u[:, m])                   # [calls, k']
        at = token[:, m].reshape(calls, 1) == sel_idx[m].reshape(1, -1)     # the j a token stands for (columns are distinct)
        bad = np.nonzero(~(ok & at).any(1))[0]
        assert bad.size == 0, (what, m, bad.tolist(), token[bad, m].tolist(), u[bad, m].tolist(), kept[bad, m].tolist())
        one += int((ok.sum(1) == 1).sum())
    assert got["ctr"].cpu().tolist() == (ctr0 + calls).tolist(), what
    return one / (calls * M)


# ---- 1, 2, 3: logits, selection, k = 1 --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_logits_selection_and_the_greedy_case(wdtype, shape):
    M, K, V = shape
    for x_f32 in (True, False):
        xbuf, wbuf, _, _ = tv._case(shape, wdtype, x_f32)
        greedy_logits = tv._logit_buffer(M, V, torch.float32)
        greedy, _ = tv._pick(M, K, V, xbuf, wbuf, greedy_logits)
        for k in sops.KS:
            got = _sample(M, K, V, xbuf, wbuf, k, 0.9, 0.7)
            assert tv._bits(got["logits"], greedy_logits), (shape, wdtype, x_f32, k)             # 1 (frame and all)
            _check_selection(got, M, V, k, (shape, wdtype, x_f32, k))                             # 2
            assert tuple(got["sel_idx"].shape) == (M, min(k, V))
        for top_p, temperature in ((1.0, 1.0), (0.9, 0.7), (1e-3, 100.0), (1.0, 1e-2)):            # 3
            got = _sample(M, K, V, xbuf, wbuf, 1, top_p, temperature, details=top_p != 1.0)
            assert torch.equal(got["token"][0], greedy), (shape, wdtype, x_f32, top_p, temperature)
            assert top_p == 1.0 or (got["kept"] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_selection_on_constructed_tables(wdtype, shape):
    M, K, V = shape
    ran = []
    for k in sops.KS:
        for name, make in (("one_tile", sops.one_tile), ("spread", sops.spread)):
            made = make(shape, wdtype, k)
            if made is None:
                continue
            x32, w, cols = made
            ran.append((name, k))
            wbuf = tv._table(w.cuda())
            for x_f32 in (True, False):
                got = _sample(M, K, V, _xbuf(x32, wdtype, x_f32), wbuf, k)
                _check_selection(got, M, V, k, (name, shape, wdtype, x_f32, k))
                assert all(sorted(row) == sorted(cols) for row in got["sel_idx"].tolist()), (name, shape, k)
    assert ("one_tile", 1) in ran and ("one_tile", 5) in ran and (V < 4808 or ("spread", 64) in ran), ran
    x32, w = sops.period3(shape, wdtype)
    wbuf = tv._table(w.cuda())
    for k in sops.KS:
        got = _sample(M, K, V, _xbuf(x32, wdtype, True), wbuf, k)
        _check_selection(got, M, V, k, ("period3", shape, wdtype, k))
        L = got["logits"][:M, :V]
        assert tv._bits(L[:, 3:], L[:, :-3])                                 # every logit at every third column
        idx = got["sel_idx"].cpu()
        n = min(k, len(range(0, V, 3)) - 1)
        assert ((idx[:, 1:n] - idx[:, :n - 1]) == 3).all()                  # the best class, lowest columns first
    for case in ops.TIE_CASES:
        made = ops.tie(shape, wdtype, 0, case)
        if made is None:
            continue
        x32, w, a, b = made
        got = _sample(M, K, V, _xbuf(x32, wdtype, False), tv._table(w.cuda()), 1, 0.9, 0.7)
        assert got["token"][0].tolist() == [a] * M and got["sel_idx"][:, 0].tolist() == [a] * M, (case, shape, a, b)
        got = _sample(M, K, V, _xbuf(x32, wdtype, False), tv._table(w.cuda()), 5)
        assert got["sel_idx"][:, :2].tolist() == [[a, b]] * M, (case, shape, a, b)
        _check_selection(got, M, V, 5, (case, shape, wdtype))


# ---- 4. the draw ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_the_draw_follows_the_counters(wdtype, shape):
    M, K, V = shape
    worst = 1.0
    for x_f32 in (True, False):
        xbuf, wbuf, _, _ = tv._case(shape, wdtype, x_f32)
        for k in sops.KS:
            for temperature in sops.TEMPERATURES:
                for top_p in sops.TOP_PS:
                    what = (shape, wdtype, x_f32, k, temperature, top_p)
                    got = _sample(M, K, V, xbuf, wbuf, k, top_p, temperature, calls=sops.DRAWS)
                    share = _check_draws(got, M, k, top_p, temperature, SEED, np.zeros(M), np.arange(M), what)
                    worst = min(worst, share)
                    assert share >= 0.95, (what, share)
                    if k > 1 and V > 16:
                        assert len(set(got["token"].reshape(-1).tolist())) > 1, what      # (it does draw)
    print(shape, wdtype, "smallest share of uniquely decided draws: %.4f" % worst)


@pytest.mark.gpu
def test_the_draw_at_the_lm_shape_and_at_large_counters():
    M, K, V = sops.LM
    wdtype = torch.bfloat16
    xbuf, wbuf, _, _ = tv._case(sops.LM, wdtype, True)
    greedy_logits = tv._logit_buffer(M, V, torch.float32)
    greedy, _ = tv._pick(M, K, V, xbuf, wbuf, greedy_logits)
    ctr0 = np.array([(1 << 32) - 3], dtype=np.int64)                       # the counter's high word comes into play
    sid = np.array([2 ** 31 - 1], dtype=np.int64)
    for k, temperature, top_p in ((40, 1.0, 0.9), (64, 0.7, 1.0), (5, 0.7, 0.9), (16, 1.0, 1.0)):
        got = _sample(M, K, V, xbuf, wbuf, k, top_p, temperature, calls=sops.DRAWS, ctr=torch.from_numpy(ctr0).cuda(),
                      sid=torch.from_numpy(sid.astype(np.int32)).cuda())
        assert tv._bits(got["logits"], greedy_logits)
        _check_selection(got, M, V, k, (sops.LM, k))
        share = _check_draws(got, M, k, top_p, temperature, SEED, ctr0, sid, (sops.LM, k, temperature, top_p))
        assert share >= 0.95, share
    got = _sample(M, K, V, xbuf, wbuf, 1, 0.9, 0.7)
    assert torch.equal(got["token"][0], greedy)


# ---- 5. non-finite rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_a_nan_or_an_infinite_best_logit_is_the_greedy_pick(wdtype, shape):
    M, K, V = shape
    x32, w, rows = ops.nan_rows(shape, wdtype, 0, True)
    winf = ops.operands(shape, wdtype, 0)[1]
    v_inf = V // 2
    winf[v_inf] = 0.0
    winf[v_inf, 0] = float("inf")                                           # x[:, 0] > 1/2: a +inf logit in every row
    wminus = ops.operands(shape, wdtype, 0)[1]
    wminus[V - 1] = 0.0
    wminus[V - 1, 0] = float("-inf")                                        # a -inf logit further down: weight 0
    xbuf = tv._case(shape, wdtype, True)[0]
    for k in (1, 5, 64):
        ctr = torch.arange(5, 5 + M, dtype=torch.long, device="cuda")
        got = _sample(M, K, V, xbuf, tv._table(w.cuda()), k, 0.9, 0.7, ctr=ctr, calls=2)
        assert got["token"].tolist() == [[rows[0]] * M] * 2 and (got["kept"] == 0).all(), (shape, k)
        assert got["ctr"].tolist() == list(range(7, 7 + M))
        assert torch.isnan(got["sel_val"][:, 0]).all() and got["sel_idx"][:, 0].tolist() == [rows[0]] * M
        if min(k, V) > 1:
            assert got["sel_idx"][:, 1].tolist() == [rows[1]] * M
        _check_selection(got, M, V, k, ("nan", shape, k))
        got = _sample(M, K, V, xbuf, tv._table(winf.cuda()), k, 0.9, 0.7, ctr=ctr, calls=2)
        assert got["token"].tolist() == [[v_inf] * M] * 2 and (got["kept"] == 0).all(), (shape, k)
        assert got["ctr"].tolist() == list(range(7, 7 + M)) and torch.isinf(got["sel_val"][:, 0]).all()
        _check_selection(got, M, V, k, ("inf", shape, k))
        got = _sample(M, K, V, xbuf, tv._table(wminus.cuda()), k, 1.0, 0.7, calls=8)
        _check_selection(got, M, V, k, ("-inf", shape, k))
        _check_draws(got, M, k, 1.0, 0.7, SEED, np.zeros(M), np.arange(M), ("-inf", shape, k))
        assert (got["token"] != V - 1).all() and (got["kept"] >= 1).all()


# ---- 6. independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_a_rows_draws_do_not_depend_on_its_batch(wdtype):
    shape = (3, 288, 40)
    M, K, V = shape
    xbuf, wbuf, _, _ = tv._case(shape, wdtype, True)
    ctr = torch.tensor([4, 0, 9], dtype=torch.long, device="cuda")
    sid = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    both = _sample(M, K, V, xbuf, wbuf, 16, 0.9, 0.8, ctr=ctr, sid=sid, calls=32)
    for m in range(3):
        one = _sample(1, K, V, xbuf[m:], wbuf, 16, 0.9, 0.8, ctr=ctr[m:m + 1], sid=sid[m:m + 1], calls=32)
        assert torch.equal(one["token"][:, 0], both["token"][:, m]), m
        assert tv._bits(one["sel_val"][0], both["sel_val"][m]) and torch.equal(one["kept"][:, 0], both["kept"][:, m])
    assert len(set(both["token"].reshape(-1).tolist())) > 3
    # two rows with one x and one sid, ctr one apart: one stream, shifted by one
    x2 = tv._rows(2, K, K + 8, torch.float32, xbuf[1:2, :K].expand(2, K))
    got = _sample(2, K, V, x2, wbuf, 16, 0.9, 0.8, ctr=torch.tensor([0, 1], dtype=torch.long, device="cuda"),
                  sid=torch.tensor([5, 5], dtype=torch.int32, device="cuda"), calls=32)
    assert torch.equal(got["token"][1:, 0], got["token"][:-1, 1])
    assert len(set(got["token"][:, 0].tolist())) > 1
    # another seed, another stream id: other draws
    other = _sample(M, K, V, xbuf, wbuf, 16, 0.9, 0.8, seed=SEED + 1, ctr=ctr, sid=sid, calls=32)
    assert not torch.equal(other["token"], both["token"])
    other = _sample(M, K, V, xbuf, wbuf, 16, 0.9, 0.8, ctr=ctr, sid=sid + 3, calls=32)
    assert not torch.equal(other["token"], both["token"])


# ---- 7. the stack -----------------------------------------------------------------------------------------------------------------
B, T, P0, C, VOCAB = tv.B, tv.T, tv.P0, tv.C, tv.VOCAB
TOP_K, TOP_P, TEMP = 8, 0.9, 0.8
_BANNED = ((F, "linear"), (torch, "addmm"), (torch, "matmul"), (torch, "argmax"), (torch.Tensor, "argmax"),
           (torch, "multinomial"), (torch, "topk"), (torch, "softmax"))


def _state(m, case, seed=SEED, sampler=True):
    opt = dict(rolling=case != "static", hold_vocab=True, per_sequence=case == "per_sequence_ragged")
    st = m.init_decoding(B, T, torch.bfloat16, "cuda", **opt)
    return m.init_sampling(st, seed, TOP_K, TOP_P, TEMP) if sampler else st


def _prompt(m, case):
    prompt = tv._tokens()[:, :P0].clone()
    if case == "per_sequence_ragged":
        for b, n in enumerate([17, 9, 1]):
            prompt[b, n:] = m.pad_idx
    return prompt


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "static", "per_sequence_ragged"])
def test_generate_samples_replayed_as_eagerly_and_every_token_follows_its_row(case):
    dtype = torch.bfloat16
    m = tv._stack()
    prompt = _prompt(m, case)
    n_new = T - P0
    out = {}
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for graph in (False, True):
            st = _state(m, case)
            with _Calls() as calls:
                calls.step()
                out[graph] = m.generate(prompt, n_new, st, graph=graph, return_rows=True) + (st,)
            assert calls.all().count(SAMPLE_FN) == (3 if graph else n_new) and tv.VOCAB_FN not in calls.all()
            assert st.sampler.ctr.tolist() == [n_new] * B and st.sampler.sid.tolist() == list(range(B))
        again = m.generate(prompt, n_new, _state(m, case), graph=True)
        other = m.generate(prompt, n_new, _state(m, case, seed=SEED ^ 1), graph=True)
        greedy = m.generate(prompt, n_new, _state(m, case, sampler=False), graph=True)
        # every token against the row it was read from: token [b, i] is draw i of stream b
        (tok_e, rows_e, _), (tok_g, rows_g, st) = out[False], out[True]
        probe = _state(m, case)
        picked, share = [], []
        for i in range(n_new):
            tok, sel_idx, sel_val, kept = m.sample_tokens(rows_g[i:i + 1], probe, return_details=True)
            picked.append(tok.clone())
            got = dict(token=tok, kept=kept.view(1, B), sel_idx=sel_idx, sel_val=sel_val, ctr=probe.sampler.ctr)
            share.append(_check_draws(got, B, TOP_K, TOP_P, TEMP, SEED, np.full(B, i), np.arange(B), (case, i)))
            L = probe.sampler.logits
            for b in range(B):
                assert sel_idx[b].tolist() == ref.topk(L[b].cpu().numpy(), TOP_K).tolist()
    assert tuple(tok_g.shape) == (B, n_new) and tok_g.dtype == torch.long and tuple(rows_g.shape) == (n_new, B, C)
    assert torch.equal(tok_g, tok_e) and tv._bits(rows_g, rows_e)           # (a warm-up draw left in ctr would shift these)
    assert torch.equal(torch.cat(picked, 0).t(), tok_g)
    assert torch.equal(again, tok_g) and not torch.equal(other, tok_g) and not torch.equal(greedy, tok_g)
    assert int(tok_g.min()) >= 0 and int(tok_g.max()) < VOCAB
    print(case, "tokens", tok_g.tolist(), "uniquely decided: %.3f" % (sum(share) / len(share)))
    assert sum(share) / len(share) >= 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_generate_samples_under_the_ban(kind, monkeypatch):
    """generate(graph=True) on a state with a sampler, its own code: from its first pick on -- through the scratch state, the
    warm-up, the capture and every replay -- the framework's GEMMs, argmax, multinomial, topk and softmax raise."""
    dtype = torch.bfloat16
    m = tv._stack()
    prompt = _prompt(m, kind)
    n_new = 8
    armed = []
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = m.generate(prompt, n_new, _state(m, kind), graph=True)
        st = _state(m, kind)

        def gated(name, real):
            def f(*a, **k):
                if armed:
                    raise AssertionError("%s reached in generate behind the prefill" % name)
                return real(*a, **k)
            return f
        for mod, name in _BANNED:
            monkeypatch.setattr(mod, name, gated(name, getattr(mod, name)))
        real_sample = m.sample_tokens

        def arming(*a, **k):
            armed.append(True)
            return real_sample(*a, **k)
        monkeypatch.setattr(m, "sample_tokens", arming)
        try:
            got = m.generate(prompt, n_new, st, graph=True)
            torch.cuda.synchronize()
        finally:
            n_calls = len(armed)
            del armed[:]
    assert n_calls == 3                                  # the first token, the warm-up, the capture
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_reorder_and_reset_move_and_restart_the_streams():
    dtype = torch.bfloat16
    m = tv._stack()
    g = torch.Generator().manual_seed(13)
    rows = torch.randn(4, 1, B, C, generator=g).cuda()

    def direct(x, ctr, sid):
        """The entry itself on the state's table at explicit counters."""
        xb = x.reshape(B, C).float().contiguous()
        got = _sample(B, C, VOCAB, xb, st.vocab, TOP_K, TOP_P, TEMP, ctr=torch.tensor(ctr, dtype=torch.long, device="cuda"),
                      sid=torch.tensor(sid, dtype=torch.int32, device="cuda"), logits=torch.full((B + 3, VOCAB + 8), 7.0, device="cuda"))
        return got["token"]
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _state(m, "per_sequence_ragged")
        m.decode(_prompt(m, "per_sequence_ragged").t(), st, _prompt(m, "per_sequence_ragged").eq(m.pad_idx))
        sm = st.sampler
        nbytes = m.decoding_state_nbytes(st)
        assert nbytes - m.decoding_state_nbytes(_state(m, "per_sequence_ragged", sampler=False)) == 4 * B * VOCAB + 12 * B
        assert torch.equal(m.sample_tokens(rows[0], st), direct(rows[0], [0, 0, 0], [0, 1, 2]))
        m.sample_tokens(rows[0, :, :2], st)                                 # two rows of the batch draw once more
        assert sm.ctr.tolist() == [2, 2, 1]
        ptrs = (sm.ctr.data_ptr(), sm.sid.data_ptr())
        assert m.reorder_decoding_state(st, torch.tensor([2, 0, 1], device="cuda")) is st
        assert sm.ctr.tolist() == [1, 2, 2] and sm.sid.tolist() == [2, 0, 1] and ptrs == (sm.ctr.data_ptr(), sm.sid.data_ptr())
        assert torch.equal(m.sample_tokens(rows[1], st), direct(rows[1], [1, 2, 2], [2, 0, 1]))
        assert m.reset_decoding_rows(st, [1]) is st
        assert sm.ctr.tolist() == [2, 0, 3] and sm.sid.tolist() == [2, B, 1] and sm.next_sid == B + 1
        assert torch.equal(m.sample_tokens(rows[2], st), direct(rows[2], [2, 0, 3], [2, B, 1]))
        m.reset_decoding_rows(st, torch.tensor([0, 1], device="cuda"))
        assert sm.ctr.tolist() == [0, 0, 4] and sm.sid.tolist() == [B + 1, B + 2, 1] and sm.next_sid == B + 3
        out = torch.full((1, B), -1, dtype=torch.long, device="cuda")
        assert m.sample_tokens(rows[3], st, out=out) is out
        assert torch.equal(out, direct(rows[3], [0, 0, 4], [B + 1, B + 2, 1]))
        assert m.refresh_decoding_weights(st) is st and sm.ctr.tolist() == [1, 1, 5]        # (nothing of the sampler's to do)
        assert m.decoding_state_nbytes(st) == nbytes
        with pytest.raises(ValueError, match="contiguous int64"):
            m.sample_tokens(rows[3], st, out=torch.zeros(1, B, dtype=torch.int32, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_a_state_without_a_sampler_is_greedy_as_before(kind):
    """generate on a state made with hold_vocab and no sampler: the tokens of decode + next_tokens, written out."""
    dtype = torch.bfloat16
    m = tv._stack()
    prompt = tv._tokens()[:, :P0].clone()
    n_new = 8
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = m.init_decoding(B, T, dtype, "cuda", rolling=kind == "rolling", hold_vocab=True)
        assert getattr(st, "sampler", None) is None
        got = m.generate(prompt, n_new, st, graph=True)
        st = m.init_decoding(B, T, dtype, "cuda", rolling=kind == "rolling", hold_vocab=True)
        tok = m.next_tokens(m.decode(prompt.t(), st)[-1:], st)
        want = [tok.clone()]
        for _ in range(1, n_new):
            tok = m.next_tokens(m.decode(tok, st), st)
            want.append(tok.clone())
    assert torch.equal(got, torch.cat(want, 0).t())
