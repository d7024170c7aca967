"""-m gpu: full-vocabulary and nucleus sampling on a held vocabulary table (csrc/ea_ceva_decode_nucleus.hip,
ea_ceva_sdecode_vocab_sample_full / _logprob) and DecoderStack.init_nucleus_sampling, against
tests/decoder_nucleus_reference.py on the kernel's own stored logits.  The draw check allows eps(S) = 2^-19 mass^h(S) + |S|;
with kept <= 2048 at most 2048 * 2 * (2^-19 + 2048 / 2^32), about 1 %, of the draws can have more than one admissible column,
and at least 0.95 of a case's draws must have exactly one (tests/test_decoder_nucleus_cpu.py confirms it on host logits)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_decoder_vocab as tv                    # the framed buffers, the shared operands, the stack
import decoder_nucleus_reference as ref
from ceva_decoding import _ctx
from ea_harness import token_pick as tp

FN = "ea_ceva_sdecode_vocab_sample_full"
W_DTYPES, W_IDS = tv.W_DTYPES, tv.W_IDS
SHAPES = [(3, 64, 16), (17, 64, 64), (2, 128, 1000), (1, 64, 2048)]
LM = (1, 1024, 32768)
PARAMS = [(T, p) for T in (0.7, 1.0) for p in (1.0, 0.9, 0.3)]
SEED, DRAWS = 0x9E3779B97F4A7C15, 64


def _draw(M, K, V, xbuf, wbuf, top_p, temperature, seed=SEED, ctr=None, sid=None, calls=1):
    """`calls` consecutive calls on one ctr buffer -> dict(token, kept, thr_idx, thr_val [calls, M], mass [calls, M, 2], logits
    (the framed buffer), ctr)."""
    from efficient_attention import _native as nv
    nbytes = nv.lib().ea_ceva_sdecode_vocab_sample_full_ws(M, V)
    assert nbytes == 8 * M * ((V + 15) // 16)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    logits = tv._logit_buffer(M, V, torch.float32)
    ctr = torch.zeros(M, dtype=torch.long, device="cuda") if ctr is None else ctr.clone()
    sid = torch.arange(M, dtype=torch.int32, device="cuda") if sid is None else sid
    new = lambda dtype, *tail: torch.full((calls, M) + tail, -7, dtype=dtype, device="cuda")     # noqa: E731
    out = dict(token=new(torch.long), kept=new(torch.int32), thr_idx=new(torch.int32), thr_val=new(torch.float32),
               mass=new(torch.long, 2), logits=logits, ctr=ctr)
    for i in range(calls):
        nv.call(FN, M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf),
                nv.io_dtype(wbuf), nv.ptr(logits), logits.stride(0), nv.ptr(ws), nbytes, top_p, temperature, seed, nv.ptr(ctr),
                nv.ptr(sid), *(nv.ptr(out[k][i]) for k in ("token", "kept", "thr_idx", "thr_val", "mass")), nv.stream())
    torch.cuda.synchronize()
    assert (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()
    return out


def _check(got, M, V, top_p, temperature, ctr0, sid, what, draws=True):
    """2, 3 and 4 on every row and call -> the share of draws with exactly one admissible column."""
    L = got["logits"][:M, :V].cpu().numpy()
    tok, kept, thr_idx, thr_val, mass = (got[k].cpu().numpy() for k in ("token", "kept", "thr_idx", "thr_val", "mass"))
    calls, one = tok.shape[0], 0
    for m in range(M):
        ordr, q = ref.order(L[m]), ref.masses(L[m], temperature)
        rank = np.empty(V, dtype=np.int64)
        rank[ordr] = np.arange(V)
        n, ti, C, Z = int(kept[0, m]), int(thr_idx[0, m]), int(mass[0, m, 0]), int(mass[0, m, 1])
        for a in (kept, thr_idx, mass):                                       # (the logits are the same in every call)
            assert (a[:, m] == a[0, m]).all(), (what, m)
        assert thr_val[:, m].copy().view(np.int32).tolist() == [int(L[m, ti:ti + 1].view(np.int32)[0])] * calls, (what, m)   # 2
        assert rank[ti] + 1 == n and (rank[tok[:, m]] < n).all(), (what, m, n, rank[ti])
        assert top_p < 1.0 or n == V
        K = np.sort(ordr[:n])                                                 # the kept set in vocabulary order
        Ch, Zh = int(q[K].sum()), int(q.sum())
        eK, eZ = ref.eps(Ch, n), ref.eps(Zh, V)
        assert Ch + eK >= top_p * (Zh - eZ) and Ch - int(q[ti]) - eK < top_p * (Zh + eZ), (what, m)      # 3
        assert abs(C - Ch) <= eK and abs(Z - Zh) <= eZ, (what, m, C - Ch, Z - Zh)
        if draws:                                                             # 4
            P = np.cumsum(q[K]).astype(np.float64)
            lo = np.concatenate([[0.0], P[:-1]]) - eK
            for i in range(calls):
                r = ref.draw(ref.word(SEED, int(ctr0[m]) + i, int(sid[m])), C)
                ok = (lo <= r) & (r < P + eK)
                assert ok[np.searchsorted(K, tok[i, m])], (what, m, i, int(tok[i, m]), r)
                one += int(ok.sum() == 1)
    assert got["ctr"].cpu().tolist() == [int(c) + calls for c in ctr0], what
    return one / (calls * M)


# ---- 1 .. 4 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("temperature,top_p", PARAMS)
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=tv._ids(SHAPES))
def test_the_nucleus_and_the_draw_follow_the_contract(shape, wdtype, temperature, top_p):
    M, K, V = shape
    xbuf, wbuf, _, _ = tv._case(shape, wdtype, True)
    greedy_logits = tv._logit_buffer(M, V, torch.float32)
    tv._pick(M, K, V, xbuf, wbuf, greedy_logits)
    ctr0 = torch.arange(M, dtype=torch.long, device="cuda") * 1000 + (1 << 32) - 3      # (both words of the counter in use)
    got = _draw(M, K, V, xbuf, wbuf, top_p, temperature, ctr=ctr0, calls=DRAWS)
    assert tv._bits(got["logits"], greedy_logits)                                        # 1 (frame and all)
    assert _check(got, M, V, top_p, temperature, ctr0.tolist(), range(M), (shape, wdtype, temperature, top_p)) >= 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_the_exact_properties_at_the_lm_shape(wdtype):
    M, K, V = LM
    xbuf, wbuf, ref32, _ = tv._case(LM, wdtype, True)
    for top_p in (0.9, 1.0):
        got = _draw(M, K, V, xbuf, wbuf, top_p, 0.7, calls=2)
        assert tv._bits(got["logits"][:M, :V], ref32)
        _check(got, M, V, top_p, 0.7, [0] * M, range(M), (LM, wdtype, top_p), draws=False)


# ---- 5. exact cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("top_p", [1.0, 0.9, 0.3])
@pytest.mark.parametrize("V", [1000, 5000])
def test_a_row_of_equal_logits_is_cut_by_index_and_drawn_exactly(V, top_p):
    M, K = 2, 64
    g = torch.Generator().manual_seed(V)
    x = torch.randn(M, K, generator=g).cuda()
    w = torch.randn(1, K, generator=g).to(torch.bfloat16).cuda().expand(V, K).contiguous()
    got = _draw(M, K, V, x, w, top_p, 0.7, calls=8)
    n = V if top_p == 1.0 else -(-ref.target(top_p, V << 32) >> 32)          # ceil(target / 2^32) columns of mass 2^32 each
    for m in range(M):
        assert got["kept"][:, m].tolist() == [n] * 8 and got["thr_idx"][:, m].tolist() == [n - 1] * 8
        assert got["mass"][:, m].tolist() == [[n << 32, V << 32]] * 8
        want = [ref.draw(ref.word(SEED, i, m), n << 32) >> 32 for i in range(8)]
        assert got["token"][:, m].tolist() == want, (V, top_p, m)


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_kept_one_is_greedy_and_special_values_follow_their_rules(wdtype):
    shape = M, K, V = (2, 128, 1000)
    xbuf, wbuf, _, _ = tv._case(shape, wdtype, True)
    greedy, _ = tv._pick(M, K, V, xbuf, wbuf)
    got = _draw(M, K, V, xbuf, wbuf, 1e-6, 1.0, calls=4)
    assert (got["kept"] == 1).all() and (got["token"] == greedy).all() and (got["thr_idx"] == greedy).all()
    # a NaN row (x holds a NaN) and a +inf logit (x[:, 0] > 0): that index, kept = 0, the counter advances
    x, w = xbuf[:M, :K].clone(), wbuf[:V].clone()
    x[0, 3] = float("nan")
    w[777, 0] = float("inf")
    got = _draw(M, K, V, x, w, 0.9, 0.7, calls=3)
    assert got["token"].tolist() == [[0, 777]] * 3 and (got["kept"] == 0).all() and got["ctr"].tolist() == [3, 3]
    # a -inf column has mass 0: kept at top_p = 1, never drawn
    w = wbuf[:V].clone()
    cold = int(greedy[0])
    w[cold, 0] = float("-inf")
    got = _draw(M, K, V, xbuf, w, 1.0, 100.0, calls=DRAWS)
    assert (got["kept"] == V).all() and (got["token"] != cold).all() and (got["thr_idx"] == cold).all()
    assert len(set(got["token"][:, 0].tolist())) > DRAWS // 2


# ---- 6. independence and reproducibility --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_a_rows_draws_do_not_depend_on_its_batch_or_the_run(top_p):
    shape = M, K, V = (3, 64, 16) if top_p == 1.0 else (3, 288, 40)
    xbuf, wbuf, _, _ = tv._case(shape, torch.bfloat16, True)
    ctr, sid = torch.tensor([5, 0, 1 << 33], device="cuda"), torch.tensor([9, 2, 4], dtype=torch.int32, device="cuda")
    keys = ("token", "kept", "thr_idx", "thr_val", "mass")
    batch = _draw(M, K, V, xbuf, wbuf, top_p, 0.7, ctr=ctr, sid=sid, calls=DRAWS)
    again = _draw(M, K, V, xbuf, wbuf, top_p, 0.7, ctr=ctr, sid=sid, calls=DRAWS)
    assert all(tv._bits(batch[k], again[k]) for k in keys)
    for m in range(M):
        alone = _draw(1, K, V, xbuf[m:m + 1], wbuf, top_p, 0.7, ctr=ctr[m:m + 1], sid=sid[m:m + 1], calls=DRAWS)
        assert all(tv._bits(batch[k][:, m:m + 1].contiguous(), alone[k]) for k in keys), m
    for other in (dict(seed=SEED ^ 1), dict(sid=sid + 1)):
        assert not torch.equal(_draw(M, K, V, xbuf, wbuf, top_p, 0.7, **dict(dict(ctr=ctr, sid=sid, calls=DRAWS), **other))["token"],
                               batch["token"])


# ---- 7. the stack -----------------------------------------------------------------------------------------------------------------
B, T, P0, C, VOCAB = tv.B, tv.T, tv.P0, tv.C, tv.VOCAB
_BANNED = ((F, "linear"), (torch, "softmax"), (torch, "sort"), (torch, "cumsum"), (torch, "multinomial"), (torch, "topk"),
           (torch, "argmax"))


def _state(m, case, top_p, seed=SEED):
    st = m.init_decoding(B, T, torch.bfloat16, "cuda", rolling=case != "static", hold_vocab=True)
    return m.init_logprobs(m.init_nucleus_sampling(st, seed, top_p, 0.8))


@pytest.mark.gpu
@pytest.mark.parametrize("case,top_p", [("rolling", 0.9), ("static", 1.0)])
def test_generate_samples_the_whole_vocabulary_with_no_framework_launch(case, top_p, monkeypatch):
    m, prompt, n_new = tv._stack(), tv._tokens()[:, :P0].clone(), 8
    with _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok_e, rows, lp_e = m.generate(prompt, n_new, _state(m, case, top_p), graph=False, return_rows=True, return_logprobs=True)
        plain = m.generate(prompt, n_new, _state(m, case, top_p), graph=True)
        other = m.generate(prompt, n_new, _state(m, case, top_p, SEED ^ 1), graph=True)
        probe = _state(m, case, top_p)
        for i in range(n_new):                                              # token [b, i] is draw i of stream b
            tok, logp = m.sample_tokens_logprobs(rows[i:i + 1], probe)
            assert torch.equal(tok[0], tok_e[:, i]) and tv._bits(logp[0], lp_e[:, i].contiguous())
            assert tv._bits(m.token_logprobs(rows[i:i + 1], probe, targets=tok)[1], logp)
        assert probe.sampler.ctr.tolist() == [n_new] * B
        st, armed = _state(m, case, top_p), []

        def gated(name, real):
            def f(*a, **k):
                if armed:
                    raise AssertionError("%s reached in generate behind the prefill" % name)
                return real(*a, **k)
            return f
        for mod, name in _BANNED:
            monkeypatch.setattr(mod, name, gated(name, getattr(mod, name)))
        select = tp.select_pick

        def arming(*a, **k):                                                # (generate selects its pick ahead of the prefill)
            pick = select(*a, **k)
            call = pick.run
            pick.run = lambda *a, **k: (armed.append(True), call(*a, **k))[1]
            return pick
        monkeypatch.setattr(tp, "select_pick", arming)
        try:
            tok_g, lp_g = m.generate(prompt, n_new, st, graph=True, return_logprobs=True)
            torch.cuda.synchronize()
        finally:
            n_calls = len(armed)
            del armed[:]
    assert n_calls == 3                                                      # the first token, the warm-up, the capture
    assert torch.equal(tok_g, tok_e) and tv._bits(lp_g, lp_e) and torch.equal(plain, tok_e) and not torch.equal(other, tok_e)
    assert st.sampler.ctr.tolist() == [n_new] * B


@pytest.mark.gpu
def test_reorder_and_reset_move_and_restart_the_streams():
    m = tv._stack()
    rows = torch.randn(3, 1, B, C, generator=torch.Generator().manual_seed(13)).cuda()
    with torch.no_grad(), _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = m.init_decoding(B, T, torch.bfloat16, "cuda", rolling=True, hold_vocab=True, per_sequence=True)
        m.init_nucleus_sampling(st, SEED, 0.9, 0.8)
        prompt = tv._tokens()[:, :P0]
        m.decode(prompt.t(), st, prompt.eq(m.pad_idx))
        sm = st.sampler

        def direct(x, ctr, sid):
            got = _draw(B, C, VOCAB, x.reshape(B, C).float().contiguous(), st.vocab, 0.9, 0.8,
                        ctr=torch.tensor(ctr, device="cuda"), sid=torch.tensor(sid, dtype=torch.int32, device="cuda"))
            return got["token"], got["kept"][0], got["mass"][0]
        tok, kept, _, _, mass = m.sample_tokens(rows[0], st, return_details=True)
        want = direct(rows[0], [0, 0, 0], [0, 1, 2])
        assert torch.equal(tok, want[0]) and torch.equal(kept, want[1]) and torch.equal(mass, want[2])
        m.reorder_decoding_state(st, torch.tensor([2, 0, 1], device="cuda"))
        assert sm.ctr.tolist() == [1, 1, 1] and sm.sid.tolist() == [2, 0, 1]
        assert torch.equal(m.sample_tokens(rows[1], st), direct(rows[1], [1, 1, 1], [2, 0, 1])[0])
        m.reset_decoding_rows(st, [1])
        assert sm.ctr.tolist() == [2, 0, 2] and sm.sid.tolist() == [2, B, 1] and sm.next_sid == B + 1
        assert torch.equal(m.sample_tokens(rows[2], st), direct(rows[2], [2, 0, 2], [2, B, 1])[0])
