"""-m gpu: the beam step on a held vocabulary table (csrc/ea_ceva_decode_vocab.hip: ceva_vocab_beam_rows_kernel,
ceva_vocab_beam_merge_kernel; ea_ceva_sdecode_vocab_beam, ea_beam_merge, C ABI 32) and DecoderStack.beam_step / beam_search.
Every comparison is exact -- bits or integers -- against tests/decoder_beam_reference.py: the rule (include/ea_hip.h) was
written so that the host can reproduce it.

 1. the rows kernel at decoder_vocab_operands.SHAPES[:6] split into (S, W) beams, bf16 and fp16 tables, x in fp32 and in the
    table's type, operands framed as in tests/test_gpu_decoder_vocab.py: logits bit-equal to ea_ceva_sdecode_vocab_argmax's,
    lse to ea_ceva_sdecode_vocab_logprob's, cand_idx / sel_val the host's top min(2 W, V) of the stored logits, cand_score
    the host's two fp32 operations from random scores with a -inf and a NaN row; the forced step; nothing outside [M, k']
    or the frames is written; once at (8, 1024, 32768).
 2. ea_beam_merge on constructed candidates: random ones (few distinct scores: ties; NaN, -inf, a frequent eos) over 6
    consecutive steps on one state, the hand-worked cases of tests/test_decoder_beam_cpu.py, a done sentence beside a live one,
    a sentence alone against the same sentence in a batch.
 3. the entry is its rows kernel followed by ea_beam_merge on the candidates it reports.
 4. DecoderStack.beam_search (the geometry of test_gpu_decoder_vocab._stack; S = 3, W = 4, bf16, max_new = 12; rolling, static,
    per-sequence ragged): replayed == eager == host_beam_search driven through next_tokens(return_logits=True),
    token_logprobs(return_lse=True) and reorder_decoding_state; W = 1 is generate; the early exit; poll; reset_beam_search.
 5. the search's steps run with the framework's GEMMs, topk, softmax, log_softmax and argmax replaced by functions that raise."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import decoder_beam_reference as ref                                                # noqa: E402
import decoder_vocab_operands as ops                                                # noqa: E402
import test_decoder_beam_cpu as tc                                                  # noqa: E402
import test_gpu_decoder_logprob as tl                                               # noqa: E402
import test_gpu_decoder_vocab as tv                                                 # noqa: E402
from ceva_decoding import _Calls, _ctx                                              # noqa: E402

BEAM_FN, MERGE_FN = "ea_ceva_sdecode_vocab_beam", "ea_beam_merge"
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
SHAPES = ops.SHAPES[:6]
BEAMS = dict(zip(SHAPES, ([(1, 1)], [(3, 1), (1, 3)], [(4, 4), (1, 16), (2, 8)], [(17, 1), (1, 17)], [(11, 3), (3, 11)],
                          [(2, 32), (16, 4), (64, 1)])))
_bits, _ids = tv._bits, tv._ids
F32 = np.float32
GUARD_I, GUARD_F = -7, 7.0


# ---- a framed beam state on the device and its mirror on the host -----------------------------------------------------------------
class State:
    """The state and the outputs of a beam step, every buffer with a guard behind it (an element, or a row) that must stay.
    `host`: numpy copies a test keeps in step by the reference."""

    def __init__(self, S, W, max_new, score=None, t=0, nfin=0, done=0):
        M = S * W
        self.S, self.W, self.M, self.max_new = S, W, M, max_new
        if score is None:
            score = np.full(M, -np.inf, dtype=F32)
            score[::W] = 0
        per = lambda v: np.broadcast_to(np.asarray(v, dtype=np.int32), (S,)).copy()       # noqa: E731
        self.host = dict(score=np.asarray(score, dtype=F32).copy(), t=per(t), nfin=per(nfin), done=per(done),
                         token=np.full(M, GUARD_I, dtype=np.int64), parent=np.full(M, GUARD_I, dtype=np.int64),
                         hist_tok=np.full((max_new, M), GUARD_I, dtype=np.int32), hist_par=np.full((max_new, M), GUARD_I, dtype=np.int32),
                         fin_score=np.full((S, W), GUARD_F, dtype=F32), fin_len=np.full((S, W), GUARD_I, dtype=np.int32),
                         fin_beam=np.full((S, W), GUARD_I, dtype=np.int32))
        self.dev = {}
        for k, v in self.host.items():
            guard = GUARD_F if v.dtype == F32 else GUARD_I
            rows = v.reshape(1, -1) if v.ndim == 1 else v
            framed = np.concatenate([rows.reshape(-1), np.full(rows.shape[-1], guard, dtype=v.dtype)])
            self.dev[k] = torch.from_numpy(framed).cuda()

    ORDER = ("score", "t", "nfin", "done", "token", "parent", "hist_tok", "hist_par", "fin_score", "fin_len", "fin_beam")

    def ptrs(self):
        from efficient_attention import _native as nv
        return [nv.ptr(self.dev[k]) for k in self.ORDER]

    def read(self):
        """-> the device's buffers as numpy arrays shaped like the host's; the guards are checked."""
        out = {}
        for k, v in self.host.items():
            got = self.dev[k].cpu().numpy()
            guard = got[v.size:]
            assert (guard == (GUARD_F if v.dtype == F32 else GUARD_I)).all(), k
            out[k] = got[:v.size].reshape(v.shape)
        return out

    def slice(self, s):
        """Sentence s alone, as a state of its own (from the host's copies)."""
        W = self.W
        one = State(1, W, self.max_new, self.host["score"][s * W:s * W + W], self.host["t"][s], self.host["nfin"][s], self.host["done"][s])
        return one


def _equal(got, want, what):
    for k, v in want.items():
        same = np.array_equal(got[k].view(np.int32), v.view(np.int32)) if v.dtype == F32 else np.array_equal(got[k], v)
        assert same, (what, k, got[k].tolist(), v.tolist())


def _host_merge(st, cand_idx, cand_score, kc, eos):
    """One step of the reference on st.host, sentence by sentence -> the events."""
    h, W, events = st.host, st.W, set()
    for s in range(st.S):
        t = int(h["t"][s])
        rows = slice(s * W, s * W + W)
        got = ref.merge(cand_idx[rows], cand_score[rows], kc, W, eos, t, int(h["nfin"][s]), int(h["done"][s]), t + 1 == st.max_new)
        events |= got["events"]
        h["token"][rows] = got["token"]
        h["parent"][rows] = [s * W + b for b in got["parent"]]
        if got["score"] is not None:
            h["score"][rows] = got["score"]
            h["hist_tok"][t, rows], h["hist_par"][t, rows] = got["hist_tok"], got["hist_par"]
            for i, (sc, n, b) in enumerate(got["records"]):
                slot = int(h["nfin"][s]) + i
                h["fin_score"][s, slot], h["fin_len"][s, slot], h["fin_beam"][s, slot] = sc, n, b
        h["t"][s], h["nfin"][s], h["done"][s] = got["t"], got["nfin"], got["done"]
    return events


def _merge(st, cand_idx, cand_score, kc, eos):
    """ea_beam_merge on the device state; the candidate lists are [M, 2 W] numpy arrays."""
    from efficient_attention import _native as nv
    ci = torch.from_numpy(np.ascontiguousarray(cand_idx, dtype=np.int32)).cuda()
    cs = torch.from_numpy(np.ascontiguousarray(cand_score, dtype=F32)).cuda()
    assert tuple(ci.shape) == tuple(cs.shape) == (st.M, 2 * st.W)
    nv.call(MERGE_FN, st.S, st.W, kc, nv.ptr(ci), nv.ptr(cs), eos, st.max_new, *st.ptrs(), nv.stream())
    torch.cuda.synchronize()


# ---- 1. the rows kernel -----------------------------------------------------------------------------------------------------------
def _beam(M, K, V, xbuf, wbuf, st, eos, reports=True):
    """ea_ceva_sdecode_vocab_beam -> dict(logits [M, V], cand_idx, cand_score, sel_val [M, 2 W], lse [M]); frames checked."""
    from efficient_attention import _native as nv
    W = st.W
    nbytes = nv.lib().ea_ceva_sdecode_vocab_beam_ws(M, V, W)
    assert nbytes == tc._ws_formula(M, V, W)
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")          # (stale candidates and sums would be NaNs)
    logits = tv._logit_buffer(M, V, torch.float32)
    ci = torch.full((M + 1, 2 * W), GUARD_I, dtype=torch.int32, device="cuda")
    cs, sv = (torch.full((M + 1, 2 * W), GUARD_F, dtype=torch.float32, device="cuda") for _ in range(2))
    lse = torch.full((M + 1,), GUARD_F, dtype=torch.float32, device="cuda")
    rep = [nv.ptr(t) for t in (ci, cs, lse, sv)] if reports else [None] * 4
    nv.call(BEAM_FN, M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf), nv.ptr(logits),
            logits.stride(0), nv.ptr(ws), nbytes, W, eos, st.max_new, *st.ptrs(), *rep, nv.stream())
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xFF).all() and (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()
    assert (ci[M] == GUARD_I).all() and (cs[M] == GUARD_F).all() and (sv[M] == GUARD_F).all() and lse[M].item() == GUARD_F
    return dict(logits=logits[:M, :V], cand_idx=ci[:M], cand_score=cs[:M], sel_val=sv[:M], lse=lse[:M])


def _scores(M, seed):
    """Random finite scores, row 1 -inf and row 2 NaN where the rows exist."""
    score = -np.random.RandomState(seed).rand(M).astype(F32) * 20
    if M > 1:
        score[1] = -np.inf
    if M > 2:
        score[2] = np.nan
    return score


def _check_rows(shape, wdtype, x_f32, S, W, xbuf, wbuf):
    M, K, V = shape
    eos, max_new = V // 2, 5
    want_logits = tv._logit_buffer(M, V, torch.float32)
    tv._pick(M, K, V, xbuf, wbuf, want_logits)
    want_lse = tl._logprob(M, K, V, xbuf, wbuf)["lse"]
    L = want_logits[:M, :V].cpu().numpy()
    lse_h = want_lse.cpu().numpy()
    score = _scores(M, M * 131 + W)
    for forced in (False, True):
        st = State(S, W, max_new, score, t=max_new - 1 if forced else 0)
        got = _beam(M, K, V, xbuf, wbuf, st, eos)
        what = (shape, wdtype, x_f32, S, W, forced)
        assert _bits(got["logits"], want_logits[:M, :V]), what
        assert _bits(got["lse"], want_lse), what
        k = 1 if forced else min(2 * W, V)
        idx, val, cand = (np.stack(a) for a in zip(*[ref.row_candidates(L[m], lse_h[m], score[m], W, eos, forced) for m in range(M)]))
        assert idx.shape == (M, k)
        ci, cs, sv = (got[n].cpu().numpy() for n in ("cand_idx", "cand_score", "sel_val"))
        assert np.array_equal(ci[:, :k], idx), what
        assert np.array_equal(sv[:, :k].view(np.int32), val.view(np.int32)), what
        assert np.array_equal(cs[:, :k].view(np.int32), cand.view(np.int32)), what
        assert (ci[:, k:] == GUARD_I).all() and (cs[:, k:] == GUARD_F).all() and (sv[:, k:] == GUARD_F).all(), what
        # the merge behind it: the reference on the reported candidates
        _host_merge(st, ci, cs, k, eos)
        _equal(st.read(), st.host, what)


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_rows_kernel_candidates_scores_and_lse(wdtype, shape):
    for x_f32 in (True, False):
        xbuf, wbuf, _, _ = tv._case(shape, wdtype, x_f32)
        for S, W in BEAMS[shape]:
            _check_rows(shape, wdtype, x_f32, S, W, xbuf, wbuf)


@pytest.mark.gpu
def test_rows_kernel_at_the_lm_shape():
    shape = (8, 1024, 32768)
    xbuf, wbuf, _, _ = tv._case(shape, torch.bfloat16, True)
    _check_rows(shape, torch.bfloat16, True, 2, 4, xbuf, wbuf)


# ---- 2. the merge on constructed candidates -----------------------------------------------------------------------------------------
MERGES = [(1, 1, 2), (3, 2, 4), (2, 5, 10), (1, 16, 32), (2, 32, 64), (2, 32, 40), (4, 3, 1)]
EOS = 3


def _random_candidates(S, W, kc, seed):
    """[M, 2 W] lists with kc live entries per row: tokens 0 .. 11 (one in twelve is eos), scores from sixteen values (ties)
    with some -inf and NaN; the dead entries hold what the kernel must not read: eos with +inf."""
    rng = np.random.RandomState(seed)
    M = S * W
    ci = np.full((M, 2 * W), EOS, dtype=np.int32)
    cs = np.full((M, 2 * W), np.inf, dtype=F32)
    ci[:, :kc] = rng.randint(0, 12, (M, kc))
    live = (-rng.randint(0, 16, (M, kc)) * 0.25).astype(F32)
    live[rng.rand(M, kc) < 0.04] = -np.inf
    live[rng.rand(M, kc) < 0.02] = np.nan
    cs[:, :kc] = live
    return ci, cs


@pytest.mark.gpu
@pytest.mark.parametrize("S, W, kc", MERGES, ids=["%dx%dx%d" % c for c in MERGES])
def test_merge_over_six_steps_equals_the_reference(S, W, kc):
    st = State(S, W, 5)
    events = set()
    for step in range(6):                                  # t = 0 .. 3, the forced step, then every sentence idle
        ci, cs = _random_candidates(S, W, kc, (S * 64 + W) * 64 + kc + 1000 * step)
        events |= _host_merge(st, ci, cs, kc, EOS)
        _merge(st, ci, cs, kc, EOS)
        _equal(st.read(), st.host, (S, W, kc, step))
    assert {"forced", "idle"} <= events or "went_idle" in events, events
    assert st.host["done"].all() and (st.host["t"] <= 5).all()


@pytest.mark.gpu
def test_merge_on_the_hand_worked_cases():
    seen = set()
    for name, arg, want, events in tc.known_cases():
        W, kc, t = arg["W"], arg["kc"], arg["t"]
        st = State(1, W, t + 1 if arg["forced"] else t + 5, np.full(W, 0.5, dtype=F32), t, arg["nfin"], arg["done"])
        ci = np.full((W, 2 * W), GUARD_I, dtype=np.int32)
        cs = np.full((W, 2 * W), np.inf, dtype=F32)
        ci[:, :kc], cs[:, :kc] = np.array(arg["cand_idx"]), np.stack(arg["cand_score"])
        got_events = _host_merge(st, ci, cs, kc, arg["eos"])
        assert events <= got_events, (name, got_events)
        seen |= got_events
        _merge(st, ci, cs, kc, arg["eos"])
        got = st.read()
        _equal(got, st.host, name)
        # .. and the hand-worked answer itself
        assert got["token"].tolist() == want["token"] and got["parent"].tolist() == want["parent"], name
        assert (int(got["t"][0]), int(got["nfin"][0]), int(got["done"][0])) == (want["t"], want["nfin"], want["done"]), name
        if want["score"] is not None:
            assert np.array_equal(got["score"].view(np.int32), np.array(want["score"], dtype=F32).view(np.int32)), name
        for i, (sc, n, b) in enumerate(want["records"]):
            slot = arg["nfin"] + i
            assert (float(got["fin_score"][0, slot]), int(got["fin_len"][0, slot]), int(got["fin_beam"][0, slot])) == (sc, n, b), name
    assert {"eos_finished", "eos_late", "eos_inf", "tie", "went_idle", "idle", "forced_finished", "dead_beam", "nan_first"} <= seen


@pytest.mark.gpu
def test_a_done_sentence_stays_while_its_neighbour_advances():
    S, W, kc = 3, 4, 8
    st = State(S, W, 6, t=[2, 2, 2], nfin=[1, 4, 0], done=[0, 1, 0])
    before = {k: v.copy() for k, v in st.host.items()}
    for step in range(2):
        ci, cs = _random_candidates(S, W, kc, 77 + step)
        _host_merge(st, ci, cs, kc, EOS)
        _merge(st, ci, cs, kc, EOS)
        got = st.read()
        _equal(got, st.host, step)
        rows = slice(W, 2 * W)
        assert got["token"][rows].tolist() == [EOS] * W and got["parent"][rows].tolist() == list(range(W, 2 * W))
        for k in ("score", "hist_tok", "hist_par"):
            assert np.array_equal(got[k][..., rows].view(np.int32), before[k][..., rows].view(np.int32)), k
        for k in ("fin_score", "fin_len", "fin_beam", "t", "nfin", "done"):
            assert np.array_equal(got[k][1].view(np.int32), before[k][1].view(np.int32)), k
        assert int(got["t"][1]) == 2 and int(got["t"][0]) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("S, W, kc", [(3, 2, 4), (2, 32, 64), (4, 3, 1)], ids=["3x2x4", "2x32x64", "4x3x1"])
def test_a_sentence_does_not_depend_on_its_batch(S, W, kc):
    rng = np.random.RandomState(S * W)
    st = State(S, W, 7, -rng.rand(S * W).astype(F32), t=rng.randint(0, 6, S), nfin=rng.randint(0, W, S))
    ci, cs = _random_candidates(S, W, kc, 5)
    alone = []
    for s in range(S):
        one = st.slice(s)
        _merge(one, ci[s * W:s * W + W], cs[s * W:s * W + W], kc, EOS)
        alone.append(one.read())
    _merge(st, ci, cs, kc, EOS)
    got = st.read()
    for s, one in enumerate(alone):
        rows = slice(s * W, s * W + W)
        assert np.array_equal(got["token"][rows], one["token"]) and np.array_equal(got["parent"][rows] - s * W, one["parent"])
        for k in ("score", "hist_tok", "hist_par"):
            assert np.array_equal(got[k][..., rows].view(np.int32), one[k].view(np.int32)), (s, k)
        for k in ("fin_score", "fin_len", "fin_beam", "t", "nfin", "done"):
            assert np.array_equal(got[k][s].view(np.int32), one[k][0].view(np.int32)), (s, k)


# ---- 3. the entry = its rows kernel + ea_beam_merge --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape, S, W", [((3, 288, 40), 1, 3), ((64, 1024, 1000), 2, 32)], ids=["3x288x40", "64x1024x1000"])
def test_the_entry_is_its_rows_kernel_and_the_merge(shape, S, W):
    M, K, V = shape
    xbuf, wbuf, _, _ = tv._case(shape, torch.bfloat16, True)
    row = tv._case(shape, torch.bfloat16, True)[2][0]
    eos = int(torch.argsort(row, descending=True)[1])     # (row 0's second best logit: an eos among the candidates)
    for t in (0, 3, 4):                                    # max_new = 5: t = 4 is the forced step
        score = _scores(M, 17 + t) if t else None
        a, b = State(S, W, 5, score, t=t), State(S, W, 5, score, t=t)
        got = _beam(M, K, V, xbuf, wbuf, a, eos)
        _merge(b, got["cand_idx"].cpu().numpy(), got["cand_score"].cpu().numpy(), min(2 * W, V), eos)
        _equal(a.read(), b.read(), (shape, t))
        c = State(S, W, 5, score, t=t)                      # .. and without the reports: the lists in the workspace
        _beam(M, K, V, xbuf, wbuf, c, eos, reports=False)
        _equal(c.read(), b.read(), (shape, t, "no reports"))
        assert (a.read()["t"] == t + 1).all()


# ---- 4. the stack -----------------------------------------------------------------------------------------------------------------
C, VOCAB, B, T, P0 = tv.C, tv.VOCAB, tv.B, tv.T, tv.P0
S4, W4, MAX_NEW = 3, 4, 12
DTYPE = torch.bfloat16
# eos is the token greedy decoding emits for sentence 0 at this step (0-based).  Step 4 (its 5th) does not serve: greedy
# decoding emits that token from its first step on, and with it every hypothesis ends within two steps; with step 5's the
# hypotheses of sentence 0 end after 5, 6, 6 and -- by the forced step -- 12 tokens.
GREEDY_STEP = 5


def _prompt(case, S=S4):
    m = tv._stack()
    prompt = tv._tokens()[:S, :P0].clone()
    if case == "per_sequence_ragged":
        for b, n in enumerate([17, 9, 1][:S]):
            prompt[b, n:] = m.pad_idx
    return prompt


def _state(case, M, hold_vocab=True):
    opt = dict(rolling=case != "static", hold_vocab=hold_vocab)
    if case == "per_sequence_ragged":
        opt["per_sequence"] = True
    return tv._stack().init_decoding(M, T, DTYPE, "cuda", **opt)


@functools.lru_cache(maxsize=None)
def _greedy(case, S=S4, n_new=MAX_NEW):
    """generate's tokens, log-probabilities and rows for the prompts of `case` (computed once, never written)."""
    m = tv._stack()
    with _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = m.init_logprobs(_state(case, S))
        tok, rows, logp = m.generate(_prompt(case, S), n_new, st, graph=False, return_rows=True, return_logprobs=True)
    return tok.cpu(), logp.cpu(), rows


def _search(case, prompt, W, eos, max_new, **kw):
    m = tv._stack()
    with _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _state(case, prompt.shape[0] * W)
        hyps = m.beam_search(prompt, st, beam_size=W, eos_idx=eos, max_new=max_new, **kw)
        torch.cuda.synchronize()
    return hyps, st


def _plain(hyps):
    """-> per sentence [(tokens, the raw score's bits)] in the order given."""
    out = []
    for sentence in hyps:
        row = []
        for h in sentence:
            raw = h["raw_score"] if "raw_score" in h else h["raw"]
            row.append((h["tokens"].tolist() if isinstance(h["tokens"], torch.Tensor) else list(h["tokens"]),
                        int(np.asarray(float(raw), dtype=F32).view(np.int32))))
        out.append(row)
    return out


def _host_search(case, prompt, W, eos, max_new):
    """host_beam_search driven through the public API: next_tokens(return_logits=True), token_logprobs(return_lse=True),
    reorder_decoding_state."""
    m = tv._stack()
    M = prompt.shape[0] * W
    st = m.init_logprobs(_state(case, M))
    fed = prompt.repeat_interleave(W, 0)

    def step_fn(tokens, parent):
        if tokens is None:
            mask = fed.eq(m.pad_idx) if case == "per_sequence_ragged" else None
            x = m.decode(fed.t(), st, mask)
            if mask is not None:
                n_b = P0 - mask.ne(0).to(torch.int32).cumsum(1).ne(0).sum(1)
                last = x[(n_b - 1).clamp_(min=0), torch.arange(M, device=x.device)].unsqueeze(0)
            else:
                last = x[P0 - 1:P0]
        else:
            m.reorder_decoding_state(st, torch.from_numpy(parent).cuda())
            last = m.decode(torch.from_numpy(tokens).cuda().view(1, M), st)
        _, logits = m.next_tokens(last, st, return_logits=True)
        _, _, lse = m.token_logprobs(last, st, return_lse=True)
        return logits[0].cpu().numpy(), lse[0].cpu().numpy()
    with torch.no_grad(), _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ref.host_beam_search(step_fn, prompt.shape[0], W, eos, max_new)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "static", "per_sequence_ragged"])
def test_beam_search_replayed_equals_eager_equals_the_host_search(case):
    prompt = _prompt(case)
    eos = int(_greedy(case)[0][0, GREEDY_STEP])
    replayed, st = _search(case, prompt, W4, eos, MAX_NEW, graph=True)
    eager, _ = _search(case, prompt, W4, eos, MAX_NEW, graph=False)
    host, info = _host_search(case, prompt, W4, eos, MAX_NEW)
    print(case, "eos", eos, "fin_len", info["fin_len"], "events", sorted(info["events"]))
    for s, sentence in enumerate(replayed):
        print(case, s, [(h["tokens"].tolist(), float(h["raw_score"]), h["score"]) for h in sentence])
    assert _plain(replayed) == _plain(eager) == _plain(host)
    assert all(len(sentence) >= 1 for sentence in replayed)
    lens = [n for sentence in info["fin_len"] for n in sentence]
    assert min(lens) < MAX_NEW and max(lens) == MAX_NEW, lens            # hypotheses finish mid-way, and by the forced step
    for sentence in replayed:                                            # the normalised score orders a sentence's hypotheses
        scores = [h["score"] for h in sentence]
        assert scores == sorted(scores, reverse=True)
        for h in sentence:
            assert h["tokens"].dtype == torch.long and h["tokens"][-1].item() == eos and (h["tokens"][:-1] != eos).all()
            assert h["score"] == float(h["raw_score"]) / len(h["tokens"])
    # the state's record agrees with what came back
    assert st.beam.done.tolist() == [1] * S4 and st.beam.replays <= MAX_NEW - 1


@pytest.mark.gpu
def test_beam_size_one_is_greedy_decoding():
    m = tv._stack()
    tok, logp, rows = _greedy("rolling")
    eos = next(v for v in range(2, VOCAB) if v not in set(tok.reshape(-1).tolist()))
    hyps, st = _search("rolling", _prompt("rolling"), 1, eos, MAX_NEW)
    with _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        held = m.init_logprobs(_state("rolling", S4))
        targets = torch.full((1, S4), eos, dtype=torch.long, device="cuda")
        _, last = m.token_logprobs(rows[MAX_NEW - 1:MAX_NEW], held, targets=targets)     # the forced eos: logit[eos] - lse
    for s in range(S4):
        assert len(hyps[s]) == 1
        assert hyps[s][0]["tokens"].tolist() == tok[s, :MAX_NEW - 1].tolist() + [eos]
        raw = F32(0)
        for v in logp[s, :MAX_NEW - 1].numpy():
            raw = F32(raw + v)
        raw = F32(raw + F32(last[0, s].item()))
        assert np.asarray(float(hyps[s][0]["raw_score"]), dtype=F32).view(np.int32) == raw.view(np.int32), (s, hyps[s][0]["raw_score"], raw)


@pytest.mark.gpu
def test_early_exit_poll_and_reset():
    m = tv._stack()
    case, max_new = "static", T - P0
    prompt = _prompt(case, 1)
    greedy = _greedy(case, 1)[0][0].tolist()
    eos = greedy[GREEDY_STEP]                               # one sentence, one beam: done when greedy decoding emits eos
    first = greedy.index(eos) + 1
    polled, st = _search(case, prompt, 1, eos, max_new, poll=2)
    assert [len(h["tokens"]) for h in polled[0]] == [first] and polled[0][0]["tokens"].tolist() == greedy[:first]
    assert st.beam.replays < max_new - 1 and st.beam.replays <= first + 1, st.beam.replays
    unpolled, st16 = _search(case, prompt, 1, eos, max_new)
    assert _plain(unpolled) == _plain(polled) and st16.beam.replays >= st.beam.replays
    # S = 3, W = 4: poll's value does not change the result
    prompt = _prompt(case)
    eos = int(_greedy(case)[0][0, GREEDY_STEP])
    want, st = _search(case, prompt, W4, eos, MAX_NEW)
    for poll in (1, 2, 5):
        got, stp = _search(case, prompt, W4, eos, MAX_NEW, poll=poll)
        assert _plain(got) == _plain(want), poll
        if all(n < MAX_NEW for n in stp.beam.fin_len.reshape(-1).tolist()) and poll <= 2:
            assert stp.beam.replays < MAX_NEW - 1
    # after reset_beam_search the same call repeats the result (the attention's own state is fresh: the beam's buffers stay)
    with _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = _state(case, S4 * W4)
        again.beam = st.beam
        ptrs = [t.data_ptr() for t in st.beam.buffers()]
        assert m.reset_beam_search(again) is again and st.beam.t.tolist() == [0] * S4
        got = m.beam_search(prompt, again, beam_size=W4, eos_idx=eos, max_new=MAX_NEW)
        assert _plain(got) == _plain(want) and [t.data_ptr() for t in again.beam.buffers()] == ptrs
        with pytest.raises(ValueError, match="beam search was made with"):
            m.beam_search(prompt, again, beam_size=W4, eos_idx=eos + 1, max_new=MAX_NEW)


# ---- 5. under the ban -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_beam_search_runs_its_steps_under_the_ban(kind, monkeypatch):
    """`DecoderStack.beam_search(graph=True)`, its own code: from the first `beam_step` on -- through the reorder, the scratch
    state, the warm-up, the capture and every replay -- the framework's GEMMs, topk, softmax, log_softmax and argmax raise."""
    m = tv._stack()
    prompt = _prompt(kind)
    eos = int(_greedy(kind)[0][0, GREEDY_STEP])
    want, _ = _search(kind, prompt, W4, eos, MAX_NEW)
    armed = []

    def gated(name, real):
        def f(*a, **k):
            if armed:
                raise AssertionError("%s reached in beam_search behind the prefill" % name)
            return real(*a, **k)
        return f
    for mod, name in ((F, "linear"), (torch, "addmm"), (torch, "matmul"), (torch, "topk"), (torch.Tensor, "topk"),
                      (torch, "softmax"), (torch.Tensor, "softmax"), (F, "softmax"), (torch, "log_softmax"),
                      (torch.Tensor, "log_softmax"), (F, "log_softmax"), (torch, "argmax"), (torch.Tensor, "argmax")):
        monkeypatch.setattr(mod, name, gated(name, getattr(mod, name)))
    real_step = m.beam_step

    def arming(*a, **k):
        armed.append(True)
        return real_step(*a, **k)
    monkeypatch.setattr(m, "beam_step", arming)
    try:
        with _Calls() as calls:
            calls.step()
            got, st = _search(kind, prompt, W4, eos, MAX_NEW)
    finally:
        n_steps = len(armed)
        del armed[:]
    assert n_steps == 3 and calls.all().count(BEAM_FN) == 3                # the first pick, the warm-up, the capture
    assert _plain(got) == _plain(want)
