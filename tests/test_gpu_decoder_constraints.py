"""-m gpu: the constrained beam step (C ABI 36; csrc/ea_ceva_decode_vocab.hip: beam_bans_kernel, ceva_vocab_beam_rows_c_kernel;
csrc/ea_voc_ban.h; csrc/ea_adaptive_pick.hip: adaptive_select_c_kernel) and DecoderStack.constrained_beam_search.  Every
comparison is exact -- bits or integers -- against tests/decoder_constraint_reference.py on the kernels' own unconstrained
logits (what the unconstrained entry stores for the same operands).

 1. ea_beam_bans alone over a scripted sequence of steps (hist_tok / hist_par seeded by hand: beams that switch parent, a dead
    beam, a sentence that becomes done): gen[t & 1] is the reference's per-beam tokens, ban[m, :nban[m]] as a set is banned(..),
    n in 0 .. 3, with and without a prompt; the forced step lists nothing; a done sentence's rows are untouched.
 2. one constrained step on the plain head against row_candidates_c and the merge: the row's best logit banned (its tile's
    maximum), a tile banned whole, the tail tile, fewer than 2 W columns unbanned (-inf candidates, an eos at -inf dropped), a
    banned NaN column, eos best while t < min_len, n-grams out of generated tokens, a one-token prompt (L = n - 1, then L = n),
    the forced step, one row at W = 32; lse
    bit-equal to the unconstrained entry's; the -inf columns of the stored logits are the ban set.
 3. the _c entry with nothing to constrain gives the unconstrained entry's bits.
 4. the adaptive head on the small geometry (cutoffs 96, 200, V = 333): bans on both sides of each cutoff, a tail's best token, a
    band banned whole; the sampler's entry keeps its bits.
 5. constrained_beam_search end to end on a tiny stack and on the small adaptive one: replayed == eager == the host search
    driven by the stack's own rows, the promises hold where the unconstrained search breaks them, a second search after
    reset repeats."""
import ctypes
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import adaptive_select_reference as sel                                              # noqa: E402
import decoder_beam_reference as bref                                                # noqa: E402
import decoder_constraint_reference as cref                                          # noqa: E402
import decoder_vocab_operands as ops                                                 # noqa: E402
import test_gpu_adaptive_pick as tap                                                 # noqa: E402
import test_gpu_adaptive_sample as tas                                               # noqa: E402
import test_gpu_decoder_beam as tb                                                   # noqa: E402
import test_gpu_decoder_vocab as tv                                                  # noqa: E402
import test_gpu_vocab_score as tvs                                                   # noqa: E402
from ceva_decoding import _ctx                                                       # noqa: E402

F32 = np.float32
GUARD = -7
BANS_FN, BEAM_C, ADP_C = "ea_beam_bans", "ea_ceva_sdecode_vocab_beam_c", "ea_adaptive_beam_c"


def _r16(n):
    return (n + 15) // 16 * 16


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _same(a, b):
    """fp32 arrays equal bit for bit; a NaN equals a NaN."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int32), b[~nan].view(np.int32))


class Constraint:
    """The constraint operands of one call on the device: the scalars, the prompt [S, prompt_cap] / [S], gen [2, M, max_new]."""

    def __init__(self, S, W, max_new, min_len=0, n=0, bans=(), prompts=None, prompt_cap=0, gen=None):
        M = S * W
        self.S, self.W, self.M, self.max_new = S, W, M, max_new
        self.min_len, self.n, self.bans, self.prompt_cap = min_len, n, tuple(bans), prompt_cap
        self.prompts = [[] for _ in range(S)] if prompts is None else [list(p) for p in prompts]
        assert all(len(p) <= prompt_cap for p in self.prompts)
        tok = np.full((S, max(prompt_cap, 1)), GUARD, dtype=np.int32)
        for s, p in enumerate(self.prompts):
            tok[s, :len(p)] = p
        self.prompt_tok, self.prompt_len = _i32(tok), _i32([len(p) for p in self.prompts])
        self.gen = _i32(np.full((2, M, max_new), GUARD) if gen is None else gen)
        self.cap = prompt_cap + max_new + 17

    def args(self, nv):
        arr = nv.host_array(ctypes.c_int32, list(self.bans)) if self.bans else None
        has = self.prompt_cap > 0
        return [self.min_len, self.n, arr, len(self.bans), nv.ptr(self.prompt_tok) if has else None, self.prompt_cap,
                nv.ptr(self.prompt_len) if has else None, nv.ptr(self.gen)]

    def ban_bytes(self):
        return _r16(4 * self.M * self.cap) + _r16(4 * self.M)

    def read_lists(self, ws, base):
        """-> per row the set ban[m, :nban[m]] out of a workspace whose ban list starts at byte `base`."""
        M, cap = self.M, self.cap
        ban = ws[base:base + 4 * M * cap].view(torch.int32).view(M, cap).cpu().numpy()
        at = base + _r16(4 * M * cap)
        nban = ws[at:at + 4 * M].view(torch.int32).cpu().numpy()
        return ban, nban


# ---- 1. ea_beam_bans alone --------------------------------------------------------------------------------------------------------
def _bans(con, eos, t, done, hist_tok, hist_par, ban, nban):
    from efficient_attention import _native as nv
    a = con.args(nv)
    nv.call(BANS_FN, con.S, con.W, eos, con.max_new, a[0], a[1], a[2], a[3], a[4], a[5], a[6], nv.ptr(t), nv.ptr(done),
            nv.ptr(hist_tok), nv.ptr(hist_par), a[7], nv.ptr(ban), con.cap, nv.ptr(nban), nv.stream())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("with_prompt", [False, True], ids=["no_prompt", "prompt"])
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_ban_list_launch_over_scripted_steps(n, with_prompt):
    S, W, max_new, eos, vocab = 2, 3, 8, 5, 5
    M = S * W
    rng = np.random.RandomState(10 * n + with_prompt)
    prompts = [[3, 1, 3, 1, 2], [4, 0]] if with_prompt else None          # (ragged: 5 and 2 tokens; a bigram seen twice)
    con = Constraint(S, W, max_new, min_len=3, n=n, bans=(7, 2), prompts=prompts, prompt_cap=5 if with_prompt else 0)
    hist_tok, hist_par = _i32(np.full((max_new, M), GUARD)), _i32(np.full((max_new, M), GUARD))
    ban = torch.full((M + 1, con.cap), GUARD, dtype=torch.int32, device="cuda")
    nban = torch.full((M + 1,), GUARD, dtype=torch.int32, device="cuda")
    G = [[] for _ in range(M)]
    done = [0, 0]
    switched = dead = False
    for t in range(max_new):
        forced = t + 1 >= max_new
        if t == 4:
            done[1] = 1                                                    # sentence 1 is done from here on: untouched
        before = (con.gen.clone(), ban.clone(), nban.clone())
        _bans(con, eos, _i32([t] * S), _i32(done), hist_tok, hist_par, ban, nban)
        gen, lists, counts = con.gen.cpu().numpy(), ban.cpu().numpy(), nban.cpu().numpy()
        assert (lists[M] == GUARD).all() and counts[M] == GUARD
        for m in range(M):
            s = m // W
            if done[s]:
                for now, was in zip((con.gen[:, m], ban[m], nban[m]), (before[0][:, m], before[1][m], before[2][m])):
                    assert torch.equal(now, was), ("a done sentence's rows are untouched", t, m)
                continue
            assert gen[t & 1, m, :t].tolist() == G[m], (n, t, m, gen[t & 1, m].tolist(), G[m])
            assert (gen[t & 1, m, t:] == GUARD).all(), "entries from t on are never written"
            x = (con.prompts[s] if with_prompt else []) + G[m]
            want = set() if forced else cref.banned(x, t, n, con.min_len, eos, con.bans)
            assert 0 <= counts[m] <= con.cap and set(lists[m, :counts[m]].tolist()) == want, (n, t, m, x, sorted(want))
            assert not forced or counts[m] == 0
        # the next merge's rows, by hand: parents within the sentence (beams switch), beam 2 of sentence 0 dead from t = 2 on
        tok, par = rng.randint(0, vocab, M), rng.randint(0, W, M)
        for m in range(M):
            if m == 2 and t >= 2:
                tok[m], par[m], dead = eos, 2, True
            switched |= par[m] != m % W
        G = [G[(m // W) * W + par[m]] + [int(tok[m])] if not done[m // W] else G[m] for m in range(M)]
        if t < max_new:
            hist_tok[t], hist_par[t] = _i32(tok), _i32(par)
    assert switched and dead


# ---- 2. one constrained step on the plain head -------------------------------------------------------------------------------------
def _beam_c(M, K, V, xbuf, wbuf, st, eos, con):
    """ea_ceva_sdecode_vocab_beam_c -> tb._beam's dict and the rows' ban sets; the frames are checked."""
    from efficient_attention import _native as nv
    W = st.W
    base = nv.lib().ea_ceva_sdecode_vocab_beam_ws(M, V, W)
    nbytes = nv.lib().ea_ceva_sdecode_vocab_beam_c_ws(M, V, W, con.prompt_cap, con.max_new)
    assert nbytes == base + con.ban_bytes()
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    logits = tv._logit_buffer(M, V, torch.float32)
    ci = torch.full((M + 1, 2 * W), tb.GUARD_I, dtype=torch.int32, device="cuda")
    cs, sv = (torch.full((M + 1, 2 * W), tb.GUARD_F, dtype=torch.float32, device="cuda") for _ in range(2))
    lse = torch.full((M + 1,), tb.GUARD_F, dtype=torch.float32, device="cuda")
    nv.call(BEAM_C, M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf), nv.ptr(logits),
            logits.stride(0), nv.ptr(ws), nbytes, W, eos, st.max_new, *st.ptrs(), *[nv.ptr(t) for t in (ci, cs, lse, sv)],
            *con.args(nv), nv.stream())
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xFF).all() and (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()
    assert (ci[M] == tb.GUARD_I).all() and (cs[M] == tb.GUARD_F).all() and (sv[M] == tb.GUARD_F).all() and lse[M].item() == tb.GUARD_F
    ban, nban = con.read_lists(ws, base)
    return dict(logits=logits[:M, :V], cand_idx=ci[:M], cand_score=cs[:M], sel_val=sv[:M], lse=lse[:M], ban=ban, nban=nban)


def _operands(shape, nan_col=None):
    """(xbuf, wbuf) of a shape, bf16 table, fp32 rows, framed as tests/test_gpu_decoder_vocab.py frames them."""
    M, K, V = shape
    if nan_col is None:
        return tv._case(shape, torch.bfloat16, True)[:2]
    x32, w = ops.operands(shape, torch.bfloat16, 0)
    w[nan_col] = float("nan")
    return tv._rows(M, K, K + 8, torch.float32, x32.cuda()), tv._table(w.cuda())


def _seed_history(st, t, gen_prev, tok, par):
    """Rows t - 1 of the history as a merge would have left them, on the device and the host; -> gen [2, M, max_new]."""
    M = st.M
    gen = np.full((2, M, st.max_new), GUARD, dtype=np.int32)
    if t >= 1:
        gen[(t - 1) & 1, :, :t - 1] = gen_prev
        for k, v in (("hist_tok", tok), ("hist_par", par)):
            st.host[k][t - 1] = v
            st.dev[k][(t - 1) * M:t * M] = _i32(v)
    return gen


def _row_tokens(t, W, gen_prev, tok, par):
    if t < 1:
        return lambda m: []
    return lambda m: [int(v) for v in gen_prev[(m // W) * W + par[m]]] + [int(tok[m])]


def _check_step(shape, S, W, max_new, t, eos, make, nan_col=None, score=None, done=None):
    """make(U) -> dict(min_len, n, bans, prompts, prompt_cap[, gen_prev, tok, par]) from the unconstrained logits U [M, V]."""
    M, K, V = shape
    assert M == S * W
    xbuf, wbuf = _operands(shape, nan_col)
    done = [0] * S if done is None else done
    plain = tb.State(S, W, max_new, score, t=t, done=done)
    un = tb._beam(M, K, V, xbuf, wbuf, plain, eos)
    U, lse = un["logits"].cpu().numpy(), un["lse"].cpu().numpy()
    spec = make(U)
    st = tb.State(S, W, max_new, score, t=t, done=done)
    gen_prev, tok, par = spec.get("gen_prev"), spec.get("tok"), spec.get("par")
    gen = _seed_history(st, t, gen_prev, tok, par)
    con = Constraint(S, W, max_new, spec.get("min_len", 0), spec.get("n", 0), spec.get("bans", ()), spec.get("prompts"),
                     spec.get("prompt_cap", 0), gen)
    got = _beam_c(M, K, V, xbuf, wbuf, st, eos, con)
    tokens_of = _row_tokens(t, W, gen_prev, tok, par)
    forced = t + 1 >= max_new
    k = 1 if forced else min(2 * W, V)
    C = got["logits"].cpu().numpy()
    ci, cs, sv, glse = (got[name].cpu().numpy() for name in ("cand_idx", "cand_score", "sel_val", "lse"))
    h_score = plain.host["score"]
    seen = dict(banned=0, inf_cand=0, ngram=0)
    for m in range(M):
        s = m // W
        if done[s]:
            assert _same(C[m], U[m]) and (ci[m] == tb.GUARD_I).all(), ("a done sentence's rows are skipped", m)
            continue
        want = set() if forced else cref.banned(con.prompts[s] + tokens_of(m), t, con.n, con.min_len, eos, con.bans)
        assert set(got["ban"][m, :got["nban"][m]].tolist()) == want, (m, sorted(want))
        inside = set(v for v in want if 0 <= v < V)
        # the stored logits: -inf at the banned columns, the unconstrained bits elsewhere
        assert set(np.nonzero(np.isneginf(C[m]) & ~np.isneginf(U[m]))[0].tolist()) == set(v for v in inside if not np.isneginf(U[m, v]))
        assert all(np.isneginf(C[m, v]) for v in inside) and _same(np.delete(C[m], sorted(inside)), np.delete(U[m], sorted(inside))), m
        assert _same(glse[m:m + 1], lse[m:m + 1]), ("lse is the unconstrained entry's", m, glse[m], lse[m])
        idx, val, cand = cref.row_candidates_c(U[m], lse[m], h_score[m], W, eos, forced, want)
        assert ci[m, :k].tolist() == idx.tolist(), (m, ci[m].tolist(), idx.tolist(), sorted(want))
        assert _same(sv[m, :k], val) and _same(cs[m, :k], cand), (m, cs[m].tolist(), cand.tolist())
        assert (ci[m, k:] == tb.GUARD_I).all() and (cs[m, k:] == tb.GUARD_F).all()
        seen["banned"] += len(inside)
        seen["ngram"] += len(inside - set(con.bans) - {eos})
        seen["inf_cand"] += int(np.isneginf(val).sum())
    live = [m for m in range(M) if not done[m // W]]
    events = tb._host_merge(st, ci, cs, k, eos)
    tb._equal(st.read(), st.host, (shape, t))
    # .. and the generated tokens the ban-list launch keeps
    g = con.gen.cpu().numpy()
    for m in live:
        assert g[t & 1, m, :t].tolist() == tokens_of(m)
    return dict(U=U, C=C, ci=ci, cs=cs, events=events, seen=seen, st=st)


@pytest.mark.gpu
def test_step_the_rows_best_logit_is_banned_and_its_tile_still_serves():
    shape, S, W = (4, 32, 50), 2, 2
    best = {}

    def make(U):                                                       # n = 1: the prompt's tokens are the bans, per sentence
        best.update({s: [int(U[s * W].argmax()), int(U[s * W + 1].argmax())] for s in range(S)})
        return dict(n=1, prompts=[best[0], best[1] + [3, 3, 60]], prompt_cap=5)      # (ragged 2 / 5; a token past V is skipped)
    out = _check_step(shape, S, W, 6, 0, 1, make, score=-np.arange(4, dtype=F32))
    for s in range(S):
        v = best[s][0]
        assert v not in out["ci"][s * W].tolist()
        # the row's next best unbanned logits are the candidates (the bit-exact comparison above carries the tile's second best)
        order = [c for c in np.argsort(-out["U"][s * W], kind="stable") if c not in best[s] and not (s == 1 and c == 3)]
        assert out["ci"][s * W].tolist() == order[:2 * W]
    assert out["seen"]["banned"] >= 6


@pytest.mark.gpu
def test_step_whole_tiles_and_the_tail_tile_banned():
    shape, S, W = (2, 64, 333), 1, 2
    tiles = list(range(16, 32)) + list(range(320, 333))                # a full tile, and the 13 live columns of the tail tile
    out = _check_step(shape, S, W, 5, 0, 0, lambda U: dict(n=1, prompts=[tiles], prompt_cap=32))
    assert not set(out["ci"].reshape(-1).tolist()) & set(tiles) and np.isneginf(out["C"][:, tiles]).all()
    # V = 17: the tail tile's only live column is the last one; it and the row's best are banned
    out = _check_step((1, 32, 17), 1, 1, 5, 0, 0, lambda U: dict(n=1, prompts=[[16, int(U[0].argmax())]], prompt_cap=2))
    assert 16 not in out["ci"][0, :2].tolist() and np.isneginf(out["C"][0, 16])


@pytest.mark.gpu
def test_step_fewer_unbanned_columns_than_candidates_and_a_dropped_eos():
    shape, S, W = (4, 32, 17), 1, 4                                    # k' = 8 of 17 columns
    ban13 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16]                # with eos (0, by min_len): 14 banned, 3 free
    out = _check_step(shape, S, W, 6, 0, 0, lambda U: dict(n=1, min_len=2, prompts=[ban13], prompt_cap=13))
    assert out["seen"]["inf_cand"] == 4 * 5 and "eos_inf" in out["events"], out["events"]
    assert np.isneginf(out["cs"][:, 3:8]).all() and out["ci"][0, 3] == 0      # the banned ones follow, the lower index first


@pytest.mark.gpu
def test_step_a_banned_nan_column_and_eos_best_under_min_len():
    shape, S, W = (2, 64, 50), 1, 2
    out = _check_step(shape, S, W, 6, 0, 4, lambda U: dict(bans=(20,)), nan_col=20)
    assert np.isnan(out["U"][:, 20]).all() and np.isneginf(out["C"][:, 20]).all() and 20 not in out["ci"][:, :4].reshape(-1).tolist()
    eos = int(tv._case(shape, torch.bfloat16, True)[2][0].argmax())
    for t, banned in ((0, True), (2, True), (3, False)):              # min_len = 3: eos is free from t = 3 on
        rng = np.random.RandomState(t)
        gen_prev, tok, par = rng.randint(5, 9, (2, max(t - 1, 0))), rng.randint(5, 9, 2), rng.randint(0, 2, 2)
        out = _check_step(shape, S, W, 8, t, eos, lambda U: dict(min_len=3, gen_prev=gen_prev, tok=tok, par=par),
                          score=np.array([-1.0, -2.0], dtype=F32))
        assert (eos in out["ci"][0, :4].tolist()) != banned and np.isneginf(out["C"][0, eos]) == banned


@pytest.mark.gpu
@pytest.mark.parametrize("S, W, K", [(2, 4, 64), (1, 32, 32), (2, 1, 32)], ids=["2x4", "1x32", "2x1"])
def test_step_ngrams_of_prompt_and_generated_tokens_the_forced_step_and_a_done_sentence(S, W, K):
    M, V, max_new = S * W, 333 if W == 32 else 50, 9
    shape = (M, K, V)
    prompts = [[9, 4, 9, 4, 7], [4, 9]][:S]
    ngram_bans = 0
    for t in (1, 4, max_new - 1):                                      # .. the last one is the forced step
        rng = np.random.RandomState(100 * W + t)
        gen_prev = rng.randint(4, 10, (M, t - 1))                      # six tokens: bigrams repeat
        tok, par = rng.randint(4, 10, M), rng.randint(0, W, M)
        score = -rng.rand(M).astype(F32) * 5
        done = [0, 1] if (S == 2 and t == 4) else None
        out = _check_step(shape, S, W, max_new, t, 11, lambda U: dict(n=2, min_len=2, bans=(1, 12), prompts=prompts, prompt_cap=5,
                                                                      gen_prev=gen_prev, tok=tok, par=par), score=score, done=done)
        if t == max_new - 1:                                           # constraints ignored: eos alone, nothing stored over
            assert "forced" in out["events"] and tb._bits(torch.from_numpy(out["C"]), torch.from_numpy(out["U"]))
            assert (out["ci"][:, 0] == 11).all() and out["seen"]["banned"] == 0
        else:
            assert out["seen"]["banned"] >= M
            ngram_bans += out["seen"]["ngram"]
    assert ngram_bans > 0, "no bigram of six tokens repeated: the case shows nothing"


@pytest.mark.gpu
def test_step_a_prompt_of_one_token_is_the_first_window_boundary():
    """Prompt length 1 with n = 2: at t = 0, L = n - 1 = 1 and there is no window to compare (nothing but the static ban and
    eos); at t = 1, L = n: window 0 is the prompt's token, and where the beam has just repeated it, its continuation -- that
    same token -- is banned.  Prompt lengths 0 and 1 side by side at S = 2."""
    shape, S, W, max_new = (4, 32, 50), 2, 2, 6
    out = _check_step(shape, S, W, max_new, 0, 3, lambda U: dict(n=2, min_len=1, bans=(9,), prompts=[[7], []], prompt_cap=1))
    assert out["seen"]["ngram"] == 0 and out["seen"]["banned"] == 2 * 4
    tok, par = np.array([7, 8, 7, 7]), np.array([0, 0, 1, 0])         # rows 0, 2, 3 repeat token 7; sentence 1 has no prompt
    out = _check_step(shape, S, W, max_new, 1, 3, lambda U: dict(n=2, bans=(9,), prompts=[[7], []], prompt_cap=1,
                                                                 gen_prev=np.zeros((4, 0), dtype=np.int64), tok=tok, par=par),
                      score=-np.arange(4, dtype=F32))
    assert np.isneginf(out["C"][0, 7]) and not np.isneginf(out["C"][[1, 2, 3], 7]).any() and out["seen"]["ngram"] == 1


# ---- 3. nothing to constrain --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape, S, W", [((3, 288, 40), 1, 3), ((8, 64, 333), 2, 4)], ids=["3x288x40", "8x64x333"])
def test_the_c_entry_with_nothing_to_constrain_is_the_unconstrained_entry(shape, S, W):
    M, K, V = shape
    xbuf, wbuf = _operands(shape)
    eos = int(torch.argsort(tv._case(shape, torch.bfloat16, True)[2][0], descending=True)[1])
    for t in (0, 3, 4):                                                # max_new = 5: t = 4 is the forced step
        score = tb._scores(M, 17 + t) if t else None
        a, b = tb.State(S, W, 5, score, t=t), tb.State(S, W, 5, score, t=t)
        want = tb._beam(M, K, V, xbuf, wbuf, a, eos)
        rng = np.random.RandomState(t)
        gen = _seed_history(b, t, rng.randint(0, V, (M, max(t - 1, 0))), rng.randint(0, V, M), rng.randint(0, W, M))
        for k in ("hist_tok", "hist_par"):                             # (state a has the same history)
            a.host[k][:] = b.host[k]
        got = _beam_c(M, K, V, xbuf, wbuf, b, eos, Constraint(S, W, 5, gen=gen))
        for name in ("logits", "cand_idx", "cand_score", "sel_val", "lse"):
            assert tb._bits(got[name], want[name]), (shape, t, name)
        ra, rb = a.read(), b.read()
        if t:
            ra["hist_tok"][t - 1], ra["hist_par"][t - 1] = rb["hist_tok"][t - 1], rb["hist_par"][t - 1]
        tb._equal(rb, ra, (shape, t))
        assert (got["nban"] == 0).all()


# ---- 4. the adaptive head -----------------------------------------------------------------------------------------------------------
def _adaptive_beam_c(geo, S, W, xbuf, dev, eos, max_new, st, con):
    from efficient_attention import _native as nv
    M = S * W
    cut, dims = geo["cutoffs"], geo["dims"]
    lay = sel.ws_layout(M, cut, dims, W)
    arrays = (nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims))
    nbytes = nv.lib().ea_adaptive_beam_c_ws(M, len(dims), *arrays, W, con.prompt_cap, max_new)
    assert nbytes == lay["total"] + con.ban_bytes()
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    cand_idx = torch.full((M, 2 * W), -9, dtype=torch.int32, device="cuda")
    cand_score = torch.full((M, 2 * W), 9.0, dtype=torch.float32, device="cuda")
    nv.call(ADP_C, M, *tas._args(geo, xbuf, dev), nv.ptr(ws), nbytes, W, eos, max_new, *[nv.ptr(st[k]) for k in tas.STATE],
            nv.ptr(cand_idx), nv.ptr(cand_score), *con.args(nv), nv.stream())
    torch.cuda.synchronize()
    assert (ws[-16:] == 0xFF).all()
    out = tas._parts(geo, M, lay, ws)
    ban, nban = con.read_lists(ws, lay["total"])
    out.update(cand_idx=cand_idx, cand_score=cand_score, ban=ban, nban=nban)
    return out


@pytest.mark.gpu
def test_adaptive_step_bans_across_the_bands_and_the_sampler_keeps_its_bits():
    m, _ = tap._fixture()
    S, W, max_new = 2, 2, 6
    M = S * W
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tables = tap._state(m, M, 8).adaptive.tables
    cut, dims = tables.cutoff, tables.dims
    assert cut == [96, 200, 333]
    geo, dev = dict(C=128, cutoffs=cut, dims=dims), (tables.head, tables.proj, tables.tables)
    x32 = torch.randn(M, 128, generator=torch.Generator().manual_seed(36))
    xbuf = tvs._xbuf(x32, tables.dtype, True)
    sampled = tas._sample(geo, M, xbuf, dev, 8)
    base = [0, 96, 200]
    for t, eos in ((0, 5), (max_new - 1, 150)):
        score = np.array([0.0, -1.5, -0.25, -3.0], dtype=F32)
        st_u = tas._beam_state(S, W, max_new, [t] * S, [0] * S, [0] * S, score)
        un = tas._beam(geo, S, W, xbuf, dev, eos, max_new, st_u)
        U, cls, lse = tas._host(un)
        # sentence 0: both sides of each cutoff, the last tail's best token of row 0, the head's best; sentence 1: band 1 whole
        p0 = [95, 96, 199, 200, 200 + int(U[2][0].argmax()), int(U[0][0].argmax())]
        p1 = list(range(96, 200)) + [0]
        st = tas._beam_state(S, W, max_new, [t] * S, [0] * S, [0] * S, score)
        con = Constraint(S, W, max_new, min_len=2, n=1, bans=(332,), prompts=[p0, p1], prompt_cap=120)
        got = _adaptive_beam_c(geo, S, W, xbuf, dev, eos, max_new, st, con)
        C, cls_c, lse_c = tas._host(got)
        forced = t + 1 >= max_new
        masked = [u.copy() for u in U]
        for r in range(M):
            want = set() if forced else cref.banned([p0, p1][r // W], t, 1, 2, eos, (332,))
            assert set(got["ban"][r, :got["nban"][r]].tolist()) == want
            for v in want:
                b = max(i for i in range(3) if v >= base[i])
                masked[b][r, v - base[b]] = -np.inf
        for b in range(3):
            assert _same(C[b], masked[b]) and _same(lse_c[b], lse[b]), ("band", b, t)
        assert _same(cls_c, cls)
        idx, val, joint = sel.select(masked, cls, lse, cut, 2 * W)
        if forced:
            idx, val = np.full((M, 1), eos), sel.eos_score(joint, cut, eos)[:, None]
        ci, cs = sel.beam_candidates(idx, val, score)
        k = ci.shape[1]
        assert np.array_equal(got["cand_idx"].cpu().numpy()[:, :k], ci) and _same(got["cand_score"].cpu().numpy()[:, :k], cs), t
        if not forced:
            assert not set(ci[:W].reshape(-1).tolist()) & set(p0 + [332, eos]) and not set(ci[W:].reshape(-1).tolist()) & set(p1)
        # the merge behind it: the reference on these candidates
        for s in range(S):
            rows = slice(s * W, s * W + W)
            want = bref.merge(ci[rows], cs[rows], min(2 * W, 333), W, eos, t, 0, 0, forced)
            assert st["token"][rows].tolist() == want["token"] and st["parent"][rows].tolist() == [s * W + b for b in want["parent"]]
            assert _same(st["score"][rows].cpu().numpy(), want["score"]) and st["t"][s].item() == t + 1
    again = tas._sample(geo, M, xbuf, dev, 8)
    for key in ("token", "logp", "sel_idx", "sel_val", "kept"):
        assert tb._bits(again[key], sampled[key]), key


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------
C5, V5, P5, MAX_NEW5, S5, W5 = 64, 50, 5, 10, 2, 3
LIMITS = dict(min_len=3, no_repeat_ngram_size=2)


@functools.lru_cache(maxsize=None)
def _tiny():
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(36)
    m = DecoderStack(V5, C5, 128, 1, 2, tv.ATTN).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        m.embed_tokens.weight.mul_(1.0 / 8)
    return m.eval()


def _tiny_state(m, case, M, **kw):
    opt = dict(hold_vocab=True, **kw)
    if case == "per_sequence_ragged":
        opt["per_sequence"] = True
    return m.init_decoding(M, P5 + MAX_NEW5 + 2, torch.bfloat16, "cuda", **opt)


def _tiny_prompt(m, case):
    prompt = torch.randint(2, V5, (S5, P5), generator=torch.Generator().manual_seed(5)).cuda()
    prompt[:, 3] = prompt[:, 1]                                        # (a repeated token: bigrams of the prompt count)
    prompt[prompt == m.pad_idx] = 2
    if case == "per_sequence_ragged":
        prompt[0, 2:] = m.pad_idx                                      # lengths (2, 5)
    return prompt


def _host_search_tiny(m, case, prompt, eos, limits, bans):
    """host_beam_search_c driven by the stack's own rows: next_tokens(return_logits=True), token_logprobs(return_lse=True)."""
    M = S5 * W5
    st = m.init_logprobs(_tiny_state(m, case, M))
    fed = prompt.repeat_interleave(W5, 0)

    def step_fn(tokens, parent):
        if tokens is None:
            last = m._prefill(fed, st)
        else:
            m.reorder_decoding_state(st, torch.from_numpy(parent).cuda())
            last = m.decode(torch.from_numpy(tokens).cuda().view(1, M), st)
        _, logits = m.next_tokens(last, st, return_logits=True)
        _, _, lse = m.token_logprobs(last, st, return_lse=True)
        return logits[0].cpu().numpy(), lse[0].cpu().numpy()
    lists = [[int(v) for v in row if int(v) != m.pad_idx] if case == "per_sequence_ragged" else row.tolist() for row in prompt.cpu()]
    return cref.host_beam_search_c(step_fn, S5, W5, eos, MAX_NEW5, 1.0, lists, limits.get("no_repeat_ngram_size", 0),
                                   limits.get("min_len", 0), bans), lists


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "per_sequence_ragged"])
def test_constrained_beam_search_replayed_equals_eager_equals_the_host_search(case):
    m = _tiny()
    prompt = _tiny_prompt(m, case)
    bans = (m.pad_idx,)
    with torch.no_grad(), _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # eos: the token greedy decoding emits first for sentence 0, so that the unconstrained search ends a hypothesis at once
        eos = int(m.generate(prompt, 1, _tiny_state(m, case, S5), graph=False)[0, 0])
        assert eos != m.pad_idx
        kw = dict(beam_size=W5, eos_idx=eos, max_new=MAX_NEW5)
        found = {}
        for graph in (True, False):
            st = _tiny_state(m, case, S5 * W5)
            found[graph] = m.constrained_beam_search(prompt, st, graph=graph, ban_tokens=bans, **LIMITS, **kw)
            torch.cuda.synchronize()
        (host, info), lists = _host_search_tiny(m, case, prompt, eos, LIMITS, bans)
        (plain, _), _ = _host_search_tiny(m, case, prompt, eos, {}, ())
        device_plain = m.beam_search(prompt, _tiny_state(m, case, S5 * W5), **kw)
        # a second search on the same beam after reset repeats the first (the attention's own state is fresh)
        again = _tiny_state(m, case, S5 * W5)
        again.beam = st.beam
        m.reset_beam_search(again)
        repeated = m.beam_search(prompt, again, **kw)
    assert tb._plain(found[True]) == tb._plain(found[False]) == tb._plain(host) == tb._plain(repeated)
    assert tb._plain(device_plain) == tb._plain(plain)
    check = lambda s, h: cref.violations(lists[s], h["tokens"], eos, MAX_NEW5, 2, 3, bans)      # noqa: E731
    broken = [check(s, h) for s in range(S5) for h in plain[s]]
    assert any(broken), "the unconstrained search must break a promise, or this test shows nothing"
    assert all(len(found[True][s]) >= 1 for s in range(S5))
    for s in range(S5):
        for h in found[True][s]:
            assert not check(s, h), (s, h["tokens"].tolist(), check(s, h))
            assert len(h["tokens"]) - 1 >= 3 and m.pad_idx not in h["tokens"].tolist()[:-1]
    assert any(bset for _, _, _, bset in info["bans"])
    print(case, "eos", eos, "constrained", [[h["tokens"].tolist() for h in hs] for hs in found[True]], "plain",
          [[list(h["tokens"]) for h in hs] for hs in plain], sorted(info["events"]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "per_sequence_ragged"])
def test_constrained_beam_search_from_the_adaptive_head(case):
    """Replayed == eager == host_beam_search_c over the kernel's own joint rows (the stored band logits, cls and lse of every
    step, as tests/test_gpu_adaptive_sample.py drives the unconstrained search), driven through decode / beam_step /
    reorder_decoding_state: the host keeps every beam's tokens by the parents itself and applies its own bans, the device's
    tokens and parents are compared at every step, and the -inf columns the device stored are the host's ban set, row by row.
    The promises hold where the unconstrained search on the same model breaks one."""
    m, tokens = tap._fixture()
    S, W, max_new, P = 2, 4, 8, 9
    M, V = S * W, 333
    prompt = tokens[:S, :P].clone()
    opt, lens = {}, [P] * S
    if case == "per_sequence_ragged":
        opt["per_sequence"] = True
        prompt[1, 5:] = m.pad_idx
        lens = [P, 5]
    lists = [row[:n] for row, n in zip(prompt.cpu().tolist(), lens)]
    bans = (m.pad_idx,)
    with torch.no_grad(), _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eos = int(m.generate(prompt, 1, tap._state(m, S, P + 2, **opt), graph=False)[0, 0])
        kw = dict(beam_size=W, eos_idx=eos, max_new=max_new)
        found = {}
        for graph in (True, False):
            with tas._Entries() as calls:
                real = calls.nv.call

                def call(name, *a, names=calls.names, real=real):
                    if name == ADP_C:
                        names.append(name)
                    return real(name, *a)
                calls.nv.call = call
                st = tap._state(m, M, P + max_new, **opt)
                found[graph] = m.constrained_beam_search(prompt, st, graph=graph, ban_tokens=bans, **LIMITS, **kw)
            if graph:
                assert calls.names == [ADP_C] * 3, calls.names          # the first pick, the warm-up, the capture
        plain = m.beam_search(prompt, tap._state(m, M, P + max_new, **opt), **kw)
        again = tap._state(m, M, P + max_new, **opt)
        again.beam = st.beam
        m.reset_beam_search(again)
        repeated = m.beam_search(prompt, again, **kw)

        # the host search over the kernel's own joint rows
        sh = m.init_beam_search(tap._state(m, M, P + max_new, **opt), W, eos, max_new)
        m.init_beam_constraints(sh, ban_tokens=bans, prompt_cap=P, **LIMITS)
        m.set_beam_prompt(sh, prompt, torch.tensor(lens))
        tbl = sh.adaptive.tables
        geo = dict(C=128, cutoffs=tbl.cutoff, dims=tbl.dims)
        fed = prompt.repeat_interleave(W, 0)
        seen = []

        def step_fn(toks, parent):
            if toks is None:
                rows = m._prefill(fed, sh)
            else:
                assert torch.equal(torch.from_numpy(toks).cuda(), step_fn.tok[0]) and torch.equal(torch.from_numpy(parent).cuda(), step_fn.par)
                rows = m.decode(step_fn.tok, sh)
            done = sh.beam.done.tolist()
            tok, par = m.beam_step(rows, sh)
            torch.cuda.synchronize()
            forced = len(seen) + 1 >= max_new
            stored = tas._parts(geo, M, sel.ws_layout(M, tbl.cutoff, tbl.dims, W), sh.beam.ws)["logits"]
            neg = np.concatenate([np.isneginf(t.cpu().numpy()) for t in stored], 1)
            seen.append((done, [set(np.nonzero(neg[r])[0].tolist()) for r in range(M)]))
            joint = tas._joint_rows(m, sh, rows, W, masked=not forced)
            step_fn.tok, step_fn.par = tok.clone(), par.clone()
            m.reorder_decoding_state(sh, par)
            return joint, np.zeros(M, dtype=F32)
        hyps, info = cref.host_beam_search_c(step_fn, S, W, eos, max_new, 1.0, lists, LIMITS["no_repeat_ngram_size"],
                                             LIMITS["min_len"], bans)
    assert tb._plain(found[True]) == tb._plain(found[False]) == tb._plain(repeated)
    for s in range(S):
        assert len(found[True][s]) == len(hyps[s]) >= 1, (case, s)
        for a, h in zip(found[True][s], hyps[s]):
            assert a["tokens"].tolist() == h["tokens"], (case, s, a["tokens"].tolist(), h["tokens"])
            assert a["raw_score"].numpy().tobytes() == F32(h["raw"]).tobytes(), (case, s)
            assert a["score"] == pytest.approx(h["score"], rel=1e-12)
    # what the device stored at -inf is what the host banned: every live row of every unforced step
    checked = ngram = 0
    for s, b, t, bset in info["bans"]:
        done, neg = seen[t]
        if not done[s]:
            assert neg[s * W + b] == set(v for v in bset if 0 <= v < V), (case, s, b, t, sorted(bset), sorted(neg[s * W + b]))
            checked += 1
            ngram += len(bset - set(bans) - {eos})
    assert checked >= M * 3 and ngram > 0 and info["steps"] >= 4
    check = lambda s, h: cref.violations(lists[s], h["tokens"].tolist(), eos, max_new, 2, 3, bans)      # noqa: E731
    assert any(check(s, h) for s in range(S) for h in plain[s]), "the unconstrained search must break a promise"
    for s in range(S):
        for h in found[True][s]:
            assert not check(s, h), (s, h["tokens"].tolist(), check(s, h))
    print(case, "eos", eos, "steps", info["steps"], sorted(info["events"]), [[h["tokens"] for h in hs] for hs in hyps])
