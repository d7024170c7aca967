"""-m gpu: the many-row vocabulary pass (csrc/ea_vocab_score.hip, ea_vocab_score, C ABI 30) and DecoderStack.rows_logprobs /
evaluate.

Kernel, with BM the row tile, BN the column block and SL the slice width of the library, at the shapes
  (65, 32, 16)                   one k-step, one 16-column tile, the first M beyond the few-row envelope
  (BM + 1, 288, 40)              a second row tile holding one row, a tail of 8 columns, K no multiple of a 64-wide stage
  (2 BM + 3, 256, BN + 24)       a second column block that is nearly empty
  (BM, 1056, SL + BN + 8)        a second slice, a second pass over K, V % 16 = 8
  (3, 1024, 2 SL + 1000)         fewer rows than one MFMA row tile, three slices
  (384, 1024, 32768), once       the LM table: 16 slices in the second launch
bf16 and fp16 tables, x in fp32 and in the table's type, in the framed buffers of tests/test_gpu_decoder_vocab.py:

 1. stored fp32 logits within decoder_vocab_operands.bound of the fp64 products of the rounded operands; the 16-bit store is
    the fp32 store rounded once; frames intact (rows >= M, columns >= V, the guard behind every output, the workspace's end).
 2. token, top, lse, logp have the same bits with and without logits, with and without top.
 3. token / top == torch.argmax / max of the kernel's own fp32 logits; decoder_vocab_operands.tie, four cases; nan_rows;
    equal logits, and two NaNs, in ONE lane of two column blocks (columns a and a + n BN).
 4. |lse - lse64| <= vocab_score_reference.tol, lse64 the fp64 log-sum-exp of the kernel's own logits; the tolerance itself
    may not exceed 2^-16 max(1, |lse64|).  The largest |lse - lse64| / tol is printed.
 5. logp has the bits of fp32(tl - lse): no targets, targets 0, V - 1, the pick, a column per row, and a sweep in which every
    column of the last column block and of the last slice is somebody's target; targets -1, V, +-2^40 give NaN in their rows.
 6. logits near -300 and +300; a +inf logit; one -inf logit; a whole slice of -inf under a finite negative top; all -inf.
 7. a call on M rows == calls on each single row, on the two halves, on the rows reversed, bit for bit; a call repeats.
 8. on 64 rows of the third shape: token agrees with ea_ceva_sdecode_vocab_logprob wherever that entry's top-two margin
    exceeds 2 bound[m]; lse within the two tolerances summed.
 9. the stack of tests/test_gpu_decoder_vocab.py, bf16, 130 rows: rows_logprobs against token_logprobs by 8's criterion;
    evaluate from the rows on with the framework's GEMMs, log_softmax, logsumexp, cross_entropy and argmax replaced by
    functions that raise; evaluate == rows_logprobs on the full path's rows, bit for bit; pad targets score 0; evaluate within
    tol + 2 bound of fp64 log_softmax values."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_decoder_vocab as tv                    # the framed buffers, _bits, the stack
import test_gpu_decoder_logprob as tl                  # the few-row entry's caller, _one_signed, _edited
import decoder_logprob_reference as lref
import decoder_vocab_operands as ops
import vocab_score_reference as ref
from ceva_decoding import _ctx

FN = "ea_vocab_score"
BM, BN, SL = ref.constants()
SHAPES = [(65, 32, 16), (BM + 1, 288, 40), (2 * BM + 3, 256, BN + 24), (BM, 1056, SL + BN + 8), (3, 1024, 2 * SL + 1000)]
LM = (384, 1024, 32768)
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
_ids = tv._ids
_bits = tv._bits
INF, NAN = float("inf"), float("nan")
KEYS = ("token", "top", "lse", "logp")


def _score(M, K, V, xbuf, wbuf, logits=None, targets=None, top=True):
    """-> dict(token [M] int64, top [M] or None, lse [M], logp [M]); every output has a guard element that must stay."""
    from efficient_attention import _native as nv
    nbytes = nv.lib().ea_vocab_score_ws(M, V)
    assert nbytes == (12 * M * (-(-V // SL)) + 4 * M + 15) // 16 * 16
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")   # (stale partials would be NaNs)
    token = torch.full((M + 1,), -7, dtype=torch.long, device="cuda")
    t = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda") if top else None
    lse = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    logp = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    if targets is not None:
        targets = torch.as_tensor(targets, dtype=torch.long).cuda()
        assert tuple(targets.shape) == (M,)
    nv.call(FN, M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf), nv.ptr(targets),
            nv.ptr(logits), 0 if logits is None else tv._code(logits), 0 if logits is None else logits.stride(0), nv.ptr(ws),
            nbytes, nv.ptr(token), nv.ptr(t), nv.ptr(lse), nv.ptr(logp), nv.stream())
    torch.cuda.synchronize()
    assert token[M].item() == -7 and (t is None or t[M].item() == 7.0) and lse[M].item() == 7.0 and logp[M].item() == 7.0
    assert (ws[nbytes:] == 0xFF).all()                                   # the workspace ends where the query says
    if logits is not None:
        assert (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()
    return dict(token=token[:M], top=None if t is None else t[:M], lse=lse[:M], logp=logp[:M])


def _same(a, b, keys=KEYS):
    return all(_bits(a[k], b[k]) for k in keys)


def _xbuf(x32, wdtype, x_f32):
    M, K = x32.shape
    return tv._rows(M, K, K + 8, torch.float32 if x_f32 else wdtype, x32.cuda() if x_f32 else x32.to(wdtype).cuda())


@functools.lru_cache(maxsize=4)
def _host(shape, wdtype):
    """fp64 products of the rounded plain operands and the bound of their fp32 sums, once per (shape, type): CPU, never written."""
    x32, w = ops.operands(shape, wdtype, 0)
    xh = x32.to(wdtype)
    return xh.double() @ w.double().t(), ops.bound(xh, w)


@functools.lru_cache(maxsize=8)
def _case(shape, wdtype, x_f32):
    """The plain operands in their frames, the kernel's own fp32 logits and its results, once (never written)."""
    M, K, V = shape
    x32, w = ops.operands(shape, wdtype, 0)
    xbuf, wbuf = _xbuf(x32, wdtype, x_f32), tv._table(w.cuda())
    logits = tv._logit_buffer(M, V, torch.float32)
    got = _score(M, K, V, xbuf, wbuf, logits)
    return xbuf, wbuf, logits, got


def _check_lse(got, logits, M, V, what):
    """4: the kernel's lse against the fp64 log-sum-exp of its own stored logits -> the largest |lse - lse64| / tol."""
    L = logits[:M, :V].cpu().numpy()
    lse = got["lse"].cpu().numpy()
    worst = 0.0
    for m in range(M):
        want = lref.lse(L[m])
        assert np.isfinite(want), (what, m)
        tol = ref.tol(L[m], want)
        assert tol <= 2.0 ** -16 * max(1.0, abs(want)), (what, m, tol, want)   # the condition on the design
        err = abs(float(lse[m]) - want)
        if err > tol:
            print(what, "row", m, "lse %.9g lse64 %.12g |diff| %.3e tol %.3e ratio %.4f" % (lse[m], want, err, tol, err / tol))
        assert err <= tol, (what, m, float(lse[m]), want, err, tol)
        worst = max(worst, err / tol)
    return worst


@pytest.mark.gpu
def test_the_librarys_constants_are_the_shapes():
    from efficient_attention import _native as nv
    assert nv.vocab_score_tiles() == (BM, BN, SL)


# ---- 1 .. 5 on the plain operands -----------------------------------------------------------------------------------------------
def _sweep_targets(M, V):
    """Target lists [M] that between them name every column of the last column block and of the last slice."""
    first = min((V - 1) // SL * SL, (V - 1) // BN * BN)
    cols = list(range(first, V))
    return [[cols[(i + m) % len(cols)] for m in range(M)] for i in range(0, len(cols), M)], cols


def _plain(shape, wdtype, x_f32s=(True, False)):
    M, K, V = shape
    worst_lse, worst_logit = 0.0, 0.0
    L64, bound = _host(shape, wdtype)
    for x_f32 in x_f32s:
        what = (shape, wdtype, x_f32)
        xbuf, wbuf, logits, got = _case(shape, wdtype, x_f32)
        L = logits[:M, :V]
        # 1
        assert torch.isfinite(L).all()
        ratio = ((L.cpu().double() - L64).abs() / bound.unsqueeze(1)).max().item()
        worst_logit = max(worst_logit, ratio)
        assert ratio <= 1.0, (what, ratio)
        l16 = tv._logit_buffer(M, V, wdtype)
        got16 = _score(M, K, V, xbuf, wbuf, l16)
        assert _bits(l16[:M, :V], L.to(wdtype)), what
        # 2
        none = _score(M, K, V, xbuf, wbuf, None)
        assert _same(got, got16) and _same(got, none), what
        notop = _score(M, K, V, xbuf, wbuf, None, top=False)
        assert notop["top"] is None and _same(got, notop, ("token", "lse", "logp")), what
        assert _same(got, _score(M, K, V, xbuf, wbuf, tv._logit_buffer(M, V, torch.float32), top=False), ("token", "lse", "logp"))
        # 3
        assert torch.equal(got["token"], torch.argmax(L, dim=1)), what
        assert _bits(got["top"], L.max(dim=1).values), what
        # 4
        worst_lse = max(worst_lse, _check_lse(got, logits, M, V, what))
        # 5
        assert _bits(got["logp"], got["top"] - got["lse"]), what
        rows = torch.arange(M, device="cuda")
        named = [("first", [0] * M), ("last", [V - 1] * M), ("pick", got["token"].tolist()),
                 ("per_row", [(7 * m + 3) % V for m in range(M)])]
        sweep, cols = _sweep_targets(M, V)
        seen = set()
        for name, tg in named + [("sweep", tg) for tg in sweep]:
            t = _score(M, K, V, xbuf, wbuf, None, targets=tg)
            assert _same(t, got, ("token", "top", "lse")), (what, name)
            want = L[rows, torch.tensor(tg, device="cuda")] - got["lse"]
            assert _bits(t["logp"], want), (what, name, tg[:4])
            if name == "pick":
                assert _bits(t["logp"], got["logp"])
            if name == "sweep":
                seen.update(tg)
        assert seen == set(cols) and V - 1 in seen and (V - 1) // SL * SL in seen and (V - 1) // BN * BN in seen
        t = _score(M, K, V, xbuf, wbuf, tv._logit_buffer(M, V, torch.float32), targets=named[3][1])
        assert _bits(t["logp"], L[rows, torch.tensor(named[3][1], device="cuda")] - got["lse"]), what
        for bad in (-1, V, -(1 << 40), 1 << 40):
            t = _score(M, K, V, xbuf, wbuf, None, targets=[bad] * M)
            assert torch.isnan(t["logp"]).all() and _same(t, got, ("token", "top", "lse")), (what, bad)
            tg = [0] * M                                 # one bad target among good ones: NaN in its row only
            tg[M // 2] = bad
            t = _score(M, K, V, xbuf, wbuf, None, targets=tg)
            keep = torch.ones(M, dtype=torch.bool, device="cuda")
            keep[M // 2] = False
            assert math.isnan(t["logp"][M // 2].item()) and _bits(t["logp"][keep], (L[:, 0] - got["lse"])[keep]), (what, bad)
    return worst_lse, worst_logit


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_logits_storage_pick_lse_and_target_logits(wdtype, shape):
    worst_lse, worst_logit = _plain(shape, wdtype)
    print(shape, wdtype, "largest |lse - lse64| / tol: %.4f; largest |logit - L64| / bound: %.4f" % (worst_lse, worst_logit))


@pytest.mark.gpu
def test_the_lm_table_with_sixteen_slices():
    assert -(-LM[2] // SL) >= 2 and LM[0] % BM == 0
    worst_lse, worst_logit = _plain(LM, torch.bfloat16, x_f32s=(True,))
    print(LM, "largest |lse - lse64| / tol: %.4f; largest |logit - L64| / bound: %.4f" % (worst_lse, worst_logit))


# ---- 3. ties and NaN ------------------------------------------------------------------------------------------------------------
def _ties(shape, wdtype):
    M, K, V = shape
    ran = []
    for case in ops.TIE_CASES:
        got = ops.tie(shape, wdtype, 0, case)
        if got is None:                                  # (the single-tile shape has no pair in two tiles)
            continue
        x32, w, a, b = got
        ran.append(case)
        if shape != LM:                                  # the operands' stated precondition, in fp64
            margin, equal = ops.tie_margin(x32, w, a, b)
            assert margin > 0.0 and equal, (shape, wdtype, case, margin, equal)
        wbuf = tv._table(w.cuda())
        for x_f32 in ((True,) if shape == LM else (True, False)):
            xbuf = _xbuf(x32, wdtype, x_f32)
            logits = tv._logit_buffer(M, V, torch.float32)
            r = _score(M, K, V, xbuf, wbuf, logits)
            assert r["token"].tolist() == [a] * M, (shape, wdtype, case, x_f32, a, b, r["token"].tolist()[:8])
            assert _bits(logits[:M, a], logits[:M, b]) and _bits(r["top"], logits[:M, a])
            assert _same(r, _score(M, K, V, xbuf, wbuf, None))
    assert ran == ops.TIE_CASES or (V == 16 and ran == ["one_tile", "ends"]), ran
    if V > SL:                                           # the four cases: one tile, two column blocks, two slices, the ends
        assert ops.tie_indices(V, "two_workgroups")[1] // BN > 0 and ops.tie_indices(V, "tail")[1] // SL > 0


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_of_two_equal_logits_the_lower_index_wins(wdtype, shape):
    _ties(shape, wdtype)


@pytest.mark.gpu
def test_ties_on_the_lm_table():
    """(The construction of decoder_vocab_operands.tie at K = 1024, V = 32768, whose precondition tests/test_decoder_vocab_cpu.py
    checks in fp64 at its own LM shapes; not checked again here: two 384 x 32768 x 1024 fp64 products per case.)"""
    _ties(LM, torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES[2:], ids=_ids(SHAPES[2:]))
def test_equal_logits_in_one_lane_of_two_column_blocks(wdtype, shape):
    """Columns a and a + n BN are held by the SAME lane (equal v % 16, equal 64-column half) in different column blocks: the
    running pick in registers must keep the earlier one -- equal numbers, and two NaNs.  The pairs of decoder_vocab_operands
    never meet in a lane.  Built on its "one_tile" tie (a = 1, precondition checked here in fp64): the winning row is copied
    to a + BN and, where the table has it, to the last column a + n BN."""
    M, K, V = shape
    x32, w, a, b = ops.tie(shape, wdtype, 0, "one_tile")
    margin, equal = ops.tie_margin(x32, w, a, b)
    assert margin > 0.0 and equal, (shape, wdtype, margin, equal)
    later = sorted({a + BN, a + (V - 1 - a) // BN * BN})
    assert all(a < c < V and c % 16 == a % 16 and (c % BN) // 64 == (a % BN) // 64 and c // BN > a // BN for c in later)
    w[later] = w[a].clone()
    _, wn, _ = ops.nan_rows(shape, wdtype, 0, False)
    wn[V // 2] = ops.operands(shape, wdtype, 0)[1][V // 2]                # (that helper's own NaN row: back to a number)
    nan_cols = [5, 5 + BN * ((V - 6) // BN)]                               # one lane again, the first and the last block
    assert nan_cols[1] > nan_cols[0] and nan_cols[1] < V
    wn[nan_cols] = float("nan")
    for x_f32 in (True, False):
        xbuf = _xbuf(x32, wdtype, x_f32)
        logits = tv._logit_buffer(M, V, torch.float32)
        r = _score(M, K, V, xbuf, tv._table(w.cuda()), logits)
        assert r["token"].tolist() == [a] * M, (shape, wdtype, x_f32, a, later, r["token"].tolist()[:8])
        assert all(_bits(logits[:M, a], logits[:M, c]) for c in later) and _bits(r["top"], logits[:M, a])
        assert _same(r, _score(M, K, V, xbuf, tv._table(w.cuda()), None))
        xplain = _case(shape, wdtype, x_f32)[0]
        logits = tv._logit_buffer(M, V, torch.float32)
        r = _score(M, K, V, xplain, tv._table(wn.cuda()), logits)
        assert r["token"].tolist() == [nan_cols[0]] * M, (shape, wdtype, x_f32, nan_cols, r["token"].tolist()[:8])
        assert torch.equal(torch.isnan(logits[:M, :V]).nonzero()[:, 1].unique().cpu(), torch.tensor(sorted(set(nan_cols))))
        assert torch.isnan(r["top"]).all() and torch.isnan(r["lse"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_a_nan_logit_is_picked_and_of_two_the_lower_index(wdtype, shape):
    M, K, V = shape
    for two in (False, True):
        _, w, rows = ops.nan_rows(shape, wdtype, 0, two)
        wbuf = tv._table(w.cuda())
        for x_f32 in (True, False):
            xbuf = _case(shape, wdtype, x_f32)[0]
            for logits in (tv._logit_buffer(M, V, torch.float32), None):
                r = _score(M, K, V, xbuf, wbuf, logits, targets=[0] * M)
                assert r["token"].tolist() == [rows[0]] * M, (shape, wdtype, x_f32, rows, r["token"].tolist()[:8])
                assert torch.isnan(r["top"]).all() and torch.isnan(r["lse"]).all() and torch.isnan(r["logp"]).all()
                if logits is not None:
                    assert torch.equal(torch.isnan(logits[:M, :V]).nonzero()[:, 1].unique().cpu(), torch.tensor(rows))
                    assert torch.equal(torch.argmax(logits[:M, :V].cpu(), dim=1), r["token"].cpu())   # torch.argmax's own rule


# ---- 6. range and special values ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("sign", [-1.0, 1.0], ids=["near_minus_300", "near_plus_300"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_logits_near_minus_and_plus_300(shape, sign, wdtype):
    M, K, V = shape
    x32, w = tl._one_signed(shape, wdtype, sign)
    wbuf = tv._table(w.cuda())
    for x_f32 in (True, False):
        xbuf = _xbuf(x32, wdtype, x_f32)
        logits = tv._logit_buffer(M, V, torch.float32)
        got = _score(M, K, V, xbuf, wbuf, logits)
        L = logits[:M, :V]
        assert torch.isfinite(L).all() and (L * sign > 100.0).all() and (L * sign).mean().item() > 250.0
        worst = _check_lse(got, logits, M, V, (shape, wdtype, sign, x_f32))
        print(shape, wdtype, sign, "largest |lse - lse64| / tol: %.4f" % worst)
        assert _bits(got["logp"], got["top"] - got["lse"]) and _same(got, _score(M, K, V, xbuf, wbuf, None))


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_special_values(wdtype, shape):
    M, K, V = shape
    NS = -(-V // SL)
    for x_f32 in (True, False):
        # a +inf logit
        v = V // 2
        x32, w = tl._edited(shape, wdtype, [v], INF)
        xb = _xbuf(x32, wdtype, x_f32)
        got = _score(M, K, V, xb, tv._table(w.cuda()), None, targets=[0] * M)
        assert got["token"].tolist() == [v] * M and (got["top"] == INF).all() and (got["lse"] == INF).all()
        assert (got["logp"] == -INF).all()               # (a finite logit under an infinite normaliser)
        # one -inf logit under a finite top
        v = V - 1
        x32, w = tl._edited(shape, wdtype, [v], -INF)
        xb = _xbuf(x32, wdtype, x_f32)
        logits = tv._logit_buffer(M, V, torch.float32)
        got = _score(M, K, V, xb, tv._table(w.cuda()), logits, targets=[v] * M)
        assert (logits[:M, v] == -INF).all() and int(torch.isinf(logits[:M, :V]).sum()) == M
        _check_lse(got, logits, M, V, (shape, wdtype, x_f32, "one -inf"))
        assert (got["logp"] == -INF).all() and torch.isfinite(got["top"]).all() and (got["token"] != v).all()
        assert _same(got, _score(M, K, V, xb, tv._table(w.cuda()), None, targets=[v] * M))
        # a whole slice of -inf logits under a finite, negative top (a table of at least two slices); and, in every shape of
        # more than one column block, a whole column block
        groups = [("a column block", list(range(BN * ((V - 1) // BN // 2), min(V, BN * ((V - 1) // BN // 2) + BN))))] \
            if V > BN else []
        if NS >= 2:
            groups.append(("a slice", list(range(SL * (NS // 2), min(V, SL * (NS // 2) + SL)))))
        for name, cols in groups:
            x32, w = tl._edited(shape, wdtype, cols, -INF, negative=True)
            xb = _xbuf(x32, wdtype, x_f32)
            logits = tv._logit_buffer(M, V, torch.float32)
            got = _score(M, K, V, xb, tv._table(w.cuda()), logits)
            assert (logits[:M, cols] == -INF).all() and (got["top"] < 0).all() and torch.isfinite(got["top"]).all()
            assert torch.isfinite(got["lse"]).all() and len(cols) < V
            worst = _check_lse(got, logits, M, V, (shape, wdtype, x_f32, name))
            print(shape, wdtype, x_f32, name, "of -inf: largest |lse - lse64| / tol: %.4f" % worst)
            assert _same(got, _score(M, K, V, xb, tv._table(w.cuda()), None))
        # every logit -inf
        x32, w = tl._edited(shape, wdtype, list(range(V)), -INF)
        xb = _xbuf(x32, wdtype, x_f32)
        logits = tv._logit_buffer(M, V, torch.float32)
        got = _score(M, K, V, xb, tv._table(w.cuda()), logits)
        assert (logits[:M, :V] == -INF).all()
        assert got["token"].tolist() == [0] * M and (got["top"] == -INF).all() and (got["lse"] == -INF).all()
        assert torch.isnan(got["logp"]).all()            # (-inf - -inf)


# ---- 7. independence and replay -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_ids([SHAPES[1], SHAPES[3]]))
def test_a_row_does_not_depend_on_its_batch_and_a_call_repeats_its_bits(wdtype, shape):
    M, K, V = shape
    for x_f32 in (True, False):
        xbuf, wbuf, _, _ = _case(shape, wdtype, x_f32)
        tg = [(11 * m + 2) % V for m in range(M)]
        whole = _score(M, K, V, xbuf, wbuf, None, targets=tg)
        assert _same(whole, _score(M, K, V, xbuf, wbuf, None, targets=tg))
        for m in range(M):
            one = _score(1, K, V, xbuf[m:m + 1], wbuf, None, targets=[tg[m]])
            for k in KEYS:
                assert _bits(one[k], whole[k][m:m + 1]), (shape, wdtype, x_f32, m, k)
        h = M // 2
        for a, b in ((0, h), (h, M)):
            half = _score(b - a, K, V, xbuf[a:b], wbuf, None, targets=tg[a:b])
            for k in KEYS:
                assert _bits(half[k], whole[k][a:b]), (shape, wdtype, x_f32, a, b, k)
        back = _score(M, K, V, xbuf[:M].flip(0).contiguous(), wbuf, None, targets=tg[::-1])
        for k in KEYS:
            assert _bits(back[k].flip(0), whole[k]), (shape, wdtype, x_f32, "reversed", k)


# ---- 8. agreement with the few-row entry ----------------------------------------------------------------------------------------
def _agree(mine, few, few_logits, bound, what):
    """token wherever the few-row entry's top-two margin exceeds 2 bound[m]; lse within the two tolerances summed."""
    L = few_logits.cpu()
    top2 = torch.topk(L, 2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]).double() > 2.0 * bound
    assert int(decided.sum()) >= L.shape[0] // 2, (what, int(decided.sum()))
    assert torch.equal(mine["token"].cpu()[decided], few["token"].cpu()[decided]), what
    Ln = L.numpy()
    a, b = mine["lse"].cpu().numpy(), few["lse"].cpu().numpy()
    for m in range(L.shape[0]):
        lse64 = lref.lse(Ln[m])
        allowed = ref.tol(Ln[m], lse64) + lref.tol(Ln[m], lse64)
        assert abs(float(a[m]) - float(b[m])) <= allowed, (what, m, float(a[m]), float(b[m]), allowed)


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_agreement_with_the_few_row_entry_on_64_rows(wdtype):
    shape = SHAPES[2]
    M, K, V = 64, shape[1], shape[2]
    _, bound = _host(shape, wdtype)
    for x_f32 in (True, False):
        xbuf, wbuf, _, _ = _case(shape, wdtype, x_f32)
        few_logits = tv._logit_buffer(M, V, torch.float32)
        few = tl._logprob(M, K, V, xbuf[:M + 1], wbuf, few_logits)
        mine = _score(M, K, V, xbuf[:M + 1], wbuf, None)
        _agree(mine, few, few_logits[:M, :V], bound[:M], (wdtype, x_f32))


# ---- 9. the stack ---------------------------------------------------------------------------------------------------------------
SB, ST = 2, 66                                           # (ST - 1) SB = 130 rows


@functools.lru_cache(maxsize=None)
def _stack_tokens():
    g = torch.Generator().manual_seed(30)
    tokens = torch.randint(2, tv.VOCAB, (SB, ST), generator=g)
    tokens[1, 20] = tokens[0, 41] = 1                    # pad_idx as a target (and as an input)
    return tokens.cuda()


def _full_rows(m, tokens, dtype):
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return m(tokens[:, :-1])


@pytest.mark.gpu
def test_rows_logprobs_against_token_logprobs_on_130_rows():
    dtype = torch.bfloat16
    m = tv._stack()
    tokens = _stack_tokens()
    rows = _full_rows(m, tokens, dtype)
    assert tuple(rows.shape) == (ST - 1, SB, tv.C) and rows.shape[0] * rows.shape[1] == 130
    st = m.init_logprobs(m.init_decoding(SB, 8, dtype, "cuda", hold_weights=False, hold_vocab=True))
    targets = tokens[:, 1:].t().contiguous()
    few_tok, few_logp, few_lse = m.token_logprobs(rows, st, targets=targets, return_lse=True)
    _, few_logits = m.next_tokens(rows, st, return_logits=True)
    tok, logp, lse = m.rows_logprobs(rows, st.vocab, targets, return_lse=True)
    tok2, logp2 = m.rows_logprobs(rows, st.vocab, targets)
    torch.cuda.synchronize()
    assert all(tuple(t.shape) == (ST - 1, SB) for t in (tok, logp, lse)) and tok.dtype == torch.long
    assert logp.dtype == lse.dtype == torch.float32 and torch.equal(tok, tok2) and _bits(logp, logp2)
    xh = rows.reshape(130, tv.C).to(dtype).cpu()
    bound = ops.bound(xh, st.vocab.cpu())
    _agree(dict(token=tok.reshape(-1), lse=lse.reshape(-1)), dict(token=few_tok.reshape(-1), lse=few_lse.reshape(-1)),
           few_logits.reshape(130, tv.VOCAB).float(), bound, "stack")
    # without targets: the pick's own log-probability
    _, top_logp = m.rows_logprobs(rows, st.vocab)
    assert (top_logp <= 0).all() and (top_logp >= logp).all()


_BANNED = ((F, "linear"), (torch, "matmul"), (torch, "log_softmax"), (F, "log_softmax"), (torch.Tensor, "log_softmax"),
           (torch, "logsumexp"), (torch.Tensor, "logsumexp"), (F, "cross_entropy"), (torch, "argmax"), (torch.Tensor, "argmax"))


@pytest.mark.gpu
def test_evaluate_is_rows_logprobs_on_the_full_path_and_runs_under_the_ban(monkeypatch):
    dtype = torch.bfloat16
    m = tv._stack()
    tokens = _stack_tokens()
    rows = _full_rows(m, tokens, dtype)
    targets = tokens[:, 1:].t().contiguous()
    pad = tokens[:, 1:].eq(m.pad_idx)
    assert int(pad.sum()) == 2
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = m.init_decoding(SB, 8, dtype, "cuda", hold_weights=False, hold_vocab=True)
        got = m.evaluate(tokens)                                            # a 16-bit copy of the table made for the call
        held, greedy = m.evaluate(tokens, table=st.vocab, return_tokens=True)
        want_tok, want = m.rows_logprobs(rows, st.vocab, targets)
        torch.cuda.synchronize()
    assert tuple(got.shape) == (SB, ST - 1) and got.dtype == torch.float32 and greedy.dtype == torch.long
    assert _bits(got, held) and (got[pad] == 0).all() and torch.equal(greedy, want_tok.t())
    assert _bits(got[~pad], want.t()[~pad]) and (got[~pad] < 0).all()
    # from the rows on: the full path stands in as a function that returns its rows, everything banned raises
    calls = []

    def forward(tok, mask=None):
        calls.append(tuple(tok.shape))
        return rows
    monkeypatch.setattr(m, "forward", forward)
    for mod, name in _BANNED:
        def banned(*a, _name=name, **k):
            raise AssertionError("%s reached in evaluate behind the full path" % _name)
        monkeypatch.setattr(mod, name, banned)
    with _ctx(dtype):
        again = m.evaluate(tokens, table=st.vocab)
        torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls == [(SB, ST - 1)] and _bits(again, got)
    with pytest.raises(NotImplementedError):
        m.train()
        try:
            m.evaluate(tokens)
        finally:
            m.eval()
    # fp64 on the host from the rows and the held table
    xh = rows.reshape((ST - 1) * SB, tv.C).to(dtype).cpu()
    table = st.vocab.cpu()
    L = (xh.double() @ table.double().t()).numpy()
    bound = ops.bound(xh, table).numpy()
    flat, tg = want.reshape(-1).cpu().numpy(), targets.reshape(-1).cpu().numpy()
    worst = 0.0
    for i in range(L.shape[0]):
        lse64 = lref.lse(L[i])
        allowed = ref.tol(L[i], lse64) + 2.0 * bound[i]
        err = abs(float(flat[i]) - (L[i, tg[i]] - lse64))
        worst = max(worst, err / allowed)
        assert err <= allowed, (i, float(flat[i]), L[i, tg[i]] - lse64, err, allowed)
    print("largest |evaluate - fp64 log-softmax| / (tol + 2 bound): %.4f" % worst)
