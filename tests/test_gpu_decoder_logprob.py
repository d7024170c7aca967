"""-m gpu: token log-probabilities on a held vocabulary table (csrc/ea_ceva_decode_vocab.hip, ea_ceva_sdecode_vocab_logprob and
ea_ceva_sdecode_vocab_sample_logprob, C ABI 28) and DecoderStack.init_logprobs / token_logprobs / sample_tokens_logprobs / score /
generate(return_logprobs=True).

Kernel, at the six small shapes of decoder_vocab_operands.SHAPES and (1, 1024, 32768) once (2048 tiles: the strided loop of the
second launch), bf16 and fp16 tables, x in fp32 and in the table's type, in the framed buffers of tests/test_gpu_decoder_vocab.py:

 1. token, top and the logits are ea_ceva_sdecode_vocab_argmax's bits, frames intact; lse, logp and token do not depend on
    whether logits are stored.
 2. |lse - lse64| <= tol[m] = (2 D_m + 40 + NB / 512) 2^-24 + 2^-22 max(1, |lse64|), lse64 the fp64 log-sum-exp of the kernel's
    own stored fp32 logits (tests/decoder_logprob_reference.py, where the terms are accounted for), D_m the spread of the
    row's finite logits.  The largest |lse - lse64| / tol is printed.
 3. logp has the bits of fp32(top - lse) without targets and of fp32(logit[m, target] - lse) with them: column 0, column V - 1,
    the pick itself, a different column per row; targets -1 and V give NaN; nothing outside [M] is written.
 4. range: a positive x against a one-signed table scaled so that every logit lies near -300, and near +300, under 2's bound.
 5. special values: a NaN table row; a +inf logit; one -inf logit under a finite top; a whole tile of -inf logits under a
    finite, negative top; every logit -inf.
 6. a batch equals single-row calls, bit for bit, across the row-tile variants of the kernel; a call repeated repeats its bits;
    130 rows through token_logprobs equal 130 single-row calls.
 7. sampled: tokens, ctr, sel_idx, sel_val and kept are ea_ceva_sdecode_vocab_sample's at the same (seed, ctr, sid); lse has
    the greedy entry's bits; logp those of fp32(logits[m, token] - lse).
 8. the stack (the geometry of tests/test_gpu_decoder_vocab.py; rolling, static, ragged per-sequence; greedy and sampled):
    generate(return_logprobs=True) replayed == eager in tokens, rows and log-probabilities; its tokens are generate's without
    the keyword; each log-probability is token_logprobs(row, targets=token); the run from the first pick on passes with the
    framework's GEMMs, argmax, logsumexp, log_softmax, cross_entropy, topk, softmax and multinomial replaced by functions
    that raise; score == token_logprobs on decode's rows and lies within tol + 2 bound of fp64 log-softmax values; the bytes
    of the scorer; a state without one is what it was."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_decoder_vocab as tv                    # the framed buffers, the shared operands, the stack
import test_gpu_decoder_sample as ts                   # the sampled entry's caller, the sampled states
import decoder_logprob_reference as ref
import decoder_vocab_operands as ops
from ceva_decoding import _ctx

LOGPROB_FN, SAMPLE_LOGPROB_FN = "ea_ceva_sdecode_vocab_logprob", "ea_ceva_sdecode_vocab_sample_logprob"
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
SHAPES = ops.SHAPES[:6]
LM = ops.SHAPES[6]
_ids = tv._ids
_bits = tv._bits
INF, NAN = float("inf"), float("nan")


def _workspaces(M, V):
    from efficient_attention import _native as nv
    nbytes, lbytes = nv.lib().ea_ceva_sdecode_vocab_ws(M, V), nv.lib().ea_ceva_sdecode_vocab_lse_ws(M, V)
    assert nbytes == 8 * M * ((V + 15) // 16) and lbytes == 4 * M * ((V + 15) // 16) + 4 * M
    # (stale candidates and sums would be NaNs)
    return (torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda"), nbytes,
            torch.full((lbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda"), lbytes)


def _logprob(M, K, V, xbuf, wbuf, logits=None, targets=None, top=True):
    """-> dict(token [M] int64, top [M] or None, lse [M], logp [M]); every output has a guard element that must stay."""
    from efficient_attention import _native as nv
    ws, nbytes, lws, lbytes = _workspaces(M, V)
    token = torch.full((M + 1,), -7, dtype=torch.long, device="cuda")
    t = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda") if top else None
    lse = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    logp = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    if targets is not None:
        targets = torch.as_tensor(targets, dtype=torch.long).cuda()
        assert tuple(targets.shape) == (M,)
    nv.call(LOGPROB_FN, M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf), nv.ptr(logits),
            0 if logits is None else tv._code(logits), 0 if logits is None else logits.stride(0), nv.ptr(ws), nbytes,
            nv.ptr(token), nv.ptr(t), nv.ptr(lws), lbytes, nv.ptr(targets), nv.ptr(lse), nv.ptr(logp), nv.stream())
    torch.cuda.synchronize()
    assert token[M].item() == -7 and (t is None or t[M].item() == 7.0) and lse[M].item() == 7.0 and logp[M].item() == 7.0
    assert (lws[lbytes:] == 0xFF).all()                                  # the workspace ends where the query says
    if logits is not None:
        assert (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()
    return dict(token=token[:M], top=None if t is None else t[:M], lse=lse[:M], logp=logp[:M])


def _same(a, b, keys=("token", "lse", "logp")):
    return all(_bits(a[k], b[k]) for k in keys)


def _xbuf(x32, wdtype, x_f32):
    M, K = x32.shape
    return tv._rows(M, K, K + 8, torch.float32 if x_f32 else wdtype, x32.cuda() if x_f32 else x32.to(wdtype).cuda())


def _check_lse(got, logits, M, V, what):
    """2: the kernel's lse against the fp64 log-sum-exp of its own stored logits -> the largest |lse - lse64| / tol."""
    L = logits[:M, :V].cpu().numpy()
    lse = got["lse"].cpu().numpy()
    worst = 0.0
    for m in range(M):
        want = ref.lse(L[m])
        assert np.isfinite(want), (what, m)
        tol = ref.tol(L[m], want)
        err = abs(float(lse[m]) - want)
        if err > tol:
            print(what, "row", m, "lse %.9g lse64 %.12g |diff| %.3e tol %.3e ratio %.4f" % (lse[m], want, err, tol, err / tol))
        assert err <= tol, (what, m, float(lse[m]), want, err, tol)
        worst = max(worst, err / tol)
    return worst


# ---- 1, 2, 3 on the plain operands --------------------------------------------------------------------------------------------------
def _plain(shape, wdtype, x_f32s=(True, False)):
    M, K, V = shape
    worst = 0.0
    for x_f32 in x_f32s:
        xbuf, wbuf, ref32, ref16 = tv._case(shape, wdtype, x_f32)
        want_tok, want_top = tv._pick(M, K, V, xbuf, wbuf, None)
        logits = tv._logit_buffer(M, V, torch.float32)
        got = _logprob(M, K, V, xbuf, wbuf, logits)
        # 1
        assert torch.equal(got["token"], want_tok) and _bits(got["top"], want_top), (shape, wdtype, x_f32)
        assert _bits(logits[:M, :V], ref32), (shape, wdtype, x_f32)
        l16 = tv._logit_buffer(M, V, wdtype)
        got16 = _logprob(M, K, V, xbuf, wbuf, l16)
        assert _bits(l16[:M, :V], ref16) and _same(got, got16, ("token", "top", "lse", "logp"))
        none = _logprob(M, K, V, xbuf, wbuf, None)
        assert _same(got, none, ("token", "top", "lse", "logp"))
        assert _same(got, _logprob(M, K, V, xbuf, wbuf, None, top=False))
        # 2
        worst = max(worst, _check_lse(got, logits, M, V, (shape, wdtype, x_f32)))
        # 3
        assert _bits(got["logp"], got["top"] - got["lse"])
        L = logits[:M, :V]
        rows = torch.arange(M, device="cuda")
        for name, tg in (("first", [0] * M), ("last", [V - 1] * M), ("pick", got["token"].tolist()),
                         ("per_row", [(7 * m + 3) % V for m in range(M)]), ("mixed", [(m * 5) % V if m % 2 else V - 1 - m % V
                                                                                     for m in range(M)])):
            for lg in (None, tv._logit_buffer(M, V, torch.float32)):
                t = _logprob(M, K, V, xbuf, wbuf, lg, targets=tg)
                assert _same(t, got, ("token", "top", "lse")), (shape, wdtype, x_f32, name)
                want = L[rows, torch.tensor(tg, device="cuda")] - got["lse"]
                assert _bits(t["logp"], want), (shape, wdtype, x_f32, name)
            if name == "pick":
                assert _bits(t["logp"], got["logp"])
        for tg in ([-1] * M, [V] * M, [V + 16] * M, [-(1 << 40)] * M, [1 << 40] * M):
            t = _logprob(M, K, V, xbuf, wbuf, None, targets=tg)
            assert torch.isnan(t["logp"]).all() and _same(t, got, ("token", "top", "lse")), (shape, tg[0])
        if M > 1:                                       # one bad target among good ones
            tg = [0] * M
            tg[M // 2] = V
            t = _logprob(M, K, V, xbuf, wbuf, None, targets=tg)
            keep = torch.ones(M, dtype=torch.bool, device="cuda")
            keep[M // 2] = False
            assert math.isnan(t["logp"][M // 2].item()) and _bits(t["logp"][keep], (L[:, 0] - got["lse"])[keep])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_pick_logits_lse_and_target_logits(wdtype, shape):
    worst = _plain(shape, wdtype)
    print(shape, wdtype, "largest |lse - lse64| / tol: %.4f" % worst)


@pytest.mark.gpu
def test_the_lm_shape_strides_over_2048_tiles():
    assert (LM[2] + 15) // 16 == 2048
    worst = _plain(LM, torch.bfloat16, x_f32s=(True,))
    print(LM, "largest |lse - lse64| / tol: %.4f" % worst)


# ---- 4. range -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_signed(shape, wdtype, sign, level=300.0):
    """x > 0 against a table of one sign, scaled so that the logits' mean is sign * level -> x32, w (CPU)."""
    x32, w = ops.operands(shape, wdtype, 0)
    x32 = x32.abs() + 0.25
    wa = w.double().abs()
    mean = (x32.to(wdtype).double() @ wa.t()).mean().item()
    return x32, (sign * level / mean * wa).to(wdtype)


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("sign", [-1.0, 1.0], ids=["near_minus_300", "near_plus_300"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_logits_near_minus_and_plus_300(shape, sign, wdtype):
    M, K, V = shape
    x32, w = _one_signed(shape, wdtype, sign)
    wbuf = tv._table(w.cuda())
    for x_f32 in (True, False):
        xbuf = _xbuf(x32, wdtype, x_f32)
        logits = tv._logit_buffer(M, V, torch.float32)
        got = _logprob(M, K, V, xbuf, wbuf, logits)
        L = logits[:M, :V]
        assert torch.isfinite(L).all() and (L * sign > 100.0).all() and (L * sign).mean().item() > 250.0
        worst = _check_lse(got, logits, M, V, (shape, wdtype, sign, x_f32))
        print(shape, wdtype, sign, "largest |lse - lse64| / tol: %.4f" % worst)
        assert _bits(got["logp"], got["top"] - got["lse"]) and _same(got, _logprob(M, K, V, xbuf, wbuf, None))


# ---- 5. special values --------------------------------------------------------------------------------------------------------------
def _edited(shape, wdtype, rows, value, negative=False):
    """The plain operands (negative: the one-signed, negative table) with table rows `rows` = (value, 0, 0, ..): x[:, 0] > 0
    makes the logit `value` in every row of x."""
    x32, w = _one_signed(shape, wdtype, -1.0, 30.0) if negative else ops.operands(shape, wdtype, 0)
    w = w.clone()
    w[rows] = 0.0
    w[rows, 0] = value
    return x32, w


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_special_values(wdtype, shape):
    M, K, V = shape
    NB = (V + 15) // 16
    for x_f32 in (True, False):
        # a NaN table row
        _, w, rows = ops.nan_rows(shape, wdtype, 0, False)
        xbuf = tv._case(shape, wdtype, x_f32)[0]
        for lg in (None, tv._logit_buffer(M, V, torch.float32)):
            got = _logprob(M, K, V, xbuf, tv._table(w.cuda()), lg)
            assert got["token"].tolist() == [rows[0]] * M and torch.isnan(got["top"]).all()
            assert torch.isnan(got["lse"]).all() and torch.isnan(got["logp"]).all()
        # a +inf logit
        v = V // 2
        x32, w = _edited(shape, wdtype, [v], INF)
        xb = _xbuf(x32, wdtype, x_f32)
        got = _logprob(M, K, V, xb, tv._table(w.cuda()), None, targets=[0] * M)
        assert got["token"].tolist() == [v] * M and (got["top"] == INF).all() and (got["lse"] == INF).all()
        assert (got["logp"] == -INF).all()               # (a finite logit under an infinite normaliser)
        # one -inf logit under a finite top
        v = V - 1
        x32, w = _edited(shape, wdtype, [v], -INF)
        xb = _xbuf(x32, wdtype, x_f32)
        logits = tv._logit_buffer(M, V, torch.float32)
        got = _logprob(M, K, V, xb, tv._table(w.cuda()), logits, targets=[v] * M)
        assert (logits[:M, v] == -INF).all() and int(torch.isinf(logits[:M, :V]).sum()) == M
        _check_lse(got, logits, M, V, (shape, wdtype, x_f32, "one -inf"))
        assert (got["logp"] == -INF).all() and torch.isfinite(got["top"]).all() and (got["token"] != v).all()
        assert _same(got, _logprob(M, K, V, xb, tv._table(w.cuda()), None, targets=[v] * M))
        # a whole tile of -inf logits under a finite, negative top (a table of at least two tiles)
        if NB >= 2:
            tile = NB // 2
            cols = list(range(16 * tile, min(V, 16 * tile + 16)))
            x32, w = _edited(shape, wdtype, cols, -INF, negative=True)
            xb = _xbuf(x32, wdtype, x_f32)
            logits = tv._logit_buffer(M, V, torch.float32)
            got = _logprob(M, K, V, xb, tv._table(w.cuda()), logits)
            assert (logits[:M, cols] == -INF).all() and (got["top"] < 0).all() and torch.isfinite(got["top"]).all()
            assert torch.isfinite(got["lse"]).all()
            worst = _check_lse(got, logits, M, V, (shape, wdtype, x_f32, "a tile of -inf"))
            print(shape, wdtype, x_f32, "a tile of -inf: largest |lse - lse64| / tol: %.4f" % worst)
            assert _same(got, _logprob(M, K, V, xb, tv._table(w.cuda()), None))
        # every logit -inf
        x32, w = _edited(shape, wdtype, list(range(V)), -INF)
        xb = _xbuf(x32, wdtype, x_f32)
        logits = tv._logit_buffer(M, V, torch.float32)
        got = _logprob(M, K, V, xb, tv._table(w.cuda()), logits)
        assert (logits[:M, :V] == -INF).all()
        assert got["token"].tolist() == [0] * M and (got["top"] == -INF).all() and (got["lse"] == -INF).all()
        assert torch.isnan(got["logp"]).all()            # (-inf - -inf)


# ---- 6. independence and replay -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape,rows", [((3, 288, 40), [0, 1, 2]), ((33, 1056, 48), [0, 16, 32]), ((64, 1024, 1000), [5, 31, 63])],
                         ids=["3x288x40", "33x1056x48", "64x1024x1000"])
def test_a_row_does_not_depend_on_its_batch_and_a_call_repeats_its_bits(wdtype, shape, rows):
    M, K, V = shape
    for x_f32 in (True, False):
        xbuf, wbuf, _, _ = tv._case(shape, wdtype, x_f32)
        tg = [(11 * m + 2) % V for m in range(M)]
        whole = _logprob(M, K, V, xbuf, wbuf, None, targets=tg)
        assert _same(whole, _logprob(M, K, V, xbuf, wbuf, None, targets=tg), ("token", "top", "lse", "logp"))
        three = _logprob(3, K, V, xbuf[rows].contiguous(), wbuf, None, targets=[tg[m] for m in rows])
        for i, m in enumerate(rows):
            one = _logprob(1, K, V, xbuf[m:m + 1], wbuf, None, targets=[tg[m]])
            for k in ("token", "top", "lse", "logp"):
                assert _bits(one[k], whole[k][m:m + 1]) and _bits(one[k], three[k][i:i + 1]), (shape, wdtype, x_f32, m, k)


@pytest.mark.gpu
def test_token_logprobs_on_130_rows_equals_row_wise_calls():
    dtype = torch.float16
    m = tv._stack()
    st = m.init_logprobs(m.init_decoding(2, 8, dtype, "cuda", hold_weights=False, hold_vocab=True))
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(65, 2, tv.C, generator=g).cuda()
    targets = torch.randint(0, tv.VOCAB, (65, 2), generator=g).cuda()
    for r in (rows, rows.to(dtype)):
        tok, logp, lse = m.token_logprobs(r, st, return_lse=True)
        assert all(tuple(t.shape) == (65, 2) for t in (tok, logp, lse)) and tok.dtype == torch.long
        assert logp.dtype == lse.dtype == torch.float32
        want_tok, logits = m.next_tokens(r, st, return_logits=True)
        assert torch.equal(tok, want_tok)
        out = torch.full((65, 2), -1, dtype=torch.long, device="cuda")
        tok_t, logp_t = m.token_logprobs(r, st, targets=targets, out=out)
        assert tok_t is out and torch.equal(out, tok)
        assert _bits(logp_t, logits.gather(2, targets.unsqueeze(2)).squeeze(2) - lse)
        assert _bits(logp, logits.gather(2, tok.unsqueeze(2)).squeeze(2) - lse)
        L = logits.cpu().numpy()
        for t in range(0, 65, 16):
            for b in range(2):
                want = ref.lse(L[t, b])
                assert abs(lse[t, b].item() - want) <= ref.tol(L[t, b], want)
        for t in range(65):
            for b in range(2):
                one = m.token_logprobs(r[t:t + 1, b:b + 1], st, targets=targets[t:t + 1, b:b + 1], return_lse=True)
                assert one[0].item() == tok[t, b].item() and _bits(one[1][0, 0], logp_t[t, b]) and _bits(one[2][0, 0], lse[t, b])
    with pytest.raises(ValueError, match="contiguous int64"):
        m.token_logprobs(rows, st, out=torch.zeros(65, 2, dtype=torch.int32, device="cuda"))


# ---- 7. sampled ---------------------------------------------------------------------------------------------------------------------
def _sample_logprob(M, K, V, xbuf, wbuf, k, top_p, temperature, ctr, sid):
    from efficient_attention import _native as nv
    ws, nbytes, lws, lbytes = _workspaces(M, V)
    logits = tv._logit_buffer(M, V, torch.float32)
    cbuf = torch.cat([ctr, torch.full((1,), -7, dtype=torch.long, device="cuda")])
    token = torch.full((M + 1,), -7, dtype=torch.long, device="cuda")
    kept = torch.full((M + 1,), -7, dtype=torch.int32, device="cuda")
    sel_idx = torch.full((M + 1, k), -7, dtype=torch.int32, device="cuda")
    sel_val = torch.full((M + 1, k), 7.0, dtype=torch.float32, device="cuda")
    lse = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    logp = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    nv.call(SAMPLE_LOGPROB_FN, M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf),
            nv.ptr(logits), logits.stride(0), nv.ptr(ws), nbytes, k, top_p, temperature, ts.SEED, nv.ptr(cbuf), nv.ptr(sid),
            nv.ptr(token), nv.ptr(sel_idx), nv.ptr(sel_val), nv.ptr(kept), nv.ptr(lws), lbytes, nv.ptr(lse), nv.ptr(logp),
            nv.stream())
    torch.cuda.synchronize()
    assert token[M].item() == -7 and kept[M].item() == -7 and cbuf[M].item() == -7 and lse[M].item() == 7.0
    assert logp[M].item() == 7.0 and (sel_idx[M] == -7).all() and (sel_val[M] == 7.0).all()
    assert (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all() and (lws[lbytes:] == 0xFF).all()
    kk = min(k, V)
    return dict(token=token[:M], kept=kept[:M], sel_idx=sel_idx[:M, :kk], sel_val=sel_val[:M, :kk], logits=logits,
                ctr=cbuf[:M], lse=lse[:M], logp=logp[:M])


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_the_sampled_entry_draws_what_the_sampler_draws_and_scores_it(wdtype, shape):
    M, K, V = shape
    rows = torch.arange(M, device="cuda")
    for x_f32, k, top_p, temp, c0 in ((True, 8, 0.9, 0.8, 0), (False, 40, 1.0, 1.0, 5), (True, 1, 0.9, 0.7, (1 << 33) + 1)):
        xbuf, wbuf, ref32, _ = tv._case(shape, wdtype, x_f32)
        sid = (torch.arange(M, dtype=torch.int32) * 3 + 1).cuda()
        ctr = torch.arange(c0, c0 + M, dtype=torch.long).cuda()
        want = ts._sample(M, K, V, xbuf, wbuf, k, top_p, temp, ts.SEED, ctr.clone(), sid)
        got = _sample_logprob(M, K, V, xbuf, wbuf, k, top_p, temp, ctr.clone(), sid)
        assert torch.equal(got["token"], want["token"][0]) and torch.equal(got["kept"], want["kept"][0])
        assert torch.equal(got["ctr"], want["ctr"]) and torch.equal(got["ctr"], ctr + 1)
        assert torch.equal(got["sel_idx"], want["sel_idx"]) and _bits(got["sel_val"], want["sel_val"])
        assert _bits(got["logits"][:M, :V], ref32)
        greedy = _logprob(M, K, V, xbuf, wbuf, None)
        assert _bits(got["lse"], greedy["lse"])
        assert _bits(got["logp"], got["logits"][rows, got["token"]] - got["lse"])
        if k == 1:
            assert torch.equal(got["token"], greedy["token"]) and _bits(got["logp"], greedy["logp"])


# ---- 8. the stack -------------------------------------------------------------------------------------------------------------------
B, T, P0, C, VOCAB = tv.B, tv.T, tv.P0, tv.C, tv.VOCAB
SCORER_BYTES = 4 * 64 * ((VOCAB + 15) // 16) + 4 * 64 + 8 * B
_BANNED = ((F, "linear"), (torch, "addmm"), (torch, "matmul"), (torch, "argmax"), (torch.Tensor, "argmax"),
           (torch, "logsumexp"), (torch, "log_softmax"), (F, "log_softmax"), (F, "cross_entropy"), (torch, "topk"),
           (torch, "softmax"), (torch, "multinomial"))


def _state(m, case, sampled, scorer=True):
    st = ts._state(m, case, sampler=sampled)
    return m.init_logprobs(st) if scorer else st


@pytest.mark.gpu
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("case", ["rolling", "static", "per_sequence_ragged"])
def test_generate_with_logprobs_replayed_equals_eager_and_scores_its_tokens(case, sampled):
    dtype = torch.bfloat16
    m = tv._stack()
    prompt = ts._prompt(m, case)
    n_new = T - P0
    out = {}
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for graph in (False, True):
            st = _state(m, case, sampled)
            out[graph] = m.generate(prompt, n_new, st, graph=graph, return_rows=True, return_logprobs=True)
            if sampled:                                  # (the warm-up's draw is undone)
                assert st.sampler.ctr.tolist() == [n_new] * B
        plain = m.generate(prompt, n_new, _state(m, case, sampled, scorer=False), graph=True)
        pair = m.generate(prompt, n_new, _state(m, case, sampled), graph=True, return_logprobs=True)
        (tok_e, rows_e, lp_e), (tok_g, rows_g, lp_g) = out[False], out[True]
        probe = _state(m, case, False)
        _, want, lse = m.token_logprobs(rows_g, probe, targets=tok_g.t().contiguous(), return_lse=True)
        greedy_tok, _ = m.token_logprobs(rows_g, probe)
        torch.cuda.synchronize()
    assert tuple(lp_g.shape) == (B, n_new) and lp_g.dtype == torch.float32 and tuple(rows_g.shape) == (n_new, B, C)
    assert torch.equal(tok_g, tok_e) and _bits(rows_g, rows_e) and _bits(lp_g, lp_e)
    assert torch.equal(tok_g, plain) and len(pair) == 2 and torch.equal(pair[0], tok_g) and _bits(pair[1], lp_g)
    assert _bits(lp_g, want.t().contiguous())
    assert torch.isfinite(lp_g).all() and (lp_g <= 0).all() and (lp_g[:, 1:] != lp_g[:, :-1]).any()
    if sampled:
        assert not torch.equal(greedy_tok.t(), tok_g)
    else:
        assert torch.equal(greedy_tok.t(), tok_g)
    print(case, "sampled" if sampled else "greedy", "logp", lp_g[0, :6].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_generate_with_logprobs_runs_under_the_ban(kind, sampled, monkeypatch):
    """generate(graph=True, return_logprobs=True), its own code: from the return of the prefill's `decode` on -- the first
    pick, the scratch state, the warm-up, the capture and every replay -- the banned functions raise."""
    dtype = torch.bfloat16
    m = tv._stack()
    prompt = ts._prompt(m, kind)
    n_new = 8
    armed, decodes = [], []
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = m.generate(prompt, n_new, _state(m, kind, sampled), graph=True, return_logprobs=True)
        st = _state(m, kind, sampled)

        def gated(name, real):
            def f(*a, **k):
                if armed:
                    raise AssertionError("%s reached in generate behind the prefill" % name)
                return real(*a, **k)
            return f
        for mod, name in _BANNED:
            monkeypatch.setattr(mod, name, gated(name, getattr(mod, name)))
        real_decode = m.decode

        def arming(*a, **k):
            y = real_decode(*a, **k)
            decodes.append(True)
            armed.append(True)
            return y
        monkeypatch.setattr(m, "decode", arming)
        try:
            got = m.generate(prompt, n_new, st, graph=True, return_logprobs=True)
            torch.cuda.synchronize()
        finally:
            del armed[:]
    assert len(decodes) == 3                             # the prefill, the warm-up, the capture
    assert torch.equal(got[0], want[0]) and _bits(got[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_score_is_token_logprobs_on_decodes_rows_and_agrees_with_fp64(kind):
    dtype = torch.bfloat16
    m = tv._stack()
    tokens = tv._tokens().clone()
    tokens[1, 20] = m.pad_idx
    opt = dict(rolling=kind == "rolling", hold_vocab=True)
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = m.init_logprobs(m.init_decoding(B, T, dtype, "cuda", **opt))
        got = m.score(tokens, st)
        st2 = m.init_logprobs(m.init_decoding(B, T, dtype, "cuda", **opt))
        with torch.no_grad():
            rows = m.decode(tokens[:, :-1].t(), st2)
        targets = tokens[:, 1:].t().contiguous()
        _, want = m.token_logprobs(rows, st2, targets=targets)
        torch.cuda.synchronize()
    assert tuple(got.shape) == (B, T - 1) and got.dtype == torch.float32
    pad = targets.t().eq(m.pad_idx)
    assert int(pad.sum()) == 1 and (got[pad] == 0).all()
    assert _bits(got[~pad], want.t()[~pad])
    # fp64 on the host from the rows and the held table
    xh = rows.reshape((T - 1) * B, C).to(dtype).cpu()
    table = st2.vocab.cpu()
    L = (xh.double() @ table.double().t()).numpy()
    bound = ops.bound(xh, table).numpy()
    flat, tg = want.reshape(-1).cpu().numpy(), targets.reshape(-1).cpu().numpy()
    worst = 0.0
    for i in range(L.shape[0]):
        lse64 = ref.lse(L[i])
        allowed = ref.tol(L[i], lse64) + 2.0 * bound[i]
        err = abs(float(flat[i]) - (L[i, tg[i]] - lse64))
        worst = max(worst, err / allowed)
        assert err <= allowed, (i, float(flat[i]), L[i, tg[i]] - lse64, err, allowed)
    print(kind, "largest |score - fp64 log-softmax| / (tol + 2 bound): %.4f" % worst)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rolling", "static"])
def test_the_scorer_adds_its_bytes_and_a_state_without_one_is_what_it_was(kind):
    m = tv._stack()
    dtype = torch.float16
    opt = dict(rolling=kind == "rolling", per_sequence=True, landmark_splits=3, hold_vocab=True)
    without = m.init_decoding(B, 500, dtype, "cuda", **opt)
    scored = m.init_logprobs(m.init_decoding(B, 500, dtype, "cuda", **opt))
    assert without.scorer is None and sorted(vars(without)) == ["ffn", "incremental", "options", "vocab", "vocab_ws"]
    assert sorted(vars(scored)) == ["ffn", "incremental", "options", "scorer", "vocab", "vocab_ws"]
    assert m.decoding_state_nbytes(scored) - m.decoding_state_nbytes(without) == SCORER_BYTES
    sc = scored.scorer
    assert sc.ws.numel() == SCORER_BYTES - 8 * B and sc.ws.data_ptr() % 16 == 0 and sc.ws.is_cuda
    assert tuple(sc.lse.shape) == tuple(sc.logp.shape) == (B,) and sc.lse.dtype == sc.logp.dtype == torch.float32
    with pytest.raises(RuntimeError, match="init_logprobs"):
        m.token_logprobs(torch.zeros(1, B, C, device="cuda"), without)
    with pytest.raises(RuntimeError, match="hold_vocab=True"):
        m.init_logprobs(m.init_decoding(B, 500, dtype, "cuda", rolling=kind == "rolling"))
    # a beam reorder, a row reset and a refresh have nothing of it to move
    ptrs = (sc.ws.data_ptr(), sc.lse.data_ptr(), sc.logp.data_ptr())
    m.reorder_decoding_state(scored, torch.tensor([2, 0, 0], device="cuda"))
    m.reset_decoding_rows(scored, [1])
    m.refresh_decoding_weights(scored)
    assert scored.scorer is sc and ptrs == (sc.ws.data_ptr(), sc.lse.data_ptr(), sc.logp.data_ptr())
