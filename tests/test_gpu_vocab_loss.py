"""-m gpu: the vocabulary cross-entropy as a training loss (csrc/ea_vocab_nll.hip: ea_vocab_nll_grad, ea_gemm_nt16, C ABI 38;
ea_harness.vocab_loss.vocab_nll; DecoderStack.loss).

With BM the row tile, BN the column block and SL the slice width of the library, at the shapes (M, K, V)
  (1, 32, 16)                                the smallest case
  (BM + 1, 288, 40)                          a ragged K stage, a second row tile holding one row
  (2 BM + 3, 256, BN + 24)                   a second column block that is nearly empty
  (BM, 1056, 2 SL + BN + 8), chunk_cols SL   three chunks, the last ragged, M pad = 0
  (130, 64, SL + 8), chunk_cols SL           a ragged M pad in the dW contraction, a second chunk of 8 columns
  (256, 1024, 32768), once per configuration the LM table
bf16 and fp16 tables, x in fp32 and in the table's type, in the framed buffers of tests/test_gpu_decoder_vocab.py:

 1. ea_vocab_nll_grad: every element of G within vocab_loss_reference.bound of the fp64 formula on the kernel's OWN stored
    fp32 logits and lse (ea_vocab_score with fp32 logits); G^T is G transposed bit for bit; pad columns / rows are zeros in
    buffers that held sevens, frames intact; d == 0 rows exact zeros, also with a NaN row of x and a NaN lse; targets at column
    0, V - 1, the last column of a block, the first column of a chunk, and out of range; a call on M rows == calls on the halves
    and on single rows, bit for bit; a call repeats its bits.  The largest error / bound is printed.
 2. ea_gemm_nt16: store and accumulate within decoder_vocab_operands.bound of the fp64 product (+ 2^-24 |prior|); ragged M, N
    and K = 96; frames intact; accumulate = 0 over NaNs leaves none.
 3. vocab_nll: logp has rows_logprobs' bits; the norm-wise relative errors of d rows and d weight against fp64 autograd of
    log_softmax on the same rounded operands are at most 1.5 times those of the framework route (F.linear on the 16-bit
    operands, .float(), log_softmax, gather) -- the margin is for the chunked accumulation order; both printed.  d weight is
    equal bit for bit between two chunk widths; d rows within the accumulate bound of 2 (16-bit rows: and one rounding each).
 4. memory at (2048, 256, 32768), chunk_cols 2 SL (at the default budget the two G images of 2048 rows are as large as the
    logits: the budget is sized for thousands of rows against a far taller table): the rise of max_memory_allocated over a
    forward + backward is at most ea_vocab_nll_ws + the gradients + the saved tensors + 2 MiB, and that sum is below M V 2 bytes -- arithmetic, before the run.
 5. forward + backward captured in one torch.cuda.graph after a warm-up on a side stream (ea_harness.trainer.capture_step's
    pattern: the gradients keep their storage and are zeroed in place), replayed twice: the eager gradients' bits.
 6. the stack of tests/test_gpu_decoder_vocab.py with dropout 0, bf16: loss(reduction="none") == -evaluate bit for bit; pad
    targets give 0 and add nothing to any gradient; every parameter's gradient finite, the embedding's non-zero at an
    input-only and at a target-only row; every gradient within gpu_checks.MODULE_TOL of the framework-loss route; backward
    runs with F.linear on the table, log_softmax, logsumexp and cross_entropy replaced by functions that raise."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_decoder_vocab as tv                    # the framed buffers, _bits, the stack's geometry
import test_gpu_vocab_score as ts                      # the scorer's caller and its cached cases
import decoder_vocab_operands as ops
import gpu_checks
import vocab_loss_reference as ref
import vocab_score_reference as sref
from ceva_decoding import _ctx
from util import scaled_err

BM, BN, SL = sref.constants()
SMALL = [((1, 32, 16), None), ((BM + 1, 288, 40), None), ((2 * BM + 3, 256, BN + 24), None),
         ((BM, 1056, 2 * SL + BN + 8), SL), ((130, 64, SL + 8), SL)]
LM = ((256, 1024, 32768), None)
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
_bits = tv._bits
_ids = lambda cases: ["%dx%dx%d" % c[0] for c in cases]                              # noqa: E731
U = 2.0 ** -24


def _up64(n):
    return (n + 63) // 64 * 64


def _chunk(M, V, cc):
    from efficient_attention import _native as nv
    return nv.lib().ea_vocab_nll_chunk(M, V) if cc is None else cc


# ---- 1. the logit gradient ------------------------------------------------------------------------------------------------------
def _grad(M, K, V, xbuf, wbuf, targets, lse, d, v0, Vc, extra=0):
    """One ea_vocab_nll_grad call into buffers of sevens -> (G [M, Vc], G^T [Vc, M]); pads and frames checked here."""
    from efficient_attention import _native as nv
    E = wbuf.dtype
    ldg, ldm = _up64(Vc) + extra, _up64(M) + extra
    g = torch.full((M + 1, ldg), 7.0, dtype=E, device="cuda")
    gt = torch.full((Vc + 1, ldm), 7.0, dtype=E, device="cuda")
    nv.call("ea_vocab_nll_grad", M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf),
            nv.ptr(targets), nv.ptr(lse), nv.ptr(d), v0, Vc, nv.ptr(g), ldg, nv.ptr(gt), ldm, nv.stream())
    torch.cuda.synchronize()
    assert (g[M] == 7.0).all() and (gt[Vc] == 7.0).all()                               # the frames
    zero = torch.zeros((), dtype=E, device="cuda")
    assert _bits(g[:M, Vc:], zero.expand(M, ldg - Vc)) and _bits(gt[:Vc, M:], zero.expand(Vc, ldm - M))   # the pads: +0
    return g[:M, :Vc], gt[:Vc, :M]


def _whole(M, K, V, cc, xbuf, wbuf, targets, lse, d, extra=0):
    """G [M, V] from the chunk loop; G^T == G transposed in every chunk."""
    out = []
    for v0 in range(0, V, cc):
        g, gt = _grad(M, K, V, xbuf, wbuf, targets, lse, d, v0, min(cc, V - v0), extra)
        assert _bits(gt, g.t()), (M, K, V, v0)
        out.append(g)
    return torch.cat(out, dim=1)


def _targets(M, V, cc):
    """Target vectors [M] that between them hold: column 0, V - 1, the last column of a block, the first column of a chunk,
    V and -1 (out of range), beside a column per row."""
    special = [0, V - 1, min(BN, V) - 1, cc if cc < V else (V - 1) // BN * BN, V, -1, 1 << 40]
    base = [(7 * m + 3) % V for m in range(M)]
    if M > max(SPECIAL_ROWS):
        for row, s in zip(SPECIAL_ROWS, special):
            base[row] = s
        return [base]
    return [base] + [[s] * M for s in special]


# where a vector of M > 10 rows holds its special targets: none of the rows whose d is zero (2, 7, 12, .. and 4, below)
SPECIAL_ROWS = (1, 3, 5, 6, 8, 9, 10)


def _live_specials(M, d):
    """Every special target meets a live gradient: in its own row of a long vector, in some row of a short one."""
    rows = list(SPECIAL_ROWS) if M > max(SPECIAL_ROWS) else [m for m in range(M) if m % 5 != 2 and m != 4]
    return len(rows) > 0 and bool((d[rows] != 0).all())


def _d(M, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    d = torch.randn(M, generator=g)
    d[2::5] = 0.0
    if M > 4:
        d[4] = -0.0
    return d.cuda()


def _check_g(case, wdtype, x_f32s=(True, False), singles=True):
    (M, K, V), cc = case
    cc = _chunk(M, V, cc)
    worst = 0.0
    for x_f32 in x_f32s:
        what = (case, wdtype, x_f32)
        xbuf, wbuf, logits, got = ts._case((M, K, V), wdtype, x_f32)
        L, lse = logits[:M, :V].cpu().numpy(), got["lse"]
        d = _d(M, 0)
        assert _live_specials(M, d), what
        for n, tg in enumerate(_targets(M, V, cc)):
            t = torch.tensor(tg, dtype=torch.long, device="cuda")
            G = _whole(M, K, V, cc, xbuf, wbuf, t, lse, d, extra=64 if n == 0 else 0)
            want = ref.grad(L, lse.cpu().numpy(), d.cpu().numpy(), tg, V=V)
            allowed = ref.bound(L, lse.cpu().numpy(), d.cpu().numpy(), tg, wdtype, V=V)
            err = np.abs(G.double().cpu().numpy() - want)
            assert np.isfinite(err).all(), what
            zero_rows = (d == 0).cpu().numpy()
            assert zero_rows.any() or M < 3
            assert _bits(G[d == 0], torch.zeros_like(G[d == 0])), what                 # exact zeros, +0
            live = ~zero_rows
            ratio = float((err[live] / allowed[live]).max()) if live.any() else 0.0
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, n, ratio)
            if n:
                continue
            # a call repeats its bits; halves and single rows: the same bits
            assert _bits(G, _whole(M, K, V, cc, xbuf, wbuf, t, lse, d)), what
            h = M // 2
            parts = [(0, h), (h, M)] if h else []
            if singles:
                parts += [(m, m + 1) for m in sorted({0, 1 % M, M // 3, M - 1})]
            for a, b in parts:
                sub = _whole(b - a, K, V, cc, xbuf[a:], wbuf, t[a:b].contiguous(), lse[a:b].contiguous(), d[a:b].contiguous())
                assert _bits(sub, G[a:b]), (what, a, b)
            # a d == 0 row whose x and lse are NaN: exact zeros there, the other rows untouched
            r = 2 if M > 2 else 0
            xn, ln, dn = xbuf.clone(), lse.clone(), d.clone()
            xn[r], ln[r], dn[r] = float("nan"), float("nan"), 0.0
            Gn = _whole(M, K, V, cc, xn, wbuf, t, ln, dn)
            keep = torch.ones(M, dtype=torch.bool, device="cuda")
            keep[r] = False
            assert _bits(Gn[r], torch.zeros_like(Gn[r])) and _bits(Gn[keep], G[keep]), what
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("case", SMALL, ids=_ids(SMALL))
def test_the_logit_gradient_against_fp64_on_the_kernels_own_logits(wdtype, case):
    from efficient_attention import _native as nv
    assert nv.vocab_score_tiles() == (BM, BN, SL)
    print(case, wdtype, "largest |G - G64| / bound: %.4f" % _check_g(case, wdtype))


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_the_logit_gradient_on_the_lm_table(wdtype):
    print(LM, wdtype, "largest |G - G64| / bound: %.4f" % _check_g(LM, wdtype, singles=False))


# ---- 2. the plain GEMM ----------------------------------------------------------------------------------------------------------
GEMMS = [(1, 16, 32), (BM + 3, BN + 24, 96), (2 * BM + 5, 3 * BN + 8, 1056), (256, 1024, 2048)]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", GEMMS, ids=["%dx%dx%d" % s for s in GEMMS])
def test_gemm_nt16_store_and_accumulate(wdtype, shape):
    from efficient_attention import _native as nv
    M, N, K = shape
    a32, b = ops.operands((M, K, N), wdtype, 0)
    a = a32.to(wdtype)
    abuf, bbuf = tv._rows(M, K, K + 8, wdtype, a.cuda()), tv._rows(N, K, K + 24, wdtype, b.cuda())
    want = a.double() @ b.double().t()
    bound = ops.bound(a, b).unsqueeze(1)
    g = torch.Generator().manual_seed(M + N + K)
    prior = torch.randn(M, N, generator=g)
    worst = 0.0
    for accumulate in (0, 1):
        out = torch.full((M + 3, N + 8), 7.0, dtype=torch.float32, device="cuda")
        out[:M, :N] = prior.cuda() if accumulate else float("nan")
        nv.call("ea_gemm_nt16", M, N, K, nv.ptr(abuf), abuf.stride(0), nv.ptr(bbuf), bbuf.stride(0), nv.io_dtype(bbuf), nv.ptr(out),
                out.stride(0), accumulate, nv.stream())
        torch.cuda.synchronize()
        assert (out[M:] == 7.0).all() and (out[:, N:] == 7.0).all()
        got = out[:M, :N].cpu().double()
        assert torch.isfinite(got).all()                                              # (accumulate = 0: the NaNs are gone)
        exact = want + (prior.double() if accumulate else 0.0)
        allowed = bound + (U * prior.double().abs() if accumulate else 0.0)
        ratio = ((got - exact).abs() / allowed).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (shape, wdtype, accumulate, ratio)
        again = out.clone()
        again[:M, :N] = prior.cuda() if accumulate else 0.0
        nv.call("ea_gemm_nt16", M, N, K, nv.ptr(abuf), abuf.stride(0), nv.ptr(bbuf), bbuf.stride(0), nv.io_dtype(bbuf),
                nv.ptr(again), again.stride(0), accumulate, nv.stream())
        torch.cuda.synchronize()
        assert _bits(again, out)
    print(shape, wdtype, "largest |out - fp64| / bound: %.4f" % worst)


# ---- 3. vocab_nll end to end ----------------------------------------------------------------------------------------------------
def _norm_err(got, want):
    return ((got.double() - want).norm() / want.norm()).item()


def _end_to_end(case, wdtype, x_f32):
    from ea_harness.vocab_loss import vocab_nll
    (M, K, V), cc = case
    x32, w = ops.operands((M, K, V), wdtype, 0)
    xh = x32.to(wdtype).cuda()                                                      # the rounded operands, shared by all routes
    w = w.cuda()
    tg = torch.tensor(_targets(M, V, _chunk(M, V, cc))[0], dtype=torch.long).clamp_(0, V - 1).cuda()
    d = _d(M, 1)
    what = (case, wdtype, x_f32)
    assert _live_specials(M, d), what

    def ours(chunk_cols):
        rows = (xh.float() if x_f32 else xh.clone()).view(M, 1, K).requires_grad_(True)
        weight = w.float().requires_grad_(True)                                     # the fp32 master: its values are w's
        with _ctx(wdtype):                                                          # (the master is cast to the autocast dtype)
            logp = vocab_nll(rows, weight, tg.view(M, 1), chunk_cols=chunk_cols)
        logp.backward(d.view(M, 1))
        return logp.detach(), rows.grad.view(M, K), weight.grad
    logp, dx, dw = ours(cc)
    assert dx.dtype == (torch.float32 if x_f32 else wdtype) and dw.dtype == torch.float32 and logp.dtype == torch.float32
    _, want_logp = tv._stack().rows_logprobs((xh.float() if x_f32 else xh).view(M, 1, K), w, tg.view(M, 1))
    assert _bits(logp, want_logp), what
    # the framework route on the same operands and the same d
    xf = (xh.float() if x_f32 else xh.clone()).requires_grad_(True)
    wf = w.float().requires_grad_(True)
    lp = torch.log_softmax(F.linear(xf.to(wdtype), wf.to(wdtype)).float(), dim=-1).gather(1, tg.view(M, 1)).view(M)
    lp.backward(d)
    # fp64 autograd
    x64, w64 = xh.double().requires_grad_(True), w.double().requires_grad_(True)
    torch.log_softmax(x64 @ w64.t(), dim=-1).gather(1, tg.view(M, 1)).view(M).backward(d.double())
    torch.cuda.synchronize()
    errs = {}
    for name, mine, theirs, exact in (("d rows", dx, xf.grad, x64.grad), ("d weight", dw, wf.grad, w64.grad)):
        assert torch.isfinite(mine).all(), (what, name)
        e_mine, e_theirs = _norm_err(mine, exact), _norm_err(theirs, exact)
        errs[name] = (e_mine, e_theirs)
        assert e_mine <= 1.5 * e_theirs, (what, name, e_mine, e_theirs)
    assert (logp.double() - torch.log_softmax(x64 @ w64.t(), dim=-1).gather(1, tg.view(M, 1)).view(M, 1)).abs().max() < 1e-2
    if V > SL:
        # another chunk width: d weight bit for bit (each element written once); d rows within the accumulate bound -- V
        # products and one addition per chunk in any order, twice -- and, into 16-bit rows, one rounding to E of each
        _, dx2, dw2 = ours(2 * SL if cc == SL else SL)
        assert _bits(dw2, dw), what
        p = torch.softmax(x64.detach() @ w64.detach().t(), dim=-1)
        p.scatter_add_(1, tg.view(M, 1), torch.ones(M, 1, dtype=torch.float64, device="cuda"))
        gabs = d.double().abs().view(M, 1) * p * (1.0 + 2.0 ** -8)                       # >= |G| as stored in 16 bits
        allowed = 2.0 * (V + 8 + -(-V // SL)) * U * (gabs @ w64.detach().abs())
        if not x_f32:
            allowed = allowed + ref.unit(wdtype) * (dx.double().abs() + dx2.double().abs() + allowed) + 2.0 * ref.floor(wdtype)
        assert ((dx2.double() - dx.double()).abs() <= allowed).all(), what
    return errs


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("case", SMALL + [LM], ids=_ids(SMALL + [LM]))
def test_vocab_nll_against_fp64_autograd_and_the_framework_route(wdtype, case):
    for x_f32 in (True, False):
        errs = _end_to_end(case, wdtype, x_f32)
        print(case, wdtype, "x fp32" if x_f32 else "x 16-bit",
              "; ".join("%s: ours %.3e framework %.3e" % (k, v[0], v[1]) for k, v in errs.items()))


# ---- 4. memory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_peak_memory_is_the_workspace_and_stays_below_the_logits():
    from efficient_attention import _native as nv
    from ea_harness.vocab_loss import vocab_nll
    M, K, V, cc = 2048, 256, 32768, 2 * SL
    ws = nv.lib().ea_vocab_nll_ws(M, K, V, cc)
    grads = 4 * M * K + 4 * V * K                        # (fp32 rows: d rows is accumulated in the tensor that is returned)
    saved = 2 * V * K + 4 * M                            # the 16-bit table and lse (rows and targets are the caller's own)
    allowed = ws + grads + saved + (2 << 20)
    assert ws > 0 and allowed < M * V * 2, (ws, allowed, M * V * 2)                   # the conditions on the design
    g = torch.Generator().manual_seed(4)
    rows = torch.randn(M, 1, K, generator=g).cuda().requires_grad_(True)
    weight = (torch.randn(V, K, generator=g) / K ** 0.5).cuda().requires_grad_(True)
    tg = torch.randint(0, V, (M, 1), generator=g).cuda()
    d = torch.randn(M, 1, generator=g).cuda()
    vocab_nll(rows, weight, tg, chunk_cols=cc).backward(d)                           # warm-up: the library, the allocator
    rows.grad = weight.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    vocab_nll(rows, weight, tg, chunk_cols=cc).backward(d)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.1f MiB, allowed %.1f MiB, logits in 16 bits %.1f MiB" % (rise / 2 ** 20, allowed / 2 ** 20, M * V * 2 / 2 ** 20))
    assert rows.grad is not None and weight.grad is not None and rise <= allowed, (rise, allowed)


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_and_backward_replay_from_one_graph():
    from ea_harness.vocab_loss import vocab_nll
    (M, K, V), cc = SMALL[3]
    x32, w = ops.operands((M, K, V), torch.bfloat16, 0)
    rows = x32.cuda().view(M, 1, K).requires_grad_(True)
    weight = w.float().cuda().requires_grad_(True)
    tg = torch.tensor(_targets(M, V, cc)[0], dtype=torch.long).clamp_(0, V - 1).cuda().view(M, 1)
    d = _d(M, 5)
    assert _live_specials(M, d)
    d = d.view(M, 1)
    rows.grad, weight.grad = torch.zeros_like(rows), torch.zeros_like(weight)

    def step():
        """ea_harness.trainer's captured step: the gradients keep their storage, zeroed in place, and backward adds to them."""
        rows.grad.zero_()
        weight.grad.zero_()
        logp = vocab_nll(rows, weight, tg, chunk_cols=cc)
        logp.backward(d)
        return logp.detach()
    eager = [t.clone() for t in (step(), rows.grad, weight.grad)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                         # the warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # (captures on a side stream of its own)
        logp = step()
    for _ in range(2):
        for t in (logp, rows.grad, weight.grad):
            t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(_bits(a, b) for a, b in zip((logp, rows.grad, weight.grad), eager))


# ---- 6. the stack ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stack0():
    """tests/test_gpu_decoder_vocab.py's stack with dropout 0."""
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(7)
    m = DecoderStack(tv.VOCAB, tv.C, tv.FFN, tv.HEADS, tv.LAYERS, tv.ATTN, dropout=0.0).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        for layer in m.layers:
            layer.self_attn.rel_pos_bias.relative_attention_bias.weight.mul_(20.0)
        m.embed_tokens.weight.mul_(1.0 / 32)
    return m


INPUT_ONLY, TARGET_ONLY = tv.VOCAB - 1, tv.VOCAB - 2


@functools.lru_cache(maxsize=None)
def _tokens():
    g = torch.Generator().manual_seed(38)
    tokens = torch.randint(2, tv.VOCAB - 2, (3, 44), generator=g)
    tokens[1, 20] = tokens[0, 41] = 1                    # pad_idx as a target (and as an input)
    tokens[2, 0], tokens[2, -1] = INPUT_ONLY, TARGET_ONLY
    return tokens.cuda()


def _grads(m, fn):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(38)                                # (training mode draws the attention's samples: the same ones every run)
    with _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = fn()
    out.backward()
    torch.cuda.synchronize()
    return out.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _same_grads(a, b):
    """Two runs of the same step: every parameter's gradient bit for bit -- the embedding's, the lookup's and the projection's
    both through this loss, among them -- but the relative-position bias tables', which the stack's own backward sums in an
    order that varies from run to run; those agree to the noise of reordered fp32 additions -- a few hundred terms at
    2^-24 each, below 1e-4 of the largest entry -- where one pad row's share of a gradient would be about 1 / 127 of it."""
    assert "embed_tokens.weight" in a
    for k in a:
        if "rel_pos_bias" not in k:
            assert _bits(a[k], b[k]), k
        elif not _bits(a[k], b[k]):
            e = scaled_err(a[k].float().cpu().numpy(), b[k].float().cpu().numpy())
            assert e[0] <= 1e-4, (k, e)


@pytest.mark.gpu
def test_stack_loss_is_minus_evaluate_and_pads_count_for_nothing():
    from ea_harness.vocab_loss import vocab_nll
    m, tokens = _stack0(), _tokens()
    m.eval()
    pad = tokens[:, 1:].eq(m.pad_idx)
    assert int(pad.sum()) == 2
    with _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        none = m.loss(tokens, reduction="none")
        want = m.evaluate(tokens)
        total, mean = m.loss(tokens, reduction="sum"), m.loss(tokens)
    assert none.dtype == torch.float32 and tuple(none.shape) == (3, 43) and none.requires_grad
    assert _bits(none.detach(), -want) and (none[pad] == 0).all() and (none[~pad] > 0).all()
    assert abs(total.item() - none.sum().item()) <= 1e-5 * none.sum().item()
    assert abs(mean.item() - total.item() / 127) <= 1e-6 * abs(mean.item())
    # pads against the same batch with other targets in their place and those rows' d zeroed by hand
    m.train()
    _, with_pads = _grads(m, lambda: m.loss(tokens, reduction="sum"))

    def by_hand():
        rows = m(tokens[:, :-1])
        targets = tokens[:, 1:].t().contiguous()
        keep = targets.ne(m.pad_idx)
        logp = vocab_nll(rows, m.embed_tokens.weight, targets.masked_fill(~keep, 5))
        return -(logp * keep.float()).sum()
    _, hand = _grads(m, by_hand)
    m.eval()
    _same_grads(with_pads, hand)


@pytest.mark.gpu
def test_stack_gradients_against_the_framework_loss_and_under_the_ban(monkeypatch):
    m, tokens = _stack0(), _tokens()
    m.train()
    try:
        loss, mine = _grads(m, lambda: m.loss(tokens))

        def framework():
            rows = m(tokens[:, :-1])
            return F.cross_entropy(m.logits(rows).float().view(-1, tv.VOCAB), tokens[:, 1:].t().reshape(-1),
                                   ignore_index=m.pad_idx, reduction="mean")
        loss_f, theirs = _grads(m, framework)
        assert abs(loss.item() - loss_f.item()) <= 2e-2 * abs(loss_f.item()), (loss.item(), loss_f.item())
        bad = {}
        for k, g in mine.items():
            assert g is not None and torch.isfinite(g).all(), k
            e = scaled_err(g.float().cpu().numpy(), theirs[k].float().cpu().numpy())
            if not (e[0] <= gpu_checks.MODULE_TOL[0] and e[1] <= gpu_checks.MODULE_TOL[1]):
                bad[k] = e
        assert not bad, bad
        emb = mine["embed_tokens.weight"]
        assert emb[INPUT_ONLY].abs().max() > 0 and emb[TARGET_ONLY].abs().max() > 0
        assert int(tokens[:, 1:].eq(INPUT_ONLY).sum()) == 0 and int(tokens[:, :-1].eq(TARGET_ONLY).sum()) == 0
        # the ban: no framework projection onto the table, no framework softmax
        linear = F.linear

        def guarded(x, w, b=None):
            if w.shape[0] == tv.VOCAB:
                raise AssertionError("F.linear on the vocabulary table reached in loss")
            return linear(x, w, b)
        monkeypatch.setattr(F, "linear", guarded)
        for mod, name in ((torch, "log_softmax"), (F, "log_softmax"), (torch.Tensor, "log_softmax"), (torch, "logsumexp"),
                          (torch.Tensor, "logsumexp"), (F, "cross_entropy")):
            def banned(*a, _name=name, **k):
                raise AssertionError("%s reached in loss" % _name)
            monkeypatch.setattr(mod, name, banned)
        loss2, again = _grads(m, lambda: m.loss(tokens))
        monkeypatch.undo()
        assert _bits(loss2, loss)
        _same_grads(again, mine)
    finally:
        m.eval()
