"""-m gpu: the adaptive-softmax training loss (csrc/ea_adaptive_nll.hip: ea_vocab_nll_grad_rows, ea_gemm_nt16_rows,
ea_rows_transpose16, ea_adaptive_score_masked; ea_harness.adaptive_loss.adaptive_nll; DecoderStack.adaptive_loss).  The entries are
called directly on framed buffers pre-filled with sevens or NaN, as in tests/test_gpu_vocab_loss.py.

 1. ea_vocab_nll_grad_rows: every live element within vocab_loss_reference.bound of the fp64 formula on the kernel's OWN fp32
    logits and lse (ea_vocab_score_rows with fp32 logits); G^T == G transposed bit for bit; dead rows, dead columns and pads +0,
    frames intact; the list a stable subset of a larger d / target vector with stale entries 2^30; d == 0 rows exact zeros also
    with NaN x and lse; target_base at a band's first and last column and out of range; NULL lists: ea_vocab_nll_grad's bits.
 2. ea_gemm_nt16_rows within decoder_vocab_operands.bound (+ 2^-24 |prior| accumulating), unlisted rows keep their sevens,
    count 0 writes nothing; ea_rows_transpose16: zeros beyond the count over NaN source rows, fp32 rounded to nearest even.
 3. adaptive_nll end to end: logp has rows_logprobs' bits; the norm-wise relative error of d rows and of EVERY parameter
    gradient against fp64 autograd on the same rounded operands is at most 1.5 times the framework route's (get_log_prob under
    autocast: 16-bit GEMMs, fp32 softmax) -- the margin tests/test_gpu_vocab_loss.py allows for the chunked order of summation;
    table gradients bit for bit between two chunk widths; d rows of M rows == that of the halves; two runs: the same bits.
 4. tail masks: the same criterion against the framework route given the same masks; a mask of ones: the unmasked bits.
 5. forward + backward in ONE torch.cuda.graph with a static targets tensor, captured with all-head targets and replayed after
    copying in the mixed and the all-one-tail targets: the eager runs' bits.  The test of the device-counted design.
 6. the stack: adaptive_loss("none") == -evaluate; pads; gradients against the framework-loss route within MODULE_TOL; the
    tying (band tables' gradients at input-only and target-only tokens); the ban; dropout 0.2 under a seed.
 7. memory: the rise of max_memory_allocated is at most ea_adaptive_nll_ws + the saved workspace + the gradients + 2 MiB, and
    that sum is below 2 M V_last bytes -- arithmetic, before the run."""
import copy
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_decoder_vocab as tv
import test_gpu_adaptive_score as tas
import decoder_vocab_operands as ops
import gpu_checks
import vocab_loss_reference as ref
import vocab_score_reference as sref
from ceva_decoding import _ctx
from util import scaled_err

BM, BN, SL = sref.constants()
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
_bits = tv._bits
U = 2.0 ** -24
STALE = 1 << 30
C = 128
SMALL_CUT, WIDE_CUT = (96, 200, 333), (96, 200, 200 + SL + 8)


def _up64(n):
    return (n + 63) // 64 * 64


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def _counts(M):
    return sorted({c for c in (0, 1, BM, BM + 1, M) if c <= M})


def _zeros_like(t):
    return torch.zeros_like(t)


# ---- 1. the logit gradient over a device-counted list ---------------------------------------------------------------------------
GRAD_CASES = [((1, 32, 16), SL), ((BM + 1, 64, 40), SL), ((2 * BM + 3, 64, SL + 8), SL)]
BASE = 1000


def _grad_rows(M, K, V, xbuf, wbuf, targets, lse, d, v0, Vc, trows, count, base, extra=0):
    """One ea_vocab_nll_grad_rows call into buffers of sevens -> the WHOLE buffers (g [M + 1, ldg], gt [Vc + 1, ldm])."""
    from efficient_attention import _native as nv
    E = wbuf.dtype
    ldg, ldm = _up64(Vc) + extra, _up64(M) + extra
    g = torch.full((M + 1, ldg), 7.0, dtype=E, device="cuda")
    gt = torch.full((Vc + 1, ldm), 7.0, dtype=E, device="cuda")
    nv.call("ea_vocab_nll_grad_rows", M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf),
            nv.ptr(targets), nv.ptr(lse), nv.ptr(d), v0, Vc, nv.ptr(g), ldg, nv.ptr(gt), ldm, nv.ptr(trows), nv.ptr(count), base,
            nv.stream())
    torch.cuda.synchronize()
    assert (g[M] == 7.0).all() and (gt[Vc] == 7.0).all()                               # the frames
    return g, gt


def _whole_rows(M, K, V, cc, live, *args, **kw):
    """G [M, V] from the chunk loop; per chunk: G^T == G transposed, the pads and everything at or beyond `live` are +0."""
    out = []
    for v0 in range(0, V, cc):
        Vc = min(cc, V - v0)
        g, gt = _grad_rows(M, K, V, *args[:5], v0, Vc, *args[5:], **kw)
        assert _bits(gt[:Vc, :M], g[:M, :Vc].t()), (M, K, V, v0)
        assert _bits(g[:M, Vc:], _zeros_like(g[:M, Vc:])) and _bits(gt[:Vc, M:], _zeros_like(gt[:Vc, M:])), (M, K, V, v0, "pads")
        assert _bits(g[live:M], _zeros_like(g[live:M])) and _bits(gt[:Vc, live:], _zeros_like(gt[:Vc, live:])), (M, K, V, v0, "dead")
        out.append(g[:M, :Vc])
    return torch.cat(out, dim=1)


def _big_vectors(M, V):
    """d and targets of 2 M + 5 entries and the list that names M of them in ascending order (a stable subset): position j
    reads entry 2 j + 1.  d is zero at positions 5, 10, ..; positions 1 .. 4 and 6 hold the band's first column, its last,
    the column behind it, the one in front of it and -1."""
    N = 2 * M + 5
    g = torch.Generator().manual_seed(77 + M)
    d = torch.randn(N, generator=g)
    t = torch.tensor([BASE + (7 * m + 3) % V for m in range(N)], dtype=torch.long)
    order = [2 * j + 1 for j in range(M)]
    for j, s in zip((1, 2, 3, 4, 6), (BASE, BASE + V - 1, BASE + V, BASE - 1, -1)):
        if j < M:
            t[order[j]] = s
    for j in range(5, M, 5):
        d[order[j]] = 0.0
    if M == 1:
        t[order[0]] = BASE + V - 1
    return d.cuda(), t.cuda(), order


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("case", GRAD_CASES, ids=["%dx%dx%d" % c[0] for c in GRAD_CASES])
def test_the_row_set_gradient_against_fp64_on_the_kernels_own_logits(wdtype, case):
    from efficient_attention import _native as nv
    (M, K, V), cc = case
    x32, w = ops.operands((M, K, V), wdtype, 0)
    wbuf = tv._table(w.cuda())
    d, t, order = _big_vectors(M, V)
    worst = 0.0
    for x_f32 in (True, False):
        xbuf = tv._rows(M, K, K + 8, torch.float32 if x_f32 else wdtype, x32.cuda() if x_f32 else x32.to(wdtype).cuda())
        logits = tv._logit_buffer(M, V, torch.float32)
        lse = tas._rows_call(M, K, V, xbuf, wbuf, logits)["lse"][:M].contiguous()     # by position: the kernel's own
        L, lse64 = logits[:M, :V].cpu().numpy(), lse.cpu().numpy()
        at = torch.tensor(order, device="cuda")
        tj, dj = (t[at] - BASE).cpu().numpy(), d[at].cpu().numpy()
        want, allowed = ref.grad(L, lse64, dj, tj, V=V), ref.bound(L, lse64, dj, tj, wdtype, V=V)
        full = None
        for count in _counts(M):
            what = (case, wdtype, x_f32, count)
            rows, cnt = _i32(order[:count] + [STALE] * (M - count)), _i32([count])
            G = _whole_rows(M, K, V, cc, count, xbuf, wbuf, t, lse, d, rows, cnt, BASE, extra=64 if count == 1 else 0)
            err = np.abs(G[:count].double().cpu().numpy() - want[:count])
            assert np.isfinite(err).all(), what
            zero = dj[:count] == 0
            assert _bits(G[:count][torch.from_numpy(zero).cuda()], _zeros_like(G[:count][torch.from_numpy(zero).cuda()])), what
            ratio = float((err[~zero] / allowed[:count][~zero]).max()) if (~zero).any() else 0.0
            worst = max(worst, ratio)
            print(what, "largest |G - G64| / bound: %.4f" % ratio)
            assert ratio <= 1.0, (what, ratio)
            if count == M:
                full = G
                assert _bits(G, _whole_rows(M, K, V, cc, M, xbuf, wbuf, t, lse, d, rows, cnt, BASE)), what   # a call repeats its bits
        for count in _counts(M)[:-1]:                                                  # a live row does not depend on the count
            rows, cnt = _i32(order[:count] + [STALE] * (M - count)), _i32([count])
            G = _whole_rows(M, K, V, cc, count, xbuf, wbuf, t, lse, d, rows, cnt, BASE)
            assert _bits(G[:count], full[:count]), (case, wdtype, x_f32, count)
        # a live d == 0 row whose x and lse are NaN: exact zeros there, the other rows untouched
        r = 5 if M > 5 else 0
        xn, ln, dn = xbuf.clone(), lse.clone(), d.clone()
        xn[r], ln[r], dn[order[r]] = float("nan"), float("nan"), 0.0
        rows, cnt = _i32(order), _i32([M])
        Gn = _whole_rows(M, K, V, cc, M, xn, wbuf, t, ln, dn, rows, cnt, BASE)
        keep = torch.ones(M, dtype=torch.bool, device="cuda")
        keep[r] = False
        assert _bits(Gn[r], _zeros_like(Gn[r])) and _bits(Gn[keep], full[keep]), (case, wdtype, x_f32, "NaN row")
        # NULL lists, NULL count, base 0: ea_vocab_nll_grad's bits
        tp, dp = (t[at] - BASE).contiguous(), d[at].contiguous()
        mine = _whole_rows(M, K, V, cc, M, xbuf, wbuf, tp, lse, dp, None, None, 0)
        assert _bits(mine, full), (case, wdtype, x_f32, "NULL lists against the list")
        plain = []
        for v0 in range(0, V, cc):
            Vc = min(cc, V - v0)
            g = torch.full((M + 1, _up64(Vc)), 7.0, dtype=wdtype, device="cuda")
            gt = torch.full((Vc + 1, _up64(M)), 7.0, dtype=wdtype, device="cuda")
            nv.call("ea_vocab_nll_grad", M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf),
                    nv.ptr(tp), nv.ptr(lse), nv.ptr(dp), v0, Vc, nv.ptr(g), g.stride(0), nv.ptr(gt), gt.stride(0), nv.stream())
            plain.append(g[:M, :Vc])
        torch.cuda.synchronize()
        assert _bits(mine, torch.cat(plain, dim=1)), (case, wdtype, x_f32, "NULL lists against ea_vocab_nll_grad")
    print(case, wdtype, "largest |G - G64| / bound over all counts: %.4f" % worst)


# ---- 2. the row-set GEMM and the gathered transpose -----------------------------------------------------------------------------
GEMMS = [(1, 16, 32), (BM + 3, BN + 24, 96), (2 * BM + 5, 40, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", GEMMS, ids=["%dx%dx%d" % s for s in GEMMS])
def test_gemm_nt16_rows_writes_the_listed_live_rows_alone(wdtype, shape):
    from efficient_attention import _native as nv
    M, N, K = shape
    a32, b = ops.operands((M, K, N), wdtype, 0)
    a = a32.to(wdtype)
    abuf, bbuf = tv._rows(M, K, K + 8, wdtype, a.cuda()), tv._rows(N, K, K + 24, wdtype, b.cuda())
    want = a.double() @ b.double().t()
    bound = ops.bound(a, b).unsqueeze(1)
    prior = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N + K))
    order = [2 * (M - 1 - j) + 1 for j in range(M)]                                   # distinct rows of out, descending
    R = 2 * M + 4
    worst = 0.0

    def call(out, accumulate, rows, cnt):
        nv.call("ea_gemm_nt16_rows", M, N, K, nv.ptr(abuf), abuf.stride(0), nv.ptr(bbuf), bbuf.stride(0), nv.io_dtype(bbuf),
                nv.ptr(out), out.stride(0), accumulate, nv.ptr(rows), nv.ptr(cnt), nv.stream())
        torch.cuda.synchronize()
    for accumulate in (0, 1):
        for count in _counts(M):
            what = (shape, wdtype, accumulate, count)
            rows, cnt = _i32(order[:count] + [STALE] * (M - count)), _i32([count])
            at = torch.tensor(order[:count], dtype=torch.long, device="cuda")
            out = torch.full((R, N + 8), 7.0, dtype=torch.float32, device="cuda")
            out[at, :N] = prior[:count].cuda() if accumulate else float("nan")
            before = out.clone()
            call(out, accumulate, rows, cnt)
            untouched = torch.ones(R, dtype=torch.bool, device="cuda")
            untouched[at] = False
            assert _bits(out[untouched], before[untouched]) and (out[:, N:] == 7.0).all(), what   # (count 0: nothing is written)
            got = out[at, :N].cpu().double()
            assert torch.isfinite(got).all(), what
            exact = want[:count] + (prior[:count].double() if accumulate else 0.0)
            allowed = bound[:count] + (U * prior[:count].double().abs() if accumulate else 0.0)
            ratio = ((got - exact).abs() / allowed).max().item() if count else 0.0
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, ratio)
            again = before.clone()
            call(again, accumulate, rows, cnt)
            assert _bits(again, out), what
        # NULL list and count: ea_gemm_nt16's bits
        mine = torch.full((M + 3, N + 8), 7.0, dtype=torch.float32, device="cuda")
        mine[:M, :N] = prior.cuda()
        theirs = mine.clone()
        call(mine, accumulate, None, None)
        nv.call("ea_gemm_nt16", M, N, K, nv.ptr(abuf), abuf.stride(0), nv.ptr(bbuf), bbuf.stride(0), nv.io_dtype(bbuf),
                nv.ptr(theirs), theirs.stride(0), accumulate, nv.stream())
        torch.cuda.synchronize()
        assert _bits(mine, theirs), (shape, wdtype, accumulate)
    print(shape, wdtype, "largest |out - fp64| / bound: %.4f" % worst)


TRANSPOSES = [(1, 32), (BM + 1, 96), (130, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", TRANSPOSES, ids=["%dx%d" % s for s in TRANSPOSES])
def test_rows_transpose16_gathers_rounds_and_zeroes_beyond_the_count(wdtype, shape):
    from efficient_attention import _native as nv
    M, K = shape
    R, ld = 2 * M + 4, K + 8
    src32 = torch.randn(R, K, generator=torch.Generator().manual_seed(5 * M + K))
    eps = 2.0 ** -8 if wdtype == torch.bfloat16 else 2.0 ** -11                        # half an ulp of the type at 1
    src32[:, 0], src32[:, 1 % K], src32[:, 2 % K] = 1.0 + eps, 1.0 + 3.0 * eps, -(1.0 + eps)   # ties: to even, both ways
    order = [2 * (M - 1 - j) + 1 for j in range(M)]
    for src_f32 in (True, False):
        for use_list in (True, False):
            for count in _counts(M):
                what = (shape, wdtype, src_f32, use_list, count)
                src = tv._rows(R - 1, K, ld, torch.float32 if src_f32 else wdtype, src32[:R - 1].cuda())
                named = order[:count] if use_list else list(range(count))
                if not use_list:
                    src[count:] = float("nan")                                        # the rows beyond the count: never read
                else:
                    dead = torch.ones(R, dtype=torch.bool, device="cuda")
                    dead[torch.tensor(named, dtype=torch.long, device="cuda")] = False
                    src[dead] = float("nan")
                rows = _i32(order[:count] + [STALE] * (M - count)) if use_list else None
                ldm = _up64(M) + (64 if count == 1 else 0)
                out = torch.full((K + 1, ldm), 7.0, dtype=wdtype, device="cuda")
                nv.call("ea_rows_transpose16", M, K, nv.ptr(src), tv._code(src), ld, nv.ptr(rows), nv.ptr(_i32([count])), nv.ptr(out),
                        nv.io_dtype(out), ldm, nv.stream())
                torch.cuda.synchronize()
                assert (out[K] == 7.0).all(), what
                want = src[torch.tensor(named, dtype=torch.long, device="cuda"), :K].to(wdtype).t()   # (the framework rounds to nearest even)
                assert torch.isfinite(want.float()).all() and _bits(out[:K, :count], want.contiguous()), what
                assert _bits(out[:K, count:], _zeros_like(out[:K, count:])), what
    # NULL count: every position is live
    src = tv._rows(M, K, ld, torch.float32, src32[:M].cuda())
    out = torch.full((K + 1, _up64(M)), 7.0, dtype=wdtype, device="cuda")
    nv.call("ea_rows_transpose16", M, K, nv.ptr(src), tv._code(src), ld, None, None, nv.ptr(out), nv.io_dtype(out), _up64(M), nv.stream())
    torch.cuda.synchronize()
    assert _bits(out[:K, :M], src[:M, :K].to(wdtype).t().contiguous()) and _bits(out[:K, M:], _zeros_like(out[:K, M:]))
    one = torch.tensor([1.0 + eps, 1.0 + 3.0 * eps]).to(wdtype).double()
    assert one[0].item() == 1.0 and one[1].item() == 1.0 + 4.0 * eps                  # what "to nearest even" means here


# ---- 3. adaptive_nll end to end -------------------------------------------------------------------------------------------------
NAMES = ("d rows", "band 0 table", "class rows", "tail 0 projection", "tail 0 table", "tail 1 projection", "tail 1 table")


@functools.lru_cache(maxsize=None)
def _softmax(cutoff, wdtype):
    """A tied AdaptiveSoftmax on the device whose fp32 masters hold values of `wdtype`: every route sees the same operands."""
    from ea_harness.adaptive import AdaptiveInput, AdaptiveSoftmax
    torch.manual_seed(100 + len(cutoff) + cutoff[-1])
    inp = AdaptiveInput(cutoff[-1], 1, C, 2, C, list(cutoff))
    sm = AdaptiveSoftmax(cutoff[-1], C, list(cutoff[:-1]), 0.0, factor=2, adaptive_inputs=inp, tie_proj=True).cuda()
    with torch.no_grad():
        for p in sm.parameters():
            p.copy_(p.to(wdtype).float())
    assert sm.band_dims() == [64, 32]
    return sm


def _params(sm):
    return [sm.head.word_proj.weight, sm.head.class_proj.weight, sm.tail[0][0].weight, sm.tail[0][2].weight,
            sm.tail[1][0].weight, sm.tail[1][2].weight]


def _mix(name, M, cutoff):
    """-> (targets [M], d [M]) on the device."""
    c0, c1, V = cutoff
    g = torch.Generator().manual_seed(M + len(name))
    d = torch.randn(M, generator=g)
    head = torch.randint(0, c0, (M,), generator=g)
    if name == "head":
        t = head
    elif name == "one_tail":
        t = torch.randint(c1, V, (M,), generator=g)
        t[0] = c1
        t[M - 1] = V - 1
    else:
        t = head.clone()
        n1 = min(BM + 1, max(M - 10, 0))                 # tail 1: BM + 1 rows where M has room for them
        at = torch.randperm(M, generator=g)
        t[at[0]] = c0 + (M % (c1 - c0))                  # tail 0: exactly one row
        t[at[1:1 + n1]] = torch.randint(c1, V, (n1,), generator=g)
        if name == "pads" and M > 10:
            rest = at[1 + n1:]
            t[rest[0]], t[rest[1]], t[rest[2]] = V, -1, 1 << 40                       # out of range: NaN, d = 0
            d[rest[:5]] = 0.0
            d[at[2]] = 0.0                               # a tail row with d = 0
    return t.cuda(), d.cuda()


def _framework(sm, x, t, masks=None):
    """AdaptiveSoftmax.get_log_prob(x, t) -- the route that reads indices back -- with the tails' masks where given."""
    if masks is None:
        return sm.get_log_prob(x, t)
    c0, n = sm.cutoff[0], len(sm.tail)
    head = F.log_softmax(F.linear(x, sm.head_table()), dim=-1)
    out = torch.full((t.numel(),), float("nan"), dtype=head.dtype, device=x.device)
    at = ((t >= 0) & (t < c0)).nonzero().squeeze(1)
    out[at] = head[at, t[at]]
    for i in range(n):
        at = ((t >= sm.cutoff[i]) & (t < sm.cutoff[i + 1])).nonzero().squeeze(1)
        if at.numel():
            h = F.linear(x[at], sm.tail_projection(i))
            if masks[i] is not None:
                h = h * masks[i][:at.numel()].to(h.dtype)
            tail = F.log_softmax(F.linear(h, sm.tail_table(i)), dim=-1)
            out[at] = head[at, c0 + i] + tail[torch.arange(at.numel(), device=at.device), t[at] - sm.cutoff[i]]
    return out


def _route(sm, x, t, d, fn):
    for p in sm.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    logp = fn(sm, xg)
    logp.backward(d.to(logp.dtype).view(logp.shape))
    torch.cuda.synchronize()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()   # noqa: E731
    out = logp.detach().reshape(-1), [xg.grad.reshape(x.shape[0], -1)] + [zero(p) for p in _params(sm)]
    for p in sm.parameters():
        p.grad = None
    return out


def _ours(sm, x, t, d, wdtype, cc, masks=None):
    from ea_harness.adaptive_loss import adaptive_nll
    M = x.shape[0]

    def fn(sm, xg):
        with _ctx(wdtype):
            return adaptive_nll(xg.view(M, 1, -1), sm, t.view(M, 1), chunk_cols=cc, tail_masks=masks)
    return _route(sm, x, t, d, fn)


def _norm_err(got, want):
    return ((got.double() - want).norm() / want.norm()).item()


def _criterion(what, sm, x, t, d, wdtype, mine, masks=None):
    """The norm-wise relative error of every gradient against fp64 autograd: at most 1.5 times the framework route's."""
    def framework(sm, xg):
        with _ctx(wdtype):
            return _framework(sm, xg, t, masks)
    _, theirs = _route(sm, x, t, d, framework)
    sm64 = copy.deepcopy(sm).double()
    m64 = None if masks is None else [None if m is None else m.double() for m in masks]
    logp64, exact = _route(sm64, x.double(), t, d.double(), lambda s, xg: _framework(s, xg, t, m64))
    errs = {}
    for name, a, b, e in zip(NAMES, mine, theirs, exact):
        assert torch.isfinite(a).all(), (what, name)
        if e.norm().item() == 0.0:                       # (a tail nobody's target lies in: exact zeros, from every route)
            assert _bits(a, _zeros_like(a)), (what, name)
            continue
        errs[name] = (_norm_err(a, e), _norm_err(b, e))
    print(what, "; ".join("%s: ours %.3e framework %.3e" % (k, v[0], v[1]) for k, v in errs.items()))
    for name, (e_mine, e_theirs) in errs.items():
        assert e_mine <= 1.5 * e_theirs, (what, name, e_mine, e_theirs)
    return logp64, errs


def _rows_of(M, wdtype, x_f32=True):
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(9 + M)).to(wdtype)
    return (x.float() if x_f32 else x).cuda()


E2E = [(SMALL_CUT, 1), (SMALL_CUT, BM + 1), (SMALL_CUT, 2 * BM + 3), (WIDE_CUT, 2 * BM + 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("mix", ["head", "one_tail", "mixed", "pads"])
@pytest.mark.parametrize("geometry", E2E, ids=["V%d-M%d" % (g[0][-1], g[1]) for g in E2E])
def test_adaptive_nll_against_fp64_autograd_and_the_framework_route(geometry, mix, wdtype):
    from ea_harness import token_pick as tp
    cutoff, M = geometry
    sm = _softmax(cutoff, wdtype)
    t, d = _mix(mix, M, cutoff)
    for x_f32 in ((True, False) if mix == "mixed" else (True,)):
        what = (cutoff, M, mix, wdtype, x_f32)
        x = _rows_of(M, wdtype, x_f32)
        logp, mine = _ours(sm, x, t, d, wdtype, SL)
        assert logp.dtype == torch.float32 and mine[0].dtype == x.dtype and all(g.dtype == torch.float32 for g in mine[1:])
        tables = tp.AdaptiveTables(sm, wdtype, x.device)
        _, want = tv._stack().rows_logprobs(x.view(M, 1, C), tables, t.view(M, 1))
        assert _bits(logp, want.view(M)), what
        logp64, _ = _criterion(what, sm, x, t, d, wdtype, mine)
        ok = (t >= 0) & (t < cutoff[-1])
        # (that it is the same quantity; the accuracy is the gradients' criterion above)
        assert torch.isnan(logp[~ok]).all() and (logp[ok].double() - logp64[ok]).abs().max() < 5e-2, what
        if mix == "head":
            assert all(_bits(g, _zeros_like(g)) for g in mine[3:]), what              # every tail has count 0
        # two runs: the same bits; another chunk width: the tables' gradients bit for bit
        logp2, again = _ours(sm, x, t, d, wdtype, SL)
        assert _bits(logp2, logp) and all(_bits(a, b) for a, b in zip(again, mine)), what
        _, wide = _ours(sm, x, t, d, wdtype, 2 * SL)
        assert all(_bits(wide[k], mine[k]) for k in (1, 2, 4, 6)), what
        if M > 1:                                                                     # the halves: d rows bit for bit
            h = M // 2
            for a, b in ((0, h), (h, M)):
                _, part = _ours(sm, x[a:b].contiguous(), t[a:b].contiguous(), d[a:b].contiguous(), wdtype, SL)
                assert _bits(part[0], mine[0][a:b]), (what, a, b)
        zero = d == 0
        if zero.any():
            assert _bits(mine[0][zero], _zeros_like(mine[0][zero])), what


# ---- 4. tail masks --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_tail_masks_against_the_framework_route_and_a_mask_of_ones(wdtype):
    M = 2 * BM + 3
    sm = _softmax(SMALL_CUT, wdtype)
    t, d = _mix("mixed", M, SMALL_CUT)
    t[:40] = torch.randint(SMALL_CUT[0], SMALL_CUT[1], (40,), generator=torch.Generator().manual_seed(1)).cuda()   # a fuller tail 0
    x = _rows_of(M, wdtype)
    g = torch.Generator().manual_seed(12)
    masks = [(torch.rand(M, dim, generator=g) < 0.8).to(wdtype).mul_(1.25).cuda() for dim in sm.band_dims()]   # {0, 1 / (1 - 0.2)}
    logp, mine = _ours(sm, x, t, d, wdtype, SL, masks)
    logp64, _ = _criterion(("masks", wdtype), sm, x, t, d, wdtype, mine, masks)
    assert (logp.double() - logp64).abs().max() < 5e-2
    one, plain = _ours(sm, x, t, d, wdtype, SL, [masks[0], None]), _ours(sm, x, t, d, wdtype, SL)
    assert not _bits(one[0], plain[0]) and not _bits(one[0], logp)                    # (each mask is felt)
    ones = [torch.ones_like(m) for m in masks]
    lp1, g1 = _ours(sm, x, t, d, wdtype, SL, ones)
    assert _bits(lp1, plain[0]) and all(_bits(a, b) for a, b in zip(g1, plain[1])), wdtype


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_and_backward_replay_from_one_graph_with_other_targets():
    from ea_harness.adaptive_loss import adaptive_nll
    wdtype, M = torch.bfloat16, 2 * BM + 3
    sm = _softmax(SMALL_CUT, wdtype)
    params = _params(sm)
    mixes = {name: _mix(name, M, SMALL_CUT)[0].view(M, 1) for name in ("head", "mixed", "one_tail")}
    d = _mix("mixed", M, SMALL_CUT)[1].view(M, 1)
    rows = _rows_of(M, wdtype).view(M, 1, C).requires_grad_(True)
    targets = mixes["head"].clone()                                                    # the static tensor
    try:
        rows.grad = torch.zeros_like(rows)
        for p in params:
            p.grad = torch.zeros_like(p)
        outs = lambda: [rows.grad] + [p.grad for p in params]                         # noqa: E731

        def step():
            """ea_harness.trainer's captured step: the gradients keep their storage, zeroed in place, and backward adds to them."""
            for gr in outs():
                gr.zero_()
            with _ctx(wdtype):
                logp = adaptive_nll(rows, sm, targets, chunk_cols=SL)
            logp.backward(d)
            return logp.detach()
        eager = {}
        for name, tg in mixes.items():
            targets.copy_(tg)
            eager[name] = [step().clone()] + [gr.clone() for gr in outs()]
        assert not _bits(eager["mixed"][0], eager["head"][0]) and eager["mixed"][4].abs().max() > 0
        targets.copy_(mixes["head"])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                                                                     # the warm-up on a side stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            logp = step()
        for name in ("mixed", "one_tail", "head"):
            targets.copy_(mixes[name])
            for tns in [logp] + outs():
                tns.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(_bits(a, b) for a, b in zip([logp] + outs(), eager[name])), name
    finally:
        for p in params:
            p.grad = None


# ---- 6. the stack ---------------------------------------------------------------------------------------------------------------
STACK_CUT = (400, 700, tv.VOCAB)
INPUT_ONLY, TARGET_ONLY = (398, 698, 998), (399, 699, 999)


@functools.lru_cache(maxsize=None)
def _stack(p):
    """tests/test_gpu_decoder_vocab.py's geometry with the adaptive layers, dropout 0 in the stack and p in the adaptive softmax."""
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(7)
    m = DecoderStack(tv.VOCAB, tv.C, tv.FFN, tv.HEADS, tv.LAYERS, tv.ATTN, dropout=0.0,
                     adaptive=dict(cutoff=list(STACK_CUT[:2]), factor=2, dropout=p)).cuda()
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.02 * torch.randn_like(q))
        for layer in m.layers:
            layer.self_attn.rel_pos_bias.relative_attention_bias.weight.mul_(20.0)
    return m.eval()


@functools.lru_cache(maxsize=None)
def _tokens():
    g = torch.Generator().manual_seed(38)
    tokens = torch.randint(2, tv.VOCAB, (3, 44), generator=g)
    for s in INPUT_ONLY + TARGET_ONLY:
        tokens[tokens == s] = 5
    tokens[1, 20] = tokens[0, 41] = 1                    # pad_idx as a target (and as an input)
    for b in range(3):
        tokens[b, 0], tokens[b, -1] = INPUT_ONLY[b], TARGET_ONLY[b]
    return tokens.cuda()


def _grads(m, fn, seed=38):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)                              # (training mode draws the attention's samples and the dropouts)
    with _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = fn()
    out.backward()
    torch.cuda.synchronize()
    got = {k: (None if q.grad is None else q.grad.detach().clone()) for k, q in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return out.detach(), got


def _same_grads(a, b):
    """Two runs of the same step: every gradient bit for bit but the relative-position bias tables', which the stack's own
    backward sums in an order that varies from run to run (tests/test_gpu_vocab_loss.py: below 1e-4 of the largest entry)."""
    assert any("embeddings" in k for k in a)
    for k in a:
        if "rel_pos_bias" not in k:
            assert _bits(a[k], b[k]), k
        elif not _bits(a[k], b[k]):
            e = scaled_err(a[k].float().cpu().numpy(), b[k].float().cpu().numpy())
            assert e[0] <= 1e-4, (k, e)


@pytest.mark.gpu
def test_stack_adaptive_loss_is_minus_evaluate_and_pads_count_for_nothing():
    from ea_harness.adaptive_loss import adaptive_nll
    m, tokens = _stack(0.0), _tokens()
    pad = tokens[:, 1:].eq(m.pad_idx)
    assert int(pad.sum()) == 2
    with _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        none = m.adaptive_loss(tokens, reduction="none")
        want = m.evaluate(tokens)
        total, mean = m.adaptive_loss(tokens, reduction="sum"), m.adaptive_loss(tokens)
    assert none.dtype == torch.float32 and tuple(none.shape) == (3, 43) and none.requires_grad
    assert _bits(none.detach(), -want) and (none[pad] == 0).all() and (none[~pad] > 0).all()
    assert abs(total.item() - none.sum().item()) <= 1e-5 * none.sum().item()
    assert abs(mean.item() - total.item() / 127) <= 1e-6 * abs(mean.item())
    m.train()
    try:
        _, with_pads = _grads(m, lambda: m.adaptive_loss(tokens, reduction="sum"))

        def by_hand():                                   # other targets in the pads' place and those rows' d zeroed by hand
            rows = m(tokens[:, :-1])
            targets = tokens[:, 1:].t().contiguous()
            keep = targets.ne(m.pad_idx)
            logp = adaptive_nll(rows, m.adaptive_softmax, targets.masked_fill(~keep, 5))
            return -(logp * keep.float()).sum()
        _, hand = _grads(m, by_hand)
    finally:
        m.eval()
    _same_grads(with_pads, hand)


@pytest.mark.gpu
def test_stack_gradients_against_the_framework_loss_the_tying_and_the_ban(monkeypatch):
    m, tokens = _stack(0.0), _tokens()
    m.train()
    try:
        loss, mine = _grads(m, lambda: m.adaptive_loss(tokens))

        def framework():
            rows = m(tokens[:, :-1])
            targets = tokens[:, 1:].t().contiguous()
            keep = targets.ne(m.pad_idx)
            logp = m.adaptive_softmax.get_log_prob(rows, targets)
            return -(logp.float().masked_fill(~keep, 0.0)).sum() / keep.sum()
        loss_f, theirs = _grads(m, framework)
        assert abs(loss.item() - loss_f.item()) <= 2e-2 * abs(loss_f.item()), (loss.item(), loss_f.item())
        bad = {}
        for k, g in mine.items():
            assert g is not None and torch.isfinite(g).all(), k
            e = scaled_err(g.float().cpu().numpy(), theirs[k].float().cpu().numpy())
            print(k, "max %.3e rms %.3e" % e)
            if not (e[0] <= gpu_checks.MODULE_TOL[0] and e[1] <= gpu_checks.MODULE_TOL[1]):
                bad[k] = e
        assert not bad, bad
        # the tying: a band's table hears of a token that is only ever an input and of one that is only ever a target
        for b in range(3):
            start = STACK_CUT[b - 1] if b else 0
            emb = mine["embed_tokens.embeddings.%d.0.weight" % b]
            assert emb[INPUT_ONLY[b] - start].abs().max() > 0 and emb[TARGET_ONLY[b] - start].abs().max() > 0, b
            assert int(tokens[:, 1:].eq(INPUT_ONLY[b]).sum()) == 0 and int(tokens[:, :-1].eq(TARGET_ONLY[b]).sum()) == 0
            assert mine["embed_tokens.embeddings.%d.1.weight" % b].abs().max() > 0
        # the ban: no framework projection onto the head or a tail table, no framework softmax, no index read-back
        linear = F.linear
        heights = {STACK_CUT[0] + 2, STACK_CUT[1] - STACK_CUT[0], STACK_CUT[2] - STACK_CUT[1]}

        def guarded(x, w, b=None):
            if w.shape[0] in heights:
                raise AssertionError("F.linear on the head or a tail table reached in adaptive_loss")
            return linear(x, w, b)
        monkeypatch.setattr(F, "linear", guarded)
        for mod, name in ((torch, "log_softmax"), (F, "log_softmax"), (torch.Tensor, "log_softmax"), (torch, "logsumexp"),
                          (torch.Tensor, "logsumexp"), (F, "cross_entropy"), (torch, "nonzero"), (torch.Tensor, "nonzero")):
            def banned(*a, _name=name, **k):
                raise AssertionError("%s reached in adaptive_loss" % _name)
            monkeypatch.setattr(mod, name, banned)
        loss2, again = _grads(m, lambda: m.adaptive_loss(tokens))
        monkeypatch.undo()
        assert _bits(loss2, loss)
        _same_grads(again, mine)
    finally:
        m.eval()


@pytest.mark.gpu
def test_stack_dropout_is_drawn_from_the_seed():
    m, plain, tokens = _stack(0.2), _stack(0.0), _tokens()
    assert m.adaptive_softmax.dropout == 0.2
    m.train()
    plain.train()
    try:
        a, ga = _grads(m, lambda: m.adaptive_loss(tokens))
        b, gb = _grads(m, lambda: m.adaptive_loss(tokens))
        c, gc = _grads(m, lambda: m.adaptive_loss(tokens), seed=39)
        d, _ = _grads(plain, lambda: plain.adaptive_loss(tokens))
    finally:
        m.eval()
        plain.eval()
    assert _bits(a, b) and not _bits(a, c) and not _bits(a, d)
    _same_grads(ga, gb)
    k = "embed_tokens.embeddings.2.0.weight"
    assert torch.isfinite(ga[k]).all() and not _bits(ga[k], gc[k])
    with _ctx(torch.bfloat16), warnings.catch_warnings():                             # eval mode: no dropout, evaluate's bits
        warnings.simplefilter("ignore")
        assert _bits(m.adaptive_loss(tokens, reduction="none").detach(), -m.evaluate(tokens))


# ---- 7. memory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_peak_memory_is_the_workspace_and_stays_below_the_last_tails_logits():
    from efficient_attention import _native as nv
    from ea_harness.adaptive import AdaptiveSoftmax
    from ea_harness.adaptive_loss import adaptive_nll
    M, K, cutoff, cc = 2048, 256, [1000, 3000, 63000], SL
    dims, n = [128, 64], 2
    heights = [cutoff[0] + n, cutoff[1] - cutoff[0], cutoff[2] - cutoff[1]]
    cut, hd = nv.host_array(ctypes.c_int64, cutoff), nv.host_array(ctypes.c_int32, dims)
    ws = nv.lib().ea_adaptive_nll_ws(M, K, n, cut, hd, cc)
    operands = heights[0] * K + sum(d * K + v * d for d, v in zip(dims, heights[1:]))   # elements of the head, projections, tables
    saved = nv.lib().ea_adaptive_score_ws(M, n, cut, hd) + 2 * operands                 # the kept workspace, the 16-bit operands
    grads = 4 * M * K + 4 * operands                     # fp32: d rows (accumulated in the tensor that is returned) and every parameter's
    allowed = ws + saved + grads + (2 << 20)
    assert ws > 0 and allowed < 2 * M * heights[2], (ws, allowed, 2 * M * heights[2])  # the conditions on the design
    torch.manual_seed(4)
    sm = AdaptiveSoftmax(cutoff[-1], K, cutoff[:-1], 0.0, factor=2).cuda()
    assert sm.band_dims() == dims
    g = torch.Generator().manual_seed(4)
    rows = torch.randn(M, 1, K, generator=g).cuda().requires_grad_(True)
    tg = torch.randint(0, cutoff[-1], (M, 1), generator=g).cuda()                      # (most of them in the tall last tail)
    d = torch.randn(M, 1, generator=g).cuda()
    adaptive_nll(rows, sm, tg, chunk_cols=cc).backward(d)                              # warm-up: the library, the allocator
    rows.grad = None
    sm.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    adaptive_nll(rows, sm, tg, chunk_cols=cc).backward(d)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.1f MiB, allowed %.1f MiB, the last tail's logits in 16 bits %.1f MiB"
          % (rise / 2 ** 20, allowed / 2 ** 20, 2 * M * heights[2] / 2 ** 20))
    assert rows.grad is not None and all(p.grad is not None and torch.isfinite(p.grad).all() for p in sm.parameters())
    assert rise <= allowed, (rise, allowed)
