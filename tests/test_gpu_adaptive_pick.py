"""-m gpu: the greedy pick from the adaptive head (csrc/ea_adaptive_pick.hip, C ABI 34) and DecoderStack on a state made by
init_adaptive_decoding.  bf16 and fp16 tables, x in fp32 and in the table's type, in the framed buffers of
tests/test_gpu_vocab_score.py (x with a NaN frame, tables with NaN / +inf rows behind them, outputs with a guard element, the
workspace 0xFF-filled with 16 guard bytes); SPAN and MAX_K are the library's (include/ea_hip.h).

 Geometries   A  C 128, cutoffs [37, 187, 257], widths (64, 32): c0 off the 16-grid, ragged last tiles
              B  C 256, cutoffs [48, 48 + 16 k + 5] with 16 k + 5 > 2 SPAN, width (256): three spans of the column-split kernel
                 and its longest accumulator chain
              C  C 128, four tails of widths (64, 32, 32, 288): the K-split fallback (288 > MAX_K) and the maximum n
              M in {1, 17, 64}
 P1 fp64      same operands (the kernel's own h_i, read from the workspace): per band lse and the best value, the class logits
              and logp, with and without targets, within adaptive_score_reference.tol_logp on decoder_vocab_operands.bound,
              summed over the bands a score uses; h_i within tol_h; the token by the gap rule of adaptive_pick_reference.
              SEEDS names the operand seeds: with h_i rounded from fp64 on the host no row of any case is a near tie.
 P2 planted   a planted winner at columns 0, 15, 16, the last column of a span, the first of the next and V_b - 1 of every
              band, by an fp64 margin >= 1 asserted on the host: the token is exact; duplicated table rows give the lower index.
 P3 rows      M = 64 equals 64 calls of M = 1 bit for bit; fp32 x holding 16-bit values equals 16-bit x; separate projections
              equal the joined copy; a NaN row beside finite rows; two calls.
 P4 capture   a captured call replayed on rewritten x and targets has the eager bits.
 P5 stack     tests/test_gpu_adaptive_score.py's fixture (V 333, C 128): generate captured == eager (tokens, rows, logp), against
              fp64 by P1's rules; next_tokens under the ban of framework ops; token_logprobs with targets; a ragged prompt on a
              per_sequence state; refresh_decoding_weights; decoding_state_nbytes; score."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import adaptive_pick_reference as pref
import adaptive_score_reference as aref
import decoder_vocab_operands as ops
import test_gpu_decoder_vocab as tv
import test_gpu_vocab_score as tvs
from ceva_decoding import _ctx
from test_adaptive_cpu import edge_targets

SPAN, MAX_K = pref.constants()
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
_bits = tv._bits
GEOMETRIES = {"A": dict(C=128, cutoffs=[37, 187, 257], dims=[64, 32]),
              "B": dict(C=256, cutoffs=[48, 48 + 2 * SPAN + 16 + 5], dims=[256]),
              "C": dict(C=128, cutoffs=[40, 100, 160, 300, 500], dims=[64, 32, 32, MAX_K + 32])}
MS = (1, 17, 64)
# the operand seeds of P1 (one per geometry): test_p1_seeds_have_no_near_tie_on_the_host checks them
SEEDS = {"A": 1, "B": 2, "C": 5}


@functools.lru_cache(maxsize=None)
def _operands(name, wdtype, M=64):
    """CPU: x32 [M, C], and in `wdtype` the head [c0 + n, C], the projections [d_i, C], the tables [V_i, d_i]."""
    geo = GEOMETRIES[name]
    C, cut, dims = geo["C"], geo["cutoffs"], geo["dims"]
    g = torch.Generator().manual_seed(100 * SEEDS[name] + ord(name) + (wdtype == torch.float16))
    x32 = torch.randn(M, C, generator=g)
    head = torch.randn(cut[0] + len(dims), C, generator=g) / C ** 0.5
    head[cut[0]:] *= 3.0                                              # (class logits large enough for tails to win rows)
    head = head.to(wdtype)
    projs = tuple((torch.randn(d, C, generator=g) / C ** 0.5).to(wdtype) for d in dims)
    tabs = tuple((torch.randn(cut[i + 1] - cut[i], d, generator=g) * (2.0 / d ** 0.5)).to(wdtype) for i, d in enumerate(dims))
    return x32, head, projs, tabs


def _device(head, projs, tabs, joined=True):
    """The framed device operands: (head, [proj_i], [table_i]); joined: the projections are the row blocks of one buffer."""
    if joined:
        both = torch.cat(list(projs), 0).cuda()
        pj = list(both.split([p.shape[0] for p in projs], 0))
    else:
        pj = [p.cuda().clone() for p in projs]
    return tv._table(head.cuda()), pj, [tv._table(w.cuda()) for w in tabs]


def _call(geo, M, xbuf, dev, targets, ws, token, logp):
    from efficient_attention import _native as nv
    C, cut, dims = geo["C"], geo["cutoffs"], geo["dims"]
    head, projs, tabs = dev
    nv.call("ea_adaptive_pick", M, C, len(dims), nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims),
            nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(targets), nv.ptr(head), nv.io_dtype(head),
            nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in projs]),
            nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tabs]), nv.ptr(ws), ws.numel() - 16, nv.ptr(token),
            nv.ptr(logp), nv.stream())


def _pick(geo, M, xbuf, dev, targets=None):
    """One ea_adaptive_pick call on fresh framed buffers -> dict(token [M], logp [M], and the workspace's parts: cls [M, n],
    h [i] [M, d_i], best_v / best_i / lse / tlogit [b] [M])."""
    from efficient_attention import _native as nv
    cut, dims = geo["cutoffs"], geo["dims"]
    n = len(dims)
    lay = pref.ws_layout(M, cut, dims)
    nbytes = nv.lib().ea_adaptive_pick_ws(M, n, nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims))
    assert nbytes == lay["total"]
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    token = torch.full((M + 1,), -7, dtype=torch.long, device="cuda")
    logp = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    _call(geo, M, xbuf, dev, targets, ws, token, logp)
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xFF).all() and token[M].item() == -7 and logp[M].item() == 7.0

    def part(name, dtype, count):
        size = torch.empty((), dtype=dtype).element_size()
        return ws[lay[name]:lay[name] + size * count].view(dtype)
    wdtype = dev[0].dtype
    hall = part("h", wdtype, M * lay["D"]).view(M, lay["D"])
    out = dict(token=token[:M], logp=logp[:M], cls=part("cls", torch.float32, M * n).view(M, n),
               h=list(hall.split(dims, 1)), best_v=[], best_i=[], lse=[], tlogit=[])
    for b in range(n + 1):
        best = part("best%d" % b, torch.int32, 2 * M).view(M, 2)
        out["best_v"].append(best[:, 0].contiguous().view(torch.float32))
        out["best_i"].append(best[:, 1].contiguous())
        out["lse"].append(part("lse%d" % b, torch.float32, M))
        out["tlogit"].append(part("tlogit%d" % b, torch.float32, M))
    return out


def _targets(cut, M, seed):
    V = cut[-1]
    t = np.random.RandomState(seed).randint(0, V, size=M).astype(np.int64)
    edges = edge_targets(cut) + [-1, V]
    k = min(M, len(edges))
    t[:k] = edges[:k]
    return t


def _band_tols(geo, wdtype, xh, head, tabs, ref, own_h):
    """-> tol [n + 1][M]: adaptive_score_reference.tol_logp of every band's pass on its own operands."""
    M, n = xh.shape[0], len(geo["dims"])
    bounds = [ops.bound(xh, head).numpy()] + [ops.bound(own_h[i], tabs[i]).numpy() for i in range(n)]
    rows = [ref["head_rows"]] + ref["tail_rows"]
    return [np.array([aref.tol_logp(bounds[b][m], rows[b][m], ref["lse"][b][m]) for m in range(M)]) for b in range(n + 1)]


def _check_p1(geo, wdtype, xh, head, projs, tabs, got, targets, what, check_h=True):
    """P1's checks of one call's results `got` (on the device) against fp64 on CPU operands -> (worst error / tolerance,
    near-tie rows).  xh: the rows as the kernel rounds them, [M, C] in wdtype."""
    cut, dims = geo["cutoffs"], geo["dims"]
    M, n, c0, V = xh.shape[0], len(dims), cut[0], cut[-1]
    own_h = [h.cpu() for h in got["h"]]
    worst = 0.0
    if check_h:
        for i in range(n):
            h64 = (xh.double() @ projs[i].double().t()).numpy()
            allowed = aref.tol_h(ops.bound(xh, projs[i]).numpy()[:, None], h64, wdtype)
            ratio = float((np.abs(own_h[i].double().numpy() - h64) / allowed).max())
            assert ratio <= 1.0, (what, "h", i, ratio)
            worst = max(worst, ratio)
    ref = pref.pick(xh.double().numpy(), head.double().numpy(), None, [w.double().numpy() for w in tabs], cut, targets,
                    h=[h.double().numpy() for h in own_h])
    tol = _band_tols(geo, wdtype, xh, head, tabs, ref, own_h)
    token, logp = got["token"].cpu().numpy(), got["logp"].cpu().numpy().astype(np.float64)
    assert ((token >= 0) & (token < V)).all(), what
    for b in range(n + 1):
        lse, bv, bi = (got[k][b].cpu().numpy() for k in ("lse", "best_v", "best_i"))
        Vb = c0 if b == 0 else cut[b] - cut[b - 1]
        rows = ref["head_rows"][:, :c0] if b == 0 else ref["tail_rows"][b - 1]
        assert ((bi >= 0) & (bi < Vb)).all(), (what, b)
        for name, err in (("lse", np.abs(lse - ref["lse"][b])), ("best", np.abs(bv - ref["best"][b])),
                          ("best index", ref["best"][b] - rows[np.arange(M), bi])):
            assert (err <= tol[b]).all(), (what, name, b, float((err / tol[b]).max()))
            worst = max(worst, float((err / tol[b]).max()))
    cls = got["cls"].cpu().numpy()
    err = np.abs(cls - ref["head_rows"][:, c0:]) / tol[0][:, None]
    assert (err <= 1.0).all(), (what, "class logits", float(err.max()))
    band = np.array([aref.band_of(int(v), cut) for v in range(V)])           # -1: a word
    tail_tol = np.stack(tol[1:], 1)                                          # [M, n]

    def score_tol(tok):                                                      # of the scores s(tok[m]), summed over their bands
        b = band[tok]
        return tol[0] + np.where(b >= 0, tail_tol[np.arange(M), np.maximum(b, 0)], 0.0)
    if targets is None:
        want, allowed = ref["joint"][np.arange(M), token], score_tol(token)
    else:
        inside = (targets >= 0) & (targets < V)
        assert np.isnan(logp[~inside]).all() and not np.isnan(logp[inside]).any(), (what, "a target outside [0, V) scores NaN")
        want, allowed = ref["logp"], score_tol(np.where(inside, targets, 0))
        logp, want, allowed = logp[inside], want[inside], allowed[inside]
    err = np.abs(logp - want) / allowed
    assert (err <= 1.0).all(), (what, "logp", float(err.max()))
    worst = max(worst, float(err.max()) if err.size else 0.0)
    # the token: the fp64 argmax where the top-two gap exceeds twice the row's tolerance, else within it of the best
    row_tol = tol[0] + tail_tol.max(1)
    want_tok, gap, decided = pref.decided(ref["joint"], row_tol)
    assert (token[decided] == want_tok[decided]).all(), (what, "token")
    near = ~decided
    best = ref["joint"].max(1)
    assert (best[near] - ref["joint"][np.arange(M), token][near] <= 2.0 * row_tol[near]).all(), (what, "near-tie token")
    assert int(near.sum()) <= M // 16, (what, "near-tie rows", int(near.sum()))
    return worst, int(near.sum())


# ---- P1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_p1_seeds_have_no_near_tie_on_the_host(name, wdtype):
    """(No GPU.)  SEEDS: with h_i rounded from fp64 no row's top-two gap is within twice its tolerance."""
    geo = GEOMETRIES[name]
    x32, head, projs, tabs = _operands(name, wdtype)
    xh = x32.to(wdtype)

    def round16(h):
        return torch.from_numpy(h).to(wdtype).double().numpy()
    ref = pref.pick(xh.double().numpy(), head.double().numpy(), [p.double().numpy() for p in projs],
                    [w.double().numpy() for w in tabs], geo["cutoffs"], None, round16=round16)
    own_h = [torch.from_numpy(h).to(wdtype) for h in ref["h"]]
    tol = _band_tols(geo, wdtype, xh, head, tabs, ref, own_h)
    row_tol = tol[0] + np.stack(tol[1:], 1).max(1)
    _, gap, decided = pref.decided(ref["joint"], row_tol)
    assert decided.all(), (name, wdtype, SEEDS[name], float((gap / row_tol).min()))
    bands = {aref.band_of(int(t), geo["cutoffs"]) for t in ref["token"]}
    assert len(bands) >= 2, "the winners lie in more than one band"


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_p1_fp64_on_the_kernels_own_operands(name, M, wdtype):
    geo = GEOMETRIES[name]
    x32, head, projs, tabs = _operands(name, wdtype)
    x32 = x32[:M]
    dev = _device(head, projs, tabs)
    xh = x32.to(wdtype)
    worst, near = 0.0, 0
    for x_f32 in (True, False):
        xbuf = tvs._xbuf(x32, wdtype, x_f32)
        for t in (None, _targets(geo["cutoffs"], M, 3)):
            got = _pick(geo, M, xbuf, dev, None if t is None else torch.from_numpy(t).cuda())
            w, k = _check_p1(geo, wdtype, xh, head, projs, tabs, got, t, (name, M, wdtype, x_f32, t is not None))
            worst, near = max(worst, w), max(near, k)
            if t is not None:                                        # tlogit: written where the target lies in the band
                cut = geo["cutoffs"]
                for b in range(len(cut)):
                    lo, hi = (0, cut[0]) if b == 0 else (cut[b - 1], cut[b])
                    inside = torch.from_numpy((t >= lo) & (t < hi))
                    raw = got["tlogit"][b].cpu()
                    assert (raw[~inside].view(torch.int32) == -1).all(), "a row whose target is elsewhere keeps the fill"
                    assert torch.isfinite(raw[inside]).all()
    print(name, M, wdtype, "largest error / tolerance %.4f, near-tie rows %d" % (worst, near))


# ---- P2 ------------------------------------------------------------------------------------------------------------------------
def _plant_operands(name, wdtype, M):
    """x[:, 0] = 4 in every row; proj_i[0] = e_0, so that h_i[:, 0] = 4 exactly: a table row 8 e_0 has the logit 32."""
    x32, head, projs, tabs = _operands(name, wdtype)
    x32 = x32[:M].clone()
    x32[:, 0] = 4.0
    projs = [p.clone() for p in projs]
    for p in projs:
        p[0] = 0.0
        p[0, 0] = 1.0
    return x32, head.clone(), projs, [w.clone() for w in tabs]


def _band_span(geo, b):
    """columns of one workgroup of band b's pass"""
    return SPAN if b and geo["dims"][b - 1] <= MAX_K else 16


def _plant_columns(geo, b):
    cut = geo["cutoffs"]
    Vb = cut[0] if b == 0 else cut[b] - cut[b - 1]
    span = _band_span(geo, b)
    return sorted({u for u in (0, 15, 16, span - 1, span, Vb - 1) if u < Vb})


def _planted(geo, b, cols, head, tabs):
    """CPU copies with the row 8 e_0 at `cols` of band b (and at the band's class row)."""
    head, tabs = head.clone(), [w.clone() for w in tabs]
    c0 = geo["cutoffs"][0]
    row = torch.zeros(head.shape[1] if b == 0 else tabs[b - 1].shape[1], dtype=head.dtype)
    row[0] = 8.0
    for u in cols:
        (head if b == 0 else tabs[b - 1])[u] = row
    if b:
        head[c0 + b - 1] = 0.0
        head[c0 + b - 1, 0] = 8.0
    return head, tabs


def _plant_margin(geo, xh, head, tabs, h, cols_global):
    """fp64: min over rows of (the planted tokens' score - the best other score)."""
    ref = pref.pick(xh.double().numpy(), head.double().numpy(), None, [w.double().numpy() for w in tabs], geo["cutoffs"],
                    None, h=[v.double().numpy() for v in h])
    j = ref["joint"].copy()
    mine = j[:, cols_global].min(1)
    j[:, cols_global] = -np.inf
    return float((mine - j.max(1)).min())


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_p2_planted_winners_and_duplicates(name, wdtype):
    geo, M = GEOMETRIES[name], 17
    cut, dims = geo["cutoffs"], geo["dims"]
    x32, head, projs, tabs = _plant_operands(name, wdtype, M)
    xh = x32.to(wdtype)
    xbuf = tvs._xbuf(x32, wdtype, True)
    seen = 0
    for b in range(len(dims) + 1):
        base = 0 if b == 0 else cut[b - 1]
        span = _band_span(geo, b)
        Vb = cut[b] - base
        cases = [[u] for u in _plant_columns(geo, b)]
        # duplicates: within a tile, across a wave's tiles (the head and the K-split tails: across workgroups), across spans
        cases += [pair for pair in ([1, 14], [3, 21], [5, span + 7], [span - 1, span], [0, Vb - 1])
                  if pair[1] < Vb and pair[0] < pair[1]]
        for cols in cases:
            hd, tb = _planted(geo, b, cols, head, tabs)
            got = _pick(geo, M, xbuf, _device(hd, projs, tb))
            own = [v.cpu() for v in got["h"]]                          # the margin is taken on the kernel's own h_i
            assert all((v[:, 0] == 4.0).all() for v in own)
            margin = _plant_margin(geo, xh, hd, tb, own, [base + u for u in cols])
            assert margin >= 1.0, (name, b, cols, margin)
            assert (got["token"] == base + cols[0]).all(), (name, wdtype, b, cols, got["token"].tolist())
            assert (got["best_i"][b] == cols[0]).all(), (name, wdtype, b, cols)
            seen += 1
    print(name, wdtype, "%d planted cases" % seen)
    if name == "B":
        assert [SPAN - 1] in [[u] for u in _plant_columns(geo, 1)] and 2 * SPAN < cut[1] - cut[0]


# ---- P3 ------------------------------------------------------------------------------------------------------------------------
OUT_KEYS = ("token", "logp")


def _same(a, b, rows=slice(None)):
    ok = all(_bits(a[k][rows], b[k]) for k in OUT_KEYS) and _bits(a["cls"][rows], b["cls"])
    for k in ("best_v", "best_i", "lse"):
        ok = ok and all(_bits(x[rows], y) for x, y in zip(a[k], b[k]))
    return ok and all(_bits(x[rows], y) for x, y in zip(a["h"], b["h"]))


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_p3_a_rows_results_depend_on_that_row_alone(name, wdtype):
    geo, M = GEOMETRIES[name], 64
    x32, head, projs, tabs = _operands(name, wdtype)
    dev = _device(head, projs, tabs)
    t = _targets(geo["cutoffs"], M, 4)
    tg = torch.from_numpy(t).cuda()
    x16 = x32.to(wdtype)
    for targets in (None, tg):
        whole = _pick(geo, M, tvs._xbuf(x32, wdtype, True), dev, targets)
        assert _same(_pick(geo, M, tvs._xbuf(x32, wdtype, True), dev, targets), whole), "two calls"
        assert _same(_pick(geo, M, tvs._xbuf(x16.float(), wdtype, True), dev, targets), whole), "fp32 x holding 16-bit values"
        assert _same(_pick(geo, M, tvs._xbuf(x32, wdtype, False), dev, targets), whole), "16-bit x"
        assert _same(_pick(geo, M, tvs._xbuf(x32, wdtype, True), _device(head, projs, tabs, joined=False), targets), whole), \
            "separate projections"
        for m in range(M):
            one = _pick(geo, 1, tvs._xbuf(x32[m:m + 1], wdtype, m % 2 == 0), dev, None if targets is None else tg[m:m + 1])
            assert _same(whole, one, slice(m, m + 1)), (name, wdtype, m, "M = 64 against M = 1")
        for M2 in (17, 33):                                          # the two-row-tile instance; a four-row-tile one in part
            part = _pick(geo, M2, tvs._xbuf(x32[:M2], wdtype, True), dev, None if targets is None else tg[:M2])
            assert _same(whole, part, slice(0, M2)), (name, wdtype, M2)
        # a NaN row beside finite rows
        bad = x32.clone()
        bad[3] = float("nan")
        got = _pick(geo, M, tvs._xbuf(bad, wdtype, True), dev, targets)
        keep = [m for m in range(M) if m != 3]
        assert all(_bits(got[k][keep], whole[k][keep]) for k in OUT_KEYS), "a NaN row changes no other row's bits"
        assert 0 <= got["token"][3].item() < geo["cutoffs"][-1] and torch.isnan(got["logp"][3])


# ---- P4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_p4_a_captured_call_follows_rewritten_rows_and_targets(name):
    from efficient_attention import _native as nv
    geo, M, wdtype = GEOMETRIES[name], 17, torch.bfloat16
    cut, dims = geo["cutoffs"], geo["dims"]
    x32, head, projs, tabs = _operands(name, wdtype)
    dev = _device(head, projs, tabs)
    first_x, second_x = x32[:M], x32[M:2 * M]
    first_t, second_t = (torch.from_numpy(_targets(cut, M, s)).cuda() for s in (5, 6))
    want = [_pick(geo, M, tvs._xbuf(x, wdtype, True), dev, t) for x, t in ((first_x, first_t), (second_x, second_t))]
    assert not _bits(want[0]["logp"], want[1]["logp"])
    nbytes = nv.lib().ea_adaptive_pick_ws(M, len(dims), nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims))
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    token = torch.zeros(M, dtype=torch.long, device="cuda")
    logp = torch.zeros(M, dtype=torch.float32, device="cuda")
    xbuf, targets = tvs._xbuf(first_x, wdtype, True), first_t.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(geo, M, xbuf, dev, targets, ws, token, logp)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(token, want[0]["token"]) and _bits(logp, want[0]["logp"])
    xbuf[:M, :geo["C"]] = second_x.cuda()
    targets.copy_(second_t)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(token, want[1]["token"]) and _bits(logp, want[1]["logp"])


# ---- P5 ------------------------------------------------------------------------------------------------------------------------
def _fixture():
    import test_gpu_adaptive_score as tas
    return tas._fixture_stack()


def _state(m, B, T, dtype=torch.bfloat16, **opt):
    return m.init_adaptive_decoding(m.init_decoding(B, T, dtype, "cuda", **opt))


def _check_rows(m, st, rows, tokens, logp, targets, what):
    """rows [T, B, C] as the stack handed them to the pick; tokens / logp [T, B] what it returned: the raw call's bits, and P1."""
    tb = st.adaptive.tables
    geo = dict(C=128, cutoffs=tb.cutoff, dims=tb.dims)
    x2 = rows.reshape(-1, 128).float().contiguous()
    M = x2.shape[0]
    assert M <= 64
    tg = None if targets is None else targets.reshape(-1).contiguous()
    raw = _pick(geo, M, x2, (tb.head, tb.proj, tb.tables), tg)
    assert torch.equal(raw["token"], tokens.reshape(-1)) and _bits(raw["logp"], logp.reshape(-1).contiguous()), what
    return _check_p1(geo, tb.dtype, x2.to(tb.dtype).cpu(), tb.head.cpu(), [p.cpu() for p in tb.proj],
                     [w.cpu() for w in tb.tables], raw, None if tg is None else tg.cpu().numpy(), what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "static", "per_sequence_ragged"])
def test_p5_generate_on_the_adaptive_pick_replayed_equals_eager(case):
    dtype = torch.bfloat16
    m, tokens = _fixture()
    B = tokens.shape[0]
    prompt = tokens[:, :9].clone()
    opt = dict(rolling=case != "static")
    if case == "per_sequence_ragged":
        opt["per_sequence"] = True
        prompt[1, 4:] = m.pad_idx
    n_new = 6
    out = {}
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for graph in (False, True):
            st = _state(m, B, 9 + n_new, **opt)
            out[graph] = m.generate(prompt, n_new, st, graph=graph, return_rows=True, return_logprobs=True) + (st,)
            plain = m.generate(prompt, n_new, _state(m, B, 9 + n_new, **opt), graph=graph)
            assert torch.equal(plain, out[graph][0]), "the tokens of the same call without the keywords"
    (tok_e, rows_e, lp_e, _), (tok_g, rows_g, lp_g, st) = out[False], out[True]
    assert tuple(tok_g.shape) == (B, n_new) and tok_g.dtype == torch.long and tuple(lp_g.shape) == (B, n_new)
    assert lp_g.dtype == torch.float32 and tuple(rows_g.shape) == (n_new, B, 128)
    assert torch.equal(tok_g, tok_e) and _bits(rows_g, rows_e) and _bits(lp_g, lp_e)
    assert (lp_g < 0).all() and int(tok_g.min()) >= 0 and int(tok_g.max()) < 333
    worst, near = _check_rows(m, st, rows_g, tok_g.t().contiguous(), lp_g.t().contiguous(), None, case)
    print(case, "tokens", tok_g.tolist(), "largest error / tolerance %.4f, near-tie rows %d" % (worst, near))


@pytest.mark.gpu
def test_p5_next_tokens_and_token_logprobs_run_on_the_kernel(monkeypatch):
    dtype = torch.bfloat16
    m, tokens = _fixture()
    B, T = tokens.shape
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _state(m, B, T)
        rows = m.decode(tokens.t()[:T - 1].contiguous(), st)                 # [T - 1, B, C]: more than 64 rows run in pieces
        piece = rows[:20]
        import test_gpu_adaptive_score as tas
        with monkeypatch.context() as mp:
            for mod, fname in tas._BANNED:
                def banned(*a, _name=fname, **k):
                    raise AssertionError("%s reached in the adaptive pick" % _name)
                mp.setattr(mod, fname, banned)
            tok = m.next_tokens(piece, st)
            tok2, lp = m.token_logprobs(piece, st)
            targets = tokens.t()[1:21].contiguous()
            tok3, lpt = m.token_logprobs(piece, st, targets=targets)
            out = torch.empty_like(tok)
            assert m.next_tokens(piece, st, out=out) is out
            torch.cuda.synchronize()
        assert torch.equal(tok, tok2) and torch.equal(tok, tok3) and torch.equal(tok, out) and tuple(tok.shape) == (20, B)
        _check_rows(m, st, piece, tok, lp, None, "token_logprobs")
        _check_rows(m, st, piece, tok3, lpt, targets, "token_logprobs with targets")
        # more than 64 rows: pieces of 64, the same bits as the rows alone
        big = torch.cat([rows, rows.flip(0)], 0).contiguous()
        n, cut = big.shape[0], 64 // B
        assert n * B > 64 and 64 % B == 0
        big_tok, big_lp = m.token_logprobs(big, st)
        assert torch.equal(big_tok[:20], tok) and _bits(big_lp[:20].contiguous(), lp)
        tail_tok, tail_lp = m.token_logprobs(big[cut:].contiguous(), st)
        assert torch.equal(big_tok[cut:], tail_tok) and _bits(big_lp[cut:].contiguous(), tail_lp)
        # score: one decode and token_logprobs with the targets; entries whose target is pad_idx are 0
        got = m.score(tokens, _state(m, B, T))
        all_t = tokens[:, 1:].t().contiguous()
        _, want = m.token_logprobs(rows, st, targets=all_t)
        pad = tokens[:, 1:].eq(m.pad_idx)
        assert tuple(got.shape) == (B, T - 1) and (got[pad] == 0).all() and _bits(got[~pad], want.t()[~pad])
        assert _bits(m.score(tokens), got), "the default state of an adaptive stack is an adaptive pick"


@pytest.mark.gpu
def test_p5_refresh_and_nbytes():
    dtype = torch.bfloat16
    m, tokens = _fixture()
    B = tokens.shape[0]
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _state(m, B, 16)
        ad = st.adaptive
        bare = m.decoding_state_nbytes(m.init_decoding(B, 16, dtype, "cuda"))
        assert ad.ws.numel() == pref.ws_layout(64, ad.tables.cutoff, ad.tables.dims)["total"]
        assert m.decoding_state_nbytes(st) == bare + ad.tables.nbytes() + ad.ws.numel() + 4 * B
        rows = m.decode(tokens.t()[:8].contiguous(), st)[-1:]
        before = m.token_logprobs(rows, st)
        ptrs = [t.data_ptr() for t in [ad.tables.head] + ad.tables.proj + ad.tables.tables]
        w = m.adaptive_softmax.head.class_proj.weight
        saved = w.detach().clone()
        try:
            w.add_(0.5)
            stale = m.token_logprobs(rows, st)
            assert _bits(stale[1], before[1]), "the state holds its own copy"
            assert m.refresh_decoding_weights(st) is st
            assert ptrs == [t.data_ptr() for t in [ad.tables.head] + ad.tables.proj + ad.tables.tables]
            fresh = m.token_logprobs(rows, st)
            assert not _bits(fresh[1], before[1])
            _check_rows(m, st, rows, fresh[0], fresh[1], None, "refreshed")
        finally:
            w.copy_(saved)
