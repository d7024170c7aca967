"""-m gpu: adaptive-softmax scoring (csrc/ea_adaptive_score.hip, C ABI 33: ea_adaptive_route, ea_vocab_score_rows,
ea_adaptive_score) and DecoderStack(adaptive=...).rows_logprobs / evaluate / decode.  bf16 and fp16 tables, x in fp32 and in
the table's type, in the framed buffers of tests/test_gpu_vocab_score.py; BM, BN, SL are the library's tile widths.

 G1 identity      ea_vocab_score_rows with rows = count = NULL has ea_vocab_score's bits (token, top, lse, logp, stored logits),
                  and ea_vocab_score has the bits it had before the tile loop became a template (recorded checksums).
 G2 gather/count  x of 2 BM + 3 rows, K = 256, V = BN + 24; a reversed list, a strided list, a list with repeats; count on the
                  device in {0, 1, BM, BM + 1, M}: position j has the bits of the identity call's row rows[j]; positions >= count
                  and every guard are untouched; list entries >= count name an extra VALID row of x that holds NaN.
 G3 route         M in {1, 1000, 9216 + 37}: head_target, count, rows[i][:count] equal the host reference; rows[i][count:] keeps
                  its fill; two calls give the same bits.
 G4 composite     same-operand fp64 checks on the kernel's own h_i (read from the workspace), two geometries, target sets that
                  name every column of each band's last column block, an empty band, all rows in one tail, targets -1 and V.
 G5 independence  halves, reversal, a repeat, and a captured call replayed on rewritten targets.
 G6 stack         the fixture's stack: evaluate == rows_logprobs on the full path's rows, under a ban of framework ops, against
                  fp64; decode, eager and captured, against the full forward; generate on the slow `logits` route; hold_vocab
                  raises."""
import ctypes
import functools
import hashlib
import warnings

import numpy as np
import pytest
import torch

import test_gpu_decoder_vocab as tv
import test_gpu_vocab_score as tvs
import adaptive_score_reference as aref
import decoder_logprob_reference as lref
import decoder_vocab_operands as ops
import vocab_score_reference as vref
from ceva_decoding import F32_TOL, _ctx, _err, _skip_f32
from test_adaptive_cpu import _small_state, adaptive_ws_layout, edge_targets

BM, BN, SL = vref.constants()
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
_bits = tv._bits
KEYS = ("token", "top", "lse", "logp")


# ---- ea_vocab_score_rows -------------------------------------------------------------------------------------------------------
def _rows_call(M, K, V, xbuf, wbuf, logits=None, targets=None, rows=None, count=None, base=0, logits_only=0):
    """-> the WHOLE output buffers (M positions and one guard element each), filled with 7 / -7 before the call."""
    from efficient_attention import _native as nv
    nbytes = nv.lib().ea_vocab_score_rows_ws(M, V)
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    out = dict(token=torch.full((M + 1,), -7, dtype=torch.long, device="cuda"),
               top=torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda"),
               lse=torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda"),
               logp=torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda"))
    nv.call("ea_vocab_score_rows", M, K, V, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(wbuf), nv.io_dtype(wbuf),
            nv.ptr(targets), nv.ptr(logits), 0 if logits is None else tv._code(logits), 0 if logits is None else logits.stride(0),
            nv.ptr(ws), nbytes, nv.ptr(out["token"]), nv.ptr(out["top"]), nv.ptr(out["lse"]), nv.ptr(out["logp"]), nv.ptr(rows),
            nv.ptr(count), base, logits_only, nv.stream())
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xFF).all()
    assert out["token"][M].item() == -7 and all(out[k][M].item() == 7.0 for k in KEYS[1:])
    if logits is not None:
        assert (logits[M:] == 7.0).all() and (logits[:, V:] == 7.0).all()
    return out


# checksums of ea_vocab_score's (token, top, lse, logp, fp32 logits) on tests/test_gpu_vocab_score.py's plain operands, recorded
# from the library BEFORE its tile loop became a template (the parent commit's build, on an MI355X); x in fp32 and in the
# table's type give the same bits: the fp32 rows are rounded as they are loaded
PARENT = {((65, 32, 16), torch.bfloat16): "54652e76ca9763dc", ((65, 32, 16), torch.float16): "93ee207f30ed5eb1",
          ((BM + 1, 288, 40), torch.bfloat16): "cfba55e108b746e8", ((BM + 1, 288, 40), torch.float16): "a0a157e689e47402"}


def _checksum(got, logits, M, V):
    h = hashlib.sha256()
    for t in (got["token"], got["top"], got["lse"], got["logp"], logits[:M, :V]):
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", [(65, 32, 16), (BM + 1, 288, 40)], ids=tv._ids([(65, 32, 16), (BM + 1, 288, 40)]))
def test_g1_identity_rows_have_the_bits_of_ea_vocab_score(shape, wdtype):
    M, K, V = shape
    if BM == 128:                                        # (the checksums belong to the shapes of the recorded tile)
        assert (shape, wdtype) in PARENT
    for x_f32 in (True, False):
        xbuf, wbuf, logits, got = tvs._case(shape, wdtype, x_f32)
        if (shape, wdtype) in PARENT:
            assert _checksum(got, logits, M, V) == PARENT[(shape, wdtype)], (shape, wdtype, x_f32)
        for ldtype in (torch.float32, wdtype):
            mine_logits = tv._logit_buffer(M, V, ldtype)
            mine = _rows_call(M, K, V, xbuf, wbuf, mine_logits)
            assert all(_bits(mine[k][:M], got[k]) for k in KEYS), (shape, wdtype, x_f32)
            assert _bits(mine_logits[:M, :V], logits[:M, :V].to(ldtype))
        tg = torch.tensor([(7 * m + 3) % V for m in range(M)], device="cuda")
        want = tvs._score(M, K, V, xbuf, wbuf, None, targets=tg.tolist())
        mine = _rows_call(M, K, V, xbuf, wbuf, None, targets=tg)
        assert all(_bits(mine[k][:M], want[k]) for k in KEYS), (shape, wdtype, x_f32, "targets")


G2_SHAPE = (2 * BM + 3, 256, BN + 24)


def _g2_lists(M):
    rev = list(range(M - 1, -1, -1))
    stride = 3 if M % 3 else 5
    strided = [(stride * j) % M for j in range(M)]       # (count < M of them: a strided subset)
    repeats = [(j // 2 * 7) % M for j in range(M)]
    return dict(reversed=rev, strided=strided, repeats=repeats)


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_g2_gathered_rows_and_a_device_count(wdtype):
    M, K, V = G2_SHAPE
    x32, w = ops.operands(G2_SHAPE, wdtype, 0)
    wbuf = tv._table(w.cuda())
    for x_f32 in (True, False):
        xbuf = tvs._xbuf(x32, wdtype, x_f32)              # [M + 1, K + 8]: row M is a VALID row of NaN
        assert torch.isnan(xbuf[M]).all()
        tg = torch.tensor([(7 * m + 3) % V for m in range(M)] + [0], device="cuda")
        base_logits = tv._logit_buffer(M, V, torch.float32)
        base = _rows_call(M, K, V, xbuf, wbuf, base_logits, targets=tg)
        assert torch.isfinite(base["lse"][:M]).all()
        shifted = _rows_call(M, K, V, xbuf, wbuf, None, targets=tg + 5, base=5)
        assert all(_bits(shifted[k], base[k]) for k in KEYS)
        for name, order in _g2_lists(M).items():
            for count in (0, 1, BM, BM + 1, M):
                what = (wdtype, x_f32, name, count)
                rows = torch.tensor(order[:count] + [M] * (M - count), dtype=torch.int32, device="cuda")
                cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
                logits = tv._logit_buffer(M, V, torch.float32)
                got = _rows_call(M, K, V, xbuf, wbuf, logits, targets=tg, rows=rows, count=cnt)
                at = torch.tensor(order[:count], dtype=torch.long, device="cuda")
                for k in KEYS:
                    assert _bits(got[k][:count], base[k][at]), (what, k)
                    fill = -7 if k == "token" else 7.0
                    assert (got[k][count:] == fill).all(), (what, k, "positions >= count were written")
                assert _bits(logits[:count, :V], base_logits[at, :V]) and (logits[count:] == 7.0).all(), what
        # logits_only: the 16-bit store alone; nothing else is written
        order, count = _g2_lists(M)["reversed"], BM + 1
        rows = torch.tensor(order[:count] + [M] * (M - count), dtype=torch.int32, device="cuda")
        cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
        l16 = tv._logit_buffer(M, V, wdtype)
        got = _rows_call(M, K, V, xbuf, wbuf, l16, rows=rows, count=cnt, logits_only=1)
        at = torch.tensor(order[:count], dtype=torch.long, device="cuda")
        assert _bits(l16[:count, :V], base_logits[at, :V].to(wdtype)) and (l16[count:] == 7.0).all()
        assert (got["token"] == -7).all() and all((got[k] == 7.0).all() for k in KEYS[1:])


# ---- ea_adaptive_route ---------------------------------------------------------------------------------------------------------
def _route(targets, cutoffs):
    from efficient_attention import _native as nv
    M, n = targets.numel(), len(cutoffs) - 1
    head = torch.full((M + 1,), -9, dtype=torch.long, device="cuda")
    rows = torch.full((n * M + 1,), -5, dtype=torch.int32, device="cuda")
    count = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    nv.call("ea_adaptive_route", M, n, nv.host_array(ctypes.c_int64, cutoffs), nv.ptr(targets), nv.ptr(head), nv.ptr(rows),
            nv.ptr(count), nv.stream())
    torch.cuda.synchronize()
    assert head[M].item() == -9 and rows[n * M].item() == -5 and count[n].item() == -3
    return head[:M], rows[:n * M].view(n, M), count[:n]


def _route_targets(M, cutoffs, seed):
    g = np.random.RandomState(seed)
    V = cutoffs[-1]
    t = g.randint(-2, V + 2, size=M).astype(np.int64)
    edges = edge_targets(cutoffs)
    k = min(M, len(edges))
    t[:k] = edges[:k]
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("cutoffs", [[96, 200, 333], [20000, 60000, 267744], [5, 6, 7, 8, 9]], ids=lambda c: "n%d" % (len(c) - 1))
@pytest.mark.parametrize("M", [1, 1000, 9216 + 37])
def test_g3_route_equals_the_host_reference(M, cutoffs):
    n = len(cutoffs) - 1
    cases = [_route_targets(M, cutoffs, 11)]
    if M > 1:
        t = _route_targets(M, cutoffs, 12)
        cases.append(np.where((t >= cutoffs[0]) & (t < cutoffs[1]), 0, t))                      # tail 0 empty
        cases.append(np.full(M, cutoffs[-1] - 1, dtype=np.int64))                              # all rows in the last tail
    for t in cases:
        want_head, want_rows, want_count = aref.route(t, cutoffs)
        tg = torch.from_numpy(t).cuda()
        head, rows, count = _route(tg, cutoffs)
        assert head.cpu().numpy().tolist() == want_head.tolist()
        assert count.cpu().numpy().tolist() == want_count.tolist()
        for i in range(n):
            c = int(want_count[i])
            assert rows[i, :c].cpu().numpy().tolist() == want_rows[i].tolist(), i
            assert (rows[i, c:] == -5).all(), i
        again = _route(tg, cutoffs)
        assert torch.equal(again[0], head) and torch.equal(again[1], rows) and torch.equal(again[2], count)


# ---- ea_adaptive_score ---------------------------------------------------------------------------------------------------------
GEOMETRIES = {"small": dict(C=128, cutoffs=[96, 200, 333], dims=[64, 32]),
              "sliced": dict(C=128, cutoffs=[40, 2140, 2190], dims=[64, 32])}
G4_M = 300


@functools.lru_cache(maxsize=None)
def _operands(name, wdtype, M=G4_M):
    """CPU: x32 [M, C], and in `wdtype` the head [c0 + n, C], the projections [d_i, C], the tables [V_i, d_i]."""
    geo = GEOMETRIES[name]
    C, cut, dims = geo["C"], geo["cutoffs"], geo["dims"]
    g = torch.Generator().manual_seed(1000 * len(name) + M + (wdtype == torch.float16))
    x32 = torch.randn(M, C, generator=g)
    head = (torch.randn(cut[0] + len(dims), C, generator=g) / C ** 0.5).to(wdtype)
    projs = tuple((torch.randn(d, C, generator=g) / C ** 0.5).to(wdtype) for d in dims)
    tabs = tuple((torch.randn(cut[i + 1] - cut[i], d, generator=g) * (2.0 / d ** 0.5)).to(wdtype) for i, d in enumerate(dims))
    return x32, head, projs, tabs


def _spread(columns, k):
    """k entries that name every one of `columns` as often as k allows."""
    return [columns[i % len(columns)] for i in range(k)]


def _target_sets(name, M=G4_M):
    """name -> {set name: int64 [M]}: one tail below BM rows and the other above; between the sets every column of each band's
    last column block is a target; one band empty (with targets -1 and V); all rows in one tail."""
    cut = GEOMETRIES[name]["cutoffs"]
    c0, c1, V = cut
    perm = np.random.RandomState(5).permutation(M)
    sets = {}

    def lay(head, tail0, tail1):
        t = np.array(head + tail0 + tail1, dtype=np.int64)
        assert t.size == M
        return t[perm]
    if name == "small":
        n0, n1 = c1 - c0, V - c1                          # 104, 133
        sets["tails"] = lay(list(range(M - n0 - 150)), list(range(c0, c1)), _spread(list(range(c1, V)), 150))
        sets["head"] = lay(list(range(c0)), _spread(list(range(c0, c1)), 60), _spread(list(range(c1, V)), M - c0 - 60))
    else:
        first = (c1 - c0 - 1) // BN * BN                  # the first column of tail 0's last column block
        last_block = list(range(c0 + first, c1))
        assert first >= SL and len(last_block) < BN
        t0 = last_block + [c0, c0 + SL - 1, c0 + SL, c0 + first - 1, c0 + BN - 1, c0 + BN]
        t0 = t0 + _spread(list(range(c0 + 1, c1, 37)), 158 - len(t0))
        sets["tails"] = lay(list(range(c0)) + [0, c0 - 1], t0, _spread(list(range(c1, V)), M - c0 - 2 - 158))
    full = sets["tails"].copy()
    empty = np.where((full >= c0) & (full < c1), full % c0, full)
    empty[3], empty[M // 2] = -1, V
    sets["tail 0 empty"] = empty
    sets["one tail"] = np.array(_spread(list(range(c1, V)), M), dtype=np.int64)
    counts = aref.route(sets["tails"], cut)[2]
    assert min(counts) < BM < max(counts), counts
    return sets


def _adaptive(geo, xbuf, head, projs, tabs, targets, token_head=True):
    """One ea_adaptive_score call on fresh buffers -> dict(logp [M], token_head, and the workspace's parts: head_target, rows
    [n, M], count [n], logp_head, h[i] [M, d_i], logp_tail[i] [M])."""
    from efficient_attention import _native as nv
    M, C, cut, dims = targets.numel(), geo["C"], geo["cutoffs"], geo["dims"]
    n = len(dims)
    hc, hd = nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims)
    nbytes = nv.lib().ea_adaptive_score_ws(M, n, hc, hd)
    lay = adaptive_ws_layout(M, cut, dims, nv.lib().ea_vocab_score_ws)
    assert nbytes == lay["total"]
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    logp = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    tok = torch.full((M + 1,), -7, dtype=torch.long, device="cuda") if token_head else None
    nv.call("ea_adaptive_score", M, C, n, hc, hd, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(targets), nv.ptr(head),
            nv.io_dtype(head), nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in projs]),
            nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tabs]), nv.ptr(ws), nbytes, nv.ptr(logp), nv.ptr(tok),
            nv.stream())
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xFF).all() and logp[M].item() == 7.0 and (tok is None or tok[M].item() == -7)

    def part(name, dtype, count):
        size = torch.empty((), dtype=dtype).element_size()
        return ws[lay[name]:lay[name] + size * count].view(dtype)
    out = dict(logp=logp[:M], token_head=None if tok is None else tok[:M], head_target=part("head_target", torch.long, M),
               rows=part("rows", torch.int32, n * M).view(n, M), count=part("count", torch.int32, n),
               logp_head=part("logp_head", torch.float32, M), h=[], logp_tail=[])
    for i, d in enumerate(dims):
        out["h"].append(part("h%d" % i, head.dtype, M * d).view(M, d))
        out["logp_tail"].append(part("logp%d" % i, torch.float32, M))
    return out


def _check_composite(geo, wdtype, x_f32, x32, head, projs, tabs, t, what):
    """G4's checks on one call -> the largest error / tolerance of (h, head logp, tail logp, final logp)."""
    M, cut, dims = t.size, geo["cutoffs"], geo["dims"]
    n = len(dims)
    xbuf = tvs._xbuf(x32, wdtype, x_f32)
    dev = [head.cuda(), [p.cuda() for p in projs], [w.cuda() for w in tabs]]
    got = _adaptive(geo, xbuf, dev[0], dev[1], dev[2], torch.from_numpy(t).cuda())
    want_head, want_rows, want_count = aref.route(t, cut)
    assert got["head_target"].cpu().numpy().tolist() == want_head.tolist(), what
    assert got["count"].cpu().numpy().tolist() == want_count.tolist(), what
    xh = x32.to(wdtype)
    own_h, worst = [], [0.0, 0.0, 0.0, 0.0]
    for i in range(n):
        c = int(want_count[i])
        assert got["rows"][i, :c].cpu().numpy().tolist() == want_rows[i].tolist(), (what, i)
        hi = got["h"][i][:c].cpu()
        own_h.append(hi.double().numpy())
        if c:
            xr = xh[torch.from_numpy(want_rows[i]).long()]
            h64 = (xr.double() @ projs[i].double().t()).numpy()
            allowed = aref.tol_h(ops.bound(xr, projs[i]).numpy()[:, None], h64, wdtype)
            ratio = float((np.abs(own_h[i] - h64) / allowed).max())
            assert ratio <= 1.0, (what, "h", i, ratio)
            worst[0] = max(worst[0], ratio)
    ref = aref.score(xh.double().numpy(), head.double().numpy(), None, [w.double().numpy() for w in tabs], cut, t, h=own_h)
    bound_head = ops.bound(xh, head).numpy()
    bound_tail = [ops.bound(got["h"][i][:int(want_count[i])].cpu(), tabs[i]).numpy() if want_count[i] else None for i in range(n)]
    place = {int(m): (i, j) for i, r in enumerate(want_rows) for j, m in enumerate(r)}
    logp, logp_head = got["logp"].cpu().numpy(), got["logp_head"].cpu().numpy()
    logp_tail = [v.cpu().numpy() for v in got["logp_tail"]]
    for m in range(M):
        if want_head[m] < 0:
            assert np.isnan(logp[m]) and np.isnan(logp_head[m]), (what, m, "a target outside [0, V) scores NaN")
            continue
        row = ref["head_rows"][m]
        tol_head = aref.tol_logp(bound_head[m], row, lref.lse(row))
        err = abs(float(logp_head[m]) - ref["logp_head"][m])
        assert err <= tol_head, (what, m, "head", err, tol_head)
        worst[1] = max(worst[1], err / tol_head)
        total, mine = tol_head, np.float32(logp_head[m])
        if m in place:
            i, j = place[m]
            row = ref["tail_rows"][m]
            tol_tail = aref.tol_logp(bound_tail[i][j], row, lref.lse(row))
            err = abs(float(logp_tail[i][j]) - ref["logp_tail"][m])
            assert err <= tol_tail, (what, m, "tail", i, j, err, tol_tail)
            worst[2] = max(worst[2], err / tol_tail)
            total += tol_tail
            mine = np.float32(logp_head[m]) + np.float32(logp_tail[i][j])
        assert np.float32(logp[m]).tobytes() == np.float32(mine).tobytes(), (what, m, "the combine is one fp32 addition")
        err = abs(float(logp[m]) - ref["logp"][m])
        assert err <= total, (what, m, "final", err, total)
        worst[3] = max(worst[3], err / total)
    # the head's pick: the fp64 argmax wherever its top-two margin exceeds 2 bound (tests/test_gpu_vocab_score.py, 8)
    top2 = np.sort(ref["head_rows"], axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2.0 * bound_head
    assert decided.sum() >= M // 2, what
    assert (got["token_head"].cpu().numpy()[decided] == ref["head_rows"].argmax(1)[decided]).all(), what
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_g4_composite_against_fp64_on_the_kernels_own_operands(name, wdtype):
    geo = GEOMETRIES[name]
    x32, head, projs, tabs = _operands(name, wdtype)
    sets = _target_sets(name)
    seen = set()
    worst = [0.0] * 4
    for set_name, t in sets.items():
        seen.update(int(v) for v in t)
        for x_f32 in ((True, False) if set_name == "tails" else (True,)):
            w = _check_composite(geo, wdtype, x_f32, x32, head, projs, tabs, t, (name, wdtype, set_name, x_f32))
            worst = [max(a, b) for a, b in zip(worst, w)]
    cut = geo["cutoffs"]
    blocks = [range(0, cut[0])] + [range(cut[i] + (cut[i + 1] - cut[i] - 1) // BN * BN, cut[i + 1]) for i in range(2)]
    assert all(v in seen for b in blocks for v in b), "every column of each band's last column block is somebody's target"
    print(name, wdtype, "largest error / tolerance: h %.4f, head logp %.4f, tail logp %.4f, final logp %.4f" % tuple(worst))


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
def test_g5_a_rows_score_does_not_depend_on_the_call(wdtype):
    name = "sliced"
    geo = GEOMETRIES[name]
    M = G4_M
    x32, head, projs, tabs = _operands(name, wdtype)
    t = _target_sets(name)["tails"]
    dev = (head.cuda(), [p.cuda() for p in projs], [w.cuda() for w in tabs])
    for x_f32 in (True, False):
        def run(sel):
            xbuf = tvs._xbuf(x32[sel], wdtype, x_f32)
            return _adaptive(geo, xbuf, *dev, torch.from_numpy(t[sel.numpy()]).cuda())
        every = torch.arange(M)
        whole = run(every)
        again = run(every)
        assert _bits(again["logp"], whole["logp"]) and torch.equal(again["token_head"], whole["token_head"])
        lo, hi = run(every[:M // 2]), run(every[M // 2:])
        assert _bits(torch.cat([lo["logp"], hi["logp"]]), whole["logp"]), (wdtype, x_f32, "halves")
        assert torch.equal(torch.cat([lo["token_head"], hi["token_head"]]), whole["token_head"])
        back = run(every.flip(0))
        assert _bits(back["logp"].flip(0), whole["logp"]), (wdtype, x_f32, "reversed")


@pytest.mark.gpu
def test_g5_a_captured_call_follows_rewritten_targets():
    from efficient_attention import _native as nv
    name, wdtype = "small", torch.bfloat16
    geo = GEOMETRIES[name]
    M, C, cut, dims = G4_M, geo["C"], geo["cutoffs"], geo["dims"]
    x32, head, projs, tabs = _operands(name, wdtype)
    sets = _target_sets(name)
    head, projs, tabs = head.cuda(), [p.cuda() for p in projs], [w.cuda() for w in tabs]
    xbuf = tvs._xbuf(x32, wdtype, True)
    first, second = torch.from_numpy(sets["tails"]).cuda(), torch.from_numpy(sets["tail 0 empty"]).cuda()
    want_first = _adaptive(geo, xbuf, head, projs, tabs, first)["logp"].clone()      # (eager: also the warm-up)
    want_second = _adaptive(geo, xbuf, head, projs, tabs, second)["logp"].clone()
    assert not _bits(want_first, want_second)
    hc, hd = nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims)
    nbytes = nv.lib().ea_adaptive_score_ws(M, len(dims), hc, hd)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    logp = torch.zeros(M, dtype=torch.float32, device="cuda")
    targets = first.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nv.call("ea_adaptive_score", M, C, len(dims), hc, hd, nv.ptr(xbuf), tv._code(xbuf), xbuf.stride(0), nv.ptr(targets),
                nv.ptr(head), nv.io_dtype(head), nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in projs]),
                nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tabs]), nv.ptr(ws), nbytes, nv.ptr(logp), None, nv.stream())
    g.replay()
    torch.cuda.synchronize()
    assert _bits(logp, want_first)
    targets.copy_(second)                                  # the band counts change: tail 0 empties, two rows leave [0, V)
    g.replay()
    torch.cuda.synchronize()
    assert _bits(logp, want_second)


# ---- the stack -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_stack():
    from ea_harness.sequence import DecoderStack
    d, sd = _small_state()
    torch.manual_seed(9)
    m = DecoderStack(333, 128, 256, 2, 2, tv.ATTN, pad_idx=1, adaptive=dict(cutoff=[96, 200], factor=2))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        for layer in m.layers:
            layer.self_attn.rel_pos_bias.relative_attention_bias.weight.mul_(20.0)
    full = dict(m.state_dict())
    full.update(sd)
    m.load_state_dict(full, strict=True)
    return m.cuda().eval(), torch.from_numpy(d["tokens"]).cuda()


_BANNED = tvs._BANNED + ((torch, "index_select"), (torch.Tensor, "index_select"), (torch, "nonzero"), (torch.Tensor, "nonzero"))


@pytest.mark.gpu
def test_g6_evaluate_on_the_adaptive_stack(monkeypatch):
    from ea_harness.sequence import AdaptiveTables
    dtype = torch.bfloat16
    m, tokens = _fixture_stack()
    SB, ST = tokens.shape
    tables = m.adaptive_tables(dtype)
    assert isinstance(tables, AdaptiveTables) and tables.dims == [64, 32] and tuple(tables.head.shape) == (98, 128)
    assert [tuple(p.shape) for p in tables.proj] == [(64, 128), (32, 128)] and tables.proj[0].is_contiguous()
    sm = m.adaptive_softmax
    assert torch.equal(tables.proj[1].float(), sm.tail[1][0].weight.t()) and torch.equal(tables.tables[0].float(), sm.tail[0][2].weight)
    ptrs = [t.data_ptr() for t in [tables.head] + tables.proj + tables.tables]
    assert tables.refresh() is tables and ptrs == [t.data_ptr() for t in [tables.head] + tables.proj + tables.tables]
    rows = tvs._full_rows(m, tokens, dtype)
    targets = tokens[:, 1:].t().contiguous()
    pad = tokens[:, 1:].eq(m.pad_idx)
    assert int(pad.sum()) >= 1
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = m.evaluate(tokens)
        held, greedy = m.evaluate(tokens, table=tables, return_tokens=True)
        want_tok, want = m.rows_logprobs(rows, tables, targets)
        torch.cuda.synchronize()
    assert tuple(got.shape) == (SB, ST - 1) and got.dtype == torch.float32 and greedy.dtype == torch.long
    assert _bits(got, held) and (got[pad] == 0).all() and torch.equal(greedy, want_tok.t())
    assert _bits(got[~pad], want.t()[~pad]) and (got[~pad] < 0).all()
    with pytest.raises(ValueError, match="logits"):
        m.rows_logprobs(rows, tables, None)
    calls = []

    def forward(tok, mask=None):
        calls.append(tuple(tok.shape))
        return rows
    monkeypatch.setattr(m, "forward", forward)
    for mod, fname in _BANNED:
        def banned(*a, _name=fname, **k):
            raise AssertionError("%s reached in evaluate behind the full path" % _name)
        monkeypatch.setattr(mod, fname, banned)
    with _ctx(dtype):
        again = m.evaluate(tokens, table=tables)
        torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls == [(SB, ST - 1)] and _bits(again, got)
    # fp64 on the 16-bit tables and the same rows, the tails on the kernel's own h_i: G4's summed tolerance
    M = (ST - 1) * SB
    geo = dict(C=128, cutoffs=tables.cutoff, dims=tables.dims)
    x2 = rows.reshape(M, 128).float().contiguous()
    t = targets.reshape(-1).cpu().numpy()
    raw = _adaptive(geo, x2, tables.head, tables.proj, tables.tables, targets.reshape(-1).contiguous())
    assert _bits(raw["logp"].view(ST - 1, SB), want)
    _, want_rows, want_count = aref.route(t, tables.cutoff)
    own_h = [raw["h"][i][:int(want_count[i])].cpu().double().numpy() for i in range(2)]
    xh = x2.to(dtype).cpu()
    tabs = [w.cpu() for w in tables.tables]
    ref = aref.score(xh.double().numpy(), tables.head.cpu().double().numpy(), None, [w.double().numpy() for w in tabs],
                     tables.cutoff, t, h=own_h)
    bound_head = ops.bound(xh, tables.head.cpu()).numpy()
    place = {int(r): (i, j) for i, rr in enumerate(want_rows) for j, r in enumerate(rr)}
    flat, worst = want.reshape(-1).cpu().numpy(), 0.0
    for i in range(M):
        row = ref["head_rows"][i]
        allowed = aref.tol_logp(bound_head[i], row, lref.lse(row))
        if i in place:
            b, j = place[i]
            row = ref["tail_rows"][i]
            allowed += aref.tol_logp(ops.bound(raw["h"][b][j:j + 1].cpu(), tabs[b]).numpy()[0], row, lref.lse(row))
        err = abs(float(flat[i]) - ref["logp"][i])
        assert err <= allowed, (i, float(flat[i]), ref["logp"][i], err, allowed)
        worst = max(worst, err / allowed)
    assert len(place) >= 8 and all(c > 0 for c in want_count)
    print("largest |evaluate - fp64 adaptive log-probability| / tolerance: %.4f" % worst)
    with pytest.raises(NotImplementedError, match="adaptive"):
        m.init_decoding(SB, 8, dtype, "cuda", hold_vocab=True)


@pytest.mark.gpu
def test_g6_decode_on_the_adaptive_stack_eager_and_captured():
    """fp32 decode rows = forward rows at the fp32 decoding criterion (tests/test_gpu_decoder_stack.py, 5); the last tokens by
    one captured single-token step: AdaptiveInput runs inside a capture."""
    _skip_f32(torch.float32)
    dtype = torch.float32
    m, tokens = _fixture_stack()
    SB, ST = tokens.shape
    P = 17
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = m(tokens)
        st = m.init_decoding(SB, ST, dtype, "cuda", hold_weights=False)
        eager = [m.decode(tokens.t()[:P], st)] + [m.decode(tokens.t()[t:t + 1], st) for t in range(P, ST)]
        e = _err(torch.cat(eager, 0), full)
        assert e[0] <= F32_TOL[0] and e[1] <= F32_TOL[1], e
        st = m.init_decoding(SB, ST, dtype, "cuda", hold_weights=False)
        rows = [m.decode(tokens.t()[:P], st)]
        xin = tokens.t()[P:P + 1].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            rows.append(m.decode(xin, st).clone())                           # token P: the warm-up step
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        xin.copy_(tokens.t()[P + 1:P + 2])
        with torch.cuda.graph(g):
            yout = m.decode(xin, st)
        for t in range(P + 1, ST):
            xin.copy_(tokens.t()[t:t + 1])
            g.replay()
            rows.append(yout.clone())
        torch.cuda.synchronize()
    got = torch.cat(rows, 0)
    e = _err(got, full)
    print("adaptive stack, fp32 (max, rms) error of captured decoding vs forward:", e)
    assert got.shape == full.shape and e[0] <= F32_TOL[0] and e[1] <= F32_TOL[1], e
    assert not m.decoding_overflowed(st)


@pytest.mark.gpu
def test_g6_generate_and_logits_on_the_slow_route():
    """A state without hold_vocab: `generate` picks from `logits`, the torch restatement of the whole distribution; captured
    and eager decoding give the same tokens (tests/test_gpu_decoder_stack.py, 8), and the distribution sums to 1 at the fp32
    oracle tolerance."""
    m, tokens = _fixture_stack()
    prompt = tokens[:, :9].contiguous()
    with _ctx(torch.bfloat16), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        replayed = m.generate(prompt, 4, graph=True)
        eager = m.generate(prompt, 4, graph=False)
    assert tuple(replayed.shape) == (2, 4) and torch.equal(replayed, eager)
    assert (replayed >= 0).all() and (replayed < 333).all()
    x = torch.randn(3, 2, 128, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        lp = m.logits(x)
    assert tuple(lp.shape) == (3, 2, 333) and lp.dtype == torch.float32
    torch.testing.assert_close(lp.exp().sum(-1), torch.ones(3, 2, device="cuda"), rtol=1e-5, atol=1e-6)
