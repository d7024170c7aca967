"""-m gpu: sampling and the beam step from the adaptive head (csrc/ea_adaptive_pick.hip, C ABI 35: ea_adaptive_sample,
ea_adaptive_beam) and DecoderStack on a state with an adaptive pick and a sampler or a beam.  The geometries, operands and framed
buffers are tests/test_gpu_adaptive_pick.py's (A: ragged tiles, k = 64 > V_0; B: one 256-wide tail over two spans plus 21
columns; C: four tails, one wider than MAX_K: both tail routes); bf16 and fp16; M in {1, 17, 64}; top_k in {1, 5, 64}.

 1 exact      the stored band logits, cls and lse are read out of the workspace; the joint scores are formed in np.float32 by
              the documented operations and the rule is applied on the host (tests/adaptive_select_reference.py): sel_idx equal,
              sel_val bitwise equal, the bands' lists likewise.  No tolerance: subtractions and additions only.
 2 fp64       the stored logits, cls and lse against the fp64 reference on the kernel's own 16-bit operands, within
              adaptive_pick_reference's tolerances (tol_h, tol_logp on decoder_vocab_operands.bound).
 3 top_k = 1  token and logp are ea_adaptive_pick's on the same operands, bit for bit.
 4 draws      u from (seed, ctr, sid) by decoder_sample_reference.uniform; kept and the drawn entry admissible on the returned
              sel_val; ctr advances by one; logp == sel_val at the drawn entry.
 5 planted    large, equal logits in every band -- a band's last ragged tile, both sides of a span boundary, duplicates.
 6 rows       M = 64 against the same rows alone; a NaN row leaves the others' bits.
 7 beam       cand_idx / cand_score against the reference for (S, W) in {(1, 1), (2, 4), (2, 32)}; forced steps with eos in
              the head and in a tail; done sentences; the merge against decoder_beam_reference.merge on those candidates.
 8 capture    a captured sampled call replayed on rewritten rows draws the eager sequence, fresh at every replay.
 9 stack      generate sampled (replayed == eager, the seed repeats, logp == token_logprobs(targets=tokens)); beam_search
              (replayed == eager loop == host search over the kernel's own joint rows); the entries issued; the bytes."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import adaptive_pick_reference as pref
import adaptive_select_reference as sel
import decoder_beam_reference as bref
import decoder_sample_reference as sref
import decoder_vocab_operands as ops
import test_gpu_adaptive_pick as tap
import test_gpu_decoder_vocab as tv
import test_gpu_vocab_score as tvs
from ceva_decoding import _ctx

GEOMETRIES, MS, KS = tap.GEOMETRIES, (1, 17, 64), (1, 5, 64)
W_DTYPES, W_IDS = ops.W_DTYPES, ["bf16", "fp16"]
_bits = tv._bits
F32 = np.float32


def _args(geo, xbuf, dev):
    """ea_adaptive_pick's operands as both entries take them (no targets), up to the workspace."""
    from efficient_attention import _native as nv
    C, cut, dims = geo["C"], geo["cutoffs"], geo["dims"]
    head, projs, tabs = dev
    return [C, len(dims), nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims), nv.ptr(xbuf), tv._code(xbuf),
            xbuf.stride(0), nv.ptr(head), nv.io_dtype(head), nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in projs]),
            nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tabs])]


def _workspace(geo, M, W=0):
    """-> (layout, the 0xFF-filled workspace with 16 guard bytes)"""
    from efficient_attention import _native as nv
    cut, dims = geo["cutoffs"], geo["dims"]
    lay = sel.ws_layout(M, cut, dims, W)
    arrays = (nv.host_array(ctypes.c_int64, cut), nv.host_array(ctypes.c_int32, dims))
    nbytes = nv.lib().ea_adaptive_beam_ws(M, len(dims), *arrays, W) if W else nv.lib().ea_adaptive_sample_ws(M, len(dims), *arrays)
    assert nbytes == lay["total"]
    return lay, torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")


def _parts(geo, M, lay, ws):
    """What a test must find in the workspace: logits [b] fp32 [M, V_b], cls [M, n], lse [b] [M], h [i], the bands' lists."""
    cut, dims = geo["cutoffs"], geo["dims"]
    n, sizes = len(dims), sel.band_sizes(cut)

    def part(name, dtype, count):
        size = torch.empty((), dtype=dtype).element_size()
        return ws[lay[name]:lay[name] + size * count].view(dtype)
    return dict(logits=[part("logits%d" % b, torch.float32, M * v).view(M, v) for b, v in enumerate(sizes)],
                cls=part("cls", torch.float32, M * n).view(M, n), lse=[part("lse%d" % b, torch.float32, M) for b in range(n + 1)],
                list_idx=part("list_idx", torch.int32, M * (n + 1) * 64).view(M, n + 1, 64),
                list_val=part("list_val", torch.float32, M * (n + 1) * 64).view(M, n + 1, 64))


def _sample(geo, M, xbuf, dev, top_k, top_p=1.0, temperature=1.0, seed=11, ctr=None, sid=None):
    """One ea_adaptive_sample call on fresh framed buffers -> its outputs and the workspace's parts."""
    from efficient_attention import _native as nv
    lay, ws = _workspace(geo, M)
    token = torch.full((M + 1,), -7, dtype=torch.long, device="cuda")
    logp = torch.full((M + 1,), 7.0, dtype=torch.float32, device="cuda")
    sel_idx = torch.full((M, top_k), -9, dtype=torch.int32, device="cuda")
    sel_val = torch.full((M, top_k), 9.0, dtype=torch.float32, device="cuda")
    kept = torch.full((M + 1,), -9, dtype=torch.int32, device="cuda")
    ctr = (torch.zeros(M, dtype=torch.long) if ctr is None else torch.as_tensor(ctr, dtype=torch.long)).cuda()
    sid = (torch.arange(M, dtype=torch.int32) if sid is None else torch.as_tensor(sid, dtype=torch.int32)).cuda()
    ctr0 = ctr.clone()
    nv.call("ea_adaptive_sample", M, *_args(geo, xbuf, dev), nv.ptr(ws), ws.numel() - 16, top_k, top_p, temperature, seed,
            nv.ptr(ctr), nv.ptr(sid), nv.ptr(token), nv.ptr(logp), nv.ptr(sel_idx), nv.ptr(sel_val), nv.ptr(kept), nv.stream())
    torch.cuda.synchronize()
    assert (ws[-16:] == 0xFF).all() and token[M].item() == -7 and logp[M].item() == 7.0 and kept[M].item() == -9
    out = dict(token=token[:M], logp=logp[:M], sel_idx=sel_idx, sel_val=sel_val, kept=kept[:M], ctr=ctr, ctr0=ctr0, sid=sid)
    out.update(_parts(geo, M, lay, ws))
    wdtype = dev[0].dtype
    hall = ws[lay["h"]:lay["h"] + 2 * M * lay["D"]].view(wdtype).view(M, lay["D"])
    out["h"] = list(hall.split(geo["dims"], 1))
    return out


def _host(got):
    return ([t.cpu().numpy() for t in got["logits"]], got["cls"].cpu().numpy(), [t.cpu().numpy() for t in got["lse"]])


def _check_exact(geo, got, k, what):
    """1: the rule on the kernel's own numbers."""
    cut = geo["cutoffs"]
    logits, cls, lse = _host(got)
    idx, val, joint = sel.select(logits, cls, lse, cut, k)
    kk = idx.shape[1]
    assert kk == min(k, cut[-1])
    assert (got["sel_idx"][:, :kk].cpu().numpy() == idx).all(), what
    assert got["sel_val"][:, :kk].cpu().numpy().tobytes() == val.tobytes(), what
    assert (got["sel_idx"][:, kk:] == -9).all() and (got["sel_val"][:, kk:] == 9.0).all(), "entries from min(k, V) on are not written"
    li, lv = got["list_idx"].cpu().numpy(), got["list_val"].cpu().numpy()
    for b, rows in enumerate(logits):
        for m in range(rows.shape[0]):
            cols = sref.topk(rows[m], k)
            assert (li[m, b, :cols.size] == cols).all() and lv[m, b, :cols.size].tobytes() == rows[m][cols].tobytes(), (what, b, m)
    return idx, val, joint


def _check_fp64(geo, wdtype, xh, head, tabs, got, what):
    """2: logits, cls and lse against fp64 on the kernel's own h_i."""
    cut, c0 = geo["cutoffs"], geo["cutoffs"][0]
    own_h = [h.cpu() for h in got["h"]]
    ref = pref.pick(xh.double().numpy(), head.double().numpy(), None, [w.double().numpy() for w in tabs], cut, None,
                    h=[h.double().numpy() for h in own_h])
    tol = tap._band_tols(geo, wdtype, xh, head, tabs, ref, own_h)
    logits, cls, lse = _host(got)
    worst = 0.0
    for b in range(len(cut)):
        want = ref["head_rows"][:, :c0] if b == 0 else ref["tail_rows"][b - 1]
        for name, err in (("logits", np.abs(logits[b] - want).max(1)), ("lse", np.abs(lse[b] - ref["lse"][b]))):
            assert (err <= tol[b]).all(), (what, name, b, float((err / tol[b]).max()))
            worst = max(worst, float((err / tol[b]).max()))
    err = np.abs(cls - ref["head_rows"][:, c0:]) / tol[0][:, None]
    assert (err <= 1.0).all(), (what, "class logits", float(err.max()))
    return max(worst, float(err.max()))


def _check_draws(got, k, top_p, temperature, seed, what):
    """4: kept and the drawn entry are admissible on the returned sel_val; ctr; logp."""
    M = got["token"].numel()
    token, logp, kept = got["token"].cpu().numpy(), got["logp"].cpu().numpy(), got["kept"].cpu().numpy()
    sel_idx, sel_val = got["sel_idx"].cpu().numpy(), got["sel_val"].cpu().numpy()
    ctr0, sid = got["ctr0"].cpu().numpy(), got["sid"].cpu().numpy()
    u = sref.uniform(seed, ctr0, sid)
    kk = int((sel_idx[0] != -9).sum())
    for m in range(M):
        c = sref.cumulative(sel_val[m, :kk], temperature)
        assert kept[m] in sref.admissible_kept(c, top_p), (what, m, int(kept[m]))
        at = np.nonzero(sel_idx[m, :kk] == token[m])[0]
        assert at.size == 1 and int(at[0]) in sref.admissible_js(c, int(kept[m]), float(u[m])), (what, m, at.tolist(), float(u[m]))
        assert logp[m:m + 1].tobytes() == sel_val[m, at[0]:at[0] + 1].tobytes(), (what, m, "logp is the drawn entry's score")
    assert got["ctr"].cpu().tolist() == (ctr0 + 1).tolist(), (what, "ctr advances by exactly one")


# ---- 1 .. 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_s1_the_selection_is_exact_and_the_draws_are_admissible(name, wdtype):
    geo = GEOMETRIES[name]
    x32, head, projs, tabs = tap._operands(name, wdtype)
    dev = tap._device(head, projs, tabs)
    worst = 0.0
    for M in MS:
        xbuf = tvs._xbuf(x32[:M], wdtype, M != 17)
        xh = x32[:M].to(wdtype)
        for k in KS:
            what = (name, wdtype, M, k)
            rs = np.random.RandomState(M + k)
            ctr, sid = rs.randint(0, 1 << 40, size=M), rs.randint(0, 1 << 30, size=M)
            got = _sample(geo, M, xbuf, dev, k, 0.8, 0.7, 5, ctr, sid)
            _check_exact(geo, got, k, what)
            _check_draws(got, k, 0.8, 0.7, 5, what)
            if k == 64:
                worst = max(worst, _check_fp64(geo, wdtype, xh, head, tabs, got, what))
                whole = _sample(geo, M, xbuf, dev, k, 1.0, 1.0, 6, ctr, sid)
                assert (whole["kept"] == min(k, geo["cutoffs"][-1])).all(), "top_p = 1 keeps the whole list"
                _check_draws(whole, k, 1.0, 1.0, 6, what)
            if k == 1:                                               # 3: ea_adaptive_pick's token and logp, bit for bit
                pick = tap._pick(geo, M, xbuf, dev)
                assert torch.equal(got["token"], pick["token"]) and _bits(got["logp"], pick["logp"]), what
                assert all(_bits(a, b) for a, b in zip(got["lse"], pick["lse"])) and _bits(got["cls"], pick["cls"]), what
                assert (got["kept"] == 1).all()
            else:                                                    # entry 0 has the pick's logp at any k
                assert _bits(got["sel_val"][:, 0].contiguous(), tap._pick(geo, M, xbuf, dev)["logp"]), what
    print(name, wdtype, "largest error / tolerance %.4f" % worst)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_s5_planted_winners_span_every_band(name, wdtype):
    geo, M = GEOMETRIES[name], 17
    cut, dims = geo["cutoffs"], geo["dims"]
    x32, head, projs, tabs = tap._plant_operands(name, wdtype, M)
    planted = []
    for b in range(len(dims) + 1):
        base = 0 if b == 0 else cut[b - 1]
        Vb, span = cut[b] - base, tap._band_span(geo, b)
        # duplicates in one tile and across tiles, both sides of a span boundary, the band's last (ragged) tile
        cols = sorted({u for u in (3, 5, 21, span - 1, span, Vb - 1) if u < Vb})
        head, tabs = tap._planted(geo, b, cols, head, tabs)
        planted += [base + u for u in cols]
    assert len(planted) <= 64 and any(v % 16 for v in sel.band_sizes(cut)), "a ragged last tile is among them"
    if name == "B":
        assert tap.SPAN - 1 + cut[0] in planted and tap.SPAN + cut[0] in planted
    got = _sample(geo, M, tvs._xbuf(x32, wdtype, True), tap._device(head, projs, tabs), 64)
    idx, val, joint = _check_exact(geo, got, 64, (name, wdtype, "planted"))
    full = np.concatenate(joint, 1)
    others = np.delete(full, planted, axis=1)
    assert (full[:, planted].min(1) - others.max(1) >= 1.0).all(), "the planted tokens lead by a margin"
    n = len(planted)
    for m in range(M):
        assert sorted(idx[m, :n].tolist()) == planted, (name, m, "the top of the list is the planted tokens, from every band")
        for b in range(len(dims) + 1):                               # equal logits of one band: equal scores, the lower index first
            lo, hi = (0, cut[0]) if b == 0 else (cut[b - 1], cut[b])
            mine = [t for t in idx[m, :n].tolist() if lo <= t < hi]
            assert mine == sorted(mine) and len(set(full[m, mine].tolist())) == 1, (name, m, b)
    print(name, wdtype, "%d planted tokens" % n)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
OUT_KEYS = ("token", "logp", "sel_idx", "sel_val", "kept", "ctr")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_s6_a_rows_results_depend_on_that_row_alone(name):
    geo, M, wdtype, k = GEOMETRIES[name], 64, torch.bfloat16, 5
    x32, head, projs, tabs = tap._operands(name, wdtype)
    dev = tap._device(head, projs, tabs)
    rs = np.random.RandomState(3)
    ctr, sid = rs.randint(0, 1 << 40, size=M), rs.randint(0, 1 << 30, size=M)
    whole = _sample(geo, M, tvs._xbuf(x32, wdtype, True), dev, k, 0.9, 0.8, 7, ctr, sid)
    again = _sample(geo, M, tvs._xbuf(x32, wdtype, False), dev, k, 0.9, 0.8, 7, ctr, sid)
    assert all(_bits(whole[key], again[key]) for key in OUT_KEYS), "two calls, 16-bit x"
    for m in range(M):
        one = _sample(geo, 1, tvs._xbuf(x32[m:m + 1], wdtype, m % 2 == 0), dev, k, 0.9, 0.8, 7, ctr[m:m + 1], sid[m:m + 1])
        assert all(_bits(whole[key][m:m + 1], one[key]) for key in OUT_KEYS), (name, m, "M = 64 against M = 1")
    part = _sample(geo, 17, tvs._xbuf(x32[:17], wdtype, True), dev, k, 0.9, 0.8, 7, ctr[:17], sid[:17])
    assert all(_bits(whole[key][:17], part[key]) for key in OUT_KEYS), "the two-row-tile instance"
    bad = x32.clone()
    bad[3] = float("nan")
    got = _sample(geo, M, tvs._xbuf(bad, wdtype, True), dev, k, 0.9, 0.8, 7, ctr, sid)
    keep = [m for m in range(M) if m != 3]
    assert all(_bits(got[key][keep], whole[key][keep]) for key in OUT_KEYS), "a NaN row changes no other row's bits"
    assert 0 <= got["token"][3].item() < geo["cutoffs"][-1] and got["kept"][3].item() == 0 and torch.isnan(got["logp"][3])
    assert got["token"][3].item() == got["sel_idx"][3, 0].item() and got["ctr"][3].item() == ctr[3] + 1


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def _beam_state(S, W, max_new, t, nfin, done, score):
    M = S * W
    i32, f32 = torch.int32, torch.float32
    return dict(score=torch.tensor(score, dtype=f32).cuda(), t=torch.tensor(t, dtype=i32).cuda(),
                nfin=torch.tensor(nfin, dtype=i32).cuda(), done=torch.tensor(done, dtype=i32).cuda(),
                token=torch.full((M,), -7, dtype=torch.long, device="cuda"),
                parent=torch.full((M,), -7, dtype=torch.long, device="cuda"),
                hist_tok=torch.full((max_new, M), -7, dtype=i32, device="cuda"),
                hist_par=torch.full((max_new, M), -7, dtype=i32, device="cuda"),
                fin_score=torch.full((S, W), 7.0, dtype=f32, device="cuda"), fin_len=torch.full((S, W), -7, dtype=i32, device="cuda"),
                fin_beam=torch.full((S, W), -7, dtype=i32, device="cuda"))


STATE = ("score", "t", "nfin", "done", "token", "parent", "hist_tok", "hist_par", "fin_score", "fin_len", "fin_beam")


def _beam(geo, S, W, xbuf, dev, eos, max_new, st, report=True):
    from efficient_attention import _native as nv
    M = S * W
    lay, ws = _workspace(geo, M, W)
    cand_idx = torch.full((M, 2 * W), -9, dtype=torch.int32, device="cuda") if report else None
    cand_score = torch.full((M, 2 * W), 9.0, dtype=torch.float32, device="cuda") if report else None
    nv.call("ea_adaptive_beam", M, *_args(geo, xbuf, dev), nv.ptr(ws), ws.numel() - 16, W, eos, max_new,
            *[nv.ptr(st[k]) for k in STATE], nv.ptr(cand_idx), nv.ptr(cand_score), nv.stream())
    torch.cuda.synchronize()
    assert (ws[-16:] == 0xFF).all()
    out = _parts(geo, M, lay, ws)
    if not report:
        cand_idx = ws[lay["cand_idx"]:lay["cand_idx"] + 8 * M * W].view(torch.int32).view(M, 2 * W)
        cand_score = ws[lay["cand_score"]:lay["cand_score"] + 8 * M * W].view(torch.float32).view(M, 2 * W)
    out.update(cand_idx=cand_idx, cand_score=cand_score)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S,W", [(1, 1), (2, 4), (2, 32)])
@pytest.mark.parametrize("name", ["A", "C"])
def test_s7_the_beam_step(name, S, W):
    geo, wdtype, max_new = GEOMETRIES[name], torch.bfloat16, 6
    cut = geo["cutoffs"]
    V, M = cut[-1], S * W
    x32, head, projs, tabs = tap._operands(name, wdtype)
    dev = tap._device(head, projs, tabs)
    xbuf = tvs._xbuf(x32[:M], wdtype, True)
    rs = np.random.RandomState(S * 100 + W)
    # a free run to learn a token the rows favour: with it as eos the merge finishes hypotheses
    probe = _sample(geo, M, xbuf, dev, 1)
    favourite = int(probe["token"][0])
    cases = [("step", favourite, [2] * S, [0] * S), ("eos in the head", 3, [2] * S, [0] * S), ("forced, eos in the head", 5, [max_new - 1] * S, [0] * S),
             ("forced, eos in a tail", cut[1] - 1, [max_new - 1] * S, [0] * S), ("forced, eos in the last tail", V - 1, [max_new - 1] * S, [0] * S)]
    if S > 1:
        cases.append(("a done sentence", favourite, [2, 4], [1, 0]))
    for what, eos, t, done in cases:
        score = rs.randn(M).astype(F32)
        if W > 1:
            score[W - 1] = -np.inf                                   # a dead beam
        nfin = [0 if not d else W for d in done]
        for report in (True, False) if what == "step" else (True,):
            st = _beam_state(S, W, max_new, t, nfin, done, score)
            got = _beam(geo, S, W, xbuf, dev, eos, max_new, st, report)
            logits, cls, lse = _host(got)
            forced = t[0] + 1 >= max_new
            idx, val, joint = sel.select(logits, cls, lse, cut, 2 * W)
            kc = idx.shape[1]
            assert kc == min(2 * W, V)
            if forced:
                idx, val = np.full((M, 1), eos), sel.eos_score(joint, cut, eos)[:, None]
            ci, cs = sel.beam_candidates(idx, val, score)
            gi, gs = got["cand_idx"].cpu().numpy(), got["cand_score"].cpu().numpy()
            for s in range(S):
                rows = slice(s * W, s * W + W)
                if done[s]:                                          # skipped: the lists keep their fill (the workspace's: 0xFF)
                    assert (gi[rows] == (-9 if report else -1)).all(), (what, "a done sentence's rows are skipped")
                else:
                    k = ci.shape[1]
                    assert (gi[rows, :k] == ci[rows]).all() and gs[rows, :k].tobytes() == cs[rows].tobytes(), (name, S, W, what)
                    if report:
                        assert (gi[rows, k:] == -9).all()
                want = bref.merge(ci[rows], cs[rows], kc, W, eos, t[s], nfin[s], done[s], forced)
                assert st["token"][rows].tolist() == want["token"], (name, S, W, what, "token")
                assert st["parent"][rows].tolist() == [s * W + b for b in want["parent"]], (what, "parent")
                assert (st["t"][s].item(), st["nfin"][s].item(), st["done"][s].item()) == (want["t"], want["nfin"], want["done"]), what
                if want["score"] is None:
                    assert st["score"][rows].cpu().numpy().tobytes() == score[rows].tobytes() and (st["hist_tok"][:, rows] == -7).all()
                    continue
                assert st["score"][rows].cpu().numpy().tobytes() == want["score"].tobytes(), (what, "score")
                assert st["hist_tok"][t[s], rows].tolist() == want["hist_tok"] and st["hist_par"][t[s], rows].tolist() == want["hist_par"]
                for i, (sc, length, b) in enumerate(want["records"]):
                    at = nfin[s] + i
                    assert st["fin_score"][s, at].cpu().numpy().tobytes() == F32(sc).tobytes(), (what, "fin_score")
                    assert (st["fin_len"][s, at].item(), st["fin_beam"][s, at].item()) == (length, b), what
                assert not forced or want["done"] == 1


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_s8_a_captured_call_draws_afresh_on_rewritten_rows(name):
    from efficient_attention import _native as nv
    geo, M, wdtype, k = GEOMETRIES[name], 17, torch.bfloat16, 5
    x32, head, projs, tabs = tap._operands(name, wdtype)
    dev = tap._device(head, projs, tabs)
    xs = [x32[:M], x32[M:2 * M], x32[:M]]
    want, ctr = [], np.zeros(M, dtype=np.int64)
    for i, x in enumerate(xs):                                       # the eager sequence: draw i at ctr = i
        got = _sample(geo, M, tvs._xbuf(x, wdtype, True), dev, k, 0.95, 1.3, 21, ctr + i)
        want.append((got["token"].clone(), got["logp"].clone()))
    assert not torch.equal(want[0][0], want[2][0]), "the same rows draw afresh at another counter"
    lay, ws = _workspace(geo, M)
    token = torch.zeros(M, dtype=torch.long, device="cuda")
    logp = torch.zeros(M, dtype=torch.float32, device="cuda")
    ctr = torch.zeros(M, dtype=torch.long, device="cuda")
    sid = torch.arange(M, dtype=torch.int32, device="cuda")
    xbuf = tvs._xbuf(xs[0], wdtype, True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nv.call("ea_adaptive_sample", M, *_args(geo, xbuf, dev), nv.ptr(ws), ws.numel() - 16, k, 0.95, 1.3, 21, nv.ptr(ctr),
                nv.ptr(sid), nv.ptr(token), nv.ptr(logp), None, None, None, nv.stream())
    for i, x in enumerate(xs):
        xbuf[:M, :geo["C"]] = x.cuda()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(token, want[i][0]) and _bits(logp, want[i][1]), (name, "replay", i)
        assert ctr.tolist() == [i + 1] * M


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
class _Entries:
    """The names of the adaptive pick entries `nv.call` is handed inside the block, in order."""

    def __enter__(self):
        from efficient_attention import _native as nv
        self.nv, self.real, self.names = nv, nv.call, []

        def call(name, *a):
            if name in ("ea_adaptive_pick", "ea_adaptive_sample", "ea_adaptive_beam"):
                self.names.append(name)
            return self.real(name, *a)
        nv.call = call
        return self

    def __exit__(self, *exc):
        self.nv.call = self.real


def _sampled_state(m, B, T, seed, **opt):
    return m.init_sampling(tap._state(m, B, T, **opt), seed, 8, 0.9, 1.2)


@pytest.mark.gpu
def test_s9_generate_samples_from_the_adaptive_head():
    dtype, n_new = torch.bfloat16, 6
    m, tokens = tap._fixture()
    B = tokens.shape[0]
    prompt = tokens[:, :9].clone()
    out = {}
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bare = m.decoding_state_nbytes(tap._state(m, B, 9 + n_new))
        for key, graph, seed in (("eager", False, 4), ("graph", True, 4), ("again", True, 4), ("other", True, 5)):
            st = _sampled_state(m, B, 9 + n_new, seed)
            with _Entries() as calls:
                out[key] = m.generate(prompt, n_new, st, graph=graph, return_rows=True, return_logprobs=True) + (st,)
            if graph:
                assert calls.names == ["ea_adaptive_sample"] * 3, calls.names
            assert torch.equal(m.generate(prompt, n_new, _sampled_state(m, B, 9 + n_new, seed), graph=graph), out[key][0])
        tok, rows, lp, st = out["graph"]
        assert torch.equal(tok, out["eager"][0]) and _bits(rows, out["eager"][1]) and _bits(lp, out["eager"][2]), "replayed == eager"
        assert torch.equal(tok, out["again"][0]) and _bits(lp, out["again"][2]), "the same seed repeats"
        assert not torch.equal(tok, out["other"][0]), "another seed draws other tokens"
        assert tuple(tok.shape) == (B, n_new) and tuple(lp.shape) == (B, n_new) and (lp < 0).all() and int(tok.max()) < 333
        assert st.sampler.ctr.tolist() == [n_new] * B
        # the drawn tokens' log-probabilities: token_logprobs with them as targets (the same passes, the same fold: the same bits)
        greedy_tok, want = m.token_logprobs(rows, tap._state(m, B, 9 + n_new), targets=tok.t().contiguous())
        assert _bits(want.t().contiguous(), lp), "return_logprobs is token_logprobs(targets=tokens)"
        assert not torch.equal(greedy_tok.t(), tok), "sampled, not greedy"
        # the public steps: sample_tokens with details, sample_tokens_logprobs
        st2 = _sampled_state(m, B, 9 + n_new, 4)
        t1, sel_idx, sel_val, kept = m.sample_tokens(rows[:1], st2, return_details=True)
        assert torch.equal(t1[0], tok[:, 0]) and tuple(sel_idx.shape) == (B, 8) and (kept >= 1).all()
        assert (sel_idx == t1.view(B, 1)).sum(1).tolist() == [1] * B
        st2.sampler.ctr.zero_()
        t2, lp2 = m.sample_tokens_logprobs(rows[:1], st2)
        assert torch.equal(t2, t1) and _bits(lp2[0], lp[:, 0].contiguous())
        # the bytes: the sampler's workspace for B rows, ctr, sid
        sm = st.sampler
        assert sm.ws.numel() == sel.ws_layout(B, st.adaptive.tables.cutoff, st.adaptive.tables.dims)["total"]
        assert m.decoding_state_nbytes(st) == bare + sm.ws.numel() + 12 * B
        # reorder and reset follow through the attachment loop
        sm.ctr.copy_(torch.arange(5, 5 + B, device="cuda"))
        m.reorder_decoding_state(st, torch.arange(B, device="cuda").flip(0))
        assert sm.ctr.tolist() == list(range(5 + B - 1, 4, -1)) and sm.sid.tolist() == list(range(B - 1, -1, -1))
    print("tokens", tok.tolist())


def _joint_rows(m, st, rows, W, masked):
    """The kernel's own joint rows [M, V] of a step, from the beam's workspace behind a beam_step on `rows`: the stored logits,
    cls and lse, the rule's fp32 operations.  masked: every token that is not among its band's 2 W best RAW logits is -inf, so
    that the best 2 W of the row are the rule's selection."""
    tb = st.adaptive.tables
    geo = dict(C=128, cutoffs=tb.cutoff, dims=tb.dims)
    M = rows.shape[1]
    got = _parts(geo, M, sel.ws_layout(M, tb.cutoff, tb.dims, W), st.beam.ws)
    logits, cls, lse = _host(got)
    joint = sel.joint(logits, cls, lse)
    if masked:
        for b, raw in enumerate(logits):
            for r in range(M):
                keep = sref.topk(raw[r], 2 * W)
                row = np.full_like(joint[b][r], -np.inf)
                row[keep] = joint[b][r][keep]
                joint[b][r] = row
    return np.concatenate(joint, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "per_sequence_ragged"])
def test_s9_beam_search_from_the_adaptive_head(case):
    dtype, W, max_new = torch.bfloat16, 4, 6
    m, tokens = tap._fixture()
    S = 2
    prompt = tokens[:S, :9].clone()
    opt = {}
    if case == "per_sequence_ragged":
        opt["per_sequence"] = True
        prompt[1, 5:] = m.pad_idx
    M = S * W
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # eos: the greedy continuation's third token, so that hypotheses finish inside the search
        eos = int(m.generate(prompt, 4, tap._state(m, S, 13, **opt), graph=False)[0, 2])
        found = {}
        for graph in (True, False):
            st = tap._state(m, M, 9 + max_new, **opt)
            with _Entries() as calls:
                found[graph] = m.beam_search(prompt, st, beam_size=W, eos_idx=eos, max_new=max_new, len_penalty=0.7, graph=graph, poll=2)
            if graph:
                assert calls.names == ["ea_adaptive_beam"] * 3, calls.names
                bm = st.beam
                bare = m.decoding_state_nbytes(tap._state(m, M, 9 + max_new, **opt))
                tb = st.adaptive.tables
                assert bm.logits is None and bm.ws.numel() == sel.ws_layout(M, tb.cutoff, tb.dims, W)["total"]
                assert m.decoding_state_nbytes(st) == bare + bm.ws.numel() + 4 * M + 12 * S + 8 * M + 8 * max_new * M + 12 * S * W
        default = m.beam_search(prompt, beam_size=W, eos_idx=eos, max_new=max_new, len_penalty=0.7) if case == "rolling" else None

        # the host search over the kernel's own joint rows, driven through decode / beam_step / reorder_decoding_state
        st = m.init_beam_search(tap._state(m, M, 9 + max_new, **opt), W, eos, max_new, 0.7)
        fed = prompt.repeat_interleave(W, 0)
        calls_made = [0]

        def step_fn(toks, parent):
            if toks is None:
                rows = m._prefill(fed, st)
            else:
                assert torch.equal(torch.from_numpy(toks).cuda(), step_fn.tok[0]) and torch.equal(torch.from_numpy(parent).cuda(), step_fn.par)
                rows = m.decode(step_fn.tok, st)
            tok, par = m.beam_step(rows, st)
            torch.cuda.synchronize()
            forced = calls_made[0] + 1 >= max_new
            calls_made[0] += 1
            joint = _joint_rows(m, st, rows, W, masked=not forced)
            step_fn.tok, step_fn.par = tok.clone(), par.clone()
            m.reorder_decoding_state(st, par)
            return joint, np.zeros(M, dtype=F32)
        hyps, info = bref.host_beam_search(step_fn, S, W, eos, max_new, 0.7)
    for s in range(S):
        assert len(found[True][s]) == len(found[False][s]) == len(hyps[s]) >= 1, (case, s)
        for a, b, h in zip(found[True][s], found[False][s], hyps[s]):
            assert torch.equal(a["tokens"], b["tokens"]) and a["tokens"].tolist() == h["tokens"], (case, s)
            assert _bits(a["raw_score"], b["raw_score"]) and a["raw_score"].numpy().tobytes() == F32(h["raw"]).tobytes(), (case, s)
            assert a["score"] == b["score"] == pytest.approx(h["score"], rel=1e-12)
        if default is not None:
            assert [h["tokens"].tolist() for h in default[s]] == [h["tokens"].tolist() for h in found[True][s]]
    assert "eos_finished" in info["events"], info["events"]
    print(case, "eos", eos, "steps", info["steps"], sorted(info["events"]), [[h["tokens"] for h in hs] for hs in hyps])
