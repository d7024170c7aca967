"""-m gpu: `landmark_splits=P` of static / rolling incremental decoding (csrc/ea_ceva_decode_split.h).

On a state made with P > 1, a step of at most 8 tokens runs attn as two launches: ea_ceva_sdecode_attn_split -- P workgroups
per (window block, b, h) share the 64-column tiles of [local keys, landmarks] and write unnormalised (acc, max, sum) partials
to the state's workspace -- and ea_ceva_sdecode_merge.  Checked here: both kernels against the fp64 restatement of
test_gpu_ceva_decode.py at the shapes where the partition can go wrong, prefix consistency of the module on split states next
to plain ones (whose cache and landmark rows they must reproduce bit for bit), the launches of each step, capture and replay,
and the bytes of the workspace."""
import ctypes
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

from test_gpu_causal_eva import RECIPE, _build                               # noqa: E402
from test_gpu_ceva_decode import _bound, _io, _ref_attn                      # noqa: E402
from ceva_decoding import DTYPES, IDS, OLD, STATIC, _Calls, _check_full, _ctx, _geometry, _skip_f32   # noqa: E402

SPLIT = STATIC[:2] + ("ea_ceva_sdecode_attn_split", "ea_ceva_sdecode_merge") + STATIC[3:]
KINDS = ["static", "rolling"]
STATE_ROWS = ("qkv", "pad", "rf_k_bar", "beta", "pos")


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. kernel level: attn_split + merge against the fp64 restatement -------------------------------------------------------
# (name, d, w, e, r, t0, T, P, ring rows or 0, bias) -- B = 2, h = 2; 64-column tiles: ceil((w + e) / 64) local ones, then
# ceil((t / r) / 64) landmark ones, shared by 4 P virtual waves
SPLIT_CASES = [
    ("L0", 64, 32, 0, 4, 1, 2, 4, 0, True),                    # no landmark yet: one tile, every part but part 0 is empty
    ("L1", 64, 32, 0, 4, 5, 1, 4, 0, False),                   # one landmark
    ("L323_P2", 64, 32, 0, 4, 1292, 1, 2, 0, True),            # 323 landmarks = 6 tiles (the last partial) + 1 on 8 waves
    ("L323_P4", 64, 32, 0, 4, 1292, 1, 4, 0, True),            # ... on 16
    ("parts_gt_tiles", 128, 128, 0, 8, 1100, 1, 16, 0, True),  # 2 + 3 tiles on 64 virtual waves
    ("boundary", 64, 32, 0, 4, 29, 6, 4, 0, True),             # tokens 29..34: two window blocks, each split
    ("ext_boundary", 64, 32, 32, 8, 60, 8, 3, 0, True),        # left extension across a boundary, P odd, T = 8
    ("d32", 32, 16, 16, 8, 3, 4, 2, 0, False),                 # D = 32, absent slots of block 0
    ("ring", 64, 32, 0, 4, 189, 5, 4, 96, True),               # ring of 96: tokens 189..193 pass its end (192 = 2 laps)
    ("ring_ext", 64, 32, 32, 4, 221, 5, 4, 96, True),          # ... and block 7's window 192..255 starts in slots 0..31
    ("max_parts", 64, 32, 0, 4, 700, 2, 64, 0, True),          # P = 64
]


def _pad_flags(B, cap, t0, T, w, e):
    """The flags of test_decode_attn_kernel_against_fp64: a fifth of the positions, and element 0's last token alone in its
    local window (its local partial carries the -5e4 fill next to landmark parts with ordinary maxima)."""
    g = torch.Generator().manual_seed(99)
    pad = torch.rand(B, cap, generator=g) < 0.2
    tl = t0 + T - 1
    bk = tl // w
    pad[0, max(bk * w - e, 0):bk * w + w] = True
    pad[0, tl] = False
    return pad, g


def _to_ring(lin, R, end):
    """Rows [end - R, end) of lin [B, cap, ...] at slots n % R."""
    n = torch.arange(end - R, end)
    out = torch.empty((lin.shape[0], R) + tuple(lin.shape[2:]), dtype=lin.dtype)
    out[:, n % R] = lin[:, n]
    return out


def _split_step(nv, dtype, d, w, e, r, T, P, cap, ring, qkv, pad, lk, lv, bias, pos, ntok=None):
    """attn_split + merge on hand-built device state -> (out [B, h, T, d], workspace [B, h, 8, P, d + 4], status)."""
    B, h = qkv.shape[0], qkv.shape[3]
    q, k, v = [qkv[:, :, i].transpose(1, 2) for i in range(3)]
    out = torch.full((B, h, T, d), 7.0, dtype=dtype, device="cuda")
    ws = torch.full((B, h, 8, P, d + 4), float("nan"), device="cuda")
    status = torch.zeros_like(pos)
    geom = nv.ea_ceva_sdec_geom(B, h, d, _io(dtype), w, e, r, T, cap, 1, 0 if bias is None else 1, ring, pos.data_ptr(),
                                status.data_ptr(), None if ntok is None else ntok.data_ptr())
    tq, tk, tv, tl, tb, to = [nv.t4(t) for t in (q, k, v, lk, lv, out)]
    nv.call("ea_ceva_sdecode_attn_split", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(pad),
            nv.ptr(bias), ctypes.byref(tl), ctypes.byref(tb), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    nv.call("ea_ceva_sdecode_merge", ctypes.byref(geom), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    torch.cuda.synchronize()
    return out, ws, geom


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_kernels_against_fp64(dtype, case):
    from efficient_attention import _native as nv
    name, d, w, e, r, t0, T, P, R, with_bias = case
    B, h = 2, 2
    cap = ((t0 + T + w - 1) // w) * w
    L = cap // r
    g = torch.Generator().manual_seed(len(name) * 7 + d)
    lin = torch.randn(B, cap, 3, h, d, generator=g).to(dtype)
    lk, lv = torch.randn(B, h, L, d, generator=g).cuda(), torch.randn(B, h, L, d, generator=g).cuda()
    pad, g = _pad_flags(B, cap, t0, T, w, e)
    bias = torch.randn(w, w + e, generator=g) if with_bias else None
    if R:
        assert R % w == 0 and R >= w + e + T and t0 >= R
        qkv, pad_d = _to_ring(lin, R, t0 + T).cuda(), _to_ring(pad, R, t0 + T).to(torch.uint8).cuda()
    else:
        qkv, pad_d = lin.cuda(), pad.to(torch.uint8).cuda()
    pos = torch.tensor([t0], dtype=torch.int32, device="cuda")
    out, ws, _ = _split_step(nv, dtype, d, w, e, r, T, P, cap, R, qkv, pad_d, lk, lv,
                             None if bias is None else bias.float().cuda(), pos)
    ql, kl, vl = [lin[:, :, i].transpose(1, 2).double() for i in range(3)]
    ref = _ref_attn(ql, kl, vl, pad, None if bias is None else bias.double(), lk.double().cpu(), lv.double().cpu(), t0, T, w, e, r)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    live = ~pad[:, t0:t0 + T].view(B, 1, T, 1)                  # padded query rows: finite only
    assert live[0, 0, T - 1, 0]                                  # element 0's last token is live by construction
    err = (got - ref).abs()
    print(name, dtype, "max |d| %.3e, max bound %.3e, max |ref| %.3e" % ((err * live).max().item(), _bound(dtype, ref).max().item(),
                                                                          ref.abs().max().item()))
    excess = (err - _bound(dtype, ref)) * live
    assert excess.max().item() <= 0, (name, dtype, excess.max().item(), ref.abs().max().item())
    # the partials: every row of a step token is written (no NaN of the fill left), rows of other step positions are not
    ws = ws.cpu()
    assert torch.isfinite(ws[:, :, :T, :, :d]).all() and not torch.isnan(ws[:, :, :T, :, d:d + 2]).any()
    assert torch.isnan(ws[:, :, T:]).all()
    assert (ws[:, :, :T, :, d + 1] >= 0).all()
    if name == "L0":                                             # one tile: parts 1 .. 3 have none
        assert (ws[:, :, :T, 1:, d] == float("-inf")).all() and (ws[:, :, :T, 1:, d + 1] == 0).all()
        assert (ws[:, :, :T, 1:, :d] == 0).all() and torch.isfinite(ws[:, :, :T, 0, d]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", [0, 96], ids=["linear", "ring"])
def test_split_kernels_with_per_sequence_counts(dtype, R):
    """append -> attn_split -> merge with ntok: rows at different counts (one across a window boundary), one row that sits
    the step out (zero rows), one whose step would pass cap (status 1, NaN rows, nothing of it written) -- the kernels' own
    handled refusal.  The live rows against the fp64 restatement of each sequence alone."""
    from efficient_attention import _native as nv
    d, w, e, r, T, P, B, h = 64, 32, 0, 4, 5, 4, 4, 2
    cap = 320
    counts, own = [125, 290, 200, cap - 2], [5, 3, 0, 5]         # 125..129 pass the boundary at 128; 318 + 5 > cap
    g = torch.Generator().manual_seed(123)
    lin = torch.randn(B, cap + T, 3, h, d, generator=g).to(dtype)
    lk, lv = torch.randn(B, h, cap // r, d, generator=g).cuda(), torch.randn(B, h, cap // r, d, generator=g).cuda()
    pad = torch.rand(B, cap + T, generator=g) < 0.2
    bias = torch.randn(w, w + e, generator=g)
    for b in range(B):
        pad[b, counts[b]:] = False                               # (append stores its tokens unflagged)
    rows = R or cap
    qkv, pad_d = torch.zeros(B, rows, 3, h, d, dtype=dtype), torch.zeros(B, rows, dtype=torch.uint8)
    for b in range(B):                                           # the tokens before each row's count
        n = torch.arange(max(counts[b] - rows, 0), counts[b])
        qkv[b, n % rows], pad_d[b, n % rows] = lin[b, n], pad[b, n].to(torch.uint8)
    qkv, pad_d = qkv.cuda(), pad_d.cuda()
    new = torch.stack([lin[b, counts[b]:counts[b] + T] for b in range(B)], 1).contiguous().cuda()       # [T, B, 3, h, d]
    flags = torch.tensor([[t >= own[b] for t in range(T)] for b in range(B)], dtype=torch.uint8, device="cuda")
    pos = torch.tensor(counts, dtype=torch.int32, device="cuda")
    status, ntok = torch.zeros_like(pos), torch.full_like(pos, -1)
    before = (qkv.clone(), pad_d.clone())
    geom = nv.ea_ceva_sdec_geom(B, h, d, _io(dtype), w, e, r, T, cap, 1, 1, R, pos.data_ptr(), status.data_ptr(), ntok.data_ptr())
    nv.call("ea_ceva_sdecode_append", ctypes.byref(geom), nv.ptr(new), nv.ptr(flags), nv.ptr(qkv), nv.ptr(pad_d), nv.stream())
    q, k, v = [qkv[:, :, i].transpose(1, 2) for i in range(3)]
    out = torch.full((B, h, T, d), 7.0, dtype=dtype, device="cuda")
    ws = torch.full((B, h, 8, P, d + 4), float("nan"), device="cuda")
    tq, tk, tv, tl, tb, to = [nv.t4(t) for t in (q, k, v, lk, lv, out)]
    bias_d = bias.float().cuda()
    nv.call("ea_ceva_sdecode_attn_split", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(pad_d),
            nv.ptr(bias_d), ctypes.byref(tl), ctypes.byref(tb), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    nv.call("ea_ceva_sdecode_merge", ctypes.byref(geom), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 1] and ntok.tolist() == own and pos.tolist() == counts
    assert torch.isnan(out[3]).all() and torch.isnan(ws[3]).all()            # refused: NaN rows, no partial
    assert torch.equal(qkv[3], before[0][3]) and torch.equal(pad_d[3], before[1][3])
    assert (out[2] == 0).all() and torch.isnan(ws[2]).all()                  # sits out: zero rows, no partial
    assert torch.equal(qkv[2], before[0][2])
    for b in (0, 1):
        n = own[b]
        assert (out[b, :, n:] == 0).all() and torch.isnan(ws[b, :, n:]).all()
        end = -(-(counts[b] + n) // w) * w                       # (the restatement indexes the whole window block)
        one = lin[b:b + 1, :end]
        ql, kl, vl = [one[:, :, i].transpose(1, 2).double() for i in range(3)]
        ref = _ref_attn(ql, kl, vl, pad[b:b + 1, :end], bias.double(), lk[b:b + 1].double().cpu(),
                        lv[b:b + 1].double().cpu(), counts[b], n, w, e, r)
        err = (out[b:b + 1, :, :n].double().cpu() - ref).abs()
        print("row", b, dtype, "max |d| %.3e, max bound %.3e" % (err.max().item(), _bound(dtype, ref).max().item()))
        assert (err - _bound(dtype, ref)).max().item() <= 0, (b, dtype)


# ---- the module on split states -------------------------------------------------------------------------------------------
def _init(m, kind, B, T, dtype, S=None, **opt):
    """ceva_decoding._init with the options of the state (per_sequence, landmark_splits) handed on."""
    st = {}
    if kind == "static":
        m.init_static_decoding(st, B, T, dtype, "cuda", **opt)
    else:
        m.init_rolling_decoding(st, B, T, dtype, "cuda", max_step_tokens=S, **opt)
    return st


def _decode(m, x, steps, kind, dtype, calls=None, **opt):
    """x [T, B, C] in steps of the given sizes, then single tokens -> (per-step rows, state)."""
    T, B = x.shape[:2]
    st, rows, t = _init(m, kind, B, T, dtype, **opt), [], 0
    for n in list(steps) + [1] * T:
        if t >= T:
            break
        n = min(n, T - t)
        if calls is not None:
            calls.step()
        rows.append(m(x[t:t + n], x[t:t + n], x[t:t + n], incremental_state=st)[0])
        t += n
    return rows, st


# ---- 2. prefix consistency, next to the plain state -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [2, 8])
def test_split_decoding_equals_full_forward_and_keeps_the_plain_state(dtype, kind, P):
    """many_chunks (w = 32, e = 16, r = 4, h = 4) over 600 tokens: 150 landmarks, 3 landmark tiles.  Steps of 200, 200 and 160
    tokens take the unsplit kernel (bitwise the plain state's rows; so do the pieces of 32 and the tail of 8 that a rolling
    state cuts the 200 into), then 5, 1, 1, .. take the split.  append and close are the
    same kernels on the same inputs in both states: qkv, pad, rf_k_bar, beta and pos equal bit for bit."""
    _skip_f32(dtype)
    aa, embed, heads, _, B = _geometry("many_chunks")
    m = _build(embed, heads, aa)
    T, steps = 600, (200, 200, 160, 5)
    torch.manual_seed(61)
    x = torch.randn(T, B, embed, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x)
        plain, pst = _decode(m, x, steps, kind, dtype)
        split, sst = _decode(m, x, steps, kind, dtype, landmark_splits=P)
    assert len(split) == len(plain) == 4 + (T - 565)
    _check_full(torch.cat(split, 0), full, dtype)
    pb, sb = m._get_input_buffer(pst), m._get_input_buffer(sst)
    assert sb["split_ws"].shape == (B, heads, 8, P, embed // heads + 4) and "split_ws" not in pb
    for k in STATE_ROWS:
        assert _bits(pb[k], sb[k]), k
    assert int(sb["pos"].item()) == T and not m.static_decoding_overflowed(sst)
    for a, b in list(zip(plain, split))[:3]:                     # above 8 tokens: the unsplit kernel
        assert _bits(a, b)
    d = (torch.cat(split[3:], 0).float() - torch.cat(plain[3:], 0).float()).abs().max().item()
    print("split vs plain rows of the short steps, max |d|:", d)


# ---- 3. launches ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_seq"])
def test_split_step_launches(kind, per):
    """A step of at most 8 tokens on a split state: the five entry points in order; a larger one: today's four.  A state with
    landmark_splits=1 and one made without the option: today's four for every step, and the same bits."""
    dtype = torch.bfloat16
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(67)
    T, B = 100, 2
    x = torch.randn(T, B, 256, device="cuda")
    steps = (7, 1, 8, 9, 40, 2, 1, 30, 1)                        # (a rolling state, S = 32, cuts the 40 into 32 + 8)
    opt = dict(per_sequence=True) if per else {}

    def core(got):
        assert not [c for c in got if c in OLD], got
        return [c for c in got if not (c.startswith("ea_linear") or c == "ea_multi_cast")]

    runs = {}
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, o in (("none", {}), ("one", dict(landmark_splits=1)), ("four", dict(landmark_splits=4))):
            with _Calls() as calls:
                rows, st = _decode(m, x, steps, kind, dtype, calls=calls, **opt, **o)
                if name == "four":                               # ... and a 1-token step on a fresh state, captured
                    xin = x[-1:].clone()
                    st2 = _init(m, kind, B, T, dtype, **opt, **o)
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    calls.step()
                    with torch.cuda.stream(s):
                        m(xin, xin, xin, incremental_state=st2)
                    torch.cuda.current_stream().wait_stream(s)
                    g = torch.cuda.CUDAGraph()
                    calls.step()
                    with torch.cuda.graph(g):
                        m(xin, xin, xin, incremental_state=st2)
                    captured, warm = calls.steps.pop(), calls.steps.pop()
            runs[name] = (rows, [core(s) for s in calls.steps])
        g.replay()
        torch.cuda.synchronize()
    sizes = list(steps) + [1] * (T - sum(steps))
    assert len(runs["four"][1]) == len(sizes)
    for n, got in zip(sizes, runs["four"][1]):
        pieces = -(-n // 32) if kind == "rolling" else 1         # the pieces of a larger step, its short tail included: unsplit
        assert got == list(SPLIT if n <= 8 else STATIC * pieces), (n, got)
    assert core(captured) == list(SPLIT) == core(warm)
    assert m.decoding_positions(st2).tolist() == [2] * B
    for name in ("none", "one"):
        assert [got for n, got in zip(sizes, runs[name][1])
                if got != list(STATIC * (-(-n // 32) if kind == "rolling" else 1))] == [], name
    assert all(_bits(a, b) for a, b in zip(runs["none"][0], runs["one"][0]))
    for n, a, b in zip(sizes, runs["none"][0], runs["four"][0]):
        if n > 8:
            assert _bits(a, b), n


# ---- 4. capture and replay ------------------------------------------------------------------------------------------------
def _run(m, x, P0, dtype, how, reorder=None, order=None, idle=None, **opt):
    """One layer on a fresh split rolling state: P0 tokens in one eager call, then single tokens, eagerly (how = "eager") or as
    one captured step replayed (the procedure of ceva_decoding._captured_run: a warm-up token on a side stream, the capture,
    replays).  reorder: before token `reorder` the state is permuted by `order` and the inputs from there on are x[:, order].
    idle: a batch row flagged in every single-token step (per-sequence states).  -> rows [T - P0, B, C], state."""
    T, B = x.shape[:2]
    st = _init(m, "rolling", B, T, dtype, **opt)
    mask = None
    if idle is not None:
        mask = torch.zeros(B, 1, dtype=torch.bool, device="cuda")
        mask[idle] = True
    f = lambda a: m(a, a, a, key_padding_mask=mask, incremental_state=st)[0]         # noqa: E731
    m(x[:P0], x[:P0], x[:P0], incremental_state=st)
    xr = x if order is None else x[:, order]
    xin = x[P0:P0 + 1].clone()
    rows = []
    if how == "eager":
        g = None
        rows.append(f(xin).clone())
    else:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            rows.append(f(xin).clone())
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            yout = f(xin)
    for t in range(P0 + 1, T):
        if reorder is not None and t == reorder:
            m.reorder_incremental_state(st, order)
        xin.copy_((xr if reorder is not None and t >= reorder else x)[t:t + 1])
        if g is None:
            rows.append(f(xin).clone())
        else:
            g.replay()
            rows.append(yout.clone())
    torch.cuda.synchronize()
    return torch.cat(rows, 0), st


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", ["plain", "reorder", "per_seq_idle"])
def test_captured_split_step_replays_equal_split_eager(dtype, mode):
    """Prefill 23 tokens, then 176 replays of one captured 1-token split step on a ring of 64 slots (w = 32, r = 4): the ring
    is lapped more than twice.  Bit for bit the eagerly decoded split rows; with a beam reorder at token 109; with per-sequence
    counts and a row that sits every replay out."""
    _skip_f32(dtype)
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(71)
    T, B, P0 = 200, 3, 23
    x = torch.randn(T, B, 256, device="cuda")
    kw = dict(landmark_splits=3)
    if mode == "reorder":
        kw.update(reorder=109, order=torch.tensor([2, 0, 0], device="cuda"))
    elif mode == "per_seq_idle":
        kw.update(per_sequence=True, idle=1)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eager, est = _run(m, x, P0, dtype, "eager", **kw)
        got, gst = _run(m, x, P0, dtype, "replay", **kw)
        full = None
        if mode == "plain":
            full, _ = m(x, x, x)
        zero = m._project_out(torch.zeros(1, B, 256, dtype=m._get_input_buffer(gst)["qkv"].dtype, device="cuda"), torch.float32)[0]
    assert _bits(got, eager), (got.float() - eager.float()).abs().max().item()
    eb, gb = m._get_input_buffer(est), m._get_input_buffer(gst)
    assert gb["qkv"].shape[1] == 64 and T - P0 >= 2 * 64 and gb["split_ws"].shape[3] == 3
    for k in STATE_ROWS:
        assert _bits(eb[k], gb[k]), k
    assert not m.static_decoding_overflowed(gst) and not m.static_decoding_overflowed(est)
    want = [T, P0, T] if mode == "per_seq_idle" else [T] * B
    assert m.decoding_positions(gst).tolist() == want
    if full is not None:
        _check_full(got, full[P0:], dtype)
    if mode == "per_seq_idle":                                   # the idle row: out_proj of a zero row, every replay
        assert all(torch.equal(row[1].float(), zero[1].float()) for row in got)


# ---- 5. bytes -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_seq"])
def test_a_split_state_is_the_plain_state_plus_its_workspace(kind, per):
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    B, T, P = 3, 500, 5
    plain = _init(m, kind, B, T, torch.bfloat16, per_sequence=per)
    one = _init(m, kind, B, T, torch.bfloat16, per_sequence=per, landmark_splits=1)
    split = _init(m, kind, B, T, torch.bfloat16, per_sequence=per, landmark_splits=P)
    ws = m._get_input_buffer(split)["split_ws"]
    assert ws.shape == (B, 4, 8, P, 64 + 4) and ws.dtype == torch.float32 and ws.data_ptr() % 16 == 0
    assert set(m._get_input_buffer(split)) == set(m._get_input_buffer(plain)) | {"split_ws"}
    assert set(m._get_input_buffer(one)) == set(m._get_input_buffer(plain))
    assert m.decoding_state_nbytes(one) == m.decoding_state_nbytes(plain)
    assert m.decoding_state_nbytes(split) == m.decoding_state_nbytes(plain) + B * 4 * 8 * P * 68 * 4
    assert m.get_incremental_state(split, "attn_static")["landmark_splits"] == P
    assert m.get_incremental_state(plain, "attn_static")["landmark_splits"] == 1
    # a beam reorder leaves the workspace alone
    ws.copy_(torch.arange(ws.numel(), device="cuda").view_as(ws))
    kept = ws.clone()
    m.reorder_incremental_state(split, torch.tensor([2, 0, 0], device="cuda"))
    assert torch.equal(ws, kept)
    if per:
        m.reset_decoding_rows(split, [1])
        assert torch.equal(ws, kept)
