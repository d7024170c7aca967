"""-m gpu: `compact_landmarks=True` of static / rolling incremental decoding (csrc/ea_ceva_decode.hip, the ceva_*_l16 kernels).

A bf16 or fp16 state made with the option keeps rf_k_bar and beta in its own dtype; its steps run ea_ceva_sdecode_close_l16,
ea_ceva_sdecode_attn_l16 and ea_ceva_sdecode_attn_split_l16.  Checked here: the attn kernels against the fp64 restatement of
test_gpu_ceva_decode.py on the same (rounded) landmark operands, close against its fp32 twin -- whose rows it must
reproduce rounded once, bit for bit -- and against fp64, prefix consistency of the module next to a plain state, the option
with `per_sequence`, `landmark_splits` and `hold_projections`, capture and replay, the launches of a step, and the bytes."""
import ctypes
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import ceva_decoding                                                                     # noqa: E402
from ceva_decoding import OLD, STATIC, _Calls, _captured_run, _check_full, _ctx, _geometry   # noqa: E402
from test_gpu_causal_eva import RECIPE, _build                                           # noqa: E402
from test_gpu_ceva_decode import _bound, _io, _ref_attn, _ref_close, _views              # noqa: E402
from test_gpu_ceva_split_decode import SPLIT, SPLIT_CASES, _pad_flags, _to_ring          # noqa: E402

DT16 = [torch.bfloat16, torch.float16]
IDS16 = ["bf16", "fp16"]
KINDS = ["static", "rolling"]
COMPACT = ("ea_ceva_sdecode_append", "ea_ceva_sdecode_close_l16", "ea_ceva_sdecode_attn_l16", "ea_ceva_sdecode_advance")
COMPACT_SPLIT = COMPACT[:2] + ("ea_ceva_sdecode_attn_split_l16", "ea_ceva_sdecode_merge") + COMPACT[3:]
TWINS = ("ea_ceva_sdecode_close", "ea_ceva_sdecode_attn", "ea_ceva_sdecode_attn_split")


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _landmarks(B, h, L, d, dtype, g):
    """Landmark rows made in fp32 and rounded to the state's dtype: what the kernel is handed (device)."""
    return [torch.randn(B, h, L, d, generator=g).to(dtype).cuda() for _ in range(2)]


def _sgeom(nv, dtype, B, h, d, w, e, r, T, cap, ring, bias, pos, status, ntok=None, adaptive=1):
    return nv.ea_ceva_sdec_geom(B, h, d, _io(dtype), w, e, r, T, cap, adaptive, 0 if bias is None else 1, ring, pos.data_ptr(),
                                status.data_ptr(), None if ntok is None else ntok.data_ptr())


# ---- 1. attn_l16 against the fp64 restatement on the same operands --------------------------------------------------------------
# (d, w, e, r, t0, T)
ATTN_CASES = [
    (64, 32, 0, 4, 1, 2),                          # no landmark yet
    (64, 32, 0, 4, 5, 1),                          # one landmark
    (64, 32, 0, 4, 1292, 1),                       # 323 landmarks = five full tiles and a tile of 3
    (128, 128, 0, 4, 2400, 1),                     # 600 landmarks at the LM head size
    (64, 32, 32, 8, 60, 9),                        # extension across a boundary, two query groups
    (32, 16, 16, 8, 3, 4),
    (128, 64, 0, 8, 0, 150),                       # a prefill
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("case", ATTN_CASES, ids=["d%d_w%d_e%d_r%d_t%d_T%d" % c for c in ATTN_CASES])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_attn_l16_kernel_against_fp64(dtype, case, with_bias):
    """The landmark rows the kernel reads are the rows the restatement gets, widened: the only roundings are the output's, as
    for the twin, and the bound is the twin's."""
    from efficient_attention import _native as nv
    d, w, e, r, t0, T = case
    B, h = 2, 2
    cap = ((t0 + T + w - 1) // w) * w
    L = max((t0 + T) // r, 1)
    g = torch.Generator().manual_seed(7 * t0 + d + T)
    qkv = torch.randn(B, cap, 3, h, d, generator=g).to(dtype).cuda()
    lk, lv = _landmarks(B, h, L, d, dtype, g)
    pad, g = _pad_flags(B, cap, t0, T, w, e)
    bias = torch.randn(w, w + e, generator=g) if with_bias else None
    bias_d = None if bias is None else bias.float().cuda()
    pad_d = pad.to(torch.uint8).cuda()
    q, k, v = _views(qkv)
    out = torch.full((B, h, T, d), 7.0, dtype=dtype, device="cuda")
    pos = torch.tensor([t0], dtype=torch.int32, device="cuda")
    status = torch.zeros_like(pos)
    geom = _sgeom(nv, dtype, B, h, d, w, e, r, T, cap, 0, bias, pos, status)
    tq, tk, tv, tl, tb, to = [nv.t4(t) for t in (q, k, v, lk, lv, out)]
    nv.call("ea_ceva_sdecode_attn_l16", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(pad_d),
            nv.ptr(bias_d), ctypes.byref(tl), ctypes.byref(tb), ctypes.byref(to), nv.stream())
    torch.cuda.synchronize()
    assert lk.dtype == dtype and lv.dtype == dtype and status.item() == 0 and pos.item() == t0
    ref = _ref_attn(*[t.double().cpu() for t in (q, k, v)], pad, None if bias is None else bias.double(),
                    lk.double().cpu(), lv.double().cpu(), t0, T, w, e, r)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    live = ~pad[:, t0:t0 + T].view(B, 1, T, 1)                   # padded query rows: finite only
    err = (got - ref).abs()
    print(case, dtype, "max |d| %.3e, max bound %.3e, max |ref| %.3e" % ((err * live).max().item(), _bound(dtype, ref).max().item(),
                                                                         ref.abs().max().item()))
    excess = (err - _bound(dtype, ref)) * live
    assert excess.max().item() <= 0, (case, dtype, excess.max().item(), ref.abs().max().item())


# ---- 2. attn_split_l16 + merge ------------------------------------------------------------------------------------------------
L16_SPLIT_CASES = [c for c in SPLIT_CASES if c[0] in ("L0", "L323_P4", "parts_gt_tiles", "ext_boundary", "ring_ext", "max_parts")]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("case", L16_SPLIT_CASES, ids=[c[0] for c in L16_SPLIT_CASES])
def test_split_l16_kernels_against_fp64(dtype, case):
    from efficient_attention import _native as nv
    assert len(L16_SPLIT_CASES) == 6
    name, d, w, e, r, t0, T, P, R, with_bias = case
    B, h = 2, 2
    cap = ((t0 + T + w - 1) // w) * w
    g = torch.Generator().manual_seed(len(name) * 7 + d)
    lin = torch.randn(B, cap, 3, h, d, generator=g).to(dtype)
    lk, lv = _landmarks(B, h, cap // r, d, dtype, g)
    pad, g = _pad_flags(B, cap, t0, T, w, e)
    bias = torch.randn(w, w + e, generator=g) if with_bias else None
    bias_d = None if bias is None else bias.float().cuda()
    if R:
        assert R % w == 0 and R >= w + e + T and t0 >= R
        qkv, pad_d = _to_ring(lin, R, t0 + T).cuda(), _to_ring(pad, R, t0 + T).to(torch.uint8).cuda()
    else:
        qkv, pad_d = lin.cuda(), pad.to(torch.uint8).cuda()
    pos = torch.tensor([t0], dtype=torch.int32, device="cuda")
    status = torch.zeros_like(pos)
    q, k, v = _views(qkv)
    out = torch.full((B, h, T, d), 7.0, dtype=dtype, device="cuda")
    ws = torch.full((B, h, 8, P, d + 4), float("nan"), device="cuda")
    geom = _sgeom(nv, dtype, B, h, d, w, e, r, T, cap, R, bias, pos, status)
    tq, tk, tv, tl, tb, to = [nv.t4(t) for t in (q, k, v, lk, lv, out)]
    nv.call("ea_ceva_sdecode_attn_split_l16", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv),
            nv.ptr(pad_d), nv.ptr(bias_d), ctypes.byref(tl), ctypes.byref(tb), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    nv.call("ea_ceva_sdecode_merge", ctypes.byref(geom), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    torch.cuda.synchronize()
    ql, kl, vl = [lin[:, :, i].transpose(1, 2).double() for i in range(3)]
    ref = _ref_attn(ql, kl, vl, pad, None if bias is None else bias.double(), lk.double().cpu(), lv.double().cpu(), t0, T, w, e, r)
    got = out.double().cpu()
    assert torch.isfinite(got).all() and status.item() == 0
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
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
def test_split_l16_kernels_with_per_sequence_counts(dtype):
    """append -> attn_split_l16 -> merge with ntok over a ring of 96: one row across a window boundary, one that sits the
    step out (zero rows), one whose step would pass cap (status 1, NaN rows, nothing of it written) -- the kernels' own handled
    refusal.  The live rows against the fp64 restatement of each sequence alone."""
    from efficient_attention import _native as nv
    d, w, e, r, T, P, B, h, R = 64, 32, 0, 4, 5, 4, 4, 2, 96
    cap = 320
    counts, own = [125, 290, 200, cap - 2], [5, 3, 0, 5]         # 125..129 pass the boundary at 128; 318 + 5 > cap
    g = torch.Generator().manual_seed(123)
    lin = torch.randn(B, cap + T, 3, h, d, generator=g).to(dtype)
    lk, lv = _landmarks(B, h, cap // r, d, dtype, g)
    pad = torch.rand(B, cap + T, generator=g) < 0.2
    bias = torch.randn(w, w + e, generator=g)
    for b in range(B):
        pad[b, counts[b]:] = False                               # (append stores its tokens unflagged)
    qkv, pad_d = torch.zeros(B, R, 3, h, d, dtype=dtype), torch.zeros(B, R, dtype=torch.uint8)
    for b in range(B):                                           # the tokens before each row's count
        n = torch.arange(max(counts[b] - R, 0), counts[b])
        qkv[b, n % R], pad_d[b, n % R] = lin[b, n], pad[b, n].to(torch.uint8)
    qkv, pad_d = qkv.cuda(), pad_d.cuda()
    new = torch.stack([lin[b, counts[b]:counts[b] + T] for b in range(B)], 1).contiguous().cuda()       # [T, B, 3, h, d]
    flags = torch.tensor([[t >= own[b] for t in range(T)] for b in range(B)], dtype=torch.uint8, device="cuda")
    pos = torch.tensor(counts, dtype=torch.int32, device="cuda")
    status, ntok = torch.zeros_like(pos), torch.full_like(pos, -1)
    before = (qkv.clone(), pad_d.clone(), lk.clone(), lv.clone())
    bias_d = bias.float().cuda()
    geom = _sgeom(nv, dtype, B, h, d, w, e, r, T, cap, R, bias_d, pos, status, ntok)
    nv.call("ea_ceva_sdecode_append", ctypes.byref(geom), nv.ptr(new), nv.ptr(flags), nv.ptr(qkv), nv.ptr(pad_d), nv.stream())
    q, k, v = _views(qkv)
    out = torch.full((B, h, T, d), 7.0, dtype=dtype, device="cuda")
    ws = torch.full((B, h, 8, P, d + 4), float("nan"), device="cuda")
    tq, tk, tv, tl, tb, to = [nv.t4(t) for t in (q, k, v, lk, lv, out)]
    nv.call("ea_ceva_sdecode_attn_split_l16", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv),
            nv.ptr(pad_d), nv.ptr(bias_d), ctypes.byref(tl), ctypes.byref(tb), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    nv.call("ea_ceva_sdecode_merge", ctypes.byref(geom), ctypes.byref(to), P, nv.ptr(ws), nv.stream())
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 1] and ntok.tolist() == own and pos.tolist() == counts
    assert torch.isnan(out[3]).all() and torch.isnan(ws[3]).all()            # refused: NaN rows, no partial
    assert torch.equal(qkv[3], before[0][3]) and torch.equal(pad_d[3], before[1][3])
    assert (out[2] == 0).all() and torch.isnan(ws[2]).all()                  # sits out: zero rows, no partial
    assert torch.equal(qkv[2], before[0][2])
    assert _bits(lk, before[2]) and _bits(lv, before[3])                     # attn reads the landmark rows only
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


# ---- 3. close_l16: the fp32 twin's rows, rounded once -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("adaptive", [1, 0], ids=["qk", "no-ln"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_close_l16_kernel_rounds_the_twins_rows_once(dtype, adaptive, d):
    """Chunks 1 .. 6 of chunk length 8 closed in one launch (the setup of test_decode_close_kernel_against_fp64 on a static
    step); chunk 2 is fully padded, chunk 4 in part.  (a) every closed row equals the fp32 twin's row `.to(dtype)`, bit for
    bit; (b) against fp64: half an ulp of the one rounding, 2^-8 (bf16) or 2^-11 (fp16) of |ref|, plus the twin's fp32 bound of
    1e-5 max |ref|; (c) the fully padded chunk's beta is exactly 0; (d) rows of chunks outside the range keep their bits."""
    from efficient_attention import _native as nv
    B, h, r, w = 2, 3, 8, 32
    cap, t0, T = 64, 9, 47                                    # tokens 9 .. 55 complete chunks 1 .. 6
    g = torch.Generator().manual_seed(d + adaptive)
    qkv = torch.randn(B, cap, 3, h, d, generator=g).to(dtype).cuda()
    lk32, lv32 = [torch.randn(B, h, cap // r, d, generator=g).cuda() for _ in range(2)]
    lk, lv = lk32.to(dtype), lv32.to(dtype)
    lk0, lv0 = lk.clone(), lv.clone()
    pad = torch.zeros(B, cap, dtype=torch.bool)
    pad[:, 16:24] = True
    pad[1, 32:37] = True
    pad_d = pad.to(torch.uint8).cuda()
    g = torch.Generator().manual_seed(5 + d)
    params = []
    for _ in range(2):
        params += [0.2 * torch.randn(d, d, generator=g), torch.randn(d, generator=g)]
        if adaptive:
            params += [1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)]
    params = [p.cuda().contiguous() for p in params]
    q, k, v = _views(qkv)
    c0, c1 = t0 // r, (t0 + T) // r - 1
    assert (c0, c1) == (1, 6)
    pos = torch.tensor([t0], dtype=torch.int32, device="cuda")
    status = torch.zeros_like(pos)
    geom = _sgeom(nv, dtype, B, h, d, w, 0, r, T, cap, 0, None, pos, status, adaptive=adaptive)
    mp = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
    tq, tk, tv = [nv.t4(t) for t in (q, k, v)]
    for entry, a, b in (("ea_ceva_sdecode_close", lk32, lv32), ("ea_ceva_sdecode_close_l16", lk, lv)):
        ta, tb = nv.t4(a), nv.t4(b)
        nv.call(entry, ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(pad_d), mp,
                ctypes.byref(ta), ctypes.byref(tb), nv.stream())
    torch.cuda.synchronize()
    assert lk.dtype == dtype and lv.dtype == dtype and status.item() == 0
    qd, kd, vd = [t.double().cpu() for t in (q, k, v)]
    half_ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    worst = 0.0
    for c in range(cap // r):
        if c0 <= c <= c1:
            assert _bits(lk[:, :, c], lk32[:, :, c].to(dtype)) and _bits(lv[:, :, c], lv32[:, :, c].to(dtype)), c      # (a)
            rk, beta = _ref_close(qd, kd, vd, pad, params, c, r, adaptive)
            for got, ref in ((lk[:, :, c], rk), (lv[:, :, c], beta)):                                                # (b)
                excess = ((got.double().cpu() - ref).abs() - half_ulp * ref.abs() - 1e-5 * ref.abs().max()).max().item()
                worst = max(worst, ((got.double().cpu() - ref).abs() / ref.abs().max().clamp_min(1e-30)).max().item())
                assert excess <= 0, (c, excess, ref.abs().max().item())
            if c == 2:
                assert lv[:, :, c].float().abs().max().item() == 0                                                   # (c)
        else:                                                                                                        # (d)
            assert _bits(lk[:, :, c], lk0[:, :, c]) and _bits(lv[:, :, c], lv0[:, :, c])
    print("close_l16", dtype, d, adaptive, "max |d| / max |ref| %.3e (half an ulp: %.3e)" % (worst, half_ulp))


# ---- the module on compact states ---------------------------------------------------------------------------------------------
def _init(m, kind, B, T, dtype, S=None, **opt):
    st = {}
    if kind == "static":
        m.init_static_decoding(st, B, T, dtype, "cuda", **opt)
    else:
        m.init_rolling_decoding(st, B, T, dtype, "cuda", max_step_tokens=S, **opt)
    return st


def _decode(m, x, steps, kind, dtype, pad=None, calls=None, **opt):
    """x [T, B, C] in steps of the given sizes, then single tokens (ceva_decoding._decode with the state's options; the mask
    alternates between fairseq's two shapes) -> (per-step rows, state)."""
    T, B = x.shape[:2]
    st, rows, t = _init(m, kind, B, T, dtype, **opt), [], 0
    for i, n in enumerate(list(steps) + [1] * T):
        if t >= T:
            break
        n = min(n, T - t)
        kpm = None if pad is None else (pad[:, t:t + n] if i % 2 == 0 else pad[:, :t + n])
        if calls is not None:
            calls.step()
        rows.append(m(x[t:t + n], x[t:t + n], x[t:t + n], key_padding_mask=kpm, incremental_state=st)[0])
        t += n
    return rows, st


def _same_state_but_rounded_landmarks(m, pst, cst, dtype):
    """The compact state next to the plain one fed the same steps: token rows, flags and counts bit for bit, the landmark rows
    the plain ones rounded once."""
    pb, cb = m._get_input_buffer(pst), m._get_input_buffer(cst)
    assert set(pb) == set(cb)
    for k in ("qkv", "pad", "pos"):
        assert _bits(pb[k], cb[k]), k
    for k in ("rf_k_bar", "beta"):
        assert pb[k].dtype == torch.float32 and cb[k].dtype == dtype
        assert _bits(pb[k].to(dtype), cb[k]), k
    assert cb["rf_k_bar"].float().abs().max().item() > 0          # (chunks were closed)


# ---- 4. prefix consistency, next to the plain state -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", ["recipe_d64", "recipe_d128", "overlap_d64", "many_chunks"])
def test_compact_decoding_equals_full_forward_and_rounds_the_plain_landmarks(dtype, kind, variant):
    """A first step without a visible landmark (bitwise the plain state's), a prompt, a few multi-token steps, then single
    tokens; overlap_d64 with left-padded positions.  Outputs within the project's 2e-2 of the full forward."""
    aa, embed, heads, T, B = _geometry(variant)
    m = _build(embed, heads, aa)
    r = aa["chunk_size"]
    steps = (3, T - 60, 7, 3, 9)
    assert steps[0] < r
    torch.manual_seed(101)
    x = torch.randn(T, B, embed, device="cuda")
    pad = live = None
    if variant == "overlap_d64":
        pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        pad[1, :2 * r + 3] = True
        live = (~pad).t().unsqueeze(-1).float()
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x, key_padding_mask=pad)
        plain, pst = _decode(m, x, steps, kind, dtype, pad=pad)
        comp, cst = _decode(m, x, steps, kind, dtype, pad=pad, compact_landmarks=True)
    assert len(comp) == len(plain) == 5 + (60 - 3 - 7 - 3 - 9)
    got = torch.cat(comp, 0)
    assert torch.isfinite(got).all()
    print(variant, kind, dtype, end=" ")
    _check_full(got, full, dtype, live)
    _same_state_but_rounded_landmarks(m, pst, cst, dtype)
    assert int(m._get_input_buffer(cst)["pos"].item()) == T and not m.static_decoding_overflowed(cst)
    assert _bits(plain[0], comp[0])                              # 3 tokens (many_chunks: r = 4): no landmark visible yet
    d = (got.float() - torch.cat(plain, 0).float()).abs().max().item()
    print("compact vs plain rows, max |d|: %.3e of max |full| %.3e" % (d, full.float().abs().max().item()))


# ---- 5. combinations and capture ------------------------------------------------------------------------------------------------
def _ragged_run(m, seqs, dtype, kind, ragged, restart=None, **opt):
    """B rows with their own token sequences seqs[b] [T_b, C].  One right-padded prompt step (ragged: rows 1, 2 shorter), then
    single-token steps while any row has tokens left; a row without a token, or (ragged) row 1 during the first 5 single steps, sits
    the step out.  restart = (row, sequence): once that row has finished, reset_decoding_rows and the new sequence.  Without
    `ragged` all rows have equal lengths and no mask is passed.  -> per-row output rows (lists of [n, C]), state."""
    B, C = len(seqs), seqs[0].shape[1]
    cap = max(s.shape[0] for s in seqs) + (restart[1].shape[0] if restart else 0)
    st = _init(m, kind, B, cap, dtype, **opt)
    seqs, cur, outs = list(seqs), [0] * B, [[] for _ in range(B)]
    first = [40, 17, 29][:B] if ragged else [40] * B
    single, restarted = 0, False

    def step(take):
        n = max(take)
        x = torch.zeros(n, B, C, device="cuda")
        mask = torch.ones(B, n, dtype=torch.bool, device="cuda")
        for b in range(B):
            x[:take[b], b] = seqs[b][cur[b]:cur[b] + take[b]]
            mask[b, :take[b]] = False
        y = m(x, x, x, key_padding_mask=mask if ragged else None, incremental_state=st)[0]
        for b in range(B):
            outs[b].append(y[:take[b], b])
            cur[b] += take[b]
    step(first)
    while True:
        left = [seqs[b].shape[0] - cur[b] for b in range(B)]
        if restart and not restarted and left[restart[0]] == 0:
            m.reset_decoding_rows(st, [restart[0]])
            seqs[restart[0]], cur[restart[0]], restarted = restart[1], 0, True
            outs.append(outs[restart[0]])                         # (the finished sequence's rows move to the end)
            outs[restart[0]] = []
            continue
        if not any(left):
            break
        take = [1 if n else 0 for n in left]
        if ragged and single < 5:
            take[1] = 0
        single += 1
        step(take)
    return [torch.cat(o, 0) for o in outs], st


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("combo", ["per_sequence", "landmark_splits", "hold_projections", "all_three"])
def test_compact_landmarks_combines_with_the_other_options(dtype, kind, combo):
    """many_chunks geometry (w = 32, e = 32, r = 4).  per_sequence: a ragged right-padded prompt, a row idle for five steps, a
    finished row restarted by reset_decoding_rows.  Each row within the 2e-2 bound of the full forward of its own sequence;
    next to a state with the same options and fp32 landmark rows: token rows, flags and counts bit for bit, landmark rows
    the fp32 ones rounded once."""
    aa = dict(RECIPE, overlap_window=True, window_size=32, chunk_size=4)
    C, B = 256, 3
    m = _build(C, 4, aa)
    opt = {"per_sequence": dict(per_sequence=True), "landmark_splits": dict(landmark_splits=4),
           "hold_projections": dict(hold_projections=True),
           "all_three": dict(per_sequence=True, landmark_splits=4, hold_projections=True)}[combo]
    ragged = "per_sequence" in opt
    torch.manual_seed(103)
    lens = [90, 70, 52] if ragged else [80] * B
    seqs = [torch.randn(n, C, device="cuda") for n in lens]
    restart = (2, torch.randn(37, C, device="cuda")) if ragged else None
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rows_p, pst = _ragged_run(m, seqs, dtype, kind, ragged, restart, **opt)
        rows_c, cst = _ragged_run(m, seqs, dtype, kind, ragged, restart, **opt, compact_landmarks=True)
        every = seqs[:2] + ([restart[1], seqs[2]] if ragged else seqs[2:])          # (the order _ragged_run returns)
        fulls = [m(s.unsqueeze(1), s.unsqueeze(1), s.unsqueeze(1))[0][:, 0] for s in every]
    assert len(rows_c) == len(fulls) == (4 if ragged else 3)
    for i, (got, full) in enumerate(zip(rows_c, fulls)):
        assert got.shape == full.shape and torch.isfinite(got).all(), i
        print(combo, kind, dtype, "sequence", i, end=" ")
        _check_full(got, full, dtype)
    _same_state_but_rounded_landmarks(m, pst, cst, dtype)
    want = [90, 70, 37] if ragged else [80] * B
    assert m.decoding_positions(cst).tolist() == want and not m.static_decoding_overflowed(cst)
    static = m.get_incremental_state(cst, "attn_static")
    assert static["compact_landmarks"] is True and "compact_landmarks" not in m.get_incremental_state(pst, "attn_static")


def _compact_init(monkeypatch, **more):
    """ceva_decoding._captured_run makes its states with ceva_decoding._init: here with the option."""
    monkeypatch.setattr(ceva_decoding, "_init", lambda m, kind, B, T, dtype, S=None: _init(m, kind, B, T, dtype, S,
                                                                                           compact_landmarks=True, **more))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("splits", [1, 4], ids=["unsplit", "split4"])
def test_captured_compact_step_replays_equal_compact_eager(dtype, splits, monkeypatch):
    """Prefill 23 tokens, then 176 replays of one captured 1-token step on a ring of 64 slots (w = 32, r = 4): the ring is
    lapped more than twice, 44 chunks close.  Bit for bit the eagerly decoded compact rows."""
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(107)
    T, B, P = 200, 2, 23
    x = torch.randn(T, B, 256, device="cuda")
    _compact_init(monkeypatch, landmark_splits=splits)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, _ = m(x, x, x)
        eager, est = _decode(m, x, (P,), "rolling", dtype, compact_landmarks=True, landmark_splits=splits)
        eager = torch.cat(eager, 0)
        got, states = _captured_run([m], x, P, dtype)           # (one residual layer: the rows are x + attn(x))
    eb, gb = m._get_input_buffer(est), m._get_input_buffer(states[0])
    assert gb["qkv"].shape[1] == 64 and T - P >= 2 * 64 and gb["rf_k_bar"].dtype == dtype and gb["beta"].dtype == dtype
    assert ("split_ws" in gb) == (splits > 1)
    assert torch.equal(got, eager[P:] + x[P:]), (got.float() - (eager[P:] + x[P:]).float()).abs().max().item()
    for k in ("qkv", "pad", "rf_k_bar", "beta", "pos"):
        assert _bits(eb[k], gb[k]), k
    _check_full(eager[P:], full[P:], dtype)
    assert not m.static_decoding_overflowed(states[0]) and int(gb["pos"].item()) == T


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("graph_reorder", [False, True], ids=["eager_reorder", "captured_reorder"])
def test_beam_reorder_between_compact_replays(dtype, graph_reorder, monkeypatch):
    """reorder_incremental_state on a compact rolling state, mid-sequence and after the ring has wrapped, outside or inside a
    graph: the 16-bit landmark rows are permuted with the rest.  The replays that follow equal the same run on the compact
    static state, bit for bit, and the full forward of the reordered batch within the bound."""
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(109)
    T, B, P, at = 180, 3, 11, 109
    x = torch.randn(T, B, 256, device="cuda")
    order = torch.tensor([2, 0, 0], device="cuda")
    _compact_init(monkeypatch)
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref, sstates = _captured_run([m], x, P, dtype, kind="static", reorder=at, order=order, graph_reorder=graph_reorder)
        sbuf = {k: v.clone() for k, v in m._get_input_buffer(sstates[0]).items() if torch.is_tensor(v)}
        got, states = _captured_run([m], x, P, dtype, reorder=at, order=order, graph_reorder=graph_reorder)
        xr = x[:, order]                                         # what each row has seen once the state is permuted
        full, _ = m(xr, xr, xr)
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max().item()
    buf = m._get_input_buffer(states[0])
    R = buf["qkv"].shape[1]
    assert R == 64 and int(buf["pos"].item()) == T and buf["rf_k_bar"].dtype == dtype
    assert _bits(buf["rf_k_bar"], sbuf["rf_k_bar"]) and _bits(buf["beta"], sbuf["beta"])
    assert torch.equal(buf["rf_k_bar"][1], buf["rf_k_bar"][2])   # rows 1 and 2 both continue old row 0 ...
    assert not torch.equal(buf["rf_k_bar"][0], buf["rf_k_bar"][1])
    _check_full(got[at - P:] - xr[at:], full[at:], dtype)


# ---- 6. launches ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_seq"])
def test_compact_step_launches(kind, per):
    """A compact step: append, close_l16, attn_l16 (or attn_split_l16 + merge for a step of at most 8 tokens on a split
    state), advance -- eagerly, for the pieces of a prompt and under capture -- never the fp32 twins nor the old cores.  A
    default state's steps are today's sequences."""
    dtype = torch.bfloat16
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    torch.manual_seed(113)
    T, B = 100, 2
    x = torch.randn(T, B, 256, device="cuda")
    steps = (7, 1, 8, 9, 40, 2, 1, 30, 1)                        # (a rolling state, S = 32, cuts the 40 into 32 + 8)
    opt = dict(per_sequence=True) if per else {}

    def core(got):
        assert not [c for c in got if c in OLD], got
        return [c for c in got if not (c.startswith("ea_linear") or c == "ea_multi_cast")]

    runs, captured = {}, {}
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, o in (("default", {}), ("default4", dict(landmark_splits=4)), ("off", dict(compact_landmarks=False)),
                        ("compact", dict(compact_landmarks=True)), ("compact4", dict(compact_landmarks=True, landmark_splits=4))):
            with _Calls() as calls:
                rows, st = _decode(m, x, steps, kind, dtype, calls=calls, **opt, **o)
                if name.startswith("compact"):                   # ... and a 1-token step on a fresh state, captured
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
                    captured[name] = (core(calls.steps.pop()), core(calls.steps.pop()), g, st2)
            runs[name] = (rows, [core(s) for s in calls.steps])
        for name in captured:
            captured[name][2].replay()
        torch.cuda.synchronize()
    sizes = list(steps) + [1] * (T - sum(steps))
    pieces = lambda n: -(-n // 32) if kind == "rolling" else 1   # noqa: E731  (the pieces of a larger step)
    for name, one, short in (("default", STATIC, STATIC), ("off", STATIC, STATIC), ("default4", STATIC, SPLIT),
                             ("compact", COMPACT, COMPACT), ("compact4", COMPACT, COMPACT_SPLIT)):
        got = runs[name][1]
        assert len(got) == len(sizes), name
        for n, calls_of in zip(sizes, got):
            assert calls_of == list(short if n <= 8 else one * pieces(n)), (name, n, calls_of)
        if name.startswith("compact"):
            assert not [c for s in got for c in s if c in TWINS], name
    assert captured["compact"][0] == list(COMPACT) == captured["compact"][1]
    assert captured["compact4"][0] == list(COMPACT_SPLIT) == captured["compact4"][1]
    for name in captured:
        assert m.decoding_positions(captured[name][3]).tolist() == [2] * B
    assert all(_bits(a, b) for a, b in zip(runs["default"][0], runs["off"][0]))


# ---- 7. bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("kind", KINDS)
def test_a_compact_state_is_smaller_by_half_its_landmark_rows(dtype, kind, monkeypatch):
    aa = dict(RECIPE, window_size=32, chunk_size=4)
    m = _build(256, 4, aa)
    B, T, h, d, r = 3, 500, 4, 64, 4
    cap = -(-T // 32) * 32
    plain = _init(m, kind, B, T, dtype)
    off = _init(m, kind, B, T, dtype, compact_landmarks=False)
    compact = _init(m, kind, B, T, dtype, compact_landmarks=True)
    pb, cb = m._get_input_buffer(plain), m._get_input_buffer(compact)
    assert set(pb) == set(cb) == set(m._get_input_buffer(off))
    assert m.decoding_state_nbytes(off) == m.decoding_state_nbytes(plain)
    assert m.decoding_state_nbytes(plain) - m.decoding_state_nbytes(compact) == 2 * B * h * (cap // r) * d * 2
    for k in ("rf_k_bar", "beta"):
        assert cb[k].dtype == dtype and pb[k].dtype == torch.float32 and cb[k].shape == pb[k].shape == (B, h, cap // r, d)
        assert cb[k].data_ptr() % 16 == 0
    assert cb["qkv"].dtype == dtype
    from efficient_attention import _f32
    monkeypatch.setattr(_f32, "ENABLED", True)                   # (refused before anything is allocated, whatever the switch)
    with pytest.raises(ValueError, match="compact_landmarks") as got:
        _init(m, kind, B, T, torch.float32, compact_landmarks=True)
    assert "fidelity path" in str(got.value)
