"""-m gpu: incremental decoding of CausalEVAttention on its own HIP kernels (csrc/ea_ceva_decode.hip).

A decoding step runs one ea_ceva_decode_close (the landmarks of every chunk the step completes) and one ea_ceva_decode_attn
(the outputs of all its tokens), both in fp32 arithmetic on rows of the cache's dtype.  Checked here: fp32 decoding equals the
fp32 full forward at fp32 tolerances (no rounding to bf16 anywhere), 16-bit decoding launches each kernel once per step and
matches the full forward, both kernels against an fp64 restatement written below, and the guards of the old behaviour."""
import ctypes
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import ceva_decoding                                     # noqa: E402
from ceva_decoding import F32_TOL, OLD, _Calls, _err, _geometry      # noqa: E402
from test_gpu_causal_eva import RECIPE, _build          # noqa: E402


def _decode(m, x, steps, calls, pad=None):
    """Decode x [T, B, C] on a fresh dynamic state in steps of the given sizes (then single tokens); -> [T, B, C]."""
    m.init_incremental_state()
    rows, state = ceva_decoding._decode(m, x, steps, "dynamic", None, pad, calls=calls)
    return torch.cat(rows, 0), state

def _fp32_checks(calls, rec):
    from efficient_attention import _ops
    assert not [w for w in rec if "rounded to bf16" in str(w.message)]
    assert not _ops._FP32_WARNED[0]
    got = calls.all()
    assert "ea_ceva_decode_attn" in got, sorted(set(got))
    assert not [c for c in got if c in OLD], sorted(set(got))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["recipe_d64", "recipe_d128", "overlap_d64", "no_rpe_noln", "many_chunks"])
def test_fp32_decoding_equals_fp32_full_forward(variant):
    """fp32 activations outside autocast: decoding keeps fp32 end to end and reproduces the fp32 full path row by row at fp32
    tolerances (the 16-bit decoding of earlier builds rounded q, k, v to bf16: about 1e-2)."""
    from efficient_attention import _ops
    aa, embed, heads, T, B = _geometry(variant)
    m = _build(embed, heads, aa)
    torch.manual_seed(11)
    x = torch.randn(T, B, embed, device="cuda")
    _ops._FP32_WARNED[0] = False
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        full, _ = m(x, x, x)
        with _Calls() as calls:
            inc, _ = _decode(m, x, (1, 1, 1, 5, 1, 2, 64, 1, 1, 7), calls)
    assert inc.dtype == torch.float32 and inc.shape == full.shape
    e = _err(inc, full)
    assert e[0] <= F32_TOL[0] and e[1] <= F32_TOL[1], (variant, e)
    _fp32_checks(calls, rec)
    assert "ea_ceva_decode_close" in calls.all()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["recipe_d64", "many_chunks"])
def test_fp32_decoding_with_padded_positions(variant):
    """Left-padded prompts in fp32: two whole padded chunks and part of a third in element 1.  Live rows match the fp32 full
    forward given the same mask; padded query rows are finite."""
    from efficient_attention import _ops
    aa, embed, heads, T, _ = _geometry(variant)
    B = 3
    m = _build(embed, heads, aa)
    r = aa["chunk_size"]
    torch.manual_seed(13)
    x = torch.randn(T, B, embed, device="cuda")
    pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    pad[1, :2 * r + 3] = True
    pad[2, :3] = True
    _ops._FP32_WARNED[0] = False
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        full, _ = m(x, x, x, key_padding_mask=pad)
        with _Calls() as calls:
            inc, _ = _decode(m, x, (1, 1, 6, 1, 20, 1, 2, 64), calls, pad=pad)
    assert torch.isfinite(inc).all()
    e = _err(inc, full, live=(~pad).t().unsqueeze(-1).double())
    assert e[0] <= F32_TOL[0] and e[1] <= F32_TOL[1], (variant, e)
    _fp32_checks(calls, rec)


@pytest.mark.gpu
def test_fp32_decoding_reorders_with_the_beam():
    from efficient_attention import _ops
    aa = dict(RECIPE, window_size=32)
    m = _build(256, 4, aa)
    torch.manual_seed(5)
    x = torch.randn(40, 3, 256, device="cuda")
    order = torch.tensor([2, 0, 0], device="cuda")
    _ops._FP32_WARNED[0] = False
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with _Calls() as calls:
            st = {}
            m.init_incremental_state()
            for t in range(20):
                calls.step()
                m(x[t:t + 1], x[t:t + 1], x[t:t + 1], incremental_state=st)
            m.reorder_incremental_state(st, order)
            xr = x[:, order]
            ys = []
            for t in range(20, 40):
                calls.step()
                ys.append(m(xr[t:t + 1], xr[t:t + 1], xr[t:t + 1], incremental_state=st)[0])
        full, _ = m(xr, xr, xr)
    e = _err(torch.cat(ys, 0), full[20:])
    assert e[0] <= F32_TOL[0] and e[1] <= F32_TOL[1], e
    _fp32_checks(calls, rec)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_decoding_runs_each_kernel_once_per_step(dtype):
    """Under autocast: a 1-token step, a 200-token step that closes 25 chunks, then single tokens and a 7-token step.  Every
    step launches ea_ceva_decode_attn exactly once and ea_ceva_decode_close at most once (once iff it completes a chunk)."""
    aa = dict(RECIPE)
    m = _build(512, 8, aa)
    r = aa["chunk_size"]
    torch.manual_seed(17)
    T, B = 260, 2
    x = torch.randn(T, B, 512, device="cuda")
    steps = (1, 200, 1, 1, 7, 1)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        full, _ = m(x, x, x)
        with _Calls() as calls:
            inc, _ = _decode(m, x, steps, calls)
    assert inc.shape == full.shape
    err = (inc.float() - full.float()).abs().max().item()
    ref = full.float().abs().max().item()
    assert err <= 2e-2 * ref, (err, ref)
    t = 0
    sizes = list(steps) + [1] * T
    for s, got in zip(sizes, calls.steps):
        n = min(s, T - t)
        closes = (t + n) // r - t // r
        assert got.count("ea_ceva_decode_attn") == 1, (t, n, got)
        assert got.count("ea_ceva_decode_close") == (1 if closes else 0), (t, n, got)
        assert not [c for c in got if c in OLD], got
        t += n
    assert (1 + 200) // r - 1 // r == 25                       # the second step closes 25 chunks


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["half", "bfloat16"])
def test_16bit_module_decodes_without_autocast(dtype):
    """fairseq's --fp16 / --bf16 generation converts the model with .half() / .bfloat16() and does not autocast: every parameter,
    the mu networks' included, is 16-bit.  Decoding still closes chunks (on fp32 copies of the mu parameters) and matches the
    full forward of the same weights under autocast."""
    import copy
    aa = dict(RECIPE, window_size=32)
    m32 = _build(256, 4, aa)
    m = copy.deepcopy(m32).to(dtype)
    assert all(p.dtype == dtype for p in m._mu_params())
    torch.manual_seed(21)
    x = torch.randn(70, 2, 256, device="cuda")
    with torch.no_grad():
        with torch.autocast("cuda", dtype=dtype):
            full, _ = m32(x, x, x)
        with _Calls() as calls:
            inc, _ = _decode(m, x.to(dtype), (1, 9, 1, 20, 3), calls)
    assert inc.dtype == dtype and inc.shape == full.shape
    assert sum(s.count("ea_ceva_decode_close") for s in calls.steps) >= 5
    assert torch.isfinite(inc).all()
    err = (inc.float() - full.float()).abs().max().item()
    ref = full.float().abs().max().item()
    assert err <= 2e-2 * ref, (err, ref)


# ---- kernel level: both entry points against an fp64 restatement -----------------------------------------------------------
def _ref_attn(q, k, v, pad, bias, lk, lv, t0, T, w, e, r):
    """fp64 restatement of ea_ceva_decode_attn: q, k, v [B,h,cap,d]; pad [B,cap] bool; bias [w, w+e] or None; lk, lv
    [B,h,L,d] -> out [B,h,T,d]."""
    B, h, cap, d = q.shape
    s = d ** -0.5
    Wk = w + e
    outs = []
    for t in range(t0, t0 + T):
        bk = t // w
        tok = torch.arange(Wk) + bk * w - e
        ok = tok >= 0
        tc = tok.clamp(min=0)
        kk = k[:, :, tc] * ok.view(1, 1, -1, 1)
        vv = v[:, :, tc] * ok.view(1, 1, -1, 1)
        lg = s * torch.einsum("bhd,bhjd->bhj", q[:, :, t], kk)
        if bias is not None:
            lg = lg + bias[t - bk * w].view(1, 1, -1)
        masked = (~ok).view(1, -1) | pad[:, tc] | (tok > t).view(1, -1) | pad[:, t].view(-1, 1)     # [B, Wk]
        lg = lg.masked_fill(masked.view(B, 1, Wk), -5e4)
        nv_ = t // r
        if nv_:
            lg = torch.cat([lg, s * torch.einsum("bhd,bhcd->bhc", q[:, :, t], lk[:, :, :nv_])], -1)
            vv = torch.cat([vv, lv[:, :, :nv_]], 2)
        p = torch.softmax(lg, -1)
        outs.append(torch.einsum("bhj,bhjd->bhd", p, vv))
    return torch.stack(outs, 2)


def _ref_close(q, k, v, pad, params, c, r, adaptive):
    """fp64 restatement of ea_ceva_decode_close for chunk c -> (rf_k_bar [B,h,d], beta [B,h,d])."""
    d = q.shape[-1]
    s = d ** -0.5
    rows = slice(c * r, (c + 1) * r)
    live = (~pad[:, rows]).double().view(pad.shape[0], 1, r, 1)
    qm = (q[:, :, rows] * live).sum(2) / r
    km = (k[:, :, rows] * live).sum(2) / r
    P = [p.double().cpu() for p in params]

    def mu_net(x, W, b, g=None, bb=None):
        y = x @ W.t() + b
        if g is not None:
            y = torch.nn.functional.layer_norm(y, (d,), g, bb, 1e-5)
        return y
    if adaptive:
        rq, rk = mu_net(qm, *P[0:4]), mu_net(km, *P[4:8])
    else:
        rq, rk = mu_net(qm, *P[0:2]), mu_net(km, *P[2:4])
    mu = rq + rk
    kk = k[:, :, rows]
    lg = s * torch.einsum("bhd,bhjd->bhj", mu, kk) - 0.5 * s * (kk * kk).sum(-1)
    lg = lg.masked_fill(pad[:, rows].view(pad.shape[0], 1, r), -5e4)
    beta = torch.einsum("bhj,bhjd->bhd", torch.softmax(lg, -1), v[:, :, rows] * live)
    return rk, beta


def _bound(dtype, ref):
    if dtype == torch.float32:
        return 1e-5 * ref.abs().max()
    return (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11) * ref.abs() + 1e-6 * ref.abs().max()


def _setup(dtype, B, h, cap, d, L, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, cap, 3, h, d, generator=g).to(dtype).cuda()
    lk = torch.randn(B, h, L, d, generator=g).cuda()
    lv = torch.randn(B, h, L, d, generator=g).cuda()
    return qkv, lk, lv


def _views(qkv):
    return [qkv[:, :, i].transpose(1, 2) for i in range(3)]


def _io(dtype):
    from efficient_attention import _native as nv
    return {torch.bfloat16: nv.EA_BF16, torch.float16: nv.EA_F16, torch.float32: nv.EA_F32}[dtype]


DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (name, d, w, e, r, t0, T, B) -- L = t / r landmark columns at the last token
ATTN_CASES = [
    ("L0", 64, 32, 0, 4, 1, 2, 2),                 # tokens 1, 2: no landmark yet
    ("L1", 64, 32, 0, 4, 5, 1, 2),                 # one landmark
    ("L600", 128, 128, 0, 4, 2400, 1, 2),          # 600 landmarks at the LM head size
    ("boundary", 64, 32, 0, 4, 29, 6, 2),          # tokens 29..34 on both sides of the window boundary at 32
    ("ext_block0", 32, 16, 16, 8, 3, 4, 2),        # left extension in block 0 (absent slots)
    ("ext_boundary", 64, 32, 32, 8, 60, 9, 2),     # extension, across a boundary
    ("prefill", 128, 64, 0, 8, 0, 150, 1),         # many queries per block, three blocks
    ("two_groups", 64, 32, 0, 4, 32, 12, 2),       # two query groups of two waves each: the in-LDS merge at waves 0 and 2
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_decode_attn_kernel_against_fp64(dtype, case, with_bias):
    from efficient_attention import _native as nv
    name, d, w, e, r, t0, T, B = case
    h = 2
    cap = ((t0 + T + w - 1) // w) * w
    L = max((t0 + T) // r, 1)
    qkv, lk, lv = _setup(dtype, B, h, cap, d, L, seed=len(name) * 7 + d)
    g = torch.Generator().manual_seed(99)
    pad = torch.rand(B, cap, generator=g) < 0.2
    # a token whose whole local window is padded except itself (element 0, the step's last token)
    tl = t0 + T - 1
    bk = tl // w
    pad[0, max(bk * w - e, 0):bk * w + w] = True
    pad[0, tl] = False
    pad = pad.cuda()
    bias = (torch.randn(w, w + e, generator=g) if with_bias else None)
    q, k, v = _views(qkv)
    out = torch.empty(B, h, T, d, dtype=dtype, device="cuda")
    geom = nv.ea_ceva_dec_geom(B, h, d, _io(dtype), w, e, r, t0, T, 0, -1, cap, 1, int(with_bias), 1)
    bias_d = bias.float().cuda() if with_bias else None
    tq, tk, tv, tl_, tb, to = [nv.t4(t) for t in (q, k, v, lk, lv, out)]
    nv.call("ea_ceva_decode_attn", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(pad.to(torch.uint8)),
            nv.ptr(bias_d), ctypes.byref(tl_), ctypes.byref(tb), ctypes.byref(to), nv.stream())
    torch.cuda.synchronize()
    ref = _ref_attn(*[t.double().cpu() for t in (q, k, v)], pad.cpu(), None if bias is None else bias.double(),
                    lk.double().cpu(), lv.double().cpu(), t0, T, w, e, r)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    live = ~pad.cpu()[:, t0:t0 + T].view(B, 1, T, 1)             # padded query rows: finite only
    excess = ((got - ref).abs() - _bound(dtype, ref)) * live
    assert excess.max().item() <= 0, (name, dtype, excess.max().item(), ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("adaptive", [1, 0], ids=["qk", "no-ln"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_decode_close_kernel_against_fp64(dtype, adaptive, d):
    """Chunks 1 .. 6 of chunk length 8 closed in one launch; chunk 2 is fully padded (means of no row; beta = 0), chunk 4 in
    part.  Bounds: 1e-5 of the maximum (the outputs are fp32 in every case)."""
    from efficient_attention import _native as nv
    B, h, r, w = 2, 3, 8, 32
    cap, t0, T = 64, 9, 47                                    # tokens 9 .. 55 complete chunks 1 .. 6
    qkv, lk, lv = _setup(dtype, B, h, cap, d, cap // r, seed=d + adaptive)
    lk0, lv0 = lk.clone(), lv.clone()
    pad = torch.zeros(B, cap, dtype=torch.bool)
    pad[:, 16:24] = True
    pad[1, 32:37] = True
    pad = pad.cuda()
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
    geom = nv.ea_ceva_dec_geom(B, h, d, _io(dtype), w, 0, r, t0, T, c0, c1, cap, adaptive, 0, 1)
    mp = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
    tq, tk, tv, tl_, tb = [nv.t4(t) for t in (q, k, v, lk, lv)]
    nv.call("ea_ceva_decode_close", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv),
            nv.ptr(pad.to(torch.uint8)), mp, ctypes.byref(tl_), ctypes.byref(tb), nv.stream())
    torch.cuda.synchronize()
    qd, kd, vd = [t.double().cpu() for t in (q, k, v)]
    for c in range(cap // r):
        if c0 <= c <= c1:
            rk, beta = _ref_close(qd, kd, vd, pad.cpu(), params, c, r, adaptive)
            for got, ref in ((lk[:, :, c], rk), (lv[:, :, c], beta)):
                err = (got.double().cpu() - ref).abs().max().item()
                assert err <= 1e-5 * max(ref.abs().max().item(), 1e-30), (c, err, ref.abs().max().item())
            if c == 2:
                assert lv[:, :, c].abs().max().item() == 0              # no row: a zero control variate
        else:                                                          # chunks outside the range are left alone
            assert torch.equal(lk[:, :, c], lk0[:, :, c]) and torch.equal(lv[:, :, c], lv0[:, :, c])


# ---- guards: what still rounds ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fp32_decoding_without_fp32_cores_rounds_with_the_warning(monkeypatch):
    from efficient_attention import _f32, _ops
    monkeypatch.setattr(_f32, "ENABLED", False)
    aa = dict(RECIPE, window_size=32)
    m = _build(256, 4, aa)
    torch.manual_seed(7)
    x = torch.randn(50, 2, 256, device="cuda")
    _ops._FP32_WARNED[0] = False
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with _Calls() as calls:
            inc, state = _decode(m, x, (1, 9, 1), calls)
        full, _ = m(x, x, x)
    assert [w for w in rec if "rounded to bf16" in str(w.message)]
    buf = m._get_input_buffer(state)
    assert buf["qkv"].dtype == torch.bfloat16
    assert inc.dtype == torch.float32 and torch.isfinite(inc).all()
    assert (inc - full).abs().max().item() <= 2e-2 * full.abs().max().item()


@pytest.mark.gpu
def test_bf16_state_continued_by_an_fp32_step_rounds_with_the_warning():
    from efficient_attention import _ops
    aa = dict(RECIPE, window_size=32)
    m = _build(256, 4, aa)
    torch.manual_seed(9)
    x = torch.randn(30, 2, 256, device="cuda")
    st = {}
    m.init_incremental_state()
    _ops._FP32_WARNED[0] = False
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ys = [m(x[:20], x[:20], x[:20], incremental_state=st)[0].float()]
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for t in range(20, 30):
                ys.append(m(x[t:t + 1], x[t:t + 1], x[t:t + 1], incremental_state=st)[0])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            full, _ = m(x, x, x)
    assert [w for w in rec if "rounded to bf16" in str(w.message)]
    assert m._get_input_buffer(st)["qkv"].dtype == torch.bfloat16
    inc = torch.cat(ys, 0)
    assert torch.isfinite(inc).all()
    assert (inc - full.float()).abs().max().item() <= 2e-2 * full.float().abs().max().item()
