"""-m gpu: `matrix_prompts=True` of static / rolling incremental decoding (csrc/ea_ceva_decode_mm.hip, ceva_attn_mm_kernel).

The kernel against the fp64 restatement of test_gpu_ceva_decode.py on the operands it multiplies, inside the bound DESIGN.md 4a
derives (a CPU model of its two roundings must stay inside it first); the module next to plain states; launches; refusals."""
import ctypes
import functools
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

from ceva_decoding import STATIC, _Calls, _check_full, _ctx                               # noqa: E402
from test_gpu_causal_eva import RECIPE, _build                                           # noqa: E402
from test_gpu_ceva_decode import _io, _ref_attn, _views                                  # noqa: E402
from test_gpu_ceva_split_decode import _bits, _pad_flags, _to_ring                       # noqa: E402

pytestmark = pytest.mark.gpu
DT16, IDS16 = [torch.bfloat16, torch.float16], ["bf16", "fp16"]
MM = STATIC[:2] + ("ea_ceva_sdecode_attn_mm",) + STATIC[3:]
# (d, w, e, r, t0, T, ring rows or 0): one group, the diagonal landmark tile only; w = 16, every wave in another block; t0 % 16 = 12,
# two workgroups; 320 landmarks, five unmasked tiles then the masked one; the LM-head prefill; local tiles that wrap the ring
CASES = [(64, 32, 0, 4, 0, 16, 0), (64, 16, 16, 8, 3, 40, 0), (64, 32, 32, 8, 60, 37, 0), (64, 32, 0, 4, 1280, 48, 0),
         (128, 64, 0, 8, 0, 150, 0), (128, 64, 64, 4, 250, 70, 256)]


def _bound(dtype, ref, wabs, ncols, vmax):
    """u (|ref| + sum_j p_j |value_j|) + 1e-6 max |ref|; fp16: + n_cols 2^-24 max |value|."""
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    return u * (ref.abs() + wabs) + 1e-6 * ref.abs().max() + (ncols * 2.0 ** -24 * vmax if dtype == torch.float16 else 0.0)


def _check_kernel(monkeypatch, dtype, case, with_bias, l16, ntok=None):
    from efficient_attention import _native as nv
    d, w, e, r, t0, T, R = case
    B = h = 2
    cap = ((t0 + T + w - 1) // w) * w
    g = torch.Generator().manual_seed(7 * t0 + d + T)
    lin = torch.randn(B, cap, 3, h, d, generator=g).to(dtype)
    lk, lv = [torch.randn(B, h, cap // r, d, generator=g) for _ in range(2)]
    pad, g = _pad_flags(B, cap, t0, T, w, e)
    bias = torch.randn(w, w + e, generator=g) if with_bias else None
    # the reference multiplies what the kernel multiplies: fp32 landmark rows rounded to the state's type
    ql, kl, vl = [t.double() for t in _views(lin)]
    lkd, lvd = lk.to(dtype).double(), lv.to(dtype).double()
    own = [T] * B if ntok is None else ntok
    ref = torch.zeros(B, h, T, d, dtype=torch.float64)
    wabs, model = ref.clone(), ref.clone()
    for b in range(B):                                           # (per element: a per-sequence row ends at its own count)
        one = [t[b:b + 1] for t in (ql, kl, vl, pad)] + [None if bias is None else bias.double(), lkd[b:b + 1]]
        ref[b, :, :own[b]] = _ref_attn(*one, lvd[b:b + 1], t0, own[b], w, e, r)[0]
        wabs[b, :, :own[b]] = _ref_attn(*one[:2], vl[b:b + 1].abs(), *one[3:], lvd[b:b + 1].abs(), t0, own[b], w, e, r)[0]
        with monkeypatch.context() as mp:                        # the rounding model: P and the output rounded to the type
            real = torch.softmax
            mp.setattr(torch, "softmax", lambda x, dim: real(x, dim).to(dtype).double())
            model[b, :, :own[b]] = _ref_attn(*one, lvd[b:b + 1], t0, own[b], w, e, r)[0].to(dtype).double()
    bound = _bound(dtype, ref, wabs, w + e + (t0 + T - 1) // r, max(vl.abs().max().item(), lvd.abs().max().item()))
    live = torch.stack([~pad[b, t0:t0 + T] & (torch.arange(T) < own[b]) for b in range(B)]).view(B, 1, T, 1)
    use = (((model - ref).abs() / bound) * live).max().item()
    print(case, dtype, "rounding model uses %.3f of the bound" % use)
    assert use <= 1.0
    qkv, pad_d = [(_to_ring(t, R, t0 + T) if R else t).cuda() for t in (lin, pad.to(torch.uint8))]
    lk_d, lv_d = [(t.to(dtype) if l16 else t).cuda() for t in (lk, lv)]
    bias_d = None if bias is None else bias.float().cuda()
    out = torch.full((B, h, T + 2, d), 7.0, dtype=dtype, device="cuda")          # two guard rows behind the step's
    pos, status = [torch.tensor(v * (1 if ntok is None else B), dtype=torch.int32, device="cuda") for v in ([t0], [0])]
    ntok_d = None if ntok is None else torch.tensor(ntok, dtype=torch.int32, device="cuda")
    geom = nv.ea_ceva_sdec_geom(B, h, d, _io(dtype), w, e, r, T, cap, 1, int(with_bias), R, pos.data_ptr(), status.data_ptr(),
                                None if ntok is None else ntok_d.data_ptr())
    tq, tk, tv, tl, tb, to = [nv.t4(t) for t in (*_views(qkv), lk_d, lv_d, out[:, :, :T])]
    nv.call("ea_ceva_sdecode_attn_mm" + ("_l16" if l16 else ""), ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk),
            ctypes.byref(tv), nv.ptr(pad_d), nv.ptr(bias_d), ctypes.byref(tl), ctypes.byref(tb), ctypes.byref(to), nv.stream())
    torch.cuda.synchronize()
    got = out.double().cpu()
    assert (got[:, :, T:] == 7.0).all() and torch.isfinite(got).all()           # rows the step does not own keep the guard
    assert all((got[b, :, own[b]:T] == 0).all() for b in range(B))              # a per-sequence row past its count: zeros
    err = (got[:, :, :T] - ref).abs()
    print(case, dtype, "max |d| / bound %.3f" % ((err / bound) * live).max().item())
    assert ((err - bound) * live).max().item() <= 0


@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("case", CASES, ids=["d%d_w%d_e%d_r%d_t%d_T%d_R%d" % c for c in CASES])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("l16", [False, True], ids=["Lf32", "L16"])
def test_attn_mm_kernel_against_fp64(monkeypatch, dtype, case, with_bias, l16):
    _check_kernel(monkeypatch, dtype, case, with_bias, l16)


@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
def test_attn_mm_kernel_with_per_sequence_counts(monkeypatch, dtype):
    _check_kernel(monkeypatch, dtype, CASES[2], True, False, ntok=[37, 5])


def _run(m, seqs, kind, dtype, calls=None, S=80, **opt):
    """Rows with their own sequences seqs[b] [T_b, C]: a prompt of up to 70 tokens, then single tokens -> (outputs, state)."""
    B, C, st = len(seqs), seqs[0].shape[1], {}
    init = m.init_static_decoding if kind == "static" else functools.partial(m.init_rolling_decoding, max_step_tokens=S)
    init(st, B, 100, dtype, "cuda", **opt)
    cur, outs = [0] * B, [[] for _ in range(B)]
    while any(cur[b] < len(seqs[b]) for b in range(B)):
        take = [min(70 if cur[b] == 0 else 1, len(seqs[b]) - cur[b]) for b in range(B)]
        x = torch.zeros(max(take), B, C, device="cuda")
        mask = torch.ones(B, max(take), dtype=torch.bool, device="cuda")
        for b in range(B):
            x[:take[b], b], mask[b, :take[b]] = seqs[b][cur[b]:cur[b] + take[b]], False
        if calls is not None:
            calls.step()
        y = m(x, x, x, key_padding_mask=mask if opt.get("per_sequence") else None, incremental_state=st)[0]
        for b in range(B):
            outs[b].append(y[:take[b], b])
            cur[b] += take[b]
    return outs, st


@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("combo", ["static", "rolling", "compact_landmarks", "per_sequence", "hold_projections", "pieces"])
def test_matrix_prompt_decoding_equals_full_forward_and_keeps_the_plain_state(dtype, combo):
    """Every row inside the project's bound of the full forward; the state and the single-token steps bit for bit the plain one's."""
    m = _build(256, 4, dict(RECIPE, window_size=32, chunk_size=4))
    opt = {combo: True} if combo in ("compact_landmarks", "per_sequence", "hold_projections") else {}
    kind, S = ("static", 80) if combo in ("static", "hold_projections") else ("rolling", 32 if combo == "pieces" else 80)
    torch.manual_seed(131)
    seqs = [torch.randn(n, 256, device="cuda") for n in ((78, 55) if combo == "per_sequence" else (78, 78))]
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings(), _Calls() as calls:
        warnings.simplefilter("ignore")
        fulls = [m(s.unsqueeze(1), s.unsqueeze(1), s.unsqueeze(1))[0][:, 0] for s in seqs]
        plain, pst = _run(m, seqs, kind, dtype, S=S, **opt)
        got, gst = _run(m, seqs, kind, dtype, calls=calls, S=S, **opt, matrix_prompts=True)
    attn = [c for c in calls.steps[0] if "_attn" in c]
    l16 = "_l16" if combo == "compact_landmarks" else ""
    mm, valu = "ea_ceva_sdecode_attn_mm" + l16, "ea_ceva_sdecode_attn" + l16
    assert attn == ([mm, mm, valu] if combo == "pieces" else [mm])               # pieces of 32, 32 and 6: the last on attn
    assert not [c for s in calls.steps[1:] for c in s if "attn_mm" in c]
    for b, full in enumerate(fulls):
        _check_full(torch.cat(got[b], 0), full, dtype)
        assert all(_bits(a, c) for a, c in zip(plain[b][1:], got[b][1:]))        # the single-token steps
    pb, gb = m._get_input_buffer(pst), m._get_input_buffer(gst)
    for k in ("qkv", "pad", "pos", "rf_k_bar", "beta"):
        assert _bits(pb[k], gb[k]), k
    assert m.get_incremental_state(gst, "attn_static")["matrix_prompts"] is True
    assert "matrix_prompts" not in m.get_incremental_state(pst, "attn_static")


def test_matrix_prompt_step_launches():
    m = _build(256, 4, dict(RECIPE, window_size=32, chunk_size=4))
    torch.manual_seed(137)
    x = torch.randn(100, 2, 256, device="cuda")
    core = lambda s: [c for c in s if not (c.startswith("ea_linear") or c == "ea_multi_cast")]      # noqa: E731
    for on in (True, False):
        st = {}
        m.init_static_decoding(st, 2, 100, torch.bfloat16, "cuda", matrix_prompts=on)
        with torch.no_grad(), _ctx(torch.bfloat16), warnings.catch_warnings(), _Calls() as calls:
            warnings.simplefilter("ignore")
            for a, n in ((0, 70), (70, 8), (78, 1), (79, 16)):
                calls.step()
                m(x[a:a + n], x[a:a + n], x[a:a + n], incremental_state=st)
        want = [MM, STATIC, STATIC, MM] if on else [STATIC] * 4
        assert [core(s) for s in calls.steps] == [list(s) for s in want]


@pytest.mark.parametrize("what", ["fp32", "head_dim_32", "window_24"])
def test_matrix_prompts_refuses_what_the_kernel_has_no_instance_for(what, monkeypatch):
    from efficient_attention import _f32, _native as nv
    monkeypatch.setattr(_f32, "ENABLED", True)
    dtype = torch.float32 if what == "fp32" else torch.bfloat16
    heads, w = (8 if what == "head_dim_32" else 4), (24 if what == "window_24" else 32)
    m = _build(256, heads, dict(RECIPE, window_size=w, chunk_size=4))
    for init in (m.init_static_decoding, m.init_rolling_decoding):
        st = {}
        with pytest.raises(ValueError, match="matrix_prompts"):
            init(st, 2, 96, dtype, "cuda", matrix_prompts=True)
        assert st == {}
    io = nv.EA_F32 if what == "fp32" else nv.EA_BF16
    pos = torch.zeros(2, dtype=torch.int32, device="cuda")
    geom = nv.ea_ceva_sdec_geom(2, heads, 256 // heads, io, w, 0, 4, 16, 96, 1, 0, 0, pos.data_ptr(), pos[1:].data_ptr(), None)
    for entry in ("ea_ceva_sdecode_attn_mm", "ea_ceva_sdecode_attn_mm_l16"):      # decided before any operand is looked at
        assert getattr(nv.lib(), entry)(ctypes.byref(geom), None, None, None, None, None, None, None, None, None) == -2
