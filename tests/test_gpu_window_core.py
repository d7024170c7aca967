"""-m gpu: the 16-bit window-attention kernels (ea_window_attn_fwd / _bwd) and the EVA landmark passes (ea_eva_chunk_mean_*,
ea_eva_beta_*) against an fp64 evaluation of the SAME operands (tests/window_reference.py), one case per host-selected plan
(tests/window_cases.py; the plans are pinned on the CPU by tests/test_window_reference_cpu.py).

Bound, per compared tensor X with the exact reference R and the rounding model M (the reference in fp32 with the kernels'
documented 16-bit roundings): a(X) = max_i |X_i - R_i| / (rms(R) + |R_i|) must satisfy a(HIP) <= 4 a(M) + f, and so must the two
norm-wise figures (max / max, rms / rms); f = 2^-9 (bf16) | 2^-12 (fp16) for tensors stored in 16 bits, 2^-20 for fp32 results.
The factor is fixed in advance (window_reference.FACTOR), M and R are computed at test time: no recorded constants.
`pytest -s` prints a(HIP) / a(M) per tensor; DESIGN.md 4b carries the worst ratios observed."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import window_cases as wc               # noqa: E402
import window_reference as wr           # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
F64 = torch.float64


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _window_operands(name, io, same_rows=False):
    """CPU operands of a window case (seeded per case), 16-bit values held in fp32: q, k = 1.5 randn, v, dout = randn rounded to
    the I/O dtype; lk, lv = randn rounded to it (the kernels convert landmark rows to the MFMA element type: identical operands
    on both sides); bias = 0.5 randn fp32.  same_rows: every batch row gets the data of row 0."""
    c = wc.WINDOW_CASES[name]
    B, h, N, d, L = (1 if same_rows else c["B"]), c["h"], c["N"], c["d"], c["L"]
    g = torch.Generator().manual_seed(_seed(name))

    def r16(t):
        return t.to(io).float()
    mult = float(c["mult"])
    o = dict(q=r16(1.5 * mult * torch.randn(B, h, N, d, generator=g)), k=r16(1.5 * mult * torch.randn(B, h, N, d, generator=g)),
             v=r16(mult * torch.randn(B, h, N, d, generator=g)),
             dout=r16((2.0 * mult if mult > 1 else 1.0) * torch.randn(B, h, N, d, generator=g)))
    o["lk"] = r16(torch.randn(B, h, L, d, generator=g)) if L else None
    o["lv"] = r16(torch.randn(B, h, L, d, generator=g)) if L else None
    w, e = c["w"], c["e"]
    Wq, Wk = (w * w, (w + 2 * e) ** 2) if c["attn_2d"] else (w, w + (e if c["causal"] else 2 * e))
    o["bias"] = 0.5 * torch.randn(h, Wq, Wk, generator=g) if c["bias"] else None
    o["mask"] = None
    if c["tail"] and not same_rows:
        o["mask"] = torch.zeros(B, N, dtype=torch.bool)
        o["mask"][1, N - (3 * Wq) // 2:] = True
    o["keep"] = (torch.rand(B, h, N, Wk + L, generator=g) < 0.8).float() if c["keep"] else None
    o["dlse"] = torch.randn(B, h, N, generator=g) if c["dlse"] else None
    if same_rows:
        o = {k_: (t if t is None or k_ == "bias" else t.expand(c["B"], *t.shape[1:]).contiguous()) for k_, t in o.items()}
    o["Wk"] = Wk
    return c, o


def _run_window_kernels(c, o, io):
    """The operands through _ops._window_fwd / _window_bwd -> dict of CPU tensors [B,h,N,d] / [B,h,L,d] / [h,Wq,Wk] / [B,h,N]."""
    from efficient_attention import _native as nv
    from efficient_attention import _ops
    dev = "cuda"
    B, h, N, d, L = c["B"], c["h"], c["N"], c["d"], c["L"]
    geom = nv.make_geom(B, h, N, d, nv._DTYPES[io], c["attn_2d"], c["seq_shape"], c["w"], c["e"], c["chunk"], L, c["causal"])
    qkv = torch.stack([o["q"], o["k"], o["v"]], 0).permute(1, 3, 0, 2, 4).to(io)              # [B,N,3,h,d]
    if c["time_first"]:
        qkv5 = qkv.transpose(0, 1).contiguous().to(dev).transpose(0, 1)                        # a view of [N,B,3,h,d]
    else:
        qkv5 = qkv.contiguous().to(dev)
    lk = None if L == 0 else o["lk"].contiguous().to(dev)
    lv = None if L == 0 else o["lv"].contiguous().to(dev)
    bias_p = None if o["bias"] is None else _ops._bias_padded(o["bias"].to(dev), geom)
    mask_u8 = None if o["mask"] is None else o["mask"].to(dev).to(torch.uint8).contiguous()
    keep, keep_scale = None, 1.0
    if o["keep"] is not None:
        keep_ld, ld = int(nv.query("ea_window_keep_ld", geom)), int(nv.query("ea_window_bias_ld", geom))
        Wk = o["Wk"]
        assert keep_ld >= ld + L and ld >= Wk
        kp = torch.zeros(B, h, N, keep_ld, dtype=torch.uint8)
        kp[..., :Wk] = o["keep"][..., :Wk].to(torch.uint8)
        kp[..., ld:ld + L] = o["keep"][..., Wk:].to(torch.uint8)
        keep, keep_scale = kp.to(dev), 1.25
    out, lse = _ops._window_fwd(geom, qkv5, lk, lv, bias_p, mask_u8, keep, keep_scale)
    assert tuple(out.shape) == (B, N, h, d) and tuple(lse.shape) == (B, h, N)
    dqkv5 = torch.empty_like(qkv5).fill_(float("nan"))               # every token must be written by some launch
    assert dqkv5.stride() == qkv5.stride()
    dout = o["dout"].permute(0, 2, 1, 3).to(io).contiguous().to(dev)  # [B,N,h,d]
    dlse = None if o["dlse"] is None else o["dlse"].contiguous().to(dev)
    dlk, dlv, dbias = _ops._window_bwd(geom, qkv5, lk, lv, bias_p, mask_u8, out, dout, lse, dqkv5, keep, keep_scale, dlse)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv5.float()).all()), "dq / dk / dv hold elements no launch wrote"
    res = dict(out=out.permute(0, 2, 1, 3), lse=lse, dq=dqkv5[:, :, 0].permute(0, 2, 1, 3), dk=dqkv5[:, :, 1].permute(0, 2, 1, 3),
               dv=dqkv5[:, :, 2].permute(0, 2, 1, 3))
    if L:
        res.update(dlk=dlk, dlv=dlv)
    if dbias is not None:
        res["dbias"] = dbias[..., :o["Wk"]]
    return {k_: t.detach().float().cpu() for k_, t in res.items()}


def _reference(c, o, dtype, round_to):
    kw = dict(bias=o["bias"], mask=o["mask"], attn_2d=c["attn_2d"], seq_shape=c["seq_shape"], w=c["w"], e=c["e"], causal=c["causal"],
              chunk=c["chunk"], dtype=dtype, round_to=round_to, store=c["store"] if round_to is not None else "single")
    if o["keep"] is not None:
        kw.update(keep=o["keep"], keep_scale=1.25)
    B = c["B"]
    step = B if B <= 8 else 8                                        # (large batches in slices: bounds the gathered copies)
    parts = []
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        kw_b = dict(kw, mask=None if o["mask"] is None else o["mask"][sl], keep=None if o["keep"] is None else o["keep"][sl])
        if o["keep"] is None:
            kw_b.pop("keep")
        parts.append(wr.window_grads(o["q"][sl], o["k"][sl], o["v"][sl], None if o["lk"] is None else o["lk"][sl],
                                     None if o["lv"] is None else o["lv"][sl], o["dout"][sl],
                                     None if o["dlse"] is None else o["dlse"][sl], **kw_b))
    res = {k_: torch.cat([p_[k_] for p_ in parts], 0) for k_ in parts[0] if k_ != "dbias"}
    if "dbias" in parts[0]:
        res["dbias"] = sum(p_["dbias"] for p_ in parts)
    return res


def _check(tag, got, M, R, round_to, names):
    bad, lines = [], []
    for n_ in names:
        ok, txt, _ = wr.bound_report(n_, got[n_], M[n_], R[n_], round_to)
        lines.append("%s %s" % (tag, txt))
        if not ok:
            bad.append(n_)
    print("\n" + "\n".join(lines))
    assert not bad, "%s: %s exceed 4 a(M) + f\n%s" % (tag, bad, "\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(wc.WINDOW_CASES))
def test_window_kernels_match_fp64_same_operand_reference(name, dt):
    io = DTYPES[dt]
    c, o = _window_operands(name, io)
    got = _run_window_kernels(c, o, io)
    R = _reference(c, o, F64, None)
    M = _reference(c, o, torch.float32, io)
    names = ["out", "lse", "dq", "dk", "dv"] + (["dlk", "dlv"] if c["L"] else []) + (["dbias"] if c["bias"] else [])
    _check("%s/%s" % (name, dt), got, M, R, io, names)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", wc.BATCH_INDEPENDENCE)
def test_window_kernels_batch_rows_are_independent(name, dt):
    """Every batch row holds the same data: the rows of every per-row result must be bit-identical."""
    io = DTYPES[dt]
    c, o = _window_operands(name, io, same_rows=True)
    got = _run_window_kernels(c, o, io)
    for n_ in ("out", "lse", "dq", "dk", "dv", "dlk", "dlv"):
        if n_ in got:
            t = got[n_]
            assert bool((t == t[:1]).all()), (name, n_)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wc.REFUSED))
def test_oversized_key_list_is_refused_not_miscomputed(name):
    """256 keys of a query block / window at D = 128 do not fit the backward's LDS image: the planner's queries still answer for these
    geometries, the backward entry must say `unsupported geometry` (and launch nothing) rather than run a tiling that does not fit."""
    from efficient_attention import _native as nv
    from efficient_attention import _ops
    c = wc.REFUSED[name]
    B, h, N, d, L = c["B"], c["h"], c["N"], c["d"], c["L"]
    geom = nv.make_geom(B, h, N, d, nv.EA_BF16, c["attn_2d"], c["seq_shape"], c["w"], c["e"], c["chunk"], L, c["causal"])
    g = torch.Generator().manual_seed(_seed(name))
    qkv5 = torch.randn(B, N, 3, h, d, generator=g).to(torch.bfloat16).cuda()
    lk, lv = torch.randn(B, h, L, d, generator=g).cuda(), torch.randn(B, h, L, d, generator=g).cuda()
    out, lse = _ops._window_fwd(geom, qkv5, lk, lv, None, None)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        _ops._window_bwd(geom, qkv5, lk, lv, None, None, out, torch.ones_like(out), lse, torch.empty_like(qkv5))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# landmark passes
# ------------------------------------------------------------------------------------------------------------------------
def _landmark_mask(c, masked):
    if not masked:
        return None
    B, N, r = c["B"], c["N"], c["r"]
    m = torch.zeros(B, N, dtype=torch.bool)
    if c["attn_2d"]:
        H, W = c["seq_shape"]
        m.view(B, H, W)[1, H - (3 * r) // 2:] = True            # the last row of chunks fully padded, the one before it half
    else:
        m[1, N - (3 * r) // 2:] = True
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "tailmask"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(wc.LANDMARK_CASES))
def test_landmark_kernels_match_fp64_same_operand_reference(name, dt, masked):
    from efficient_attention import _native as nv
    io = DTYPES[dt]
    c = wc.LANDMARK_CASES[name]
    B, h, N, d, L = c["B"], c["h"], c["N"], c["d"], c["L"]
    g = torch.Generator().manual_seed(_seed(name))

    def r16(t):
        return t.to(io).float()
    q, k = r16(1.5 * torch.randn(B, h, N, d, generator=g)), r16(1.5 * torch.randn(B, h, N, d, generator=g))
    v, omega = r16(torch.randn(B, h, N, d, generator=g)), r16(torch.randn(B, h, L, d, generator=g))
    pre = [r16(torch.randn(B, h, N, d, generator=g)) for _ in range(4)]                   # rows the backward passes add to
    dqm, dkm, dbeta = [torch.randn(B, h, L, d, generator=g) for _ in range(3)]
    mask = _landmark_mask(c, masked)
    geo = dict(r=c["r"], e=c["e"], attn_2d=c["attn_2d"], seq_shape=c["seq_shape"])

    dev = "cuda"
    geom = nv.make_geom(B, h, N, d, nv._DTYPES[io], c["attn_2d"], c["seq_shape"], c["w"], c["e"], c["r"], L, 0)

    def rows(t):                                                                           # [B,h,N,d] fp32 -> strided [B,h,N,d] view
        return t.permute(0, 2, 1, 3).to(io).contiguous().to(dev).permute(0, 2, 1, 3)
    tq, tk, tv = rows(q), rows(k), rows(v)
    m8 = None if mask is None else mask.to(dev).to(torch.uint8).contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    qmean, kmean, beta, d_omega = [torch.full((B, h, L, d), float("nan"), **f32) for _ in range(4)]
    t4 = {n_: nv.t4(t) for n_, t in (("q", tq), ("k", tk), ("v", tv))}
    st = nv.stream()
    nv.call("ea_eva_chunk_mean_fwd", ctypes.byref(geom), ctypes.byref(t4["q"]), ctypes.byref(t4["k"]), nv.ptr(m8), nv.ptr(qmean),
            nv.ptr(kmean), st)
    om_d = omega.contiguous().to(dev)
    nv.call("ea_eva_beta_fwd", ctypes.byref(geom), ctypes.byref(t4["k"]), ctypes.byref(t4["v"]), nv.ptr(m8), nv.ptr(om_d), nv.ptr(beta), st)
    # chunk-mean backward adds to dq, dk; beta backward to dk, dv (separate buffers per pass: each is compared on its own)
    cm_dq, cm_dk, b_dk, b_dv = [rows(t) for t in pre]
    dqm_d, dkm_d, dbeta_d = dqm.contiguous().to(dev), dkm.contiguous().to(dev), dbeta.contiguous().to(dev)
    td = {n_: nv.t4(t) for n_, t in (("cm_dq", cm_dq), ("cm_dk", cm_dk), ("b_dk", b_dk), ("b_dv", b_dv))}
    nv.call("ea_eva_chunk_mean_bwd", ctypes.byref(geom), nv.ptr(dqm_d), nv.ptr(dkm_d), nv.ptr(m8), ctypes.byref(td["cm_dq"]),
            ctypes.byref(td["cm_dk"]), st)
    nv.call("ea_eva_beta_bwd", ctypes.byref(geom), ctypes.byref(t4["k"]), ctypes.byref(t4["v"]), nv.ptr(m8), nv.ptr(om_d), nv.ptr(beta),
            nv.ptr(dbeta_d), ctypes.byref(td["b_dk"]), ctypes.byref(td["b_dv"]), nv.ptr(d_omega), st)
    torch.cuda.synchronize()
    got_cm = dict(qmean=qmean, kmean=kmean, dq=cm_dq, dk=cm_dk)
    got_b = dict(beta=beta, d_omega=d_omega, dk=b_dk, dv=b_dv)
    got_cm, got_b = [{n_: t.detach().float().cpu() for n_, t in gd.items()} for gd in (got_cm, got_b)]
    for gd in (got_cm, got_b):
        assert all(bool(torch.isfinite(t).all()) for t in gd.values())

    tag = "%s/%s/%s" % (name, dt, "tailmask" if masked else "nomask")
    R = wr.chunk_mean_grads(q, k, mask, dqm, dkm, pre[0], pre[1], dtype=F64, **geo)
    M = wr.chunk_mean_grads(q, k, mask, dqm, dkm, pre[0], pre[1], dtype=torch.float32, round_to=io, **geo)
    _check(tag + " chunk_mean", got_cm, M, R, io, ["qmean", "kmean", "dq", "dk"])
    R = wr.beta_grads(k, v, omega, mask, dbeta, pre[2], pre[3], dtype=F64, **geo)
    M = wr.beta_grads(k, v, omega, mask, dbeta, pre[2], pre[3], dtype=torch.float32, round_to=io, **geo)
    _check(tag + " beta", got_b, M, R, io, ["beta", "d_omega", "dk", "dv"])
