"""-m gpu: the causal streaming softmax kernels (csrc/ea_softmax_causal.hip: smc_fwd_kernel, smc_bwd_dq_kernel,
smc_bwd_dkv_kernel) through the C ABI on the test's own tensors, results prefilled with NaN, against an fp64 evaluation of the
SAME 16-bit operands in plain torch (logits with -inf above the diagonal and on padded keys, softmax, logsumexp, autograd).

Bound: the softmax core's, unchanged (tests/softmax_reference.py / window_reference.py): a(HIP) <= 4 a(M) + f for out, lse, delta,
dq, dk, dv, M = window_reference._ModelAttn on the same causal logits; bound_report and floor_for as they are.  Every geometry is
crossed with every `tiles` value each direction allows for it, so every instantiation runs at a small N."""
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

import softmax_reference as sr          # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
B, H = 2, 2
GEOMS = [(63, 64), (64, 64), (65, 64), (130, 32), (200, 128), (257, 64)]
KEEP_P = 0.25
NAN = float("nan")


def _tiles(d, keep):
    """(forward, backward) tile counts crossed: the longer list paced, the shorter one cycled."""
    fwd = [1, 2] + ([4] if d <= 64 and not keep else [])
    bwd = [1] + ([2] if d <= 64 else [])
    return [(f, bwd[i % len(bwd)]) for i, f in enumerate(fwd)]


CASES = [(N, d, tf, tb, "plain") for N, d in GEOMS for tf, tb in _tiles(d, False)]
CASES += [(200, 128, tf, tb, "mask") for tf, tb in _tiles(128, False)] + [(130, 32, tf, tb, "mask") for tf, tb in _tiles(32, False)]
CASES += [(257, 64, tf, tb, "keep") for tf, tb in _tiles(64, True)] + [(200, 128, tf, tb, "keep") for tf, tb in _tiles(128, True)]

_OPERANDS = {}


def _operands(N, d, io, variant):
    """q, k, v, dout [B,h,N,d] rounded once to the I/O dtype (held in fp32), the padding mask and the keep decisions."""
    key = (N, d, io, variant)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(1000 * N + d)
        o = {n: torch.randn(B, H, N, d, generator=g).to(io).float() for n in ("q", "k", "v", "dout")}
        o["mask"] = o["keep"] = None
        if variant == "mask":                            # a padded tail on row 0, one interior key (>= 1) on row 1
            m = torch.zeros(B, N, dtype=torch.bool)
            m[0, N - 37:] = True
            m[1, 70] = True
            o["mask"] = m
        if variant == "keep":
            o["keep"] = (torch.rand(B, H, N, N, generator=g) >= KEEP_P).to(torch.uint8)
        _OPERANDS[key] = o
    return _OPERANDS[key]


def _reference(o, dtype, round_to):
    """fp64 exact (round_to None) or the rounding model M in fp32 -> dict(out, lse, delta, dq, dk, dv)."""
    leaves = [o[n].detach().to(dtype).requires_grad_(True) for n in ("q", "k", "v")]
    q, k, v = leaves
    N, d = q.shape[2], q.shape[3]
    logits = d ** -0.5 * torch.einsum("bhid,bhjd->bhij", q, k)
    dead = torch.ones(N, N, dtype=torch.bool).triu(1)[None, None]
    if o["mask"] is not None:
        dead = dead | o["mask"][:, None, None, :]
    logits = logits.masked_fill(dead, float("-inf"))
    keepmul = None if o["keep"] is None else o["keep"].to(dtype) / (1.0 - KEEP_P)
    if round_to is None:
        pr = torch.softmax(logits, -1)
        out, lse = torch.matmul(pr if keepmul is None else pr * keepmul, v), torch.logsumexp(logits, -1)
    else:
        out, lse = sr._ModelAttn.apply(logits, v, keepmul, round_to)
    dout = o["dout"].to(dtype)
    res = dict(out=out.detach(), lse=lse.detach(), delta=(dout * out.detach()).sum(-1))
    gs = torch.autograd.grad([out, lse], leaves, [dout, torch.zeros_like(lse)])
    res.update({n: sr.rnd(g_, round_to) for n, g_ in zip(("dq", "dk", "dv"), gs)})
    return res


_REFS = {}


def _refs(N, d, io, variant):
    key = (N, d, io, variant)
    if key not in _REFS:
        o = _operands(N, d, io, variant)
        _REFS[key] = (_reference(o, torch.float64, None), _reference(o, torch.float32, io))
    return _REFS[key]


def _run(o, io, tf, tb, forward_only=False, kv=None):
    """ea_softmax_causal_fwd / _bwd on a fused [B,N,3,h,d] tensor -> dict of CPU fp32 tensors [B,h,N,d] / [B,h,N]."""
    from efficient_attention import _native as nv
    N, d = o["q"].shape[2:]
    k_, v_ = (o["k"], o["v"]) if kv is None else kv
    qkv5 = torch.stack([o["q"], k_, v_], 0).permute(1, 3, 0, 2, 4).to(io).contiguous().cuda()      # [B,N,3,h,d]
    q, k, v = [qkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    dqkv5 = torch.full_like(qkv5, NAN)
    dq, dk, dv = [dqkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    out = torch.full((B, N, H, d), NAN, dtype=io, device="cuda")
    lse, delta = [torch.full((B * H, N), NAN, dtype=torch.float32, device="cuda") for _ in range(2)]
    mask = None if o["mask"] is None else o["mask"].to(torch.uint8).contiguous().cuda()
    keep, ks = None, 1.0
    if o["keep"] is not None:
        keep = torch.ones(B, H, N, (N + 63) // 64 * 64, dtype=torch.uint8)
        keep[..., :N] = o["keep"]
        keep, ks = keep.cuda(), 1.0 / (1.0 - KEEP_P)
    ot = out.permute(0, 2, 1, 3)
    ts = [nv.t4(t) for t in (q, k, v, ot)]
    nv.call("ea_softmax_causal_fwd", B, H, N, d, nv.io_dtype(q), float(d) ** -0.5, *[ctypes.byref(t) for t in ts[:3]],
            nv.ptr(mask), ctypes.byref(ts[3]), nv.ptr(lse), nv.ptr(keep), float(ks), tf, nv.stream())
    res = dict(out=ot, lse=lse.view(B, H, N))
    if not forward_only:
        dout = o["dout"].permute(0, 2, 1, 3).to(io).contiguous().cuda().permute(0, 2, 1, 3)
        ts += [nv.t4(t) for t in (dout, dq, dk, dv)]
        nv.call("ea_softmax_causal_bwd", B, H, N, d, nv.io_dtype(q), float(d) ** -0.5, *[ctypes.byref(t) for t in ts[:3]],
                nv.ptr(mask), ctypes.byref(ts[3]), ctypes.byref(ts[4]), nv.ptr(lse), nv.ptr(delta),
                *[ctypes.byref(t) for t in ts[5:]], nv.ptr(keep), float(ks), tb, nv.stream())
        res.update(delta=delta.view(B, H, N), dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return {n: t.detach().float().cpu() for n, t in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("N,d,tf,tb,variant", CASES, ids=["%dx%d-t%d%d-%s" % c for c in CASES])
def test_causal_kernels_match_fp64_same_operand_reference(N, d, tf, tb, variant, dt):
    io = DTYPES[dt]
    o = _operands(N, d, io, variant)
    got = _run(o, io, tf, tb)
    assert set(got) == set(sr.NAMES)
    for n_, t in got.items():
        assert bool(torch.isfinite(t).all()), "%s holds elements no launch wrote (or non-finite values)" % n_
    again = _run(o, io, tf, tb)
    assert bool((got["dk"] == again["dk"]).all()) and bool((got["dv"] == again["dv"]).all()), "dk / dv of two runs differ"
    if o["mask"] is not None:
        pad = o["mask"][:, None, :, None].expand_as(got["dk"])
        assert bool((got["dk"][pad] == 0).all()) and bool((got["dv"][pad] == 0).all()), "dk / dv of padded keys must be exactly 0"
    R, M = _refs(N, d, io, variant)
    bad, lines = [], []
    for n_ in sr.NAMES:
        ok, txt, _ = sr.bound_report(n_, got[n_], M[n_], R[n_], io)
        lines.append("%dx%d %s tiles %d/%d %s %s" % (N, d, dt, tf, tb, variant, txt))
        if not ok:
            bad.append(n_)
    print("\n" + "\n".join(lines))
    assert not bad, "%s exceed 4 a(M) + f\n%s" % (bad, "\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("tf", [1, 2, 4])
def test_a_query_does_not_see_later_keys(tf):
    """out and lse of query i are unchanged, bit for bit, when the keys and values after i are overwritten with other data."""
    io, N, d = torch.bfloat16, 130, 64
    o = _operands(N, d, io, "plain")
    base = _run(o, io, tf, 1, forward_only=True)
    g = torch.Generator().manual_seed(7)
    for i in (0, 15, 16, 63, 64, 79, 128):
        k2, v2 = o["k"].clone(), o["v"].clone()
        k2[:, :, i + 1:] = (8 * torch.randn(B, H, N - i - 1, d, generator=g)).to(io).float()
        v2[:, :, i + 1:] = (8 * torch.randn(B, H, N - i - 1, d, generator=g)).to(io).float()
        got = _run(o, io, tf, 1, forward_only=True, kv=(k2, v2))
        assert bool((got["out"][:, :, :i + 1] == base["out"][:, :, :i + 1]).all()), i
        assert bool((got["lse"][:, :, :i + 1] == base["lse"][:, :, :i + 1]).all()), i
