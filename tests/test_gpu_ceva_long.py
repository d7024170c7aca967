"""-m gpu: causal EVA past 64 chunks on the 16-bit kernels (csrc/ea_ceva_lm.hip, _ops.ceva_lm_fwd / ceva_lm_bwd).

Core: the landmark half of the softmax plus its join with a GIVEN window half (o_loc, lse_loc) against a plain torch evaluation
of the joint softmax on the same 16-bit-rounded operands, under the bound of the 16-bit window core (tests/window_reference.py:
a(got) <= 4 a(model) + f, the model being the same evaluation in fp32 with the kernels' documented 16-bit roundings -- P and dS
packed for their MFMA, out and d o_loc stored in the I/O dtype, delta read from the stored out).  Module: CausalEVAttention
in training at 80 chunks against the same module on the fp32 gathered-attention route it took before."""
import argparse
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

MASK_VAL = -5e4


def _join(ops, r, dtype, round_to):
    """out, zl and every gradient of sum(dout * out) for the joint softmax over [window half | L causal landmark columns]."""
    from window_reference import rnd
    q, lk, lv, o_loc, lse_loc, dout, kf = [None if t is None else t.to(dtype) for t in ops]
    N, d, L = q.shape[2], q.shape[3], lk.shape[2]
    scale = d ** -0.5
    vis = torch.arange(L)[None, :] < (torch.arange(N) // r)[:, None]         # landmark c < t / r
    s = torch.where(vis, scale * q @ lk.transpose(-1, -2), torch.full((), MASK_VAL, dtype=dtype))
    lse_lm = torch.logsumexp(s, -1)
    Z = torch.logaddexp(lse_loc, lse_lm)
    p = torch.exp(s - Z[..., None])
    pk = rnd(p if kf is None else p * kf, round_to)                          # dropped entries leave the numerator only
    w = torch.exp(lse_loc - Z)[..., None]
    out = rnd(w * o_loc + pk @ lv, round_to)
    delta = (dout * out).sum(-1, keepdim=True)
    dp = dout @ lv.transpose(-1, -2)
    ds = rnd(torch.where(vis, p * ((dp if kf is None else dp * kf) - delta), torch.zeros((), dtype=dtype)), round_to)
    return dict(out=out, Z=Z, dq_lm=scale * ds @ lk, dlk=scale * ds.transpose(-1, -2) @ q,
                dlv=pk.transpose(-1, -2) @ dout, do_loc=rnd(w * dout, round_to),
                dlse_loc=w[..., 0] * ((dout * o_loc).sum(-1) - delta[..., 0]))


CORE_CASES = [  # N, r, d, padding tail, keep mask: L = 68 (a tile + 4 rows), 136 (a third, partial tile), 128 (two tiles, r !| 64)
    (272, 4, 64, False, False), (272, 2, 128, True, False), (384, 3, 64, False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,r,d,tail,drop", CORE_CASES)
def test_landmark_half_and_join_match_fp64(N, r, d, tail, drop, dtype):
    from efficient_attention import _native as nv, _ops
    from window_reference import bound_report
    B, h, L = 1, 2, N // r
    gen = torch.Generator().manual_seed(N + r + d)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    q, o_loc, dout = [rn(B, h, N, d).to(dtype) for _ in range(3)]
    lk, lv = rn(B, h, L, d), rn(B, h, L, d)
    lse_loc = math.log(32.0) + rn(B, h, N)
    if tail:             # padded queries see no local key: their window half is Wk fills, the landmarks follow the causal rule
        lse_loc[..., N - 40:] = MASK_VAL + math.log(32.0)
    keep, p_drop = None, 0.25
    if drop:
        keep = torch.zeros(B, h, N, -(-L // 16) * 16, dtype=torch.uint8)
        keep[..., :L] = (torch.rand(B, h, N, L, generator=gen) >= p_drop).to(torch.uint8)
    ks = 1.0 / (1.0 - p_drop) if drop else 1.0
    kf = None if keep is None else keep[..., :L].double() * ks
    ops = (q.double(), lk.to(dtype).double(), lv.to(dtype).double(), o_loc.double(), lse_loc.double(), dout.double(), kf)
    ref, model = _join(ops, r, torch.float64, None), _join(ops, r, torch.float32, dtype)

    dev = lambda t: None if t is None else t.cuda()
    g = nv.make_geom(B, h, N, d, nv.io_dtype(q), False, (N,), 32, 0, r, L, 2)
    bnhd = lambda t: dev(t).transpose(1, 2).contiguous()                     # [B,N,h,d] buffers, as the window kernels leave them
    qd, old, doutd = bnhd(q).transpose(1, 2), bnhd(o_loc), bnhd(dout)
    lkd, lvd, lsed, keepd = dev(lk), dev(lv), dev(lse_loc), dev(keep)
    out, zl, img = _ops.ceva_lm_fwd(g, qd, lkd, lvd, old, lsed, keepd, ks)
    runs = [_ops.ceva_lm_bwd(g, qd, img, old, lsed, keepd, ks, out, doutd, zl) for _ in range(2)]
    do_loc, dlse, dq_lm, dlk, dlv = runs[0]
    got = dict(out=out.transpose(1, 2), Z=zl[..., 0], dq_lm=dq_lm.transpose(1, 2), dlk=dlk, dlv=dlv,
               do_loc=do_loc.transpose(1, 2), dlse_loc=dlse)
    bad = []
    for name, ref_t in ref.items():
        stored16 = "out" if name in ("out", "do_loc") else name              # (the floor of a tensor stored in 16 bits)
        ok, txt, _ = bound_report(stored16, got[name].cpu(), model[name], ref_t, dtype)
        print(name, txt)
        if not ok:
            bad.append(txt)
    assert not bad, "\n".join(bad)
    assert torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][4], runs[1][4])     # no atomics: bit for bit


@pytest.mark.gpu
def test_module_trains_past_64_chunks_on_the_16_bit_kernels():
    """The recipe's options at T = 160, chunk 2 (80 chunks): y, dx and every parameter gradient against the same module on the
    route it took before (fp32 up-cast, ea_f32_attn_*), and the new kernels ran in place of the fp32 ones."""
    import efficient_attention as ea
    from efficient_attention import _native as nv, _ops
    from gpu_checks import MODULE_TOL
    from util import scaled_err
    aa = dict(window_size=32, chunk_size=2, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None, overlap_window=False)
    torch.manual_seed(5)
    m = ea.AttentionFactory.build_attention(
        "causal_eva", dict(embed_dim=128, num_heads=2, self_attention=True, dropout=0.0, attn_args=argparse.Namespace(**aa))).cuda()
    m.train()
    x0 = torch.randn(160, 2, 128, device="cuda")
    noise = torch.randn(2, 2, 80, 64, device="cuda")
    dy = torch.randn(160, 2, 128, device="cuda")

    def run(on):
        calls, real, real_like, was = [], nv.call, torch.randn_like, _ops.USE_CEVA_LONG
        nv.call = lambda nm, *a: (calls.append(nm), real(nm, *a))[1]
        torch.randn_like = lambda t, **kw: noise.to(t.dtype)                 # the omega noise: the same draw on both routes
        _ops.USE_CEVA_LONG = on
        try:
            m.zero_grad()
            x = x0.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = m(x, x, x)[0]
            y.backward(dy.to(y.dtype))
        finally:
            nv.call, torch.randn_like, _ops.USE_CEVA_LONG = real, real_like, was
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        return dict(grads, y=y.detach(), dx=x.grad), calls

    new, calls = run(True)
    old, old_calls = run(False)
    assert {"ea_ceva_lm_fwd", "ea_ceva_lm_bwd_q", "ea_ceva_lm_bwd_k"} <= set(calls), sorted(set(calls))
    assert not [c for c in calls if c.startswith("ea_f32_attn")] and "ea_f32_attn_fwd" in old_calls
    assert set(new) == set(old) and len(new) >= 12
    for name in old:
        e = scaled_err(new[name].float().cpu().numpy(), old[name].float().cpu().numpy())
        print(name, e)
        assert e[0] <= MODULE_TOL[0] and e[1] <= MODULE_TOL[1], (name, e)
