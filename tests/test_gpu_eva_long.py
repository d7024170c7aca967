"""-m gpu: EVA past 64 landmarks on the 16-bit kernels (csrc/ea_eva_lm.hip, _ops.eva_lm_fwd / eva_lm_bwd).

Core: the dense landmark half of the softmax plus its join with a GIVEN window half (o_loc, lse_loc) against a plain torch
evaluation of the joint softmax on the same 16-bit-rounded operands, under the bound of the 16-bit window core
(tests/window_reference.py: a(got) <= 4 a(model) + f, the model being the same evaluation in fp32 with the kernels' documented
16-bit roundings -- P and dS packed for their MFMA, out and d o_loc stored in the I/O dtype, delta read from the stored out).
Module: EVA in training at 100 landmarks against the same module on the fp32 gathered-attention route it took before."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

MASK_VAL = -5e4


def _join(ops, dtype, round_to):
    """out, Z and every gradient of sum(dout * out) for the joint softmax over [window half | all L landmark columns]."""
    from window_reference import rnd
    q, lk, lv, o_loc, lse_loc, dout = [t.to(dtype) for t in ops]
    scale = q.shape[3] ** -0.5
    s = scale * q @ lk.transpose(-1, -2)
    Z = torch.logaddexp(lse_loc, torch.logsumexp(s, -1))
    p = torch.exp(s - Z[..., None])
    pk = rnd(p, round_to)
    w = torch.exp(lse_loc - Z)[..., None]
    out = rnd(w * o_loc + pk @ lv, round_to)
    delta = (dout * out).sum(-1, keepdim=True)
    ds = rnd(p * (dout @ lv.transpose(-1, -2) - delta), round_to)
    return dict(out=out, Z=Z, dq_lm=scale * ds @ lk, dlk=scale * ds.transpose(-1, -2) @ q,
                dlv=pk.transpose(-1, -2) @ dout, do_loc=rnd(w * dout, round_to),
                dlse_loc=w[..., 0] * ((dout * o_loc).sum(-1) - delta[..., 0]))


CORE_CASES = [  # B, h, N, L, d, slices (None: the planner's), rows at the end whose window half is fills only
    (1, 2, 100, 65, 64, None, 0),      # one landmark tile plus one row, a partial query tile
    (1, 2, 272, 136, 128, None, 0),    # a partial third tile of both
    (1, 2, 400, 128, 64, 3, 0),        # exact landmark tiles; 7 query tiles in slices of 3, 3, 1
    (1, 2, 272, 68, 64, 1, 40),
    (1, 2, 100, 577, 64, None, 0),     # images past 128 KB of LDS: landmark tiles stream through two slots
    (4, 16, 1024, 65, 64, None, 0)]    # 1024 query tiles on 256 CUs: a workgroup walks two, the second without staging


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,h,N,L,d,slices,fills", CORE_CASES)
def test_dense_landmark_half_and_join_match_fp64(B, h, N, L, d, slices, fills, dtype):
    from efficient_attention import _native as nv, _ops
    from window_reference import bound_report
    gen = torch.Generator().manual_seed(N + L + d)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    q, o_loc, dout = [rn(B, h, N, d).to(dtype) for _ in range(3)]
    lk, lv = rn(B, h, L, d), rn(B, h, L, d)
    lse_loc = math.log(32.0) + rn(B, h, N)
    if fills:            # no visible local key: the window half is 32 fills and the row must come out as the landmark half alone
        lse_loc[..., N - fills:] = MASK_VAL + math.log(32.0)
    ops = (q.double(), lk.to(dtype).double(), lv.to(dtype).double(), o_loc.double(), lse_loc.double(), dout.double())
    ref, model = _join(ops, torch.float64, None), _join(ops, torch.float32, dtype)

    g = nv.make_geom(B, h, N, d, nv.io_dtype(q), False, (N,), 32, 0, 1, L, 0)
    bnhd = lambda t: t.cuda().transpose(1, 2).contiguous()                   # [B,N,h,d] buffers, as the window kernels leave them
    qd, old, doutd = bnhd(q).transpose(1, 2), bnhd(o_loc), bnhd(dout)
    lsed = lse_loc.cuda()
    out, zl, img = _ops.eva_lm_fwd(g, qd, lk.cuda(), lv.cuda(), old, lsed)
    runs = [_ops.eva_lm_bwd(g, qd, img, old, lsed, out, doutd, zl, slices=slices) for _ in range(2)]
    do_loc, dlse, dq_lm, dlk, dlv = runs[0]
    got = dict(out=out.transpose(1, 2), Z=zl[..., 0], dq_lm=dq_lm.transpose(1, 2), dlk=dlk, dlv=dlv,
               do_loc=do_loc.transpose(1, 2), dlse_loc=dlse)
    bad = []
    for name, ref_t in ref.items():
        assert torch.isfinite(got[name].float()).all(), name
        stored16 = "out" if name in ("out", "do_loc") else name              # (the floor of a tensor stored in 16 bits)
        ok, txt, _ = bound_report(stored16, got[name].cpu(), model[name], ref_t, dtype)
        print(name, txt)
        if not ok:
            bad.append(txt)
    assert not bad, "\n".join(bad)
    assert torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][4], runs[1][4])     # no atomics: bit for bit


def _eva(**args):
    import efficient_attention as ea
    torch.manual_seed(5)
    return ea.AttentionFactory.build_attention("eva", dict(num_heads=2, **args)).cuda().train()


def _train_step(m, x0, dy, noise, mask, long_route):
    """One step under bf16 autocast -> (y, dx and every parameter gradient; the C-ABI entries it called with their geometry's L)."""
    from efficient_attention import _native as nv, _ops
    calls, real, real_like, was = [], nv.call, torch.randn_like, _ops.USE_EVA_LONG
    nv.call = lambda nm, *a: (calls.append((nm, getattr(getattr(a[0], "_obj", None), "L", None))), real(nm, *a))[1]
    torch.randn_like = lambda t, **kw: noise.to(t.dtype)                     # the omega noise: the same draw on both routes
    _ops.USE_EVA_LONG = long_route
    try:
        m.zero_grad()
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x, mask) if mask is not None else m(x)
        y.backward(dy.to(y.dtype))
    finally:
        nv.call, torch.randn_like, _ops.USE_EVA_LONG = real, real_like, was
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return dict(grads, y=y.detach(), dx=x.grad), calls


MODULES = {
    "2d": ((2, 20, 20, 128), dict(dim=128, window_size=5, attn_2d=True, use_rpe=True, num_landmarks=100), 0),
    "1d": ((2, 200, 128), dict(dim=128, window_size=8, overlap_window=True, use_t5_rpe=True, num_landmarks=100,
                               adaptive_proj="no-ln"), 13)}


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", sorted(MODULES))
def test_module_trains_past_64_landmarks_on_the_16_bit_kernels(geometry):
    """L = 100, d = 64: y, dx and every parameter gradient against the same module on the route it took before (fp32 up-cast,
    ea_f32_attn_*), and the new kernels ran in place of the fp32 ones."""
    from gpu_checks import MODULE_TOL
    from util import scaled_err
    shape, args, pad = MODULES[geometry]
    m = _eva(**args)
    x0, dy = torch.randn(*shape, device="cuda"), torch.randn(*shape, device="cuda")
    noise = torch.randn(2, 2, 100, 64, device="cuda")
    mask = None
    if pad:
        mask = torch.zeros(shape[0], shape[1], dtype=torch.bool, device="cuda")
        mask[1, shape[1] - pad:] = True
    new, calls = _train_step(m, x0, dy, noise, mask, True)
    old, old_calls = _train_step(m, x0, dy, noise, mask, False)
    names, old_names = {c[0] for c in calls}, {c[0] for c in old_calls}
    assert {"ea_eva_lm_fwd", "ea_eva_lm_bwd_q", "ea_eva_lm_bwd_k"} <= names, sorted(names)
    assert not [c for c in names if c.startswith("ea_f32_attn")] and "ea_f32_attn_fwd" in old_names
    assert set(new) == set(old) and len(new) >= 10
    for name in old:
        e = scaled_err(new[name].float().cpu().numpy(), old[name].float().cpu().numpy())
        print(name, e)
        assert e[0] <= MODULE_TOL[0] and e[1] <= MODULE_TOL[1], (name, e)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,grid,window,entry,L", [(64, 20, 5, "ea_f32_attn_fwd", None), (128, 16, 4, "ea_window_attn_fwd", 64)],
                         ids=["d32_L100", "d64_L64"])
def test_outside_the_envelope_the_routes_stay(dim, grid, window, entry, L):
    """Head dim 32 at 100 landmarks keeps the fp32 route; 64 landmarks keep the window kernels with their landmark columns."""
    m = _eva(dim=dim, window_size=window, attn_2d=True, use_rpe=True, num_landmarks=(grid // 2) ** 2, adaptive_proj="no-ln")
    x0 = torch.randn(2, grid, grid, dim, device="cuda")
    noise = torch.randn(2, 2, (grid // 2) ** 2, dim // 2, device="cuda")
    _, calls = _train_step(m, x0, torch.randn_like(x0), noise, None, True)
    hit = [c for c in calls if c[0] == entry]
    assert hit and (L is None or hit[0][1] == L) and not [c for c in calls if c[0].startswith("ea_eva_lm")], sorted(set(calls))
