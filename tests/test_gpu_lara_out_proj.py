"""-m gpu: the LARA forward combine with the output projection inside (ea_lara_xp.hip; ea_lara_layer_fwd_proj,
ea_lara_out_proj_fwd_merge, C ABI 29) against the two launches it replaces, ea_lara_layer_fwd + ea_linear[192->192].

out, the per-token statistics and the merged per-landmark tensors: bit for bit (the whole `saved` workspace is compared).
y: both paths against an fp64 product of the (identical) rounded `out` and the rounded weight, in units of the derivable bound
    u = 1/2 ulp_E(|ref|) + 192 * 2^-24 * sum_k |out_k w_k|
(products of 16-bit values are exact in fp32: only the 192-term fp32 sum and the one final rounding err).  The fused path's
largest error may not exceed 1.5 x max(1, the two-launch path's): two summation orders draw different last-bit errors from one
distribution, nothing bigger.  Every element of y is compared (y is pre-filled with NaN).
The kernel takes its k-slots and its order of accumulation from lin_kernel, so y is ALSO asserted equal to ea_linear's bit for
bit (tests/test_gpu_primitives.py::test_prepared_weight_path_is_bit_identical needs exactly that of the module).
Measured on MI355X, largest error over all cases of test_direct_call: 0.999 u for both paths (bf16), 0.985 u (fp16)."""
import ctypes
import os

import pytest

pytestmark = pytest.mark.gpu

_MANT = {"bfloat16": 7, "float16": 10}


def _err_units(y, out2, w16, bias32):
    """max over ALL elements of |y - ref| / u, ref = fp64(out2) fp64(w16)^T + fp64(bias rounded to the element type)."""
    import torch
    o64, w64 = out2.double(), w16.double()
    ref = o64 @ w64.t()
    mag = o64.abs() @ w64.abs().t()
    if bias32 is not None:
        ref = ref + bias32.to(w16.dtype).double()
    p = _MANT[str(w16.dtype).split(".")[1]]
    _, e = torch.frexp(ref.abs())                       # |ref| = m 2^e, m in [0.5, 1): ulp = 2^(e - 1 - p)
    if w16.dtype == torch.float16:
        e = e.clamp(min=-13)                            # subnormals: ulp stays 2^-24
    u = 0.5 * torch.exp2((e - 1 - p).double()) + 192 * 2.0 ** -24 * mag
    err = (y.double() - ref).abs() / u
    assert err.numel() == y.numel() and not bool(torch.isnan(err).any()), "an element of y was not written"
    return float(err.max())


def _inputs(B, H, W, r, h, d, dtype, mis, dup=0, has_mlp=1, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + 7 * mis + B)
    L = (H // r) * (W // r)
    qkv = (0.5 * torch.randn(B, H * W, 3, h, d, device="cuda", generator=g)).to(dtype)
    noise = torch.randn(B, h, L, d, device="cuda", generator=g)
    params = []
    if has_mlp:
        for _ in range(2):
            params += [torch.randn(d, d, device="cuda", generator=g) * d ** -0.5, torch.randn(d, device="cuda", generator=g) * 0.1,
                       1 + 0.1 * torch.randn(d, device="cuda", generator=g), 0.1 * torch.randn(d, device="cuda", generator=g)]
    C = h * d
    w16 = (torch.randn(C, C, device="cuda", generator=g) * C ** -0.5).to(dtype)
    bias = 0.2 * torch.randn(C, device="cuda", generator=g)
    icfg = [H, W, r, has_mlp, 1, mis, dup, 1]
    return qkv, noise, params, w16, bias, icfg, [2.0, d ** -0.5]


def _layer_fwd(qkv, noise, params, icfg, fcfg, keep, proj=None):
    """The composite C entry on zero-filled workspaces (so that unwritten padding compares equal) -> (rc, out, saved, y)."""
    import torch
    from efficient_attention import _native as nv, _ops
    lcfg, sizes = _ops._lara_layer_cfg(qkv, icfg, fcfg)
    assert lcfg is not None
    B, N, _, h, d = qkv.shape
    q, k, v = _ops._qkv_views(qkv)
    tq, tk, tv = nv.t4(q), nv.t4(k), nv.t4(v)
    ws = torch.zeros(sizes.n_saved, dtype=torch.float32, device="cuda")
    tmp = torch.zeros(sizes.n_fwd_tmp, dtype=torch.float32, device="cuda")
    out = torch.zeros((B, N, h, d), dtype=qkv.dtype, device="cuda")
    to = nv.t4(out.permute(0, 2, 1, 3))
    ps = [t.float().contiguous() for t in params]
    pp = _ops._param_ptrs(ps) if ps else None
    args = (ctypes.byref(lcfg), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), None, nv.ptr(noise), pp, ctypes.byref(to),
            nv.ptr(ws), nv.ptr(tmp), int(keep))
    if proj is None:
        return nv.lib().ea_lara_layer_fwd(*args, nv.stream()), out, ws, None
    w16, bias = proj
    y = torch.full((B * N, h * d), float("nan"), dtype=qkv.dtype, device="cuda")
    rc = nv.lib().ea_lara_layer_fwd_proj(*args, nv.ptr(w16), nv.ptr(bias), nv.ptr(y), y.stride(0), nv.stream())
    return rc, out, ws, y


def _s_fwd(B, h, N, d, dtype, C, mis):
    from efficient_attention import _native as nv
    g = nv.ea_lara_geom(B, h, N, d, 0 if "bfloat16" in str(dtype) else 1, C, mis, 2.0, d ** -0.5)
    return nv.lib().ea_lara_parts(ctypes.byref(g))


# (grid, r): N = 36 < one 64-token step, C = 9 | N = 196 = 12.25 tiles, C = 49: one real row in the last landmark tile | the
# benchmark's image.  B = 64 at 28 x 28 is the smallest batch at which that image runs the folded merge (S_fwd <= 4); at
# B = 1 and 3 its statistics pass cuts the sequence into 7 slices and the composite declines (asserted).
_CASES = [(H, W, r, B, t) for (H, W, r) in ((6, 6, 2), (14, 14, 2), (28, 28, 4)) for B in (1, 3) for t in ("bfloat16", "float16")]
_CASES.append((28, 28, 4, 64, "bfloat16"))


@pytest.mark.parametrize("H,W,r,B,dtype_name", _CASES)
def test_direct_call(H, W, r, B, dtype_name):
    import torch
    from efficient_attention import _ops
    dtype = getattr(torch, dtype_name)
    h, d, N, C = 3, 64, H * W, (H // r) * (W // r)
    worst = [0.0, 0.0]
    seen_S = set()
    for mis in (0, 1, 2):
        qkv, noise, params, w16, bias, icfg, fcfg = _inputs(B, H, W, r, h, d, dtype, mis)
        S = _s_fwd(B, h, N, d, dtype, C, mis)
        seen_S.add(S)
        for use_bias in (True, False):
            for keep in (0, 1):
                b = bias if use_bias else None
                rc0, out0, ws0, _ = _layer_fwd(qkv, noise, params, icfg, fcfg, keep)
                assert rc0 == 0
                y0 = _ops.ea_linear(out0.view(B * N, h * d), w16, b, dtype)[0]
                rc1, out1, ws1, y1 = _layer_fwd(qkv, noise, params, icfg, fcfg, keep, proj=(w16, b))
                if S > 4:
                    assert rc1 == -2                                    # declined before any launch: nothing was written
                    assert not bool(out1.any()) and not bool(ws1.any()) and bool(torch.isnan(y1).all())
                    continue
                assert rc1 == 0
                assert torch.equal(out1, out0)
                assert torch.equal(ws1, ws0)                            # lseZ / tmean, merged kv / lse_k / cst / lse_t, all else
                e0 = _err_units(y0, out0.view(B * N, h * d), w16, b)
                e1 = _err_units(y1, out0.view(B * N, h * d), w16, b)
                print("out_proj %dx%d r%d B%d %s mis%d bias%d keep%d S%d: two-launch %.3f u, fused %.3f u"
                      % (H, W, r, B, dtype_name, mis, use_bias, keep, S, e0, e1))
                worst = [max(worst[0], e0), max(worst[1], e1)]
                assert e1 <= 1.5 * max(1.0, e0), (e1, e0)
                assert torch.equal(y1, y0)
    print("out_proj %dx%d r%d B%d %s: S_fwd %s, largest error two-launch %.3f u, fused %.3f u"
          % (H, W, r, B, dtype_name, sorted(seen_S), worst[0], worst[1]))


@pytest.mark.parametrize("case", ["heads", "d"])
def test_declines(case):
    """Heads != 3, d != 64: the composite answers EA_E_UNSUPPORTED, and the layer (lara_fwd_impl asked to project) still gives
    exactly what the two calls give."""
    import torch
    from efficient_attention import _native as nv, _ops
    dtype = torch.bfloat16
    H, W, r, B, h, d = {"heads": (14, 14, 2, 2, 2, 64), "d": (14, 14, 2, 2, 6, 32)}[case]
    qkv, noise, params, w16, bias, icfg, fcfg = _inputs(B, H, W, r, h, d, dtype, 0, seed=3)
    N = H * W
    rc = _layer_fwd(qkv, noise, params, icfg, fcfg, 1, proj=(w16, bias))
    assert rc[0] == -2 and not bool(rc[1].any()) and not bool(rc[2].any()) and bool(torch.isnan(rc[3]).all())
    ref = _ops.lara_fwd_impl(qkv, None, noise, icfg, fcfg, params)
    y_ref = _ops.ea_linear(ref[0].view(B * N, h * d), w16, bias, dtype)[0]
    proj = [w16, bias, torch.full((B * N, h * d), float("nan"), dtype=dtype, device="cuda")]
    got = _ops.lara_fwd_impl(qkv, None, noise, icfg, fcfg, params, proj=proj)
    assert len(got) == len(ref) and torch.equal(got[0], ref[0]) and torch.equal(proj[2], y_ref)


def test_declines_more_than_64_samples():
    """C > 64 (antithetic sampling at 49 landmarks, training): the composite answers EA_E_UNSUPPORTED before any launch, and
    the layer's output and gradients are those of the two-call path exactly, whatever the switch says."""
    import warnings
    import torch
    import efficient_attention as ea
    from efficient_attention import _native as nv
    lcfg = nv.ea_lara_layer(2, 3, 64, 0, 14, 14, 2, 1, 1, 0, 1, 2.0, 0.125)
    assert nv.lib().ea_lara_layer_fwd_proj(ctypes.byref(lcfg), *([None] * 9), 1, None, None, None, 192, None) == -2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(13)
        m = ea.AttentionFactory.build_attention("lara", dict(dim=192, num_heads=3, num_landmarks=49, proposal_gen="pool-mixed",
                                                             mis_type="mis-opt", alpha_coeff=2.0, use_antithetics=True)).cuda()
    m.train(True)
    x0 = torch.randn(2, 14, 14, 192, device="cuda")
    g = torch.randn(2, 14, 14, 192, device="cuda").bfloat16()
    res = {}
    for fused in ("1", "0"):
        os.environ["EA_LARA_OUT_PROJ"] = fused
        try:
            for p in m.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            torch.manual_seed(5)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = m(x)
            y.backward(g)
            res[fused] = (y.detach(), x.grad, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
        finally:
            os.environ.pop("EA_LARA_OUT_PROJ", None)
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])
    for n in res["1"][2]:
        assert torch.equal(res["1"][2][n], res["0"][2][n]), n


def test_module_forward_backward():
    """LinearRA (14 x 14, B = 2, bf16 autocast), fused on and off: every gradient bit for bit (the backward gets the same saved
    tensors), y within the bound."""
    import warnings
    import torch
    import efficient_attention as ea
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(11)
        m = ea.AttentionFactory.build_attention("lara", dict(dim=192, num_heads=3, num_landmarks=49, proposal_gen="pool-mixed",
                                                             mis_type="mis-opt", alpha_coeff=2.0)).cuda()
    m.train(True)
    x0 = torch.randn(2, 14, 14, 192, device="cuda")
    g = torch.randn(2, 14, 14, 192, device="cuda").bfloat16()
    res = {}
    for fused in ("1", "0"):
        os.environ["EA_LARA_OUT_PROJ"] = fused
        try:
            for p in m.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            torch.manual_seed(5)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = m(x)
            assert type(y.grad_fn).__name__.startswith("LaraModuleFn")
            o2 = y.grad_fn.saved_tensors[2].clone()
            y.backward(g)
            res[fused] = (y.detach(), o2, x.grad, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
        finally:
            os.environ.pop("EA_LARA_OUT_PROJ", None)
    assert torch.equal(res["1"][1], res["0"][1])
    assert torch.equal(res["1"][2], res["0"][2])
    assert res["1"][3].keys() == res["0"][3].keys() and len(res["1"][3]) >= 4
    for n in res["1"][3]:
        assert torch.equal(res["1"][3][n], res["0"][3][n]), n
    w16 = m.proj.weight.detach().bfloat16()
    e1 = _err_units(res["1"][0].reshape(-1, 192), res["1"][1], w16, m.proj.bias.detach().float())
    e0 = _err_units(res["0"][0].reshape(-1, 192), res["0"][1], w16, m.proj.bias.detach().float())
    print("out_proj module 14x14 B2 bf16: two-launch %.3f u, fused %.3f u" % (e0, e1))
    assert e1 <= 1.5 * max(1.0, e0), (e1, e0)
    assert torch.equal(res["1"][0], res["0"][0])


def test_graph_capture():
    """The fused step captured in a graph: three replays, each equal to the eager result bit for bit on the same inputs."""
    import torch
    from efficient_attention import _ops
    dtype = torch.bfloat16
    H, W, r, B, h, d = 14, 14, 2, 2, 3, 64
    qkv, noise, params, w16, bias, icfg, fcfg = _inputs(B, H, W, r, h, d, dtype, 0, seed=5)
    N = H * W

    def step():
        proj = [w16, bias, torch.empty((B * N, h * d), dtype=dtype, device="cuda")]
        outs = _ops.lara_fwd_impl(qkv, None, noise, icfg, fcfg, params, proj=proj)
        return outs[0], outs[1], proj[2]
    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for _ in range(3):
        for t in held:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(held[0], eager[0]) and torch.equal(held[2], eager[2])
