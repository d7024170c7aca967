"""-m gpu: ScatterBrain with overlapping windows (overlap_window=True, ext = window // 2) -- the feature half and the
merge on the HIP kernels of ea_scatter.hip (ea_scatter_ov_*), not on torch device ops.

Comparators: the committed reference fixtures (scatterbrain_1d_overlap / scatterbrain_2d_overlap), the CPU oracle
(oracle.scatterbrain_core(..., ext_size)), and the module's own torch-op path behind `_ops.SCATTER_TORCH`."""
import math
import os
import sys
import warnings

import pytest
import torch

import cases
from gpu_checks import check_module_case, tol_for
from util import scaled_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

X_SCALE = 0.3          # the overlapping variant is finite for small keys only; 2d_w7_28 is NaN at 1.0
OV = dict(use_rpe=True, overlap_window=True)
# name: (x shape, constructor arguments); the last column of DESIGN 4b's table is the key patch Wk
GEOMETRIES = {
    "2d_w7_28": ((2, 28, 28, 192), dict(dim=192, num_heads=3, window_size=7, attn_2d=True, approx_attn_dim=64, **OV)),          # 169
    "2d_w7_56_m32": ((1, 56, 56, 192), dict(dim=192, num_heads=3, window_size=7, attn_2d=True, approx_attn_dim=32, **OV)),      # 169
    "2d_w8_32_m16": ((1, 32, 32, 128), dict(dim=128, num_heads=2, window_size=8, attn_2d=True, approx_attn_dim=16, **OV)),      # 256
    "1d_w16_1024": ((2, 1024, 512), dict(dim=512, num_heads=8, window_size=16, attn_2d=False, approx_attn_dim=64, **OV)),       # 32
    "1d_w64_512_m32": ((2, 512, 128), dict(dim=128, num_heads=2, window_size=64, attn_2d=False, approx_attn_dim=32, **OV)),     # 128
    "1d_w8_200": ((2, 200, 192), dict(dim=192, num_heads=3, window_size=8, attn_2d=False, approx_attn_dim=64, **OV)),           # 16
}


def _build(args):
    """Parameters seeded 21 and perturbed by 0.02, as tests/test_gpu_configs.py builds its modules."""
    import efficient_attention as ea
    torch.manual_seed(21)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ea.AttentionFactory.build_attention("scatterbrain", dict(args)).cuda()
    m.eval()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
    return m


def _ban_torch_ops(monkeypatch):
    def banned(*a, **k):
        raise AssertionError("torch einsum / logsumexp / logaddexp reached in ScatterBrain's overlapping feature half")
    for fn in ("einsum", "logsumexp", "logaddexp"):
        monkeypatch.setattr(torch, fn, banned)
    for fn in ("logsumexp", "logaddexp"):
        monkeypatch.setattr(torch.Tensor, fn, banned)


# ---- 1. the path is HIP ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", ["scatterbrain_1d_overlap", "scatterbrain_2d_overlap"])
def test_overlap_feature_half_stays_on_hip(name, mode, dtype, monkeypatch):
    """The reference fixtures with window overlap, forward and backward, with the torch ops of the former feature half
    replaced by functions that raise; tolerances: what gpu_checks.tol_for gives ScatterBrain in test_gpu_modules."""
    _ban_torch_ops(monkeypatch)
    errs = check_module_case(name, mode, dtype=torch.bfloat16 if dtype == "bf16" else torch.float16)
    print(name, mode, dtype, {k: "%.2e/%.2e" % v for k, v in errs.items()})


# ---- 2. sizes the fixtures do not reach, module level against the CPU oracle ------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_overlap_one_element_matches_oracle(name, monkeypatch):
    """tests/test_gpu_configs.py::test_one_element_matches_oracle for the overlapping geometries (input scale 0.3): y and dx
    of one batch element against the fp32 CPU oracle at tol_for("scatterbrain", "bf16", "test_gpu_configs")."""
    import oracle
    shape, args = GEOMETRIES[name]
    m = _build(args)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = (X_SCALE * torch.randn(*shape, device="cuda", generator=gen)).requires_grad_(True)
    gy = torch.randn(*shape, device="cuda", generator=gen)
    _ban_torch_ops(monkeypatch)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    (y.float() * gy).sum().backward()
    monkeypatch.undo()
    b = shape[0] // 2
    sl = slice(b, b + 1)
    params = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    xr = x.detach()[sl].cpu().requires_grad_(True)
    ref = oracle.module_forward("scatterbrain", dict(args), params, xr, None, training=False)
    (ref * gy[sl].cpu()).sum().backward()
    assert torch.isfinite(ref).all() and torch.isfinite(xr.grad).all(), "the oracle itself is not finite here"
    tol = tol_for("scatterbrain", "bf16", "test_gpu_configs")
    for what, got, want in (("y", y.detach().float()[sl].cpu(), ref.detach()), ("dx", x.grad[sl].cpu(), xr.grad)):
        e = scaled_err(got.numpy(), want.numpy())
        print(name, what, "%.3e/%.3e" % e, "tol", tol)
        assert e[0] <= tol[0] and e[1] <= tol[1], (name, what, e, tol)


# ---- 3. core level, same 16-bit operands ----------------------------------------------------------------------------------
def _core_errors(name, overlap, dtype):
    """m._scatter on HIP against an fp64 evaluation of oracle.scatterbrain_core on the same rounded qkv5:
    {out, dqkv: (max, rms) error scaled by the reference}."""
    import oracle
    from oracle import attention as oa
    shape, args = GEOMETRIES[name]
    args = dict(args, overlap_window=overlap)
    m = _build(args)
    B, *seq, C = shape
    h, d, N = args["num_heads"], 64, int(math.prod(seq))
    gen = torch.Generator(device="cuda").manual_seed(5)
    qkv5 = (X_SCALE * torch.randn(B, N, 3, h, d, device="cuda", generator=gen)).to(dtype)
    g = torch.randn(B, N, h, d, device="cuda", generator=gen).to(dtype)
    x = qkv5.clone().requires_grad_(True)
    out = m._scatter(x, None, list(seq))
    (out.float() * g.float()).sum().backward()
    a = oa.default_args("scatterbrain")
    a.update(args)
    e = m.ext_size
    params = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    xr = qkv5.double().cpu().requires_grad_(True)
    q, k, v = [xr[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    bias = oa._local_bias(params, a, h, e, d ** -0.5)
    ref = oracle.scatterbrain_core(q, k, v, None, args["attn_2d"], list(seq), args["window_size"], params["eval_proj"], bias,
                                   d ** -0.5, ext_size=e)                                   # [B,h,N,d]
    (ref.permute(0, 2, 1, 3) * g.double().cpu()).sum().backward()
    assert torch.isfinite(ref).all() and torch.isfinite(xr.grad).all(), "the oracle itself is not finite here"
    return {"out": scaled_err(out.detach().float().cpu().numpy(), ref.detach().permute(0, 2, 1, 3).numpy()),
            "dqkv": scaled_err(x.grad.float().cpu().numpy(), xr.grad.numpy())}


# What the NON-overlapping kernels (overlap_window=False: the kernels as they were before the overlapping ones were added)
# give in this harness on MI355X, (max, rms) of out | d qkv5.  The overlapping kernels are allowed TWICE these figures: they
# sum up to four times as many keys per window in the same arithmetic (16-bit PK / V operands, fp32 accumulation).
NON_OVERLAPPING = {
    ("2d_w7_28", "bf16"): {"out": (5.648e-3, 2.506e-3), "dqkv": (9.873e-3, 3.380e-3)},
    ("2d_w7_28", "fp16"): {"out": (7.422e-4, 3.143e-4), "dqkv": (9.306e-4, 4.225e-4)},
    ("1d_w64_512_m32", "bf16"): {"out": (6.266e-3, 2.579e-3), "dqkv": (6.495e-3, 3.629e-3)},
    ("1d_w64_512_m32", "fp16"): {"out": (5.790e-4, 3.250e-4), "dqkv": (6.819e-4, 4.572e-4)},
}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["2d_w7_28", "1d_w64_512_m32"])
def test_overlap_core_matches_fp64_oracle_on_the_same_operands(name, dtype):
    """`_scatter` with overlap against the fp64 oracle on the same 16-bit qkv5, bound 2 x NON_OVERLAPPING (above).  Observed
    with overlap on MI355X: 2d_w7_28 bf16 out 5.9e-3 / 2.5e-3, dqkv 7.3e-3 / 3.0e-3, fp16 7.5e-4 / 3.1e-4, 8.3e-4 / 3.8e-4;
    1d_w64_512_m32 bf16 5.5e-3 / 2.6e-3, 5.8e-3 / 3.2e-3, fp16 7.5e-4 / 3.3e-4, 4.8e-4 / 4.1e-4."""
    dt = torch.bfloat16 if dtype == "bf16" else torch.float16
    got = _core_errors(name, True, dt)
    base = NON_OVERLAPPING[(name, dtype)]
    for key in ("out", "dqkv"):
        print(name, dtype, key, "overlap %.3e/%.3e" % got[key], "non-overlapping (recorded) %.3e/%.3e" % base[key])
    for key in ("out", "dqkv"):
        assert got[key][0] <= 2 * base[key][0] and got[key][1] <= 2 * base[key][1], (name, dtype, key, got[key], base[key])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["2d_w7_28", "1d_w64_512_m32"])
def test_non_overlapping_core_in_the_same_harness(name, dtype):
    """The origin of NON_OVERLAPPING: the same harness with overlap_window=False stays at the recorded figures (to the 5 %
    that a different reduction order of the torch sums may move them), so the bound above keeps its meaning."""
    got = _core_errors(name, False, torch.bfloat16 if dtype == "bf16" else torch.float16)
    base = NON_OVERLAPPING[(name, dtype)]
    for key in ("out", "dqkv"):
        print(name, dtype, key, "non-overlapping %.3e/%.3e" % got[key], "recorded %.3e/%.3e" % base[key])
        assert got[key][0] <= 1.05 * base[key][0] and got[key][1] <= 1.05 * base[key][1], (name, dtype, key, got[key], base[key])


# ---- 4. the reference's NaN behaviour is kept -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,args", [
    ((2, 14, 14, 192), dict(dim=192, num_heads=3, window_size=7, attn_2d=True, approx_attn_dim=64, **OV)),
    ((2, 16, 128), dict(dim=128, num_heads=2, window_size=8, attn_2d=False, approx_attn_dim=32, **OV))])
def test_overlap_border_padding_gives_the_reference_nan(shape, args):
    """A grid of 2 x 2 windows / a 1-D sequence of two windows: every window's padding outweighs the keys outside its patch
    and the reference returns NaN for every row.  The kernels return the same (no clamp, no fault), and an ordinary call
    afterwards is correct."""
    import oracle
    m = _build(args)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = X_SCALE * torch.randn(*shape, device="cuda", generator=gen)
    params = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    ref = oracle.module_forward("scatterbrain", dict(args), params, x[:1].cpu(), None, training=False)
    rows_ref = torch.isfinite(ref.reshape(-1, shape[-1])).all(-1)
    assert not rows_ref.any(), "the oracle is finite somewhere: not the case this test is about"
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    torch.cuda.synchronize()
    rows = torch.isfinite(y.float().reshape(-1, shape[-1])).all(-1)
    assert not rows.any(), "%d of %d rows are finite" % (int(rows.sum()), rows.numel())
    errs = check_module_case("scatterbrain_2d_overlap", "eval")
    print({k: "%.2e/%.2e" % v for k, v in errs.items()})


# ---- 5. reproducible bits -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_overlap_feature_op_is_bit_reproducible():
    """ScatterFeatureFn (forward output, dq / dk / dv, d o_loc, d lse_loc) on fixed inputs at 2d_w7_28, twice."""
    from efficient_attention import _ops
    shape, args = GEOMETRIES["2d_w7_28"]
    m = _build(args)
    B, H, W, C = shape
    h, d, N = 3, 64, H * W
    gen = torch.Generator(device="cuda").manual_seed(5)
    qkv5 = (X_SCALE * torch.randn(B, N, 3, h, d, device="cuda", generator=gen)).to(torch.bfloat16)
    g = torch.randn(B, N, h, d, device="cuda", generator=gen).to(torch.bfloat16)
    proj = m.get_proj_matrix(device=qkv5.device, dtype=torch.float32)
    mask_u8 = _ops._mask_u8(None, B, N, qkv5.device)
    with torch.no_grad():
        o_loc, lse_loc = _ops.LocalAttnLseFn.apply(qkv5, m._table_bias(), mask_u8, True, (H, W), 7, m.ext_size)
    runs = []
    for _ in range(2):
        x, o, l = qkv5.clone().requires_grad_(True), o_loc.clone().requires_grad_(True), lse_loc.clone().requires_grad_(True)
        out = _ops.ScatterFeatureFn.apply(x, o, l, mask_u8, proj, True, (H, W), 7, m.ext_size)
        out.backward(g)
        runs.append((out.detach(), x.grad, o.grad, l.grad))
    assert m.ext_size == 3 and all(torch.isfinite(t.float()).all() for t in runs[0])
    for name, a, b in zip(("out", "dqkv", "d o_loc", "d lse_loc"), *runs):
        assert torch.equal(a, b), name


# ---- 6. single-node path --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("attn_2d", [True, False])
def test_overlap_single_node_path_equals_three_node_path(attn_2d, monkeypatch):
    """tests/test_gpu_primitives.py::test_scatterbrain_single_node_path_equals_three_node_path with overlap=True: the
    training step through CoreModuleFn + GraphCore against the three-node path."""
    import efficient_attention as ea
    from efficient_attention import _ops
    assert _ops.USE_CORE_MODULE_FN and _ops.USE_LARA_MODULE_FN and not _ops.SCATTER_TORCH
    torch.manual_seed(9)
    kw = dict(dim=192, num_heads=3, qkv_bias=True, attn_drop=0.0, proj_drop=0.0, window_size=7 if attn_2d else 8, attn_2d=attn_2d,
              use_rpe=True, overlap_window=True, approx_attn_dim=64)
    m = ea.AttentionFactory.build_attention("scatterbrain", kw).cuda().train()
    x = torch.randn(8, 28, 28, 192, device="cuda") if attn_2d else torch.randn(8, 200, 192, device="cuda")
    x = x * X_SCALE
    gy = torch.randn_like(x)
    res = []
    for on in (True, False):
        monkeypatch.setattr(_ops, "USE_GRAPH_CORE", on)
        for p in m.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(True)
        torch.manual_seed(11)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(xi)
        y.backward(gy.to(y.dtype))
        assert y.shape == x.shape
        res.append([y.float(), xi.grad] + [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in m.parameters()])
    names = ["y", "dx"] + [n for n, _ in m.named_parameters()]
    assert torch.equal(res[0][0], res[1][0])
    assert float(res[0][2 + [n for n, _ in m.named_parameters()].index("local_relative_position_bias_table")].abs().max()) > 0
    for n, a, b in zip(names, *res):
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), n
        assert torch.allclose(a, b, rtol=2e-3, atol=2e-3 * float(b.abs().max()) + 1e-12), \
            (n, float((a - b).abs().max()), float(b.abs().max()))


# ---- 8. memory ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_overlap_hip_path_needs_less_memory_than_the_torch_op_path(monkeypatch):
    """Peak allocated memory of one forward + backward of `_scatter` at 2d_w7_28 with batch 32: the HIP path keeps the
    per-window statistics on chip and a [BH, G, m, d] gradient workspace; the torch-op path gathers [B,h,G,Wk,m] and
    [B,h,G,Wk,d] in fp32 and keeps them for autograd."""
    from efficient_attention import _ops
    _, args = GEOMETRIES["2d_w7_28"]
    m = _build(args)
    B, N, h, d = 32, 784, 3, 64
    gen = torch.Generator(device="cuda").manual_seed(5)
    x0 = X_SCALE * torch.randn(B, N, h * d, device="cuda", generator=gen)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        qkv5 = m.project_qkv(x0).detach()                  # (the module's own q, k, v: the regime where the variant is finite)
    assert qkv5.shape == (B, N, 3, h, d) and qkv5.dtype == torch.bfloat16
    g = torch.randn(B, N, h, d, device="cuda", generator=gen).to(torch.bfloat16)
    peak = {}
    for path in ("hip", "torch", "hip"):                   # (the first pass also warms the allocator and the kernels up)
        monkeypatch.setattr(_ops, "SCATTER_TORCH", path == "torch")
        x = qkv5.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = m._scatter(x, None, [28, 28])
        out.backward(g)
        torch.cuda.synchronize()
        peak[path] = torch.cuda.max_memory_allocated() - base
        assert torch.isfinite(x.grad.float()).all(), path
        del x, out
    print("peak bytes above the inputs: HIP %d, torch ops %d" % (peak["hip"], peak["torch"]))
    assert peak["hip"] < peak["torch"], peak
