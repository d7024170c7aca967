"""-m "not gpu": KernelizedAttention's feature maps (relu / fourier / relu-only / sigmoid-only / dpfp, cos weighting, the
fixed and learnable sample schemes) -- construction, state_dict tables against the reference fixtures, the argparse flags,
the refusals, and the fp64 restatement of the contract (tests/kz_contract.py) against every fixture."""
import argparse

import numpy as np
import pytest
import torch

import cases_kernelized
from kz_checks import KzFixture, contract_case

MAPS = ["favorp", "relu", "fourier", "relu-only", "sigmoid-only", "dpfp"]
SCHEMES = ["default", "fixed", "learnable"]


def _build(**kw):
    import efficient_attention as ea
    args = dict(dim=128, num_heads=2)
    args.update(kw)
    return ea.KernelizedAttention(**args)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("cos", [False, True])
@pytest.mark.parametrize("proj_method", MAPS)
def test_every_supported_combination_constructs(proj_method, cos, scheme):
    m = 128 if proj_method == "dpfp" else 64
    mod = _build(approx_attn_dim=m, proj_method=proj_method, cos_weighting=cos, sample_scheme=scheme)
    keys = {k: tuple(v.shape) for k, v in mod.state_dict().items() if k.endswith("_proj")}
    if proj_method in ("favorp", "relu", "fourier"):
        assert mod.use_random_proj
        assert keys == {("eval_proj" if scheme == "default" else "random_proj"): (2, m, 64)}
        assert ("random_proj" in dict(mod.named_parameters())) == (scheme == "learnable")
    else:
        assert not mod.use_random_proj and keys == {}
        assert mod.get_proj_matrix() is None


@pytest.mark.parametrize("name", sorted(cases_kernelized.CASES))
def test_state_dict_matches_the_reference(name):
    import efficient_attention as ea
    fx = KzFixture(name)
    mod = ea.AttentionFactory.build_attention(fx.case["attn"], dict(fx.case["args"]))
    assert {k: list(v.shape) for k, v in mod.state_dict().items()} == fx.key_shapes
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in fx.params_np.items()}, strict=True)
    learn = fx.case["args"]["sample_scheme"] == "learnable" and "random_proj" in fx.key_shapes
    assert ("random_proj" in dict(mod.named_parameters())) == learn


def test_argparse_flags_reach_the_constructor():
    import efficient_attention as ea
    parser = argparse.ArgumentParser()
    ea.KernelizedAttention.add_attn_specific_args(parser)
    ns = parser.parse_args(["--approx-attn-dim", "32", "--proj-method", "fourier", "--cos-weighting",
                            "--sample-scheme", "learnable"], namespace=ea.NestedNamespace())
    mod = ea.AttentionFactory.build_attention("performer", dict(vars(ns.attn_args), dim=128, num_heads=2))
    assert (mod.approx_attn_dim, mod.proj_method, mod.cos_weighting, mod.sample_scheme) == (32, "fourier", True, "learnable")
    assert tuple(mod.random_proj.shape) == (2, 32, 64) and mod.random_proj.requires_grad


def test_refusals_name_their_case():
    with pytest.raises(NotImplementedError, match="mlp-fourier"):
        _build(approx_attn_dim=64, proj_method="mlp-fourier")
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        _build(dim=128, num_heads=4, approx_attn_dim=64, proj_method="relu")          # d = 32
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        _build(dim=128, num_heads=4, approx_attn_dim=64, proj_method="favorp", cos_weighting=True)
    with pytest.raises(NotImplementedError, match="features"):
        _build(approx_attn_dim=128, proj_method="fourier", cos_weighting=True)        # 512 features
    with pytest.raises(NotImplementedError, match="features"):
        _build(approx_attn_dim=384, proj_method="dpfp")                               # nu = 3: 384 features
    with pytest.raises(NotImplementedError, match="approx_attn_dim"):
        _build(approx_attn_dim=40, proj_method="relu")                                # not a multiple of 16
    with pytest.raises(NotImplementedError, match="approx_attn_dim"):
        _build(approx_attn_dim=160, proj_method="relu")                               # m > 128
    with pytest.raises(AssertionError):
        _build(approx_attn_dim=64, proj_method="dpfp")                                # nu = (64 // 64) // 2 = 0
    with pytest.raises(NotImplementedError):
        _build(approx_attn_dim=64, proj_method="nope")


@pytest.mark.parametrize("kw", [dict(proj_method="relu"), dict(proj_method="fourier"), dict(proj_method="dpfp"),
                                dict(proj_method="favorp", cos_weighting=True), dict(sample_scheme="learnable")])
def test_scatterbrain_refuses_other_feature_maps(kw):
    import efficient_attention as ea
    args = dict(dim=128, num_heads=2, approx_attn_dim=128, window_size=7, attn_2d=True)
    args.update(kw)
    with pytest.raises(NotImplementedError):
        ea.ScatterBrain(**args)


def test_fixture_sizes_and_clamp_regime():
    import os
    from util import GOLDEN_DIR
    for name in cases_kernelized.CASES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, name + ".npz")) < 512 * 1024, name
    fx = KzFixture("kz_fourier_2d_clamp")
    for mode in cases_kernelized.MODES:
        assert 0.2 < float(fx.z["%s.clamped_fraction" % mode]) < 0.8


@pytest.mark.parametrize("mode", cases_kernelized.MODES)
@pytest.mark.parametrize("name", sorted(cases_kernelized.CASES))
def test_fp64_restatement_matches_the_reference(name, mode):
    """The yardstick of the full-size GPU tests agrees with the reference's own outputs on every fixture."""
    fx = KzFixture(name)
    y, dx, grads, stats = contract_case(fx, mode)
    frac = float((stats["den"] < 1e-2).double().mean())
    assert abs(frac - float(fx.z["%s.clamped_fraction" % mode])) < 1e-9

    def close(got, ref, what):
        # 1e-5 of the tensor's scale (rms), and every element within 2e-5 of its max: the reference runs in fp32, and in
        # the clamp fixture its rounding reaches 1.2e-5 of max |dx|
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        d = got - ref
        rms = np.sqrt((d * d).mean()) / max(np.sqrt((ref * ref).mean()), 1e-30)
        mx = np.abs(d).max() / max(np.abs(ref).max(), 1e-30)
        assert rms <= 1e-5 and mx <= 2e-5, (name, mode, what, rms, mx)
    close(y.numpy(), fx.y(mode), "y")
    close(dx.numpy(), fx.dx(mode), "dx")
    for key in fx.grad_keys(mode):
        got, ref = fx.grad_ref(mode, key, grads[key].numpy())
        close(got, ref, "d" + key)
