"""Fixture access and module-level checks for the kernelized-attention feature maps (tests/golden/cases_kernelized.py)."""
import contextlib
import json
import os
import warnings

import numpy as np
import torch

import cases
import cases_kernelized
import kz_contract
from util import GOLDEN_DIR, Fixture, scaled_err, elementwise_excess


class KzFixture(Fixture):
    """util.Fixture over cases_kernelized.CASES (same parameter / noise streams, this table's inputs)."""

    def __init__(self, name):
        self.name = name
        self.case = cases_kernelized.CASES[name]
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.key_shapes = json.loads(str(self.z["key_shapes"]))
        self.params_np = cases.make_params(name, self.key_shapes)
        self.x_np, self.g_np, self.mask_np = cases_kernelized.make_inputs(name)

    def grad_ref(self, mode, key, got):
        """(got, ref) arrays for a parameter gradient: whole, or at the stored sample positions."""
        pre = "%s.grad.%s" % (mode, key)
        if pre in self.z.files:
            return np.asarray(got).reshape(self.z[pre].shape), self.z[pre]
        idx = cases.grad_sample_index(self.name, key, np.asarray(got).size)
        return np.asarray(got).reshape(-1)[idx], self.z[pre + ".sample"]


def feature_matrix(fx, mode, params, device, dtype):
    """The W the module uses in `mode` (default scheme in training: the first noise draw, [h, m, d]), or None."""
    a = fx.case["args"]
    if a["proj_method"] not in ("favorp", "relu", "fourier"):
        return None
    if a["sample_scheme"] == "default":
        if mode == "train":
            h, d = a["num_heads"], a["dim"] // a["num_heads"]
            return torch.from_numpy(cases.make_noise(fx.name, (h, a["approx_attn_dim"], d), 0)).to(device=device, dtype=dtype)
        return params["eval_proj"]
    return params["random_proj"]


def contract_case(fx, mode, device="cpu", dtype=torch.float64):
    """The fp64 restatement on a fixture: -> (y, dx, {param key: grad}, stats)."""
    a = fx.case["args"]
    params = {k: torch.from_numpy(v).to(device=device, dtype=dtype).requires_grad_(True) for k, v in fx.params_np.items()}
    W = feature_matrix(fx, mode, params, device, dtype)
    x = torch.from_numpy(fx.x_np).to(device=device, dtype=dtype).requires_grad_(True)
    mask = None if fx.mask_np is None else torch.from_numpy(fx.mask_np).to(device)
    stats = {}
    y = kz_contract.module_forward(x, params, a["num_heads"], a["proj_method"], a["approx_attn_dim"], a["cos_weighting"], W,
                                   mask, stats)
    (y * torch.from_numpy(fx.g_np).to(device=device, dtype=dtype)).sum().backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in params.items()}
    return y.detach(), x.grad, grads, stats


def build_module(fx, device="cuda"):
    import efficient_attention as ea
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mod = ea.AttentionFactory.build_attention(fx.case["attn"], cases.ctor_args(fx.case))
    sd = mod.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == fx.key_shapes
    mod.load_state_dict({k: (torch.from_numpy(fx.params_np[k]) if k in fx.params_np else v) for k, v in sd.items()},
                        strict=True)
    return mod.to(device)


def check_module_case(name, mode, dtype, tol, etol=None, backward=True):
    """The product module (HIP cores) on a fixture: y, dx and every parameter gradient (backward) within `tol` = (max, rms)
    scaled errors, and element-wise within `etol` (or None).  dtype: autocast dtype, or torch.float32 for no autocast."""
    from gpu_checks import injected_noise
    fx = KzFixture(name)
    mod = build_module(fx)
    mod.train(mode == "train")
    x = torch.from_numpy(fx.x_np).cuda().requires_grad_(True)
    mask = None if fx.mask_np is None else torch.from_numpy(fx.mask_np).cuda()
    with injected_noise(fx, mode, "cuda") as calls:
        with (torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else contextlib.nullcontext()):
            y = cases.call_module(fx.case, mod, x, mask)
    assert calls == fx.expected_noise_shapes(mode), (calls, fx.expected_noise_shapes(mode))
    assert y.shape == x.shape
    errs, elem = {}, {}

    def both(key, got, ref):
        errs[key] = scaled_err(got, ref)
        elem[key] = lambda coef, got=got, ref=ref: elementwise_excess(got, ref, coef)
    both("y", y.detach().float().cpu().numpy(), fx.y(mode))
    if backward:
        (y.float() * torch.from_numpy(fx.g_np).cuda()).sum().backward()
        both("dx", x.grad.float().cpu().numpy(), fx.dx(mode))
    for key, p in (mod.named_parameters() if backward else ()):
        got = np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.float().cpu().numpy()
        got, ref = fx.grad_ref(mode, key, got)
        if np.abs(ref).max() > 0:
            both("d" + key, got, ref)
        else:
            assert np.abs(got).max() == 0, key
    bad = {k: v for k, v in errs.items() if not (v[0] <= tol[0] and v[1] <= tol[1])}
    assert not bad, "%s/%s out of tolerance %s: %s (all: %s)" % (name, mode, tol, bad, errs)
    if etol is not None:
        ebad = {k: v(etol) for k, v in elem.items() if v(etol) > 1.0}
        assert not ebad, "%s/%s element-wise bound %s exceeded: %s" % (name, mode, etol, ebad)
    return errs
