#!/usr/bin/env python3
"""Generate the golden vectors of KernelizedAttention's feature maps (cases_kernelized.CASES) by RUNNING THE REFERENCE.

Same scheme as gen_golden.py, whose reference import and noise injection it reuses: the reference module is built with the
case's kwargs, loaded with cases.make_params, fed the seeded inputs, and its outputs (y, dL/dx, dL/dtheta for L = sum(y*g),
`random_proj` included when learnable) are stored per mode.  Additionally `<mode>.clamped_fraction`: the fraction of
(b, h, query) rows whose normaliser phi(q).sum phi(k) lies below the clamp 1e-2 (recorded from the reference's own
linear_attention inputs).

    python tests/golden/gen_golden_kernelized.py            # every case
    python tests/golden/gen_golden_kernelized.py kz_relu_2d
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402
import cases_kernelized as kz  # noqa: E402
import gen_golden  # noqa: E402


GRAD_FULL_MAX = 8192      # (cases.GRAD_FULL_MAX is 16384: the output projection's gradient would push a 2-D fixture past 0.5 MB)


def pack_grad(name, key, arr):
    """cases.pack_grad with the smaller full-storage limit: larger gradients as cases.grad_sample_index samples + moments."""
    arr = np.asarray(arr, np.float32)
    if arr.size <= GRAD_FULL_MAX:
        return {"": arr}
    idx = cases.grad_sample_index(name, key, arr.size)
    flat = arr.reshape(-1)
    return {".sample": flat[idx],
            ".moments": np.array([flat.sum(dtype=np.float64), np.abs(flat).sum(dtype=np.float64),
                                  (flat.astype(np.float64) ** 2).sum()], np.float64)}


def run_case(ref, name):
    case = kz.CASES[name]
    torch.manual_seed(0)
    mod = ref.AttentionFactory.build_attention(case["attn"], cases.ctor_args(case))
    sd = mod.state_dict()
    key_shapes = {k: list(v.shape) for k, v in sd.items()}
    params = cases.make_params(name, key_shapes)
    mod.load_state_dict({k: (torch.from_numpy(params[k]).to(v.dtype) if k in params else v) for k, v in sd.items()},
                        strict=True)
    ka = sys.modules[type(mod).__module__]
    seen = []

    def cos_linear(q, k, v, lengths=None, eps=1e-2, _f=ka.cos_reweighted_linear_attention):
        n = q.shape[-2]
        t = torch.outer(torch.ones(1), (torch.pi / 2) * torch.arange(n, dtype=q.dtype) / n).reshape(1, 1, n, 1)
        qq, kk = torch.cat([q * t.cos(), q * t.sin()], -1), torch.cat([k * t.cos(), k * t.sin()], -1)
        seen.append(torch.einsum("...nm,...m->...n", qq, kk.sum(-2)))
        return _f(q, k, v)

    def plain_linear(q, k, v, eps=1e-2, _f=ka.linear_attention):
        seen.append(torch.einsum("...nm,...m->...n", q, k.sum(-2)))
        return _f(q, k, v, eps)

    x_np, g_np, mask_np = kz.make_inputs(name)
    out = {"key_shapes": np.array(json.dumps(key_shapes))}
    real = (ka.linear_attention, ka.cos_reweighted_linear_attention)
    ka.linear_attention, ka.cos_reweighted_linear_attention = plain_linear, cos_linear
    try:
        for mode in kz.MODES:
            mod.train(mode == "train")
            mod.zero_grad(set_to_none=True)
            seen.clear()
            x = torch.from_numpy(x_np).clone().requires_grad_(True)
            mask = None if mask_np is None else torch.from_numpy(mask_np)
            with gen_golden._NoisePatch(name) as np_patch:
                y = cases.call_module(case, mod, x, mask)
            (y * torch.from_numpy(g_np)).sum().backward()
            assert torch.isfinite(y).all(), (name, mode)
            out["%s.y" % mode] = y.detach().numpy()
            out["%s.dx" % mode] = x.grad.numpy()
            out["%s.noise_shapes" % mode] = np.array(json.dumps(np_patch.calls))
            out["%s.clamped_fraction" % mode] = np.array(float((seen[0].detach() < 1e-2).double().mean()))
            for k, p in mod.named_parameters():
                gnp = np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.numpy()
                for suffix, arr in pack_grad(name, k, gnp).items():
                    out["%s.grad.%s%s" % (mode, k, suffix)] = arr
    finally:
        ka.linear_attention, ka.cos_reweighted_linear_attention = real
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    return path, os.path.getsize(path), float(out["eval.clamped_fraction"]), float(out["train.clamped_fraction"])


def main(argv):
    ref = gen_golden._import_reference()
    for name in argv or list(kz.CASES):
        path, size, ce, ct = run_case(ref, name)
        print("%-30s %8.1f KB   clamped eval %.3f train %.3f" % (name, size / 1024.0, ce, ct))


if __name__ == "__main__":
    main(sys.argv[1:])
