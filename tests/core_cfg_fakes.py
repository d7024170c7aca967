"""The cases of tests/golden/core_cfg_fakes.json: torch.ops.ea.{lara,eva,local}_{fwd,bwd} under FakeTensorMode (fake CUDA tensors
need no GPU; the LARA fake asks the library's host-side plan query).  tools/record_core_cfg_fakes.py wrote the golden file from
these cases; tests/test_core_cfg_cpu.py runs them again.  The op arguments are literal int / float lists: the public schema."""
import os

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

B, N, H, D = 2, 196, 2, 64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

# name -> (icfg, fcfg, generator parameters: see _params)
LARA = {
    "opcheck": ([14, 14, 2, 1, 1, 0, 0, 1], [2.0, 0.125], "WbgcWbgc"),
    "trailing0": ([14, 14, 2, 1, 1, 0, 0, 0], [2.0, 0.125], "WbgcWbgc"),
    "absent": ([14, 14, 2, 1, 1, 0, 0], [2.0, 0.125], "WbgcWbgc"),
    "mis1": ([14, 14, 2, 1, 1, 1, 0, 1], [2.0, 0.125], "WbgcWbgc"),
    "mis2": ([14, 14, 2, 1, 1, 2, 0, 1], [2.0, 0.125], "WbgcWbgc"),
    "no_mlp": ([14, 14, 2, 0, 1, 0, 0, 1], [2.0, 0.125], ""),
    "dup": ([14, 14, 2, 1, 1, 0, 1, 1], [2.0, 0.125], "WbgcWbgc"),            # C = 98: the step-by-step shape
}
# name -> (icfg, fcfg, adaptive_proj, bias shape | None, mu-network parameters)
EVA = {
    "opcheck": ([1, 14, 14, 7, 0, 7, 4, 0, 1], [0.5, 1.0], "default", (H, 49, 49), "WbgcWbgc"),
    "no_bias": ([1, 14, 14, 7, 0, 7, 4, 0, 1], [0.5, 1.0], "default", None, "WbgcWbgc"),
    "trailing0": ([1, 14, 14, 7, 0, 7, 4, 0, 0], [0.5, 1.0], "default", (H, 49, 49), "WbgcWbgc"),
    "absent": ([1, 14, 14, 7, 0, 7, 4, 0], [0.5, 1.0], "default", (H, 49, 49), "WbgcWbgc"),
    "no_ln": ([1, 14, 14, 7, 0, 7, 4, 0, 1], [0.5, 1.0], "no-ln", (H, 49, 49), "WbWb"),
    "no_ln_trailing0": ([1, 14, 14, 7, 0, 7, 4, 0, 0], [0.5, 1.0], "no-ln", (H, 49, 49), "WbWb"),
    "none": ([1, 14, 14, 7, 0, 7, 4, 0, 1], [0.5, 1.0], "none", (H, 49, 49), "Wbgc"),
    "none_trailing0": ([1, 14, 14, 7, 0, 7, 4, 0, 0], [0.5, 1.0], "none", (H, 49, 49), "Wbgc"),
    "mu1": ([1, 14, 14, 7, 0, 7, 4, 0, 1], [1.0, 1.0], "default", (H, 49, 49), "WbgcWbgc"),      # not the fused mu networks
    "causal_1d": ([0, 196, 0, 14, 7, 14, 14, 2, 1], [1.0, 1.25], "default", (H, 14, 21), "WbgcWbgc"),
    "causal_1d_no_ln": ([0, 196, 0, 14, 0, 14, 14, 2], [1.0, 1.0], "no-ln", None, "WbWb"),
}
# name -> (geo, bias shape | None)
LOCAL = {
    "2d_bias": ([1, 14, 14, 7, 0], (H, 49, 49)),
    "2d": ([1, 14, 14, 7, 0], None),
    "1d_ext_bias": ([0, 196, 0, 14, 7], (H, 14, 28)),
}

CASES = (["lara/%s/composite%s/%s" % (n, c, dt) for n in LARA for c in "10" for dt in DTYPES]
         + ["eva/%s/%s" % (n, dt) for n in EVA for dt in DTYPES]
         + ["local/%s/%s" % (n, dt) for n in LOCAL for dt in DTYPES])


def _f32(*shape):
    return torch.empty(shape, dtype=torch.float32, device="cuda")


def _params(layout):
    """The landmark / mu networks' parameters, one per letter: W a [d, d] matrix, anything else a [d] vector."""
    return [_f32(D, D) if c == "W" else _f32(D) for c in layout]


def _sig(ts):
    return [[list(t.shape), str(t.dtype)] for t in ts]


def run(case):
    """-> {"fwd": [[shape, dtype] ...], "bwd": [...]} of one case; the backward op is fed what the forward op returned.
    The caller sets EA_LARA_COMPOSITE for the lara cases (the fake takes the composite decision at call time)."""
    import efficient_attention  # noqa: F401  (registers torch.ops.ea.*)
    family, name, *rest = case.split("/")
    dtype = DTYPES[rest[-1]]
    ops = torch.ops.ea
    with FakeTensorMode():
        qkv = torch.empty((B, N, 3, H, D), dtype=dtype, device="cuda")
        dout = torch.empty((B, N, H, D), dtype=dtype, device="cuda")
        if family == "lara":
            assert os.environ.get("EA_LARA_COMPOSITE", "1") == rest[0][-1]
            icfg, fcfg, n = LARA[name]
            params, noise = _params(n), _f32(B, H, 49, D)
            fwd = ops.lara_fwd(qkv, None, noise, icfg, fcfg, params)
            bwd = ops.lara_bwd(dout, qkv, None, noise, fwd[1:], icfg, fcfg, params)
        elif family == "eva":
            icfg, fcfg, adaptive, bshape, n = EVA[name]
            params, noise = _params(n), _f32(B, H, icfg[6], D)
            bias = None if bshape is None else _f32(*bshape)
            fwd = ops.eva_fwd(qkv, bias, noise, None, None, icfg, fcfg, adaptive, params)
            bwd = ops.eva_bwd(dout, qkv, None, None, noise, fwd[0], fwd[1:], icfg, fcfg, adaptive,
                              0 if bshape is None else bshape[-1], params)
        else:
            geo, bshape = LOCAL[name]
            bias = None if bshape is None else _f32(*bshape)
            fwd = ops.local_fwd(qkv, bias, None, geo)
            bwd = ops.local_bwd(dout, None, qkv, None if bias is None else fwd[2], None, fwd[0], fwd[1], geo,
                                0 if bshape is None else bshape[-1])
        return {"fwd": _sig(fwd), "bwd": _sig(bwd)}
