"""Golden-vector case table of KernelizedAttention's feature maps (proj_method relu / fourier / relu-only / sigmoid-only /
dpfp, cos weighting, learnable / fixed random features), kept apart from cases.CASES: test_oracle_golden.py runs every entry of
that table against the oracle, which has favorp only.  Inputs, parameters and sampling noise come from cases.py's generators
(seeded by the case name), so a fixture stores only what the reference computed.

    python tests/golden/gen_golden_kernelized.py [names...]      (build container only: runs the reference)
"""
import numpy as np

import cases

_2D = (1, 14, 14, 128)
_1D = (2, 50, 128)
_PAD = ("tail", [0, 9])


def _kz(x_shape, mask, proj_method, m=64, cos=False, scheme="default", **extra):
    return dict(attn="performer", x_shape=x_shape, mask=mask,
                args=dict(dim=128, num_heads=2, approx_attn_dim=m, proj_method=proj_method, cos_weighting=cos,
                          sample_scheme=scheme), **extra)


CASES = {
    "kz_favorp_2d_cos": _kz(_2D, None, "favorp", cos=True, x_scale=0.3),
    "kz_favorp_1d_learnable": _kz(_1D, _PAD, "favorp", scheme="learnable", x_scale=0.3),
    "kz_relu_2d": _kz(_2D, None, "relu"),
    "kz_relu_1d_cos": _kz(_1D, _PAD, "relu", cos=True),
    "kz_relu_2d_learnable": _kz(_2D, None, "relu", scheme="learnable"),
    "kz_relu_1d_fixed_fullpad": _kz((2, 24, 128), ("tail", [0, 24]), "relu", scheme="fixed"),    # one fully padded row
    "kz_fourier_2d": _kz(_2D, None, "fourier", x_scale=0.3),
    "kz_fourier_1d_cos_f256": _kz(_1D, _PAD, "fourier", cos=True, x_scale=0.3),                  # 2 m * 2 = 256 features
    # part of the queries under the clamp of the normaliser (fourier features can be negative): clamped fraction recorded
    "kz_fourier_2d_clamp": _kz(_2D, None, "fourier", x_scale=0.8),
    "kz_fourier_1d_learnable": _kz(_1D, _PAD, "fourier", scheme="learnable", x_scale=0.3),
    "kz_reluonly_2d_cos": _kz(_2D, None, "relu-only", cos=True),
    "kz_reluonly_1d": _kz(_1D, _PAD, "relu-only"),
    "kz_sigmoidonly_2d": _kz(_2D, None, "sigmoid-only"),
    "kz_sigmoidonly_1d_cos": _kz(_1D, _PAD, "sigmoid-only", cos=True),
    "kz_dpfp_2d_nu1_cos": _kz(_2D, None, "dpfp", m=128, cos=True),                               # nu = 1, 256 features
    "kz_dpfp_1d_nu2": _kz(_1D, _PAD, "dpfp", m=256),                                              # nu = 2, 256 features
}

MODES = cases.MODES


def make_inputs(name):
    """x, cotangent g, key_padding_mask of a case (cases.make_inputs' streams, this table's shapes)."""
    case = CASES[name]
    x = (case.get("x_scale", 1.0) * cases.rng_for(name, "x").standard_normal(case["x_shape"])).astype(np.float32)
    g = cases.rng_for(name, "g").standard_normal(case["x_shape"]).astype(np.float32)
    mask = None
    if case["mask"] is not None:
        kind, pads = case["mask"]
        assert kind == "tail"
        B, N = case["x_shape"][0], case["x_shape"][1]
        mask = np.zeros((B, N), dtype=bool)
        for b, p in enumerate(pads):
            if p:
                mask[b, N - p:] = True
    return x, g, mask
