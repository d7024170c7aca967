"""Host side of kernelized attention with every feature map of the reference (csrc/ea_kernelized.hip).

KernelizedAttention's feature maps (kernelized_attention.py: favorp / relu / fourier / relu-only / sigmoid-only / dpfp),
optionally with cos weighting, and learnable random features: the functional forward / backward (C-ABI launches on the
current stream), the autograd Function, and the core spec of the single-node module path (_ops.CoreModuleFn).  Like the
Performer's exact-fp32 core the arithmetic is fp32 whatever the I/O type (the reference runs its linear attention in full
precision, kernelized_attention.py:345): bf16 / fp16 qkv under autocast, fp32 outside it, fp32 features and products.

A configuration is `cfg = (map id, m, nu, cos)`; W is the [h, m, 64] fp32 feature matrix of the maps that have one, else
None.  With `learn`, W receives its gradient (sample_scheme='learnable')."""
import torch

from . import _feature_cores as _fc
from . import _native as nv
from ._ops import Core, _ea_op, _IO32

MAPS = {"favorp": 0, "relu": 1, "fourier": 2, "relu-only": 3, "sigmoid-only": 4, "dpfp": 5}
W_MAPS = ("favorp", "relu", "fourier")
STAT_MAPS = (0, 2)                 # map ids with a sequence statistic (favorp's key stabiliser, fourier's maxima)
MAX_FEATURES = 256
MAX_M = 128


def feature_count(proj_method, m, d, cos_weighting):
    """Features the map produces (after cos weighting)."""
    if proj_method in ("favorp", "relu"):
        f = m
    elif proj_method == "fourier":
        f = 2 * m
    elif proj_method in ("relu-only", "sigmoid-only"):
        f = d
    elif proj_method == "dpfp":
        f = 2 * d * ((m // d) // 2)
    else:
        raise ValueError(proj_method)
    return f * (2 if cos_weighting else 1)


def make_cfg(proj_method, m, d, cos_weighting):
    nu = (m // d) // 2 if proj_method == "dpfp" else 0
    return (MAPS[proj_method], int(m) if proj_method in W_MAPS else 0, nu, 1 if cos_weighting else 0)


def _features(cfg):
    map_id, m, nu, cos = cfg
    f = {0: m, 1: m, 2: 2 * m, 3: 64, 4: 64, 5: 128 * nu}[map_id]
    return f * (2 if cos else 1)


def _has_stat(cfg):
    return cfg[0] in STAT_MAPS


def _geom(qkv5, cfg):
    B, N, _, h, d = qkv5.shape
    map_id, m, nu, cos = cfg
    return nv.ea_kz_geom(B, h, N, d, _IO32[qkv5.dtype], map_id, m, _features(cfg), nu, cos)


def _parts(geom):
    return nv.query("ea_kernelized_parts", geom)


_FAMILY = _fc.Family("ea_kernelized_", "stats", stats_take_q=True, q_side_stat=True, has_dw=True)


def kernelized_fwd_impl(qkv5, mask_u8, W, cfg):
    """torch.ops.ea.kernelized_fwd -> [out [B,N,h,d], p_st [BH,S,2] (empty for the maps without statistics), kv [BH,F,d],
    ksum [BH,F]]."""
    nv.require_cuda(qkv5, "qkv")
    cfg = tuple(int(c) for c in cfg)
    geom = _geom(qkv5, cfg)
    return list(_fc.forward(_FAMILY, geom, _parts(geom), _features(cfg), qkv5, mask_u8, W,
                            (2,) if _has_stat(cfg) else None))


def kernelized_bwd_impl(dout, qkv5, mask_u8, W, p_st, kv, ksum, cfg, need_dw):
    """torch.ops.ea.kernelized_bwd -> [dqkv [B,N,3,h,d], dW [h,m,d] fp32 (need_dw) or empty]."""
    cfg = tuple(int(c) for c in cfg)
    geom = _geom(qkv5, cfg)
    dqkv5, dW = _fc.backward(_FAMILY, geom, _parts(geom), _features(cfg), dout, qkv5, mask_u8, W,
                             p_st, kv, ksum, need_dw)
    return [dqkv5, dW if need_dw else torch.empty((0,), dtype=torch.float32, device=qkv5.device)]


def supported(qkv5):
    return qkv5.is_cuda and qkv5.dtype in _IO32 and qkv5.shape[-1] == 64


class KernelizedFn(torch.autograd.Function):
    """out = phi(q) (phi(k)^T v) / clamp(phi(q) . sum phi(k), 1e-2) for every feature map, exact fp32 arithmetic on qkv of any
    I/O type; W [h, m, 64] receives its gradient when `learn`."""

    @staticmethod
    def forward(ctx, qkv5, mask_u8, W, cfg, learn):
        out, p_st, kv, ksum = _ea_op("kernelized_fwd", kernelized_fwd_impl, qkv5, mask_u8, W, list(cfg))
        ctx.save_for_backward(qkv5, mask_u8, W, p_st, kv, ksum)
        ctx.cfg, ctx.learn = cfg, learn
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv5, mask_u8, W, p_st, kv, ksum = ctx.saved_tensors
        need_dw = bool(ctx.learn and ctx.needs_input_grad[2])
        dqkv5, dW = _ea_op("kernelized_bwd", kernelized_bwd_impl, dout, qkv5, mask_u8, W, p_st, kv, ksum, list(ctx.cfg),
                           need_dw)
        return dqkv5, None, (dW.to(W.dtype) if need_dw else None), None, None


def kernelized_attention(qkv5, mask_u8, W, cfg, learn):
    if not supported(qkv5):
        raise RuntimeError("kernelized attention: the HIP kernels take a CUDA qkv of bf16 / fp16 / fp32 with head_dim 64, "
                           "got %s %s" % (qkv5.dtype, tuple(qkv5.shape)))
    return KernelizedFn.apply(qkv5, mask_u8, W, tuple(cfg), bool(learn))


class KernelizedCore(Core):
    """Core spec of _ops.CoreModuleFn: this core on the 16-bit qkv of an autocast step.  With `learn` the feature matrix is
    the node's one differentiable input (W is then passed through `inputs`), else it is fixed state (or None)."""

    def __init__(self, mask_u8, W, cfg, learn):
        self.mask_u8, self.W, self.cfg, self.learn = mask_u8, W, tuple(cfg), bool(learn)

    def _w(self, inputs):
        return inputs[0] if self.learn else self.W

    def fwd(self, qkv5, inputs):
        W = self._w(inputs)
        out, p_st, kv, ksum = kernelized_fwd_impl(qkv5, self.mask_u8, W, self.cfg)
        return out, (p_st, kv, ksum) + ((W,) if self.learn else ())

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        W = saved[3] if self.learn else self.W
        dqkv5, dW = kernelized_bwd_impl(dout, qkv5, self.mask_u8, W, saved[0], saved[1], saved[2], self.cfg, self.learn)
        return dqkv5, ((dW,) if self.learn else ()), (), None
