"""The launch sequence of the exact-fp32 feature cores (csrc/ea_performer_f32.hip, csrc/ea_kernelized.hip).

Both families are linear attention over a feature map with sequence-wide sums that leave the kernels as per-slice partials:

    forward    statistics -> slice partials of KV, ksum -> ea_slice_sum (twice) -> out
    backward   bwd_q (dq, slice partials of d KV, d ksum) -> ea_slice_sum (twice) -> bwd_k (dk, dv)

and differ in their entry names, in whether the query-side calls take the statistic, and in whether partials of dW exist.
A `Family` says so; the geometry struct, the slice count S and the feature count F come from the caller."""
import ctypes

import torch

from . import _native as nv


class Family:
    def __init__(self, prefix, stats, stats_take_q, q_side_stat, has_dw):
        self.stats, self.kv, self.out, self.bwd_q, self.bwd_k = (prefix + s for s in (stats, "kv", "out", "bwd_q", "bwd_k"))
        self.stats_take_q, self.q_side_stat, self.has_dw = stats_take_q, q_side_stat, has_dw


def _views(*qkv5s):
    """ea_t4 references of the q, k, v [B,h,N,d] strided views of each [B,N,3,h,d] tensor"""
    return [ctypes.byref(nv.t4(x[:, :, i].permute(0, 2, 1, 3))) for x in qkv5s for i in range(3)]


def _slice_sums(BH, S, F, d, p_kv, p_ks, stream, f32):
    kv, ksum = torch.empty((BH, F, d), **f32), torch.empty((BH, F), **f32)
    nv.call("ea_slice_sum", BH, S, F * d, 1.0, None, nv.ptr(p_kv), nv.ptr(kv), stream)
    nv.call("ea_slice_sum", BH, S, F, 1.0, None, nv.ptr(p_ks), nv.ptr(ksum), stream)
    return kv, ksum


def forward(fam, geom, S, F, qkv5, mask_u8, W, stat_tail):
    """-> out [B,N,h,d] (dtype of qkv5), the statistic [BH, S, *stat_tail] (stat_tail None: the map has none, [0]),
    kv [BH,F,d], ksum [BH,F]."""
    B, N, _, h, d = qkv5.shape
    BH, f32 = B * h, dict(dtype=torch.float32, device=qkv5.device)
    W = None if W is None else W.float().contiguous()
    w = nv.ptr(W)
    gp, stream = ctypes.byref(geom), nv.stream()
    tq, tk, tv = _views(qkv5)
    if stat_tail is None:
        p_st, st = torch.empty((0,), **f32), None
    else:
        p_st = torch.empty((BH, S) + stat_tail, **f32)
        st = nv.ptr(p_st)
        nv.call(fam.stats, gp, *((tq, tk) if fam.stats_take_q else (tk,)), w, st, stream)
    p_kv, p_ks = torch.empty((BH, S, F, d), **f32), torch.empty((BH, S, F), **f32)
    nv.call(fam.kv, gp, tk, tv, nv.ptr(mask_u8), w, st, nv.ptr(p_kv), nv.ptr(p_ks), stream)
    kv, ksum = _slice_sums(BH, S, F, d, p_kv, p_ks, stream, f32)
    out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=qkv5.device)
    to = ctypes.byref(nv.t4(out.permute(0, 2, 1, 3)))
    nv.call(fam.out, gp, tq, w, *((st,) if fam.q_side_stat else ()), nv.ptr(kv), nv.ptr(ksum), to, stream)
    return out, p_st, kv, ksum


def backward(fam, geom, S, F, dout, qkv5, mask_u8, W, p_st, kv, ksum, need_dw=False):
    """-> dqkv [B,N,3,h,d], dW [h,m,d] fp32 (need_dw) or None."""
    B, N, _, h, d = qkv5.shape
    BH, f32 = B * h, dict(dtype=torch.float32, device=qkv5.device)
    W = None if W is None else W.float().contiguous()
    w = nv.ptr(W)
    gp, stream = ctypes.byref(geom), nv.stream()
    dout = dout.to(qkv5.dtype).contiguous()
    dqkv5 = torch.empty_like(qkv5)
    tq, tk, tv, tdq, tdk, tdv = _views(qkv5, dqkv5)
    tdo = ctypes.byref(nv.t4(dout.permute(0, 2, 1, 3)))
    st = nv.ptr(p_st) if p_st.numel() else None
    p_dw = torch.empty((h, B, 2, S) + tuple(W.shape[1:]), **f32) if need_dw else None
    dw = (nv.ptr(p_dw),) if fam.has_dw else ()
    p_dkv, p_dks = torch.empty((BH, S, F, d), **f32), torch.empty((BH, S, F), **f32)
    nv.call(fam.bwd_q, gp, tq, tdo, w, *((st,) if fam.q_side_stat else ()), nv.ptr(kv), nv.ptr(ksum), tdq, nv.ptr(p_dkv),
            nv.ptr(p_dks), *dw, stream)
    dkv, dksum = _slice_sums(BH, S, F, d, p_dkv, p_dks, stream, f32)
    nv.call(fam.bwd_k, gp, tk, tv, nv.ptr(mask_u8), w, st, nv.ptr(dkv), nv.ptr(dksum), tdk, tdv, *dw, stream)
    dW = None
    if need_dw:
        dW = torch.empty(tuple(W.shape), **f32)
        nv.call("ea_slice_sum", h, B * 2 * S, W.shape[1] * d, 1.0, None, nv.ptr(p_dw), nv.ptr(dW), stream)
    return dqkv5, dW
