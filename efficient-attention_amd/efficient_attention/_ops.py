"""Autograd wrappers around the HIP attention cores (libea_hip.so via _native.py).

One torch.autograd.Function per attention variant; each forward/backward is a short sequence
of HIP kernel launches on the current stream.  q, k and v are never split out of the fused
projection output: the kernels address the [B, N, 3, h, d] tensor produced by `qkv = Linear(x)`
in place through strides, and the backward kernels write dq/dk/dv straight into one
[B, N, 3, h, d] gradient buffer, so none of the reference's permute/contiguous/select-backward
copies exist here.
"""
import collections
import ctypes
import math
import os
import threading
import typing
import warnings

import torch
import torch.nn.functional as F

from . import _feature_cores as _fc
from . import _native as nv

KERNEL_TIMER = nv.KERNEL_TIMER
# algorithmic HBM traffic of one launch, in units of one [B,H,N,D] I/O-dtype tensor
# Eager calls of the cores skip the dispatcher: torch.ops.ea.<name> costs ~15-20 us of host time per call (Python -> C++
# dispatcher -> Python implementation), six of them per layer step.  While a graph is being traced (torch.compile) the
# dispatcher op stays, so the core is one opaque node there (its fake implementation lives in _dispatch.py).
_DIRECT = os.environ.get("EA_DIRECT_IMPL", "1") == "1"


def _ea_op(name, impl, *args):
    # (any active dispatch mode -- fake tensors, make_fx proxies, functionalisation -- means somebody is tracing)
    if _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0:
        return impl(*args)
    return getattr(torch.ops.ea, name)(*args)


def landmark_flops(BH, L, C, D, has_mlp, mixed, eva, bwd):
    """FLOPs executed by one ea_lara_landmarks_fwd/bwd launch (real sizes, 2 per multiply-add): the
    matrix products of ea_lara_landmark.hip.  The backward reloads the forward's saved intermediates
    and only recomputes M = omega mu^T."""
    f = 0
    if not bwd:
        if has_mlp:
            f += 2 * (2 * L * D * D)                  # H = P W^T, both sides
        if not eva and mixed:
            f += 2 * (2 * L * L * D)                  # A = k0 k0^T ; k_bar = A k0
    if not eva:
        f += 2 * C * L * D                            # M = omega mu^T
    if bwd:
        if not eva:
            f += 2 * (2 * L * D * C)                  # dMU, dOM
            if mixed:
                f += 4 * (2 * L * L * D)              # dK0 = A^T dKb, dA, dK0 += dG K0, += dG^T K0
        if has_mlp:
            f += 2 * (2 * L * D * D) + 2 * (2 * D * D * L)   # dP = dH W, dW = dH^T P, both sides
    return BH * f


def landmark_bytes(BH, L, C, D, has_mlp, mixed, eva, bwd):
    """Algorithmic HBM bytes of one ea_lara_landmarks_fwd/bwd launch: the [B*h, L|C, D] fp32 tensors it
    must read and write (the pipeline itself lives in LDS; parameters and per-landmark scalars are
    negligible).  The kernel is latency-bound -- these are the bytes its roofline is priced on."""
    row = D * 4
    saved = (3 * L * D + 64 * L + 128) * 4
    if not bwd:
        per = 2 * L * row + C * row + 2 * C * row + saved           # pq, pk, noise -> omega, qbar_rows, saved
    else:
        per = saved + C * row + 2 * C * row + 2 * L * row            # saved, noise, d_omega, d_qbar_rows, pq/pk
        per += 2 * L * row                                           # -> dpq, dpk
        if has_mlp:
            per += 2 * D * D * 4 + 6 * D * 4                         # -> dW_part, dvec_part
    return BH * per


LAST_LMK_GEOM = None      # (BH, L, C, D, has_mlp, mixed, eva) of the most recent landmark launch (bench.py)

KERNEL_ALGO_UNITS = {
    "ea_window_attn_fwd": 4,      # read q,k,v; write out
    "ea_window_attn_bwd": 8,      # read q,k,v,out,dout; write dq,dk,dv
    "ea_eva_chunk_mean_fwd": 2,   # read q,k
    "ea_eva_chunk_mean_bwd": 4,   # read+write dq,dk
    "ea_eva_beta_fwd": 2,         # read k,v
    "ea_eva_beta_bwd": 6,         # read k,v; read+write dk,dv
    "ea_softmax_attn_fwd": 4,     # read q,k,v; write out
    "ea_softmax_attn_bwd": 8,     # read q,k,v,out,dout; write dq,dk,dv (two passes)
    "ea_performer_kmax": 1,       # read k
    "ea_performer_kv": 2,         # read k,v
    "ea_performer_out": 2,        # read q; write out
    "ea_performer_bwd_q": 4,      # read q,out,dout; write dq
    "ea_performer_bwd_qstats": 2, # read q,dout
    "ea_performer_bwd_k": 4,      # read k,v; write dk,dv
    "ea_performer_f32_kmax": 1,   # read k
    "ea_performer_f32_kv": 2,     # read k,v
    "ea_performer_f32_out": 2,    # read q; write out
    "ea_performer_f32_bwd_q": 3,  # read q,dout; write dq
    "ea_performer_f32_bwd_k": 4,  # read k,v; write dk,dv
    "ea_kernelized_stats": 1,     # read k (fourier: q,k -- counted as one: favorp, the common case, reads k only)
    "ea_kernelized_kv": 2,        # read k,v
    "ea_kernelized_out": 2,       # read q; write out
    "ea_kernelized_bwd_q": 3,     # read q,dout; write dq
    "ea_kernelized_bwd_k": 4,     # read k,v; write dk,dv
    "ea_lara_stats_fwd": 3,       # read q,k,v
    "ea_lara_out_fwd": 2,         # read q; write out
    "ea_lara_out_proj_fwd": 2,    # read q; write out (+ y = out W_proj^T + bias, priced under LABEL_ALGO_BYTES)
    "ea_lara_bwd_q": 3,           # read q,dout; write dq
    "ea_lara_bwd_qstats": 2,      # read q,dout
    "ea_lara_bwd_k": 4,           # read k,v; write dk,dv
    "ea_lara_bwd_kstats": 2,      # read k,v
    "ea_lara_bwd_qcorr": 3,       # read q; read+write dq
    "ea_lara_bwd_q_fused": 3,     # read q,dout; write dq
    "ea_lara_bwd_k_fused": 4,     # read k,v; write dk,dv
    "ea_lara_bwd_finish": 5,      # read q; read+write dq,dk
}


def _qkv_views(qkv5):
    """[B,N,S>=3,h,d] -> the q, k, v [B,h,N,d] strided views (no copy); further slots (the pre-LayerNorm
    rows of LARA's 1-D proposals) are left alone."""
    return tuple(qkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def _mask_u8(mask, B, N, device):
    if mask is None:
        return None
    m = mask.to(device=device, dtype=torch.uint8).reshape(B, N).contiguous()
    return m


_LOG2E = 1.4426950408889634

class DerivedCache:
    """Derived weights (concatenations / products of parameters) re-used across calls of an EVALUATION-mode
    module: never while the owner is training, autograd is on (a cached tensor carries no graph) or a
    hipGraph is being captured (a capture must record the producing kernels, or its replays would see
    stale values after an in-graph optimizer step).  `_version` is not a change detector -- optimizers
    that update through `.data` (fairseq's Adam / FP16 optimizers, `p.data.copy_()`) never bump it -- so
    the owner drops the cache on every `train()` call and on `load_state_dict` (`DerivedCacheOwner`);
    the key (identity, storage pointer, `_version`, device, dtype of every source) only catches
    re-assigned parameters on top of that."""

    def __init__(self):
        self.key, self.value = None, None

    def invalidate(self):
        self.key, self.value = None, None

    def get(self, owner, sources, build):
        if (owner.training or torch.is_grad_enabled()
                or (sources[0].is_cuda and torch.cuda.is_current_stream_capturing())):
            self.invalidate()
            return build()
        key = tuple((id(t), t.data_ptr(), t._version, t.device, t.dtype) for t in sources if t is not None)
        if key != self.key:
            self.key, self.value = key, build()
        return self.value


class DerivedCacheOwner:
    """Mixin for modules holding DerivedCache attributes: every mode switch and every state-dict load
    drops them (an optimizer step between two validation passes always sits between two `train()` calls)."""

    def _drop_derived(self):
        for v in list(vars(self).values()):
            if isinstance(v, DerivedCache):
                v.invalidate()

    def train(self, mode=True):
        self._drop_derived()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self._drop_derived()
        return super()._load_from_state_dict(*args, **kwargs)

    def invalidate_derived_weights(self):
        """Call after writing parameters in place (through `.data`) while the module stays in eval mode."""
        self._drop_derived()


_FP32_WARNED = [False]


def to_io_dtype(t):
    """Tensor entering an attention core -> the kernels' I/O dtype (bf16 / fp16 operands, fp32
    accumulation and softmax).  Under autocast the projection already emits it.  An fp32 tensor
    outside autocast is where this build departs from the reference, which computes attention in
    fp32 there (abstract_attention.py:120-133): it is rounded to bf16 and the caller is told once
    (EA_STRICT_FP32=1 turns the warning into an error)."""
    if t.dtype in (torch.bfloat16, torch.float16):
        return t
    warn_fp32_rounded(t.dtype, stacklevel=4)
    return t.to(torch.bfloat16)


def warn_fp32_rounded(dtype, stacklevel=3):
    """The one-time notice of to_io_dtype (EA_STRICT_FP32=1: the error), for a caller that rounds fp32 activations inside its
    own kernel (the held projections of a decoding state)."""
    if os.environ.get("EA_STRICT_FP32", "0") == "1":
        raise RuntimeError("efficient_attention (MI355X build): %s activations reached an attention core outside "
                           "torch.autocast; the HIP cores take bf16/fp16 operands (EA_STRICT_FP32=1)" % dtype)
    if not _FP32_WARNED[0]:
        _FP32_WARNED[0] = True
        warnings.warn("efficient_attention (MI355X build): %s activations outside torch.autocast are rounded to "
                      "bf16 for the attention cores (bf16 operands, fp32 accumulation / softmax); the reference "
                      "computes fp32 here. Wrap the call in torch.autocast('cuda', dtype=torch.bfloat16 | "
                      "torch.float16) to choose the operand type explicitly." % dtype, stacklevel=stacklevel)


USE_TABLE_BIAS = os.environ.get("EA_TABLE_BIAS", "1") == "1"
TABLE_BIAS_SPLIT = os.environ.get("EA_TABLE_BIAS_SPLIT", "1") == "1"      # dev switch: long position lists in pieces
BIAS_HEAD_SUM = os.environ.get("EA_BIAS_HEAD_SUM", "1") == "1"            # dev switch: heads of a one-column table added by the colsum
class _Hint(threading.local):
    """(per thread: autograd runs a device's backward on its own thread)"""
    on = False


_BIAS_HEAD_SUM = _Hint()                                                   # set by EvaAttnFn.backward around its (direct) call


class TableBias:
    """A dense window bias that is a table read through a fixed index (round 6):
        bias[hd, i, j] = scale * table[idx[i, j], hd]
    -- `relative_position_bias_table[relative_position_index]` of the 2-D windows (local_attention.py:70-79) and the bucketed T5
    bias (eva.py:53-65).  dense() builds it in the layout and units the window kernels stage ([h, Wq, ld] fp32, log2 units) in
    ONE launch (ea_table_bias_fwd) and grad() takes the kernels' bias gradient back to the table in one (ea_table_bias_bwd):
    the framework spent an index_select, a permute copy, a scalar multiply, a pad (fill + copy) and, in the backward, a slice
    copy and the transposed chain on it -- six to eight launches of ~4 us in every EVA / local-window step.
    The single-node module paths (CoreModuleFn around an EvaCore or a LocalCore) take the TABLE as their differentiable input
    together with this spec; every other path keeps the dense [h, Wq, Wk] bias."""

    def __init__(self, idx, rows, Wq, Wk, scale, inv=None):
        flat = idx.detach().reshape(-1).cpu().long()
        if flat.numel() != Wq * Wk:
            raise ValueError("TableBias: the index does not cover [Wq, Wk]")
        self.rows, self.Wq, self.Wk, self.scale = int(rows), int(Wq), int(Wk), float(scale)
        self._idx = flat.to(torch.int32)
        self._inv = inv.detach().cpu().to(torch.int32) if inv is not None else None
        self._dev = {}
        self._ld = {}
        self._parts = 1

    def _on(self, device):
        hit = self._dev.get(device)
        if hit is None:
            if self._inv is None:
                from .local_attention import _inverse_index
                self._inv = _inverse_index(self._idx.long(), self.rows)
            inv = self._inv.contiguous()
            # a far T5 bucket of a causal 128 x 128 window holds ~8 k positions and ea_table_bias_bwd gives a (row, head) ONE
            # 256-lane workgroup: the longest list is the launch (26.7 us in the LM step).  Lists longer than 1024 are cut into
            # P pieces -- the kernel sees rows * P shorter rows, grad() adds the P partial cells in a fixed order
            K = inv.shape[1]
            P = max(1, min(16, K // 512)) if TABLE_BIAS_SPLIT else 1
            if P > 1:
                K2 = -(-K // P) * P
                if K2 != K:
                    inv = F.pad(inv, (0, K2 - K), value=-1)
                inv = inv.view(self.rows * P, K2 // P).contiguous()
            self._parts = P
            hit = (self._idx.to(device), inv.to(device))
            self._dev[device] = hit
        return hit

    def ld(self, B, h, N, d, io, attn_2d, seq_shape, window, ext, chunk=0, L=0, causal=0):
        key = (B, h, N, d, io, bool(attn_2d), tuple(seq_shape), window, ext, chunk, L, causal)
        v = self._ld.get(key)
        if v is None:
            geom = nv.make_geom(B, h, N, d, io, bool(attn_2d), tuple(seq_shape), window, ext, chunk, L, causal)
            v = int(nv.query("ea_window_bias_ld", geom))
            if len(self._ld) < 64:
                self._ld[key] = v
        return v

    def dense(self, table, ld, heads=None):
        """-> [h, Wq, ld] fp32, already in the kernels' log2 units and padded (marked `_ea_ready`: _bias_padded hands it on).
        heads: a one-column table (causal EVA's single-head T5 table) is broadcast over that many heads."""
        idx, _ = self._on(table.device)
        t32 = _f32c(table)
        th = t32.shape[1]
        h = th if heads is None else int(heads)
        if th != h and th != 1:
            raise ValueError("TableBias: a table of %d columns for %d heads" % (th, h))
        out = torch.empty((h, self.Wq, ld), dtype=torch.float32, device=table.device)
        nv.call("ea_table_bias_fwd", h, th, self.Wq, self.Wk, ld, self.scale * _LOG2E, nv.ptr(t32), nv.ptr(idx), nv.ptr(out),
                nv.stream())
        out._ea_ready = True
        return out

    def grad(self, g, table_heads=None):
        """g [h, Wq, ld] fp32 = d loss / d (natural-unit bias) as the window backward returns it -> d table [rows, th] fp32
        (th = table_heads or h; th = 1: summed over the heads)."""
        _, inv = self._on(g.device)
        g = _f32c(g)
        h, Wq, ld = g.shape                    # (h = 1: the heads of a one-column table were added up on the way here)
        P = self._parts
        out = torch.empty((self.rows * P, h), dtype=torch.float32, device=g.device)
        nv.call("ea_table_bias_bwd", self.rows * P, inv.shape[1], h, Wq, self.Wk, ld, self.scale, nv.ptr(g), nv.ptr(inv),
                nv.ptr(out), nv.stream())
        one_col = table_heads is not None and int(table_heads) == 1 and h != 1
        if P > 1 and one_col:
            return out.view(self.rows, P * h).sum(1, keepdim=True)
        if P > 1:
            out = out.view(self.rows, P, h).sum(1)
        if one_col:
            out = out.sum(1, keepdim=True)
        return out


def _bias_padded(bias, geom):
    """[h, Wq, Wk] fp32 -> rows padded to the kernel's leading dimension, pre-multiplied by
    log2(e): the kernels evaluate the softmax in the log2 domain (the bias GRADIENT they return is
    with respect to the natural-unit bias)."""
    if bias is None:
        return None
    if getattr(bias, "_ea_ready", False):       # TableBias.dense(): padded and in log2 units already
        return bias
    ld = nv.query("ea_window_bias_ld", geom)
    b = bias.float() * _LOG2E
    if b.shape[-1] != ld:
        b = F.pad(b, (0, ld - b.shape[-1]))
    return b.contiguous()


def _window_fwd(geom, qkv5, lk, lv, bias_p, mask_u8, keep=None, keep_scale=1.0):
    B, N, _, h, d = qkv5.shape
    q, k, v = _qkv_views(qkv5)
    if qkv5.stride(1) > qkv5.stride(0):
        # time-first qkv (a transposed view of [N,B,3,h,d], fairseq's layout): out follows it
        out = torch.empty((N, B, h, d), dtype=qkv5.dtype, device=qkv5.device).transpose(0, 1)
    else:
        out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=qkv5.device)
    lse = torch.empty((B, h, N), dtype=torch.float32, device=qkv5.device)
    tq, tk, tv, to = nv.t4(q), nv.t4(k), nv.t4(v), nv.t4(out.permute(0, 2, 1, 3))
    nv.call("ea_window_attn_fwd", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk),
            ctypes.byref(tv), nv.ptr(lk), nv.ptr(lv), nv.ptr(bias_p), nv.ptr(mask_u8),
            ctypes.byref(to), nv.ptr(lse), nv.ptr(keep), float(keep_scale), nv.stream())
    return out, lse


def _rows_contiguous(t):
    """A [B,N,h,d] tensor the kernels can address through strides (rows of d contiguous, heads packed)
    as it is -- e.g. a batch-first view of a time-first buffer -- or a contiguous copy."""
    if t.stride(-1) == 1 and t.stride(-2) == t.shape[-1] and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0:
        return t
    return t.contiguous()


def _window_bwd(geom, qkv5, lk, lv, bias_p, mask_u8, out, dout, lse, dqkv5, keep=None, keep_scale=1.0, dlse=None):
    """out, dout: [B,N,h,d] with contiguous rows.  Writes dq,dk,dv into dqkv5; returns dlk, dlv, dbias_padded."""
    B, N, _, h, d = qkv5.shape
    q, k, v = _qkv_views(qkv5)
    dq, dk, dv = _qkv_views(dqkv5)
    parts = nv.query("ea_window_bwd_parts", geom)
    L = geom.L
    dev = qkv5.device
    dlk_p = dlv_p = dbias_p = None
    if L > 0:
        # both landmark-gradient partial sets in one buffer [2, parts, B*h*L*d]: ONE slice reduction below
        dl_p = torch.empty((2, parts, B * h, L, d), dtype=torch.float32, device=dev)
        dlk_p, dlv_p = dl_p[0], dl_p[1]
    if bias_p is not None:
        # several query blocks per window: each launch writes only its block's rows
        alloc = torch.zeros if nv.query("ea_window_bwd_query_blocks", geom) > 1 else torch.empty
        bparts = nv.query("ea_window_bwd_bias_parts", geom)
        dbias_p = alloc((bparts, B) + tuple(bias_p.shape), dtype=torch.float32, device=dev)
    dk_acc = dv_acc = None
    slices = nv.query("ea_window_bwd_acc_slices", geom)
    if slices:
        dk_acc = torch.empty((slices, B, h, N, d), dtype=torch.float32, device=dev)
        dv_acc = torch.empty_like(dk_acc)
    bias_t = None
    if bias_p is not None and nv.query("ea_window_bwd_needs_bias_t", geom):
        wq_pad = -(-bias_p.shape[1] // 16) * 16
        bias_t = F.pad(bias_p.transpose(1, 2), (0, wq_pad - bias_p.shape[1])).contiguous()   # [h, ld, WqPad]
    ts = [nv.t4(t) for t in (q, k, v, out.permute(0, 2, 1, 3), dout.permute(0, 2, 1, 3), dq, dk, dv)]
    nv.call("ea_window_attn_bwd", ctypes.byref(geom), ctypes.byref(ts[0]), ctypes.byref(ts[1]),
            ctypes.byref(ts[2]), nv.ptr(lk), nv.ptr(lv), nv.ptr(bias_p), nv.ptr(mask_u8),
            ctypes.byref(ts[3]), ctypes.byref(ts[4]), nv.ptr(lse), ctypes.byref(ts[5]),
            ctypes.byref(ts[6]), ctypes.byref(ts[7]), nv.ptr(dlk_p), nv.ptr(dlv_p), nv.ptr(dbias_p),
            nv.ptr(dk_acc), nv.ptr(dv_acc), nv.ptr(bias_t), nv.ptr(keep), float(keep_scale), nv.ptr(dlse),
            nv.stream())
    dlk = dlv = dbias = None
    if L > 0:
        # per-workgroup partials [parts, B*h*L*d] -> one pass each (fixed summation order)
        dl = torch.empty((2, B, h, L, d), dtype=torch.float32, device=dev)
        n = B * h * L * d
        nv.call("ea_slice_sum", 2, parts, n, 1.0, None, nv.ptr(dl_p), nv.ptr(dl), nv.stream())
        dlk, dlv = dl[0], dl[1]
    if bias_p is not None:
        if _BIAS_HEAD_SUM.on and bias_p.shape[0] > 1:
            # the bias is a one-column table broadcast over the heads (causal EVA's T5 table): its gradient wants the SUM over
            # the heads, so the heads join the rows of this reduction -- [parts * B * h, Wq * ld] instead of [parts * B, h * Wq * ld]
            # (LM step: 144 rows x 24 k columns instead of 18 x 197 k: 21.9 -> ~9 us) and the table kernel sees one head
            dbias = colsum_f32(dbias_p.view(dbias_p.shape[0] * B * bias_p.shape[0], -1)).view((1,) + tuple(bias_p.shape[1:]))
        else:
            dbias = colsum_f32(dbias_p.view(dbias_p.shape[0] * B, -1)).view(bias_p.shape)
    return dlk, dlv, dbias


# ------------------------------------------------------------------------------------------
# local window attention  (reference local_attention.py:134-182)
# ------------------------------------------------------------------------------------------
def _f32c(t):
    """A parameter as the kernels read it (fp32, contiguous: only its data pointer is taken).  fp32 master parameters -- the
    normal case -- pass through untouched: detach() + float() + contiguous() were three dispatcher calls per parameter, 48 per
    eager step of a layer with two landmark networks."""
    if t.dtype is torch.float32 and t.is_contiguous():
        return t
    return t.detach().float().contiguous()


def _opt(t):
    """Dispatcher ops carry `None` tensors of a Tensor[] as empty tensors."""
    return None if (t is None or t.numel() == 0) else t


def _e(t, like):
    return like.new_empty(0) if t is None else t


def _local_geom(qkv5, geo):
    """geo = [attn_2d, s0, s1, window, ext] of the local ops (_geo) -> ea_geom."""
    B, N, _, h, d = qkv5.shape
    attn_2d, s0, s1, window, ext = [int(v) for v in geo]
    return nv.make_geom(B, h, N, d, nv.io_dtype(qkv5), bool(attn_2d), (s0, s1) if attn_2d else (s0,), window, ext, 0, 0)


def local_fwd_impl(qkv5, bias, mask_u8, geo):
    """torch.ops.ea.local_fwd: geo = [attn_2d, s0, s1, window, ext] -> [out, lse, bias_padded | empty]."""
    nv.require_cuda(qkv5, "qkv")
    geom = _local_geom(qkv5, geo)
    bias_p = _bias_padded(bias, geom)
    out, lse = _window_fwd(geom, qkv5, None, None, bias_p, mask_u8)
    return [out, lse, _e(bias_p, lse)]


def local_bwd_impl(dout, dlse, qkv5, bias_p, mask_u8, out, lse, geo, bias_cols):
    """torch.ops.ea.local_bwd -> [dqkv, dbias | empty]."""
    geom = _local_geom(qkv5, geo)
    dqkv5 = torch.empty_like(qkv5)
    _, _, dbias = _window_bwd(geom, qkv5, None, None, bias_p, mask_u8, out, dout.contiguous(), lse, dqkv5,
                              dlse=None if dlse is None else dlse.float().contiguous())
    if dbias is not None:
        dbias = dbias[..., :bias_cols].contiguous()
    return [dqkv5, _e(dbias, lse)]


def _geo(attn_2d, seq_shape, window, ext):
    seq_shape = tuple(int(v) for v in seq_shape)
    return [1 if attn_2d else 0, seq_shape[0], seq_shape[1] if len(seq_shape) > 1 else 0, int(window), int(ext)]


class LocalAttnFn(torch.autograd.Function):
    """out[B,N,h,d] = per-window softmax(s QK^T + bias, -5e4 mask) V on a fused qkv tensor
    (torch.ops.ea.local_fwd / local_bwd)."""

    @staticmethod
    def forward(ctx, qkv5, bias, mask_u8, attn_2d, seq_shape, window, ext):
        geo = _geo(attn_2d, seq_shape, window, ext)
        out, lse, bias_p = _ea_op("local_fwd", local_fwd_impl, qkv5, bias, mask_u8, geo)
        ctx.save_for_backward(qkv5, _opt(bias_p), mask_u8, lse, out)
        ctx.geo = geo
        ctx.bias_cols = 0 if bias is None else bias.shape[-1]
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv5, bias_p, mask_u8, lse, out = ctx.saved_tensors
        dqkv5, dbias = _ea_op("local_bwd", local_bwd_impl, dout, None, qkv5, bias_p, mask_u8, out, lse, ctx.geo, ctx.bias_cols)
        return dqkv5, _opt(dbias), None, None, None, None, None


class LocalAttnLseFn(torch.autograd.Function):
    """LocalAttnFn that also returns the per-query log-sum-exp [B,h,N] (natural log) as a
    differentiable output, for callers that merge further softmax columns with the window's."""

    @staticmethod
    def forward(ctx, qkv5, bias, mask_u8, attn_2d, seq_shape, window, ext):
        geo = _geo(attn_2d, seq_shape, window, ext)
        out, lse, bias_p = _ea_op("local_fwd", local_fwd_impl, qkv5, bias, mask_u8, geo)
        ctx.save_for_backward(qkv5, _opt(bias_p), mask_u8, lse, out)
        ctx.geo = geo
        ctx.bias_cols = 0 if bias is None else bias.shape[-1]
        return out, lse.clone()

    @staticmethod
    def backward(ctx, dout, dlse):
        qkv5, bias_p, mask_u8, lse, out = ctx.saved_tensors
        dqkv5, dbias = _ea_op("local_bwd", local_bwd_impl, dout, dlse, qkv5, bias_p, mask_u8, out, lse, ctx.geo, ctx.bias_cols)
        return dqkv5, _opt(dbias), None, None, None, None, None


def _mlp_grads(dW, dvec, d):
    """The two d x d matrices and the 2 x 3 vectors of the landmark / mu networks' gradient, [2 d d] and [6 d] floats as the
    kernels (or the sums over their per-(b,h) partials) leave them -> the eight gradients in parameter order: W, b, gamma,
    beta of the q side, then of the k side."""
    dWs, dvs = dW.view(2, d, d), dvec.view(2, 3, d)
    return [dWs[0], dvs[0, 0], dvs[0, 1], dvs[0, 2], dWs[1], dvs[1, 0], dvs[1, 1], dvs[1, 2]]


# ------------------------------------------------------------------------------------------
# EVA  (reference eva.py:145-227)
# ------------------------------------------------------------------------------------------
class EvaCfg(typing.NamedTuple):
    """The EVA core's configuration (plain values, hashable).  causal / mu_scale select causal_eva.py's geometry, masks
    (ea_geom.causal) and its mu = rq + rk; keep_scale = 1 / (1 - p) scales the attention dropout's keep mask (EvaExtras.keep).
    lists() / from_lists() are the ONE encoder and decoder of the int[] / float[] arguments of torch.ops.ea.eva_fwd / eva_bwd:
    icfg = [attn_2d, s0, s1 | 0, window, ext, chunk, L, causal(, keep_for_backward = 1)], fcfg = [mu_scale, keep_scale]."""
    attn_2d: bool
    seq_shape: tuple
    window: int
    ext: int
    chunk: int
    L: int
    adaptive_proj: str
    causal: int = 0
    mu_scale: float = 0.5
    keep_scale: float = 1.0

    def lists(self, need_grad):
        return (_geo(self.attn_2d, self.seq_shape, self.window, self.ext)
                + [int(self.chunk), int(self.L), int(self.causal), int(bool(need_grad))],
                [float(self.mu_scale), float(self.keep_scale)])

    @classmethod
    def from_lists(cls, icfg, fcfg, adaptive_proj):
        """-> (cfg, need_grad); an absent trailing entry means keep for backward."""
        attn_2d, s0, s1, window, ext, chunk, L, causal, *keep = [int(v) for v in icfg]
        mu_scale, keep_scale = [float(v) for v in fcfg]
        cfg = cls(bool(attn_2d), (s0, s1) if attn_2d else (s0,), window, ext, chunk, L, adaptive_proj, causal, mu_scale, keep_scale)
        return cfg, not keep or bool(keep[0])


# what an EVA call may carry besides its EvaCfg: the uint8 keep mask of the attention dropout (causal_eva only), a TableBias
# -- `bias` is then the TABLE ([rows, h] or [rows, 1]); direct calls only --, the Pooled chunk means a projection kernel wrote
EvaExtras = collections.namedtuple("EvaExtras", "keep table_bias pooled", defaults=(None, None, None))


def _eva_cfg(qkv5, cfg):
    """-> (ea_geom, whether the fused mu networks -- Linear + LayerNorm + mu + omega in one kernel -- apply)."""
    B, N, _, h, d = qkv5.shape
    geom = nv.make_geom(B, h, N, d, nv.io_dtype(qkv5), cfg.attn_2d, cfg.seq_shape, cfg.window, cfg.ext, cfg.chunk, cfg.L, cfg.causal)
    return geom, _eva_fused_mu(cfg, d)


def _eva_fused_mu(cfg, d):
    return cfg.adaptive_proj == "default" and cfg.L <= 64 and d in (32, 64) and cfg.mu_scale == 0.5


def _eva_use_composite():
    """The FORWARD's decision between ea_eva_layer_fwd and the step-by-step launches (bench.py's per-kernel timing needs the
    individual entry points); the backward follows what the forward saved (see _lara_use_composite)."""
    return os.environ.get("EA_EVA_COMPOSITE", "1") == "1" and not nv.KERNEL_TIMER.enabled


_EVA_LAYER_CFG = {}


def _eva_layer_cfg_dims(B, h, d, io, cfg, has_bias, masked):
    """(ea_eva_layer, ea_eva_layer_sizes: the workspace plan, read by field name) of the composite entry points, or
    (None, None): 2-D non-overlapping windows, no pad mask / dropout, the fused mu networks.  Memoised per geometry."""
    chunk = cfg.chunk
    if (not cfg.attn_2d or cfg.ext != 0 or cfg.causal != 0 or masked or cfg.adaptive_proj != "default" or cfg.mu_scale != 0.5
            or cfg.keep_scale != 1.0 or chunk <= 0):
        return None, None
    s0, s1 = cfg.seq_shape
    if s0 % chunk or s1 % chunk or (s0 // chunk) * (s1 // chunk) != cfg.L:
        return None, None
    key = (B, h, d, io, s0, s1, cfg.window, chunk, int(has_bias))
    hit = _EVA_LAYER_CFG.get(key)
    if hit is None:
        lcfg = nv.ea_eva_layer(B, h, d, io, s0, s1, cfg.window, chunk, int(has_bias), float(d) ** -0.5)
        sizes = nv.ea_eva_layer_sizes()
        hit = (lcfg, sizes) if nv.lib().ea_eva_layer_plan(ctypes.byref(lcfg), ctypes.byref(sizes)) == 0 else (None, None)
        if len(_EVA_LAYER_CFG) < 256:
            _EVA_LAYER_CFG[key] = hit
    return hit


# pooled q / k rows [BH, L, d] (fp32) a projection kernel wrote (_pooled_rows): inside the fresh `saved` workspace `ws` of a
# composite entry, or as two tensors for the step-by-step launches -- exactly one of ws and the pq / pk pair is set
Pooled = collections.namedtuple("Pooled", "ws pq pk")
# of _lara_backward / _eva_backward.  params: the summed parameter gradients (fp32, parameter order), None when deferred; partials:
# (key, tensor [S, n], meta) entries for the caller's terminal sum; finish: the operands of qkv_dgrad_finish (a Finish) or None
CoreGrads = collections.namedtuple("CoreGrads", "dqkv dbias params partials finish")
# the operands of qkv_dgrad_finish: the r x r cells of a gh x gw grid, C samples; dpq / dpk [BH, L, d] the gradients of the pooled
# rows (EVA: of the chunk means); uq, qbar [BH, C, d] and lse_t [BH, C] only for LARA's softmax-over-sequence correction
Finish = collections.namedtuple("Finish", "B gh gw r C scale dpq dpk uq qbar lse_t", defaults=(None, None, None))


def _ws_rows(ws, at, rows, cols=None):
    """rows [x cols] floats of a composite workspace from offset `at` (a field of its plan)."""
    return ws[at:at + rows] if cols is None else ws[at:at + rows * cols].view(rows, cols)


def _param_partials(dW, dvec):
    """The landmark / mu networks' per-(b,h) gradient partials W [BH, 2 d d], v [BH, 6 d] -> entries for the terminal sum."""
    return [("mlp_W", dW, None), ("mlp_v", dvec, None)]


def _eva_saved_is_composite(saved_list):
    """TWO tensors after `out` = eva_fwd_impl (just below) ran ea_eva_layer_fwd: the count crosses save_for_backward and the dispatcher."""
    return len(saved_list) == 2


def eva_fwd_impl(qkv5, bias, noise, mask_u8, keep, icfg, fcfg, adaptive_proj, mlp_params, pooled=None, composite=False):
    """torch.ops.ea.eva_fwd: chunk means -> mu MLP -> omega -> beta -> window attention with control-variate
    columns (eva.py:145-227).  icfg, fcfg, adaptive_proj: an EvaCfg and the keep-for-backward flag as EvaCfg.lists() encodes
    them.  -> [out, bias_padded, lse, qmean, kmean, omega, beta, rf_k_bar, lmk_saved, zhat, rstd] (absent tensors are empty).
    composite (direct calls only, never through the dispatcher): ONE C-ABI call (ea_eva_layer_fwd) on a caller-owned
    workspace where the geometry allows it -> [out, bias_padded, saved workspace]; pooled (direct calls only): a Pooled --
    the chunk means the projection kernel already wrote, into that workspace or as two tensors -- or None."""
    global LAST_LMK_GEOM
    nv.require_cuda(qkv5, "qkv")
    cfg, need_grad = EvaCfg.from_lists(icfg, fcfg, adaptive_proj)
    B, N, _, h, d = qkv5.shape
    dev = qkv5.device
    lcfg, sizes = _eva_layer_cfg_dims(B, h, d, nv.io_dtype(qkv5), cfg, bias is not None,
                                      mask_u8 is not None or keep is not None) if composite else (None, None)
    if pooled is not None and (pooled.ws is not None) != (lcfg is not None):
        raise RuntimeError("eva_fwd: chunk means prepared for the other launch path")
    geom, fused_mu = _eva_cfg(qkv5, cfg)
    L, mu_scale = cfg.L, cfg.mu_scale
    q, k, v = _qkv_views(qkv5)
    tq, tk, tv = nv.t4(q), nv.t4(k), nv.t4(v)
    if lcfg is not None:
        ws = pooled.ws if pooled is not None else torch.empty(sizes.n_saved, dtype=torch.float32, device=dev)
        out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=dev)
        to = nv.t4(out.permute(0, 2, 1, 3))
        bias_p = _bias_padded(bias, geom)
        noise_c = None if noise is None else noise.float().contiguous()
        ps = [_f32c(p) for p in mlp_params]
        LAST_LMK_GEOM = (B * h, L, L, d, 1, 0, 1)
        nv.call("ea_eva_layer_fwd", ctypes.byref(lcfg), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv),
                nv.ptr(bias_p), nv.ptr(noise_c), _param_ptrs(ps), ctypes.byref(to), nv.ptr(ws),
                int(need_grad) | (2 if pooled is not None else 0), nv.stream())
        return [out, _e(bias_p, ws), ws]                  # composite: _eva_saved_is_composite
    if pooled is not None:
        # (direct calls only) the chunk means came out of the projection kernel (ea_linear_w32_pool, LinearPoolFn)
        qmean, kmean = pooled.pq.view(B, h, L, d), pooled.pk.view(B, h, L, d)
    else:
        qmean = torch.empty((B, h, L, d), dtype=torch.float32, device=dev)
        kmean = torch.empty_like(qmean)
        nv.call("ea_eva_chunk_mean_fwd", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk),
                nv.ptr(mask_u8), nv.ptr(qmean), nv.ptr(kmean), nv.stream())
    ps = [_f32c(p) for p in mlp_params]
    noise_c = saved = zhat = rstd = None
    if fused_mu:
        # Linear + LayerNorm + mu + omega in one HIP kernel (ea_lara_landmarks_fwd, eva mode)
        lg = nv.ea_lmk_geom(B * h, L, L, d, 1, 0, 0, 0, float(d) ** -0.5, 1)
        LAST_LMK_GEOM = (B * h, L, L, d, 1, 0, 1)
        noise_c = None if noise is None else noise.float().contiguous()
        omega = torch.empty_like(qmean)
        rf_k_bar = torch.empty_like(qmean)
        saved = _lmk_saved(lg, dev) if need_grad else None
        nv.call("ea_lara_landmarks_fwd", ctypes.byref(lg), nv.ptr(qmean), nv.ptr(kmean),
                *[nv.ptr(t) for t in ps], nv.ptr(noise_c), nv.ptr(omega), nv.ptr(rf_k_bar), None, None,
                nv.ptr(saved), nv.stream())
    else:
        # Linear (+ LayerNorm) of both sides in one exact-fp32 HIP pass (ea_rows_mlp_fwd)
        sides = 1 if cfg.adaptive_proj == "none" else 2
        ln = cfg.adaptive_proj != "no-ln"
        per = 4 if ln else 2
        side_p = [ps[i * per:(i + 1) * per] for i in range(sides)]          # (W, b[, gamma, beta]) per side
        xs = [qmean, kmean] if sides == 2 else [kmean]
        ys = [torch.empty_like(kmean) for _ in range(sides)]
        R = B * h * L
        if ln and need_grad:
            zhat = torch.empty((sides, R, d), dtype=torch.float32, device=dev)
            rstd = torch.empty((sides, R), dtype=torch.float32, device=dev)

        def pick(i):                                                      # i-th tensor of each side
            col = [sp[i] if i < len(sp) else None for sp in side_p] + [None]
            return [nv.ptr(col[0]), nv.ptr(col[1])]
        nv.call("ea_rows_mlp_fwd", R, d, sides, 1 if ln else 0,
                nv.ptr(xs[0]), nv.ptr(xs[1] if sides == 2 else None), *pick(0), *pick(1), *pick(2), *pick(3),
                nv.ptr(ys[0]), nv.ptr(ys[1] if sides == 2 else None), nv.ptr(zhat), nv.ptr(rstd), nv.stream())
        rf_k_bar = ys[-1]
        # omega = mu_scale (rq + rk) [+ noise] in two launches (one without noise at mu_scale = 1): the scale rides on the second
        # addition's alpha -- exact for the two scales in use (1: causal EVA, 0.5: a power of two, so the fused multiply-add
        # rounds once at the same place as multiply-then-add)
        if sides == 2:
            s_ = torch.add(ys[0], ys[1])
            if noise is not None:
                omega = torch.add(noise.float(), s_, alpha=mu_scale)
            else:
                omega = s_ if mu_scale == 1.0 else s_.mul_(mu_scale)
        else:
            omega = torch.zeros_like(rf_k_bar) if noise is None else noise.float().clone()
        omega = omega.contiguous()
    beta = torch.empty_like(qmean)
    nv.call("ea_eva_beta_fwd", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv),
            nv.ptr(mask_u8), nv.ptr(omega), nv.ptr(beta), nv.stream())
    bias_p = _bias_padded(bias, geom)
    out, lse = _window_fwd(geom, qkv5, rf_k_bar, beta, bias_p, mask_u8, keep, cfg.keep_scale)
    e = lse
    return [out, _e(bias_p, e), lse, qmean, kmean, omega, beta, rf_k_bar, _e(saved, e), _e(zhat, e), _e(rstd, e)]


def eva_bwd_impl(dout, qkv5, mask_u8, keep, noise, out, saved_list, icfg, fcfg, adaptive_proj, bias_cols, mlp_params):
    """torch.ops.ea.eva_bwd -> [dqkv, dbias | empty, *parameter gradients (fp32, in the order of mlp_params)]."""
    cfg, _ = EvaCfg.from_lists(icfg, fcfg, adaptive_proj)
    g = _eva_backward(dout, qkv5, mask_u8, keep, noise, out, saved_list, cfg, bias_cols, mlp_params)
    return [g.dqkv, _e(g.dbias, saved_list[1])] + g.params


def _eva_backward(dout, qkv5, mask_u8, keep, noise, out, saved_list, cfg, bias_cols, mlp_params,
                  defer_param_sums=False, defer_chunk_mean=False):
    """The EVA core's backward -> CoreGrads.  defer_param_sums: the per-(b,h) partials of the mu networks' (composite: and the bias)
    gradients wait for the caller's terminal sum; defer_chunk_mean (composite only, round 5): ea_linear_dgrad_finish adds
    d(chunk mean) / r^2 to dq, dk on its way through the gradient rows."""
    B, N, _, h, d = qkv5.shape
    noise_c = None if noise is None else noise.float().contiguous()
    dqkv5 = torch.empty_like(qkv5)
    if _eva_saved_is_composite(saved_list):
        bias_p, ws = _opt(saved_list[0]), saved_list[1]
        lcfg, sizes = _eva_layer_cfg_dims(B, h, d, nv.io_dtype(qkv5), cfg, bias_p is not None, False)
        if lcfg is None:
            raise RuntimeError("eva_bwd: a composite workspace was saved for a geometry ea_eva_layer_plan rejects")
        dout = _rows_contiguous(dout)
        q, k, v = _qkv_views(qkv5)
        dq, dk, dv = _qkv_views(dqkv5)
        ts = [nv.t4(t) for t in (q, k, v, out.permute(0, 2, 1, 3), dout.permute(0, 2, 1, 3), dq, dk, dv)]
        tmp = torch.empty(sizes.n_bwd_tmp, dtype=torch.float32, device=qkv5.device)
        ps = [_f32c(p) for p in mlp_params]
        # deferred sums: the bias-gradient partials join the caller's terminal reductions too (one launch for all of them)
        defer_bias = bool(defer_param_sums and bias_p is not None)
        dbias = None if (bias_p is None or defer_bias) else torch.empty_like(bias_p)
        dpar = None if defer_param_sums else torch.empty(2 * d * d + 6 * d, dtype=torch.float32, device=qkv5.device)
        nv.call("ea_eva_layer_bwd", ctypes.byref(lcfg), ctypes.byref(ts[0]), ctypes.byref(ts[1]), ctypes.byref(ts[2]),
                nv.ptr(bias_p), nv.ptr(noise_c), _param_ptrs(ps), ctypes.byref(ts[3]), ctypes.byref(ts[4]), ctypes.byref(ts[5]),
                ctypes.byref(ts[6]), ctypes.byref(ts[7]), nv.ptr(ws), nv.ptr(tmp), nv.ptr(dbias), nv.ptr(dpar),
                1 if defer_chunk_mean else 0, nv.stream())
        if dbias is not None:
            dbias = dbias[..., :bias_cols].contiguous()
        BH, fin = B * h, None
        if defer_chunk_mean:
            Lc = (lcfg.gh // lcfg.chunk) * (lcfg.gw // lcfg.chunk)
            fin = Finish(B=B, gh=lcfg.gh, gw=lcfg.gw, r=lcfg.chunk, C=Lc, scale=float(lcfg.scale),
                         dpq=_ws_rows(tmp, sizes.bwd_dqmean, BH * Lc * d), dpk=_ws_rows(tmp, sizes.bwd_dkmean, BH * Lc * d))
        if not defer_param_sums:
            return CoreGrads(dqkv5, dbias, _mlp_grads(dpar[:2 * d * d], dpar[2 * d * d:], d), (), fin)
        parts = _param_partials(_ws_rows(tmp, sizes.bwd_dW, BH, 2 * d * d), _ws_rows(tmp, sizes.bwd_dvec, BH, 6 * d))
        if defer_bias:
            parts.append(("dbias", _ws_rows(tmp, sizes.bwd_dbias_part, sizes.dbias_part_rows, bias_p.numel()), tuple(bias_p.shape)))
        return CoreGrads(dqkv5, dbias, None, parts, fin)
    if defer_chunk_mean:
        raise RuntimeError("eva_bwd: defer_chunk_mean needs the composite entry points")
    geom, fused_mu = _eva_cfg(qkv5, cfg)
    L, mu_scale = cfg.L, cfg.mu_scale
    bias_p, lse, qmean, kmean, omega, beta, rf_k_bar, saved, zhat, rstd = [_opt(t) for t in saved_list]
    d_rfk, d_beta, dbias = _window_bwd(geom, qkv5, rf_k_bar, beta, bias_p, mask_u8, out,
                                       _rows_contiguous(dout), lse, dqkv5, keep, cfg.keep_scale)
    q, k, v = _qkv_views(qkv5)
    dq, dk, dv = _qkv_views(dqkv5)
    tk, tv, tdq, tdk, tdv = nv.t4(k), nv.t4(v), nv.t4(dq), nv.t4(dk), nv.t4(dv)
    d_omega = torch.empty_like(omega)
    d_beta = d_beta.contiguous()
    nv.call("ea_eva_beta_bwd", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv),
            nv.ptr(mask_u8), nv.ptr(omega), nv.ptr(beta), nv.ptr(d_beta), ctypes.byref(tdk),
            ctypes.byref(tdv), nv.ptr(d_omega), nv.stream())
    ps = [_f32c(p) for p in mlp_params]
    if dbias is not None:
        dbias = dbias[..., :bias_cols].contiguous()
    if fused_mu:
        lg = nv.ea_lmk_geom(B * h, L, L, d, 1, 0, 0, 0, float(d) ** -0.5, 1)
        dqm = torch.empty_like(qmean)
        dkm = torch.empty_like(kmean)
        dW = torch.empty((lg.BH, 2, d, d), dtype=torch.float32, device=qmean.device)
        dvec = torch.empty((lg.BH, 2, 3, d), dtype=torch.float32, device=qmean.device)
        nv.call("ea_lara_landmarks_bwd", ctypes.byref(lg), nv.ptr(qmean), nv.ptr(kmean),
                *[nv.ptr(t) for t in ps], nv.ptr(noise_c), nv.ptr(d_omega), nv.ptr(d_rfk.contiguous()),
                None, None, nv.ptr(dqm), nv.ptr(dkm), nv.ptr(dW), nv.ptr(dvec), nv.ptr(saved), nv.stream())
        nv.call("ea_eva_chunk_mean_bwd", ctypes.byref(geom), nv.ptr(dqm), nv.ptr(dkm),
                nv.ptr(mask_u8), ctypes.byref(tdq), ctypes.byref(tdk), nv.stream())
        if defer_param_sums:                       # the per-(b,h) partials, still to be added up
            return CoreGrads(dqkv5, dbias, None, _param_partials(dW.view(lg.BH, -1), dvec.view(lg.BH, -1)), None)
        return CoreGrads(dqkv5, dbias, _mlp_grads(*colsum2_f32(dW.view(lg.BH, -1), dvec.view(lg.BH, -1)), d), (), None)
    # mu networks backward (ea_rows_mlp_bwd): dz, dx = d(chunk means), per-workgroup dW partials
    # and the feed buffer whose column sums are the bias / gamma / beta gradients
    sides = 1 if cfg.adaptive_proj == "none" else 2
    ln = cfg.adaptive_proj != "no-ln"
    per = 4 if ln else 2
    side_p = [ps[i * per:(i + 1) * per] for i in range(sides)]
    R = B * h * L
    d_rfk = d_rfk.contiguous()
    if sides == 2:
        d_rq = d_omega.contiguous() if mu_scale == 1.0 else (mu_scale * d_omega).contiguous()
        dys = [d_rq, d_rq + d_rfk]
        xs = [qmean, kmean]
    else:
        dys, xs = [d_rfk], [kmean]
    dxs = [torch.empty_like(kmean) for _ in range(sides)]
    planes = 3 if ln else 1
    parts = nv.lib().ea_rows_mlp_parts(R, d)
    feed = torch.empty((R, planes, sides, d), dtype=torch.float32, device=kmean.device)
    dW_part = torch.empty((parts, sides, d, d), dtype=torch.float32, device=kmean.device)

    def two(ts):
        ts = list(ts) + [None]
        return [nv.ptr(ts[0]), nv.ptr(ts[1])]
    nv.call("ea_rows_mlp_bwd", R, d, sides, 1 if ln else 0, *two(dys), *two(xs),
            *two([sp[0] for sp in side_p]), *two([sp[2] if ln else None for sp in side_p]),
            nv.ptr(zhat), nv.ptr(rstd), *two(dxs), nv.ptr(feed), nv.ptr(dW_part), nv.stream())
    dkm = dxs[-1]
    dqm = dxs[0] if sides == 2 else torch.zeros_like(qmean)
    nv.call("ea_eva_chunk_mean_bwd", ctypes.byref(geom), nv.ptr(dqm), nv.ptr(dkm),
            nv.ptr(mask_u8), ctypes.byref(tdq), ctypes.byref(tdk), nv.stream())
    dW = colsum_f32(dW_part.view(parts, -1)).view(sides, d, d)
    vec = colsum_f32(feed.view(R, -1)).view(planes, sides, d)
    raw = []
    for i in range(sides):
        raw += [dW[i], vec[0, i]] + ([vec[1, i], vec[2, i]] if ln else [])
    return CoreGrads(dqkv5, dbias, raw, (), None)


class EvaAttnFn(torch.autograd.Function):
    """EVA core on a fused qkv tensor (torch.ops.ea.eva_fwd / eva_bwd): chunk means -> mu MLP -> omega ->
    beta -> window attention with control-variate columns.  Returns out [B,N,h,d].
    cfg: an EvaCfg; extras: an EvaExtras (keep mask, TableBias, pooled chunk means) or None."""

    @staticmethod
    def forward(ctx, qkv5, bias, noise, mask_u8, cfg, extras, *mlp_params):
        keep, tb, pooled = extras or EvaExtras()
        icfg, fcfg = cfg.lists(any(ctx.needs_input_grad))
        direct = _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0
        # a TableBias (round 6; direct calls only): `bias` is the TABLE ([rows, h] or [rows, 1]) and the dense bias is built
        # from it / its gradient taken back to it in one launch each way
        ctx.tb, ctx.tb_heads = tb, None
        if tb is not None:
            if not direct:
                raise RuntimeError("EvaAttnFn: a TableBias spec needs the direct (untraced) call path")
            B_, N_, _, h_, d_ = qkv5.shape
            ctx.tb_heads = bias.shape[1]
            bias = tb.dense(bias, tb.ld(B_, h_, N_, d_, nv.io_dtype(qkv5), cfg.attn_2d, cfg.seq_shape, cfg.window, cfg.ext,
                                        int(cfg.chunk), int(cfg.L), int(cfg.causal)), heads=h_)
        if pooled is not None:
            outs = eva_fwd_impl(qkv5, bias, noise, mask_u8, keep, icfg, fcfg, cfg.adaptive_proj, list(mlp_params), pooled=pooled)
        elif direct:
            # round 4: one C-ABI call for the whole core where the geometry allows it (ea_eva_layer_fwd)
            outs = eva_fwd_impl(qkv5, bias, noise, mask_u8, keep, icfg, fcfg, cfg.adaptive_proj, list(mlp_params),
                                composite=_eva_use_composite())
        else:
            outs = _ea_op("eva_fwd", eva_fwd_impl, qkv5, bias, noise, mask_u8, keep, icfg, fcfg, cfg.adaptive_proj, list(mlp_params))
        ctx.save_for_backward(qkv5, mask_u8, keep, noise, *outs, *mlp_params)
        ctx.nsaved = len(outs) - 1
        ctx.cfg, ctx.bias_cols = cfg, 0 if bias is None else bias.shape[-1]
        ctx.pdtypes = [p.dtype for p in mlp_params]
        return outs[0]

    @staticmethod
    def backward(ctx, dout):
        qkv5, mask_u8, keep, noise, out, *rest = ctx.saved_tensors
        saved, params = rest[:ctx.nsaved], rest[ctx.nsaved:]
        cfg = ctx.cfg
        head, tail = (dout, qkv5, mask_u8, keep, noise, out, list(saved)), (ctx.bias_cols, list(params))
        if _eva_saved_is_composite(saved):             # only a direct forward saves a composite workspace
            g = _eva_backward(*head, cfg, *tail)
        elif ctx.tb is not None and ctx.tb_heads == 1 and BIAS_HEAD_SUM:
            # (a TableBias means a direct call: the implementation runs right here, in this thread)
            _BIAS_HEAD_SUM.on = True
            try:
                g = _eva_backward(*head, cfg, *tail)
            finally:
                _BIAS_HEAD_SUM.on = False
        else:
            g = _ea_op("eva_bwd", eva_bwd_impl, *head, *cfg.lists(True), cfg.adaptive_proj, *tail)
            g = CoreGrads(g[0], _opt(g[1]), g[2:], (), None)
        pgrads = [t.to(dt) for t, dt in zip(g.params, ctx.pdtypes)]
        dbias = g.dbias
        if ctx.tb is not None and dbias is not None:
            dbias = ctx.tb.grad(dbias, ctx.tb_heads)
        return (g.dqkv, dbias, None, None, None, None) + tuple(pgrads)


USE_EVA_MODULE_FN = os.environ.get("EA_EVA_MODULE_FN", "1") == "1"


def eva_module_fn_supported(x, qkv, proj, cdtype, adaptive_proj, L, d):
    """The single-node path of EVA (EvaModuleFn = CoreModuleFn around an EvaCore): what the module node needs of the projections
    (lara_module_fn_supported), plus the fused landmark kernel for the mu networks (adaptive_proj 'default', L <= 64, d in {32, 64})."""
    return (USE_EVA_MODULE_FN and adaptive_proj == "default" and L <= 64 and d in (32, 64)
            and lara_module_fn_supported(x, qkv, proj, cdtype, allow_lib=True)
            and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0 and _DIRECT)


# ------------------------------------------------------------------------------------------
# LARA  (reference lara.py:177-251)
# ------------------------------------------------------------------------------------------
MIS = {"mis-opt": 0, "mis-biased": 1, "mis-bh": 2}


class _GradSlot:
    """Side channel between two autograd Functions that share one gradient buffer: the core's
    backward publishes the [B,N,3,h,d] buffer it returns for qkv; the pooling backward, which the
    graph orders after it (its outputs feed the core), accumulates into that buffer in place and
    reports no gradient of its own, so autograd never materialises a second full-size tensor."""

    def __init__(self):
        self.buf = None
        # LARA 'adaptive-1d' (round 6): the core's backward leaves its last dq correction (ea_lara_bwd_finish's operands) here
        # instead of running it when `defer_fin` is set; the segment backward, which rewrites the dq rows anyway, applies it
        self.defer_fin = False
        self.fin = None


class PoolMeanFn(torch.autograd.Function):
    """Uniform 2-D average pool of q and k over r x r token blocks -> fp32 [B,h,L,d] x2 through the
    chunk-mean kernel (the adaptive pool of lara.py:43,48 when the grid divides evenly)."""

    @staticmethod
    def forward(ctx, qkv5, H, W, r, slot):
        nv.require_cuda(qkv5, "qkv")
        B, N, _, h, d = qkv5.shape
        L = (H // r) * (W // r)
        geom = nv.make_geom(B, h, N, d, nv.io_dtype(qkv5), True, (H, W), r, 0, r, L)
        q, k, _ = _qkv_views(qkv5)
        tq, tk = nv.t4(q), nv.t4(k)
        qmean = torch.empty((B, h, L, d), dtype=torch.float32, device=qkv5.device)
        kmean = torch.empty_like(qmean)
        nv.call("ea_eva_chunk_mean_fwd", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), None,
                nv.ptr(qmean), nv.ptr(kmean), nv.stream())
        ctx.geom, ctx.slot = geom, slot
        ctx.shape, ctx.dtype = qkv5.shape, qkv5.dtype
        return qmean, kmean

    @staticmethod
    def backward(ctx, dqm, dkm):
        slot = ctx.slot
        dqm = dqm.float().contiguous()
        dkm = dkm.float().contiguous()
        own = slot.buf is None
        buf = torch.zeros(ctx.shape, dtype=ctx.dtype, device=dqm.device) if own else slot.buf
        dq, dk, _ = _qkv_views(buf)
        tdq, tdk = nv.t4(dq), nv.t4(dk)
        nv.call("ea_eva_chunk_mean_bwd", ctypes.byref(ctx.geom), nv.ptr(dqm), nv.ptr(dkm), None,
                ctypes.byref(tdq), ctypes.byref(tdk), nv.stream())
        slot.buf = None
        return (buf if own else None), None, None, None, None


class SegmentLnMeanFn(torch.autograd.Function):
    """LARA 'adaptive-1d' proposals (lara.py:84-127): segment means of LayerNorm(Linear(q)) and
    LayerNorm(Linear(k)).  The Linear is folded into the qkv projection by the module, whose output
    qkvE [B,N,5,h,d] carries its (bias-free) rows in slots 3 and 4; this Function normalises and
    averages them (ea_lara_segment_fwd/bwd) and, like the 2-D pooling, writes its input gradient
    straight into the gradient buffer the attention core publishes for qkvE.
    bias_* [h,d]: bias of an ordinary token's row; mbias_* [d]: the whole row of a masked token."""

    @staticmethod
    def forward(ctx, qkvE, mask_u8, L, slot, bias_q, bias_k, mbias_q, mbias_k, gq, cq, gk, ck):
        nv.require_cuda(qkvE, "qkv")
        B, N, S, h, d = qkvE.shape
        geom = nv.make_geom(B, h, N, d, nv.io_dtype(qkvE), False, (N,), 0, 0, 0, L)
        ps = [t.detach().float().contiguous() for t in (bias_q, bias_k, mbias_q, mbias_k, gq, cq, gk, ck)]
        q2, k2 = qkvE[:, :, 3].permute(0, 2, 1, 3), qkvE[:, :, 4].permute(0, 2, 1, 3)
        tq, tk = nv.t4(q2), nv.t4(k2)
        qbar = torch.empty((B, h, L, d), dtype=torch.float32, device=qkvE.device)
        kbar = torch.empty_like(qbar)
        nv.call("ea_lara_segment_fwd", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), nv.ptr(mask_u8),
                *[nv.ptr(t) for t in ps], nv.ptr(qbar), nv.ptr(kbar), nv.stream())
        ctx.save_for_backward(qkvE, mask_u8, *ps)
        ctx.geom, ctx.slot = geom, slot
        return qbar, kbar

    @staticmethod
    def backward(ctx, dqb, dkb):
        qkvE, mask_u8, *ps = ctx.saved_tensors
        geom, slot = ctx.geom, ctx.slot
        B, N, S, h, d = qkvE.shape
        L = geom.L
        own = slot is None or slot.buf is None
        buf = torch.zeros_like(qkvE) if own else slot.buf
        q2, k2 = qkvE[:, :, 3].permute(0, 2, 1, 3), qkvE[:, :, 4].permute(0, 2, 1, 3)
        dq2, dk2 = buf[:, :, 3].permute(0, 2, 1, 3), buf[:, :, 4].permute(0, 2, 1, 3)
        ts = [nv.t4(t) for t in (q2, k2, dq2, dk2)]
        part = torch.empty((B, h, L, 2, 4, d), dtype=torch.float32, device=qkvE.device)
        nv.call("ea_lara_segment_bwd", ctypes.byref(geom), ctypes.byref(ts[0]), ctypes.byref(ts[1]), nv.ptr(mask_u8),
                *[nv.ptr(t) for t in ps], nv.ptr(dqb.float().contiguous()), nv.ptr(dkb.float().contiguous()),
                ctypes.byref(ts[2]), ctypes.byref(ts[3]), nv.ptr(part), nv.stream())
        if slot is not None:
            slot.buf = None
        sums = part.sum((0, 2))                                   # [h, 2, 4, d]
        tot = sums.sum(0)                                         # [2, 4, d]
        # bias_q, bias_k, mbias_q, mbias_k, gq, cq, gk, ck
        grads = (sums[:, 0, 2], sums[:, 1, 2], tot[0, 3], tot[1, 3], tot[0, 0], tot[0, 1], tot[1, 0], tot[1, 1])
        return ((buf if own else None), None, None, None) + grads


USE_SEGLIN = os.environ.get("EA_SEGLIN", "1") == "1"
# dev switch: the estimator's last dq correction applied by the segment backward (ea_lara_seglin_bwd_fin) instead of a pass of its own
USE_SEGLIN_FIN = os.environ.get("EA_SEGLIN_FIN", "1") == "1"


class SegLinLnMeanFn(torch.autograd.Function):
    """LARA 'adaptive-1d' proposals (lara.py:56-63,84-127) from the stored q / k rows of qkv5 [B,N,3,h,64]: generator Linear,
    LayerNorm and segment mean in one HIP pass each way (ea_lara_seglin_fwd / _bwd; round 4) -- the qkv projection stays 3C wide.
    The backward ACCUMULATES its input gradient into the gradient buffer the attention core publishes for qkv5 (slot.buf), like
    the 2-D pooling does.  -> q_bar, k_bar [B,h,L,64] fp32."""

    @staticmethod
    def forward(ctx, qkv5, L, slot, Gq, gqb, Gk, gkb, lqw, lqb, lkw, lkb):
        nv.require_cuda(qkv5, "qkv")
        B, N, _, h, d = qkv5.shape
        geom = nv.make_geom(B, h, N, d, nv.io_dtype(qkv5), False, (N,), 0, 0, 0, L)
        ps = [t.detach().float().contiguous() for t in (Gq, gqb, Gk, gkb, lqw, lqb, lkw, lkb)]
        q, k, _ = _qkv_views(qkv5)
        tq, tk = nv.t4(q), nv.t4(k)
        qbar = torch.empty((B, h, L, d), dtype=torch.float32, device=qkv5.device)
        kbar = torch.empty_like(qbar)
        nv.call("ea_lara_seglin_fwd", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk), *[nv.ptr(t) for t in ps],
                nv.ptr(qbar), nv.ptr(kbar), nv.stream())
        ctx.save_for_backward(qkv5, *ps)
        ctx.geom, ctx.slot = geom, slot
        ctx.pdtypes = [t.dtype for t in (Gq, gqb, Gk, gkb, lqw, lqb, lkw, lkb)]
        return qbar, kbar

    @staticmethod
    def backward(ctx, dqb, dkb):
        qkv5, *ps = ctx.saved_tensors
        geom, slot = ctx.geom, ctx.slot
        B, N, _, h, d = qkv5.shape
        L = geom.L
        dev = qkv5.device
        own = slot is None or slot.buf is None
        buf = torch.zeros_like(qkv5) if own else slot.buf
        q, k, _ = _qkv_views(qkv5)
        dq, dk, _ = _qkv_views(buf)
        ts = [nv.t4(t) for t in (q, k, dq, dk)]
        groups = nv.query("ea_lara_seglin_groups", geom)
        part = torch.empty((B * h * groups, 2 * 4 * d), dtype=torch.float32, device=dev)
        dG_part = torch.empty((B * h * groups, 2 * d * d), dtype=torch.float32, device=dev)
        stats = torch.empty((B * h * 2 * N, 4), dtype=torch.float32, device=dev)
        fin = None if (own or slot is None) else slot.fin
        common = [ctypes.byref(geom), ctypes.byref(ts[0]), ctypes.byref(ts[1]), *[nv.ptr(t) for t in ps],
                  nv.ptr(dqb.float().contiguous()), nv.ptr(dkb.float().contiguous()), ctypes.byref(ts[2]), ctypes.byref(ts[3]),
                  nv.ptr(part), nv.ptr(dG_part), nv.ptr(stats)]
        if fin is not None:
            f_qbar, f_uq, f_lse, f_C, f_scale = fin
            nv.call("ea_lara_seglin_bwd_fin", *common, nv.ptr(f_qbar), nv.ptr(f_uq), nv.ptr(f_lse), int(f_C), float(f_scale),
                    nv.stream())
        else:
            nv.call("ea_lara_seglin_bwd", *common, nv.stream())
        if slot is not None:
            slot.buf = None
            slot.fin = None
        # tall, narrow partial matrices: the column-sum kernel (64 row lanes per 16 columns), not the slice reduction
        sums, dGs = colsum2_f32(part, dG_part)                        # (same number of rows: one launch)
        sums, dGs = sums.view(2, 4, d), dGs.view(2, d, d)
        # Gq, gqb, Gk, gkb, lqw, lqb, lkw, lkb
        grads = [dGs[0], sums[0, 2], dGs[1], sums[1, 2], sums[0, 0], sums[0, 1], sums[1, 0], sums[1, 1]]
        grads = [g_.to(dt) for g_, dt in zip(grads, ctx.pdtypes)]
        return ((buf if own else None), None, None) + tuple(grads)


USE_FOLD_KERNELS = os.environ.get("EA_FOLD_KERNELS", "1") == "1"


class FoldedQkvFn(torch.autograd.Function):
    """LARA 'adaptive-1d' (lara.py:56-63,100-103): qkv projection with the generators' per-token Linear folded in --
    x [B,N,C] -> (qkvE [B,N,5C] in `dtype`: q, k, v, G_q q, G_k k without the folded rows' biases; bias_q, bias_k [h,d] fp32:
    those biases).  The extended weight is built and its gradient taken apart by ea_lara_fold_fwd / _bwd (one launch each
    way instead of ~30 framework kernels: cat / permute copies / small GEMMs / casts / adds); the GEMMs are the library's
    (512-wide models), the weight gradient ea_wgrad."""

    @staticmethod
    def forward(ctx, x, W, b, Gq, gqb, Gk, gkb, dtype, heads):
        C = x.shape[-1]
        d = C // heads
        dev = x.device
        x2 = x.reshape(-1, C)
        xl = x2 if x2.dtype == dtype else x2.to(dtype)
        ps = [None if t is None else t.detach().float().contiguous() for t in (W, b, Gq, gqb, Gk, gkb)]
        w_ext = torch.empty((5 * C, C), dtype=dtype, device=dev)
        b_ext = torch.empty((5 * C,), dtype=dtype, device=dev)
        bias_q = torch.empty((heads, d), dtype=torch.float32, device=dev)
        bias_k = torch.empty_like(bias_q)
        nv.call("ea_lara_fold_fwd", _ELEM[dtype], C, heads, nv.ptr(ps[0]), nv.ptr(ps[1]), nv.ptr(ps[2]), nv.ptr(ps[3]),
                nv.ptr(ps[4]), nv.ptr(ps[5]), nv.ptr(w_ext), nv.ptr(b_ext), nv.ptr(bias_q), nv.ptr(bias_k), nv.stream())
        y = F.linear(xl, w_ext, b_ext)
        ctx.save_for_backward(xl, w_ext, *[t for t in ps if t is not None])
        ctx.has_b = b is not None
        ctx.meta = (x.shape, x.dtype, heads, [None if t is None else t.dtype for t in (W, b, Gq, gqb, Gk, gkb)])
        return y.view(x.shape[:-1] + (5 * C,)), bias_q, bias_k

    @staticmethod
    def backward(ctx, dy, dbias_q, dbias_k):
        xl, w_ext, *ps = ctx.saved_tensors
        xshape, xdtype, heads, pd = ctx.meta
        if ctx.has_b:
            W, b, Gq, gqb, Gk, gkb = ps
        else:
            (W, Gq, gqb, Gk, gkb), b = ps, None
        C = xshape[-1]
        d = C // heads
        dev = dy.device
        dy2 = dy.reshape(-1, 5 * C)
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        dx = _mm_out(dy2, w_ext, xdtype).view(xshape) if ctx.needs_input_grad[0] else None
        if wgrad_supported(dy2, xl):
            dW_ext, db_ext = wgrad(dy2, xl, b is not None)
        else:
            dW_ext = torch.mm(dy2.t(), xl).float()
            db_ext = dy2.sum(0, dtype=torch.float32) if b is not None else None
        zq = torch.zeros((heads, d), dtype=torch.float32, device=dev)
        dbq = zq if dbias_q is None else dbias_q.float().contiguous()
        dbk = zq if dbias_k is None else dbias_k.float().contiguous()
        dW = torch.empty((3 * C, C), dtype=torch.float32, device=dev)
        db = torch.empty((3 * C,), dtype=torch.float32, device=dev) if b is not None else None
        dG = torch.empty((2, d, d), dtype=torch.float32, device=dev)
        S = nv.lib().ea_lara_fold_parts(heads)
        scratch = torch.empty(((2 * S + 2) * d * d,), dtype=torch.float32, device=dev)
        dgqb = torch.empty((d,), dtype=torch.float32, device=dev)
        dgkb = torch.empty_like(dgqb)
        nv.call("ea_lara_fold_bwd", C, heads, nv.ptr(W), nv.ptr(b), nv.ptr(Gq), nv.ptr(Gk), nv.ptr(dW_ext), dW_ext.stride(0),
                nv.ptr(db_ext), nv.ptr(dbq), nv.ptr(dbk), nv.ptr(dW), nv.ptr(db), nv.ptr(dG), nv.ptr(scratch), nv.ptr(dgqb),
                nv.ptr(dgkb), nv.stream())
        outs = [dW, db, dG[0], dgqb, dG[1], dgkb]
        outs = [None if (o is None or t is None) else o.to(t) for o, t in zip(outs, pd)]
        return (dx,) + tuple(outs) + (None, None)


def pool2d_qkv(qkv5, H, W, side, slot=None, need_v=False):
    """Adaptive 2-D average pool of q, k (and v when asked) over the token grid -> fp32
    [B, h, side*side, d] each (nn.AdaptiveAvgPool2d on each head's [d, H, W] map,
    lara.py:43,48,145-151,166-169).  Evenly dividing grids go through the HIP chunk-mean kernel."""
    B, N, _, h, d = qkv5.shape
    pv = None
    if H % side == 0 and W % side == 0 and H // side == W // side:
        pq, pk = PoolMeanFn.apply(qkv5, H, W, H // side, slot if slot is not None else _GradSlot())
        if need_v:
            x = qkv5.view(B, side, H // side, side, W // side, 3, h, d)[:, :, :, :, :, 2]
            pv = x.mean(dim=(2, 4), dtype=torch.float32).reshape(B, side * side, h, d).permute(0, 2, 1, 3)
        return pq, pk, pv

    # bins that overlap (the grid does not divide): adaptive-pool kernels, one launch per tensor
    slot = slot if slot is not None else _GradSlot()
    outs = AdaptivePoolFn.apply(qkv5, H, W, side, 3 if need_v else 2, slot)
    return outs[0], outs[1], (outs[2] if need_v else None)


class AdaptivePoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d of q, k (and v) over a token grid `side` does not divide (ea_adaptive_pool2d_fwd/bwd);
    like PoolMeanFn its input gradient is added into the buffer the attention core publishes for qkv."""

    @staticmethod
    def forward(ctx, qkv5, H, W, side, n, slot):
        nv.require_cuda(qkv5, "qkv")
        B, N, _, h, d = qkv5.shape
        outs = []
        for t in _qkv_views(qkv5)[:n]:
            m = torch.empty((B, h, side * side, d), dtype=torch.float32, device=qkv5.device)
            tt = nv.t4(t)
            nv.call("ea_adaptive_pool2d_fwd", nv.io_dtype(qkv5), B, h, H, W, side, d, ctypes.byref(tt), nv.ptr(m), nv.stream())
            outs.append(m)
        ctx.cfg = (H, W, side, n, slot, qkv5.shape, qkv5.dtype)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dms):
        H, W, side, n, slot, shape, dtype = ctx.cfg
        B, N, _, h, d = shape
        own = slot.buf is None
        buf = torch.zeros(shape, dtype=dtype, device=dms[0].device) if own else slot.buf
        for t, dm in zip(_qkv_views(buf)[:n], dms):
            if dm is None:
                continue
            tt = nv.t4(t)
            nv.call("ea_adaptive_pool2d_bwd", nv.io_dtype(buf), B, h, H, W, side, d, nv.ptr(dm.float().contiguous()),
                    ctypes.byref(tt), nv.stream())
        slot.buf = None
        return (buf if own else None), None, None, None, None, None


def lara_fold(C, S):
    """Round 5: the merge launches between the LARA token passes are folded into their consumers (C <= 64 samples, S <= 4
    slices): ea_lara_out_fwd_merge, ea_lara_bwd_k_fused_merge, ea_lara_landmarks_bwd_parts.  EA_LARA_FOLD=0 keeps the merge
    launches (the composite entry points read the same switch)."""
    return C <= 64 and 1 <= S <= 4 and os.environ.get("EA_LARA_FOLD", "1") != "0"


def lara_out_proj_on():
    """ABI 29: the output projection of a three-head, 64-channel layer inside the forward combine (ea_lara_xp.hip).
    EA_LARA_OUT_PROJ=0 keeps the two launches (read per call: the tests and the A/B runs switch it inside one process)."""
    return os.environ.get("EA_LARA_OUT_PROJ", "1") != "0"


def _lara_proj_fallback(out, proj):
    """The library declined the fused launch (it does so before launching anything): the projection as its own launch."""
    proj[2] = ea_linear(out.view(out.shape[0] * out.shape[1], -1), proj[0], proj[1], out.dtype)[0]


def _lara_fwd_core(geom, qkv5, mask_u8, omega, qbar_c, bhv_c, lp_c, want_tokst=True, proj=None):
    """Estimator forward (ea_lara_stats_fwd -> ea_lara_merge_fwd -> ea_lara_out_fwd) on contiguous fp32
    landmark tensors [BH,C,d] / [BH,C].  Returns out [B,N,h,d] and (cst, kv, lse_k, lse_t).
    proj = [w16p, bias32, y2]: the output projection y2 = out W^T + bias leaves with the combine pass (or, declined, after it)."""
    B, N, _, h, d = qkv5.shape
    C, BH, dev, mis = geom.C, B * h, qkv5.device, geom.mis
    q, k, v = _qkv_views(qkv5)
    tq, tk, tv = nv.t4(q), nv.t4(k), nv.t4(v)
    S = nv.lib().ea_lara_parts(ctypes.byref(geom))
    p_ml = torch.empty((BH, S, C, 4), dtype=torch.float32, device=dev)
    p_kv = torch.empty((BH, S, C, d), dtype=torch.float32, device=dev)
    nv.call("ea_lara_stats_fwd", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tk),
            ctypes.byref(tv), nv.ptr(mask_u8), nv.ptr(omega), nv.ptr(qbar_c), nv.ptr(p_ml),
            nv.ptr(p_kv), nv.stream())
    kv = torch.empty((BH, C, d), dtype=torch.float32, device=dev)
    lse_k = torch.empty((BH, C), dtype=torch.float32, device=dev)     # (separate allocations: they leave the
    cst = torch.empty_like(lse_k)                                     #  dispatcher op as distinct outputs)
    lse_t = torch.empty_like(lse_k) if mis == 0 else None
    out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=dev)
    to = nv.t4(out.permute(0, 2, 1, 3))
    # per-token softmax statistics (lse_Z in log2 units, mean_c t) for the fused backward: 8 bytes per token-head
    tokst = torch.empty((2, BH, N), dtype=torch.float32, device=dev) if (want_tokst and C <= 64) else None
    if proj is not None and lara_fold(C, S):
        label = "ea_lara_out_proj_fwd"
        if nv.KERNEL_TIMER.enabled:
            _note_bytes(label, B * N * 3 * h * d * 2)                 # q in, out and y out
        if nv.call_probe(label, "ea_lara_out_proj_fwd_merge", ctypes.byref(geom), ctypes.byref(tq), nv.ptr(omega), nv.ptr(qbar_c),
                         nv.ptr(bhv_c), S, nv.ptr(p_ml), nv.ptr(p_kv), nv.ptr(lp_c), nv.ptr(kv), nv.ptr(lse_k), nv.ptr(lse_t),
                         nv.ptr(cst), ctypes.byref(to), nv.ptr(tokst), None if tokst is None else nv.ptr(tokst[1]),
                         nv.ptr(proj[0]), nv.ptr(proj[1]), nv.ptr(proj[2]), proj[2].stride(0), nv.stream()):
            return out, (cst, kv, lse_k, lse_t, tokst)
    if lara_fold(C, S):
        # round 5: the combine pass merges the slice partials in its prologue (block 0 of a (b,h) writes kv / lse / cst)
        nv.call_as("ea_lara_out_fwd", "ea_lara_out_fwd_merge", ctypes.byref(geom), ctypes.byref(tq), nv.ptr(omega), nv.ptr(qbar_c), nv.ptr(bhv_c),
                S, nv.ptr(p_ml), nv.ptr(p_kv), nv.ptr(lp_c), nv.ptr(kv), nv.ptr(lse_k), nv.ptr(lse_t), nv.ptr(cst),
                ctypes.byref(to), nv.ptr(tokst), None if tokst is None else nv.ptr(tokst[1]), nv.stream())
        if proj is not None:
            _lara_proj_fallback(out, proj)
        return out, (cst, kv, lse_k, lse_t, tokst)
    # merge the sequence slices: log-sum-exp merge of the online-softmax partials (one tiny kernel)
    nv.call("ea_lara_merge_fwd", BH, S, C, d, 1 if mis == 0 else 0, nv.ptr(p_ml), nv.ptr(p_kv),
            nv.ptr(lp_c), nv.ptr(kv), nv.ptr(lse_k), nv.ptr(lse_t), nv.ptr(cst), nv.stream())
    nv.call("ea_lara_out_fwd", ctypes.byref(geom), ctypes.byref(tq), nv.ptr(omega), nv.ptr(qbar_c),
            nv.ptr(kv), nv.ptr(lse_t), nv.ptr(bhv_c), nv.ptr(cst), ctypes.byref(to),
            nv.ptr(tokst), None if tokst is None else nv.ptr(tokst[1]), nv.stream())
    if proj is not None:
        _lara_proj_fallback(out, proj)
    return out, (cst, kv, lse_k, lse_t, tokst)


def _lara_bwd_core(geom, qkv5, mask_u8, dout, dqkv5, omega, qbar, bhv, cst, kv, lse_k, lse_t, tokst, want_parts=False):
    """Estimator backward up to (not including) the softmax-over-sequence correction of dq.
    Writes dq (uncorrected), dk, dv into dqkv5; returns d_omega [BH,C,d], d_qbar, d_bhv, d_lp and uq
    (the u_c q_bar_c rows of the correction, mis-opt only).
    C <= 64: one fused pass per side (ea_lara_bwd_q_fused / ea_lara_bwd_k_fused); larger sample counts
    take the round-1 two-pass kernels."""
    B, N, _, h, d = qkv5.shape
    C, BH, dev, mis = geom.C, B * h, qkv5.device, geom.mis
    scale = geom.scale
    q, k, v = _qkv_views(qkv5)
    dq, dk, dv = _qkv_views(dqkv5)
    tq, tk, tv, tdo = nv.t4(q), nv.t4(k), nv.t4(v), nv.t4(dout.permute(0, 2, 1, 3))
    tdq, tdk, tdv = nv.t4(dq), nv.t4(dk), nv.t4(dv)
    fused = C <= 64
    if fused:
        S = nv.lib().ea_lara_fused_parts(ctypes.byref(geom))
        if S <= 0:
            raise RuntimeError("ea_lara_fused_parts: %d" % S)
    else:
        S = nv.lib().ea_lara_parts(ctypes.byref(geom))
    p_ml = torch.empty((BH, S, C, 4), dtype=torch.float32, device=dev)
    p_acc = torch.empty((4, BH, S, C, d), dtype=torch.float32, device=dev)
    if fused:
        if tokst is None:
            raise RuntimeError("ea_lara_bwd_q_fused needs the forward's per-token statistics (lse_Z, mean t)")
        nv.call("ea_lara_bwd_q_fused", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tdo), nv.ptr(omega),
                nv.ptr(qbar), nv.ptr(kv), nv.ptr(lse_t), nv.ptr(bhv), nv.ptr(cst), nv.ptr(tokst[0]), nv.ptr(tokst[1]),
                ctypes.byref(tdq),
                nv.ptr(p_ml), nv.ptr(p_acc[0]), nv.ptr(p_acc[1]), nv.ptr(p_acc[2]), nv.ptr(p_acc[3]), nv.stream())
    else:
        tok = torch.empty((4, BH, N), dtype=torch.float32, device=dev)
        lseZ, tmean, rowdot, sda = tok[0], tok[1], tok[2], tok[3]
        nv.call("ea_lara_bwd_q", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tdo), nv.ptr(omega),
                nv.ptr(qbar), nv.ptr(kv), nv.ptr(lse_t), nv.ptr(bhv), nv.ptr(cst), ctypes.byref(tdq),
                nv.ptr(lseZ), nv.ptr(tmean), nv.ptr(rowdot), nv.ptr(sda), nv.stream())
        nv.call("ea_lara_bwd_qstats", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tdo),
                nv.ptr(omega), nv.ptr(qbar), nv.ptr(kv), nv.ptr(lse_t), nv.ptr(bhv), nv.ptr(cst),
                nv.ptr(lseZ), nv.ptr(tmean), nv.ptr(rowdot), nv.ptr(sda), nv.ptr(p_ml),
                nv.ptr(p_acc[0]), nv.ptr(p_acc[1]), nv.ptr(p_acc[2]), nv.ptr(p_acc[3]), nv.stream())
    # sums over the slices + derived per-landmark quantities (one tiny kernel)
    big = torch.empty((4, BH, C, d), dtype=torch.float32, device=dev)
    dkv, dom_q, dqbar_m, uq = big[0], big[1], big[2], big[3]
    small = torch.empty((4, BH, C), dtype=torch.float32, device=dev)
    r, dbh, dlp_m, dkk = small[0], small[1], small[2], small[3]
    want_dqbar = mis in (0, 1)
    if fused and lara_fold(C, S):
        # round 5: the key-side pass merges the query side's partials itself (no ea_lara_merge_bwd launch); with want_parts the
        # caller's landmark backward also adds up the key side's d omega partials on load (no ea_slice_sum launch):
        # d omega = scale (dom_q + sum_s p_domk[:, s])
        p_domk = torch.empty((BH, S, C, d), dtype=torch.float32, device=dev)
        nv.call_as("ea_lara_bwd_k_fused", "ea_lara_bwd_k_fused_merge", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8),
                nv.ptr(omega), nv.ptr(qbar), nv.ptr(kv), nv.ptr(lse_k), S, nv.ptr(p_ml), nv.ptr(p_acc[0]), nv.ptr(p_acc[1]),
                nv.ptr(p_acc[2]), nv.ptr(p_acc[3]), ctypes.byref(tdk), ctypes.byref(tdv), nv.ptr(p_domk),
                nv.ptr(dbh) if mis == 0 else None, nv.ptr(dlp_m), nv.ptr(dom_q), nv.ptr(dqbar_m) if want_dqbar else None,
                nv.ptr(uq) if mis == 0 else None, nv.stream())
        d_qbar = dqbar_m if want_dqbar else None
        d_bhv = dbh if mis == 0 else None
        if want_parts:
            return ("parts", dom_q, p_domk, S, float(scale)), d_qbar, d_bhv, dlp_m, (uq if mis == 0 else None)
        d_omega = torch.empty((BH, C, d), dtype=torch.float32, device=dev)
        nv.call("ea_slice_sum", BH, S, C * d, float(scale), nv.ptr(dom_q), nv.ptr(p_domk), nv.ptr(d_omega), nv.stream())
        return d_omega, d_qbar, d_bhv, dlp_m, (uq if mis == 0 else None)
    nv.call("ea_lara_merge_bwd", BH, S, C, d, 1 if mis == 0 else 0, float(scale), nv.ptr(p_ml),
            nv.ptr(p_acc[0]), nv.ptr(p_acc[1]), nv.ptr(p_acc[2]), nv.ptr(p_acc[3]), nv.ptr(kv), nv.ptr(qbar),
            nv.ptr(r), nv.ptr(dbh), nv.ptr(dlp_m), nv.ptr(dkk), nv.ptr(dkv), nv.ptr(dom_q),
            nv.ptr(dqbar_m) if want_dqbar else None, nv.ptr(uq) if mis == 0 else None, nv.stream())
    p_domk = p_acc[1]                                      # (its contents were consumed by the merge)
    if fused:
        nv.call("ea_lara_bwd_k_fused", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8),
                nv.ptr(omega), nv.ptr(dkv), nv.ptr(lse_k), nv.ptr(dkk), nv.ptr(r), ctypes.byref(tdk),
                ctypes.byref(tdv), nv.ptr(p_domk), nv.stream())
    else:
        nv.call("ea_lara_bwd_k", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8),
                nv.ptr(omega), nv.ptr(dkv), nv.ptr(lse_k), nv.ptr(dkk), nv.ptr(r), ctypes.byref(tdk),
                ctypes.byref(tdv), nv.stream())
        nv.call("ea_lara_bwd_kstats", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv),
                nv.ptr(mask_u8), nv.ptr(omega), nv.ptr(dkv), nv.ptr(lse_k), nv.ptr(dkk), nv.ptr(r),
                nv.ptr(p_domk), nv.stream())
    d_omega = torch.empty((BH, C, d), dtype=torch.float32, device=dev)
    nv.call("ea_slice_sum", BH, S, C * d, float(scale), nv.ptr(dom_q), nv.ptr(p_domk), nv.ptr(d_omega), nv.stream())
    d_qbar = dqbar_m if want_dqbar else None
    d_bhv = dbh if mis == 0 else None
    return d_omega, d_qbar, d_bhv, dlp_m, (uq if mis == 0 else None)


def _lara_finish(geom, qkv5, dqkv5, qbar, uq, lse_t, dpq=None, dpk=None, pool=None):
    """dq -= s sum_c t[c,n] (u q_bar)_c and, with pool = (r, H, W), the pooling backward
    dq += dpq[chunk]/r^2, dk += dpk[chunk]/r^2 -- one pass (ea_lara_bwd_finish)."""
    if uq is None and pool is None:
        return
    q, _, _ = _qkv_views(qkv5)
    dq, dk, _ = _qkv_views(dqkv5)
    tq, tdq, tdk = nv.t4(q), nv.t4(dq), nv.t4(dk)
    r, H, W = pool if pool is not None else (0, 0, 0)
    if geom.C <= 64:
        nv.call("ea_lara_bwd_finish", ctypes.byref(geom), ctypes.byref(tq), nv.ptr(qbar), nv.ptr(uq), nv.ptr(lse_t),
                nv.ptr(dpq), nv.ptr(dpk), int(r), int(H), int(W), ctypes.byref(tdq), ctypes.byref(tdk), nv.stream())
        return
    if uq is not None:
        nv.call("ea_lara_bwd_qcorr", ctypes.byref(geom), ctypes.byref(tq), nv.ptr(qbar), nv.ptr(uq),
                nv.ptr(lse_t), ctypes.byref(tdq), nv.stream())
    if pool is not None:
        B, N, _, h, d = qkv5.shape
        pg = nv.make_geom(B, h, N, d, geom.dtype, True, (H, W), r, 0, r, (H // r) * (W // r))
        nv.call("ea_eva_chunk_mean_bwd", ctypes.byref(pg), nv.ptr(dpq), nv.ptr(dpk), None,
                ctypes.byref(tdq), ctypes.byref(tdk), nv.stream())


class LaraAttnFn(torch.autograd.Function):
    """LARA estimator on a fused qkv tensor given the landmark-side tensors (all fp32):
    omega [B,h,C,d], qbar [B,h,C,d] (q_bar rows for mis-opt, mu rows for mis-biased; rows already
    repeated for antithetic / multi-sample noise), bhv [B,h,C] balanced-heuristic weights and
    lp [B,h,C] log-proposal.  Returns out [B,N,h,d]."""

    @staticmethod
    def forward(ctx, qkv5, mask_u8, omega, qbar, bhv, lp, mis, kappa, slot=None):
        nv.require_cuda(qkv5, "qkv")
        B, N, _, h, d = qkv5.shape
        C = omega.shape[2]
        ctx.slot = slot
        geom = nv.ea_lara_geom(B, h, N, d, nv.io_dtype(qkv5), C, mis, float(kappa), float(d) ** -0.5)
        BH = B * h
        omega = omega.float().reshape(BH, C, d).contiguous()
        qbar_c = None if qbar is None else qbar.float().reshape(BH, C, d).contiguous()
        lp_c = lp.reshape(BH, C).float().contiguous()
        bhv_c = None if bhv is None else bhv.reshape(BH, C).float().contiguous()
        out, (cst, kv, lse_k, lse_t, tokst) = _lara_fwd_core(geom, qkv5, mask_u8, omega, qbar_c, bhv_c, lp_c)
        ctx.save_for_backward(qkv5, mask_u8, omega, qbar_c, bhv_c, cst, kv, lse_k, lse_t, tokst)
        ctx.geom = geom
        ctx.has = (qbar is not None, bhv is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv5, mask_u8, omega, qbar, bhv, cst, kv, lse_k, lse_t, tokst = ctx.saved_tensors
        geom = ctx.geom
        B, N, _, h, d = qkv5.shape
        C = geom.C
        dout = dout.contiguous()
        dqkv5 = torch.empty_like(qkv5)
        d_omega, d_qbar, d_bhv, d_lp, uq = _lara_bwd_core(geom, qkv5, mask_u8, dout, dqkv5, omega, qbar, bhv,
                                                          cst, kv, lse_k, lse_t, tokst)
        slot = ctx.slot
        if slot is not None and slot.defer_fin and uq is not None and C <= 64 and d == 64:
            slot.fin = (qbar, uq, lse_t, C, float(d) ** -0.5)
        else:
            _lara_finish(geom, qkv5, dqkv5, qbar, uq, lse_t)
        has_qbar, has_bhv = ctx.has
        if ctx.slot is not None:
            ctx.slot.buf = dqkv5          # the pooling backward accumulates into this buffer in place
        return (dqkv5, None, d_omega.view(B, h, C, d),
                d_qbar.view(B, h, C, d) if (has_qbar and d_qbar is not None) else None,
                d_bhv.reshape(B, h, C) if (has_bhv and d_bhv is not None) else None,
                d_lp.view(B, h, C), None, None, None)


class LaraCfg(typing.NamedTuple):
    """The 2-D pooled LARA core's configuration (plain values, hashable): r x r pooling of an H x W grid, the generator
    networks, the MIS flavour (MIS), duplicated samples, kappa = alpha_coeff.  lists() / from_lists() are the ONE encoder and decoder
    of the int[] / float[] arguments of torch.ops.ea.lara_fwd / lara_bwd:
    icfg = [H, W, r, has_mlp, mixed, mis, dup(, keep_for_backward = 1)], fcfg = [kappa, scale]."""
    H: int
    W: int
    r: int
    has_mlp: bool
    mixed: bool
    mis: int
    dup: int
    kappa: float
    scale: float

    @property
    def L(self):
        return (self.H // self.r) * (self.W // self.r)

    @property
    def C(self):
        return self.L * (2 if self.dup else 1)

    def lists(self, need_grad):
        return ([int(self.H), int(self.W), int(self.r), int(bool(self.has_mlp)), int(bool(self.mixed)), int(self.mis), int(self.dup),
                 int(bool(need_grad))], [float(self.kappa), float(self.scale)])

    @classmethod
    def from_lists(cls, icfg, fcfg):
        """-> (cfg, need_grad); an absent trailing entry means keep for backward."""
        H, W, r, has_mlp, mixed, mis, dup, *keep = [int(v) for v in icfg]
        kappa, scale = [float(v) for v in fcfg]
        return cls(H, W, r, has_mlp, mixed, mis, dup, kappa, scale), not keep or bool(keep[0])


def _lara_cfg(qkv5, cfg):
    """-> the pooling's ea_geom, the landmark pipeline's ea_lmk_geom, the estimator's ea_lara_geom."""
    B, N, _, h, d = qkv5.shape
    io = nv.io_dtype(qkv5)
    pgeom = nv.make_geom(B, h, N, d, io, True, (cfg.H, cfg.W), cfg.r, 0, cfg.r, cfg.L)
    lg = nv.ea_lmk_geom(B * h, cfg.L, cfg.C, d, cfg.has_mlp, cfg.mixed, cfg.mis, cfg.dup, cfg.scale, 0)
    geom = nv.ea_lara_geom(B, h, N, d, io, cfg.C, cfg.mis, cfg.kappa, cfg.scale)
    return pgeom, lg, geom


def _lara_layer_plan(qkv5, cfg):
    """ea_lara_layer of the composite entry points, or None when the geometry needs the step-by-step path (C > 64)."""
    B, N, _, h, d = qkv5.shape
    return _lara_layer_cfg_dims(B, h, d, nv.io_dtype(qkv5), cfg)


def _lara_layer_cfg(qkv5, icfg, fcfg):
    """_lara_layer_plan of an op call's lists (the suite drives the C entries with them)."""
    return _lara_layer_plan(qkv5, LaraCfg.from_lists(icfg, fcfg)[0])


_LARA_LAYER_CFG = {}


def _lara_layer_cfg_dims(B, h, d, io, cfg):
    """(ea_lara_layer, ea_lara_layer_sizes: the workspace plan, read by field name) or (None, None) -- a pure function of the
    geometry, memoised (a host call per query otherwise, twice per eager step)."""
    key = (B, h, d, io, cfg)
    hit = _LARA_LAYER_CFG.get(key)
    if hit is None:
        lcfg = nv.ea_lara_layer(B, h, d, io, cfg.H, cfg.W, cfg.r, cfg.has_mlp, cfg.mixed, cfg.mis, cfg.dup, cfg.kappa, cfg.scale)
        sizes = nv.ea_lara_layer_sizes()
        hit = (lcfg, sizes) if nv.lib().ea_lara_layer_plan(ctypes.byref(lcfg), ctypes.byref(sizes)) == 0 else (None, None)
        if len(_LARA_LAYER_CFG) < 256:
            _LARA_LAYER_CFG[key] = hit
    return hit


def _lara_use_composite():
    """The FORWARD's decision between the composite entry and the step-by-step launches (per-kernel timing -- bench.py's
    instrumented pass -- needs the individual entry points).  The backward never re-takes it: it follows what the forward
    saved (one workspace tensor = composite), so flipping the switch or the timer between the two cannot desynchronise them."""
    return os.environ.get("EA_LARA_COMPOSITE", "1") == "1" and not nv.KERNEL_TIMER.enabled


def _param_ptrs(ps):
    """const float* const params[8] for the composite entry points (kept alive by the caller)."""
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ps])
    return arr


def _lara_saved_is_composite(saved_list):
    """ONE tensor after `out` = lara_fwd_impl (just below) ran a composite entry: the count crosses save_for_backward and the dispatcher."""
    return len(saved_list) == 1


def lara_fwd_impl(qkv5, mask_u8, noise, icfg, fcfg, params, pooled=None, proj=None):
    """torch.ops.ea.lara_fwd: uniform r x r pooling of q, k -> fused landmark pipeline -> estimator.
    icfg, fcfg: a LaraCfg and the keep-for-backward flag as LaraCfg.lists() encodes them; params = (Wq, bq, gq, cq, Wk, bk,
    gk, ck) when has_mlp.
    C <= 64: ONE composite C-ABI call (ea_lara_layer_fwd) on two workspaces -> [out, saved workspace].
    Otherwise the step-by-step launch sequence -> [out, omega, qrows, bhv, cst, kv, lse_k, lse_t, pq, pk, noise, lmk_saved, tokst]
    (absent tensors are empty).
    pooled (direct calls only, never through the dispatcher): a Pooled -- the pooled q / k rows already computed by the
    projection kernel, inside the composite workspace or as two tensors: the pooling pass is skipped.
    proj (direct calls only) = [w16p, bias32, y2]: the output projection y2 [B*N, h*d] = out w16p^T + bias is written by the
    combine pass (ea_lara_layer_fwd_proj / ea_lara_out_proj_fwd_merge); where the library declines, by ea_linear after it."""
    global LAST_LMK_GEOM
    nv.require_cuda(qkv5, "qkv")
    cfg, need_grad = LaraCfg.from_lists(icfg, fcfg)
    lcfg, sizes = _lara_layer_plan(qkv5, cfg) if _lara_use_composite() else (None, None)
    if pooled is not None and (pooled.ws is not None) != (lcfg is not None):
        raise RuntimeError("lara_fwd: pooled rows prepared for the other launch path")
    B, N, _, h, d = qkv5.shape
    BH, dev = B * h, qkv5.device
    if lcfg is not None:
        q, k, v = _qkv_views(qkv5)
        tq, tk, tv = nv.t4(q), nv.t4(k), nv.t4(v)
        ws = pooled.ws if pooled is not None else torch.empty(sizes.n_saved, dtype=torch.float32, device=dev)
        tmp = torch.empty(sizes.n_fwd_tmp, dtype=torch.float32, device=dev)
        out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=dev)
        to = nv.t4(out.permute(0, 2, 1, 3))
        noise_c = None if noise is None else noise.float().contiguous()
        ps = [_f32c(t) for t in params]
        pp = _param_ptrs(ps) if ps else None
        LAST_LMK_GEOM = (B * h, cfg.L, cfg.C, d, cfg.has_mlp, cfg.mixed, 0)
        keep = int(need_grad) | (2 if pooled is not None else 0)
        if proj is not None and nv.call_probe("ea_lara_layer_fwd_proj", "ea_lara_layer_fwd_proj", ctypes.byref(lcfg), ctypes.byref(tq),
                                              ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8), nv.ptr(noise_c), pp, ctypes.byref(to),
                                              nv.ptr(ws), nv.ptr(tmp), keep, nv.ptr(proj[0]), nv.ptr(proj[1]), nv.ptr(proj[2]),
                                              proj[2].stride(0), nv.stream()):
            return [out, ws]                              # composite: _lara_saved_is_composite
        nv.call("ea_lara_layer_fwd", ctypes.byref(lcfg), ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv),
                nv.ptr(mask_u8), nv.ptr(noise_c), pp, ctypes.byref(to), nv.ptr(ws), nv.ptr(tmp), keep, nv.stream())
        if proj is not None:
            _lara_proj_fallback(out, proj)
        return [out, ws]
    pgeom, lg, geom = _lara_cfg(qkv5, cfg)
    L, C, has_mlp, mis = cfg.L, cfg.C, cfg.has_mlp, cfg.mis
    q, k, _ = _qkv_views(qkv5)
    tq, tk = nv.t4(q), nv.t4(k)
    if pooled is not None:
        pq, pk = pooled.pq.view(BH, L, d), pooled.pk.view(BH, L, d)
    else:
        pq = torch.empty((BH, L, d), dtype=torch.float32, device=dev)
        pk = torch.empty_like(pq)
        nv.call("ea_eva_chunk_mean_fwd", ctypes.byref(pgeom), ctypes.byref(tq), ctypes.byref(tk), None,
                nv.ptr(pq), nv.ptr(pk), nv.stream())
    noise_c = None if noise is None else noise.float().contiguous()
    ps = [_f32c(t) for t in params]
    LAST_LMK_GEOM = (BH, L, C, d, has_mlp, cfg.mixed, 0)
    omega = torch.empty((BH, C, d), dtype=torch.float32, device=dev)
    qrows = torch.empty_like(omega) if mis != 2 else None
    bhv = torch.empty((BH, C), dtype=torch.float32, device=dev) if mis == 0 else None
    lp = torch.empty((BH, C), dtype=torch.float32, device=dev)
    pp = [nv.ptr(t) for t in ps] if has_mlp else [None] * 8
    saved = _lmk_saved(lg, dev) if need_grad else None
    nv.call("ea_lara_landmarks_fwd", ctypes.byref(lg), nv.ptr(pq), nv.ptr(pk), *pp, nv.ptr(noise_c),
            nv.ptr(omega), nv.ptr(qrows), nv.ptr(bhv), nv.ptr(lp), nv.ptr(saved), nv.stream())
    out, (cst, kv, lse_k, lse_t, tokst) = _lara_fwd_core(geom, qkv5, mask_u8, omega, qrows, bhv, lp, need_grad, proj=proj)
    e = lp
    return [out, omega, _e(qrows, e), _e(bhv, e), cst, kv, lse_k, _e(lse_t, e), pq, pk, _e(saved, e), _e(tokst, e)]


def lara_bwd_impl(dout, qkv5, mask_u8, noise, saved_list, icfg, fcfg, params):
    """torch.ops.ea.lara_bwd -> [dqkv, *parameter gradients (fp32, in the order of params)].  saved_list is what lara_fwd
    returned after `out`: the composite workspace (one tensor -> ea_lara_layer_bwd) or the step-by-step tensors."""
    g = _lara_backward(dout, qkv5, mask_u8, noise, saved_list, LaraCfg.from_lists(icfg, fcfg)[0], params)
    return [g.dqkv] + g.params


def _lara_backward(dout, qkv5, mask_u8, noise, saved_list, cfg, params, defer_param_sums=False, defer_finish=False):
    """The 2-D pooled LARA core's backward -> CoreGrads (dbias: None).  defer_param_sums: the per-(b,h) partials of the generator
    parameters' gradients wait for the caller's terminal sum; defer_finish (C <= 64, round 5): ea_linear_dgrad_finish applies the
    softmax-over-sequence correction of dq and the pooling terms of dq / dk on its way through the gradient rows."""
    B, N, _, h, d = qkv5.shape
    BH, dev = B * h, qkv5.device
    noise_c = None if noise is None else noise.float().contiguous()
    ps = [_f32c(t) for t in params]
    dqkv5 = torch.empty_like(qkv5)
    if _lara_saved_is_composite(saved_list):
        lcfg, sizes = _lara_layer_plan(qkv5, cfg)                # pure geometry / size query: valid whenever the forward's was
        if lcfg is None:
            raise RuntimeError("lara_bwd: a composite workspace was saved for a geometry ea_lara_layer_plan rejects")
        ws = saved_list[0]
        dout = _rows_contiguous(dout)
        q, k, v = _qkv_views(qkv5)
        dq, dk, dv = _qkv_views(dqkv5)
        ts = [nv.t4(t) for t in (q, k, v, dout.permute(0, 2, 1, 3), dq, dk, dv)]
        tmp = torch.empty(sizes.n_bwd_tmp, dtype=torch.float32, device=dev)
        pp = _param_ptrs(ps) if ps else None
        defer = bool(defer_param_sums and ps)
        dpar = torch.empty(2 * d * d + 6 * d, dtype=torch.float32, device=dev) if (ps and not defer) else None
        nv.call("ea_lara_layer_bwd", ctypes.byref(lcfg), ctypes.byref(ts[0]), ctypes.byref(ts[1]), ctypes.byref(ts[2]),
                nv.ptr(mask_u8), nv.ptr(noise_c), pp, ctypes.byref(ts[3]), ctypes.byref(ts[4]), ctypes.byref(ts[5]),
                ctypes.byref(ts[6]), nv.ptr(ws), nv.ptr(tmp), nv.ptr(dpar), 1 if defer_finish else 0, nv.stream())
        fin = None
        if defer_finish:
            L, C = cfg.L, cfg.C
            fin = Finish(B=B, gh=cfg.H, gw=cfg.W, r=cfg.r, C=C, scale=float(lcfg.scale),
                         dpq=_ws_rows(tmp, sizes.bwd_dpq, BH * L * d), dpk=_ws_rows(tmp, sizes.bwd_dpk, BH * L * d))
            if cfg.mis == 0:
                fin = fin._replace(uq=_ws_rows(tmp, sizes.bwd_uq, BH * C * d), qbar=_ws_rows(ws, sizes.saved_qrows, BH * C * d),
                                   lse_t=_ws_rows(ws, sizes.saved_lse_t, BH * C))
        if defer:                      # the per-(b,h) partials, still to be added up: [B*h, 2 d d], [B*h, 6 d]
            parts = _param_partials(_ws_rows(tmp, sizes.bwd_dW, BH, 2 * d * d), _ws_rows(tmp, sizes.bwd_dvec, BH, 6 * d))
            return CoreGrads(dqkv5, None, None, parts, fin)
        return CoreGrads(dqkv5, None, _mlp_grads(dpar[:2 * d * d], dpar[2 * d * d:], d) if ps else [], (), fin)
    pgeom, lg, geom = _lara_cfg(qkv5, cfg)
    has_mlp = cfg.has_mlp
    if defer_finish and cfg.C > 64:
        raise RuntimeError("lara_bwd: defer_finish needs C <= 64 samples")
    omega, qrows, bhv, cst, kv, lse_k, lse_t, pq, pk, saved, tokst = [_opt(t) for t in saved_list]
    dout = dout.contiguous()
    d_omega, d_qrows, d_bhv, d_lp, uq = _lara_bwd_core(geom, qkv5, mask_u8, dout, dqkv5, omega, qrows, bhv,
                                                       cst, kv, lse_k, lse_t, tokst, want_parts=True)
    dpq = torch.empty_like(pq)
    dpk = torch.empty_like(pk)
    dW = dvec = None
    if has_mlp:
        dW = torch.empty((BH, 2, d, d), dtype=torch.float32, device=dev)
        dvec = torch.empty((BH, 2, 3, d), dtype=torch.float32, device=dev)
    pp = [nv.ptr(t) for t in ps] if has_mlp else [None] * 8
    if isinstance(d_omega, tuple):
        _, dom_q, p_domk, S_, scale_ = d_omega
        nv.call_as("ea_lara_landmarks_bwd", "ea_lara_landmarks_bwd_parts", ctypes.byref(lg), nv.ptr(pq), nv.ptr(pk), *pp, nv.ptr(noise_c),
                nv.ptr(dom_q), S_, nv.ptr(p_domk), scale_, nv.ptr(d_qrows), nv.ptr(d_bhv), nv.ptr(d_lp), nv.ptr(dpq),
                nv.ptr(dpk), nv.ptr(dW), nv.ptr(dvec), nv.ptr(saved), nv.stream())
    else:
        nv.call("ea_lara_landmarks_bwd", ctypes.byref(lg), nv.ptr(pq), nv.ptr(pk), *pp, nv.ptr(noise_c),
                nv.ptr(d_omega), nv.ptr(d_qrows), nv.ptr(d_bhv), nv.ptr(d_lp), nv.ptr(dpq), nv.ptr(dpk),
                nv.ptr(dW), nv.ptr(dvec), nv.ptr(saved), nv.stream())
    fin = None
    if defer_finish:
        fin = Finish(B=B, gh=cfg.H, gw=cfg.W, r=cfg.r, C=cfg.C, scale=cfg.scale, dpq=dpq, dpk=dpk)
        if uq is not None:
            fin = fin._replace(uq=uq, qbar=qrows, lse_t=lse_t)
    else:
        _lara_finish(geom, qkv5, dqkv5, qrows, uq, lse_t, dpq, dpk, (cfg.r, cfg.H, cfg.W))
    if has_mlp and defer_param_sums:
        return CoreGrads(dqkv5, None, None, _param_partials(dW.view(BH, -1), dvec.view(BH, -1)), fin)
    return CoreGrads(dqkv5, None, _mlp_grads(*colsum2_f32(dW.view(BH, -1), dvec.view(BH, -1)), d) if has_mlp else [], (), fin)


class LaraPooledFn(torch.autograd.Function):
    """The whole 2-D LARA core as ONE autograd node (no gradient side channels between nodes): uniform
    r x r average pooling of q, k (lara.py:43,48,145-151) -> fused landmark pipeline (:45-54,157-198,
    214-238) -> estimator (:201-246), through the dispatcher ops torch.ops.ea.lara_fwd / lara_bwd.
    cfg: a LaraCfg; params = (Wq, bq, gq, cq, Wk, bk, gk, ck) when has_mlp.  Returns out [B,N,h,d].
    Backward: one fused pass per side, the landmark backward, and ONE finish pass that applies the
    softmax-over-sequence correction of dq together with the pooling backward of dq and dk."""

    @staticmethod
    def forward(ctx, qkv5, mask_u8, noise, cfg, *params):
        ctx.lists = cfg.lists(any(ctx.needs_input_grad))
        outs = _ea_op("lara_fwd", lara_fwd_impl, qkv5, mask_u8, noise, *ctx.lists, list(params))
        ctx.save_for_backward(qkv5, mask_u8, noise, *outs[1:], *params)
        ctx.nsaved = len(outs) - 1
        ctx.pdtypes = [t.dtype for t in params]
        return outs[0]

    @staticmethod
    def backward(ctx, dout):
        qkv5, mask_u8, noise, *rest = ctx.saved_tensors
        saved, params = rest[:ctx.nsaved], rest[ctx.nsaved:]
        grads = _ea_op("lara_bwd", lara_bwd_impl, dout, qkv5, mask_u8, noise, list(saved), *ctx.lists, list(params))
        pgrads = [g.to(dt) for g, dt in zip(grads[1:], ctx.pdtypes)]
        return (grads[0], None, None, None) + tuple(pgrads)


USE_PROJ_POOL = os.environ.get("EA_PROJ_POOL", "1") == "1"
USE_MULTI_SUM = os.environ.get("EA_MULTI_SUM", "1") == "1"


def proj_pool_supported(x2, w32, cdtype, B, H, W, r, heads):
    """ea_linear_w32_pool: the qkv projection of a 192-wide three-head model that also emits the r x r pooled q / k rows."""
    C = x2.shape[1]
    return (USE_PROJ_POOL and heads == 3 and C == 192 and tuple(w32.shape) == (576, 192) and w32.dtype == torch.float32
            and x2.shape[0] == B * H * W and x2.is_contiguous()
            and bool(nv.lib().ea_linear_pool_supported(192, 576, B, H, W, r)))


def project_qkv_pooled(x2, wq, bq32, cdtype, want_cast, B, H, W, r, pq, pk, w_cast=None):
    """qkv = x2 @ wq.T + bq in `cdtype` with the means of the rounded q / k rows over the r x r cells written to pq / pk
    (fp32 [B*3, L, 64]) by the same kernel (ea_linear_w32_pool) -> (y [rows, 576], rounded copy of an fp32 x2 or None).
    w_cast: a [576, 192] `cdtype` tensor that receives the rounded weight (for the backward's input-gradient GEMM), or None."""
    rows, K = x2.shape
    a_f32 = x2.dtype == torch.float32
    y = torch.empty((rows, 576), dtype=cdtype, device=x2.device)
    a_cast = torch.empty((rows, K), dtype=cdtype, device=x2.device) if (a_f32 and want_cast) else None
    label = "ea_linear_w32_pool"
    if nv.KERNEL_TIMER.enabled:
        label = "ea_linear[192->576,%s->16,+pool]" % ("f32" if a_f32 else "16")
        _note_bytes(label, rows * (K * x2.element_size() + 576 * 2 + (K * 2 if a_cast is not None else 0)))
    nv.call_as(label, "ea_linear_w32_pool", _ELEM[cdtype], B, H, W, r, K, 576, nv.ptr(x2), int(a_f32), x2.stride(0), nv.ptr(wq),
               nv.ptr(bq32), nv.ptr(y), 576, nv.ptr(a_cast), nv.ptr(pq), nv.ptr(pk), nv.ptr(w_cast), nv.stream())
    return y, a_cast


USE_W192 = os.environ.get("EA_W192_PREPARE", "1") == "1"


def w192_usable(wq, wp, cdtype):
    """The prepared-weight flavour of a 192-wide layer's projections (round 6): fp32 master weights [576, 192] / [192, 192] of
    a direct (untraced) call."""
    return (USE_W192 and _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0
            and cdtype in _ELEM and wq.is_cuda and wq.dtype == torch.float32 and wp.dtype == torch.float32
            and tuple(wq.shape) == (576, 192) and tuple(wp.shape) == (192, 192) and wq.is_contiguous() and wp.is_contiguous()
            and (wq.storage_offset() * 4) % 16 == 0 and (wp.storage_offset() * 4) % 16 == 0)


def prepare_w192(wq, wp, cdtype):
    """(w16q [576, 192], wq_sw, w16p [192, 192], w16p^T) in `cdtype`, ONE launch (ea_linear_w192_prepare): the rounded qkv weight
    for the input-gradient kernels, the same values in the staging order of the register-resident projection kernel, the
    rounded output-projection weight and its transpose (its input gradient through the same streaming kernel).  The kernels
    fed by the fp32 master weights pull twice the bytes through every CU's L2 port before their first tile: 13 us of the
    pooled projection at any row count (workgroup timelines of round 6)."""
    return _prepare_w192(wq, wp, cdtype, False)


def prepare_w192_t(wq, wp, cdtype):
    """prepare_w192 with a fifth image from the same launch (ea_linear_w192_prepare_t): wqT_sw, the bits of w16q in the order the
    input-gradient kernels hold W^T in registers -- 16-byte piece (wave, ks, lane = 16 g + li) = wq[32 ks + 8 g .. + 7, 16 wave + li]
    -- which qkv_dgrad / qkv_dgrad_finish load directly instead of transposing w16q through LDS at the start of every launch."""
    return _prepare_w192(wq, wp, cdtype, True)


# The 192 -> 192 products of a prepared layer (output projection, its input gradient) on the register-resident kernel
# (ea_linear_rs192); EA_LIN_RS192=0 (dev switch) keeps them on ea_linear and the prepare launch at five images.
USE_LIN_RS192 = os.environ.get("EA_LIN_RS192", "1") == "1"


def prepare_w192_rs(wq, wp, cdtype):
    """prepare_w192_t with two more images from the same launch (ea_linear_w192_prepare_rs): W_proj and W_proj^T -- the bits of
    w16p and w16pT -- in the register order of ea_linear_rs192: 16-byte piece ((pair * 2 + j) * 6 + ks) * 64 + 16 g + li =
    W[32 pair + 8 (li >> 2) + (li & 3) + 4 j, 32 ks + 8 g .. + 7].  With EA_LIN_RS192=0 the two are None (prepare_w192_t's launch)."""
    if not USE_LIN_RS192:
        return _prepare_w192(wq, wp, cdtype, True) + (None, None)
    dev = wq.device
    w16q = torch.empty((576, 192), dtype=cdtype, device=dev)
    wsw = torch.empty((576 * 192,), dtype=cdtype, device=dev)
    wtsw = torch.empty((576 * 192,), dtype=cdtype, device=dev)
    w16p, w16pT, wp_rs, wpT_rs = torch.empty((4, 192, 192), dtype=cdtype, device=dev).unbind(0)
    nv.call("ea_linear_w192_prepare_rs", _ELEM[cdtype], nv.ptr(wq.detach()), nv.ptr(wp.detach()), nv.ptr(w16q), nv.ptr(wsw),
            nv.ptr(w16p), nv.ptr(w16pT), nv.ptr(wtsw), nv.ptr(wp_rs), nv.ptr(wpT_rs), nv.stream())
    return w16q, wsw, w16p, w16pT, wtsw, wp_rs.view(-1), wpT_rs.view(-1)


def _rs192_rows_ok(a2, cdtype):
    """What ea_linear_rs192 serves: _lin_rows_ok rows of the compute dtype, 192 wide, with a row stride of at least 192 (a
    broadcast row, stride 0, passes _lin_rows_ok and stays on ea_linear)."""
    return a2.dtype == cdtype and _lin_rows_ok(a2, cdtype) and a2.shape[1] == 192 and a2.stride(0) >= 192


def linear_rs192(a2, image, bias32, cdtype):
    """y = a2 @ W.T (+ bias) at 192 -> 192 from an image of prepare_w192_rs: the weight resident in registers (ea_linear_rs192),
    ea_linear's bits.  a2 [rows, 192] in cdtype as _rs192_rows_ok asks."""
    rows = a2.shape[0]
    y = torch.empty((rows, 192), dtype=cdtype, device=a2.device)
    label = "ea_linear_rs192"
    if nv.KERNEL_TIMER.enabled:
        label = "ea_linear_rs192[192->192,16->16]"
        _note_bytes(label, rows * (192 * 2 + 192 * 2))
    nv.call_as(label, "ea_linear_rs192", _ELEM[cdtype], nv.ptr(a2), a2.stride(0), nv.ptr(image), nv.ptr(bias32), nv.ptr(y), 192,
               rows, nv.stream())
    return y


def _prepare_w192(wq, wp, cdtype, with_t):
    dev = wq.device
    w16q = torch.empty((576, 192), dtype=cdtype, device=dev)
    wsw = torch.empty((576 * 192,), dtype=cdtype, device=dev)
    w16p = torch.empty((192, 192), dtype=cdtype, device=dev)
    w16pT = torch.empty((192, 192), dtype=cdtype, device=dev)
    if not with_t:
        nv.call("ea_linear_w192_prepare", _ELEM[cdtype], nv.ptr(wq.detach()), nv.ptr(wp.detach()), nv.ptr(w16q), nv.ptr(wsw),
                nv.ptr(w16p), nv.ptr(w16pT), nv.stream())
        return w16q, wsw, w16p, w16pT
    wtsw = torch.empty((576 * 192,), dtype=cdtype, device=dev)
    nv.call("ea_linear_w192_prepare_t", _ELEM[cdtype], nv.ptr(wq.detach()), nv.ptr(wp.detach()), nv.ptr(w16q), nv.ptr(wsw),
            nv.ptr(w16p), nv.ptr(w16pT), nv.ptr(wtsw), nv.stream())
    return w16q, wsw, w16p, w16pT, wtsw


def project_qkv_wsw(x2, wsw, w16q, bq32, cdtype, want_cast, grid=None, pq=None, pk=None):
    """qkv = x2 @ wq.T + bq from the prepared weight: the register-resident kernel (ea_linear_wsw; with grid = (B, H, W, r) the
    pooled q / k rows leave with it as from project_qkv_pooled) from 65 536 rows on or whenever the pooled rows are wanted, the
    LDS-resident streaming kernel on the rounded weight below that -> (y [rows, 576], rounded copy of an fp32 x2 or None)."""
    rows, K = x2.shape
    a_f32 = x2.dtype == torch.float32
    if grid is None and rows < 65536:
        y, ac = ea_linear(x2, w16q, bq32, cdtype, want_cast)
        return y, ac
    y = torch.empty((rows, 576), dtype=cdtype, device=x2.device)
    a_cast = torch.empty((rows, K), dtype=cdtype, device=x2.device) if (a_f32 and want_cast) else None
    B, H, W, r = grid if grid is not None else (0, 0, 0, 0)
    label = "ea_linear_wsw"
    if nv.KERNEL_TIMER.enabled:
        label = "ea_linear[192->576,%s->16%s]" % ("f32" if a_f32 else "16", ",+pool" if grid is not None else "")
        _note_bytes(label, rows * (K * x2.element_size() + 576 * 2 + (K * 2 if a_cast is not None else 0)))
    nv.call_as(label, "ea_linear_wsw", _ELEM[cdtype], rows, B, H, W, r, nv.ptr(x2), int(a_f32), x2.stride(0), nv.ptr(wsw),
               nv.ptr(bq32), nv.ptr(y), 576, nv.ptr(a_cast), nv.ptr(pq), nv.ptr(pk), nv.stream())
    return y, a_cast


USE_CORE_MODULE_FN = os.environ.get("EA_CORE_MODULE_FN", "1") == "1"


class Core:
    """What CoreModuleFn asks of a core spec, the holder of a core's non-differentiable state.  A spec defines fwd and bwd; the
    other methods default to "nothing to do" / "declined".  `inputs` are the core's differentiable inputs."""

    def setup(self, B, N, heads, d, elem, inputs, need_grad):
        """Before anything is launched: geometry, derived inputs."""

    def project(self, x2, wq, bq32, cdtype, want, need_dx, w192):
        """The qkv projection by a kernel that also emits the core's pooled q / k rows (direct calls only)
        -> (y, rounded x | None, rounded qkv weight | None), or None to decline."""
        return None

    def fwd(self, qkv5, inputs):
        """-> out [B,N,h,d], tensors to save."""
        raise NotImplementedError

    def fwd_project(self, qkv5, inputs, w16p, bp32, cdtype):
        """fwd with the output projection y2 = out w16p^T + bias formed by the core's last pass (direct calls with the prepared
        192-wide weights only) -> (out, y2, saved), or None -- before anything is launched or consumed -- to decline."""
        return None

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        """-> d qkv5, gradients of `inputs`, partials, fin.  partials: (key, [S, n] fp32, meta) entries for the terminal sum
        (only when `defer`), else (); fin = (Finish, qkv rows | None) leaves the core's last correction of dq / dk to the
        input-gradient kernel (qkv_dgrad_finish; only when fin_ok), else None."""
        raise NotImplementedError

    def scatter(self, sums, grads):
        """After the terminal sum; sums: key -> (summed partial, meta) -> gradients of `inputs`."""
        return grads


class SoftmaxCore(Core):
    """Core spec of CoreModuleFn (protocol: Core): dropout(softmax(s QK^T)) V (softmax_fwd_impl / softmax_bwd_impl)."""

    def __init__(self, mask_u8, keep=None, keep_scale=1.0):
        self.mask_u8, self.keep, self.keep_scale = mask_u8, keep, float(keep_scale)

    def fwd(self, qkv5, inputs):
        out, lse = softmax_fwd_impl(qkv5, self.mask_u8, self.keep, self.keep_scale)
        return out, (lse,)

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        return softmax_bwd_impl(dout, qkv5, self.mask_u8, out, saved[0], self.keep, self.keep_scale), (), (), None


class LocalCore(Core):
    """Core spec of CoreModuleFn: per-window softmax attention with the dense per-head bias (local_fwd_impl / local_bwd_impl);
    its one differentiable input is the bias [h, Wq, Wk] (or None)."""

    def __init__(self, mask_u8, attn_2d, seq_shape, window, ext, tb=None):
        self.mask_u8, self.geo = mask_u8, _geo(attn_2d, seq_shape, window, ext)
        self.bias_cols = 0
        self.tb = tb                                   # TableBias: the differentiable input is then the TABLE [rows, h]

    def fwd(self, qkv5, inputs):
        bias = inputs[0]
        if self.tb is not None and bias is not None:
            B, N, _, h, d = qkv5.shape
            a2, s0, s1, window, ext = self.geo
            bias = self.tb.dense(bias, self.tb.ld(B, h, N, d, nv.io_dtype(qkv5), bool(a2), (s0, s1) if a2 else (s0,), window, ext))
        self.bias_cols = 0 if bias is None else bias.shape[-1]
        out, lse, bias_p = local_fwd_impl(qkv5, bias, self.mask_u8, self.geo)
        return out, (lse, bias_p)

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        dqkv5, dbias = local_bwd_impl(dout, None, qkv5, _opt(saved[1]), self.mask_u8, out, saved[0], self.geo, self.bias_cols)
        dbias = _opt(dbias)
        if self.tb is not None and dbias is not None:
            dbias = self.tb.grad(dbias)
        return dqkv5, (dbias,), (), None


class PerformerCore(Core):
    """Core spec of CoreModuleFn: the Performer core in exact fp32 arithmetic on the 16-bit qkv of an autocast step
    (performer_f32_fwd / performer_f32_bwd); the random features W [h, m, d] carry no gradient."""

    def __init__(self, mask_u8, W):
        self.mask_u8, self.W = mask_u8, W

    def fwd(self, qkv5, inputs):
        out, p_max, kv, ksum = performer_f32_fwd(qkv5, self.mask_u8, self.W)
        return out, (p_max, kv, ksum)

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        return performer_f32_bwd(dout, qkv5, self.mask_u8, self.W, saved[0], saved[1], saved[2]), (), (), None


USE_LARA_1D_MODULE_FN = os.environ.get("EA_LARA_1D_MODULE_FN", "1") == "1"
USE_CAUSAL_MODULE_FN = os.environ.get("EA_CAUSAL_MODULE_FN", "1") == "1"
EVA_1D_NO_MASK = os.environ.get("EA_EVA_1D_NO_MASK", "1") == "1"            # dev switch: 1-D EVA builds no all-false mask
USE_GRAPH_CORE = os.environ.get("EA_GRAPH_CORE", "1") == "1"                # opt-in subclasses of MultiheadAttention (RA, ScatterBrain)


class GraphCore(Core):
    """Core spec of CoreModuleFn for a core that is itself a small autograd graph -- LinearRA 'adaptive-1d': segment kernels ->
    landmark kernels -> estimator, three Functions with hand-overs between them (_GradSlot).  fwd() builds that graph on a
    detached qkv with autograd switched back on (a Function's forward runs without it), bwd() differentiates it with
    torch.autograd.grad: the launches are exactly those of the three-node module, but the two projections around them now
    share CoreModuleFn's backward -- both weight gradients in one launch (ea_wgrad_pair) and one terminal ea_multi_sum instead of
    two ea_wgrad + two ea_part_sum (cfg5 LARA at the recipe's batch of one: 28 launches of ~10 us each, profiles/
    r06_step_trace_cfg5_lara_b1.txt).  fn(qkv5, *inputs) -> out [B,N,h,d]; the differentiable inputs are its parameters."""

    def __init__(self, fn, need_grad):
        self.fn, self.need_grad = fn, bool(need_grad)
        self.leaf = self.out = self.inputs = None

    def fwd(self, qkv5, inputs):
        if not self.need_grad:
            return self.fn(qkv5, *inputs), ()
        with torch.enable_grad():
            leaf = qkv5.detach().requires_grad_(True)
            out = self.fn(leaf, *inputs)
        self.leaf, self.out, self.inputs = leaf, out, list(inputs)
        return out.detach(), ()

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        if self.out is None:
            raise RuntimeError("GraphCore: backward without a recorded forward (or a second backward through it)")
        idx = [i for i, t in enumerate(self.inputs) if t is not None and t.requires_grad]
        g = torch.autograd.grad(self.out, [self.leaf] + [self.inputs[i] for i in idx], dout.to(self.out.dtype),
                                allow_unused=True)
        extra = [None] * len(self.inputs)
        for i, gi in zip(idx, g[1:]):
            extra[i] = gi
        dqkv5 = g[0]
        self.leaf = self.out = self.inputs = None
        if dqkv5 is None:
            dqkv5 = torch.zeros_like(qkv5)
        return (dqkv5 if dqkv5.is_contiguous() else dqkv5.contiguous()), tuple(extra), (), None


def _pooled_rows(where, BH, L, d, device):
    """Where a projection kernel leaves the pooled q / k rows [BH, L, d] (fp32) -> (Pooled for the core's forward, pq, pk): inside
    a fresh `saved` workspace of a composite entry, where = (n_saved, the rows' two offsets) of its plan, or (None) on their own."""
    if where is None:
        pq = torch.empty((BH, L, d), dtype=torch.float32, device=device)
        pk = torch.empty_like(pq)
        return Pooled(None, pq, pk), pq, pk
    ws = torch.empty(where[0], dtype=torch.float32, device=device)
    return Pooled(ws, None, None), _ws_rows(ws, where[1], BH * L * d), _ws_rows(ws, where[2], BH * L * d)


def _project_qkv_grid(x2, wq, bq32, cdtype, want, need_dx, w192, grid, pq, pk):
    """The `project` hook's launch: the qkv projection that writes the cell means of q / k over grid = (B, H, W, r) to pq / pk
    (round 4: no pooling pass, 87 MB / 17 us at cfg3), from the prepared weights (round 6) or from the fp32 master weight, whose
    rounded copy for the backward's input-gradient GEMM leaves with the same launch -> (y, rounded x | None, rounded weight | None)."""
    if w192 is not None:
        y, xc = project_qkv_wsw(x2, w192[1], w192[0], bq32, cdtype, want, grid, pq, pk)
        return y, xc, w192[0]
    w16 = torch.empty(tuple(wq.shape), dtype=cdtype, device=x2.device) if need_dx else None
    y, xc = project_qkv_pooled(x2, wq, bq32, cdtype, want, *grid, pq, pk, w_cast=w16)
    return y, xc, w16


class EvaCore(Core):
    """Core spec of the module node (EvaModuleFn): the EVA core (eva_fwd_impl / eva_bwd_impl, the composite entry points where
    the geometry allows).  cfg: an EvaCfg with its defaults (not causal, no dropout); the differentiable inputs are the dense
    window bias [h, Wq, Wk] | None -- with table_bias, a TableBias, its TABLE [rows, h] -- and then the mu-network parameters."""

    def __init__(self, mask_u8, noise, cfg, table_bias=None):
        self.mask_u8, self.noise, self.cfg, self.tb = mask_u8, noise, cfg, table_bias

    def setup(self, B, N, heads, d, elem, inputs, need_grad):
        cfg = self.cfg
        bias = inputs[0]
        if self.tb is not None:
            bias = self.tb.dense(bias, self.tb.ld(B, heads, N, d, elem, cfg.attn_2d, cfg.seq_shape, cfg.window, cfg.ext,
                                                  int(cfg.chunk), int(cfg.L), 0))
        self.bias, self.bias_cols = bias, 0 if bias is None else bias.shape[-1]       # (the dense bias lives until fwd())
        self.lists = cfg.lists(need_grad)
        self.sizes = (_eva_layer_cfg_dims(B, heads, d, elem, cfg, bias is not None, self.mask_u8 is not None)[1]
                      if _eva_use_composite() else None)                              # None: step by step
        self.dims, self.pooled = (B, heads, d), None

    def project(self, x2, wq, bq32, cdtype, want, need_dx, w192):
        cfg = self.cfg
        B, heads, d = self.dims
        if not (cfg.attn_2d and cfg.ext == 0 and self.mask_u8 is None
                and proj_pool_supported(x2, wq, cdtype, B, cfg.seq_shape[0], cfg.seq_shape[1], cfg.chunk, heads)):
            return None
        pl = self.sizes                                              # (composite: straight into the entry's workspace)
        where = None if pl is None else (pl.n_saved, pl.saved_qmean, pl.saved_kmean)
        self.pooled, pq, pk = _pooled_rows(where, B * heads, cfg.L, d, x2.device)
        return _project_qkv_grid(x2, wq, bq32, cdtype, want, need_dx, w192, (B, cfg.seq_shape[0], cfg.seq_shape[1], cfg.chunk),
                                 pq, pk)

    def fwd(self, qkv5, inputs):
        bias, pooled, self.bias, self.pooled = self.bias, self.pooled, None, None
        outs = eva_fwd_impl(qkv5, bias, self.noise, self.mask_u8, None, *self.lists, self.cfg.adaptive_proj, list(inputs[1:]),
                            pooled=pooled, composite=self.sizes is not None)
        self.nsaved = len(outs) - 1
        return outs[0], tuple(outs[1:]) + tuple(inputs[1:])

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        saved, params = saved[:self.nsaved], saved[self.nsaved:]
        use_fin = fin_ok and _eva_saved_is_composite(saved)   # round 5: ea_linear_dgrad_finish adds the d(chunk mean) / r^2 terms
        g = _eva_backward(dout, qkv5, self.mask_u8, None, self.noise, out, list(saved), self.cfg, self.bias_cols, list(params),
                          defer_param_sums=defer, defer_chunk_mean=use_fin)
        return g.dqkv, [g.dbias] + (g.params or []), g.partials, (g.finish, None) if use_fin else None

    def scatter(self, res, extra):
        dbias, pgrads = extra[0], extra[1:]
        if "mlp_W" in res:
            pgrads = _mlp_grads(res["mlp_W"][0], res["mlp_v"][0], self.dims[2])
        if "dbias" in res:
            dbias = res["dbias"][0].view(res["dbias"][1])[..., :self.bias_cols].contiguous()
        if dbias is not None and self.tb is not None:
            dbias = self.tb.grad(dbias)                # [h, Wq, ld] -> d table [rows, h], one launch
        return [dbias] + pgrads


class LaraCore(Core):
    """Core spec of the module node (LaraModuleFn): the 2-D pooled LARA core (lara_fwd_impl / lara_bwd_impl; through the
    dispatcher ops while somebody is tracing).  cfg: a LaraCfg; the differentiable inputs are the generator parameters."""

    def __init__(self, mask_u8, noise, cfg):
        self.mask_u8, self.noise, self.cfg = mask_u8, noise, cfg

    def setup(self, B, N, heads, d, elem, inputs, need_grad):
        self.lists = self.cfg.lists(need_grad)
        self.dims, self.pooled = (B, heads, d, elem), None

    def project(self, x2, wq, bq32, cdtype, want, need_dx, w192):
        cfg = self.cfg
        B, heads, d, elem = self.dims
        if not proj_pool_supported(x2, wq, cdtype, B, cfg.H, cfg.W, cfg.r, heads):
            return None
        pl = _lara_layer_cfg_dims(B, heads, d, elem, cfg)[1] if _lara_use_composite() else None
        where = None if pl is None else (pl.n_saved, pl.saved_pq, pl.saved_pk)
        self.pooled, pq, pk = _pooled_rows(where, B * heads, cfg.L, d, x2.device)
        return _project_qkv_grid(x2, wq, bq32, cdtype, want, need_dx, w192, (B, cfg.H, cfg.W, cfg.r), pq, pk)

    def fwd(self, qkv5, inputs):
        pooled, self.pooled = self.pooled, None
        if pooled is not None:
            outs = lara_fwd_impl(qkv5, self.mask_u8, self.noise, *self.lists, list(inputs), pooled=pooled)
        else:
            outs = _ea_op("lara_fwd", lara_fwd_impl, qkv5, self.mask_u8, self.noise, *self.lists, list(inputs))
        self.nsaved = len(outs) - 1
        return outs[0], tuple(outs[1:]) + tuple(inputs)

    def fwd_project(self, qkv5, inputs, w16p, bp32, cdtype):
        """fwd with the module's output projection inside the combine pass (ABI 29) -> (out, y2 [B*N, h*d], saved), or None
        -- before anything is launched or consumed -- where that pass does not apply: not three heads of 64 channels, more
        than 64 samples, the projection switched off (EA_LARA_OUT_PROJ=0)."""
        B, heads, d, elem = self.dims
        if not (lara_out_proj_on() and heads == 3 and d == 64 and self.cfg.C <= 64 and qkv5.dtype == cdtype and w16p.dtype == cdtype
                and w16p.is_contiguous() and tuple(w16p.shape) == (192, 192)
                and (bp32 is None or (bp32.dtype == torch.float32 and bp32.is_contiguous()))):
            return None
        y2 = torch.empty((qkv5.shape[0] * qkv5.shape[1], heads * d), dtype=cdtype, device=qkv5.device)
        proj = [w16p, bp32, y2]
        pooled, self.pooled = self.pooled, None
        outs = lara_fwd_impl(qkv5, self.mask_u8, self.noise, *self.lists, list(inputs), pooled=pooled, proj=proj)
        self.nsaved = len(outs) - 1
        return outs[0], proj[2], tuple(outs[1:]) + tuple(inputs)

    def bwd(self, dout, qkv5, out, saved, defer, fin_ok):
        saved, params = saved[:self.nsaved], saved[self.nsaved:]
        head = (dout, qkv5, self.mask_u8, self.noise, list(saved))
        if not defer:
            g = _ea_op("lara_bwd", lara_bwd_impl, *head, *self.lists, list(params))
            return g[0], g[1:], (), None
        # round 5: the finish pass of the core is left to the input-gradient kernel (ea_linear_dgrad_finish: one pass, not two)
        use_fin = bool(fin_ok and self.cfg.dup == 0 and self.cfg.L <= 64)
        g = _lara_backward(*head, self.cfg, list(params), defer_param_sums=True, defer_finish=use_fin)
        fin = (g.finish, qkv5.view(qkv5.shape[0] * qkv5.shape[1], -1)) if use_fin else None
        return g.dqkv, g.params or [], g.partials, fin

    def scatter(self, res, extra):
        return _mlp_grads(res["mlp_W"][0], res["mlp_v"][0], self.dims[2]) if "mlp_W" in res else extra


class CoreModuleFn(torch.autograd.Function):
    """qkv projection -> attention core -> output projection as ONE autograd node: the launches of LinearFn + the core's Function
    + LinearFn without two of the three nodes' host cost (ctx objects, saved-tensor packing, engine hand-overs: ~0.1 ms of the
    host-bound eager step).  Only for the common training case -- 16-bit autocast, fp32 master weights (the
    *_module_fn_supported predicates); every other case keeps the three nodes.  This is the ONE body of that scheme: EvaModuleFn
    and LaraModuleFn are its names around the two landmark cores.
    args: x [B, *seq, C], qkv weight / bias, proj weight / bias, core spec, compute dtype, heads, the core's differentiable inputs.
    Projections: library GEMMs on 16-bit operands at widths the streaming kernels do not cover (module_proj_lib, round 6: the
    four parameter casts in one launch, the rounded weights kept for the backward's input-gradient GEMMs), else the prepared
    16-bit weights of a 192-wide layer (prepare_w192), else the fp32 master weights (linear_w32).  Backward: both weight
    gradients in one launch where possible (ea_wgrad_pair), else the output projection's before the core's backward and the qkv
    projection's after it; all terminal sums -- the weight gradients' slice partials, the core's partials -- in ONE ea_multi_sum.
    The core spec's protocol: Core."""

    @staticmethod
    def forward(ctx, x, wq, bq, wp, bp, core, cdtype, heads, *inputs):
        B, C = x.shape[0], x.shape[-1]
        N = x.numel() // (B * C)
        d = C // heads
        x2 = x.reshape(-1, C)
        elem = _ELEM[cdtype]
        need = ctx.needs_input_grad
        # (only LaraModuleFn is reached while somebody is tracing: its projections and core are dispatcher ops then)
        direct = _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0
        lin = linear_w32_impl if direct else torch.ops.ea.linear_w32
        core.setup(B, N, heads, d, elem, inputs, any(need))
        bq32 = None if bq is None else (bq if bq.dtype == torch.float32 else bq.float())
        bp32 = None if bp is None else (bp if bp.dtype == torch.float32 else bp.float())
        want = x2.dtype == torch.float32 and need[1]
        lib = module_proj_lib(C)
        w16q = w16p = b16p = None
        w192 = prepare_w192_rs(wq, wp, cdtype) if (not lib and w192_usable(wq, wp, cdtype)) else None
        w16pT = None if w192 is None else w192[3]
        wpT_rs = None if w192 is None else w192[6]
        if lib:
            w16q, b16q, w16p, b16p = lib_casts(wq, bq, wp, bp, cdtype)
            y, xc = lib_project(x2, wq, bq32, w16q, b16q, cdtype)
            want = True
        else:
            done = core.project(x2, wq, bq32, cdtype, want, need[0], w192) if direct else None
            if done is not None:
                y, xc, w16q = done
            elif w192 is not None:
                w16q = w192[0]
                y, xc = project_qkv_wsw(x2, w192[1], w16q, bq32, cdtype, want)
            else:
                y, xc = lin(x2, wq, bq32, elem, False, False, want)
        xl = x2 if x2.dtype == cdtype else (xc if want else None)
        qkv5 = y.view(B, N, 3, heads, d)
        # the output projection inside the core's last pass, where the core offers it (LaraCore.fwd_project, ABI 29)
        done = core.fwd_project(qkv5, inputs, w192[2], bp32, cdtype) if (direct and w192 is not None) else None
        if done is not None:
            out, y2, saved = done
        else:
            out, saved = core.fwd(qkv5, inputs)
        o2 = out.reshape(-1, C)
        if done is not None:
            pass
        elif lib:
            with torch.autocast(device_type="cuda", enabled=False):
                y2 = F.linear(o2, w16p, b16p)
        elif w192 is not None and w192[5] is not None and _rs192_rows_ok(o2, cdtype):
            y2 = linear_rs192(o2, w192[5], bp32, cdtype)
        elif w192 is not None:
            y2 = ea_linear(o2, w192[2], bp32, cdtype)[0]
        else:
            y2 = lin(o2, wp, bp32, elem, False, False, False)[0]
        # the prepared W^T goes with the rounded weight it was made from
        wqT = w192[4] if (w192 is not None and w16q is w192[0]) else None
        ctx.save_for_backward(xl, qkv5, o2, wq, wp, w16q, w16p, w16pT, wqT, wpT_rs, *saved)
        ctx.core = core
        ctx.meta = (x.shape, x.dtype, cdtype, None if bq is None else bq.dtype, None if bp is None else bp.dtype, wq.dtype, wp.dtype,
                    heads, [None if t is None else t.dtype for t in inputs])
        return y2.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        xl, qkv5, o2, wq, wp, w16q, w16p, w16pT, wqT, wpT_rs, *saved = ctx.saved_tensors
        xshape, xdtype, cdtype, bqd, bpd, wqd, wpd, heads, in_dtypes = ctx.meta
        core = ctx.core
        C = xshape[-1]
        d = C // heads
        need = ctx.needs_input_grad
        if need[1] and xl is None:
            raise RuntimeError("%s: the weight gradient was requested but the forward did not keep its input"
                               % ctx._forward_cls.__name__)
        direct = _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0
        dy2 = dy.reshape(-1, C)
        if dy2.dtype != cdtype:
            dy2 = dy2.to(cdtype)
        # output projection, input gradient: on the rounded weight (library flavour), the prepared W^T, or the master weight transposed
        if w16p is not None:
            dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
            d_o2 = dy2 @ w16p
        elif wpT_rs is not None and _rs192_rows_ok(dy2, cdtype):
            d_o2 = linear_rs192(dy2, wpT_rs, None, cdtype)
        elif w16pT is not None and _lin_rows_ok(dy2, cdtype):
            d_o2 = ea_linear(dy2, w16pT, None, cdtype)[0]
        else:
            lin = linear_w32_impl if direct else torch.ops.ea.linear_w32
            d_o2 = lin(dy2, wp, None, _ELEM[cdtype], True, False, False)[0]
        defer = direct and USE_MULTI_SUM                    # the terminal sums wait for ONE ea_multi_sum at the end
        need_bq, need_bp = bqd is not None and need[2], bpd is not None and need[4]
        qkv2 = qkv5.view(-1, 3 * C)
        # both weight gradients in ONE launch after the core's backward (ea_wgrad_pair; d qkv has the shape and type of qkv)
        pair = bool(defer and need[1] and need[3] and wgrad_pair_usable(qkv2, xl, dy2, o2))
        dwq = dbq = dwp = dbp = dx = None
        pend = []                                           # (what, partial tensor, meta)
        if need[3] and not pair:
            r_ = wgrad(dy2, o2, need_bp, defer=defer)
            if defer:
                pend.append(("proj", r_[0], r_[1]))
            else:
                dwp, dbp = r_[0].to(wpd), (r_[1].to(bpd) if need_bp else None)
        elif need_bp and not pair:
            dbp = bias_grad(dy2 if dy2.is_contiguous() else dy2.contiguous()).to(bpd)
        B, N = qkv5.shape[:2]
        dout, out = d_o2.view(B, N, heads, d), o2.view(B, N, heads, d)
        dqkv5, extra, parts, fin = core.bwd(dout, qkv5, out, saved, defer,
                                            bool(need[0] and dgrad_finish_usable(qkv2, wq, xdtype, heads, d)))
        pend += parts
        dqkv2 = dqkv5.view(-1, 3 * C)
        if fin is not None:
            # corrects the dq / dk columns of dqkv2 in place: BEFORE the weight gradient reads them
            dx = qkv_dgrad_finish(dqkv2, fin[1], wq, w16q, xdtype, fin[0], wqT).view(xshape)
        if pair:
            rq, rp = wgrad_pair(dqkv2, xl, need_bq, dy2, o2, need_bp)
            pend += [("qkv", rq[0], rq[1]), ("proj", rp[0], rp[1])]
        elif need[1]:
            r_ = wgrad(dqkv2, xl, need_bq, defer=defer)
            if defer:
                pend.append(("qkv", r_[0], r_[1]))
            else:
                dwq, dbq = r_[0].to(wqd), (r_[1].to(bqd) if need_bq else None)
        elif need_bq:
            # frozen qkv weight, trainable bias (bias-only fine-tuning): a column sum of d qkv, no input rows needed
            dbq = bias_grad(dqkv2).to(bqd)
        if need[0] and dx is None:
            dx = qkv_dgrad(dqkv2, wq, w16q, xdtype, wqT).view(xshape)
        res = {}
        if pend:
            sums = multi_sum([t for _, t, _ in pend])
            res = {what: (o, meta) for (what, _, meta), o in zip(pend, sums)}
            if "proj" in res:
                dwp, dbp = _wgrad_split(*res["proj"])
                dwp, dbp = dwp.to(wpd), (dbp.to(bpd) if need_bp else None)
            if "qkv" in res:
                dwq, dbq = _wgrad_split(*res["qkv"])
                dwq, dbq = dwq.to(wqd), (dbq.to(bqd) if need_bq else None)
        extra = core.scatter(res, extra)
        egrads = tuple(None if (g is None or dt is None) else g.to(dt) for g, dt in zip(extra, in_dtypes))
        return (dx, dwq, dbq, dwp, dbp, None, None, None) + egrads


class EvaModuleFn(CoreModuleFn):
    """CoreModuleFn around an EvaCore, under the name EVA's single node has in graphs, tests and messages."""


class LaraModuleFn(CoreModuleFn):
    """CoreModuleFn around a LaraCore, under the name LinearRA's single node has in graphs, tests and messages."""


USE_WIDE_MODULE_FN = os.environ.get("EA_WIDE_MODULE_FN", "1") == "1"


def multi_cast(ts, dtype):
    """fp32 tensors -> their `dtype` copies in ONE launch (ea_multi_cast; round 6): the autocast casts of a wide layer's two
    weights and two biases, four `.to(dtype)` launches until now."""
    ts = [t.detach() if t.is_contiguous() else t.detach().contiguous() for t in ts]
    outs = [torch.empty(t.shape, dtype=dtype, device=t.device) for t in ts]
    K = len(ts)
    src = (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])
    dst = (ctypes.c_void_p * K)(*[o.data_ptr() for o in outs])
    n = (ctypes.c_int64 * K)(*[t.numel() for t in ts])
    nv.call("ea_multi_cast", _ELEM[dtype], K, src, n, dst, nv.stream())
    return outs


def module_proj_lib(C):
    """The single-node module paths run their two projections on this library's streaming kernels where those exist (64 ..
    256 input channels) and, round 6, as library GEMMs on 16-bit operands elsewhere (320 / 512 / 1024-wide layers): True = the
    library-GEMM flavour."""
    return not (_lin_geometry(C, 3 * C) and _lin_geometry(C, C))


def lib_project(x2, w32, b32, w16, b16, cdtype):
    """(y = x2 @ w^T + b in cdtype by the library GEMM, the 16-bit x it ran on)."""
    xl = x2 if x2.dtype == cdtype else x2.to(cdtype)        # the one activation-sized cast of the layer
    with torch.autocast(device_type="cuda", enabled=False):
        y = F.linear(xl, w16, b16)
    return y, xl


def lib_casts(wq, bq, wp, bp, cdtype):
    """16-bit copies of (qkv weight, qkv bias | None, proj weight, proj bias | None), one launch."""
    src = [t for t in (wq, bq, wp, bp) if t is not None]
    if all(t.dtype == torch.float32 for t in src):
        cs = multi_cast(src, cdtype)
    else:
        cs = [t if t.dtype == cdtype else t.to(cdtype) for t in src]
    it = iter(cs)
    return tuple(None if t is None else next(it) for t in (wq, bq, wp, bp))


def core_module_fn_supported(x, qkv, proj, cdtype):
    """The single-node path of the softmax / local-window baselines (CoreModuleFn): what the module node asks of the projections
    (lara_module_fn_supported), direct calls only."""
    return (USE_CORE_MODULE_FN and _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0
            and lara_module_fn_supported(x, qkv, proj, cdtype, allow_lib=True))


def lara_module_fn_supported(x, qkv, proj, cdtype, allow_lib=False):
    """What the module node (CoreModuleFn; here for LinearRA's LaraModuleFn) needs: 16-bit autocast dtype, fp32 master weights
    both projection kernels cover (forward of both layers, the output projection's transposed input gradient), the one-pass
    weight gradient.  allow_lib (every core but LARA; round 6): widths outside the streaming kernels' 64 .. 256 channels qualify too --
    their projections run as library GEMMs inside the node (module_proj_lib)."""
    if not (USE_LARA_MODULE_FN and x.is_cuda and cdtype in _ELEM and x.dtype in (torch.float32, cdtype)):
        return False
    C = x.shape[-1]
    x2 = x.reshape(-1, C)

    def w_ok(w, out):
        return (w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and tuple(w.shape) == (out, C)
                and (w.storage_offset() * 4) % 16 == 0)
    geo = (_lin_geometry(C, 3 * C) and _lin_geometry(C, C)) or (allow_lib and USE_WIDE_MODULE_FN)
    return (w_ok(qkv.weight, 3 * C) and w_ok(proj.weight, C) and _lin_rows_ok(x2, cdtype) and geo
            and USE_WGRAD and C % 64 == 0 and x2.shape[0] >= 64)


def _lmk_saved(geom, device):
    """Workspace in which ea_lara_landmarks_fwd keeps its intermediates for the backward."""
    n = nv.lib().ea_lara_landmarks_saved_floats(ctypes.byref(geom))
    if n < 0:
        raise RuntimeError("ea_lara_landmarks_saved_floats: %d" % n)
    return torch.empty(n, dtype=torch.float32, device=device)


class LaraLandmarkFn(torch.autograd.Function):
    """Fused landmark pipeline (ea_lara_landmarks_fwd/bwd): pooled q/k [B,h,L,d] (or ready q_bar/k_bar
    when has_mlp = mixed = 0) -> omega, qbar_rows [B,h,C,d], bhv, lp [B,h,C].  params = (Wq, bq,
    gq, cq, Wk, bk, gk, ck) when has_mlp; colbias [B,h,L] (or None) is the '-vmixed' column bias of the
    mixing logits."""

    @staticmethod
    def forward(ctx, pq, pk, noise, colbias, cfg, *params):
        has_mlp, mixed, mis, dup, scale = cfg
        nv.require_cuda(pq, "pooled q/k")
        B, h, L, d = pq.shape
        C = L * (2 if dup else 1)
        BH, dev = B * h, pq.device
        pq = pq.float().contiguous()
        pk = pk.float().contiguous()
        noise_c = None if noise is None else noise.float().contiguous()
        cb = None if colbias is None else colbias.float().contiguous()
        ps = [t.float().contiguous() for t in params]
        geom = nv.ea_lmk_geom(BH, L, C, d, int(has_mlp), int(mixed), mis, dup, float(scale), 0)
        global LAST_LMK_GEOM
        LAST_LMK_GEOM = (BH, L, C, d, int(has_mlp), int(mixed), 0)
        omega = torch.empty((B, h, C, d), dtype=torch.float32, device=dev)
        qrows = torch.empty_like(omega) if mis != 2 else None
        bhv = torch.empty((B, h, C), dtype=torch.float32, device=dev) if mis == 0 else None
        lp = torch.empty((B, h, C), dtype=torch.float32, device=dev)
        pp = [nv.ptr(t) for t in ps] if has_mlp else [None] * 8
        saved = _lmk_saved(geom, dev) if any(ctx.needs_input_grad) else None
        if cb is None:
            nv.call("ea_lara_landmarks_fwd", ctypes.byref(geom), nv.ptr(pq), nv.ptr(pk), *pp, nv.ptr(noise_c),
                    nv.ptr(omega), nv.ptr(qrows), nv.ptr(bhv), nv.ptr(lp), nv.ptr(saved), nv.stream())
        else:
            nv.call("ea_lara_landmarks_fwd_cb", ctypes.byref(geom), nv.ptr(pq), nv.ptr(pk), *pp, nv.ptr(noise_c), nv.ptr(cb),
                    nv.ptr(omega), nv.ptr(qrows), nv.ptr(bhv), nv.ptr(lp), nv.ptr(saved), nv.stream())
        ctx.save_for_backward(pq, pk, noise_c, cb, *ps)
        ctx.lmk_saved = saved
        ctx.geom = geom
        ctx.pdtypes = [t.dtype for t in params]
        return omega, qrows, bhv, lp

    @staticmethod
    def backward(ctx, d_omega, d_qrows, d_bhv, d_lp):
        pq, pk, noise_c, cb, *ps = ctx.saved_tensors
        geom = ctx.geom
        BH, L, C, d = geom.BH, geom.L, geom.C, geom.D
        dev = pq.device

        def fz(t, shape):
            return (torch.zeros(shape, dtype=torch.float32, device=dev) if t is None
                    else t.float().contiguous())
        d_omega = fz(d_omega, (BH, C, d))
        d_lp = fz(d_lp, (BH, C))
        d_qrows = None if d_qrows is None else d_qrows.float().contiguous()
        d_bhv = None if d_bhv is None else d_bhv.float().contiguous()
        dpq = torch.empty_like(pq)
        dpk = torch.empty_like(pk)
        dW = dvec = d_cb = None
        if geom.has_mlp:
            dW = torch.empty((BH, 2, d, d), dtype=torch.float32, device=dev)
            dvec = torch.empty((BH, 2, 3, d), dtype=torch.float32, device=dev)
        pp = [nv.ptr(t) for t in ps] if geom.has_mlp else [None] * 8
        if cb is None:
            nv.call("ea_lara_landmarks_bwd", ctypes.byref(geom), nv.ptr(pq), nv.ptr(pk), *pp, nv.ptr(noise_c),
                    nv.ptr(d_omega), nv.ptr(d_qrows), nv.ptr(d_bhv), nv.ptr(d_lp), nv.ptr(dpq), nv.ptr(dpk),
                    nv.ptr(dW), nv.ptr(dvec), nv.ptr(ctx.lmk_saved), nv.stream())
        else:
            d_cb = torch.empty_like(cb)
            nv.call("ea_lara_landmarks_bwd_cb", ctypes.byref(geom), nv.ptr(pq), nv.ptr(pk), *pp, nv.ptr(noise_c), nv.ptr(cb),
                    nv.ptr(d_omega), nv.ptr(d_qrows), nv.ptr(d_bhv), nv.ptr(d_lp), nv.ptr(dpq), nv.ptr(dpk),
                    nv.ptr(dW), nv.ptr(dvec), nv.ptr(d_cb), nv.ptr(ctx.lmk_saved), nv.stream())
        pgrads = []
        if geom.has_mlp:
            raw = _mlp_grads(*colsum2_f32(dW.view(BH, -1), dvec.view(BH, -1)), d)
            pgrads = [g.to(dt) for g, dt in zip(raw, ctx.pdtypes)]
        return (dpq, dpk, None, d_cb, None) + tuple(pgrads)


def lara_landmarks(pq, pk, noise, mis_type, mode, scale, params=None, mixed=False, colbias=None):
    """-> omega, qbar_rows, bhv, lp through the fused HIP landmark kernels (L, C <= 64).  mixed: the softmax mixing of
    k_bar (lara.py:157-174) runs inside the kernel; colbias [B,h,L]: its '-vmixed' column bias."""
    has_mlp = params is not None
    cfg = (has_mlp, bool(mixed), MIS[mis_type], int(mode) if noise is not None else 0, float(scale))
    return LaraLandmarkFn.apply(pq, pk, noise, colbias, cfg, *(params or ()))


def _prm(data, proj, scale):
    """s <proj_c, data_n> - s |data_n|^2 / 2  (prm_projection normalize=False), tiny tensors."""
    return scale * torch.einsum("bhcd,bhnd->bhcn", proj, data) - 0.5 * scale * (data * data).sum(-1).unsqueeze(-2)


class LaraSampleFn(torch.autograd.Function):
    """omega, qbar_rows, bhv, lp from q_bar, mu = q_bar + k_bar and the noise draw (ea_lara_sample_fwd/bwd): the sampling and
    the [C x L] proposal-density algebra for sample counts the fused landmark kernels do not hold (C > 64)."""

    @staticmethod
    def forward(ctx, q_bar, mu, noise, mis, mode, scale):
        nv.require_cuda(mu, "landmarks")
        B, h, L, d = mu.shape
        mode = int(mode) if noise is not None else 0
        C = L * (2 if mode else 1)
        dev = mu.device
        q_bar, mu = q_bar.float().contiguous(), mu.float().contiguous()
        noise_c = None if noise is None else noise.float().contiguous()
        omega = torch.empty((B, h, C, d), dtype=torch.float32, device=dev)
        qrows = torch.empty_like(omega) if mis != 2 else None
        bhv = torch.empty((B, h, C), dtype=torch.float32, device=dev) if mis == 0 else None
        lp = torch.empty((B, h, C), dtype=torch.float32, device=dev)
        nv.call("ea_lara_sample_fwd", B * h, L, C, d, mis, mode, float(scale), nv.ptr(q_bar), nv.ptr(mu), nv.ptr(noise_c),
                nv.ptr(omega), nv.ptr(qrows), nv.ptr(bhv), nv.ptr(lp), nv.stream())
        ctx.save_for_backward(q_bar, mu, noise_c)
        ctx.cfg = (mis, mode, float(scale), C)
        return omega, qrows, bhv, lp

    @staticmethod
    def backward(ctx, d_omega, d_qrows, d_bhv, d_lp):
        q_bar, mu, noise_c = ctx.saved_tensors
        mis, mode, scale, C = ctx.cfg
        B, h, L, d = mu.shape

        def f(t):
            return None if t is None else t.float().contiguous()
        d_omega = torch.zeros((B, h, C, d), dtype=torch.float32, device=mu.device) if d_omega is None else f(d_omega)
        d_qbar, d_mu = torch.empty_like(q_bar), torch.empty_like(mu)
        nv.call("ea_lara_sample_bwd", B * h, L, C, d, mis, mode, scale, nv.ptr(q_bar), nv.ptr(mu), nv.ptr(noise_c),
                nv.ptr(d_omega), nv.ptr(f(d_qrows)), nv.ptr(f(d_bhv)), nv.ptr(f(d_lp)), nv.ptr(d_qbar), nv.ptr(d_mu), nv.stream())
        return d_qbar, d_mu, None, None, None, None


def _sample_fits(L, C, d):
    """LDS budget of ea_lara_sample_bwd (lara_sample_lds, ea_lara_segment.hip)."""
    return C <= 256 and ((L + C) * (d + 1) + ((L + 3) & ~3) + C * (L + 1)) * 4 <= 150 * 1024


def lara_attention(qkv5, mask_u8, q_bar, mu, noise, mis_type, alpha_coeff, mode, scale, slot=None):
    """Sampling + the [C x L] proposal-density algebra on the landmarks (lara.py:187-238), then the HIP estimator.
    mode: 0 single, 1 antithetic, 2 multi-sample noise.  The algebra is ea_lara_sample_* (fp32 HIP); landmark sets too
    large for its LDS image fall back to tiny torch ops with autograd."""
    mis = MIS[mis_type]
    q_bar, mu = q_bar.float(), mu.float()
    dup = noise is not None and mode in (1, 2)
    L, d = mu.shape[-2], mu.shape[-1]
    if mu.is_cuda and _sample_fits(L, L * (2 if dup else 1), d):
        omega, qbar_rows, bhv, lp = LaraSampleFn.apply(q_bar, mu, noise, mis, mode, float(scale))
        return LaraAttnFn.apply(qkv5, mask_u8, omega, qbar_rows, bhv, lp, mis, float(alpha_coeff), slot)
    if noise is None:
        omega = mu
    elif mode == 2:
        omega = mu.repeat(1, 1, 2, 1) + noise.float()
    elif mode == 1:
        omega = torch.cat([mu + noise.float(), mu - noise.float()], dim=-2)
    else:
        omega = mu + noise.float()
    rep = (lambda t: t.repeat(1, 1, 2, 1)) if dup else (lambda t: t)
    qbar_rows = bhv = None
    if mis == 0:
        lpmu = _prm(rep(mu), omega, scale)                               # [B,h,C,C]
        lp = torch.diagonal(lpmu, dim1=-1, dim2=-2)
        bhv = torch.exp(lp - torch.logsumexp(lpmu, dim=-1))
        qbar_rows = rep(q_bar)
    elif mis == 1:
        lp = torch.logsumexp(_prm(mu, omega, scale), dim=-1)            # [B,h,C]
        qbar_rows = rep(mu)
    else:
        lp = torch.logsumexp(_prm(mu, omega, scale), dim=-1)
    return LaraAttnFn.apply(qkv5, mask_u8, omega, qbar_rows, bhv, lp, mis, float(alpha_coeff), slot)


# ------------------------------------------------------------------------------------------
# softmax baseline  (reference abstract_attention.py:120-133)
# ------------------------------------------------------------------------------------------
def softmax_fwd_impl(qkv5, mask_u8, keep, keep_scale):
    """torch.ops.ea.softmax_fwd -> [out [B,N,h,d], lse [B*h,N]]."""
    nv.require_cuda(qkv5, "qkv")
    B, N, _, h, d = qkv5.shape
    q, k, v = _qkv_views(qkv5)
    out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=qkv5.device)
    lse = torch.empty((B * h, N), dtype=torch.float32, device=qkv5.device)
    tq, tk, tv, to = nv.t4(q), nv.t4(k), nv.t4(v), nv.t4(out.permute(0, 2, 1, 3))
    nv.call("ea_softmax_attn_fwd", B, h, N, d, nv.io_dtype(qkv5), float(d) ** -0.5, ctypes.byref(tq),
            ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8), ctypes.byref(to), nv.ptr(lse),
            nv.ptr(keep), float(keep_scale), 0, nv.stream())
    return [out, lse]


def softmax_bwd_impl(dout, qkv5, mask_u8, out, lse, keep, keep_scale):
    """torch.ops.ea.softmax_bwd -> dqkv [B,N,3,h,d]."""
    B, N, _, h, d = qkv5.shape
    dout = dout.contiguous()
    dqkv5 = torch.empty_like(qkv5)
    delta = torch.empty_like(lse)
    q, k, v = _qkv_views(qkv5)
    dq, dk, dv = _qkv_views(dqkv5)
    ts = [nv.t4(t) for t in (q, k, v, out.permute(0, 2, 1, 3), dout.permute(0, 2, 1, 3), dq, dk, dv)]
    nv.call("ea_softmax_attn_bwd", B, h, N, d, nv.io_dtype(qkv5), float(d) ** -0.5, ctypes.byref(ts[0]),
            ctypes.byref(ts[1]), ctypes.byref(ts[2]), nv.ptr(mask_u8), ctypes.byref(ts[3]),
            ctypes.byref(ts[4]), nv.ptr(lse), nv.ptr(delta), ctypes.byref(ts[5]), ctypes.byref(ts[6]),
            ctypes.byref(ts[7]), nv.ptr(keep), float(keep_scale), 0, nv.stream())
    return dqkv5


class SoftmaxAttnFn(torch.autograd.Function):
    """out[B,N,h,d] = dropout(softmax(s QK^T, -inf on padded keys)) V on a fused qkv tensor; keep: None
    or the uint8 keep decisions [B,h,N,64*ceil(N/64)] of the attention dropout, scaled by keep_scale
    (torch.ops.ea.softmax_fwd / softmax_bwd)."""

    @staticmethod
    def forward(ctx, qkv5, mask_u8, keep=None, keep_scale=1.0):
        out, lse = _ea_op("softmax_fwd", softmax_fwd_impl, qkv5, mask_u8, keep, float(keep_scale))
        ctx.save_for_backward(qkv5, mask_u8, out, lse, keep)
        ctx.keep_scale = float(keep_scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv5, mask_u8, out, lse, keep = ctx.saved_tensors
        return _ea_op("softmax_bwd", softmax_bwd_impl, dout, qkv5, mask_u8, out, lse, keep, ctx.keep_scale), None, None, None


class SoftmaxQKVFn(torch.autograd.Function):
    """out[B,N,h,d] = softmax_j(s q.k_j [- s |k_j|^2 / 2]) v_j for separate q, k, v [B,h,N,d] (any
    strides, rows contiguous; k and v may be the same tensor).  key_norm_bias = 1 is the second softmax
    of randomized attention (randomized_attention.py:44-51)."""

    @staticmethod
    def forward(ctx, q, k, v, key_norm_bias):
        nv.require_cuda(q, "q")
        B, h, N, d = q.shape
        q, k, v = [t if (t.stride(-1) == 1 and all(st % 8 == 0 for st in t.stride()[:-1])) else t.contiguous()
                   for t in (q, k, v)]
        out = torch.empty((B, N, h, d), dtype=q.dtype, device=q.device)
        lse = torch.empty((B * h, N), dtype=torch.float32, device=q.device)
        tq, tk, tv, to = nv.t4(q), nv.t4(k), nv.t4(v), nv.t4(out.permute(0, 2, 1, 3))
        nv.call("ea_softmax_attn_fwd", B, h, N, d, nv.io_dtype(q), float(d) ** -0.5, ctypes.byref(tq),
                ctypes.byref(tk), ctypes.byref(tv), None, ctypes.byref(to), nv.ptr(lse), None, 1.0,
                int(key_norm_bias), nv.stream())
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.key_norm_bias = int(key_norm_bias)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        B, h, N, d = q.shape
        dout = dout.contiguous()
        dqkv = torch.empty((B, N, 3, h, d), dtype=q.dtype, device=q.device)
        delta = torch.empty_like(lse)
        dq, dk, dv = _qkv_views(dqkv)
        ts = [nv.t4(t) for t in (q, k, v, out.permute(0, 2, 1, 3), dout.permute(0, 2, 1, 3), dq, dk, dv)]
        nv.call("ea_softmax_attn_bwd", B, h, N, d, nv.io_dtype(q), float(d) ** -0.5, ctypes.byref(ts[0]),
                ctypes.byref(ts[1]), ctypes.byref(ts[2]), None, ctypes.byref(ts[3]),
                ctypes.byref(ts[4]), nv.ptr(lse), nv.ptr(delta), ctypes.byref(ts[5]), ctypes.byref(ts[6]),
                ctypes.byref(ts[7]), None, 1.0, ctx.key_norm_bias, nv.stream())
        return dq, dk, dv, None


def softmax_sample(q, k):
    """One key index per query, drawn from softmax(s q k^T) without forming it (Gumbel-max in
    ea_softmax_sample; the seed comes from torch's generator on the device): int64 [B,h,N]."""
    nv.require_cuda(q, "q")
    B, h, N, d = q.shape
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=q.device)
    index = torch.empty((B * h, N), dtype=torch.int64, device=q.device)
    tq, tk = nv.t4(q), nv.t4(k)
    nv.call("ea_softmax_sample", B, h, N, d, nv.io_dtype(q), float(d) ** -0.5, ctypes.byref(tq),
            ctypes.byref(tk), nv.ptr(seed), nv.ptr(index), nv.stream())
    return index.view(B, h, N)


# ------------------------------------------------------------------------------------------
# Performer / FAVOR+  (reference kernelized_attention.py:20-56,116-121,326-346)
# ------------------------------------------------------------------------------------------
def performer_fwd_impl(qkv5, mask_u8, W):
    """torch.ops.ea.performer_fwd -> [out, stab [BH], kv [BH,m,d], ksum [BH,m]]."""
    nv.require_cuda(qkv5, "qkv")
    B, N, _, h, d = qkv5.shape
    m = W.shape[1]
    BH, dev = B * h, qkv5.device
    W = W.float().contiguous()
    geom = nv.ea_perf_geom(B, h, N, d, nv.io_dtype(qkv5), m)
    q, k, v = _qkv_views(qkv5)
    tq, tk, tv = nv.t4(q), nv.t4(k), nv.t4(v)
    S = nv.lib().ea_performer_parts(ctypes.byref(geom))
    p_ml = torch.empty((BH, S, m, 4), dtype=torch.float32, device=dev)
    nv.call("ea_performer_kmax", ctypes.byref(geom), ctypes.byref(tk), nv.ptr(W), nv.ptr(p_ml), nv.stream())
    stab = p_ml[..., 0].amax((1, 2)).contiguous()                     # [BH]
    p_kv = torch.empty((BH, S, m, d), dtype=torch.float32, device=dev)
    nv.call("ea_performer_kv", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8),
            nv.ptr(W), nv.ptr(stab), nv.ptr(p_ml), nv.ptr(p_kv), nv.stream())
    kv = p_kv.sum(1).contiguous()                                     # [BH, m, d]
    ksum = p_ml[..., 0].sum(1).contiguous()                           # [BH, m]
    out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=dev)
    to = nv.t4(out.permute(0, 2, 1, 3))
    nv.call("ea_performer_out", ctypes.byref(geom), ctypes.byref(tq), nv.ptr(W), nv.ptr(kv), nv.ptr(ksum),
            ctypes.byref(to), nv.stream())
    return [out, stab, kv, ksum]


def performer_bwd_impl(dout, qkv5, mask_u8, W, stab, kv, ksum, out):
    """torch.ops.ea.performer_bwd -> dqkv."""
    B, N, _, h, d = qkv5.shape
    m = W.shape[1]
    W = W.float().contiguous()
    geom = nv.ea_perf_geom(B, h, N, d, nv.io_dtype(qkv5), m)
    BH, dev = B * h, qkv5.device
    dout = dout.contiguous()
    dqkv5 = torch.empty_like(qkv5)
    q, k, v = _qkv_views(qkv5)
    dq, dk, dv = _qkv_views(dqkv5)
    tq, tk, tv = nv.t4(q), nv.t4(k), nv.t4(v)
    to, tdo = nv.t4(out.permute(0, 2, 1, 3)), nv.t4(dout.permute(0, 2, 1, 3))
    tdq, tdk, tdv = nv.t4(dq), nv.t4(dk), nv.t4(dv)
    tok = torch.empty((3, BH, N), dtype=torch.float32, device=dev)
    nv.call("ea_performer_bwd_q", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(to), ctypes.byref(tdo),
            nv.ptr(W), nv.ptr(kv), nv.ptr(ksum), ctypes.byref(tdq), nv.ptr(tok[0]), nv.ptr(tok[1]),
            nv.ptr(tok[2]), nv.stream())
    S = nv.lib().ea_performer_parts(ctypes.byref(geom))
    p_ml = torch.empty((BH, S, m, 4), dtype=torch.float32, device=dev)
    p_dkv = torch.empty((BH, S, m, d), dtype=torch.float32, device=dev)
    nv.call("ea_performer_bwd_qstats", ctypes.byref(geom), ctypes.byref(tq), ctypes.byref(tdo), nv.ptr(W),
            nv.ptr(tok[0]), nv.ptr(tok[1]), nv.ptr(tok[2]), nv.ptr(p_ml), nv.ptr(p_dkv), nv.stream())
    dkv = p_dkv.sum(1).contiguous()
    dksum = p_ml[..., 0].sum(1).contiguous()
    nv.call("ea_performer_bwd_k", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8),
            nv.ptr(W), nv.ptr(stab), nv.ptr(dkv), nv.ptr(dksum), ctypes.byref(tdk), ctypes.byref(tdv),
            nv.stream())
    return dqkv5


class PerformerAttnFn(torch.autograd.Function):
    """out[B,N,h,d] = phi(q) (phi(k)^T v) / clamp(phi(q) . sum phi(k), 1e-2) with positive random
    features W [h, m, d] (no gradient to W: the default sample scheme redraws / fixes it)
    (torch.ops.ea.performer_fwd / performer_bwd)."""

    @staticmethod
    def forward(ctx, qkv5, mask_u8, W):
        out, stab, kv, ksum = _ea_op("performer_fwd", performer_fwd_impl, qkv5, mask_u8, W)
        ctx.save_for_backward(qkv5, mask_u8, W, stab, kv, ksum, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv5, mask_u8, W, stab, kv, ksum, out = ctx.saved_tensors
        return _ea_op("performer_bwd", performer_bwd_impl, dout, qkv5, mask_u8, W, stab, kv, ksum, out), None, None


# ------------------------------------------------------------------------------------------
# ScatterBrain, low-rank half  (reference scatterbrain_attention.py:99-160)
# ------------------------------------------------------------------------------------------
SCATTER_TORCH = os.environ.get("EA_SCATTER_TORCH", "0") == "1"     # dev switch: feature half on torch ops


def scatter_supported(qkv5, W, attn_2d, seq_shape, window, ext_size=0):
    """The feature half has HIP kernels for d = 64, m <= 64 and query windows of <= 64 tokens; with window overlap
    (ext_size > 0) the key patch may be any size that follows from that, as long as it reaches the adjacent windows only."""
    B, N, _, h, d = qkv5.shape
    wq = window * window if attn_2d else window
    return d == 64 and W.shape[1] <= 64 and wq <= 64 and 0 <= ext_size <= window


def _sb_geom(qkv5, W, attn_2d, seq_shape, window):
    B, N, _, h, d = qkv5.shape
    gh, gw = (seq_shape if attn_2d else (1, N))
    return nv.ea_sb_geom(B, h, N, d, nv.io_dtype(qkv5), W.shape[1], 1 if attn_2d else 0, int(gh), int(gw), int(window))


def scatter_stats(geom, qkv5, mask_u8, W, ext_size=0):
    """Sequence-wide feature statistics of the keys: mx [BH,M], z_all [BH,M], S_all [BH,M,d] (fp32).  With window
    overlap the patches of the border windows hold padding slots with log phi = 0, which enter the stabiliser (the
    reference takes the maximum over the padded partition as well): mx >= log(M) / 2 in the kernels' scaling."""
    B, N, _, h, d = qkv5.shape
    BH, M, dev = B * h, W.shape[1], qkv5.device
    _, k, v = _qkv_views(qkv5)
    tk, tv = nv.t4(k), nv.t4(v)
    S = nv.lib().ea_scatter_parts(ctypes.byref(geom))
    p_ml = torch.empty((BH, S, M, 4), dtype=torch.float32, device=dev)
    nv.call("ea_scatter_kmax", ctypes.byref(geom), ctypes.byref(tk), nv.ptr(mask_u8), nv.ptr(W), nv.ptr(p_ml), nv.stream())
    mx = p_ml[..., 0].amax(1).contiguous()                                 # [BH, M]
    if ext_size > 0:
        mx = mx.clamp_(min=0.5 * math.log(M))
    p_kv = torch.empty((BH, S, M, d), dtype=torch.float32, device=dev)
    nv.call("ea_scatter_kv", ctypes.byref(geom), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(mask_u8), nv.ptr(W),
            nv.ptr(mx), nv.ptr(p_ml), nv.ptr(p_kv), nv.stream())
    return mx, p_ml[..., 0].sum(1).contiguous(), p_kv.sum(1).contiguous()


def scatter_feature_fwd(qkv5, mask_u8, W, o_loc, lse_loc, attn_2d, seq_shape, window, ext_size=0):
    """out [B,N,h,d] = merge of the window half (o_loc [B,N,h,d], lse_loc [B,h,N]) with the m feature columns;
    also returns r [B,h,N] and the statistics (for the backward).  ext_size > 0: overlapping windows (ea_scatter_ov_*)."""
    B, N, _, h, d = qkv5.shape
    W = W.float().contiguous()
    geom = _sb_geom(qkv5, W, attn_2d, seq_shape, window)
    mx, zall, sall = scatter_stats(geom, qkv5, mask_u8, W, ext_size)
    q, k, v = _qkv_views(qkv5)
    out = torch.empty((B, N, h, d), dtype=qkv5.dtype, device=qkv5.device)
    r = torch.empty((B, h, N), dtype=torch.float32, device=qkv5.device)
    lse_loc = lse_loc.float().contiguous()
    ts = [nv.t4(t) for t in (q, k, v, o_loc.permute(0, 2, 1, 3), out.permute(0, 2, 1, 3))]
    name, head = ("ea_scatter_ov_fwd", (ctypes.byref(geom), int(ext_size))) if ext_size > 0 else ("ea_scatter_fwd", (ctypes.byref(geom),))
    nv.call(name, *head, ctypes.byref(ts[0]), ctypes.byref(ts[1]), ctypes.byref(ts[2]),
            nv.ptr(mask_u8), nv.ptr(W), nv.ptr(mx), nv.ptr(zall), nv.ptr(sall), ctypes.byref(ts[3]), nv.ptr(lse_loc),
            ctypes.byref(ts[4]), nv.ptr(r), nv.stream())
    return out, r, (mx, zall, sall)


class ScatterFeatureFn(torch.autograd.Function):
    """ScatterBrain's feature half + the merge with the window half, on HIP (ea_scatter_*):
    (qkv5, o_loc [B,N,h,d], lse_loc [B,h,N], W [h,m,d]) -> out [B,N,h,d].  The backward returns the feature
    half's dq / dk / dv and the cotangents of the window half (d o_loc, d lse_loc), which flow on into
    LocalAttnLseFn; no gradient reaches W (redrawn / fixed, like PerformerAttnFn)."""

    @staticmethod
    def forward(ctx, qkv5, o_loc, lse_loc, mask_u8, W, attn_2d, seq_shape, window, ext_size=0):
        nv.require_cuda(qkv5, "qkv")
        out, r, (mx, zall, sall) = scatter_feature_fwd(qkv5, mask_u8, W, o_loc, lse_loc, attn_2d, seq_shape, window, ext_size)
        Wc = W.float().contiguous()
        ctx.save_for_backward(qkv5, o_loc, lse_loc.float().contiguous(), mask_u8, Wc, r, mx, zall, sall)
        ctx.geo = (attn_2d, tuple(seq_shape), window, int(ext_size))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv5, o_loc, lse_loc, mask_u8, W, r, mx, zall, sall = ctx.saved_tensors
        attn_2d, seq_shape, window, ext = ctx.geo
        B, N, _, h, d = qkv5.shape
        BH, M, dev = B * h, W.shape[1], qkv5.device
        geom = _sb_geom(qkv5, W, attn_2d, seq_shape, window)
        dout = dout.contiguous()
        dqkv5 = torch.empty_like(qkv5)
        d_oloc = torch.empty_like(o_loc)
        dlse = torch.empty_like(lse_loc)
        if ext > 0:
            # overlapping patches: the window pass leaves every window's statistics gradients in a workspace, the key pass
            # sums them per key over the windows whose patch holds it (stores only: the same bits on every run)
            G = nv.lib().ea_scatter_ov_windows(ctypes.byref(geom), ext)
            if G <= 0:
                raise RuntimeError("ea_scatter_ov_windows refused the geometry (%d)" % G)
            w_ds = torch.empty((BH, G, M, d), dtype=torch.float32, device=dev)
            w_dz = torch.empty((2, BH, G, M), dtype=torch.float32, device=dev)          # shares of d z_all | d z_win
            q, k, v = _qkv_views(qkv5)
            dq, dk, dv = _qkv_views(dqkv5)
            ts = [nv.t4(t) for t in (q, k, v, o_loc.permute(0, 2, 1, 3), dout.permute(0, 2, 1, 3), dq, dk, dv,
                                     d_oloc.permute(0, 2, 1, 3))]
            nv.call("ea_scatter_ov_bwd_window", ctypes.byref(geom), ext, ctypes.byref(ts[0]), ctypes.byref(ts[1]),
                    ctypes.byref(ts[2]), nv.ptr(mask_u8), nv.ptr(W), nv.ptr(mx), nv.ptr(zall), nv.ptr(sall), ctypes.byref(ts[3]),
                    nv.ptr(lse_loc), nv.ptr(r), ctypes.byref(ts[4]), ctypes.byref(ts[5]), ctypes.byref(ts[8]), nv.ptr(dlse),
                    nv.ptr(w_ds), nv.ptr(w_dz[0]), nv.ptr(w_dz[1]), nv.stream())
            dsall = w_ds.sum(1).contiguous()
            dzall = w_dz[0].sum(1).contiguous()
            nv.call("ea_scatter_ov_bwd_keys", ctypes.byref(geom), ext, ctypes.byref(ts[1]), ctypes.byref(ts[2]), nv.ptr(mask_u8),
                    nv.ptr(W), nv.ptr(mx), nv.ptr(dsall), nv.ptr(dzall), nv.ptr(w_ds), nv.ptr(w_dz[1]), ctypes.byref(ts[6]),
                    ctypes.byref(ts[7]), nv.stream())
            return dqkv5, d_oloc, dlse, None, None, None, None, None, None
        P = nv.lib().ea_scatter_bwd_parts(ctypes.byref(geom))
        p_ds = torch.empty((BH, P, M, d), dtype=torch.float32, device=dev)
        p_dz = torch.empty((BH, P, M), dtype=torch.float32, device=dev)
        q, k, v = _qkv_views(qkv5)
        dq, dk, dv = _qkv_views(dqkv5)
        ts = [nv.t4(t) for t in (q, k, v, o_loc.permute(0, 2, 1, 3), dout.permute(0, 2, 1, 3), dq, dk, dv,
                                 d_oloc.permute(0, 2, 1, 3))]
        nv.call("ea_scatter_bwd_window", ctypes.byref(geom), ctypes.byref(ts[0]), ctypes.byref(ts[1]), ctypes.byref(ts[2]),
                nv.ptr(mask_u8), nv.ptr(W), nv.ptr(mx), nv.ptr(zall), nv.ptr(sall), ctypes.byref(ts[3]), nv.ptr(lse_loc),
                nv.ptr(r), ctypes.byref(ts[4]), ctypes.byref(ts[5]), ctypes.byref(ts[6]), ctypes.byref(ts[7]),
                ctypes.byref(ts[8]), nv.ptr(dlse), nv.ptr(p_ds), nv.ptr(p_dz), nv.stream())
        dsall = p_ds.sum(1).contiguous()
        dzall = p_dz.sum(1).contiguous()
        nv.call("ea_scatter_bwd_global", ctypes.byref(geom), ctypes.byref(ts[1]), ctypes.byref(ts[2]), nv.ptr(mask_u8),
                nv.ptr(W), nv.ptr(mx), nv.ptr(dsall), nv.ptr(dzall), ctypes.byref(ts[6]), ctypes.byref(ts[7]), nv.stream())
        return dqkv5, d_oloc, dlse, None, None, None, None, None, None


# ---- Performer in exact fp32 arithmetic (ea_performer_f32_*; round 4) --------------------------------------
# The reference's linear attention is full precision whatever the AMP state (kernelized_attention.py:116-121,343-345);
# this is the default Performer core.  EA_PERFORMER_16BIT=1 selects the faster 16-bit-operand kernels above (phi rounded
# to bf16 / fp16 for the MFMA -- narrower than the reference).
PERFORMER_16BIT = os.environ.get("EA_PERFORMER_16BIT", "0") == "1"
_IO32 = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def performer_f32_supported(qkv5, W):
    return qkv5.is_cuda and qkv5.dtype in _IO32 and qkv5.shape[-1] == 64 and W.shape[1] <= 96 and W.shape[1] % 16 == 0


_PERFORMER_F32 = _fc.Family("ea_performer_f32_", "kmax", stats_take_q=False, q_side_stat=False, has_dw=False)


def _performer_f32_geom(qkv5, W):
    B, N, _, h, d = qkv5.shape
    return nv.ea_perf_geom(B, h, N, d, _IO32[qkv5.dtype], W.shape[1])


def performer_f32_fwd(qkv5, mask_u8, W):
    """-> out [B,N,h,d] (dtype of qkv5), p_max [BH,S], kv [BH,m,d], ksum [BH,m]."""
    nv.require_cuda(qkv5, "qkv")
    geom = _performer_f32_geom(qkv5, W)
    S = nv.lib().ea_performer_f32_parts(ctypes.byref(geom))
    if S <= 0:
        raise RuntimeError("ea_performer_f32_parts: %d" % S)
    return _fc.forward(_PERFORMER_F32, geom, S, W.shape[1], qkv5, mask_u8, W, ())


def performer_f32_bwd(dout, qkv5, mask_u8, W, p_max, kv, ksum):
    return _fc.backward(_PERFORMER_F32, _performer_f32_geom(qkv5, W), p_max.shape[1], W.shape[1], dout, qkv5, mask_u8, W,
                        p_max, kv, ksum)[0]


class PerformerF32Fn(torch.autograd.Function):
    """The Performer core in exact fp32 arithmetic on qkv of any I/O type (bf16 / fp16 under autocast, fp32 outside):
    out = phi(q) (phi(k)^T v) / clamp(phi(q) . sum phi(k), 1e-2); no gradient to the random features."""

    @staticmethod
    def forward(ctx, qkv5, mask_u8, W):
        out, p_max, kv, ksum = performer_f32_fwd(qkv5, mask_u8, W)
        ctx.save_for_backward(qkv5, mask_u8, W, p_max, kv, ksum)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv5, mask_u8, W, p_max, kv, ksum = ctx.saved_tensors
        return performer_f32_bwd(dout, qkv5, mask_u8, W, p_max, kv, ksum), None, None


def performer_attention(qkv5, mask_u8, proj):
    tracing = torch.compiler.is_compiling() or torch._C._len_torch_dispatch_stack() != 0
    # (while a graph is being traced the dispatcher ops torch.ops.ea.performer_fwd / _bwd -- the 16-bit kernels -- stay)
    if not PERFORMER_16BIT and (not tracing or qkv5.dtype == torch.float32) and performer_f32_supported(qkv5, proj):
        return PerformerF32Fn.apply(qkv5, mask_u8, proj)
    if qkv5.dtype == torch.float32:
        qkv5 = to_io_dtype(qkv5)
    return PerformerAttnFn.apply(qkv5, mask_u8, proj)


# ------------------------------------------------------------------------------------------
# projections: Linear with a split-K weight gradient
# ------------------------------------------------------------------------------------------
def _split_k(rows):
    """Slices for the weight-gradient reduction over `rows` tokens: the largest divisor of rows
    that is <= 64 and leaves >= 512 rows per slice (1 = no split)."""
    best = 1
    for s in range(2, 65):
        if rows % s == 0 and rows // s >= 512:
            best = s
    return best


def _colsum_raw(x2):
    rows, cols = x2.shape
    out = torch.empty(cols, dtype=torch.float32, device=x2.device)
    nv.call("ea_colsum_f32", rows, cols, nv.ptr(x2), nv.ptr(out), nv.stream())
    return out


COLSUM_TWO_STAGE = os.environ.get("EA_COLSUM_TWO_STAGE", "1") == "1"


def _colsum_fold(rows, cols):
    """k > 1: read a TALL [rows, cols] matrix as [rows / k, k * cols] (the same memory) -- ea_colsum_f32 gives a block 16
    columns, so a 768-column matrix of 9216 rows (the mu networks' feed buffer of the LM step) ran on 48 workgroups; folded by
    k = 32 it is 1536 workgroups, and the k partial rows [k, cols] take one more (tiny) launch.  Fixed order either way."""
    # (measured, tools/colsum_bench.py on one box, eager: 9216 x 768 20.9 -> 14.0 us, 65536 x 768 137 -> 62 us; below ~16 MB the
    #  second launch costs more than the first gains -- 4096 x 768: 6.0 us in one stage, 13.8 in two)
    if not COLSUM_TWO_STAGE or cols >= 8192 or rows * cols < (4 << 20):
        return 1
    best = 1
    for k in (64, 32, 16, 12, 8, 4):
        if rows % k == 0 and rows // k >= 64 and k * cols <= 32768:
            best = k
            break
    return best


def colsum_f32(x2):
    """x2.sum(0) of a contiguous fp32 [rows, cols] tensor through ea_colsum_f32 (fixed order); tall matrices in two
    stages (_colsum_fold)."""
    rows, cols = x2.shape
    k = _colsum_fold(rows, cols)
    if k > 1:
        return _colsum_raw(_colsum_raw(x2.view(rows // k, k * cols)).view(k, cols))
    return _colsum_raw(x2)


def colsum2_f32(x1, x2):
    """(x1.sum(0), x2.sum(0)) of two contiguous fp32 [rows, *] tensors with the same rows, ONE launch."""
    rows, c1 = x1.shape
    c2 = x2.shape[1]
    out = torch.empty(c1 + c2, dtype=torch.float32, device=x1.device)
    nv.call_as("ea_colsum_f32", "ea_colsum2_f32", rows, c1, nv.ptr(x1), nv.ptr(out), c2, nv.ptr(x2),
               ctypes.c_void_p(out.data_ptr() + 4 * c1), nv.stream())
    return out[:c1], out[c1:]


def bias_grad(dy2):
    """db = dY.sum(0) in fp32 through ea_bias_grad (dY: contiguous [rows, cols] bf16/fp16)."""
    rows, cols = dy2.shape
    if dy2.dtype not in (torch.bfloat16, torch.float16) or cols % 8 or cols > 16384 or not dy2.is_contiguous():
        return dy2.sum(0, dtype=torch.float32)
    nb = nv.lib().ea_bias_grad_parts(rows, cols)
    part = torch.empty(nb * cols, dtype=torch.float32, device=dy2.device)
    db = torch.empty(cols, dtype=torch.float32, device=dy2.device)
    nv.call("ea_bias_grad", 0 if dy2.dtype == torch.bfloat16 else 1, rows, cols, nv.ptr(dy2),
                 nv.ptr(part), nv.ptr(db), nv.stream())
    return db


_MM_OUT_DTYPE = [True]      # torch.mm(..., out_dtype=) available (library GEMM with fp32 output)


def _mm_out(a, b, out_dtype):
    """a @ b with the result in `out_dtype`.  For a low-precision product consumed in fp32 (the input
    gradient of a projection whose input is fp32) the library GEMM writes fp32 directly instead of
    bf16 + a separate cast pass over the activation-sized tensor."""
    if out_dtype == torch.float32 and a.dtype in (torch.bfloat16, torch.float16) and _MM_OUT_DTYPE[0]:
        try:
            return torch.mm(a, b, out_dtype=torch.float32)
        except (TypeError, RuntimeError, NotImplementedError):
            _MM_OUT_DTYPE[0] = False
    return (a @ b).to(out_dtype)


USE_DGRAD_RS = os.environ.get("EA_DGRAD_RS", "1") == "1"
DGRAD_RS_MIN_ROWS = int(os.environ.get("EA_DGRAD_RS_MIN_ROWS", "16384"))


def _dgrad_weight(wq, w16, wt, cdtype):
    """(weight operand of ea_linear_dgrad*, its kind: 0 = [576, 192] in cdtype, 1 = fp32 master, 2 = prepare_w192_t's image)."""
    if wt is not None and wt.dtype == cdtype and wt.is_contiguous() and wt.numel() == 576 * 192:
        return wt, 2
    w = w16 if (w16 is not None and w16.dtype == cdtype and w16.is_contiguous()) else wq
    return w, int(w.dtype == torch.float32)


def qkv_dgrad(dqkv2, wq, w16, xdtype, wt=None):
    """dx = dqkv2 @ W for the qkv projection (abstract_attention.py:72-78 differentiated) in `xdtype`.
    192-wide layers: ea_linear_dgrad (round 5) -- the weight resident in registers (the 16-bit copy the forward projection
    left, `w16`, its prepared transpose `wt`, or the fp32 master `wq` rounded on the way), the gradient rows through LDS once; no library GEMM and no cast
    kernel.  Other widths, tracing and small row counts: the library GEMM with an fp32 result."""
    rows, NO = dqkv2.shape
    cdtype = dqkv2.dtype
    K = wq.shape[1]
    direct = _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0
    if (USE_DGRAD_RS and direct and rows >= DGRAD_RS_MIN_ROWS and cdtype in _ELEM and xdtype in (torch.float32, cdtype)
            and tuple(wq.shape) == (NO, K) and dqkv2.stride(1) == 1 and dqkv2.stride(0) % 8 == 0
            and (w16 is not None or wq.dtype == torch.float32)
            and bool(nv.lib().ea_linear_dgrad_supported(K, NO))):
        w, w_kind = _dgrad_weight(wq, w16, wt, cdtype)
        if w.dtype in (torch.float32, cdtype) and w.is_contiguous():
            dx = torch.empty((rows, K), dtype=xdtype, device=dqkv2.device)
            label = "ea_linear_dgrad"
            if nv.KERNEL_TIMER.enabled:
                label = "ea_linear_dgrad[%d->%d,16->%s]" % (NO, K, "f32" if xdtype == torch.float32 else "16")
                _note_bytes(label, rows * (NO * 2 + K * dx.element_size()))
            nv.call_as(label, "ea_linear_dgrad", _ELEM[cdtype], rows, K, NO, nv.ptr(dqkv2), dqkv2.stride(0), nv.ptr(w),
                       w_kind, nv.ptr(dx), int(xdtype == torch.float32), K, nv.stream())
            return dx
    return _mm_out(dqkv2, w16 if w16 is not None else wq.to(cdtype), xdtype)


USE_DGRAD_FIN = os.environ.get("EA_DGRAD_FIN", "1") == "1"


def dgrad_finish_usable(dqkv2, wq, xdtype, heads, d):
    """ea_linear_dgrad_finish: 192-wide, three heads of 64 channels, contiguous 576-column gradient rows."""
    direct = _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0
    return (USE_DGRAD_FIN and USE_DGRAD_RS and direct and heads == 3 and d == 64 and dqkv2.dtype in _ELEM
            and xdtype in (torch.float32, dqkv2.dtype) and tuple(wq.shape) == (576, 192) and dqkv2.is_contiguous()
            and dqkv2.shape[0] >= DGRAD_RS_MIN_ROWS)


def qkv_dgrad_finish(dqkv2, qkv2, wq, w16, xdtype, fin, wt=None):
    """dx = dqkv2 @ W after the LAST corrections of the dq / dk columns of dqkv2 (in place) -- ea_linear_dgrad_finish, one pass:
    fin: a Finish (or its fields as a dict) -- LARA: from _lara_backward(defer_finish=True) (lara.py:223, 43,48,145-151
    differentiated); EVA: uq = qbar = lse_t = None, dpq / dpk = the chunk-mean gradients (eva.py:178-181)."""
    if isinstance(fin, dict):
        fin = Finish(**fin)
    rows = dqkv2.shape[0]
    cdtype = dqkv2.dtype
    w, w_kind = _dgrad_weight(wq, w16, wt, cdtype)
    if not (w.dtype in (torch.float32, cdtype) and w.is_contiguous()):
        w, w_kind = wq.to(cdtype).contiguous(), 0
    dx = torch.empty((rows, 192), dtype=xdtype, device=dqkv2.device)
    label = "ea_linear_dgrad_finish"
    if nv.KERNEL_TIMER.enabled:
        label = "ea_linear_dgrad_finish[576->192,16->%s%s]" % ("f32" if xdtype == torch.float32 else "16", ",+t" if fin.uq is not None else "")
        # dqkv read + dq, dk rewritten, dx written, q read for the t correction
        _note_bytes(label, rows * (576 * 2 + 384 * 2 + 192 * dx.element_size() + (192 * 2 if fin.uq is not None else 0)))
    nv.call_as(label, "ea_linear_dgrad_finish", _ELEM[cdtype], fin.B, fin.gh, fin.gw, fin.r, fin.C, fin.scale,
               nv.ptr(dqkv2), dqkv2.stride(0), nv.ptr(qkv2), 0 if qkv2 is None else qkv2.stride(0), nv.ptr(w),
               w_kind, nv.ptr(dx), int(xdtype == torch.float32), 192, nv.ptr(fin.qbar),
               nv.ptr(fin.uq), nv.ptr(fin.lse_t), nv.ptr(fin.dpq), nv.ptr(fin.dpk), nv.stream())
    return dx


def slice_sum(part):
    """part [S, ...] fp32 -> sum over S in a fixed order (ea_slice_sum)."""
    S = part.shape[0]
    n = part[0].numel()
    out = torch.empty(part.shape[1:], dtype=torch.float32, device=part.device)
    nv.call("ea_slice_sum", 1, S, n, 1.0, None, nv.ptr(part), nv.ptr(out), nv.stream())
    return out


USE_EA_LINEAR = os.environ.get("EA_LINEAR", "1") == "1"
LABEL_ALGO_BYTES = {}     # timer label -> [summed algorithmic bytes, launches] of the projection kernels (one label per shape)


def _note_bytes(label, nbytes):
    """bench.py's instrumented pass: algorithmic bytes of every launch timed under `label`, SUMMED -- the achieved rate of a
    label is summed bytes / summed time, never a maximum over one and a mean over the other."""
    rec = LABEL_ALGO_BYTES.setdefault(label, [0, 0])
    rec[0] += nbytes
    rec[1] += 1
_ELEM = {torch.bfloat16: 0, torch.float16: 1}


def _lin_geometry(K, NO):
    """Mirror of ea_linear_supported (ea_linear.hip): in in {64,128,192,256}; out = 1..4 parts of 64/128/192/256 columns whose
    weight rows fit 72 KB of LDS."""
    if K not in (64, 128, 192, 256):
        return False
    for ns in (1, 2, 3, 4):
        if NO % ns == 0 and NO // ns in (64, 128, 192, 256) and (NO // ns) * K * 2 <= 72 * 1024:
            return True
    return False


def _lin_rows_ok(a2, wdtype):
    """Activation-side requirements of ea_linear: row-contiguous [rows, in], 16-byte aligned rows, bf16 / fp16 / fp32."""
    return (USE_EA_LINEAR and a2.is_cuda and a2.dim() == 2 and a2.stride(1) == 1 and a2.stride(0) % 8 == 0
            and a2.shape[0] > 0 and (a2.storage_offset() * a2.element_size()) % 16 == 0
            and a2.dtype in (wdtype, torch.float32))


def ea_linear_supported(a2, w):
    """ea_linear: a [rows, in] (row-contiguous, bf16 / fp16 / fp32), w [out, in] contiguous in the 16-bit dtype."""
    return (w.dtype in _ELEM and w.is_contiguous() and _lin_rows_ok(a2, w.dtype)
            and _lin_geometry(w.shape[1], w.shape[0]))


def linear_impl(a2, w, bias32, y_f32, want_cast):
    """torch.ops.ea.linear: [y, rounded copy of a2 (empty unless asked for)]."""
    nv.require_cuda(a2, "a")
    y, ac = ea_linear(a2, w, bias32, torch.float32 if y_f32 else w.dtype, want_cast)
    return [y, ac if ac is not None else a2.new_empty(0, dtype=w.dtype)]


_ELEM_DT = [torch.bfloat16, torch.float16]


def linear_w32_impl(a2, w32, bias32, elem, transposed, y_f32, want_cast):
    """torch.ops.ea.linear_w32: the same product from the fp32 master weight (rounded while it is staged, no cast
    kernel); transposed: w32 is [in, out] and y = a2 @ w32 (the input gradient of the layer w32 belongs to)."""
    nv.require_cuda(a2, "a")
    dt = _ELEM_DT[int(elem)]
    y, ac = ea_linear(a2, w32, bias32, torch.float32 if y_f32 else dt, want_cast, elem_dtype=dt, transposed=bool(transposed))
    return [y, ac if ac is not None else a2.new_empty(0, dtype=dt)]


def ea_linear_w32_supported(a2, w32, dtype, transposed=False):
    """ea_linear_w32: fp32 contiguous weight, the 16-bit compute dtype `dtype`, activations as for ea_linear."""
    K, NO = (w32.shape[0], w32.shape[1]) if transposed else (w32.shape[1], w32.shape[0])
    return (dtype in _ELEM and w32.dtype == torch.float32 and w32.is_contiguous() and w32.dim() == 2
            and (w32.storage_offset() * 4) % 16 == 0 and _lin_rows_ok(a2, dtype) and a2.shape[1] == K and _lin_geometry(K, NO))


def ea_linear(a2, w, bias32, out_dtype, want_cast=False, elem_dtype=None, transposed=False):
    """y = a2 @ w.T (+ bias) by the streaming projection kernel (ea_linear.hip); fp32 `a2` is rounded to the compute
    dtype on the way in and, with want_cast, that rounded copy is returned as well.  With elem_dtype given, `w` is the
    fp32 master weight ([out, in], or [in, out] with transposed) and is rounded while it is staged (ea_linear_w32)."""
    rows, K = a2.shape
    w32 = elem_dtype is not None
    cdt = elem_dtype if w32 else w.dtype
    NO = w.shape[1] if (w32 and transposed) else w.shape[0]
    y = torch.empty((rows, NO), dtype=out_dtype, device=a2.device)
    a_f32 = a2.dtype == torch.float32
    a_cast = torch.empty((rows, K), dtype=cdt, device=a2.device) if (a_f32 and want_cast) else None
    label = "ea_linear"
    if nv.KERNEL_TIMER.enabled:
        # one label per shape; what the launch has to move: activations in, result out, the rounded copy when asked for
        # (the weight is noise)
        label = "ea_linear[%d->%d,%s->%s]" % (K, NO, "f32" if a_f32 else "16", "f32" if out_dtype == torch.float32 else "16")
        _note_bytes(label, rows * (K * a2.element_size() + NO * y.element_size() + (K * 2 if a_cast is not None else 0)))
    if w32:
        nv.call_as(label, "ea_linear_w32", _ELEM[cdt], rows, K, NO, nv.ptr(a2), int(a_f32), a2.stride(0), nv.ptr(w),
                   int(transposed), nv.ptr(bias32), nv.ptr(y), int(out_dtype == torch.float32), NO, nv.ptr(a_cast), nv.stream())
    else:
        nv.call_as(label, "ea_linear", _ELEM[cdt], rows, K, NO, nv.ptr(a2), int(a_f32), a2.stride(0), nv.ptr(w), nv.ptr(bias32),
                   nv.ptr(y), int(out_dtype == torch.float32), NO, nv.ptr(a_cast), nv.stream())
    return y, a_cast


def wgrad_supported(dy2, x2):
    """ea_wgrad takes contiguous bf16 / fp16 [rows, out] and [rows, in] with out, in multiples of 64."""
    return (dy2.is_cuda and dy2.dtype in (torch.bfloat16, torch.float16) and x2.dtype == dy2.dtype
            and dy2.shape[1] % 64 == 0 and x2.shape[1] % 64 == 0 and dy2.shape[0] >= 64)


# The hand-written one-pass weight + bias gradient (ea_wgrad): [192 x 192] tiles of dW per 8-wave workgroup, one workgroup
# per CU, dY read once and X once per 192 output channels; slice partials (dW and db side by side) added by ea_part_sum.
# 51 us / 31 us for the two cfg3 projections against 94 / 48 us for the library split-K GEMM + its reduction + the
# bias-gradient pass.  EA_WGRAD=0 switches back to the library path.
USE_WGRAD = os.environ.get("EA_WGRAD", "1") == "1"
# LinearRA as one autograd node (LaraModuleFn: CoreModuleFn around a LaraCore); EA_LARA_MODULE_FN=0 keeps the three nodes
USE_LARA_MODULE_FN = os.environ.get("EA_LARA_MODULE_FN", "1") == "1"


_WGRAD_PARTS = {}       # (rows, out, in) -> slice count of ea_wgrad (a pure function of the shape)


def wgrad(dy2, x2, with_bias=True, defer=False):
    """dW [out, in] = dY^T X and db [out] = dY.sum(0), both fp32, from one pass over dY and X (ea_wgrad:
    token slices x output tiles, slice partials summed in a fixed order)."""
    dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    rows, M = dy2.shape
    K = x2.shape[1]
    S = _WGRAD_PARTS.get((rows, M, K))
    if S is None:
        S = nv.lib().ea_wgrad_parts(rows, M, K)
        if S <= 0:
            raise RuntimeError("ea_wgrad_parts: %d" % S)
        if len(_WGRAD_PARTS) < 1024:
            _WGRAD_PARTS[(rows, M, K)] = S
    n = M * K + (M if with_bias else 0)
    part = torch.empty((S, n), dtype=torch.float32, device=dy2.device)      # slice s: dW partial, then db partial
    db_ptr = ctypes.c_void_p(part.data_ptr() + M * K * 4) if with_bias else None
    label = "ea_wgrad"
    if nv.KERNEL_TIMER.enabled:
        label = "ea_wgrad[%dx%d]" % (M, K)
        _note_bytes(label, rows * (M + K) * 2 + n * 4)
    nv.call_as(label, "ea_wgrad", nv.io_dtype(dy2), rows, M, K, nv.ptr(dy2), nv.ptr(x2), nv.ptr(part), db_ptr, n, nv.stream())
    if defer:
        return part, (M, K, with_bias)            # the caller adds the slices up (multi_sum: several reductions, one launch)
    out = torch.empty(n, dtype=torch.float32, device=dy2.device)
    nv.call("ea_part_sum", S, n, n, nv.ptr(part), nv.ptr(out), nv.stream())
    return _wgrad_split(out, (M, K, with_bias))


USE_WGRAD_PAIR = os.environ.get("EA_WGRAD_PAIR", "1") == "1"
_WGRAD_PAIR_PARTS = {}


def wgrad_pair_parts(rows, M1, K1, M2, K2):
    """Slice count of ea_wgrad_pair for the two products, or 0 when they cannot share a launch."""
    key = (rows, M1, K1, M2, K2)
    S = _WGRAD_PAIR_PARTS.get(key)
    if S is None:
        S = max(int(nv.lib().ea_wgrad_pair_parts(rows, M1, K1, M2, K2)), 0)
        if len(_WGRAD_PAIR_PARTS) < 1024:
            _WGRAD_PAIR_PARTS[key] = S
    return S


def wgrad_pair(dy1, x1, bias1, dy2, x2, bias2):
    """The weight (+ bias) gradients of two projections over the same token rows in ONE launch (ea_wgrad_pair) ->
    ((partials [S, n1], meta1), (partials [S, n2], meta2)), each as wgrad(..., defer=True) returns them: the caller adds the
    slices up (multi_sum).  A layer's qkv and output projections: 64 slices for the pair instead of 80 + 256 at cfg3 -- half
    the partial-sum traffic, one launch less."""
    dy1 = dy1 if dy1.is_contiguous() else dy1.contiguous()
    x1 = x1 if x1.is_contiguous() else x1.contiguous()
    dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    rows, M1 = dy1.shape
    K1 = x1.shape[1]
    M2, K2 = dy2.shape[1], x2.shape[1]
    S = wgrad_pair_parts(rows, M1, K1, M2, K2)
    if S <= 0:
        raise RuntimeError("ea_wgrad_pair_parts: the two products cannot share a launch")
    n1 = M1 * K1 + (M1 if bias1 else 0)
    n2 = M2 * K2 + (M2 if bias2 else 0)
    part1 = torch.empty((S, n1), dtype=torch.float32, device=dy1.device)
    part2 = torch.empty((S, n2), dtype=torch.float32, device=dy1.device)
    db1 = ctypes.c_void_p(part1.data_ptr() + M1 * K1 * 4) if bias1 else None
    db2 = ctypes.c_void_p(part2.data_ptr() + M2 * K2 * 4) if bias2 else None
    label = "ea_wgrad_pair"
    if nv.KERNEL_TIMER.enabled:
        label = "ea_wgrad_pair[%dx%d+%dx%d]" % (M1, K1, M2, K2)
        _note_bytes(label, rows * (M1 + K1 + M2 + K2) * 2 + (n1 + n2) * 4)
    nv.call_as(label, "ea_wgrad_pair", nv.io_dtype(dy1), rows, M1, K1, nv.ptr(dy1), nv.ptr(x1), nv.ptr(part1), db1, n1,
               M2, K2, nv.ptr(dy2), nv.ptr(x2), nv.ptr(part2), db2, n2, nv.stream())
    return (part1, (M1, K1, bool(bias1))), (part2, (M2, K2, bool(bias2)))


def wgrad_pair_usable(dy1, x1, dy2, x2):
    """Both products go through ea_wgrad and share their rows and tile edges."""
    return (USE_WGRAD_PAIR and x1 is not None and x2 is not None
            and wgrad_supported(dy1, x1) and wgrad_supported(dy2, x2) and dy1.shape[0] == dy2.shape[0]
            and wgrad_pair_parts(dy1.shape[0], dy1.shape[1], x1.shape[1], dy2.shape[1], x2.shape[1]) > 0)


def _wgrad_split(out, meta):
    M, K, with_bias = meta
    return out[:M * K].view(M, K), (out[M * K:] if with_bias else None)


def multi_sum(parts):
    """parts: up to six contiguous fp32 [S_k, n_k] tensors (n_k % 4 == 0) -> [sum over S_k] in ONE launch (ea_multi_sum)."""
    K = len(parts)
    outs = [torch.empty(p.shape[1], dtype=torch.float32, device=p.device) for p in parts]
    P = (ctypes.c_void_p * K)(*[p.data_ptr() for p in parts])
    O = (ctypes.c_void_p * K)(*[o.data_ptr() for o in outs])
    S = (ctypes.c_int32 * K)(*[p.shape[0] for p in parts])
    n = (ctypes.c_int32 * K)(*[p.shape[1] for p in parts])
    ld = (ctypes.c_int64 * K)(*[p.stride(0) for p in parts])
    nv.call("ea_multi_sum", K, P, S, n, ld, O, nv.stream())
    return outs


class LinearFn(torch.autograd.Function):
    """y = x W^T + b in the autocast dtype.  dW = dY^T X contracts over all B*N tokens with a
    [out, in] result of a few tiles: left to a single library GEMM it occupies ~9 of 256 CUs
    (rocprof: 425 us for 576x192x100352).  Here the token axis is cut into S slices run as one
    batched GEMM (S x as many workgroups) whose [S, out, in] partials are summed in fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias, dtype):
        x2 = x.reshape(-1, x.shape[-1])
        b32 = None if bias is None else (bias if bias.dtype == torch.float32 else bias.float())
        want = x2.dtype == torch.float32 and ctx.needs_input_grad[1]
        if weight.dtype == torch.float32 and dtype != torch.float32 and ea_linear_w32_supported(x2, weight, dtype):
            # streaming projection kernel fed by the fp32 MASTER weight: both autocast casts (of x and of the weight) are
            # folded into the kernel's loads -- no cast kernels in a training step
            y, xc = _ea_op("linear_w32", linear_w32_impl, x2, weight, b32, _ELEM[dtype], False, False, want)
            xl = x2 if x2.dtype == dtype else (xc if want else None)
            wl = weight
        else:
            bl_pre = None
            if (weight.dtype == torch.float32 and dtype in _ELEM and weight.is_cuda and bias is not None
                    and bias.dtype == torch.float32 and _DIRECT and not torch.compiler.is_compiling()
                    and torch._C._len_torch_dispatch_stack() == 0):
                wl, bl_pre = multi_cast([weight, bias], dtype)       # both autocast casts of the layer in one launch (round 6)
            else:
                wl = weight if weight.dtype == dtype else weight.to(dtype)
            if ea_linear_supported(x2, wl):
                # an fp32 x is rounded on the way in (no cast pass), its rounded copy comes back only when the weight
                # gradient will need it
                y, xc = _ea_op("linear", linear_impl, x2, wl, b32, False, want)
                xl = x2 if x2.dtype == dtype else (xc if want else None)
            else:
                xl = x2 if x2.dtype == dtype else x2.to(dtype)
                bl = bl_pre if bl_pre is not None else (None if bias is None else (bias if bias.dtype == dtype else bias.to(dtype)))
                y = F.linear(xl, wl, bl)
        ctx.save_for_backward(xl, wl)
        ctx.meta = (x.shape, x.dtype, weight.dtype, None if bias is None else bias.dtype, dtype)
        return y.view(x.shape[:-1] + (weight.shape[0],))

    @staticmethod
    def backward(ctx, dy):
        xl, wl = ctx.saved_tensors
        xshape, xdtype, wdtype, bdtype, cdtype = ctx.meta
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.dtype != cdtype:
            dy2 = dy2.to(cdtype)           # (xl is None when the weight is frozen and x arrived in fp32)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            y_f32 = xdtype == torch.float32
            if (wl.dtype == torch.float32 and cdtype != torch.float32 and xdtype in (torch.float32, cdtype)
                    and ea_linear_w32_supported(dy2, wl, cdtype, transposed=True)):
                # dX = dY W straight from the master weight [out, in] read as the transposed operand: no W^T copy, no cast
                dx = _ea_op("linear_w32", linear_w32_impl, dy2, wl, None, _ELEM[cdtype], True, y_f32, False)[0].view(xshape)
            else:
                wc = wl if wl.dtype == cdtype else wl.to(cdtype)
                # the launch is y = dY (W^T)^T: the geometry to validate is K = out, NO = in of the forward weight
                if (xdtype in (torch.float32, wc.dtype) and wc.dtype in _ELEM and _lin_geometry(wc.shape[0], wc.shape[1])
                        and _lin_rows_ok(dy2, wc.dtype) and wc.numel() * 2 <= 128 * 1024):
                    # dX = dY W as the same streaming kernel on the transposed weight: a [in, out] copy per backward, so only
                    # for weights of <= 128 KB (a pure 16-bit model has no fp32 master weight to read transposed;
                    # above the cap the library GEMM takes it without a copy)
                    dx = _ea_op("linear", linear_impl, dy2, wc.t().contiguous(), None, y_f32, False)[0].view(xshape)
                else:
                    # 576-deep (the qkv projection of a 192-wide layer): ea_linear_dgrad; other shapes: the library GEMM
                    dx = qkv_dgrad(dy2, wl, wc if wc is not wl else None, xdtype).view(xshape)
        need_w, need_b = ctx.needs_input_grad[1], (bdtype is not None and ctx.needs_input_grad[2])
        if need_w and xl is None:
            raise RuntimeError("LinearFn: the weight gradient was requested but the forward did not keep its input")
        if need_w and USE_WGRAD and wgrad_supported(dy2, xl):
            # one pass over dY and X: weight gradient (+ bias gradient riding along) -- ea_wgrad
            dw, db32 = wgrad(dy2, xl, need_b)
            dw = dw.to(wdtype)
            if need_b:
                db = db32.to(bdtype)
            return dx, dw, db, None
        if need_w:
            rows = xl.shape[0]
            S = _split_k(rows)
            if S > 1:
                dy3 = (dy2 if dy2.is_contiguous() else dy2.contiguous()).view(S, rows // S, -1)
                part = torch.bmm(dy3.transpose(1, 2), xl.view(S, rows // S, -1))     # [S, out, in]
                # the slices are added with fp32 accumulation and rounded once (one streaming reduction)
                dw = part.sum(0, dtype=torch.float32).to(wdtype)
            else:
                dw = (dy2.t() @ xl).to(wdtype)
        if need_b:
            db = bias_grad(dy2).to(bdtype)
        return dx, dw, db, None


_XTYPE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


class LayerNormFn(torch.autograd.Function):
    """F.layer_norm over the last axis of a [rows, C] matrix with fp32 statistics and fp32 output (ea_layernorm_fwd / _bwd):
    what torch computes for nn.LayerNorm under autocast on a 16-bit input.  The LayerNorm of LinearRA's 'dense' landmark
    generators (lara.py:34-44,64-71)."""

    @staticmethod
    def forward(ctx, x2, weight, bias, eps):
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        rows, C = x2.shape
        y = torch.empty((rows, C), dtype=torch.float32, device=x2.device)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=x2.device)
        w32, b32 = _f32c(weight), _f32c(bias)
        nv.call("ea_layernorm_fwd", _XTYPE[x2.dtype], rows, C, nv.ptr(x2), nv.ptr(w32), nv.ptr(b32), float(eps), nv.ptr(y),
                nv.ptr(stats), nv.stream())
        ctx.save_for_backward(x2, weight, stats)
        ctx.pd = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, weight, stats = ctx.saved_tensors
        rows, C = x2.shape
        dy = dy.float().contiguous()
        dx = torch.empty_like(x2)
        nb = int(nv.lib().ea_layernorm_parts(rows))
        part = torch.empty((nb, 2 * C), dtype=torch.float32, device=x2.device)
        nv.call("ea_layernorm_bwd", _XTYPE[x2.dtype], rows, C, nv.ptr(x2), nv.ptr(_f32c(weight)), nv.ptr(stats), nv.ptr(dy),
                nv.ptr(dx), nv.ptr(part), nv.stream())
        sums = colsum_f32(part)
        return dx, sums[:C].to(ctx.pd[0]), sums[C:].to(ctx.pd[1]), None


def layer_norm_supported(x, layer):
    """ea_layernorm_*: CUDA rows of C <= 1024 channels (C % 64 == 0), affine LayerNorm over the last axis, direct calls."""
    C = x.shape[-1]
    return (x.is_cuda and x.dtype in _XTYPE and C % 64 == 0 and C <= 1024 and layer.elementwise_affine and layer.bias is not None
            and tuple(layer.normalized_shape) == (C,) and x.numel() >= C
            and _DIRECT and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0)


def layer_norm(x, layer):
    """nn.LayerNorm(x) as torch evaluates it under autocast (fp32 statistics and output), through LayerNormFn where it applies."""
    # (outside autocast a 16-bit input gets a 16-bit result from torch: left to it)
    if not layer_norm_supported(x, layer) or (x.dtype != torch.float32 and not torch.is_autocast_enabled()):
        return layer(x)
    y = LayerNormFn.apply(x.reshape(-1, x.shape[-1]), layer.weight, layer.bias, layer.eps)
    return y.view(x.shape)


def linear(x, layer):
    """nn.Linear forward through LinearFn, in the autocast dtype when autocast is on."""
    if not x.is_cuda:
        return layer(x)
    return linear_wb(x, layer.weight, layer.bias)


class LinearPoolFn(torch.autograd.Function):
    """LinearFn for the qkv projection of a 192-wide three-head model on a 2-D token grid that ALSO returns the r x r pooled
    q / k rows (ea_linear_w32_pool; round 4): -> (qkv [B, N, 576], pooled_q, pooled_k [B*3, L, 64] fp32).  The pooled rows are
    non-differentiable hints for the attention core that consumes qkv: the core computes them itself otherwise
    (ea_eva_chunk_mean_fwd) and differentiates through the pooling in its own backward, so the gradient of this node is
    LinearFn's."""

    @staticmethod
    def forward(ctx, x, weight, bias, dtype, grid):
        B, H, W, r = grid
        x2 = x.reshape(-1, x.shape[-1])
        b32 = None if bias is None else (bias if bias.dtype == torch.float32 else bias.float())
        want = x2.dtype == torch.float32 and ctx.needs_input_grad[1]
        L = (H // r) * (W // r)
        pq = torch.empty((B * 3, L, 64), dtype=torch.float32, device=x.device)
        pk = torch.empty_like(pq)
        y, xc = project_qkv_pooled(x2, weight, b32, dtype, want, B, H, W, r, pq, pk)
        xl = x2 if x2.dtype == dtype else (xc if want else None)
        ctx.save_for_backward(xl, weight)
        ctx.meta = (x.shape, x.dtype, weight.dtype, None if bias is None else bias.dtype, dtype)
        ctx.mark_non_differentiable(pq, pk)
        return y.view(x.shape[:-1] + (weight.shape[0],)), pq, pk

    @staticmethod
    def backward(ctx, dy, _dpq, _dpk):
        return LinearFn.backward(ctx, dy) + (None,)


def linear_pool_usable(x, layer, grid, heads):
    """LinearPoolFn applies: autocast in a 16-bit dtype, fp32 master weight, the geometry ea_linear_w32_pool covers, and
    nobody tracing (the pooled rows travel outside the dispatcher ops)."""
    if not (x.is_cuda and torch.is_autocast_enabled() and _DIRECT and not torch.compiler.is_compiling()
            and torch._C._len_torch_dispatch_stack() == 0):
        return False
    dtype = torch.get_autocast_dtype("cuda")
    B, H, W, r = grid
    x2 = x.reshape(-1, x.shape[-1])
    return (dtype in _ELEM and x2.dtype in (torch.float32, dtype) and layer.weight.is_contiguous()
            and _lin_rows_ok(x2, dtype) and proj_pool_supported(x2, layer.weight, dtype, B, H, W, r, heads))


def multi_cast_into(srcs, dsts, dtype):
    """fp32 tensors -> `dtype` copies written into caller-provided contiguous destinations (slices of one stacked buffer), ONE
    launch (ea_multi_cast)."""
    K = len(srcs)
    srcs = [t.detach() if t.is_contiguous() else t.detach().contiguous() for t in srcs]
    src = (ctypes.c_void_p * K)(*[t.data_ptr() for t in srcs])
    dst = (ctypes.c_void_p * K)(*[o.data_ptr() for o in dsts])
    n = (ctypes.c_int64 * K)(*[t.numel() for t in srcs])
    nv.call("ea_multi_cast", _ELEM[dtype], K, src, n, dst, nv.stream())


USE_STACKED_LINEAR = os.environ.get("EA_STACKED_LINEAR", "1") == "1"


def stacked_linear_usable(x, weights, biases, dtype):
    """StackedLinearFn applies: a layer whose projection LinearFn would hand to the library GEMM anyway (widths outside
    ea_linear's 64 .. 256 input channels), fp32 master weights / biases of one width on the GPU, a 16-bit autocast dtype, the
    one-pass weight gradient, nobody tracing."""
    if not (USE_STACKED_LINEAR and USE_WGRAD and _DIRECT and x.is_cuda and dtype in _ELEM
            and not torch.compiler.is_compiling() and torch._C._len_torch_dispatch_stack() == 0):
        return False
    K = x.shape[-1]
    outs = sum(w.shape[0] for w in weights)
    has_b = [b is not None for b in biases]
    return (all(w.dtype == torch.float32 and w.dim() == 2 and w.shape[1] == K and w.is_cuda for w in weights)
            and (all(has_b) or not any(has_b)) and all(b is None or b.dtype == torch.float32 for b in biases)
            and len(weights) * (2 if all(has_b) else 1) <= 8
            and not _lin_geometry(K, outs) and K % 64 == 0 and all(w.shape[0] % 64 == 0 for w in weights)
            and x.dtype in (torch.float32, dtype) and x.numel() // K >= 64)


class StackedLinearFn(torch.autograd.Function):
    """y = x [W_1; W_2; ...]^T + [b_1; b_2; ...] for the separate fp32 master weights of ONE fused projection (causal EVA's
    q_proj / k_proj / v_proj, causal_eva.py:511-513) on the library GEMM: the 16-bit stacked operand is written by one
    ea_multi_cast launch straight into the slices of one buffer -- `torch.cat` of the masters (12.6 MB read + written at
    C = 1024) followed by the cast of the copy was two launches and twice the bytes -- and the weight gradient of the stack
    leaves as views of one [sum out, in] result (ea_wgrad, bias gradient riding along).
    args: x [..., in], compute dtype, n, then n weights and n biases (all None or all given)."""

    @staticmethod
    def forward(ctx, x, dtype, n, *wb):
        ws, bs = list(wb[:n]), list(wb[n:])
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        outs = [w.shape[0] for w in ws]
        tot = sum(outs)
        w16 = torch.empty((tot, K), dtype=dtype, device=x.device)
        has_b = bs[0] is not None
        b16 = torch.empty((tot,), dtype=dtype, device=x.device) if has_b else None
        dsts, o = [], 0
        for m in outs:
            dsts.append(w16[o:o + m])
            o += m
        if has_b:
            o = 0
            for m in outs:
                dsts.append(b16[o:o + m])
                o += m
        multi_cast_into(ws + (bs if has_b else []), dsts, dtype)
        xl = x2 if x2.dtype == dtype else x2.to(dtype)          # the one activation-sized cast of the layer
        xl = xl if xl.is_contiguous() else xl.contiguous()
        with torch.autocast(device_type="cuda", enabled=False):
            y = F.linear(xl, w16, b16)
        ctx.save_for_backward(xl, w16)
        ctx.meta = (x.shape, x.dtype, [w.dtype for w in ws], [None if b is None else b.dtype for b in bs], dtype, outs)
        return y.view(x.shape[:-1] + (tot,))

    @staticmethod
    def backward(ctx, dy):
        xl, w16 = ctx.saved_tensors
        xshape, xdtype, wdts, bdts, cdtype, outs = ctx.meta
        n = len(outs)
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.dtype != cdtype:
            dy2 = dy2.to(cdtype)
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = qkv_dgrad(dy2, w16, w16, xdtype).view(xshape)
        need_w = any(ctx.needs_input_grad[3:3 + n])
        need_b = bdts[0] is not None and any(ctx.needs_input_grad[3 + n:3 + 2 * n])
        dws, dbs = [None] * n, [None] * n
        if need_w:
            dw, db32 = wgrad(dy2, xl, need_b)
            o = 0
            for i, m in enumerate(outs):
                dws[i] = dw[o:o + m].to(wdts[i])
                if need_b:
                    dbs[i] = db32[o:o + m].to(bdts[i])
                o += m
        elif need_b:
            db32 = bias_grad(dy2)
            o = 0
            for i, m in enumerate(outs):
                dbs[i] = db32[o:o + m].to(bdts[i])
                o += m
        return (dx, None, None) + tuple(dws) + tuple(dbs)


def linear_stacked(x, layers):
    """The fused projection of several nn.Linear layers over the same input (-> [..., sum out]); None when StackedLinearFn
    does not apply (the caller then stacks the parameters itself)."""
    if not torch.is_autocast_enabled():
        return None
    dtype = torch.get_autocast_dtype("cuda")
    ws, bs = [l.weight for l in layers], [l.bias for l in layers]
    if not stacked_linear_usable(x, ws, bs, dtype):
        return None
    return StackedLinearFn.apply(x, dtype, len(ws), *ws, *bs)


def linear_wb(x, weight, bias):
    """F.linear(x, weight, bias) through LinearFn, in the autocast dtype when autocast is on."""
    if torch.is_autocast_enabled():
        dtype = torch.get_autocast_dtype("cuda")
    else:
        dtype = x.dtype
    return LinearFn.apply(x, weight, bias, dtype)
