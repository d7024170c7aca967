"""Causal softmax self-attention for autoregressive language modelling, MI355X build: the baseline causal EVA is compared
against.

The reference builds decoder self-attention as `causal_eva` or as fairseq's stock MultiheadAttention under the future mask
(fairseq/modules/transformer_layer.py:295-321).  This module is the second one, under fairseq's member names (`q_proj`,
`k_proj`, `v_proj`, `out_proj`; the `self_attn.*` keys of a reference softmax-LM checkpoint load with strict=True) and with
its initialisation, time-first `forward(query, key, value, key_padding_mask=None, incremental_state=None, ...) -> (out, None)`.

The core runs in libea_hip.so (csrc/ea_softmax_causal.hip through `_ops.CausalSoftmaxAttnFn`): causality is built into the
kernels' schedule, no [T, T] mask or score tensor exists, attention dropout is a keep mask drawn here and applied in the kernels.
There is no CPU fallback.  Not built (NotImplementedError): token-by-token decoding with an incremental state, quantization
noise, cross attention, fp32 activations outside autocast.  A query whose visible keys are all padded (left padding) gives NaN,
as in the reference.
"""
import math

import torch
import torch.nn as nn

from . import _ops


class CausalSoftmaxAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, dropout=0.0, bias=True, self_attention=True, q_noise=0.0, qn_block_size=8):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.dropout_module = nn.Dropout(dropout)       # holds p (fairseq reads it); applied inside the kernels
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.scaling = self.head_dim ** -0.5
        self.self_attention = self_attention
        self.q_noise, self.qn_block_size = float(q_noise), int(qn_block_size)
        self.k_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.v_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.reset_parameters()
        self._keep_mask_fn = None                       # tests: the keep decisions of a fixture instead of bernoulli_

    def reset_parameters(self):
        """CausalEVAttention's (fairseq's, for equal q / k / v sizes): xavier with gain 1 / sqrt(2) on q / k / v."""
        for proj in (self.k_proj, self.v_proj, self.q_proj):
            nn.init.xavier_uniform_(proj.weight, gain=1 / math.sqrt(2))
        nn.init.xavier_uniform_(self.out_proj.weight)
        if self.out_proj.bias is not None:
            nn.init.constant_(self.out_proj.bias, 0.0)

    @staticmethod
    def _is_future_mask(attn_mask, T):
        """The standard future mask: [T, T] (or larger, as fairseq caches it), -inf (float) or True (bool) strictly above the
        diagonal and 0 / False elsewhere."""
        if attn_mask.dim() != 2 or attn_mask.shape[0] < T or attn_mask.shape[1] < T:
            return False
        m = attn_mask[:T, :T]
        above = torch.ones(T, T, dtype=torch.bool, device=m.device).triu(1)
        blocked = m if m.dtype == torch.bool else torch.isneginf(m)
        free = ~m if m.dtype == torch.bool else m == 0
        return bool((blocked == above).all()) and bool((free == ~above).all())

    def _attn_keep(self, B, N, device):
        """Attention dropout on the [B, h, N, N] probabilities: the Bernoulli keep decisions are drawn here, one per
        (query, key) as the softmax baseline module draws them, and applied inside the kernels -> (keep, 1/(1-p)) or ()."""
        p = self.dropout_module.p
        if not (self.training and p > 0):
            return ()
        if p >= 1:
            raise NotImplementedError("attention dropout with p = 1")
        ld = -(-N // 64) * 64
        if self._keep_mask_fn is not None:
            keep = self._keep_mask_fn((B, self.num_heads, N, N)).to(device=device, dtype=torch.uint8)
            if ld != N:
                keep = torch.nn.functional.pad(keep, (0, ld - N))
        else:
            keep = torch.empty((B, self.num_heads, N, ld), device=device, dtype=torch.uint8).bernoulli_(1 - p)
        return (keep.contiguous(), 1.0 / (1.0 - p))

    def _project(self, x):
        """Time-first [T, B, C] -> the fused [T, B, 3, h, d] of the three projections, in the kernels' I/O dtype."""
        T, B, _ = x.shape
        layers = [self.q_proj, self.k_proj, self.v_proj]
        qkv = _ops.linear_stacked(x, layers) if torch.is_grad_enabled() else None
        if qkv is None:
            bias = None if self.q_proj.bias is None else torch.cat([l.bias for l in layers], 0)
            qkv = _ops.linear_wb(x, torch.cat([l.weight for l in layers], 0), bias)
        return qkv.reshape(T, B, 3, self.num_heads, self.head_dim)

    def forward(self, query, key, value, key_padding_mask=None, incremental_state=None, need_weights=False, attn_mask=None):
        """query/key/value: Time x Batch x Channel (self-attention: the same tensor); key_padding_mask: [B, T], 1 = pad.
        attn_mask: None or the standard future mask (causality is built in; anything else raises).
        Returns (out [T, B, C], None)."""
        if incremental_state is not None:
            raise NotImplementedError("softmax decoding is not built: CausalSoftmaxAttention has no incremental state "
                                      "(KV-cache decoding); run the full causal path")
        if self.q_noise > 0:
            raise NotImplementedError("quantization noise (q_noise > 0) is not built for CausalSoftmaxAttention")
        if not self.self_attention or (key is not None and key is not query) or (value is not None and value is not query):
            raise NotImplementedError("cross attention is not built: CausalSoftmaxAttention is decoder self-attention "
                                      "(query, key and value are the same tensor)")
        if need_weights:
            raise NotImplementedError("need_weights: the streaming kernels never form the attention weights")
        T, B, C = query.shape
        assert C == self.embed_dim, "query dim %d != %d" % (C, self.embed_dim)
        if not query.is_cuda:
            raise RuntimeError("CausalSoftmaxAttention runs on HIP kernels only: there is no CPU fallback")
        if attn_mask is not None and not self._is_future_mask(attn_mask, T):
            raise ValueError("attn_mask must be None or the standard future mask: causality is built into the kernels")
        qkv5 = self._project(query)
        if qkv5.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError("fp32 activations outside autocast: the causal softmax kernels take bf16 / fp16 operands "
                                      "(fp32 accumulation and softmax); run under torch.autocast")
        if self.head_dim not in (32, 64, 128):
            raise NotImplementedError("head dim %d: the causal softmax kernels are built for 32, 64 and 128" % self.head_dim)
        qkv5 = qkv5.transpose(0, 1)                       # [B, T, 3, h, d] view of the time-first buffer
        mask = _ops._mask_u8(key_padding_mask, B, T, query.device)
        out = _ops.CausalSoftmaxAttnFn.apply(qkv5, mask, *self._attn_keep(B, T, query.device))
        y = _ops.linear(out.transpose(0, 1).reshape(T, B, C), self.out_proj)
        if not torch.is_autocast_enabled() and y.dtype != query.dtype:
            y = y.to(query.dtype)
        return y.contiguous(), None
