"""Causal softmax self-attention for autoregressive language modelling, MI355X build: the baseline causal EVA is compared
against.

The reference builds decoder self-attention as `causal_eva` or as fairseq's stock MultiheadAttention under the future mask
(fairseq/modules/transformer_layer.py:295-321).  This module is the second one, under fairseq's member names (`q_proj`,
`k_proj`, `v_proj`, `out_proj`; the `self_attn.*` keys of a reference softmax-LM checkpoint load with strict=True) and with
its initialisation, time-first `forward(query, key, value, key_padding_mask=None, incremental_state=None, ...) -> (out, None)`.

The core runs in libea_hip.so (csrc/ea_softmax_causal.hip through `_ops.CausalSoftmaxAttnFn`): causality is built into the
kernels' schedule, no [T, T] mask or score tensor exists, attention dropout is a keep mask drawn here and applied in the kernels.
There is no CPU fallback.  Incremental decoding runs on a static, graph-capturable KV cache made by `init_kv_cache`
(csrc/ea_softmax_decode.hip); an incremental state without one raises.  Not built (NotImplementedError): quantization
noise, cross attention, fp32 activations outside autocast, and for decoding a rolling or windowed cache and fp32 caches
(follow-ups).  A query whose visible keys are all padded (left padding) gives NaN,
as in the reference.
"""
import ctypes
import inspect
import math
import numbers
import uuid

import torch
import torch.nn as nn

from . import _ops
from ._ceva_decode import CevaDecoding, _LINEAR_MAX_ROWS, _SPLIT_MAX_PARTS, _SPLIT_MAX_STEP

# what a beam reorder permutes: the rest is step-invariant, and so are the counters unless the state counts per row
_KV_BATCH_FIRST = ("kv", "pad")
_PER_SEQUENCE = ("pos", "status", "ntok")


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
        self._incremental_state_id = str(uuid.uuid4())  # fairseq's protocol: this module's own key of an incremental state

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
            buf = self._get_input_buffer(incremental_state)
            if "kv" not in buf:
                raise NotImplementedError("softmax decoding is not built for an incremental state without a KV cache: "
                                          "CausalSoftmaxAttention has no grown-on-demand state; make it with init_kv_cache")
            return self._decode(query, key, value, key_padding_mask, incremental_state, buf, need_weights, attn_mask)
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

    # ---- incremental decoding on a static KV cache ------------------------------------------------------------------------------
    def _get_input_buffer(self, incremental_state):
        found = (incremental_state or {}).get(self._incremental_state_id + ".kv_state")
        return {} if found is None else found

    def _kv_buffer(self, incremental_state, what):
        buf = self._get_input_buffer(incremental_state)
        if "kv" not in buf:
            raise RuntimeError("%s needs a KV cache (init_kv_cache); this incremental state holds none" % what)
        return buf

    # what a state that holds its projections shares with CausalEVAttention's: the checks, the copies and the two launches
    _check_hold_projections = CevaDecoding._check_hold_projections
    _load_held_projections = CevaDecoding._load_held_projections
    _held_x = staticmethod(CevaDecoding._held_x)
    _held_linear = CevaDecoding._held_linear
    _held_gemm = CevaDecoding._held_gemm
    decoding_state_nbytes = CevaDecoding.decoding_state_nbytes
    static_decoding_overflowed = CevaDecoding.static_decoding_overflowed

    def init_kv_cache(self, incremental_state, batch_size, max_tokens, dtype, device, kv_splits=0, hold_projections=False, *,
                      per_sequence=False):
        """Allocate, once, every buffer a decoding step touches, under this module's key of `incremental_state`: every later
        `forward(..., incremental_state=incremental_state)` is then a decoding step of T_new tokens -- a prompt, a piece of one,
        a single token -- that can be captured into a graph and replayed: the token count lives in device memory, the kernels
        read and advance it, nothing is read back and nothing is allocated but the step's outputs.
            kv        [B, 2, h, cap, d]   `dtype` (bf16 or fp16), cap = max_tokens: a head's keys, and its values, are one stream
            pad       [B, cap]            uint8, 1 = padded key
            pos       [1]                 int32 on the device: tokens decoded so far (one count for the whole batch)
            status    [1]                 int32 on the device: 1 once a step would have passed cap
            ntok      [B]                 int32, per_sequence only: the tokens each row took from the last step (written by it)
            split_ws  [B, h, 8, P, d + 4] fp32, with P > 1: the partials of a step of at most 8 tokens (scratch)
        A step is the projection, ea_softmax_sdecode_append, the attention, ea_softmax_sdecode_advance and out_proj.  The
        attention of a step of at most 8 tokens is ea_softmax_sdecode_attn_split, P workgroups per (b, h) sharing the cache's
        64-key tiles (with P > 1 followed by ea_softmax_sdecode_merge); a longer step runs ea_softmax_sdecode_attn_mm on the
        matrix cores.  `kv_splits` is P: 0 takes ea_softmax_sdecode_parts' choice for this device, an int in [1, 64] fixes it.
        The last T_new columns of `key_padding_mask`, in either of fairseq's shapes, are the step's flags.  A step that does
        not fit writes nothing, sets `status` and returns NaN rows (`static_decoding_overflowed`); eagerly it raises first.
        `hold_projections=True`: the state also holds 16-bit `w_qkv`, `b_qkv`, `w_out`, `b_out` and `proj_rows [64, 3 C]`, as
        CausalEVAttention's states do; a step of at most 64 rows runs both projections on ea_ceva_sdecode_linear, a larger
        one the library GEMM on the held operands; `refresh_decoding_weights` re-reads them.
        `per_sequence=True` (keyword-only; combines with `kv_splits` and `hold_projections`): `pos` and `status` are [B], every
        batch row has its own count, as in CausalEVAttention's per-sequence states.  Of a step's T_new positions a row takes
        those before its first flag in the step's `key_padding_mask` columns -- all without one, none when the first is
        flagged: the row sits the step out -- so ragged prompts are prefilled right-padded, a finished row idles, and
        `reset_decoding_rows` hands a row to a new sequence while a captured step keeps replaying.  Nothing is stored for the
        other positions and their output rows are zero (before out_proj: its bias alone behind it).  Overflow is per row and
        reported by `status` only: the host does not know the counts, so an eager step does not raise.  A row's outputs are
        bit for bit those of the row decoded alone.  The step issues the `_seq` entry points.
        Refuses fp32 caches, CPU devices, training mode, q_noise > 0 and head dims outside 32 / 64 / 128.  A rolling or
        windowed cache and fp32 decoding are follow-ups."""
        nv = _ops.nv
        if not self.self_attention:
            raise NotImplementedError("incremental decoding of encoder-decoder attention")
        if self.training:
            raise NotImplementedError("incremental decoding in training mode")
        if self.q_noise > 0:
            raise NotImplementedError("quantization noise (q_noise > 0) is not built for CausalSoftmaxAttention")
        if self.head_dim not in (32, 64, 128):
            raise NotImplementedError("head dim %d: the softmax decoding kernels are built for 32, 64 and 128" % self.head_dim)
        if dtype == torch.float32:
            raise NotImplementedError("fp32 decoding is not built for CausalSoftmaxAttention (a follow-up): the KV cache holds "
                                      "bf16 or fp16 rows")
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("the KV cache holds bf16 or fp16 rows, not %s" % (dtype,))
        if not isinstance(per_sequence, bool):
            raise TypeError("per_sequence must be a bool, got %r" % (per_sequence,))
        device = torch.device(device)
        nv.require_cuda(torch.empty(0, device=device), "the KV cache")
        B, cap = int(batch_size), int(max_tokens)
        if B <= 0 or cap <= 0:
            raise ValueError("the KV cache needs batch_size > 0 and max_tokens > 0, got %d, %d" % (B, cap))
        P = kv_splits
        if isinstance(P, bool) or not isinstance(P, numbers.Integral) or not 0 <= P <= _SPLIT_MAX_PARTS:
            raise ValueError("kv_splits must be 0 (the planner's choice) or an int in [1, %d], got %r" % (_SPLIT_MAX_PARTS, P))
        self._check_hold_projections(hold_projections, dtype)
        h, d, C = self.num_heads, self.head_dim, self.embed_dim
        if P == 0:
            with torch.cuda.device(device):
                P = nv.lib().ea_softmax_sdecode_parts(B, h, cap, 0)
            if P < 1:
                raise RuntimeError("ea_softmax_sdecode_parts refused (%d, %d, %d): %d" % (B, h, cap, P))
        state = {
            "kv": torch.zeros((B, 2, h, cap, d), dtype=dtype, device=device),
            "pad": torch.zeros((B, cap), dtype=torch.uint8, device=device),
            "pos": torch.zeros((B if per_sequence else 1,), dtype=torch.int32, device=device),
            "status": torch.zeros((B if per_sequence else 1,), dtype=torch.int32, device=device),
        }
        if per_sequence:
            state["ntok"] = torch.zeros((B,), dtype=torch.int32, device=device)
        if P > 1:
            state["split_ws"] = torch.zeros((B, h, _SPLIT_MAX_STEP, P, d + 4), dtype=torch.float32, device=device)
        if hold_projections:
            qkv_b, out_b = self.q_proj.bias is not None, self.out_proj.bias is not None
            state["proj_rows"] = torch.zeros((_LINEAR_MAX_ROWS, 3 * C), dtype=dtype, device=device)
            state["w_qkv"] = torch.empty((3 * C, C), dtype=dtype, device=device)
            state["b_qkv"] = torch.empty((3 * C,), dtype=dtype, device=device) if qkv_b else None
            state["w_out"] = torch.empty((C, C), dtype=dtype, device=device)
            state["b_out"] = torch.empty((C,), dtype=dtype, device=device) if out_b else None
            self._load_held_projections(state)
        incremental_state[self._incremental_state_id + ".kv_state"] = state
        # host side: the shadow count of EAGER steps (a replay advances only the device count), for the eager overflow check
        # (a per-sequence state: the host does not know the counts, overflow is reported by the device flags only)
        static = {"count": 0, "kv_splits": P}
        if per_sequence:
            static["per_sequence"] = True
        incremental_state[self._incremental_state_id + ".kv_static"] = static
        return incremental_state
    # (the reported parameter list stays the positional interface: callers that pin it see what they saw, as with the options
    #  of CausalEVAttention's init_*_decoding)
    init_kv_cache.__signature__ = inspect.signature(init_kv_cache).replace(
        parameters=list(inspect.signature(init_kv_cache).parameters.values())[:-1])

    def refresh_decoding_weights(self, incremental_state):
        """Re-read the projection parameters into what a state made with `hold_projections=True` holds of them, in place and by
        device ops only: a step captured before sees the new weights.  A state that holds none has nothing to refresh."""
        buf = self._kv_buffer(incremental_state, "refresh_decoding_weights")
        if "w_qkv" in buf:
            self._load_held_projections(buf)
        return incremental_state

    def reorder_incremental_state(self, incremental_state, new_order):
        """Permute the batch rows of `kv` and `pad` (a per-sequence state: and of `pos`, `status` and `ntok`), in place: the
        pointers a captured step holds stay valid."""
        buf = self._get_input_buffer(incremental_state)
        for k in _KV_BATCH_FIRST + (_PER_SEQUENCE if "ntok" in buf else ()) if "kv" in buf else ():
            buf[k].copy_(buf[k].index_select(0, new_order))
        return incremental_state

    def reset_decoding_rows(self, incremental_state, rows):
        """Restart batch rows: `pos` and `status` of `rows` back to 0, in place and by device ops only; no cache byte is
        cleared, nothing at or past a row's count is ever read.  A per-sequence state takes any subset (a sequence of ints or
        an integer tensor; a device tensor makes the reset itself capturable), between replays of a captured step: the next
        tokens of those rows are a new sequence's.  With one token count for the whole batch `rows` must name every batch
        row or be empty; a subset needs a state made with `per_sequence=True`."""
        buf = self._kv_buffer(incremental_state, "reset_decoding_rows")
        if "ntok" in buf:
            idx = torch.as_tensor(rows, device=buf["pos"].device).reshape(-1).long()
            buf["pos"].index_fill_(0, idx, 0)
            buf["status"].index_fill_(0, idx, 0)
            return incremental_state
        idx = sorted(set(torch.as_tensor(rows).reshape(-1).tolist()))
        if not idx:
            return incremental_state
        if idx != list(range(buf["kv"].shape[0])):
            raise NotImplementedError("reset_decoding_rows of a subset of the batch: the KV cache has one token count for the "
                                      "whole batch (per-sequence counts: init_kv_cache(per_sequence=True))")
        buf["pos"].zero_()
        buf["status"].zero_()
        incremental_state[self._incremental_state_id + ".kv_static"]["count"] = 0
        return incremental_state

    def decoding_positions(self, incremental_state):
        """The tokens decoded so far per batch row, a [B] int32 copy on the host (a shared-count state: its one count
        repeated).  Reads back."""
        buf = self._kv_buffer(incremental_state, "decoding_positions")
        return buf["pos"].expand(buf["kv"].shape[0]).cpu().clone()

    def decoding_positions_tensor(self, incremental_state):
        """The device tensor the state counts in -- `pos [1]` int32, or `[B]` on a per-sequence state -- itself: no read-back,
        a captured step may index with it."""
        return self._kv_buffer(incremental_state, "decoding_positions_tensor")["pos"]

    def _decode(self, query, key, value, key_padding_mask, incremental_state, state, need_weights, attn_mask):
        """One decoding step on the state of `init_kv_cache`: query [T_new, B, C] -> (out [T_new, B, C], None)."""
        nv = _ops.nv
        if self.training:
            raise NotImplementedError("incremental decoding in training mode")
        if not self.self_attention or (key is not None and key is not query) or (value is not None and value is not query):
            raise NotImplementedError("incremental decoding of encoder-decoder attention")
        if need_weights:
            raise NotImplementedError("need_weights: the decoding kernels never form the attention weights")
        if attn_mask is not None:
            raise ValueError("attn_mask in a decoding step: causality against the cache is built into the kernels")
        nv.require_cuda(query, "query")
        T_new, B, C = query.shape
        kv, pad = state["kv"], state["pad"]
        h, d, cap = self.num_heads, self.head_dim, kv.shape[3]
        if kv.shape[0] != B:
            raise RuntimeError("the KV cache holds batch %d, the step has %d" % (kv.shape[0], B))
        if key_padding_mask is not None and (key_padding_mask.dim() != 2 or key_padding_mask.shape[0] != B
                                             or key_padding_mask.shape[1] < T_new):
            raise ValueError("key_padding_mask %s does not cover the %d new positions of a batch of %d"
                             % (tuple(key_padding_mask.shape), T_new, B))
        static = incremental_state[self._incremental_state_id + ".kv_static"]
        capturing = torch.cuda.is_current_stream_capturing()
        seq = "ntok" in state
        if not capturing and not seq and static["count"] + T_new > cap:
            raise RuntimeError("the KV cache is full: %d of its %d tokens decoded, the step adds %d "
                               "(init_kv_cache(max_tokens=...))" % (static["count"], cap, T_new))
        dev = query.device
        held = "w_qkv" in state
        held_rows = held and T_new * B <= _LINEAR_MAX_ROWS
        if held_rows:
            qkv_new = self._held_linear(query.reshape(T_new * B, C), state["w_qkv"], state["b_qkv"], state["proj_rows"])
        elif held:
            qkv_new = self._held_gemm(query, state["w_qkv"], state["b_qkv"]).contiguous()
        else:
            with torch.no_grad():
                qkv_new = self._project(query)
            if qkv_new.dtype != kv.dtype:                          # (an fp32 step outside autocast: rounded, with the one-time warning)
                qkv_new = _ops.to_io_dtype(qkv_new).to(kv.dtype)
            qkv_new = qkv_new.contiguous()
        step_pad = None
        if key_padding_mask is not None:
            step_pad = key_padding_mask[:, -T_new:].to(device=dev, dtype=torch.uint8).contiguous()
        # the launches of a step and what follows their views: a per-sequence state issues the _seq entries with ntok
        sfx, tail = ("_seq", (nv.ptr(state["ntok"]),)) if seq else ("", ())
        geom = nv.ea_softmax_sdec_geom(B, h, d, nv.io_dtype(kv), T_new, cap, state["pos"].data_ptr(), state["status"].data_ptr())
        g = ctypes.byref(geom)
        rows = qkv_new.view(-1)[:T_new * B * 3 * C].view(T_new, B, 3, h, d)      # (proj_rows: the step's rows lead the buffer)
        tq = nv.t4(rows[:, :, 0].permute(1, 2, 0, 3))              # [B, h, T_new, d] view of the time-first rows
        tk, tv = nv.t4(kv[:, 0]), nv.t4(kv[:, 1])
        out = torch.empty((T_new, B, h, d), dtype=kv.dtype, device=dev)
        to = nv.t4(out.permute(1, 2, 0, 3))
        views = (ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), nv.ptr(pad), ctypes.byref(to))
        st = nv.stream()
        nv.call("ea_softmax_sdecode_append" + sfx, g, nv.ptr(rows), nv.ptr(step_pad), views[1], views[2], nv.ptr(pad), *tail, st)
        if T_new <= _SPLIT_MAX_STEP:
            ws = state.get("split_ws")
            parts = 1 if ws is None else ws.shape[3]
            nv.call("ea_softmax_sdecode_attn_split" + sfx, g, *views, parts, nv.ptr(ws), *tail, st)
            if parts > 1:
                nv.call("ea_softmax_sdecode_merge" + sfx, g, views[4], parts, nv.ptr(ws), *tail, st)
        else:
            nv.call("ea_softmax_sdecode_attn_mm" + sfx, g, *views, *tail, st)
        nv.call("ea_softmax_sdecode_advance" + sfx, g, *tail, st)
        if not capturing and not seq:                              # (a replay advances only the device count)
            static["count"] += T_new
        ydtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else query.dtype
        if held_rows:
            ytype = ydtype if ydtype in (kv.dtype, torch.float32) else torch.float32
            y = torch.empty((T_new, B, C), dtype=ytype, device=dev)
            self._held_linear(out.view(T_new * B, C), state["w_out"], state["b_out"], y.view(T_new * B, C))
        elif held:
            y = self._held_gemm(out.view(T_new, B, C), state["w_out"], state["b_out"])
        else:
            with torch.no_grad():
                y = _ops.linear(out.view(T_new, B, C), self.out_proj)
            if torch.is_autocast_enabled():
                return y.contiguous(), None
        return (y if y.dtype == ydtype else y.to(ydtype)).contiguous(), None
