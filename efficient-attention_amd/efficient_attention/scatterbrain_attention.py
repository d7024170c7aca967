"""ScatterBrain (sparse local windows + low-rank random features under one softmax, arXiv
2110.15343), MI355X build.

Mirrors efficient_attention/scatterbrain_attention.py:46-180 of the reference: the class is
`KernelizedAttention` x `LocalAttention` (constructor kwargs, `eval_proj` buffer, relative-position
table, argparse flags of both), `forward(x, key_padding_mask=None)` with the 1-D padding rule of
LocalAttention._process_input.  Per window g and query i the softmax runs over the window's keys and
m feature columns with logits `log phi(q_i)[c] + log(sum_{j outside g} phi(k_j)[c])` and values the
phi-weighted mean of v outside the window (reference :99-160).

Split of the work in this build: the window part -- logits, mask, relative-position bias, softmax
statistics, P.V and its backward -- is the HIP window kernel (`_ops.LocalAttnLseFn`, which hands back
the per-query log-sum-exp); the feature columns are merged with it exactly through that log-sum-exp
(out = e^{lse_loc - Z} o_loc + e^{R - Z} o_rfa, Z = logaddexp(lse_loc, R)).  The feature statistics
themselves (global-minus-window sums) and the merge are HIP kernels as well (ea_scatter.hip)
for head_dim 64, at most 64 features and query windows of at most 64 tokens, with and without window
overlap; beyond those limits, and behind the dev switch `_ops.SCATTER_TORCH`, the same algebra runs as
batched GEMMs and reductions on torch device ops in fp32.  With window overlap the key side of a window
is the extended patch and the reference's zero padding of the partitioned log-features makes every
out-of-range slot count as a key with phi = 1 and v = 0 (reference :99-100); the kernels walk the patch
in 64-row tiles and the backward sums every key's gradient over the windows whose patch holds it.
(The reference returns NaN there as soon as a border window's padding outweighs the features of the keys
outside it -- tests/golden/cases.py -- so it is a path for small-key regimes; the kernels keep that.)
"""
import math

import torch
import torch.nn.functional as F

from . import add_nested_argument
from . import _ops
from .kernelized_attention import KernelizedAttention
from .local_attention import LocalAttention


class ScatterBrain(KernelizedAttention, LocalAttention):
    _F32_CORE = False           # (no fp32-operand kernels for this variant yet: fp32 input is rounded to bf16 with a warning)
    _FEATURE_MAPS = False       # its feature half is built for favorp only: other proj_method / cos / learnable W are refused
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._slot_cache = {}
        self.apply(self._init_weights)

    def project_qkv(self, x):
        """The window kernels take 16-bit rows: the fp32 pass-through of KernelizedAttention.project_qkv (for the exact-fp32
        Performer core) must not reach them through the MRO (plain fp32 input, head_dim 64, 64 features crashed)."""
        from .abstract_attention import MultiheadAttention
        return MultiheadAttention.project_qkv(self, x)

    def _key_slots(self, seq_shape, device):
        """[G, Wk] token index of every slot of every extended key window, N (one past the end) for the slots that
        leave the sequence (attn_utils.py:155-166 / 190-210 as an index table)."""
        key = (tuple(seq_shape), str(device))
        if key not in self._slot_cache:
            w, e = self.window_size, self.ext_size
            t = w + 2 * e
            if self.attn_2d:
                H, W = seq_shape
                y = (torch.arange(H // w, device=device) * w - e).view(-1, 1, 1, 1) + torch.arange(t, device=device).view(1, 1, -1, 1)
                x = (torch.arange(W // w, device=device) * w - e).view(1, -1, 1, 1) + torch.arange(t, device=device).view(1, 1, 1, -1)
                ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
                tok = torch.where(ok, y * W + x, torch.full_like(y * W + x, H * W)).reshape(-1, t * t)
            else:
                N = seq_shape[0]
                tok = (torch.arange(N // w, device=device) * w - e).view(-1, 1) + torch.arange(t, device=device).view(1, -1)
                tok = torch.where((tok >= 0) & (tok < N), tok, torch.full_like(tok, N))
            self._slot_cache[key] = tok
        return self._slot_cache[key]

    def forward(self, x, key_padding_mask=None):
        B, *seq_shape, C = x.shape
        orig_n = int(math.prod(seq_shape))
        w = self.window_size
        if self.attn_2d:
            assert len(seq_shape) == 2 and seq_shape[0] % w == 0 and seq_shape[1] % w == 0
            N, xs, mask = orig_n, x.reshape(B, orig_n, C), key_padding_mask
        else:
            N = int(math.ceil(orig_n / w) * w)
            xs = F.pad(x, (0, 0, 0, N - orig_n)) if N != orig_n else x
            mask = None
            if key_padding_mask is not None or N != orig_n:
                mask = torch.zeros(B, N, dtype=torch.bool, device=x.device)
                if key_padding_mask is not None:
                    mask[:, :orig_n] = key_padding_mask.to(torch.bool)
                mask[:, orig_n:] = True
            seq_shape = [N]
        # the training step as ONE autograd node (round 6, _ops.GraphCore: `_scatter` -- window kernel, feature kernels and their
        # glue -- recorded inside CoreModuleFn's forward); the relative-position table is the one parameter `_scatter` reads
        from .abstract_attention import MultiheadAttention
        if (_ops.USE_GRAPH_CORE and torch.is_autocast_enabled() and xs.is_cuda and (self.proj_drop.p == 0.0 or not self.training)
                and type(self).merge_and_project is MultiheadAttention.merge_and_project
                and type(self).project_qkv is ScatterBrain.project_qkv
                and _ops.core_module_fn_supported(xs, self.qkv, self.proj, torch.get_autocast_dtype("cuda"))):
            params = (self.local_relative_position_bias_table,) if self.use_rpe else ()
            shape = list(seq_shape)
            core = _ops.GraphCore(lambda qkv5, *ps: self._scatter(qkv5, mask, shape), torch.is_grad_enabled())
            y = _ops.CoreModuleFn.apply(xs, self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias, core,
                                        torch.get_autocast_dtype("cuda"), self.num_heads, *params)
            y = self.proj_drop(y.view(B, *seq_shape, C))
            return y if self.attn_2d else y[..., :orig_n, :]
        qkv5 = self.project_qkv(xs)
        out = self._scatter(qkv5, mask, seq_shape)
        y = self.merge_and_project(out, B, seq_shape, C, x.dtype)
        return y if self.attn_2d else y[..., :orig_n, :]

    def _scatter(self, qkv5, mask, seq_shape):
        B, N, _, h, d = qkv5.shape
        w = self.window_size
        proj = self.get_proj_matrix(device=qkv5.device, dtype=torch.float32)      # [h, m, d]
        m = proj.shape[1]
        mask_u8 = _ops._mask_u8(mask, B, N, qkv5.device)
        o_loc, lse_loc = _ops.LocalAttnLseFn.apply(
            qkv5, self._table_bias(), mask_u8, self.attn_2d, tuple(seq_shape), w, self.ext_size)
        if _ops.scatter_supported(qkv5, proj, self.attn_2d, seq_shape, w, self.ext_size) and not _ops.SCATTER_TORCH:
            # feature half + merge on HIP (ea_scatter.hip), with and without window overlap; wider windows / more features
            # fall through to torch ops
            return _ops.ScatterFeatureFn.apply(qkv5, o_loc, lse_loc, mask_u8, proj, self.attn_2d, tuple(seq_shape), w,
                                               self.ext_size)

        if self.attn_2d:
            H, W = seq_shape
            G, Wq = (H // w) * (W // w), w * w

            def win(t):                                   # [B,h,N,c] -> [B,h,G,Wq,c]
                c = t.shape[-1]
                return t.reshape(B, h, H // w, w, W // w, w, c).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, h, G, Wq, c)

            def unwin(t):                                 # [B,h,G,Wq,c] -> [B,h,N,c]
                c = t.shape[-1]
                return t.reshape(B, h, H // w, W // w, w, w, c).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, h, N, c)
        else:
            G, Wq = N // w, w

            def win(t):
                return t.reshape(B, h, G, Wq, t.shape[-1])

            def unwin(t):
                return t.reshape(B, h, N, t.shape[-1])

        with torch.autocast(device_type="cuda", enabled=False):
            q, k, v = [t.float() for t in _ops._qkv_views(qkv5)]

            def log_phi(x):
                return d ** -0.25 * torch.einsum("bhnd,hmd->bhnm", x, proj) \
                    - 0.5 * d ** -0.5 * (x * x).sum(-1, keepdim=True) - math.log(m) / 2
            lq, lk = log_phi(q), log_phi(k)
            if mask is not None:
                lk = lk.masked_fill(mask.to(torch.bool)[:, None, :, None], float("-inf"))
            # phi(k) sums over all keys minus those of the window, one (detached) stabiliser per feature
            mx = lk.amax(dim=-2, keepdim=True).detach()
            if self.ext_size > 0:
                # overlapping windows: sums over the extended patch, gathered; a slot outside the sequence is a key
                # with log-feature 0 and v = 0 (the reference's zero padding), which also enters the stabiliser.
                # Memory: the gathers below are fp32 [B,h,G,Wk,m] / [B,h,G,Wk,d] and stay alive for autograd -- with
                # e = w/2 on a 2-D grid that is ~4x the token count times (m + d) floats per layer (the reference
                # materialises the same padded tensors).  This variant is kept for parity with the reference's
                # behaviour (NaN beyond small keys), not as a production path.
                mx = mx.clamp(min=0.0)
                pk = torch.exp(lk - mx)
                slots = self._key_slots(seq_shape, q.device)                            # [G, Wk], N = outside
                w_pk = torch.cat([pk, torch.exp(-mx)], dim=2)[:, :, slots]              # [B,h,G,Wk,m]
                w_v = torch.cat([v, v.new_zeros(B, h, 1, d)], dim=2)[:, :, slots]       # [B,h,G,Wk,d]
                s_win = torch.einsum("bhgwc,bhgwd->bhgcd", w_pk, w_v)
                z_win = w_pk.sum(-2)
                s_all = torch.einsum("bhnc,bhnd->bhcd", pk, v).unsqueeze(2)
                z_all = pk.sum(-2).unsqueeze(2)
            else:
                pk = torch.exp(lk - mx)                                                 # [B,h,N,m]
                w_pk, w_v = win(pk), win(v)
                s_win = torch.einsum("bhgwc,bhgwd->bhgcd", w_pk, w_v)                   # [B,h,G,m,d]
                z_win = w_pk.sum(-2)                                                    # [B,h,G,m]
                # the global sums are the sums of the window sums (windows partition the sequence)
                s_all, z_all = s_win.sum(2, keepdim=True), z_win.sum(2, keepdim=True)
            kv_stats = (s_all - s_win) / (z_all - z_win).unsqueeze(-1).clamp(min=1e-3)
            # log-sum-exp of the log-features from the same sums: log z + stabiliser
            lse_all = torch.log(z_all) + mx                                         # [B,h,1,m]
            lse_win = torch.log(z_win) + mx                                         # [B,h,G,m]
            a = torch.maximum(lse_all, lse_win)
            nonlocal_ = a + ((lse_all - a).exp() - (lse_win - a).exp() + 1e-5).log()
            log_rfa = win(lq) + nonlocal_.unsqueeze(-2)                             # [B,h,G,Wq,m]
            r = torch.logsumexp(log_rfa, dim=-1, keepdim=True)                      # [B,h,G,Wq,1]
            o_rfa = torch.einsum("bhgwc,bhgcd->bhgwd", torch.exp(log_rfa - r), kv_stats)
            r_t, o_rfa_t = unwin(r).squeeze(-1), unwin(o_rfa)                       # [B,h,N], [B,h,N,d]
            z = torch.logaddexp(lse_loc, r_t)
            out = torch.exp(lse_loc - z).unsqueeze(-1) * o_loc.permute(0, 2, 1, 3).float() \
                + torch.exp(r_t - z).unsqueeze(-1) * o_rfa_t
        return out.permute(0, 2, 1, 3).to(qkv5.dtype).contiguous()

    @staticmethod
    def add_attn_specific_args(parent_parser, struct_name="attn_args", prefix=""):
        parent_parser = LocalAttention.add_attn_specific_args(parent_parser, struct_name=struct_name, prefix=prefix)
        group = parent_parser.add_argument_group("Attention")
        fp = prefix + "-" if len(prefix) > 1 else ""
        kw = dict(struct_name=struct_name, prefix=prefix)
        add_nested_argument(group, "--%sapprox-attn-dim" % fp, default=64, type=int, help="number of random features", **kw)
        add_nested_argument(group, "--%sproj-method" % fp, default="favorp", type=str,
                            help="which attention method is used for RFA", **kw)
        add_nested_argument(group, "--%scos-weighting" % fp, action="store_true", default=False, help="", **kw)
        add_nested_argument(group, "--%ssample-scheme" % fp, default="default", type=str, **kw)
        return parent_parser
