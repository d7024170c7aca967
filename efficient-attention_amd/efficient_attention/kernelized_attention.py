"""Kernelized attention (Performer / FAVOR+ and the reference's other feature maps), MI355X build.

Mirrors efficient_attention/kernelized_attention.py:223-359: constructor kwargs, buffers / parameters (`eval_proj` for
`sample_scheme='default'` with fresh Gaussian features on every training call, `random_proj` as a buffer for 'fixed' and as
a Parameter for 'learnable'; none for the maps without random features) and the argparse flags.
  proj_method='favorp' without cos weighting, 'default' / 'fixed': the Performer cores (_ops.PerformerF32Fn, the 16-bit
      _ops.PerformerAttnFn), as before.
  every other supported configuration -- favorp / relu / fourier / relu-only / sigmoid-only / dpfp, with or without
      cos_weighting, any sample scheme -- the feature-map kernels (ea_kernelized.hip, _kernelized.KernelizedFn): head_dim
      64, at most 256 features after cos weighting, approx_attn_dim <= 128 (a multiple of 16) for the maps with W.
'mlp-fourier' is not built: its backward fails inside the reference itself (an in-place masked_fill_ on a ReLU output that
autograd saved), so there is no contract to match.
"""
import math

import torch
import torch.nn as nn

from . import add_nested_argument
from . import _kernelized
from . import _ops
from .abstract_attention import MultiheadAttention


def gaussian_orthogonal_random_matrix(nb_rows, nb_columns, seed=0, device=None, dtype=None):
    """Stacked QR blocks with chi-distributed row norms (reference :203-221)."""
    blocks = []
    for _ in range(nb_rows // nb_columns):
        q, _ = torch.linalg.qr(torch.randn(nb_columns, nb_columns), mode='reduced')
        blocks.append(q.t())
    rest = nb_rows - (nb_rows // nb_columns) * nb_columns
    if rest > 0:
        q, _ = torch.linalg.qr(torch.randn(nb_columns, nb_columns), mode='reduced')
        blocks.append(q.t()[:rest])
    mat = torch.cat(blocks).to(device=device, dtype=dtype)
    norms = torch.randn(nb_rows, nb_columns, device=device, dtype=dtype).norm(dim=1)
    return norms.unsqueeze(1) * mat


def create_proj_matrix(num_heads, proj_dim, input_dim, ortho=False, seed=0, device=None, dtype=None):
    if not ortho:
        return torch.randn(num_heads, proj_dim, input_dim, device=device, dtype=dtype)
    return torch.stack([gaussian_orthogonal_random_matrix(proj_dim, input_dim, seed=seed + 1000 * i,
                                                          device=device, dtype=dtype)
                        for i in range(num_heads)], dim=0)


class KernelizedAttention(MultiheadAttention):
    _F32_CORE = False           # no fp32-operand kernels for this core's estimator (the Performer core has its own fp32 path)
    _FEATURE_MAPS = True        # every proj_method / cos weighting / sample scheme below (False: favorp's fixed / redrawn only)
    def __init__(self, approx_attn_dim=64, proj_method='favorp', cos_weighting=False,
                 sample_scheme='default', *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.approx_attn_dim = approx_attn_dim
        self.proj_method = proj_method
        self.cos_weighting = cos_weighting
        self.sample_scheme = sample_scheme
        if not type(self)._FEATURE_MAPS and (proj_method != 'favorp' or cos_weighting or sample_scheme == 'learnable'):
            # (a subclass with a core of its own -- ScatterBrain -- keeps favorp's fixed / redrawn features only)
            raise NotImplementedError(
                "%s: only proj_method='favorp' without cos_weighting and without learnable features is built for MI355X "
                "(got proj_method=%r, cos_weighting=%r, sample_scheme=%r)"
                % (type(self).__name__, proj_method, cos_weighting, sample_scheme))
        self.use_random_proj = False
        if proj_method == 'dpfp':
            self.nu = (approx_attn_dim // self.head_dim) // 2
            assert self.nu > 0 and isinstance(self.nu, int), "approx_attn_dim must be a multiple of 2*head_dim!"
        elif proj_method == 'mlp-fourier':
            raise NotImplementedError(
                "proj_method='mlp-fourier' is not built for MI355X: its backward fails in the reference itself "
                "(masked_fill_ writes in place into a ReLU output that autograd saved), so there is nothing to match")
        elif proj_method in _kernelized.W_MAPS:
            self.use_random_proj = True
        elif proj_method not in ('relu-only', 'sigmoid-only'):
            raise NotImplementedError("proj_method=%r" % (proj_method,))
        if self.use_random_proj and sample_scheme not in ('default', 'fixed', 'learnable'):
            raise NotImplementedError('other sample schemes are not implemented yet.')
        if self._generic():
            self._check_generic()
        if self.use_random_proj:
            mat = create_proj_matrix(self.num_heads, approx_attn_dim, self.head_dim, ortho=True)
            if sample_scheme == 'default':
                self.register_buffer('eval_proj', mat)
            elif sample_scheme == 'fixed':
                self.register_buffer('random_proj', mat)
            else:
                self.random_proj = nn.Parameter(mat)
        self.apply(self._init_weights)

    def _generic(self):
        """True: the feature-map kernels (ea_kernelized_*); False: favorp on the Performer cores, as before."""
        return self.proj_method != 'favorp' or self.cos_weighting or self.sample_scheme == 'learnable'

    def _check_generic(self):
        what = "proj_method=%r%s" % (self.proj_method, ", cos_weighting" if self.cos_weighting else "")
        if self.head_dim != 64:
            raise NotImplementedError("%s: the feature-map kernels are built for head_dim 64, got %d" % (what, self.head_dim))
        m = self.approx_attn_dim
        if self.use_random_proj and not (0 < m <= _kernelized.MAX_M and m % 16 == 0):
            raise NotImplementedError("%s: approx_attn_dim must be a multiple of 16 in [16, %d], got %d"
                                      % (what, _kernelized.MAX_M, m))
        F = _kernelized.feature_count(self.proj_method, m, self.head_dim, self.cos_weighting)
        if F > _kernelized.MAX_FEATURES:
            raise NotImplementedError("%s: %d features (approx_attn_dim %d); the feature-map kernels hold at most %d"
                                      % (what, F, m, _kernelized.MAX_FEATURES))

    def _cfg(self):
        return _kernelized.make_cfg(self.proj_method, self.approx_attn_dim, self.head_dim, self.cos_weighting)

    def get_proj_matrix(self, device=None, dtype=None):
        if not self.use_random_proj:
            return None
        if self.sample_scheme == 'default':
            if self.training:
                return create_proj_matrix(self.num_heads, self.approx_attn_dim, self.head_dim,
                                          ortho=False, device=device, dtype=dtype)
            return self.eval_proj
        return self.random_proj

    def project_qkv(self, x):
        """fp32 activations outside autocast stay fp32: the Performer core computes in exact fp32 arithmetic
        (_ops.PerformerF32Fn), as the reference does there (abstract_attention.py:120-133); so do the feature-map kernels."""
        # (only for the Performer core itself: a subclass with another `_attend` -- ScatterBrain inherits this method through the
        #  MRO and feeds the window kernels -- takes the 16-bit activations those kernels want: ADVICE r04)
        if (type(self)._attend is KernelizedAttention._attend
                and x.dtype == torch.float32 and not torch.is_autocast_enabled() and x.is_cuda and self.head_dim == 64
                and (self._generic() or (not _ops.PERFORMER_16BIT and self.approx_attn_dim <= 96
                                         and self.approx_attn_dim % 16 == 0))):
            B, N, C = x.shape
            return _ops.linear(x, self.qkv).reshape(B, N, 3, self.num_heads, C // self.num_heads)
        return super().project_qkv(x)

    project_qkv._ea_builtin = True

    def _core_spec(self, B, N, seq_shape, key_padding_mask, device):
        """The single-node path (_ops.CoreModuleFn, round 4) for the exact-fp32 cores; everything else keeps the three nodes."""
        if type(self)._attend is not KernelizedAttention._attend:
            return None, ()
        if self._generic():
            W = self.get_proj_matrix(device=device, dtype=torch.float32)
            mask = _ops._mask_u8(key_padding_mask, B, N, device)
            learn = self.sample_scheme == 'learnable' and self.use_random_proj
            return _kernelized.KernelizedCore(mask, None if learn else W, self._cfg(), learn), ((W,) if learn else ())
        if _ops.PERFORMER_16BIT or self.head_dim != 64 or self.approx_attn_dim > 96 or self.approx_attn_dim % 16 != 0:
            return None, ()
        proj = self.get_proj_matrix(device=device, dtype=torch.float32)
        return _ops.PerformerCore(_ops._mask_u8(key_padding_mask, B, N, device), proj), ()

    def _attend(self, qkv5, key_padding_mask, seq_shape):
        B, N = qkv5.shape[:2]
        proj = self.get_proj_matrix(device=qkv5.device, dtype=torch.float32)
        mask = _ops._mask_u8(key_padding_mask, B, N, qkv5.device)
        if self._generic():
            learn = self.sample_scheme == 'learnable' and self.use_random_proj
            return _kernelized.kernelized_attention(qkv5, mask, proj, self._cfg(), learn)
        return _ops.performer_attention(qkv5, mask, proj)

    @staticmethod
    def add_attn_specific_args(parent_parser, struct_name="attn_args", prefix=""):
        parent_parser = MultiheadAttention.add_attn_specific_args(parent_parser, struct_name=struct_name, prefix=prefix)
        group = parent_parser.add_argument_group("Attention")
        fp = prefix + "-" if len(prefix) > 1 else ""
        kw = dict(struct_name=struct_name, prefix=prefix)
        add_nested_argument(group, "--%sapprox-attn-dim" % fp, default=64, type=int,
                            help='number of random features', **kw)
        add_nested_argument(group, "--%sproj-method" % fp, default='favorp', type=str,
                            help='which random feature map is used', **kw)
        add_nested_argument(group, "--%scos-weighting" % fp, action='store_true', default=False, help='', **kw)
        add_nested_argument(group, "--%ssample-scheme" % fp, default='default', type=str, **kw)
        return parent_parser
