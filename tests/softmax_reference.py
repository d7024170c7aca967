"""Same-operand reference of the 16-bit streaming softmax core (plain torch, CPU; imports window_reference only, nothing of the
product; tests/test_softmax_reference_cpu.py holds it to the oracle): what ea_softmax_attn_fwd / ea_softmax_attn_bwd compute
(csrc/ea_softmax.hip),

    out_i = sum_j keep_ij keep_scale softmax_j(l_i)_j v_j,    l_ij = s q_i.k_j [- s |k_j|^2 / 2], -inf on padded keys,

the softmax baseline (abstract_attention.py:120-133: mask, attention dropout from explicit keep decisions; the normaliser is
that of the full row) and, with key_norm_bias, the second softmax of randomized attention (randomized_attention.py:44-51; the
first one is the plain form with v = k).  lse is in natural-log units and includes the key-norm term; delta = dout . out.
Gradients are those of the loss <out, dout>, from autograd.

Two evaluations of the same function:
  R  exact reference: dtype = torch.float64, round_to = None (torch.softmax / logsumexp and their autograd).
  M  rounding model : dtype = torch.float32, round_to = torch.bfloat16 | torch.float16 -- window_reference._ModelAttn, which
     states this kernel family's roundings, on the logits above; everything in fp32 except (lines of csrc/ea_softmax.hip)
       forward  sm_fwd_kernel     : the unnormalised P = exp2(l - m) is packed to the MFMA element type before P.V (:164-165),
                                    with the keep scaling applied first (:158-163); the normaliser sums the unrounded,
                                    undropped P (:156-157, :167-173); out is stored in the I/O dtype (:248)
       backward sm_bwd_dq_kernel  : delta = dO . O reads the STORED out (:286-296) and is kept in fp32 (:298); P is recomputed from
                                    the saved lse (:374-375), dS = P (keep dP - delta) is packed for dQ (:380-381); dq is stored
                                    in the I/O dtype (:422)
                sm_bwd_dkv_kernel : P (keep-scaled, :554) and dS (:552) are packed for dV^T = dO^T P and dK^T = Q^T dS
                                    (:556-557); dk, dv are stored in the I/O dtype (:622-623)
       key_norm_bias              : the term -s |k_j|^2 / 2 is formed in fp32 from the 16-bit k (:24-31, :467-479); its gradient
                                    -s k_j sum_i dS_ij is added to dk BEFORE that store (:615).  The kernel sums the unrounded dS
                                    there (:553); the model feeds it the rounded dS (autograd through the packed dS, as
                                    window_reference does for the bias gradient), a slightly larger error.
     Not modelled (the factor of the bound stands for them): the fp32 accumulation order, v_exp_f32 / v_log_f32, and the online
     rescale -- a P of an early chunk is packed against the running maximum of that chunk, not the final one.
     model=True with round_to=None is M's arithmetic without roundings (tests/test_softmax_reference_cpu.py holds it to R).

k and v are separate leaves even where a caller passes the same tensor for both (RA's first softmax): the kernels write dk and dv
to separate rows and leave the sum to the caller.

DEFECTS: single-defect variants of M (`defect=`), with which tests/test_softmax_reference_cpu.py shows that the bound
a(X) <= 4 a(M) + f notices a subtly wrong kernel."""
import torch

from window_reference import FACTOR, _ModelAttn, a_err, bound_report, floor_for, norm_errs, rnd  # noqa: F401

NAMES = ("out", "lse", "delta", "dq", "dk", "dv")

DEFECTS = (
    "padded_keys_in_normaliser",      # the normaliser (and lse) counts the padded keys; the numerator does not
    "tail_keys_missing",              # the last N % 64 keys are never visited
    "last_query_tile_unwritten",      # out / lse / delta / dq of the last 16-query tile stay at the NaN prefill
    "dp_without_keep_scale",          # backward: dS = P (keep dP - delta) with the 0/1 keep instead of keep keep_scale
    "dropout_in_normaliser",          # dropped entries leave the normaliser too
    "kb_missing_in_forward",          # out, lse (and delta) without the key-norm term; the backward has it
    "kb_grad_missing_in_dk",          # dk without -s k_j sum_i dS_ij
    "delta_without_keep_scale",       # delta from the unscaled out: dO . O / keep_scale
)


class _AttnDpUnscaled(_ModelAttn):
    """_ModelAttn whose backward forms dS from keep dP with the 0/1 decisions (defect dp_without_keep_scale); dV as in the model."""

    @staticmethod
    def backward(ctx, dout, dlse):
        full = ctx.keepmul
        dvals = _ModelAttn.backward(ctx, dout, dlse)[1]
        ctx.keepmul = (full != 0).to(full.dtype)
        ds = _ModelAttn.backward(ctx, dout, dlse)[0]
        ctx.keepmul = full
        return ds, dvals, None, None


def softmax_core_ref(q, k, v, *, mask=None, keep=None, keep_scale=1.0, key_norm_bias=False, scale=None, dtype=torch.float64,
                     round_to=None, model=None, defect=None):
    """q, k, v [B,h,N,d]; mask [B,N] bool (True = padded key) or None; keep [B,h,N,N] 0/1 or None -> (out [B,h,N,d], lse [B,h,N])."""
    B, h, n, d = q.shape
    scale = d ** -0.5 if scale is None else scale
    model = (round_to is not None) if model is None else model
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    logits = scale * torch.einsum("bhid,bhjd->bhij", q, k)
    if key_norm_bias and defect != "kb_missing_in_forward":
        kn = k.detach() if defect == "kb_grad_missing_in_dk" else k
        logits = logits - 0.5 * scale * (kn * kn).sum(-1).unsqueeze(-2)
    dead = torch.zeros(B, n, dtype=torch.bool) if mask is None else mask.bool().clone()
    if defect == "tail_keys_missing":
        dead[:, n - n % 64:] = True
    keepmul = None if keep is None else keep.to(dtype) * keep_scale
    if defect == "padded_keys_in_normaliser":
        alive = (~dead).to(dtype)[:, None, None, :].expand(B, h, n, n)
        keepmul = alive if keepmul is None else keepmul * alive
    else:
        logits = logits.masked_fill(dead[:, None, None, :], float("-inf"))
    if defect == "dropout_in_normaliser":
        logits = logits.masked_fill(keep[:, :, :, :] == 0, float("-inf"))
        keepmul = torch.full_like(logits, keep_scale)
    if not model:
        p = torch.softmax(logits, -1)
        return torch.matmul(p if keepmul is None else p * keepmul, v), torch.logsumexp(logits, -1)
    fn = _AttnDpUnscaled if defect == "dp_without_keep_scale" else _ModelAttn
    return fn.apply(logits, v, keepmul, round_to)


def _grads_slice(q, k, v, dout, *, dtype, round_to, defect, forward_only, **kw):
    leaves = [t.detach().to(dtype).requires_grad_(not forward_only) for t in (q, k, v)]
    out, lse = softmax_core_ref(*leaves, dtype=dtype, round_to=round_to, defect=defect, **kw)
    dout = dout.to(dtype)
    delta = (dout * out.detach()).sum(-1)
    res = dict(out=out.detach(), lse=lse.detach(), delta=delta)
    if forward_only:
        return res
    dlse = torch.zeros_like(lse)
    if defect == "delta_without_keep_scale":
        # _ModelAttn's backward subtracts dlse from dO . O: this leaves dO . O / keep_scale
        res["delta"] = delta / kw["keep_scale"]
        dlse = (delta - res["delta"]).detach()
    gs = torch.autograd.grad([out, lse], leaves, [dout, dlse])
    for n_, g in zip(("dq", "dk", "dv"), gs):
        res[n_] = rnd(g, round_to)                                     # the 16-bit store of dq / dk / dv
    return res


def softmax_grads(q, k, v, dout, *, mask=None, keep=None, keep_scale=1.0, key_norm_bias=False, scale=None, dtype, round_to,
                  batch_step=8, model=None, defect=None, forward_only=False):
    """Forward and gradients of the loss <out, dout> -> dict(out, lse, delta, dq, dk, dv) (forward_only: out, lse, delta).
    q, k, v, dout [B,h,N,d]; keep [B,h,N,N] 0/1 (any dtype).  Evaluated in batch slices of `batch_step` rows: the largest
    intermediate is [batch_step, h, N, N]."""
    assert defect is None or defect in DEFECTS
    B = q.shape[0]
    parts = []
    for b0 in range(0, B, batch_step):
        sl = slice(b0, b0 + batch_step)
        parts.append(_grads_slice(q[sl], k[sl], v[sl], dout[sl], mask=None if mask is None else mask[sl],
                                  keep=None if keep is None else keep[sl], keep_scale=keep_scale, key_norm_bias=key_norm_bias,
                                  scale=scale, dtype=dtype, round_to=round_to, model=model,
                                  defect=None if defect in ("last_query_tile_unwritten",) else defect, forward_only=forward_only))
    res = {n_: torch.cat([p_[n_] for p_ in parts], 0) for n_ in parts[0]}
    if defect == "kb_missing_in_forward":
        # forward results of the defective kernel, gradients of the sound one (its backward recomputes P with the term)
        good = softmax_grads(q, k, v, dout, mask=mask, keep=keep, keep_scale=keep_scale, key_norm_bias=key_norm_bias, scale=scale,
                             dtype=dtype, round_to=round_to, batch_step=batch_step, model=model)
        res = dict(good, out=res["out"], lse=res["lse"], delta=res["delta"])
    if defect == "last_query_tile_unwritten":
        n = q.shape[2]
        first = (n - 1) // 16 * 16
        for n_ in ("out", "lse", "delta", "dq"):
            if n_ in res:
                res[n_] = res[n_].clone()
                res[n_][:, :, first:] = float("nan")
    return res


# ------------------------------------------------------------------------------------------------------------------------
# the Gumbel-max sampler (sm_sample_kernel, csrc/ea_softmax.hip:629-696), predicted draw for draw
# ------------------------------------------------------------------------------------------------------------------------
NEAR_TOL = 1e-3          # the drawn key's score lies within this of the row maximum ...
NEAR_SHARE = 0.999       # ... for at least this share of the queries,
EXACT_SHARE = 0.99       # and the draw IS the fp64 argmax for at least this share


def sampler_operands(shape, io, seed=2024):
    """q, k [B,h,N,d]: standard normal, drawn in fp32 and rounded once to the I/O dtype (held in fp32)."""
    g = torch.Generator().manual_seed(seed + sum(shape))
    return [torch.randn(*shape, generator=g).to(io).float() for _ in range(2)]


def _mix32(x):
    """mix32 of the kernel (:632-635) on a uint64 array holding 32-bit values."""
    import numpy as np
    m = np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    return x ^ (x >> np.uint64(16))


def uniform_counts(seed, BH, N):
    """hsh >> 8 of every (b h, query, key) as float64 [BH,N,N]: the kernel's counter-based hash (:655-657, :680); the uniform is
    u = (count + 0.5) / 2^24."""
    import numpy as np
    m = np.uint64(0xffffffff)
    seed = int(seed)
    lo, hi = np.uint64(seed & 0xffffffff), np.uint64(seed >> 32)
    bh = np.arange(BH, dtype=np.uint64).reshape(BH, 1, 1)
    qt = np.arange(N, dtype=np.uint64).reshape(1, N, 1)
    j = np.arange(N, dtype=np.uint64).reshape(1, 1, N)
    inner = _mix32((hi + ((np.uint64(0x9e3779b9) * bh) & m)) & m)
    base = _mix32(lo ^ inner) ^ ((np.uint64(0x85ebca77) * qt) & m)
    hsh = _mix32((base + ((np.uint64(0xc2b2ae3d) * j) & m)) & m)
    return (hsh >> np.uint64(8)).astype(np.float64)


def gumbel_scores(q, k, seed, scale=None):
    """score_ij = s q_i.k_j + G_ij in fp64 [B,h,N,N], G = -ln(-ln u): what the kernel takes the argmax of."""
    import numpy as np
    B, h, N, d = q.shape
    scale = d ** -0.5 if scale is None else scale
    u = (uniform_counts(seed, B * h, N) + 0.5) / 16777216.0
    gum = -np.log(-np.log(u))
    return scale * torch.einsum("bhid,bhjd->bhij", q.double(), k.double()) + torch.from_numpy(gum).view(B, h, N, N)


def fp32_emulated_draw(q, k, seed, scale=None):
    """The kernel's formula in float32 (:681-684): u = ((float) count + 0.5f) 2^-24, G = -LN2 log2(-LN2 log2 u) with float32 log2,
    val = acc * s + G, first index of the maximum (:684, :693).  -> int64 [B,h,N]."""
    import numpy as np
    B, h, N, d = q.shape
    f = np.float32
    scale = f(d ** -0.5 if scale is None else scale)
    ln2 = f(0.6931471805599453)
    u = (uniform_counts(seed, B * h, N).astype(f) + f(0.5)) * f(1.0 / 16777216.0)
    with np.errstate(divide="ignore"):
        gum = -ln2 * np.log2(-ln2 * np.log2(u, dtype=f), dtype=f)
    acc = torch.einsum("bhid,bhjd->bhij", q.float(), k.float()).numpy().reshape(B * h, N, N)
    val = acc * scale + gum
    return torch.from_numpy(val.argmax(-1)).view(B, h, N)


def sampler_shares(score, draw):
    """(share of queries whose drawn key scores within NEAR_TOL of the row maximum, share whose draw is the fp64 argmax)."""
    best = score.max(-1)
    got = torch.gather(score, -1, draw.unsqueeze(-1)).squeeze(-1)
    return float(((best.values - got) <= NEAR_TOL).double().mean()), float((best.indices == draw).double().mean())
