"""Same-operand reference of the 16-bit window-attention core and of the EVA landmark passes (plain torch, CPU; imports the
oracle only, nothing of the product).

    window_core      one softmax per query over [local window keys | L landmark keys], the landmarks given as OPERANDS --
                     what ea_window_attn_fwd / ea_window_attn_bwd compute (csrc/ea_window_fwd.hip, ea_window_bwd.hip)
    beta_core        beta_c = softmax_j(s w_c.k_j - s |k_j|^2 / 2) . v_j over the (extended) chunk c   (ea_eva_beta_*)
    chunk_mean_core  masked means of q and k over every chunk                                          (ea_eva_chunk_mean_*)

Index tables, gathers, the -5e4 fill, absent slots, the 1-D tail padding and the causal visibility rules are the oracle's own
(oracle/attention.py: window_index_1d/2d, causal_window_index_1d, _gather_tokens, _gather_mask, _scatter_windows, MASK_VAL): a
padded query sees no local key (causal geometry), local keys j <= i + e and only the landmarks of earlier chunks (causal = 2).
Gradients come from autograd; lse is in natural-log units; bias is in natural units and so is its gradient.

Two evaluations of the same functions:
  R  exact reference: dtype = torch.float64, round_to = None.
  M  rounding model : dtype = torch.float32, round_to = torch.bfloat16 | torch.float16 -- everything in fp32 except the 16-bit
     roundings the kernels document:
       forward  (ea_window_fwd.hip) : the unnormalised P = exp2(s - m) is packed to the MFMA element type before P.V (:255-256,
                                      with the keep mask :269-271); the normaliser sums the unrounded P (:253, :274); out is
                                      stored in the I/O dtype (:296-300 / :308-311)
       backward (ea_window_bwd.hip) : delta = dO . O reads the STORED (rounded) out (:320-331); P is recomputed from the saved lse
                                      (:474) and packed for dV^T = dO^T P (:486 hand-over tiles, :709); dS = P (keep dP - delta)
                                      is packed for dQ (:481-482) and for dK, d(landmark keys) (:710); dq (:514-528), dk, dv
                                      (:785-786; the finish pass of the scratch slices :952-953) are stored in the I/O dtype;
                                      half-window overlap (`cdirect`, :788-804): class 0 stores, class 1 adds to the stored
                                      value -- two roundings of dk / dv
       (the bias gradient sums the unrounded dS in the kernels, :491 and :706; the model feeds it the rounded dS, a slightly
        larger error)
       ea_eva_landmark.hip          : beta / chunk means and d_omega are fp32 end to end (no rounding); beta_bwd adds to the
                                      existing 16-bit dk / dv rows and stores them (:456-464, :741-748) once per colour class of
                                      overlapping chunks (:770, :815-818); chunk_mean_bwd adds to dq / dk and stores (:141-151,
                                      :603-610), the gather kernel of overlapping chunks once per token (:188-198)
"""
import math

import torch

from oracle.attention import MASK_VAL, _gather_mask, _gather_tokens, _scatter_windows
from oracle.geometry import causal_window_index_1d, window_index_1d, window_index_2d


def rnd(x, round_to):
    """x rounded to `round_to` and back (None: unchanged)."""
    return x if round_to is None else x.to(round_to).to(x.dtype)


class _ModelAttn(torch.autograd.Function):
    """softmax(s) (keep-scaled) . vals with the kernels' roundings, forward and backward (module docstring)."""

    @staticmethod
    def forward(ctx, s, vals, keepmul, round_to):
        m = s.amax(-1, keepdim=True)
        pu = torch.exp(s - m)
        l = pu.sum(-1, keepdim=True)
        pn = pu if keepmul is None else pu * keepmul
        out = rnd(torch.matmul(rnd(pn, round_to), vals) / l, round_to)
        lse = (m + torch.log(l)).squeeze(-1)
        ctx.save_for_backward(s, vals, out, lse)
        ctx.keepmul, ctx.round_to = keepmul, round_to
        return out, lse

    @staticmethod
    def backward(ctx, dout, dlse):
        s, vals, out, lse = ctx.saved_tensors
        keepmul, round_to = ctx.keepmul, ctx.round_to
        p = torch.exp(s - lse.unsqueeze(-1))
        dp = torch.matmul(dout, vals.transpose(-1, -2))
        pk = p
        if keepmul is not None:
            dp, pk = dp * keepmul, p * keepmul
        delta = (dout * out).sum(-1, keepdim=True) - dlse.unsqueeze(-1)
        ds = rnd(p * (dp - delta), round_to)
        dvals = torch.matmul(rnd(pk, round_to).transpose(-1, -2), dout)
        return ds, dvals, None, None


def window_tables(n, w, e, attn_2d=False, seq_shape=None, causal=0):
    """(idx_q [G, Wq], idx_k [G, Wk], n_pad): token of every query / key slot, -1 = absent (oracle/geometry.py)."""
    if causal:
        assert not attn_2d and n % w == 0
        return window_index_1d(n, w, 0), causal_window_index_1d(n, w, e), n
    if attn_2d:
        H, W = seq_shape
        assert H * W == n and H % w == 0 and W % w == 0
        return window_index_2d(H, W, w, 0), window_index_2d(H, W, w, e), n
    n_pad = int(math.ceil(n / w) * w)                     # pad_to_multiple of the 1-D modules: the tail slots are absent
    idx_q = window_index_1d(n_pad, w, 0)
    idx_k = window_index_1d(n_pad, w, e)
    return idx_q, torch.where(idx_k >= n, torch.full_like(idx_k, -1), idx_k), n_pad


def window_core(q, k, v, lk=None, lv=None, *, bias=None, mask=None, attn_2d=False, seq_shape=None, w, e=0, causal=0, chunk=0,
                keep=None, keep_scale=1.0, round_to=None, dtype=torch.float64, scale=None, hooks=None):
    """q, k, v [B,h,N,d]; lk, lv [B,h,L,d] or None; bias [h,Wq,Wk] (natural units) or None; mask [B,N] bool (True = padded) or
    None; causal 0 | 1 (causal_eva.py geometry: left extension, padded queries masked) | 2 (+ the causal masks, landmark c
    belongs to tokens [c chunk, (c+1) chunk)); keep [B,h,N,Wk+L] 0/1 decisions of the attention dropout (kept probabilities
    are scaled by keep_scale, the normaliser keeps every column) or None.  -> (out [B,h,N,d], lse [B,h,N]).
    hooks: test-only interception points {name: fn(tensor, ctx) -> tensor} (idx_k, bias, local_kv, lm_kv, local_logits,
    lm_logits, keepmul; ctx: the intermediate tables) with which tests/test_window_reference_cpu.py builds deliberately wrong
    variants."""
    hooks = hooks or {}
    ctx = {}

    def hook(name, t):
        return hooks[name](t, ctx) if name in hooks else t
    B, h, n, d = q.shape
    scale = d ** -0.5 if scale is None else scale
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    idx_q, idx_k, n_pad = window_tables(n, w, e, attn_2d, seq_shape, causal)
    ctx.update(e=e, causal=causal)
    idx_k = hook("idx_k", idx_k)
    G, Wq = idx_q.shape
    Wk = idx_k.shape[1]
    mask = torch.zeros(B, n, dtype=torch.bool) if mask is None else mask.bool()
    ctx.update(idx_q=idx_q, idx_k=idx_k, mask=mask, Wq=Wq, Wk=Wk, e=e, chunk=chunk, keep_scale=keep_scale)
    idx_qg = torch.where(idx_q >= n, torch.full_like(idx_q, -1), idx_q)     # queries of the 1-D tail: zeros, dropped at the end
    wq = _gather_tokens(q, idx_qg)
    wk, wv = hook("local_kv", (_gather_tokens(k, idx_k), _gather_tokens(v, idx_k)))
    dots = scale * torch.einsum("bhwie,bhwje->bhwij", wq, wk)
    if bias is not None:
        dots = dots + hook("bias", bias.to(dtype))[None, :, None]
    blocked = _gather_mask(mask, idx_k)[:, None, :, None, :]                 # [B,1,G,1,Wk]: padded or absent keys
    if causal:
        blocked = blocked | _gather_mask(mask, idx_qg)[:, None, :, :, None]
    if causal == 2:
        i = torch.arange(Wq).view(-1, 1)
        j = torch.arange(Wk).view(1, -1)
        blocked = blocked | (j - i >= 1 + e)[None, None, None]
    dots = hook("local_logits", dots.masked_fill(blocked, MASK_VAL))
    vals, logits = wv, dots
    L = 0 if lk is None else lk.shape[2]
    if L:
        lk_w, lv_w = hook("lm_kv", (lk.to(dtype)[:, :, None].expand(B, h, G, L, d), lv.to(dtype)[:, :, None].expand(B, h, G, L, d)))
        cv = scale * torch.einsum("bhwid,bhwcd->bhwic", wq, lk_w)
        ctx["cv_raw"] = cv
        if causal == 2:
            q_chunk = torch.div(idx_q, chunk, rounding_mode="floor").unsqueeze(-1)          # [G,Wq,1]
            cv = cv.masked_fill((torch.arange(L).view(1, 1, -1) >= q_chunk)[None, None], MASK_VAL)
        logits = torch.cat([dots, hook("lm_logits", cv)], -1)
        vals = torch.cat([wv, lv_w], -2)
    keepmul = None
    if keep is not None:
        kq = torch.cat([keep, keep.new_zeros(B, h, 1, Wk + L)], 2)[:, :, torch.where(idx_qg < 0, torch.full_like(idx_qg, n), idx_qg)]
        keepmul = hook("keepmul", kq.to(dtype) * keep_scale)                 # [B,h,G,Wq,Wk+L]
    if round_to is None:
        p = torch.softmax(logits, -1)
        out_w = torch.matmul(p if keepmul is None else p * keepmul, vals)
        lse_w = torch.logsumexp(logits, -1)
    else:
        out_w, lse_w = _ModelAttn.apply(logits, vals, keepmul, round_to)
    out = _scatter_windows(out_w, idx_q, n_pad)[:, :, :n]
    lse = _scatter_windows(lse_w.unsqueeze(-1), idx_q, n_pad)[:, :, :n, 0]
    return out, lse


def window_grads(q, k, v, lk, lv, dout, dlse=None, *, store="single", **kw):
    """Forward and gradients of window_core for the loss <out, dout> (+ <lse, dlse>): dict with out, lse, dq, dk, dv and, where
    given, dlk, dlv, dbias.  With round_to set, dq / dk / dv carry the rounding of their store; store = 'cdirect' models the
    half-window plan (class 0 = even windows store, class 1 = odd windows add: two roundings of dk / dv)."""
    dtype, round_to = kw.get("dtype", torch.float64), kw.get("round_to")
    bias = kw.pop("bias", None)
    leaves = {"dq": q, "dk": k, "dv": v, "dlk": lk, "dlv": lv, "dbias": bias}
    leaves = {n_: t.detach().to(dtype).requires_grad_(True) for n_, t in leaves.items() if t is not None}
    out, lse = window_core(leaves["dq"], leaves["dk"], leaves["dv"], leaves.get("dlk"), leaves.get("dlv"), bias=leaves.get("dbias"), **kw)
    dout = dout.to(dtype)
    gl = torch.zeros_like(lse) if dlse is None else dlse.to(dtype)
    names = list(leaves)

    def grads(go):
        gs = torch.autograd.grad([out, lse], [leaves[n_] for n_ in names], [go, gl], retain_graph=True, allow_unused=True)
        return {n_: (torch.zeros_like(leaves[n_]) if g is None else g) for n_, g in zip(names, gs)}
    if store == "cdirect":
        n, w = q.shape[2], kw["w"]
        even = ((torch.arange(n) // w) % 2 == 0).to(dtype).view(1, 1, n, 1)
        assert dlse is None
        g0, g1 = grads(dout * even), grads(dout * (1 - even))
        res = {n_: g0[n_] + g1[n_] for n_ in names}
        for n_ in ("dk", "dv"):
            res[n_] = rnd(rnd(g0[n_], round_to) + g1[n_], round_to)
        res["dq"] = rnd(res["dq"], round_to)
    else:
        res = grads(dout)
        for n_ in ("dq", "dk", "dv"):
            res[n_] = rnd(res[n_], round_to)
    res["out"], res["lse"] = out.detach(), lse.detach()
    return res


# ------------------------------------------------------------------------------------------------------------------------
# landmark passes (oracle/attention.py:226-236; header of csrc/ea_eva_landmark.hip)
# ------------------------------------------------------------------------------------------------------------------------
def chunk_table(n, r, e, attn_2d=False, seq_shape=None, causal=0):
    """[C, J] token of slot j of chunk c, -1 outside (chunks of the causal geometry are never extended)."""
    if attn_2d:
        return window_index_2d(seq_shape[0], seq_shape[1], r, e)
    return window_index_1d(n, r, 0 if causal else e)


def chunk_colours(n, r, e, attn_2d=False, seq_shape=None, causal=0):
    """Colour class of every chunk in launch order: chunks closer than nc = 1 + ceil(2e / r) per axis share tokens."""
    e = 0 if causal else e
    nc = 1 + -(-2 * e // r) if e > 0 else 1
    if attn_2d:
        per_row = seq_shape[1] // r
        c = torch.arange((seq_shape[0] // r) * per_row)
        return ((c // per_row) % nc) * nc + (c % per_row) % nc, nc * nc
    return torch.arange(n // r) % nc, nc


def _masked_chunks(t, idx_c, cmask):
    return _gather_tokens(t, idx_c) * (~cmask)[:, None, :, :, None].to(t.dtype)


def chunk_mean_core(q, k, mask, *, r, e=0, attn_2d=False, seq_shape=None, causal=0, dtype=torch.float64):
    """-> (qmean, kmean) [B,h,C,d]: sums over the unmasked in-range slots of every chunk divided by the slot count J."""
    B, h, n, d = q.shape
    idx_c = chunk_table(n, r, e, attn_2d, seq_shape, causal)
    mask = torch.zeros(B, n, dtype=torch.bool) if mask is None else mask.bool()
    cmask = _gather_mask(mask, idx_c)
    return _masked_chunks(q.to(dtype), idx_c, cmask).mean(-2), _masked_chunks(k.to(dtype), idx_c, cmask).mean(-2)


def beta_core(k, v, omega, mask, *, r, e=0, attn_2d=False, seq_shape=None, causal=0, dtype=torch.float64, scale=None):
    """-> beta [B,h,C,d]; padded and outside slots count as zero rows with the finite -5e4 logit."""
    B, h, n, d = k.shape
    scale = d ** -0.5 if scale is None else scale
    idx_c = chunk_table(n, r, e, attn_2d, seq_shape, causal)
    mask = torch.zeros(B, n, dtype=torch.bool) if mask is None else mask.bool()
    cmask = _gather_mask(mask, idx_c)
    ck, cv = _masked_chunks(k.to(dtype), idx_c, cmask), _masked_chunks(v.to(dtype), idx_c, cmask)
    logit = scale * torch.einsum("bhcd,bhcjd->bhcj", omega.to(dtype), ck) - 0.5 * scale * (ck * ck).sum(-1)
    logit = logit.masked_fill(cmask[:, None], MASK_VAL)
    return torch.einsum("bhcj,bhcjd->bhcd", torch.softmax(logit, -1), cv)


def beta_grads(k, v, omega, mask, dbeta, dk0, dv0, *, round_to=None, dtype=torch.float64, **geo):
    """beta and the gradients of <beta, dbeta>: d_omega, and dk / dv ADDED to the existing rows dk0 / dv0 the way ea_eva_beta_bwd
    does -- one read-modify-write (one rounding) per colour class of the chunks, classes in launch order."""
    k_, v_, om = [t.detach().to(dtype).requires_grad_(True) for t in (k, v, omega)]
    beta = beta_core(k_, v_, om, mask, dtype=dtype, **geo)
    col, ncol = chunk_colours(k.shape[2], geo["r"], geo.get("e", 0), geo.get("attn_2d", False), geo.get("seq_shape"), geo.get("causal", 0))
    dk, dv, dom = dk0.to(dtype), dv0.to(dtype), torch.zeros_like(om)
    for cl in range(ncol):
        sel = (col == cl).to(dtype).view(1, 1, -1, 1)
        gk, gv, go = torch.autograd.grad(beta, [k_, v_, om], dbeta.to(dtype) * sel, retain_graph=True)
        dk, dv, dom = rnd(dk + gk, round_to), rnd(dv + gv, round_to), dom + go
    return dict(beta=beta.detach(), d_omega=dom, dk=dk, dv=dv)


def chunk_mean_grads(q, k, mask, dqmean, dkmean, dq0, dk0, *, round_to=None, dtype=torch.float64, **geo):
    """Chunk means and the gradients of <qmean, dqmean> + <kmean, dkmean> added to the existing rows dq0 / dk0: one rounding per
    token (disjoint chunks: one read-modify-write each; overlapping chunks: the token-centric gather kernel)."""
    q_, k_ = [t.detach().to(dtype).requires_grad_(True) for t in (q, k)]
    qm, km = chunk_mean_core(q_, k_, mask, dtype=dtype, **geo)
    gq, gk = torch.autograd.grad([qm, km], [q_, k_], [dqmean.to(dtype), dkmean.to(dtype)])
    return dict(qmean=qm.detach(), kmean=km.detach(), dq=rnd(dq0.to(dtype) + gq, round_to), dk=rnd(dk0.to(dtype) + gk, round_to))


# ------------------------------------------------------------------------------------------------------------------------
# the model-relative bound
# ------------------------------------------------------------------------------------------------------------------------
def a_err(x, ref):
    """max_i |x_i - ref_i| / (rms(ref) + |ref_i|): util.elementwise_excess with a = b = 1 (nan / inf in x: inf)."""
    x, ref = x.detach().double(), ref.detach().double()
    if not bool(torch.isfinite(x).all()):
        return float("inf")
    rms = float(ref.pow(2).mean().sqrt())
    return float(((x - ref).abs() / (rms + ref.abs()).clamp_min(1e-300)).max())


def norm_errs(x, ref):
    """util.scaled_err: (max |err| / max |ref|, rms(err) / rms(ref))."""
    x, ref = x.detach().double(), ref.detach().double()
    if not bool(torch.isfinite(x).all()):
        return float("inf"), float("inf")
    dlt = x - ref
    return (float(dlt.abs().max() / ref.abs().max().clamp_min(1e-30)),
            float(dlt.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30)))


FACTOR = 4.0          # 2 (what M does not model: fp32 accumulation order, v_exp, the log2-domain rescale) x 2 (spread of a maximum
                      # over 1e4 .. 1e7 independently rounded elements); fixed in advance, not fitted


def floor_for(name, round_to):
    """f of the bound: half an ulp of the largest element for tensors stored in 16 bits, 2^-20 for fp32 results (under fp32 I/O,
    round_to = torch.float32, every result is one)."""
    if round_to == torch.float32:
        return 2.0 ** -20
    if name in ("out", "dq", "dk", "dv"):
        return 2.0 ** -9 if round_to == torch.bfloat16 else 2.0 ** -12
    return 2.0 ** -20


def bound_report(name, got, model, ref, round_to):
    """(ok, text): a(got) <= 4 a(model) + f and the same for the two norm-wise figures."""
    f = floor_for(name, round_to)
    ag, am = a_err(got, ref), a_err(model, ref)
    ng, nm = norm_errs(got, ref), norm_errs(model, ref)
    ok = ag <= FACTOR * am + f and ng[0] <= FACTOR * nm[0] + f and ng[1] <= FACTOR * nm[1] + f
    txt = "%-7s a=%.3e (model %.3e, ratio %.2f)  max=%.3e (model %.3e)  rms=%.3e (model %.3e)  f=%.1e%s" % (
        name, ag, am, ag / max(am, 1e-300), ng[0], nm[0], ng[1], nm[1], f, "" if ok else "   <-- EXCEEDS")
    return ok, txt, ag / max(am, 1e-300)
