"""Same-operand reference of the 16-bit LARA estimator core (plain torch, CPU; imports nothing of the product): exactly what
_ops.LaraAttnFn receives -- q, k, v [B,h,N,d], the landmark-side OPERANDS omega, qbar [B,h,C,d] and bhv, lp [B,h,C] -- through
the formulas of include/ea_hip.h (the LARA block; reference lara.py:177-251):

    lpk[c,m]  = s w_c.k_m - s |k_m|^2 / 2   (-inf on padded keys)      kv_c = sum_m softmax_m(lpk) v_m      lse_k = LSE_m lpk
    mis-opt   : t = softmax_n(s qbar_c.q_n), alpha = bhv_c + kappa (t - mean_c t), log_alpha = log max(alpha, 1e-8)
    mis-biased: log_alpha = s qbar_c.q_n                 mis-bh: log_alpha = 0
    W = softmax_c(log_alpha + s w_c.q_n + lse_k[c] - lp_c)             out_n = sum_c W[c,n] kv_c

Gradients of <out, dout> come from autograd; lse_k is in natural-log units.

Two evaluations of the same function:
  R  exact reference: dtype = torch.float64, round_to = None (plain torch, autograd).
  M  rounding model : dtype = torch.float32, round_to = torch.bfloat16 | torch.float16 -- the arithmetic of the kernels in
     fp32 with the 16-bit roundings they document, forward and backward written out (_ModelLara; with round_to = None it is
     the exact function again, which tests/test_lara_reference_cpu.py holds against autograd).  Paths below are under
     efficient-attention_amd/csrc/.
       landmark matrices   omega, qbar, kv, d kv_stats and u qbar are fp32 in memory and are converted to the MFMA element type
                           when a pass stages them: ea_lara_f.hip:34-36 (stage_rows3, :63-64; the merged d kv_stats rows :565),
                           ea_lara_x_body.h:127-128, :207-218 (the merged kv rows :199), ea_lara_y.hip:32-40 (conv_lm_frag).
                           The fp32 originals stay in the scalar algebra: dkk = dkv . kv (ea_lara_f.hip:561-563,
                           ea_lara_merge.hip:176-178), u qbar (ea_lara_f.hip:610-611, ea_lara_merge.hip:187)
       forward statistics  the unnormalised exp2(lpk - m) is packed before P.v, its normaliser sums the unrounded values
                           (ea_lara_y.hip:324-329); kv = sum / l, lse_k and lse_t stay fp32 (ea_lara_merge.hip:45-49, :85-86;
                           ea_lara_x_body.h:196-203)
       forward combine     the unnormalised W = alpha 2^(z - max) is packed before W.kv (ea_lara_x_body.h:545-546), the
                           normaliser sums the unrounded values (:359-362); out is stored in the I/O dtype (:573-575 / :609-611)
       query side          rd = sum_c W dW and d alpha use the unrounded W (ea_lara_f.hip:259-262, :278; ea_lara_x_body.h:381-383,
                           :395); W, dZ, t dt and t are packed (ea_lara_f.hip:283-284, :300-305; ea_lara_x_body.h:545-549;
                           ea_lara_y.hip:345-346) for dq = s (omega^T dZ + qbar^T t dt) and for the per-landmark contractions
                           d kv_stats = sum_n W dout, sum_n dZ q, sum_n t dt q, sum_n t q; dq is stored in the I/O dtype
                           (ea_lara_f.hip:339-341 / :349; ea_lara_x_body.h:631).  The scalar sums r_c = sum_n dZ and
                           u_c = sum_n t dt add the PACKED slabs in the fused pass (an MFMA against ones, ea_lara_f.hip:390-391)
                           and the unrounded values in the two-pass route (ea_lara_y.hip:267-269); d bhv = sum_n d alpha is
                           unrounded in both (ea_lara_f.hip:279-280, ea_lara_y.hip:267)
       key side            Pk and dB = Pk (dW - dkk + r) are packed for dv = dkv^T Pk, dk = s omega^T dB - s k sum_c dB (the sum
                           over c unrounded) and d omega (key part) = sum_m dB k (ea_lara_f.hip:688, :699-702, :738, :750-751;
                           ea_lara_x_body.h:529, :545-549, :670; ea_lara_y.hip:345); dk and dv are stored in the I/O dtype
                           (ea_lara_f.hip:721-722 / :731, :739; ea_lara_x_body.h:661, :672)
       finish (mis-opt)    t is recomputed from the staged qbar and packed, u qbar is staged (ea_lara_f.hip:833-835, :870-871;
                           ea_lara_x_body.h:137, :508, :545-546); the stored dq is read, corrected and stored again -- a second
                           rounding of dq (ea_lara_f.hip:900-908; ea_lara_x_body.h:650-656)
     (fp32 accumulation order, the online-softmax rescales, v_exp / v_rcp and the log2 domain are not modelled: that is what
      window_reference.FACTOR is for)
"""
import torch

from window_reference import FACTOR, a_err, bound_report, floor_for, norm_errs, rnd   # noqa: F401  (re-exported for the tests)

MIS = {"opt": 0, "biased": 1, "bh": 2}
CLAMP = 1e-8

# single deliberate defects of the model (tests/test_lara_reference_cpu.py plays them as "the kernel")
DEFECTS = ("tmean_over_padded_slots", "padded_keys_in_lse_k", "lp_dropped", "kv_slice_missing", "tail_tokens_missing",
           "uq_correction_missing", "kappa_missing_in_backward", "dlp_wrong_sign")


def _log_proj(omega, x, scale):
    """[B,h,C,N]: s w_c.x_n - s |x_n|^2 / 2."""
    return scale * torch.einsum("bhcd,bhnd->bhcn", omega, x) - 0.5 * scale * (x * x).sum(-1).unsqueeze(-2)


def lara_alpha(q, qbar, bhv, *, kappa, scale, dtype=torch.float64):
    """alpha [B,h,C,N] of mis-opt before the clamp."""
    t = torch.softmax(scale * torch.einsum("bhcd,bhnd->bhcn", qbar.to(dtype), q.to(dtype)), -1)
    return bhv.to(dtype).unsqueeze(-1) + kappa * (t - t.mean(-2, keepdim=True))


class _ModelLara(torch.autograd.Function):
    """The estimator with the kernels' roundings, forward and backward (module docstring).  cfg: mis, kappa, scale, round_to,
    fused (C <= 64: ea_lara_f.hip; else the two-pass kernels), defect (None | one of DEFECTS)."""

    @staticmethod
    def forward(ctx, q, k, v, omega, qbar, bhv, lp, mask, cfg):
        mis, kappa, s, r16, defect = cfg["mis"], cfg["kappa"], cfg["scale"], cfg["round_to"], cfg.get("defect")
        B, h, N, d = q.shape
        C = omega.shape[2]
        use_t = mis != 2
        om16 = rnd(omega, r16)
        qb16 = rnd(qbar, r16) if use_t else None
        dead = torch.zeros(B, 1, 1, N, dtype=torch.bool) if mask is None else mask.bool()[:, None, None, :]
        # ---- statistics pass ----
        lpk = _log_proj(om16, k, s).masked_fill(dead, float("-inf"))
        mx = lpk.amax(-1, keepdim=True)
        pu = torch.exp(lpk - mx)
        l = pu.sum(-1, keepdim=True)
        if defect == "padded_keys_in_lse_k":
            l = torch.exp(_log_proj(om16, k, s) - mx).sum(-1, keepdim=True)
        pu_n = pu
        if defect == "kv_slice_missing":
            pu_n = pu.clone()
            pu_n[..., 64:] = 0
        kv = torch.matmul(rnd(pu_n, r16), v) / l
        lse_k = (mx + torch.log(l)).squeeze(-1)
        T = s * torch.einsum("bhcd,bhnd->bhcn", qb16, q) if use_t else None
        lse_t = torch.logsumexp(T, -1) if mis == 0 else None
        cst = lse_k if defect == "lp_dropped" else lse_k - lp
        # ---- combine pass ----
        kv16 = rnd(kv, r16)
        A = s * torch.einsum("bhcd,bhnd->bhcn", om16, q)
        invC = 1.0 / (16 * ((C + 15) // 16)) if defect == "tmean_over_padded_slots" else 1.0 / C
        z = A + cst.unsqueeze(-1)
        t = tmean = alpha = None
        if mis == 0:
            t = torch.exp(T - lse_t.unsqueeze(-1))
            tmean = t.sum(-2, keepdim=True) * invC
            alpha = kappa * t + (bhv.unsqueeze(-1) - kappa * tmean)
            al = alpha.clamp(min=CLAMP)
        elif mis == 1:
            z = z + T
        mz = z.amax(-2, keepdim=True)
        ez = torch.exp(z - mz)
        wv = ez * al if mis == 0 else ez
        ssum = wv.sum(-2, keepdim=True)
        out = rnd(torch.einsum("bhcn,bhcd->bhnd", rnd(wv, r16), kv16) / ssum.transpose(-1, -2), r16)
        lseZ = mz + torch.log(ssum)
        ctx.cfg, ctx.mask_dead, ctx.invC = cfg, dead, invC
        ctx.saved = (q, k, v, om16, qb16, qbar, kv, kv16, lse_k, lse_t, z, lseZ, t, alpha)
        return out, kv, lse_k

    @staticmethod
    def backward(ctx, dout, _dkv_ext, _dlse_ext):
        cfg, dead, invC = ctx.cfg, ctx.mask_dead, ctx.invC
        mis, kappa, s, r16, defect, fused = cfg["mis"], cfg["kappa"], cfg["scale"], cfg["round_to"], cfg.get("defect"), cfg["fused"]
        q, k, v, om16, qb16, qbar, kv, kv16, lse_k, lse_t, z, lseZ, t, alpha = ctx.saved
        N = q.shape[2]
        # ---- query side ----
        dw = torch.einsum("bhcd,bhnd->bhcn", kv16, dout)
        wz = torch.exp(z - lseZ)
        W = wz * alpha.clamp(min=CLAMP) if mis == 0 else wz
        rd = (W * dw).sum(-2, keepdim=True)
        dd = dw - rd
        dz = W * dd
        dz16 = rnd(dz, r16)
        W16 = rnd(W, r16)
        tdt = tdt16 = t16 = da = None
        if mis == 0:
            da = torch.where(alpha > CLAMP, wz * dd, torch.zeros_like(dd))
            kb = 1.0 if defect == "kappa_missing_in_backward" else kappa
            tdt = t * kb * (da - da.sum(-2, keepdim=True) * invC)
            tdt16, t16 = rnd(tdt, r16), rnd(t, r16)
        elif mis == 1:
            tdt, tdt16 = dz, dz16
        dq = torch.einsum("bhcn,bhcd->bhnd", dz16, om16)
        if mis != 2:
            dq = dq + torch.einsum("bhcn,bhcd->bhnd", tdt16, qb16)
        dq = rnd(s * dq, r16)
        # per-landmark sums over the tokens
        nn = N - N % 16 if defect == "tail_tokens_missing" else N

        def over_n(wgt, rows):
            return torch.einsum("bhcn,bhnd->bhcd", wgt[..., :nn], rows[:, :, :nn])
        dkv = over_n(W16, dout)
        domq = over_n(dz16, q)
        r = (dz16 if fused else dz)[..., :nn].sum(-1)
        d_lp = r if defect == "dlp_wrong_sign" else -r
        d_qbar = d_bhv = uq = None
        if mis == 0:
            u = (tdt16 if fused else tdt)[..., :nn].sum(-1).unsqueeze(-1)
            d_qbar = s * (over_n(tdt16, q) - u * over_n(t16, q))
            uq = u * qbar
            d_bhv = da[..., :nn].sum(-1)
        elif mis == 1:
            d_qbar = s * domq
        dkk = (dkv * kv).sum(-1)
        # ---- key side ----
        dkv16 = rnd(dkv, r16)
        lpk = _log_proj(om16, k, s)
        pk = torch.exp(lpk - lse_k.unsqueeze(-1)).masked_fill(dead, 0.0)
        db = pk * (torch.einsum("bhcd,bhmd->bhcm", dkv16, v) - dkk.unsqueeze(-1) + r.unsqueeze(-1))
        db16 = rnd(db, r16)
        dv = rnd(torch.einsum("bhcm,bhcd->bhmd", rnd(pk, r16), dkv16), r16)
        dk = rnd(s * torch.einsum("bhcm,bhcd->bhmd", db16, om16) - s * k * db.sum(-2).unsqueeze(-1), r16)
        d_omega = s * (domq + torch.einsum("bhcm,bhmd->bhcd", db16, k))
        # ---- finish: the softmax-over-sequence correction of t ----
        if mis == 0 and defect != "uq_correction_missing":
            tf = torch.exp(s * torch.einsum("bhcd,bhnd->bhcn", qb16, q) - lse_t.unsqueeze(-1))
            dq = rnd(dq - s * torch.einsum("bhcn,bhcd->bhnd", rnd(tf, r16), rnd(uq, r16)), r16)
        return dq, dk, dv, d_omega, d_qbar, d_bhv, d_lp, None, None


def lara_estimator(q, k, v, mask, omega, qbar, bhv, lp, *, mis, kappa, scale, dtype, round_to=None, model=None, defect=None):
    """q, k, v [B,h,N,d]; mask [B,N] bool (True = padded key) or None; omega, qbar [B,h,C,d]; bhv, lp [B,h,C]; mis 'opt' | 'biased'
    | 'bh' (qbar unused for bh, bhv for biased / bh).  -> (out [B,h,N,d], kv [B,h,C,d], lse_k [B,h,C]).
    round_to = None: the exact function in plain torch; else the rounding model (model = True forces the model's arithmetic
    with round_to = None as well; defect: test-only, one of DEFECTS)."""
    m = MIS[mis]
    q, k, v, omega, lp = [x.to(dtype) for x in (q, k, v, omega, lp)]
    qbar = None if (qbar is None or m == 2) else qbar.to(dtype)
    bhv = None if (bhv is None or m != 0) else bhv.to(dtype)
    if model is None:
        model = round_to is not None or defect is not None
    if model:
        cfg = dict(mis=m, kappa=float(kappa), scale=float(scale), round_to=round_to, fused=omega.shape[2] <= 64, defect=defect)
        return _ModelLara.apply(q, k, v, omega, qbar, bhv, lp, mask, cfg)
    lpk = _log_proj(omega, k, scale)
    if mask is not None:
        lpk = lpk.masked_fill(mask.bool()[:, None, None, :], float("-inf"))
    kv = torch.einsum("bhcm,bhmd->bhcd", torch.softmax(lpk, -1), v)
    lse_k = torch.logsumexp(lpk, -1)
    if m == 0:
        t = torch.softmax(scale * torch.einsum("bhcd,bhnd->bhcn", qbar, q), -1)
        alpha = bhv.unsqueeze(-1) + kappa * (t - t.mean(-2, keepdim=True))
        log_alpha = torch.log(alpha.clamp(min=CLAMP))
    elif m == 1:
        log_alpha = scale * torch.einsum("bhcd,bhnd->bhcn", qbar, q)
    else:
        log_alpha = 0.0
    W = torch.softmax(log_alpha + scale * torch.einsum("bhcd,bhnd->bhcn", omega, q) + (lse_k - lp).unsqueeze(-1), -2)
    return torch.einsum("bhcn,bhcd->bhnd", W, kv), kv, lse_k


def lara_grads(q, k, v, mask, omega, qbar, bhv, lp, dout, *, mis, batch_step=8, **kw):
    """Forward and gradients of lara_estimator for the loss <out, dout>: dict with out, kv, lse_k, dq, dk, dv, d_omega, d_lp and
    d_qbar (opt, biased), d_bhv (opt).  Landmark tensors belong to one (b, h): evaluated in batch slices of `batch_step`."""
    dtype = kw["dtype"]
    m = MIS[mis]
    B = q.shape[0]
    parts = []
    for b0 in range(0, B, batch_step):
        sl = slice(b0, b0 + batch_step)
        leaves = dict(dq=q[sl], dk=k[sl], dv=v[sl], d_omega=omega[sl], d_lp=lp[sl])
        if m != 2:
            leaves["d_qbar"] = qbar[sl]
        if m == 0:
            leaves["d_bhv"] = bhv[sl]
        leaves = {n_: x.detach().to(dtype).requires_grad_(True) for n_, x in leaves.items()}
        out, kv, lse_k = lara_estimator(leaves["dq"], leaves["dk"], leaves["dv"], None if mask is None else mask[sl], leaves["d_omega"],
                                        leaves.get("d_qbar"), leaves.get("d_bhv"), leaves["d_lp"], mis=mis, **kw)
        names = list(leaves)
        gs = torch.autograd.grad(out, [leaves[n_] for n_ in names], dout[sl].to(dtype))
        res = dict(zip(names, gs))
        res.update(out=out.detach(), kv=kv.detach(), lse_k=lse_k.detach())
        parts.append(res)
    return {n_: torch.cat([p_[n_] for p_ in parts], 0) for n_ in parts[0]}
