"""Same-operand reference of the LARA / EVA landmark pipeline (plain torch, CPU; imports nothing of the product): exactly what
ea_lara_landmarks_fwd / _bwd / _bwd_parts / _fwd_cb / _bwd_cb receive -- pooled rows pq, pk [BH,L,D], the eight parameters of the
two Linear + LayerNorm bodies, the noise draw, the '-vmixed' column bias and the incoming gradients, all fp32 -- through the
formulas of include/ea_hip.h (the landmark block) and oracle/attention.py (_mlp, lara_landmarks_2d, lara_core, eva_core):

    q_bar = LN(pq Wq^T + bq) gq + cq, k0 = LN(pk Wk^T + bk) gk + ck           (has_mlp; else q_bar = pq, k0 = pk; eps 1e-5)
    A = softmax_l'(s k0 k0^T + colbias[None, :]), k_bar = A k0                   (mixed; else k_bar = k0)
    mu = q_bar + k_bar;  omega by dup: 0 mu + eps | 1 cat(mu + eps, mu - eps) | 2 mu.repeat(2) + eps
    M[c,l] = s omega_c.mu_l - s |mu_l|^2 / 2                                   (prm_log_features(mu, omega))
    mis-opt   : lp_c = M[c, c mod L], bhv_c = exp(lp_c - LSE over the C repeated columns), qbar_rows = q_bar.repeat
    mis-biased: lp_c = LSE_l M[c,l], qbar_rows = mu.repeat;     mis-bh: lp_c = LSE_l M[c,l], no qbar_rows
    eva       : qbar_rows = k0, omega = (q_bar + k0) / 2 + eps

The parameters are given to the function as per-(b,h) copies, so that their gradients are the kernel's per-(b,h) partials
dW_part [BH,2,D,D] (q then k; [out][in]) and dvec_part [BH,2,3,D] (Linear bias, LN weight, LN bias) slice by slice.  The loss is
sum(out * g) over d_omega, d_qbar_rows, d_bhv, d_lp; with `parts` the gradient of omega is dom_scale (d_omega + sum_s parts[s]).

Two evaluations:
  R  exact reference: fp64, forward in plain torch (F.layer_norm, softmax, logsumexp, the diagonal of the [C x C] matrix),
     gradients from autograd.
  M  rounding model: the kernel's arithmetic written out forward and backward in fp32 (_ModelLmk) with the roundings
     lmk2_kernel performs.  Every MFMA operand is fp16 whatever the I/O dtype.  Lines of efficient-attention_amd/csrc/ea_lmk2.hip
     (ea_strip.h where said):
       forward   pq, pk, Wq, Wk packed to fp16 by commit_rows (:44-56, pack8<H> at :55; staged at :153-156); the Linear bias, the
                 LayerNorm and its affine stay fp32 (:167-177)
                 k0 packed at scale 1 (:203) for G = s k0 k0^T (:208) and k_bar = A k0 (:235); the softmax is fp32 (:209-231),
                 A is saved in fp32 (:232) and packed at scale 1 (:233)
                 mu = q_bar + k_bar in fp32, |mu|^2 from the UNROUNDED mu (:245-247); mu packed at scale 1 (:253), omega packed at
                 scale 1 (:276) for M (:281); the stored omega and qbar_rows are the fp32 values (:274-275); densities fp32 (:282-313)
       backward  mu, omega, k0, A packed again from the saved fp32 strips (:433-437), |mu|^2 fp32 (:423-429); M and the densities
                 recomputed (:446-473)
                 dM packed as rnd16(dM 2^-e) 2^e, e from the absolute maximum over the valid C x L block (:491, :497-498;
                 strip_absmax ea_strip.h:156-165, pow2_scale ea_strip.h:167-173); the fp32 dM stays in s colsum(dM) mu (:495, :512, :519)
                 d k_bar packed the same way over L x D (:548, :552-553) for dK0 = A^T dKb (:557) and dA = dKb K0^T (:558); the
                 softmax backward uses the fp32 A and dA (:563-569); d colbias sums the fp32 dG (:570, :577); dG packed over L x L
                 (:572, :578-579) for dG K0 + dG^T K0 (:583-584)
                 d gamma, d beta sum the fp32 dY (:605-623); the LayerNorm backward is fp32 (:626-644); the Linear bias gradient
                 sums the fp32 dH (:648-649, :656-657); dH_q, dH_k packed over L x D (:651-652, :659-662) for dP = dH W (:668, :673)
                 and dW = dH^T P (:680, :685) against the fp16 W and P tiles (:365-366 / :414-415)
     Not modelled (what window_reference.FACTOR is for): fp32 accumulation order, __expf / __logf / rsqrtf.
     With roundings off (round16 = False, fp64) M equals the autograd of R: tests/test_lmk_reference_cpu.py holds it to 1e-10.
"""
import math

import torch
import torch.nn.functional as F

from window_reference import FACTOR, a_err, bound_report, floor_for, norm_errs, rnd   # noqa: F401  (re-exported for the tests)

MIS = {"opt": 0, "biased": 1, "bh": 2}
PARAMS = ("Wq", "bq", "gq", "cq", "Wk", "bk", "gk", "ck")
OUTPUTS = ("omega", "qbar_rows", "bhv", "lp")
GRADS = ("dpq", "dpk", "dW_part", "dvec_part", "d_colbias")
H16 = torch.float16

# single deliberate defects of the model (tests/test_lmk_reference_cpu.py plays them as "the kernel")
DEFECTS = ("antithetic_sign_missing", "nrep_missing_in_normaliser", "pad_columns_unmasked", "colbias_along_rows",
           "fold_missing", "dqs_first_copy_only", "eva_half_missing", "dom_scale_on_d_omega_only", "dgamma_dbeta_swapped",
           "ln_xhat_term_dropped")


def _noise_rows(noise, dup, defect=None):
    """eps of the C sample rows: antithetic rows c >= L re-use the first L rows with the opposite sign."""
    if noise is None:
        return None
    if dup == 1:
        return torch.cat([noise, noise if defect == "antithetic_sign_missing" else -noise], 1)
    return noise


def _bmm_t(a, b):
    return torch.matmul(a, b.transpose(-1, -2))


# ------------------------------------------------------------------------------------------------------------------------
# R: the operation in plain torch
# ------------------------------------------------------------------------------------------------------------------------
def mlp(x, W, b, gamma, beta):
    """Linear + LayerNorm (eps 1e-5, affine) with per-(b,h) parameters: x [BH,L,D], W [BH,D,D] ([out][in]), b, gamma, beta [BH,D]."""
    y = _bmm_t(x, W) + b[:, None]
    return F.layer_norm(y, (y.shape[-1],), None, None, 1e-5) * gamma[:, None] + beta[:, None]


def mixing(k0, colbias, scale):
    """k_bar = softmax(s k0 k0^T + colbias[None, :]) k0 (lara.py:157-174); -> (k_bar, A)."""
    logits = scale * _bmm_t(k0, k0)
    if colbias is not None:
        logits = logits + colbias[:, None, :]
    A = torch.softmax(logits, -1)
    return torch.matmul(A, k0), A


def prm(data, proj, scale):
    """oracle.attention.prm_log_features on [BH, ., D] tensors: out[c,n] = s proj_c.data_n - s |data_n|^2 / 2."""
    return scale * _bmm_t(proj, data) - 0.5 * scale * (data * data).sum(-1).unsqueeze(-2)


def lmk_forward(pq, pk, P, noise, colbias, c):
    """The pipeline in plain torch on tensors of one dtype.  P: dict of per-(b,h) parameters or None.  -> dict with omega,
    qbar_rows, bhv, lp (None where the geometry has none) and the intermediates q_bar, k0, k_bar, A, mu."""
    L, dup, s = c["L"], c["dup"], c["scale"]
    rep = 2 if dup else 1
    if c["has_mlp"]:
        q_bar, k0 = mlp(pq, P["Wq"], P["bq"], P["gq"], P["cq"]), mlp(pk, P["Wk"], P["bk"], P["gk"], P["ck"])
    else:
        q_bar, k0 = pq, pk
    if c["eva"]:
        omega = 0.5 * (q_bar + k0)
        return dict(omega=omega if noise is None else omega + noise, qbar_rows=k0, bhv=None, lp=None, q_bar=q_bar, k0=k0, A=None, mu=None)
    A = None
    k_bar = k0
    if c["mixed"]:
        k_bar, A = mixing(k0, colbias, s)
    mu = q_bar + k_bar
    if dup == 1:
        omega = torch.cat([mu + noise, mu - noise], 1)
    elif dup == 2:
        omega = mu.repeat(1, 2, 1) + noise
    else:
        omega = mu if noise is None else mu + noise
    mis = MIS[c["mis"]]
    bhv = qrows = None
    if mis == 0:
        lpmu = prm(mu.repeat(1, rep, 1), omega, s)                                # [BH,C,C]: the repeated mu columns counted
        lp = torch.diagonal(lpmu, dim1=-1, dim2=-2)
        bhv = torch.exp(lp - torch.logsumexp(lpmu, -1))
        qrows = q_bar.repeat(1, rep, 1)
    else:
        lp = torch.logsumexp(prm(mu, omega, s), -1)
        if mis == 1:
            qrows = mu.repeat(1, rep, 1)
    return dict(omega=omega, qbar_rows=qrows, bhv=bhv, lp=lp, q_bar=q_bar, k0=k0, k_bar=k_bar, A=A, mu=mu)


# ------------------------------------------------------------------------------------------------------------------------
# M: the kernel's arithmetic, forward and backward
# ------------------------------------------------------------------------------------------------------------------------
def _pow2_pack(x, on):
    """rnd16(x 2^-e) 2^e with e from the absolute maximum of every (b,h) block (pow2_scale: max * scale in [0.5, 1); 1 for an
    all-zero or non-finite block)."""
    if not on:
        return x
    m = x.abs().amax((-1, -2), keepdim=True)
    _, e = torch.frexp(m)
    sc = torch.where((m > 0) & (m <= 3e38), torch.ldexp(torch.ones_like(m), -e), torch.ones_like(m))
    return rnd(x * sc, H16) / sc


class _ModelLmk(torch.autograd.Function):
    """lmk2_kernel<D, false> and <D, true> (module docstring).  cfg: the case's geometry + round16 (bool) + defect."""

    @staticmethod
    def _lin_ln(p, W, b, r):
        h = _bmm_t(r(p), r(W)) + b[:, None]
        c0 = h - h.mean(-1, keepdim=True)
        rstd = torch.rsqrt((c0 * c0).mean(-1, keepdim=True) + 1e-5)
        return c0 * rstd, rstd

    @staticmethod
    def _densities(mu, noise, cfg, r):
        """omega rows, M, the normaliser and the diagonal of the sample rows, as F4 / F5 and B1 form them."""
        L, C, s, defect = cfg["L"], cfg["C"], cfg["scale"], cfg["defect"]
        idx = torch.arange(C) % L
        nz = _noise_rows(noise, cfg["dup"], defect)
        muc = mu[:, idx]
        om = muc if nz is None else muc + nz
        Mm = s * _bmm_t(r(om), r(mu)) - 0.5 * s * (mu * mu).sum(-1).unsqueeze(-2)
        d0 = Mm[:, torch.arange(C), idx]
        nrep = 1 if defect == "nrep_missing_in_normaliser" else C // L
        lse = torch.logsumexp(Mm, -1)
        if cfg["mis"] == 0:
            lse = lse + math.log(nrep)
        return om, muc, Mm, d0, lse, idx

    @staticmethod
    def forward(ctx, pq, pk, colbias, noise, cfg, *params):
        on, defect, s, L = cfg["round16"], cfg["defect"], cfg["scale"], cfg["L"]

        def r(x):
            return rnd(x, H16) if on else x
        xq = xk = rsq = rsk = None
        if cfg["has_mlp"]:
            Wq, bq, gq, cq, Wk, bk, gk, ck = params
            xq, rsq = _ModelLmk._lin_ln(pq, Wq, bq, r)
            xk, rsk = _ModelLmk._lin_ln(pk, Wk, bk, r)
            qb, k0 = gq[:, None] * xq + cq[:, None], gk[:, None] * xk + ck[:, None]
        else:
            qb, k0 = pq, pk
        ctx.cfg, ctx.r, ctx.has_cb = cfg, r, colbias is not None
        if cfg["eva"]:
            om = 0.5 * (qb + k0)
            ctx.saved = (pq, pk, params, noise, xq, xk, rsq, rsk, k0, None, None)
            return (om if noise is None else om + noise), k0, None, None
        A = None
        kb = k0
        if cfg["mixed"]:
            k0h = r(k0)
            G = s * _bmm_t(k0h, k0h)
            if colbias is not None:
                G = G + (colbias[:, :, None] if defect == "colbias_along_rows" else colbias[:, None, :])
            if defect == "pad_columns_unmasked":              # the zero rows L..63 of the K0 tile: logit 0 on 64 - L more columns
                G = torch.cat([G, G.new_zeros(G.shape[0], L, 64 - L)], -1)
            A = torch.softmax(G, -1)[..., :L]
            kb = torch.matmul(r(A), k0h)
        mu = qb + kb
        om, muc, Mm, d0, lse, idx = _ModelLmk._densities(mu, noise, cfg, r)
        mis = cfg["mis"]
        ctx.saved = (pq, pk, params, noise, xq, xk, rsq, rsk, k0, A, mu)
        if mis == 0:
            return om, qb[:, idx], torch.exp(d0 - lse), d0
        return om, (muc if mis == 1 else None), None, lse

    @staticmethod
    def _tail(dy, xh, rstd, gam, p, W, cfg, r):
        """LayerNorm + Linear backward of one side: -> dP, dW, db, dgamma, dbeta."""
        dgam, dbet = (dy * xh).sum(1), dy.sum(1)
        dxh = dy * gam[:, None]
        s1 = dxh.mean(-1, keepdim=True)
        s2 = (dxh * xh).mean(-1, keepdim=True)
        if cfg["defect"] == "ln_xhat_term_dropped":
            s2 = torch.zeros_like(s2)
        dh = rstd * (dxh - s1 - xh * s2)
        dh16 = _pow2_pack(dh, cfg["round16"])
        return torch.matmul(dh16, r(W)), torch.matmul(dh16.transpose(-1, -2), r(p)), dh.sum(1), dgam, dbet

    @staticmethod
    def backward(ctx, g_om, g_qr, g_bhv, g_lp):
        cfg, r = ctx.cfg, ctx.r
        on, defect, s, L, C, mis = cfg["round16"], cfg["defect"], cfg["scale"], cfg["L"], cfg["C"], cfg["mis"]
        pq, pk, params, noise, xq, xk, rsq, rsk, k0, A, mu = ctx.saved
        nrep = C // L
        d_cb = None
        if cfg["eva"]:
            gin = torch.zeros_like(pq) if g_om is None else g_om
            half = 1.0 if defect == "eva_half_missing" else 0.5
            dqb = half * gin
            dk0 = half * gin if g_qr is None else half * gin + g_qr
        else:
            om, muc, Mm, d0, lse, idx = _ModelLmk._densities(mu, noise, cfg, r)
            gin = torch.zeros_like(om) if g_om is None else g_om
            g_lp = torch.zeros_like(lse) if g_lp is None else g_lp
            pm = torch.exp(Mm - lse.unsqueeze(-1))
            if mis == 0:
                dbh = torch.zeros_like(lse) if g_bhv is None else g_bhv * torch.exp(d0 - lse)
                dM = (-dbh).unsqueeze(-1) * pm * float(nrep)
                dM = dM + F.one_hot(idx, L).to(dM.dtype)[None] * (g_lp + dbh).unsqueeze(-1)
            else:
                dM = g_lp.unsqueeze(-1) * pm
            dM16 = _pow2_pack(dM, on)
            dmu = s * torch.matmul(dM16.transpose(-1, -2), r(om)) - s * dM.sum(1).unsqueeze(-1) * mu
            dom = gin + s * torch.matmul(dM16, r(mu))
            if mis == 1 and g_qr is not None:
                dom = dom + g_qr
            d = dmu + dom[:, :L]
            if defect != "fold_missing":
                for k in range(1, nrep):
                    d = d + dom[:, k * L:(k + 1) * L]
            dqb = d
            if mis == 0 and g_qr is not None:
                for k in range(1 if defect == "dqs_first_copy_only" else nrep):
                    dqb = dqb + g_qr[:, k * L:(k + 1) * L]
            dk0 = d
            if cfg["mixed"]:
                k0h = r(k0)
                dkb16 = _pow2_pack(d, on)
                dkk = torch.matmul(r(A).transpose(-1, -2), dkb16)
                dA = _bmm_t(dkb16, k0h)
                dG = A * (dA - (A * dA).sum(-1, keepdim=True))
                d_cb = dG.sum(1) if ctx.has_cb else None
                dG16 = _pow2_pack(dG, on)
                dk0 = dkk + s * (torch.matmul(dG16, k0h) + torch.matmul(dG16.transpose(-1, -2), k0h))
        if not cfg["has_mlp"]:
            return (dqb, dk0, d_cb, None, None)
        Wq, bq, gq, cq, Wk, bk, gk, ck = params
        dpq, dWq, dbq, dgq, dcq = _ModelLmk._tail(dqb, xq, rsq, gq, pq, Wq, cfg, r)
        dpk, dWk, dbk, dgk, dck = _ModelLmk._tail(dk0, xk, rsk, gk, pk, Wk, cfg, r)
        if defect == "dgamma_dbeta_swapped":
            dgq, dcq, dgk, dck = dcq, dgq, dck, dgk
        return (dpq, dpk, d_cb, None, None, dWq, dbq, dgq, dcq, dWk, dbk, dgk, dck)


# ------------------------------------------------------------------------------------------------------------------------
# one entry for both
# ------------------------------------------------------------------------------------------------------------------------
def fold_d_omega(d_omega, parts, dom_scale, defect=None):
    """ea_slice_sum's order of additions: ((a + parts[0]) + parts[1]) + ..., then the scale."""
    if parts is None:
        return d_omega
    if defect == "dom_scale_on_d_omega_only":
        acc = d_omega * dom_scale
        for s_ in range(parts.shape[1]):
            acc = acc + parts[:, s_]
        return acc
    acc = d_omega
    for s_ in range(parts.shape[1]):
        acc = acc + parts[:, s_]
    return acc * dom_scale


def lmk_grads(c, o, *, dtype, model=False, round16=False, defect=None, use=("g_omega", "g_qrows", "g_bhv", "g_lp")):
    """Forward and gradients of a case (tests/lmk_cases.py: c = geometry, o = fp32 operands).  model = False: R (plain torch +
    autograd).  model = True: _ModelLmk in `dtype` with (round16) or without the kernel's roundings; defect: one of DEFECTS.
    `use`: the incoming gradients that are given (the others are NULL for the kernel).  -> dict of OUTPUTS and GRADS that the
    geometry has."""
    BH, D = c["BH"], c["D"]
    cast = lambda t: None if t is None else t.detach().to(dtype)                                    # noqa: E731
    leaves = dict(pq=cast(o["pq"]).requires_grad_(True), pk=cast(o["pk"]).requires_grad_(True))
    if c["has_mlp"]:
        for n_ in PARAMS:
            leaves[n_] = cast(o[n_]).unsqueeze(0).expand(BH, *o[n_].shape).clone().requires_grad_(True)
    colbias = None
    if c.get("cb"):
        colbias = leaves["colbias"] = cast(o["colbias"]).requires_grad_(True)
    noise = cast(o.get("noise"))
    cfg = dict(c, mis=MIS[c["mis"]], round16=round16, defect=defect)
    if model or defect is not None:
        plist = [leaves[n_] for n_ in PARAMS] if c["has_mlp"] else []
        om, qr, bh, lp = _ModelLmk.apply(leaves["pq"], leaves["pk"], colbias, noise, cfg, *plist)
        outs = dict(omega=om, qbar_rows=qr, bhv=bh, lp=lp)
    else:
        outs = lmk_forward(leaves["pq"], leaves["pk"], leaves if c["has_mlp"] else None, noise, colbias, c)
    g_om = fold_d_omega(cast(o["g_omega"]), cast(o.get("parts")), c.get("dom_scale", 1.0), defect)
    gin = dict(omega=g_om, qbar_rows=cast(o.get("g_qrows")), bhv=cast(o.get("g_bhv")), lp=cast(o.get("g_lp")))
    given = dict(omega="g_omega" in use, qbar_rows="g_qrows" in use, bhv="g_bhv" in use, lp="g_lp" in use)
    ys = [n_ for n_ in OUTPUTS if outs[n_] is not None and gin[n_] is not None and given[n_]]
    names = list(leaves)
    gs = torch.autograd.grad([outs[n_] for n_ in ys], [leaves[n_] for n_ in names], [gin[n_] for n_ in ys], allow_unused=True)
    g = {n_: (torch.zeros_like(leaves[n_]) if x is None else x) for n_, x in zip(names, gs)}
    res = {n_: outs[n_].detach() for n_ in OUTPUTS if outs[n_] is not None}
    res["dpq"], res["dpk"] = g["pq"], g["pk"]
    if c["has_mlp"]:
        res["dW_part"] = torch.stack([g["Wq"], g["Wk"]], 1)
        res["dvec_part"] = torch.stack([torch.stack([g["bq"], g["gq"], g["cq"]], 1), torch.stack([g["bk"], g["gk"], g["ck"]], 1)], 1)
    if colbias is not None:
        res["d_colbias"] = g["colbias"]
    return res


def reference(c, o, **kw):
    """R: fp64, plain torch, autograd."""
    return lmk_grads(c, o, dtype=torch.float64, **kw)


def model(c, o, **kw):
    """M: fp32 with the kernel's fp16 roundings."""
    return lmk_grads(c, o, dtype=torch.float32, model=True, round16=True, **kw)
