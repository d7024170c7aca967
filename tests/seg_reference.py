"""Same-operand reference of LARA's 1-D landmark proposals and of the overlapping adaptive pool (plain torch, CPU; imports nothing of
the product): exactly what ea_lara_segment_fwd / _bwd, ea_lara_seglin_fwd / _bwd / _bwd_fin and ea_adaptive_pool2d_fwd / _bwd
receive, through the formulas of include/ea_hip.h and oracle/attention.py (lara_landmarks_1d, _mlp), oracle/geometry.py
(adaptive_pool_matrix).

Segments (restated from oracle.attention.lara_landmarks_1d): segs = N // L; N % L == 0: L segments of segs tokens; otherwise the
first (segs + 1) L - N segments have segs tokens and the rest segs + 1.

    segment kernel  bar_l = mean_{n in l} row_n,  row_n = LayerNorm(x_n + bias[h]) gamma + beta for an unmasked token and
                    LayerNorm(x_n + mbias) gamma + beta for a masked one; plain means (no gamma): row_n = x_n (+ bias / mbias).
                    include/ea_hip.h:556-561 words mbias as "the whole row of a masked token"; the kernel ADDS mbias to the STORED
                    row (ea_lara_segment.hip:65, `f[i] += masked ? m8[i] : b8[i]`) and relies on the module having zeroed the stored
                    rows of masked tokens.  This file models what the code does: x_n + mbias.
    seglin          bar_l = mean_{n in l} LayerNorm(G x_n + g_b) ln_w + ln_b; dq / dk = base + G^T dz; the fused finish
                    dq_n -= s sum_c t[c,n] (u qbar)_c, t[c,n] = exp(s qbar_c . q_n - lse_t[c]) with lse_t an OPERAND.
    pool            bin o of an axis of n cells = [floor(o n / side), ceil((o + 1) n / side)); forward the bin mean, backward
                    added to a prefilled buffer.
LayerNorm eps is 1e-5.  Parameters are given to R as per-(b,h) copies, so that their gradients are per-(b,h) sums: the kernels'
partials summed over the segments (segment kernel) or the groups (seglin) of a (b,h).

Two evaluations:
  R  exact reference: fp64, forward in plain torch (F.layer_norm, the averaging matrix), gradients from autograd.
  M  rounding model: the kernels' arithmetic written out forward and backward in fp32 with their roundings to the I/O dtype.
     efficient-attention_amd/csrc/ea_lara_segment.hip:
       lara_segment_kernel  no operand rounding (rows unpacked to fp32 :63, statistics fp32 :67-77); the partial planes are fp32 sums
                            (:104-106); dq / dk are WRITTEN with one rounding (pack8 at :101)
       pool2d_*             forward: fp32 sum times 1 / count (:191-192), no rounding; backward: one read-modify-write rounding per
                            element (:213)
     efficient-attention_amd/csrc/ea_lara_seglin.hip:
       G is rounded to the element type when staged (:38 forward A operand, :159 transposed operand, :362 dG pass)
       dz is rounded before G^T dz (:256-259) and before the dG product (:483); x enters the dG product exactly (0 / 1 pattern
       :364-376, :466, :484-485)
       dq / dk = rnd(old + fp32 dx) (:307-311); d ln_w, d g_b sum the unrounded values (:478-479), d ln_b = sum_l d bar_l (:442)
       fused finish: qbar and u qbar rounded to the element type in LDS (:129); t rounded before the product (:285-286); the
       correction is subtracted in fp32 (:297) before the single rounding of the store
     Not modelled (what window_reference.FACTOR is for): fp32 accumulation order, rsqrtf, fast_exp2.
     With roundings off (round_to = None, fp64) M equals the autograd of R: tests/test_seg_reference_cpu.py holds it to 1e-10.
"""
import math

import torch
import torch.nn.functional as F

from window_reference import FACTOR, a_err, bound_report, floor_for, norm_errs, rnd   # noqa: F401  (re-exported for the tests)

EPS = 1e-5
F64 = torch.float64

# single deliberate defects of the model (tests/test_seg_reference_cpu.py plays them as "the kernel")
DEFECTS = ("short_segments_last", "long_segments_div_by_segs", "last_token_dropped", "row_past_end_counted", "eps_1e6",
           "masked_rows_get_bias", "bias_of_head0", "dmbias_dbias_swapped", "dlnb_without_len", "last_segment_of_dg_group_missing",
           "lse_natural_units", "padded_rows_t1", "finish_on_dk_too", "pool_floor_upper_edge", "pool_bwd_wrong_count")
CONTROL = "mean_a_xhat_uncentred"          # mean(a xhat) with a instead of a - mean a: an identity, must NOT be rejected


# ------------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------------
def seg_sizes(N, L):
    """Segment lengths of lara_landmarks_1d (N > L)."""
    assert N > L
    segs = N // L
    if N % L == 0:
        return [segs] * L
    nshort = (segs + 1) * L - N
    return [segs] * nshort + [segs + 1] * (L - nshort)


def seg_weights(N, L, dtype, defect=None):
    """(W [L,N] how often token n is counted in segment l, den [L] what the sum is divided by)."""
    sizes = seg_sizes(N, L)
    if defect == "short_segments_last":
        sizes = sizes[::-1]
    W = torch.zeros(L, N, dtype=dtype)
    den = torch.tensor(sizes, dtype=dtype)
    pos = 0
    for l, sz in enumerate(sizes):
        W[l, pos:pos + sz] = 1
        if defect == "last_token_dropped":
            W[l, pos + sz - 1] = 0
        if defect == "row_past_end_counted":
            W[l, pos + sz - 1] = 2
        if defect == "long_segments_div_by_segs" and sz == N // L + 1:
            den[l] = N // L
        pos += sz
    assert pos == N
    return W, den


def seglin_groups(BH, L):
    """ea_lara_seglin_groups (seglin_groups, ea_lara_seglin.hip:531-536) -> (groups, segments per group)."""
    per = max((BH * 4 * L + 2047) // 2048, 1)
    groups = (L + per - 1) // per
    return groups, (L + groups - 1) // groups


def col_groups(B, h, L, cus, bwd):
    """seglin_dispatch's column-pass grouping (ea_lara_seglin.hip:545-549) -> (per, cgroups, segments per group)."""
    cap = cus * (8 if bwd else 12)
    per = max((B * h * 2 * L + cap - 1) // cap, 1)
    cg = (L + per - 1) // per
    return per, cg, (L + cg - 1) // cg


def pool_bins(n, side, defect=None):
    out = []
    for o in range(side):
        lo, hi = (o * n) // side, -((-(o + 1) * n) // side)
        if defect == "pool_floor_upper_edge":
            hi = max(((o + 1) * n) // side, lo + 1)
        out.append((lo, hi))
    return out


def pool_matrix(gh, gw, side, dtype, defect=None):
    """(P [side^2, gh gw] 0 / 1 membership, cnt [side^2] cells per bin)."""
    P = torch.zeros(side * side, gh * gw, dtype=dtype)
    by, bx = pool_bins(gh, side, defect), pool_bins(gw, side, defect)
    for oy, (y0, y1) in enumerate(by):
        for ox, (x0, x1) in enumerate(bx):
            m = torch.zeros(gh, gw, dtype=dtype)
            m[y0:y1, x0:x1] = 1
            P[oy * side + ox] = m.reshape(-1)
    return P, P.sum(1)


# ------------------------------------------------------------------------------------------------------------------------
# segment kernel (folded projection form)
# ------------------------------------------------------------------------------------------------------------------------

def segment_reference(c, o):
    """R of a G case.  -> qbar, kbar [B,h,L,D]; dq, dk [B,h,N,D]; part [B,h,2,4,D] = (d gamma, d beta, d bias over unmasked rows,
    d mbias over masked rows) of every (b,h) (plain means: gamma = 1, beta = 0 implied)."""
    B, h, N, L, D = c["B"], c["h"], c["N"], c["L"], c["D"]
    W, den = seg_weights(N, L, F64)
    S = W / den[:, None]
    mask = o["mask"]
    res, parts = {}, []
    for sd in ("q", "k"):
        x = o["x" + sd].double().requires_grad_(True)
        gam = (torch.ones(D, dtype=F64) if o["g" + sd] is None else o["g" + sd].double())
        bet = (torch.zeros(D, dtype=F64) if o["c" + sd] is None else o["c" + sd].double())
        gam, bet = [t.expand(B, h, D).clone().requires_grad_(True) for t in (gam, bet)]
        bias = torch.zeros(h, D, dtype=F64) if o["bias_" + sd] is None else o["bias_" + sd].double()
        bias = bias.unsqueeze(0).expand(B, h, D).clone().requires_grad_(True)
        mb = torch.zeros(D, dtype=F64) if o["mbias_" + sd] is None else o["mbias_" + sd].double()
        mb = mb.expand(B, h, D).clone().requires_grad_(True)
        add = bias[:, :, None].expand(B, h, N, D)
        if mask is not None:
            add = torch.where(mask[:, None, :, None], mb[:, :, None].expand(B, h, N, D), add)
        row = x + add
        if c["ln"]:
            row = F.layer_norm(row, (D,), None, None, EPS)
        y = row * gam[:, :, None] + bet[:, :, None]
        bar = torch.einsum("ln,bhnd->bhld", S, y)
        gx, gg, gb, gbi, gmb = torch.autograd.grad(bar, [x, gam, bet, bias, mb], o["d_" + sd + "bar"].double(), allow_unused=True)
        gmb = torch.zeros_like(gg) if gmb is None else gmb
        res[sd + "bar"], res["d" + sd] = bar.detach(), gx
        parts.append(torch.stack([gg, gb, gbi, gmb], 2))
    res["part"] = torch.stack(parts, 2)
    return res


def _ln_stats(z, eps):
    xc = z - z.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return xc * rstd, rstd


def segment_model(c, o, dtype=torch.float32, round_to=None, defect=None):
    """M of a G case: lara_segment_kernel's arithmetic (module docstring)."""
    B, h, N, L, D = c["B"], c["h"], c["N"], c["L"], c["D"]
    W, den = seg_weights(N, L, dtype, defect)
    eps = 1e-6 if defect == "eps_1e6" else EPS
    mask = o["mask"]
    res, parts = {}, []
    for sd in ("q", "k"):
        x = o["x" + sd].to(dtype)
        gam = torch.ones(D, dtype=dtype) if o["g" + sd] is None else o["g" + sd].to(dtype)
        bet = torch.zeros(D, dtype=dtype) if o["c" + sd] is None else o["c" + sd].to(dtype)
        bias = torch.zeros(h, D, dtype=dtype) if o["bias_" + sd] is None else o["bias_" + sd].to(dtype)
        if defect == "bias_of_head0":
            bias = bias[:1].expand(h, D)
        mb = torch.zeros(D, dtype=dtype) if o["mbias_" + sd] is None else o["mbias_" + sd].to(dtype)
        add = bias[None, :, None].expand(B, h, N, D)
        mk = torch.zeros(B, 1, N, 1, dtype=torch.bool) if mask is None else mask[:, None, :, None]
        if defect != "masked_rows_get_bias":
            add = torch.where(mk, mb.expand(B, h, N, D), add)
        f = x + add
        xh, rstd = _ln_stats(f, eps) if c["ln"] else (f, None)
        bar = torch.einsum("ln,bhnd->bhld", W, gam * xh + bet) / den[:, None]
        dy = torch.einsum("ln,bhld->bhnd", W, o["d_" + sd + "bar"].to(dtype) / den[:, None])          # dy8 of the token's segment
        if c["ln"]:
            dh = dy * gam
            s1, s2 = dh.mean(-1, keepdim=True), (dh * xh).mean(-1, keepdim=True)
            dh = rstd * (dh - s1 - xh * s2)
        else:
            dh = dy
        mkf = mk.to(dtype)
        planes = [(dy * xh).sum(2), dy.sum(2), (dh * (1 - mkf)).sum(2), (dh * mkf).sum(2)]
        if defect == "dmbias_dbias_swapped":
            planes[2], planes[3] = planes[3], planes[2]
        res[sd + "bar"], res["d" + sd] = bar, rnd(dh, round_to)
        parts.append(torch.stack(planes, 2))
    res["part"] = torch.stack(parts, 2)
    return res


# ------------------------------------------------------------------------------------------------------------------------
# seglin (+ the fused finish)
# ------------------------------------------------------------------------------------------------------------------------

def _finish_t(qbar, x, lse, s):
    """t[c,n] = exp(s qbar_c . x_n - lse[c])."""
    return torch.exp(s * torch.einsum("bhcd,bhnd->bhcn", qbar, x) - lse[..., None])


def seglin_reference(c, o):
    """R of an H / F case.  -> qbar, kbar; dq, dk (base included), dq_inc, dk_inc (without it); part [B,h,2,3,64] = (d ln_w, d ln_b,
    d g_b), dG [B,h,2,64,64] of every (b,h)."""
    B, h, N, L = c["B"], c["h"], c["N"], c["L"]
    W, den = seg_weights(N, L, F64)
    S = W / den[:, None]
    res, parts, dGs = {}, [], []
    for sd in ("q", "k"):
        x = o["x" + sd].double().requires_grad_(True)
        G, gb, lw, lb = [o[n_ + sd].double().expand(B, h, *o[n_ + sd].shape).clone().requires_grad_(True) for n_ in ("G", "gb", "lw", "lb")]
        z = torch.einsum("bhnd,bhed->bhne", x, G) + gb[:, :, None]
        y = F.layer_norm(z, (64,), None, None, EPS) * lw[:, :, None] + lb[:, :, None]
        bar = torch.einsum("ln,bhnd->bhld", S, y)
        gx, gG, ggb, glw, glb = torch.autograd.grad(bar, [x, G, gb, lw, lb], o["d_" + sd + "bar"].double())
        if sd == "q" and c.get("C"):
            xq = o["xq"].double()
            t = _finish_t(o["fin_qbar"].double(), xq, o["fin_lse"].double(), c["scale"])
            gx = gx - c["scale"] * torch.einsum("bhcn,bhcd->bhnd", t, o["fin_uq"].double())
        res[sd + "bar"], res["d" + sd + "_inc"], res["d" + sd] = bar.detach(), gx, o["base_" + sd].double() + gx
        parts.append(torch.stack([glw, glb, ggb], 2))
        dGs.append(gG)
    res["part"], res["dG"] = torch.stack(parts, 2), torch.stack(dGs, 2)
    return res


def seglin_model(c, o, dtype=torch.float32, round_to=None, defect=None):
    """M of an H / F case: seglin_col_kernel / seglin_dg_kernel's arithmetic (module docstring)."""
    B, h, N, L = c["B"], c["h"], c["N"], c["L"]
    W, den = seg_weights(N, L, dtype, defect)
    eps = 1e-6 if defect == "eps_1e6" else EPS
    r = lambda t: rnd(t, round_to)                                                   # noqa: E731
    Wg = W
    if defect == "last_segment_of_dg_group_missing":
        groups, spg = seglin_groups(B * h, L)
        Wg = W.clone()
        for g_ in range(groups):
            Wg[min(L, (g_ + 1) * spg) - 1] = 0
    res, parts, dGs = {}, [], []
    for sd in ("q", "k"):
        x = o["x" + sd].to(dtype)
        G, gb, lw, lb = r(o["G" + sd].to(dtype)), o["gb" + sd].to(dtype), o["lw" + sd].to(dtype), o["lb" + sd].to(dtype)
        xh, rstd = _ln_stats(torch.matmul(x, G.t()) + gb, eps)
        bar = lw * (torch.einsum("ln,bhnd->bhld", W, xh) / den[:, None]) + lb
        dbar = o["d_" + sd + "bar"].to(dtype)
        dyv = dbar / den[:, None]                                                    # [B,h,L,64]
        a = dyv * lw
        ac = a - a.mean(-1, keepdim=True)
        a_tok = torch.einsum("ln,bhld->bhnd", W, ac)                                 # as1 of the token's segment
        s2 = ((torch.einsum("ln,bhld->bhnd", W, a) if defect == CONTROL else a_tok) * xh).mean(-1, keepdim=True)
        dz = (a_tok - xh * s2) * rstd
        dx = torch.matmul(r(dz), G)
        if c.get("C") and (sd == "q" or defect == "finish_on_dk_too"):
            C, s = c["C"], c["scale"]
            qb, uq, lse = r(o["fin_qbar"].to(dtype)), r(o["fin_uq"].to(dtype)), o["fin_lse"].to(dtype)
            if defect == "lse_natural_units":
                lse = lse * math.log(2.0)                                            # 2^(s log2e dot - lse) = exp(s dot - lse ln 2)
            t = _finish_t(qb, x, lse, s)
            if defect == "padded_rows_t1":                                           # the slots C .. 16 NCT - 1 hold the rows that follow in memory
                pad = (32 if C <= 32 else 64) - C
                flat = torch.cat([uq.reshape(B * h * C, 64), torch.zeros(pad, 64, dtype=dtype)])
                nxt = torch.stack([flat[(i + 1) * C:(i + 1) * C + pad] for i in range(B * h)]).view(B, h, pad, 64)
                uq, t = torch.cat([uq, nxt], 2), torch.cat([t, torch.ones(B, h, pad, N, dtype=dtype)], 2)
            dx = dx - s * torch.einsum("bhcn,bhcd->bhnd", r(t), uq)
        base = o["base_" + sd].to(dtype)
        res[sd + "bar"], res["d" + sd] = bar, r(base + dx)
        res["d" + sd + "_inc"] = res["d" + sd] - base
        # the dG pass: the same statistics, its own group walk
        ag_tok = torch.einsum("ln,bhld->bhnd", Wg, ac)
        s2g = (ag_tok * xh).mean(-1, keepdim=True)
        dzg = (ag_tok - xh * s2g) * rstd
        dlw = (torch.einsum("ln,bhld->bhnd", Wg, dyv) * xh).sum(2)
        live = (Wg.sum(1) > 0).to(dtype)
        dlb = (dyv * (live if defect == "dlnb_without_len" else live * den)[:, None]).sum(2)
        parts.append(torch.stack([dlw, dlb, dzg.sum(2)], 2))
        dGs.append(torch.einsum("bhne,bhnd->bhed", r(dzg), x))
    res["part"], res["dG"] = torch.stack(parts, 2), torch.stack(dGs, 2)
    return res


# ------------------------------------------------------------------------------------------------------------------------
# adaptive pool with overlapping bins
# ------------------------------------------------------------------------------------------------------------------------

def pool_reference(c, o):
    """R of a P case: plain torch + autograd.  -> mean [B,h,side^2,D], dx (base included), dx_inc."""
    P, cnt = pool_matrix(c["gh"], c["gw"], c["side"], F64)
    x = o["x"].double().requires_grad_(True)
    mean = torch.einsum("ln,bhnd->bhld", P / cnt[:, None], x)
    gx, = torch.autograd.grad(mean, [x], o["d_mean"].double())
    return dict(mean=mean.detach(), dx=o["base"].double() + gx, dx_inc=gx)


def pool_model(c, o, dtype=torch.float32, round_to=None, defect=None):
    """M of a P case: pool2d_fwd_kernel / pool2d_bwd_kernel's arithmetic (module docstring)."""
    P, cnt = pool_matrix(c["gh"], c["gw"], c["side"], dtype, defect)
    x, base = o["x"].to(dtype), o["base"].to(dtype)
    mean = torch.einsum("ln,bhnd->bhld", P, x) * (1.0 / cnt)[:, None]
    cb = cnt[:1].expand_as(cnt) if defect == "pool_bwd_wrong_count" else cnt
    gx = torch.einsum("ln,bhld->bhnd", P, o["d_mean"].to(dtype) / cb[:, None])
    dx = rnd(base + gx, round_to)
    return dict(mean=mean, dx=dx, dx_inc=dx - base)


# ------------------------------------------------------------------------------------------------------------------------
# one entry for the three families
# ------------------------------------------------------------------------------------------------------------------------
_FAM = {"G": (segment_reference, segment_model), "H": (seglin_reference, seglin_model), "F": (seglin_reference, seglin_model),
        "P": (pool_reference, pool_model)}


def reference(c, o):
    """R: fp64, plain torch, autograd."""
    return _FAM[c["fam"]][0](c, o)


def model(c, o, round_to, defect=None):
    """M: fp32 with the kernel's roundings to `round_to`."""
    return _FAM[c["fam"]][1](c, o, torch.float32, round_to, defect)


def model_exact(c, o):
    """M's arithmetic in fp64 without roundings."""
    return _FAM[c["fam"]][1](c, o, F64, None, None)
