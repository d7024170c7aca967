"""Same-operand reference of the kernelized-attention core (csrc/ea_kernelized.hip; plain torch, CPU): what the 50 kernels of the
family compute on given operands q, k, v, dout [B,h,N,64] (the I/O dtype), W [h,m,64] fp32 (the maps that have one) and a key
padding mask [B,N].  A case is a dict of tests/kz_cases.py (map, m, cos, B, h, N, S, tps, need_dw).

Two evaluations:
  R  reference(c, o): fp64.  out, den and dq, dk, dv, dW are kz_contract.core and its autograd (imported -- the contract that
     tests/test_kernelized_cpu.py pins to the reference project's fixtures); kv, ksum are kz_contract.features with the contract's
     mask and cos-weighting lines, and dkv, dksum the gradients of <out, dout> with respect to them (the restated tail is asserted
     equal to core's out); p_st follows include/ea_hip.h: favorp side 0 = max over (all tokens, j) of the key logits, fourier
     sides 0 / 1 = max of c2 |k|^2 / c2 |q|^2, padded keys included, nothing beyond N.
  M  model(c, o): the same operation in fp32 the way the kernels arrange it, gradients by autograd.  What differs from a plain
     fp32 run of the contract, by line of csrc/ea_kernelized.hip (f32tile: csrc/ea_f32_tile.h):
       * out, dq, dk, dv are rounded ONCE to the I/O dtype when stored (store_tile, ea_f32_tile.h:67-83; called at :451, :533,
         :589, :593); everything else the kernels write is fp32
       * the cos-weighting angle is th = (fp32(pi/2) * tok) * (1 / N) evaluated in fp32 (rows_prologue :139)
       * bwd_q forms out and den again from kv, ksum (pass A, :477-487) and does not read the stored out: the gradients see the
         UNROUNDED out (here: autograd on the unrounded graph)
       * the clamp: d den = 0 where den < 1e-2, -(dout . out) / den elsewhere (:491-496) -- torch's clamp(min=) has this gradient
       * favorp subtracts rs = c2 |x|^2 + stab in one step (:136, :111); fourier scales by rs = r exp(c2 |x|^2 - max) (:137, :116);
         r = rsqrtf(m) (:348)
       * the logits are c * (W . x) with c applied to the finished dot product (:91); dW is accumulated per 64-token tile and per
         side into slice partials (dw_accumulate :276-288): the model keeps one copy of W per tile and side, so a partial exists
         as a tensor (and the defects below can drop one)
       * fast_exp=True models __expf of favorp (:111), sigmoid-only (:119, :190) and fourier's envelope (:137) as
         exp2(fp32(x * log2 e)); OFF unless a GPU run shows that it matters (DESIGN 4e records whether it did)
     With dtype = float64 and rounding off, M is R to 1e-10 (tests/test_kz_reference_cpu.py).

DEFECTS: single deliberate errors of M ("the kernel" of the sensitivity tests), each a way a block index, a slice or a
statistic can go wrong in ea_kernelized.hip.  The bound (window_reference.bound_report) must reject every one of them."""
import math

import torch

import kz_contract as kc
from window_reference import FACTOR, a_err, bound_report, floor_for, norm_errs, rnd   # noqa: F401  (re-exported for the tests)

W_MAPS = ("favorp", "relu", "fourier")
STAT_SIDES = {"favorp": 1, "fourier": 2}
TB = 64
LOG2E = 1.4426950408889634
IO_NAMES = ("out", "dq", "dk", "dv")          # stored in the I/O dtype; every other result is fp32

DEFECTS = (
    "second_16_columns_dropped",      # 1  the features of columns 16..31 of every 32-column span are zero
    "fourier_cos_reads_sin",          # 2  fourier's cos half evaluated with the sin branch
    "cos_angle_tile_local",           # 3  the cos weight's angle from the row within the tile, not from the token
    "kv_slice_missing",               # 4  slice 1's partial of kv never added
    "dw_second_tile_overwrites",      # 5  a slice's later tile writes its dW partial and does not add to it
    "padded_keys_in_ksum",            # 6  padded keys counted in ksum
    "padded_keys_off_stabiliser",     # 7  favorp's key stabiliser taken over the unpadded keys only
    "zero_rows_in_key_max",           # 8  the zero rows of a ragged tile enter favorp's key maximum
    "dden_not_clamped",               # 9  d den not zeroed where den < 1e-2
    "dpfp_roll_negated",              # 10 dpfp rolled by -j
)


def base_features(c):
    return {"favorp": c["m"], "relu": c["m"], "fourier": 2 * c["m"], "relu-only": 64, "sigmoid-only": 64}.get(c["map"]) or 128 * ((c["m"] // 64) // 2)


def _weights(N, dtype, model, tile_local=False):
    """cos / sin of t_n = (pi/2) n / N, [N, 1] each."""
    tok = torch.arange(N)
    if tile_local:
        tok = tok % TB
    if model and dtype == torch.float32:
        th = (torch.tensor(1.5707963267948966, dtype=torch.float32) * tok.float()) * (torch.tensor(1.0, dtype=torch.float32) / float(N))
    else:
        th = (math.pi / 2) * tok.to(dtype) / N
    return torch.cos(th)[:, None], torch.sin(th)[:, None]


def _mask_and_weight(phi, mask, cos, N, dtype):
    """The contract's padded-key and cos-weighting lines (kz_contract.core)."""
    if mask is not None:
        phi = phi * (~mask).to(phi.dtype)[:, None, :, None]
    if cos:
        cw, sw = _weights(N, dtype, False)
        phi = torch.cat([phi * cw, phi * sw], -1)
    return phi


def reference(c, o):
    """R: dict of fp64 tensors out, den, kv, ksum, dq, dk, dv, dkv, dksum (+ dW for the W maps, p_st [BH, sides] for the maps
    with statistics)."""
    F64 = torch.float64
    B, h, N = c["B"], c["h"], c["N"]
    q, k, v = [o[n_].detach().clone().to(F64).requires_grad_(True) for n_ in ("q", "k", "v")]
    dout = o["dout"].to(F64)
    has_w = c["map"] in W_MAPS
    W = o["W"].to(F64).requires_grad_(True) if has_w else None
    mask = o["mask"]
    stats = {}
    out = kc.core(q, k, v, mask, W, c["map"], c["m"], c["cos"], stats)
    grads = torch.autograd.grad(out, [q, k, v] + ([W] if has_w else []), dout)
    res = dict(out=out.detach(), den=stats["den"], dq=grads[0], dk=grads[1], dv=grads[2])
    if has_w:
        res["dW"] = grads[3]
    with torch.no_grad():
        Wd = None if W is None else W.detach()
        pq = _mask_and_weight(kc.features(q.detach(), Wd, c["map"], c["m"], True), None, c["cos"], N, F64)
        pk = _mask_and_weight(kc.features(k.detach(), Wd, c["map"], c["m"], False), mask, c["cos"], N, F64)
        kv = torch.einsum("bhnf,bhne->bhfe", pk, v.detach())
        ksum = pk.sum(-2)
    kv_l, ks_l = kv.clone().requires_grad_(True), ksum.clone().requires_grad_(True)
    den = torch.einsum("bhnf,bhf->bhn", pq, ks_l)
    out2 = torch.einsum("bhnf,bhfe->bhne", pq, kv_l) / den.clamp(min=1e-2)[..., None]
    assert float((out2 - out).detach().abs().max()) <= 1e-12 * max(float(out.detach().abs().max()), 1e-300), "the restated tail is not kz_contract.core"
    dkv, dksum = torch.autograd.grad(out2, [kv_l, ks_l], dout)
    F = kv.shape[-2]
    res.update(kv=kv.reshape(B * h, F, 64), ksum=ksum.reshape(B * h, F), dkv=dkv.reshape(B * h, F, 64), dksum=dksum.reshape(B * h, F))
    with torch.no_grad():
        if c["map"] == "favorp":
            l = 64 ** -0.25 * torch.einsum("bhnd,hjd->bhnj", k.detach(), Wd)
            res["p_st"] = l.amax((-1, -2)).reshape(B * h, 1)
        elif c["map"] == "fourier":
            c2 = 64 ** -0.5 / 2
            res["p_st"] = torch.stack([c2 * (k.detach() ** 2).sum(-1).amax(-1), c2 * (q.detach() ** 2).sum(-1).amax(-1)], -1).reshape(B * h, 2)
    return res


def _exp(x, fast):
    if fast and x.dtype == torch.float32:
        return torch.exp2(x * LOG2E)
    return torch.exp(x)


def logits(x, Wt, dtype):
    """c (W . x) with one copy of W per 64-token tile: x [B,h,N,64], Wt [T,h,m,64] -> [B,h,N,m]."""
    B, h, N, d = x.shape
    T = Wt.shape[0]
    xp = torch.cat([x, x.new_zeros(B, h, T * TB - N, d)], 2).view(B, h, T, TB, d)
    return (torch.einsum("bhtnd,thjd->bhtnj", xp, Wt) * torch.tensor(64 ** -0.25, dtype=dtype)).reshape(B, h, T * TB, -1)[:, :, :N]


def _model_features(x, Wt, c, is_query, mask, dtype, defect, fast_exp, aux):
    """phi before the mask and the cos weighting, the kernels' arrangement (module docstring)."""
    mp, m = c["map"], c["m"]
    c2 = torch.tensor(64 ** -0.5 / 2, dtype=dtype)
    if mp in W_MAPS:
        r = torch.tensor(float(m), dtype=dtype).rsqrt()
        l = logits(x, Wt, dtype)
        aux["lq" if is_query else "lk"] = l.detach()
        sq = (x * x).sum(-1, keepdim=True) * c2
        if mp == "favorp":
            if is_query:
                stab = l.amax(-1, keepdim=True)
            else:
                lk = l
                if defect == "padded_keys_off_stabiliser" and mask is not None:
                    lk = l.masked_fill(mask[:, None, :, None], -float("inf"))
                stab = lk.amax((-1, -2), keepdim=True)
                stab = torch.where(torch.isinf(stab), torch.zeros_like(stab), stab)      # (a fully padded row)
                if defect == "zero_rows_in_key_max" and x.shape[2] % TB:
                    stab = stab.clamp(min=0.0)
                aux["p_st"] = stab.detach().reshape(-1, 1)
            return r * _exp(l - (sq + stab.detach()), fast_exp) + 1e-4
        if mp == "relu":
            return torch.relu(r * l) + 1e-3
        mx = sq.amax(-2, keepdim=True).detach()
        aux["st_q" if is_query else "st_k"] = mx.reshape(-1)
        rs = r * _exp(sq - mx, fast_exp)
        second = torch.sin(l) if defect == "fourier_cos_reads_sin" else torch.cos(l)
        return rs * torch.cat([torch.sin(l), second], -1)
    if mp == "relu-only":
        return torch.relu(x) + 0.1
    if mp == "sigmoid-only":
        return 1.0 / (1.0 + _exp(-x, fast_exp)) + 0.1
    nu = (m // 64) // 2
    xp = torch.cat([torch.relu(x), torch.relu(-x)], -1)
    sign = -1 if defect == "dpfp_roll_negated" else 1
    return torch.cat([xp * torch.roll(xp, sign * j, -1) for j in range(1, nu + 1)], -1)


def model(c, o, io=None, dtype=torch.float32, rounding=True, defect=None, fast_exp=False, reorder=None):
    """M (or, with `defect`, M with that one error): the tensors of reference() in `dtype`, out / dq / dk / dv rounded to the I/O
    dtype `io` (default: the operands' own) when `rounding`.  reorder (a seed, W maps): the same model with the 64 channels of q, k
    and W permuted alike -- the same function, another order of additions in every logit and in dq, dk, dW: a second, equally
    legitimate fp32 evaluation (tests/test_kz_reference_cpu.py holds the two to each other)."""
    assert defect is None or defect in DEFECTS
    if reorder is not None:
        perm = torch.randperm(64, generator=torch.Generator().manual_seed(reorder))
        o2 = dict(o, q=o["q"][..., perm].contiguous(), k=o["k"][..., perm].contiguous(), W=o["W"][..., perm].contiguous())
        res = model(c, o2, io, dtype, rounding, defect, fast_exp)
        inv = torch.argsort(perm)
        for n_ in ("dq", "dk", "dW"):
            res[n_] = res[n_][..., inv]
        return res
    B, h, N = c["B"], c["h"], c["N"]
    io = o["q"].dtype if io is None else io
    round_to = io if (rounding and io != torch.float32) else None
    q, k, v = [o[n_].detach().clone().to(dtype).requires_grad_(True) for n_ in ("q", "k", "v")]
    dout = o["dout"].to(dtype)
    mask = o["mask"]
    has_w = c["map"] in W_MAPS
    T = -(-N // TB)
    Wq = Wk = None
    if has_w:
        Wq = o["W"].to(dtype).unsqueeze(0).repeat(T, 1, 1, 1).requires_grad_(True)
        Wk = o["W"].to(dtype).unsqueeze(0).repeat(T, 1, 1, 1).requires_grad_(True)
    aux = {}
    pq = _model_features(q, Wq, c, True, mask, dtype, defect, fast_exp, aux)
    pk = _model_features(k, Wk, c, False, mask, dtype, defect, fast_exp, aux)
    pk_all = pk
    if mask is not None:
        pk = torch.where(mask[:, None, :, None], torch.zeros((), dtype=dtype), pk)      # (dead keys: selected, not multiplied, :159)
    if c["cos"]:
        cw, sw = _weights(N, dtype, True, tile_local=(defect == "cos_angle_tile_local"))
        pq, pk, pk_all = [torch.cat([p * cw, p * sw], -1) for p in (pq, pk, pk_all)]
    if defect == "second_16_columns_dropped":
        keep = ((torch.arange(pq.shape[-1]) % 32) < 16).to(dtype)
        pq, pk = pq * keep, pk * keep
    pk_kv = pk
    if defect == "kv_slice_missing":
        pk_kv = pk * ((torch.arange(N) // c["tps"]) != 1).to(dtype)[:, None]
    kv = torch.einsum("bhnf,bhne->bhfe", pk_kv, v)
    ksum = (pk_all if defect == "padded_keys_in_ksum" else pk).sum(-2)
    den = torch.einsum("bhnf,bhf->bhn", pq, ksum)
    denc = den.clamp(min=1e-2)
    if defect == "dden_not_clamped":
        denc = den + (denc - den).detach()
    out = torch.einsum("bhnf,bhfe->bhne", pq, kv) / denc[..., None]
    leaves = [q, k, v, kv, ksum] + ([Wq, Wk] if has_w else [])
    g = torch.autograd.grad(out, leaves, dout)
    F = kv.shape[-2]
    res = dict(out=rnd(out.detach(), round_to), den=den.detach(), dq=rnd(g[0], round_to), dk=rnd(g[1], round_to), dv=rnd(g[2], round_to),
               kv=kv.detach().reshape(B * h, F, 64), ksum=ksum.detach().reshape(B * h, F), dkv=g[3].reshape(B * h, F, 64),
               dksum=g[4].reshape(B * h, F))
    if has_w:
        tiles = g[5] + g[6]                                   # [T, h, m, 64]: both sides of every tile, summed over b
        if defect == "dw_second_tile_overwrites":
            tpt = c["tps"] // TB
            last = torch.tensor([(t + 1) % tpt == 0 or t == T - 1 for t in range(T)])
            tiles = tiles * last.to(dtype)[:, None, None, None]
        res["dW"] = tiles.sum(0)
    if c["map"] == "favorp":
        res["p_st"] = aux["p_st"]
    elif c["map"] == "fourier":
        res["p_st"] = torch.stack([aux["st_k"], aux["st_q"]], -1)
    res["_lq"], res["_lk"] = aux.get("lq"), aux.get("lk")     # the logits, for the input conditions (not compared)
    return res


def compared(R):
    """Names the kernels write (den is R's and M's alone: no kernel stores it)."""
    return [n_ for n_ in R if n_ != "den" and not n_.startswith("_")]


def excess(name, X, M, R, io):
    """The largest of the three figures of X over its bound FACTOR * figure(M) + f (> 1: the bound rejects X)."""
    f = floor_for(name, io)
    got = (a_err(X, R),) + norm_errs(X, R)
    mod = (a_err(M, R),) + norm_errs(M, R)
    return max(g_ / (FACTOR * m_ + f) for g_, m_ in zip(got, mod))
