"""The kernelized-attention contract restated in torch, fp64, from its formulas (kernelized_attention.py of the reference,
as the ABI comment of include/ea_hip.h states them) -- the yardstick of the full-size GPU tests, itself pinned to the
reference's fixtures by tests/test_kernelized_cpu.py.

  c = d^-1/4, c2 = d^-1/2 / 2, r = m^-1/2, l = c W x (W [h, m, d])
  favorp        r exp(l - c2|x|^2 - stab) + 1e-4       stab = max_j l (queries), max over (tokens, j) (keys); detached
  relu          relu(r l) + 1e-3
  fourier       r [sin l, cos l] exp(c2|x|^2 - max_n c2|x_n|^2)      (max over the sequence of that side; detached)
  relu-only     relu(x) + 0.1        sigmoid-only   sigmoid(x) + 0.1
  dpfp          x' = [relu(x), relu(-x)],  phi = concat_{j = 1..nu} x' * roll(x', j),  nu = (m // d) // 2
  padded keys: phi = 0;  cos weighting: [phi cos t_n, phi sin t_n], t_n = (pi/2) n / N
  out_n = phi(q_n) (sum_k phi(k)^T v) / max(phi(q_n) . sum_k phi(k), 1e-2)
"""
import math

import torch


def features(x, W, proj_method, m, is_query):
    """x [B, h, N, d] -> phi [B, h, N, F] (before the mask and the cos weighting)."""
    d = x.shape[-1]
    c, c2 = d ** -0.25, d ** -0.5 / 2
    if proj_method in ("favorp", "relu", "fourier"):
        r = W.shape[1] ** -0.5
        l = c * torch.einsum("bhnd,hjd->bhnj", x, W)
        sq = c2 * (x * x).sum(-1, keepdim=True)
        if proj_method == "favorp":
            stab = l.amax(-1, keepdim=True) if is_query else l.amax((-1, -2), keepdim=True)
            return r * torch.exp(l - sq - stab.detach()) + 1e-4
        if proj_method == "relu":
            return torch.relu(r * l) + 1e-3
        hx = torch.exp(sq - sq.amax(-2, keepdim=True).detach())
        return r * torch.cat([torch.sin(l), torch.cos(l)], -1) * hx
    if proj_method == "relu-only":
        return torch.relu(x) + 0.1
    if proj_method == "sigmoid-only":
        return torch.sigmoid(x) + 0.1
    if proj_method == "dpfp":
        nu = (m // d) // 2
        xp = torch.cat([torch.relu(x), torch.relu(-x)], -1)
        return torch.cat([xp * torch.roll(xp, j, -1) for j in range(1, nu + 1)], -1)
    raise ValueError(proj_method)


def core(q, k, v, mask, W, proj_method, m, cos_weighting, stats=None):
    """q, k, v [B, h, N, d]; mask [B, N] bool (True = padded) or None -> out [B, h, N, d].  stats: dict that receives the
    normaliser `den` [B, h, N] (before the clamp)."""
    B, h, N, d = q.shape
    pq = features(q, W, proj_method, m, True)
    pk = features(k, W, proj_method, m, False)
    if mask is not None:
        pk = pk * (~mask).to(pk.dtype)[:, None, :, None]
    if cos_weighting:
        t = (math.pi / 2) * torch.arange(N, dtype=q.dtype, device=q.device) / N
        cw, sw = torch.cos(t)[:, None], torch.sin(t)[:, None]
        pq = torch.cat([pq * cw, pq * sw], -1)
        pk = torch.cat([pk * cw, pk * sw], -1)
    kv = torch.einsum("bhnf,bhne->bhfe", pk, v)
    den = torch.einsum("bhnf,bhf->bhn", pq, pk.sum(-2))
    if stats is not None:
        stats["den"] = den.detach()
    return torch.einsum("bhnf,bhfe->bhne", pq, kv) / den.clamp(min=1e-2)[..., None]


def module_forward(x, params, heads, proj_method, m, cos_weighting, W, mask=None, stats=None):
    """The whole layer: qkv Linear -> core -> output Linear.  x [B, *seq, C]; params: qkv.weight / qkv.bias / proj.weight /
    proj.bias; W: the feature matrix the call uses (or None)."""
    B, C = x.shape[0], x.shape[-1]
    xs = x.reshape(B, -1, C)
    N, d = xs.shape[1], C // heads
    qkv = (xs @ params["qkv.weight"].t() + params["qkv.bias"]).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    out = core(qkv[0], qkv[1], qkv[2], mask, W, proj_method, m, cos_weighting, stats)
    y = out.permute(0, 2, 1, 3).reshape(B, N, C) @ params["proj.weight"].t() + params["proj.bias"]
    return y.reshape(x.shape)
