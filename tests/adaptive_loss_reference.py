"""Host reference of the adaptive-softmax training loss (ea_harness.adaptive_loss.adaptive_nll, csrc/ea_adaptive_nll.hip): numpy,
fp64, on the CPU.

  forward(x, head, projs, tabs, cutoff, targets, round_h=None, masks=None) -> dict
      x [M, C], head [c0 + n, C], projs[i] [d_i, C] (K-contiguous: h = x projs[i]^T), tabs[i] [V_i, d_i], cutoff [c0, .., V],
      targets [M].  head_target [M] (t, c0 + i, or -1), rows[i] (the ascending rows of tail i), a = x head^T and lse_h [M],
      per tail h[i] = round_h(x[rows_i] projs[i]^T) (times masks[i][:count_i], rounded again, where a mask is given),
      b[i] = h[i] tabs[i]^T, lse[i], and logp [M] (NaN for a target outside [0, V)).
  band_grads(f, cutoff, targets, d) -> (G_h [M, c0 + n], [G_i [count_i, V_i]])
      the logit gradients, each through vocab_loss_reference.grad:  G_h = d ((v == ht) - exp(a - lse_h)),
      G_i[j, u] = d[rows_i[j]] ((u == t - c_i) - exp(b_i[j, u] - lse_i[j])).
  band_bounds(f, cutoff, targets, d, dtype) -> the same shapes, through vocab_loss_reference.bound.
  grads(x, head, projs, tabs, cutoff, targets, d, round_h=None, masks=None) -> dict(dx, dhead, dproj=[..], dtab=[..])
      dX = G_h H + scatter_i(dh_i Q_i),  dH = G_h^T X,  dE_i = G_i^T h_i,  dh_i = (G_i E_i) * mask,  dQ_i = dh_i^T x[rows_i];
      the rounding of h_i passes the gradient straight through."""
import numpy as np

import vocab_loss_reference as vref


def _lse(a):
    m = a.max(1, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(1, keepdims=True))).reshape(-1)


def forward(x, head, projs, tabs, cutoff, targets, round_h=None, masks=None):
    x, head = np.asarray(x, np.float64), np.asarray(head, np.float64)
    t = np.asarray(targets, np.int64)
    c0, n, V = cutoff[0], len(cutoff) - 1, cutoff[-1]
    ht = np.where((t >= 0) & (t < c0), t, -1)
    rows = []
    for i in range(n):
        at = np.nonzero((t >= cutoff[i]) & (t < cutoff[i + 1]))[0]
        ht[at] = c0 + i
        rows.append(at)
    a = x @ head.T
    lse_h = _lse(a)
    logp = np.full(len(t), np.nan)
    ok = ht >= 0
    logp[ok] = a[ok, ht[ok]] - lse_h[ok]
    f = dict(head_target=ht, rows=rows, a=a, lse_h=lse_h, h=[], b=[], lse=[], logp=logp, V=V)
    for i in range(n):
        h = x[rows[i]] @ np.asarray(projs[i], np.float64).T
        if round_h is not None:
            h = round_h(h)
        if masks is not None and masks[i] is not None:
            h = h * np.asarray(masks[i], np.float64)[:len(rows[i])]
            if round_h is not None:
                h = round_h(h)
        b = h @ np.asarray(tabs[i], np.float64).T
        lse = _lse(b) if len(rows[i]) else np.zeros(0)
        logp[rows[i]] += b[np.arange(len(rows[i])), t[rows[i]] - cutoff[i]] - lse
        f["h"].append(h)
        f["b"].append(b)
        f["lse"].append(lse)
    return f


def _band(fn, f, cutoff, targets, d, *extra):
    t, d = np.asarray(targets, np.int64), np.asarray(d, np.float64)
    head = fn(f["a"], f["lse_h"], d, f["head_target"], *extra, V=f["a"].shape[1])
    tails = [fn(f["b"][i], f["lse"][i], d[r], t[r] - cutoff[i], *extra, V=cutoff[i + 1] - cutoff[i])
             for i, r in enumerate(f["rows"])]
    return head, tails


def band_grads(f, cutoff, targets, d):
    return _band(vref.grad, f, cutoff, targets, d)


def band_bounds(f, cutoff, targets, d, dtype):
    return _band(vref.bound, f, cutoff, targets, d, dtype)


def grads(x, head, projs, tabs, cutoff, targets, d, round_h=None, masks=None):
    x, head = np.asarray(x, np.float64), np.asarray(head, np.float64)
    f = forward(x, head, projs, tabs, cutoff, targets, round_h, masks)
    gh, gtails = band_grads(f, cutoff, targets, d)
    out = dict(dx=gh @ head, dhead=gh.T @ x, dproj=[], dtab=[], forward=f)
    for i, g in enumerate(gtails):
        r = f["rows"][i]
        dh = g @ np.asarray(tabs[i], np.float64)
        if masks is not None and masks[i] is not None:
            dh = dh * np.asarray(masks[i], np.float64)[:len(r)]
        out["dtab"].append(g.T @ f["h"][i])
        out["dproj"].append(dh.T @ x[r])
        out["dx"][r] += dh @ np.asarray(projs[i], np.float64)
    return out
