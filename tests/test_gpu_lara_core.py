"""-m gpu: the 16-bit LARA estimator passes -- the three calls of _ops.LaraAttnFn: _lara_fwd_core (ea_lara_stats_fwd, the merge,
ea_lara_out_fwd), _lara_bwd_core (ea_lara_bwd_q_fused / _k_fused or the two-pass ea_lara_bwd_q / _qstats / _k / _kstats, the merge,
ea_slice_sum) and _lara_finish (ea_lara_bwd_finish / ea_lara_bwd_qcorr) -- against an fp64 evaluation of the SAME operands
(tests/lara_reference.py), one case per host-selected variant (tests/lara_cases.py; the plans are pinned on the CPU by
tests/test_lara_reference_cpu.py).

Bound, per compared tensor X with the exact reference R and the rounding model M (the reference in fp32 with the kernels'
documented 16-bit roundings): a(X) = max_i |X_i - R_i| / (rms(R) + |R_i|) must satisfy a(HIP) <= 4 a(M) + f, and so must the two
norm-wise figures (max / max, rms / rms); f = 2^-9 (bf16) | 2^-12 (fp16) for tensors stored in 16 bits, 2^-20 for fp32 results.
The factor is fixed in advance (window_reference.FACTOR), M and R are computed at test time: no recorded constants.
`pytest -s` prints a(HIP) / a(M) per tensor; DESIGN.md 4b carries the worst ratios observed."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lara_cases as lc                 # noqa: E402
import lara_reference as lr             # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
F64 = torch.float64


def _run_lara_kernels(c, o, mis, io):
    """The operands through _ops._lara_fwd_core / _lara_bwd_core / _lara_finish, as LaraAttnFn calls them -> dict of CPU tensors
    [B,h,N,d] / [B,h,C,d] / [B,h,C]."""
    from efficient_attention import _native as nv
    from efficient_attention import _ops
    dev = "cuda"
    B, h, N, d, C = c["B"], c["h"], c["N"], c["d"], c["C"]
    BH, m = B * h, lc.MIS_CODE[mis]
    qkv = torch.stack([o["q"], o["k"], o["v"]], 0).permute(1, 3, 0, 2, 4).to(io)              # [B,N,3,h,d]
    if c["time_first"]:
        qkv5 = qkv.transpose(0, 1).contiguous().to(dev).transpose(0, 1)                        # a view of [N,B,3,h,d]
    else:
        qkv5 = qkv.contiguous().to(dev)
    geom = nv.ea_lara_geom(B, h, N, d, nv.io_dtype(qkv5), C, m, float(lc.KAPPA), float(d) ** -0.5)
    omega = o["omega"].float().reshape(BH, C, d).contiguous().to(dev)
    qbar = None if o["qbar"] is None else o["qbar"].float().reshape(BH, C, d).contiguous().to(dev)
    bhv = None if o["bhv"] is None else o["bhv"].float().reshape(BH, C).contiguous().to(dev)
    lp = o["lp"].float().reshape(BH, C).contiguous().to(dev)
    mask_u8 = None if o["mask"] is None else o["mask"].to(dev).to(torch.uint8).contiguous()
    out, (cst, kv, lse_k, lse_t, tokst) = _ops._lara_fwd_core(geom, qkv5, mask_u8, omega, qbar, bhv, lp)
    assert tuple(out.shape) == (B, N, h, d) and tuple(kv.shape) == (BH, C, d) and tuple(lse_k.shape) == (BH, C)
    dqkv5 = torch.empty_like(qkv5).fill_(float("nan"))               # every token must be written by some launch
    assert dqkv5.stride() == qkv5.stride()
    dout = o["dout"].permute(0, 2, 1, 3).to(io).contiguous().to(dev)  # [B,N,h,d]
    d_omega, d_qbar, d_bhv, d_lp, uq = _ops._lara_bwd_core(geom, qkv5, mask_u8, dout, dqkv5, omega, qbar, bhv, cst, kv, lse_k, lse_t, tokst)
    assert (uq is not None) == (mis == "opt")
    _ops._lara_finish(geom, qkv5, dqkv5, qbar, uq, lse_t)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv5.float()).all()), "dq / dk / dv hold elements no launch wrote"
    # lse_k is in the reference's natural-log units: cst = lse_k - lp is what the combine pass exponentiates
    assert float((cst - (lse_k - lp)).abs().max()) <= 1e-6 * float(1.0 + cst.abs().max())
    res = dict(out=out.permute(0, 2, 1, 3), kv=kv.view(B, h, C, d), lse_k=lse_k.view(B, h, C), dq=dqkv5[:, :, 0].permute(0, 2, 1, 3),
               dk=dqkv5[:, :, 1].permute(0, 2, 1, 3), dv=dqkv5[:, :, 2].permute(0, 2, 1, 3), d_omega=d_omega.view(B, h, C, d),
               d_lp=d_lp.view(B, h, C))
    if mis != "bh":
        res["d_qbar"] = d_qbar.view(B, h, C, d)
    if mis == "opt":
        res["d_bhv"] = d_bhv.view(B, h, C)
    return {k_: t.detach().float().cpu() for k_, t in res.items()}


def _reference(c, o, mis, dtype, round_to):
    return lr.lara_grads(o["q"], o["k"], o["v"], o["mask"], o["omega"], o["qbar"], o["bhv"], o["lp"], o["dout"], mis=mis,
                         kappa=lc.KAPPA, scale=c["d"] ** -0.5, dtype=dtype, round_to=round_to, batch_step=8)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name,mis", lc.RUNS)
def test_lara_passes_match_fp64_same_operand_reference(name, mis, dt, monkeypatch):
    io = DTYPES[dt]
    c, o = lc.operands(name, mis, io)
    monkeypatch.setenv("EA_LARA_FOLD", "1" if c["fold"] else "0")         # (read per call: _ops.lara_fold)
    got = _run_lara_kernels(c, o, mis, io)
    if o["mask"] is not None:
        pad = o["mask"][:, None, :, None].expand_as(got["dk"])
        assert bool((got["dk"][pad] == 0).all()) and bool((got["dv"][pad] == 0).all()), "dk / dv of padded keys must be exactly 0"
    R = _reference(c, o, mis, F64, None)
    M = _reference(c, o, mis, torch.float32, io)
    assert set(got) == set(R)
    tag = "%s/%s/%s" % (name, mis, dt)
    bad, lines, worst = [], [], 0.0
    for n_ in ("out", "kv", "lse_k", "dq", "dk", "dv", "d_omega", "d_lp", "d_qbar", "d_bhv"):
        if n_ not in R:
            continue
        ok, txt, ratio = lr.bound_report(n_, got[n_], M[n_], R[n_], io)
        f = lr.floor_for(n_, io)
        used = max(g_ / (lr.FACTOR * m_ + f) for g_, m_ in zip((lr.a_err(got[n_], R[n_]),) + lr.norm_errs(got[n_], R[n_]),
                                                               (lr.a_err(M[n_], R[n_]),) + lr.norm_errs(M[n_], R[n_])))
        worst = max(worst, used)
        lines.append("%s %s  bound used %.2f" % (tag, txt, used))
        if not ok:
            bad.append(n_)
    print("\n" + "\n".join(lines) + "\n%s worst share of the bound %.2f" % (tag, worst))
    assert not bad, "%s: %s exceed 4 a(M) + f\n%s" % (tag, bad, "\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_lara_passes_batch_rows_are_independent(dt):
    """Every batch row holds the same data: the rows of every result must be bit-identical."""
    io = DTYPES[dt]
    c, o = lc.operands("A1", "opt", io, same_rows=True)
    got = _run_lara_kernels(c, o, "opt", io)
    for n_, t in got.items():
        assert bool((t == t[:1]).all()), n_
