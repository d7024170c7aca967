"""-m gpu: the kernelized-attention kernels of csrc/ea_kernelized.hip (statistics, kv, out, bwd_q, bwd_k for six feature maps with
and without cos weighting) called at core level -- _kernelized.kernelized_fwd_impl / kernelized_bwd_impl, the bodies of
torch.ops.ea.kernelized_fwd / _bwd -- on the test's own operands, against an fp64 evaluation of the SAME operands
(tests/kz_reference.py), one case per branch of the dispatcher and of the kernels (tests/kz_cases.py; the reference, the model, the
plan of every case and the input conditions are held on the CPU by tests/test_kz_reference_cpu.py).

Bound, per compared tensor X with the exact reference R and the model M (the kernels' arithmetic in fp32 with the one rounding of the
stored out, dq, dk, dv): a(X) = max_i |X_i - R_i| / (rms(R) + |R_i|) must satisfy a(HIP) <= 4 a(M) + f, and so must the two norm-wise
figures (max / max, rms / rms); f = 2^-9 / 2^-12 for out, dq, dk, dv stored in bf16 / fp16 and 2^-20 for every fp32 result.  The
factor and the floors are window_reference's, fixed before anything was measured; M and R are computed at test time.  `pytest -s`
prints a(HIP) / a(M) and the share of the bound used per tensor; DESIGN.md 4e carries the worst figures observed.

Compared: p_st (the maximum over the slices), kv, ksum, out, dq, dk, dv, dW; dkv and dksum through the C ABI (ea_kernelized_bwd_q +
ea_slice_sum on NaN-prefilled outputs).  No element is exempt."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kz_cases as kzc                  # noqa: E402
import kz_reference as kr               # noqa: E402

NAN = float("nan")
EA_E_BADARG = -1
FWD = ("p_st", "kv", "ksum", "out")
RUN_IDS = ["%s-%s" % r for r in kzc.RUNS]


def _cfg(c):
    from efficient_attention import _kernelized as kz
    return kz.make_cfg(c["map"], c["m"], 64, c["cos"])


def _qkv5(o, pad_to=64):
    """[B,N,3,h,64] on the device (pad_to > 64: the [..., :64] slice of a wider buffer)."""
    x = torch.stack([o["q"], o["k"], o["v"]], 0).permute(1, 3, 0, 2, 4).contiguous().cuda()
    if pad_to == 64:
        return x
    buf = torch.full(tuple(x.shape[:-1]) + (pad_to,), NAN, dtype=x.dtype, device="cuda")
    buf[..., :64] = x
    return buf[..., :64]


def _bhnd(t):
    """[B,N,h,d] -> [B,h,N,d] on the CPU."""
    return t.detach().permute(0, 2, 1, 3).contiguous().cpu()


def _p_st(c, p_st):
    """[BH,S,2] slice maxima -> [BH, sides] (an empty slice holds -inf)."""
    return p_st.detach().cpu().amax(1)[:, :kr.STAT_SIDES[c["map"]]]


def _run(c, o, pad_to=64, dout=None):
    """The forward and the backward through the impl functions -> dict of CPU tensors named as in kz_reference."""
    from efficient_attention import _kernelized as kz
    cfg = _cfg(c)
    qkv5 = _qkv5(o, pad_to)
    mask = None if o["mask"] is None else o["mask"].to(torch.uint8).cuda()
    W = None if o["W"] is None else o["W"].cuda()
    out, p_st, kv, ksum = kz.kernelized_fwd_impl(qkv5, mask, W, cfg)
    B, h, N = c["B"], c["h"], c["N"]
    assert tuple(out.shape) == (B, N, h, 64) and out.dtype == qkv5.dtype
    assert tuple(kv.shape) == (B * h, c["F"], 64) and tuple(ksum.shape) == (B * h, c["F"]) and kv.dtype == torch.float32
    assert tuple(p_st.shape) == ((B * h, c["S"], 2) if c["map"] in kr.STAT_SIDES else (0,))
    do = (o["dout"] if dout is None else dout).permute(0, 2, 1, 3).contiguous().cuda()
    dqkv5, dW = kz.kernelized_bwd_impl(do, qkv5, mask, W, p_st, kv, ksum, cfg, c["need_dw"])
    torch.cuda.synchronize()
    got = dict(out=_bhnd(out), kv=kv.cpu(), ksum=ksum.cpu(), dq=_bhnd(dqkv5[:, :, 0]), dk=_bhnd(dqkv5[:, :, 1]), dv=_bhnd(dqkv5[:, :, 2]))
    if c["map"] in kr.STAT_SIDES:
        got["p_st"] = _p_st(c, p_st)
    if c["need_dw"]:
        assert tuple(dW.shape) == tuple(o["W"].shape) and dW.dtype == torch.float32
        got["dW"] = dW.cpu()
    else:
        assert dW.numel() == 0                                                   # need_dw = False: empty
    for n_, t in got.items():
        assert bool(torch.isfinite(t).all()), "%s holds NaN or inf" % n_
    if o["mask"] is not None:                                                    # padded keys: dk = dv = 0 exactly
        dead = o["mask"][:, None, :].expand(B, h, N)
        assert bool((got["dk"][dead] == 0).all()) and bool((got["dv"][dead] == 0).all())
    return got


_GOT, _REF = {}, {}


def _got(name, dt):
    if (name, dt) not in _GOT:
        c, o = _ref(name, dt)[:2]
        _GOT[(name, dt)] = _run(c, o)
    return _GOT[(name, dt)]


def _ref(name, dt="fp32"):
    """(c, o, R, M) of a run, computed once and shared."""
    if (name, dt) not in _REF:
        c, o, _ = kzc.operands(name, dt)
        _REF[(name, dt)] = (c, o, kr.reference(c, o), kr.model(c, o))
    return _REF[(name, dt)]


def _hold_to_bound(tag, got, R, M, io, names):
    bad, lines, worst, worst_ratio = [], [], 0.0, (0.0, "")
    for n_ in names:
        ok, txt, ratio = kr.bound_report(n_, got[n_], M[n_], R[n_], io)
        used = kr.excess(n_, got[n_], M[n_], R[n_], io)
        worst = max(worst, used)
        if kr.a_err(M[n_], R[n_]) > 0 and ratio > worst_ratio[0]:
            worst_ratio = (ratio, n_)
        lines.append("%s %s  bound used %.2f" % (tag, txt, used))
        if not ok:
            bad.append(n_)
    print("\n" + "\n".join(lines) + "\n%s worst a(HIP) / a(M) %.2f (%s), worst share of the bound %.2f" % ((tag,) + worst_ratio + (worst,)))
    assert not bad, "%s: %s exceed 4 a(M) + f\n%s" % (tag, bad, "\n".join(lines))


def _names(c, R):
    return [n_ for n_ in kr.compared(R) if n_ not in ("dkv", "dksum") and (n_ != "dW" or c["need_dw"])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dt", kzc.RUNS, ids=RUN_IDS)
def test_kernels_match_fp64_same_operand_reference(name, dt):
    got = _got(name, dt)                                                 # (finite, dk = dv = 0 at padded keys, dW empty: _run)
    c, o, R, M = _ref(name, dt)
    names = _names(c, R)
    assert set(got) == set(names)
    _hold_to_bound("%s %s" % (name, dt), got, R, M, kzc.DTYPES[dt], names)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dt", kzc.RUNS, ids=RUN_IDS)
def test_two_runs_are_bit_identical(name, dt):
    c, o = _ref(name, dt)[:2]
    a, b = _got(name, dt), _run(c, o)
    for n_ in a:
        assert torch.equal(a[n_], b[n_]), (name, dt, n_)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n_ for n_ in kzc.NAMES if kzc.CASES[n_]["B"] > 1])
def test_batch_rows_are_independent(name):
    """Every batch row holds the same data and the same mask: the rows of every per-row result are bit-identical."""
    c, o, _ = kzc.operands(name, same_rows=True)
    got = _run(c, o)
    B, h = c["B"], c["h"]
    for n_, t in got.items():
        if n_ == "dW":
            continue                                                     # (summed over the rows)
        t = t.reshape(B, h, *t.shape[1:]) if n_ in ("kv", "ksum", "p_st") else t
        assert bool((t == t[:1]).all()), (name, n_)


@pytest.mark.gpu
@pytest.mark.parametrize("name", kzc.NAMES)
def test_zero_cotangent_gives_exactly_zero_gradients(name):
    """dout = 0: bwd_q's recomputed out and den enter dq only through d den = -(dout . out) / den and d num = dout / den, so every
    gradient is exactly 0 whatever the recomputation gives -- and a NaN or an inf in it would show (0 * inf)."""
    c, o = _ref(name)[:2]
    got = _run(c, o, dout=torch.zeros_like(o["dout"]))
    for n_ in ("dq", "dk", "dv") + (("dW",) if c["need_dw"] else ()):
        assert bool((got[n_] == 0).all()), (name, n_)
    ref = _got(name, "fp32")
    for n_ in FWD:
        if n_ in got:
            assert torch.equal(got[n_], ref[n_]), (name, n_)


@pytest.mark.gpu
def test_strided_views_hold_the_same_bound():
    """qkv as the [..., :64] slice of a 68-wide buffer (NaN in the four columns behind every row): the same bound against the same
    R, and the same bits as the contiguous call."""
    for name in ("favorp_m16", "fourier_m48_cos"):
        c, o, R, M = _ref(name, "fp32")
        got = _run(c, o, pad_to=68)
        _hold_to_bound(name + " strided", got, R, M, torch.float32, _names(c, R))
        base = _got(name, "fp32")
        for n_ in got:
            assert torch.equal(got[n_], base[n_]), (name, n_)


DIRECT = ("favorp_m16", "fourier_m48_cos", "relu_m112_cos", "dpfp_nu2", "sigmoid_cos", "L1_fourier_m32", "L2_relu_m48_cos", "mask_favorp_m64",
          "clamp_fourier_m32", "relu_m64_nodw")


@pytest.mark.gpu
@pytest.mark.parametrize("name", DIRECT)
def test_dkv_and_dksum_through_the_c_abi(name):
    """ea_kernelized_bwd_q + ea_slice_sum called directly on NaN-prefilled outputs: dkv, dksum (and dq) within the bound; every
    element of the partials written; bwd_q writes side 0 of the dW partials -- zeros for an empty slice -- and leaves side 1 alone."""
    from efficient_attention import _kernelized as kz
    from efficient_attention import _native as nv
    c, o, R, M = _ref(name, "fp32")
    B, h, N, S, F = c["B"], c["h"], c["N"], c["S"], c["F"]
    BH = B * h
    cfg = _cfg(c)
    qkv5 = _qkv5(o)
    mask = None if o["mask"] is None else o["mask"].to(torch.uint8).cuda()
    W = None if o["W"] is None else o["W"].cuda()
    out, p_st, kv, ksum = kz.kernelized_fwd_impl(qkv5, mask, W, cfg)
    geom = kz._geom(qkv5, cfg)
    assert kz._parts(geom) == S

    def nan(*shape):
        return torch.full(shape, NAN, dtype=torch.float32, device="cuda")
    dout = o["dout"].permute(0, 2, 1, 3).contiguous().cuda()
    dq = nan(B, N, h, 64)
    p_dkv, p_dks = nan(BH, S, F, 64), nan(BH, S, F)
    p_dw = nan(h, B, 2, S, c["m"], 64) if c["need_dw"] else None
    t4 = lambda t: ctypes.byref(nv.t4(t.permute(0, 2, 1, 3)))                 # noqa: E731
    st = nv.ptr(p_st) if p_st.numel() else None
    rc = nv.lib().ea_kernelized_bwd_q(ctypes.byref(geom), t4(qkv5[:, :, 0]), t4(dout), nv.ptr(W), st, nv.ptr(kv), nv.ptr(ksum), t4(dq),
                                      nv.ptr(p_dkv), nv.ptr(p_dks), nv.ptr(p_dw), nv.stream())
    assert rc == 0
    dkv, dksum = nan(BH, F, 64), nan(BH, F)
    nv.call("ea_slice_sum", BH, S, F * 64, 1.0, None, nv.ptr(p_dkv), nv.ptr(dkv), nv.stream())
    nv.call("ea_slice_sum", BH, S, F, 1.0, None, nv.ptr(p_dks), nv.ptr(dksum), nv.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p_dkv).all()) and bool(torch.isfinite(p_dks).all()) and bool(torch.isfinite(dq).all())
    got = dict(dkv=dkv.cpu(), dksum=dksum.cpu(), dq=_bhnd(dq))
    _hold_to_bound(name + " C ABI", got, R, M, torch.float32, ("dkv", "dksum", "dq"))
    assert torch.equal(got["dq"], _got(name, "fp32")["dq"])
    empty = [s for s in range(S) if s * c["tps"] >= N]
    assert bool((p_dkv[:, empty] == 0).all()) and bool((p_dks[:, empty] == 0).all())
    if p_dw is not None:
        assert bool(torch.isfinite(p_dw[:, :, 0]).all()) and bool(torch.isnan(p_dw[:, :, 1]).all())
        assert bool((p_dw[:, :, 0, empty] == 0).all())
    elif c["map"] not in kr.W_MAPS:                                           # dW partials for a map without W: a bad argument
        junk = nan(16)
        assert nv.lib().ea_kernelized_bwd_q(ctypes.byref(geom), t4(qkv5[:, :, 0]), t4(dout), None, st, nv.ptr(kv), nv.ptr(ksum), t4(dq),
                                            nv.ptr(p_dkv), nv.ptr(p_dks), nv.ptr(junk), nv.stream()) == EA_E_BADARG
        torch.cuda.synchronize()
        assert bool(torch.isnan(junk).all())


@pytest.mark.gpu
def test_stats_entry_refuses_a_map_without_statistics_on_real_tensors():
    from efficient_attention import _kernelized as kz
    from efficient_attention import _native as nv
    c, o = _ref("relu_m16")[:2]
    qkv5 = _qkv5(o)
    geom = kz._geom(qkv5, _cfg(c))
    p_st = torch.full((c["B"] * c["h"], c["S"], 2), NAN, dtype=torch.float32, device="cuda")
    t4 = lambda t: ctypes.byref(nv.t4(t.permute(0, 2, 1, 3)))                 # noqa: E731
    W = o["W"].cuda()
    assert nv.lib().ea_kernelized_stats(ctypes.byref(geom), t4(qkv5[:, :, 0]), t4(qkv5[:, :, 1]), nv.ptr(W), nv.ptr(p_st), nv.stream()) == EA_E_BADARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(p_st).all())


# ------------------------------------------------------------------------------------------------------------------------
# the Performer's exact-fp32 unit on the same R: it blocks the feature dimension differently (csrc/ea_performer_f32.hip)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", kzc.PERFORMER)
def test_performer_f32_kernels_hold_the_same_bound(name):
    from efficient_attention import _ops
    c, o, R, M = _ref(name, "fp32")
    assert c["map"] == "favorp" and not c["cos"] and c["m"] <= 96
    qkv5 = _qkv5(o)
    mask = None if o["mask"] is None else o["mask"].to(torch.uint8).cuda()
    W = o["W"].cuda()
    B, h, N = c["B"], c["h"], c["N"]

    def run():
        out, p_max, kv, ksum = _ops.performer_f32_fwd(qkv5, mask, W)
        assert tuple(p_max.shape) == (B * h, c["S"])
        dqkv5 = _ops.performer_f32_bwd(o["dout"].permute(0, 2, 1, 3).contiguous().cuda(), qkv5, mask, W, p_max, kv, ksum)
        torch.cuda.synchronize()
        return dict(out=_bhnd(out), kv=kv.cpu(), ksum=ksum.cpu(), p_st=p_max.cpu().amax(1, keepdim=True), dq=_bhnd(dqkv5[:, :, 0]),
                    dk=_bhnd(dqkv5[:, :, 1]), dv=_bhnd(dqkv5[:, :, 2]))
    got, again = run(), run()
    for n_, t in got.items():
        assert bool(torch.isfinite(t).all()), n_
        assert torch.equal(t, again[n_]), n_
    if o["mask"] is not None:
        dead = o["mask"][:, None, :].expand(B, h, N)
        assert bool((got["dk"][dead] == 0).all()) and bool((got["dv"][dead] == 0).all())
    _hold_to_bound(name + " performer_f32", got, R, M, torch.float32, list(got))
