"""-m gpu: the 16-bit streaming softmax kernels (ea_softmax_attn_fwd / _bwd: sm_fwd_kernel, sm_bwd_dq_kernel, sm_bwd_dkv_kernel) and
the Gumbel-max sampler (ea_softmax_sample) of csrc/ea_softmax.hip, called through the C ABI on the test's own tensors, against an
fp64 evaluation of the SAME operands (tests/softmax_reference.py), one case per kernel variant (tests/softmax_cases.py; the tile
counts are pinned on the CPU by tests/test_softmax_reference_cpu.py and checked against this device here).

Bound, per compared tensor X with the exact reference R and the rounding model M (the reference in fp32 with the kernels'
documented 16-bit roundings): a(X) = max_i |X_i - R_i| / (rms(R) + |R_i|) must satisfy a(HIP) <= 4 a(M) + f, and so must the two
norm-wise figures (max / max, rms / rms); f = 2^-9 (bf16) | 2^-12 (fp16) for tensors stored in 16 bits, 2^-20 for fp32 results.
The factor and the floors are window_reference's, fixed before that work measured anything; M and R are computed at test time: no
recorded constants.  `pytest -s` prints a(HIP) / a(M) and the share of the bound used per tensor; DESIGN.md 4b carries the worst
figures observed."""
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

import softmax_cases as sc              # noqa: E402
import softmax_reference as sr          # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
F64 = torch.float64
NAN = float("nan")


def _rows(t, io, dev="cuda"):
    """[B,h,N,d] fp32 on the CPU -> a strided [B,h,N,d] view of a [B,N,h,d] device tensor in the I/O dtype."""
    return t.permute(0, 2, 1, 3).to(io).contiguous().to(dev).permute(0, 2, 1, 3)


def _assert_plan_on_this_device(c, name):
    from efficient_attention import _native as nv
    got = tuple(int(nv.lib().ea_softmax_tiles(w, c["B"], c["h"], c["N"], c["d"], int(c["keep"]), 0)) for w in (0, 1))
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert got == sc.PINS[name], ("case %s is written for (forward, backward) tile counts %s at %d compute units; this device has %d and "
                                  "would run %s -- another kernel variant than the case claims" % (name, sc.PINS[name], sc.CUS, cus, got))


def _run_softmax_kernels(c, o, io, forward_only=False, mask=None):
    """The operands through ea_softmax_attn_fwd / _bwd as softmax_fwd_impl / softmax_bwd_impl (fused qkv5) and SoftmaxQKVFn
    (separate views) call them; every result is prefilled with NaN.  -> dict of CPU tensors [B,h,N,d] / [B,h,N]."""
    from efficient_attention import _native as nv
    assert "EA_SM_QT" not in os.environ and "EA_SM_BQT" not in os.environ
    dev = "cuda"
    B, h, N, d = c["B"], c["h"], c["N"], c["d"]
    mask = o["mask"] if mask is None else mask
    if c["views"] == "fused":
        qkv5 = torch.stack([o["q"], o["k"], o["v"]], 0).permute(1, 3, 0, 2, 4).to(io).contiguous().to(dev)      # [B,N,3,h,d]
        q, k, v = [qkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
        dqkv5 = torch.full_like(qkv5, NAN)
        dq, dk, dv = [dqkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    else:
        q, k = _rows(o["q"], io), _rows(o["k"], io)
        v = k if c["v_is_k"] else _rows(o["v"], io)
        dq, dk, dv = [torch.full((B, N, h, d), NAN, dtype=io, device=dev).permute(0, 2, 1, 3) for _ in range(3)]
    out = torch.full((B, N, h, d), NAN, dtype=io, device=dev)
    lse, delta = [torch.full((B * h, N), NAN, dtype=torch.float32, device=dev) for _ in range(2)]
    mask_u8 = None if mask is None else mask.to(torch.uint8).contiguous().to(dev)
    keep, keep_scale = None, 1.0
    if o["keep"] is not None:
        keep_ld = (N + 63) // 64 * 64
        assert keep_ld > N
        kp = torch.ones(B, h, N, keep_ld, dtype=torch.uint8)            # (the columns past N belong to no key: any value)
        kp[..., :N] = o["keep"]
        keep, keep_scale = kp.to(dev), sc.KEEP_SCALE
    kb = int(c["kb"])
    tq, tk, tv, to = nv.t4(q), nv.t4(k), nv.t4(v), nv.t4(out.permute(0, 2, 1, 3))
    nv.call("ea_softmax_attn_fwd", B, h, N, d, nv.io_dtype(q), float(d) ** -0.5, ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv),
            nv.ptr(mask_u8), ctypes.byref(to), nv.ptr(lse), nv.ptr(keep), float(keep_scale), kb, nv.stream())
    res = dict(out=out.permute(0, 2, 1, 3), lse=lse.view(B, h, N))
    if not forward_only:
        dout = _rows(o["dout"], io)
        ts = [nv.t4(t) for t in (q, k, v, out.permute(0, 2, 1, 3), dout, dq, dk, dv)]
        nv.call("ea_softmax_attn_bwd", B, h, N, d, nv.io_dtype(q), float(d) ** -0.5, ctypes.byref(ts[0]), ctypes.byref(ts[1]),
                ctypes.byref(ts[2]), nv.ptr(mask_u8), ctypes.byref(ts[3]), ctypes.byref(ts[4]), nv.ptr(lse), nv.ptr(delta),
                ctypes.byref(ts[5]), ctypes.byref(ts[6]), ctypes.byref(ts[7]), nv.ptr(keep), float(keep_scale), kb, nv.stream())
        res.update(delta=delta.view(B, h, N), dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return {k_: t.detach().float().cpu() for k_, t in res.items()}


def _reference(c, o, dtype, round_to, **extra):
    return sr.softmax_grads(o["q"], o["k"], o["v"], o["dout"], dtype=dtype, round_to=round_to, batch_step=8,
                            **dict(sc.reference_kw(c, o), **extra))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_softmax_kernels_match_fp64_same_operand_reference(name, dt):
    io = DTYPES[dt]
    c, o = sc.operands(name, io)
    _assert_plan_on_this_device(c, name)
    got = _run_softmax_kernels(c, o, io)
    assert set(got) == set(sr.NAMES)
    for n_, t in got.items():                                        # every query and key was written by some launch
        assert bool(torch.isfinite(t).all()), "%s holds elements no launch wrote (or non-finite values)" % n_
    if o["mask"] is not None:
        pad = o["mask"][:, None, :, None].expand_as(got["dk"])
        assert bool((got["dk"][pad] == 0).all()) and bool((got["dv"][pad] == 0).all()), "dk / dv of padded keys must be exactly 0"
    R = _reference(c, o, F64, None)
    M = _reference(c, o, torch.float32, io)
    tag = "%s/%s QT %d/%d" % ((name, dt) + sc.PINS[name])
    bad, lines, worst = [], [], 0.0
    for n_ in sr.NAMES:
        ok, txt, ratio = sr.bound_report(n_, got[n_], M[n_], R[n_], io)
        f = sr.floor_for(n_, io)
        used = max(g_ / (sr.FACTOR * m_ + f) for g_, m_ in zip((sr.a_err(got[n_], R[n_]),) + sr.norm_errs(got[n_], R[n_]),
                                                               (sr.a_err(M[n_], R[n_]),) + sr.norm_errs(M[n_], R[n_])))
        worst = max(worst, used)
        lines.append("%s %s  bound used %.2f" % (tag, txt, used))
        if not ok:
            bad.append(n_)
    print("\n" + "\n".join(lines) + "\n%s worst share of the bound %.2f" % (tag, worst))
    assert not bad, "%s: %s exceed 4 a(M) + f\n%s" % (tag, bad, "\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sc.BATCH_INDEPENDENCE)
def test_softmax_kernels_batch_rows_are_independent(name, dt):
    """Every batch row holds the same data (S4: the dead-leading-chunk mask on every row): the rows of every result must be
    bit-identical."""
    io = DTYPES[dt]
    c, o = sc.operands(name, io, same_rows=True)
    _assert_plan_on_this_device(c, name)
    got = _run_softmax_kernels(c, o, io)
    for n_, t in got.items():
        assert bool(torch.isfinite(t).all()), n_
        assert bool((t == t[:1]).all()), (name, n_)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_fully_padded_batch_row_is_nan_and_leaves_the_other_row_alone(dt):
    """S1's operands, forward only, with every key of batch row 1 padded: that row's out is NaN as in the reference (a softmax
    over -inf only), and row 0 is bit-identical to the run in which row 1 is not padded.  The run compared with passes an
    all-clear mask: a NULL mask selects the other chunk body (PL: the scale folded into the shift, one rounding per score instead
    of two -- ea_softmax.hip `nfull`), so its bits may differ by design; whether they do is printed, not asserted."""
    io = DTYPES[dt]
    c, o = sc.operands("S1", io)
    B, N = c["B"], c["N"]
    clear = torch.zeros(B, N, dtype=torch.bool)
    full = clear.clone()
    full[1] = True
    got = _run_softmax_kernels(c, o, io, forward_only=True, mask=full)
    base = _run_softmax_kernels(c, o, io, forward_only=True, mask=clear)
    plain = _run_softmax_kernels(c, o, io, forward_only=True)
    R = _reference(c, o, F64, None, mask=full, forward_only=True)
    assert bool(torch.isnan(R["out"][1]).all()) and bool(torch.isfinite(R["out"][0]).all())
    assert bool(torch.isnan(got["out"][1]).all()), "out of a fully padded row must be NaN"
    assert bool(torch.isfinite(got["out"][0]).all()) and bool(torch.isfinite(got["lse"][0]).all())
    assert bool((got["out"][0] == base["out"][0]).all()) and bool((got["lse"][0] == base["lse"][0]).all())
    print("\nS1/%s row 0 against the run with a NULL mask (PL body): out identical %s, lse identical %s" % (
        dt, bool((got["out"][0] == plain["out"][0]).all()), bool((got["lse"][0] == plain["lse"][0]).all())))
    assert sr.a_err(got["out"][0], R["out"][0]) <= (0.05 if dt == "bf16" else 0.01)      # (and row 0 is the right answer)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", sc.SAMPLER_SHAPES, ids=["x".join(map(str, s)) for s in sc.SAMPLER_SHAPES])
def test_sampler_draws_are_predicted_draw_for_draw(shape, dt):
    """ea_softmax_sample with a seed tensor of the test's choosing (two seeds, one above 2^32): the kernel's counter-based hash,
    uniform and Gumbel noise restated in numpy / fp64 give score_ij = s q_i.k_j + G_ij; the drawn key's score lies within 1e-3 of
    the row maximum for >= 99.9 % of the queries and the draw is the fp64 argmax for >= 99 % (an fp32 emulation of the kernel's
    formula meets both on these inputs: tests/test_softmax_reference_cpu.py).  An index outside [0, N) fails in any case."""
    from efficient_attention import _native as nv
    io = DTYPES[dt]
    B, h, N, d = shape
    q, k = sr.sampler_operands(shape, io)
    tq, tk = _rows(q, io), _rows(k, io)
    for seed in sc.SAMPLER_SEEDS:
        seed_t = torch.tensor([seed if seed < 2 ** 63 else seed - 2 ** 64], dtype=torch.int64, device="cuda")
        index = torch.full((B * h, N), -1, dtype=torch.int64, device="cuda")
        a, b = nv.t4(tq), nv.t4(tk)
        nv.call("ea_softmax_sample", B, h, N, d, nv.io_dtype(tq), float(d) ** -0.5, ctypes.byref(a), ctypes.byref(b), nv.ptr(seed_t),
                nv.ptr(index), nv.stream())
        torch.cuda.synchronize()
        draw = index.cpu().view(B, h, N)
        assert int(draw.min()) >= 0 and int(draw.max()) < N, "a drawn index lies outside [0, N)"
        near, exact = sr.sampler_shares(sr.gumbel_scores(q, k, seed), draw)
        print("\nsampler %s %s seed %#x: within %.0e of the row maximum %.4f, fp64 argmax %.4f" % (shape, dt, seed, sr.NEAR_TOL, near, exact))
        assert near >= sr.NEAR_SHARE and exact >= sr.EXACT_SHARE, (seed, near, exact)
