"""-m gpu: LARA's 1-D landmark proposals and the overlapping adaptive pool at core level -- lara_segment_kernel<E, D, BWD>,
pool2d_fwd_kernel / pool2d_bwd_kernel (csrc/ea_lara_segment.hip) and seglin_col_kernel<E, BWD, NCT>, seglin_dg_kernel<E>
(csrc/ea_lara_seglin.hip) -- called through the C ABI (ea_lara_segment_fwd / _bwd, ea_lara_seglin_fwd / _bwd / _bwd_fin,
ea_adaptive_pool2d_fwd / _bwd) on the test's own tensors in the modules' layouts, against an fp64 evaluation of the SAME operands
(tests/seg_reference.py), one case per branch of the kernels (tests/seg_cases.py; the reference, the model and the input conditions
are held on the CPU by tests/test_seg_reference_cpu.py).

Bound, per compared tensor X with the exact reference R and the rounding model M (the kernel's arithmetic in fp32 with its
roundings to the I/O dtype): a(X) = max_i |X_i - R_i| / (rms(R) + |R_i|) must satisfy a(HIP) <= 4 a(M) + f, and so must the two
norm-wise figures (max / max, rms / rms); f = 2^-9 (bf16) / 2^-12 (fp16) for the 16-bit buffers dq, dk, dx and 2^-20 for fp32
results.  The factor and the floors are window_reference's, fixed before anything was measured; M and R are computed at test time:
no recorded constants.  Partials are compared after an fp64 host sum over the segments / groups of every (b,h).  `pytest -s` prints
a(HIP) / a(M) and the share of the bound used per tensor; DESIGN.md carries the worst figures observed.

Every fp32 output is prefilled with NaN and followed by a 64-float NaN guard; `stats` is a workspace (only its guard is looked at).
The slots of the 16-bit buffers no kernel may touch are compared with their prefill bit for bit in every run."""
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

import seg_cases as sc                  # noqa: E402
import seg_reference as sr              # noqa: E402

NAN = float("nan")
GUARD = 64
DT = ("bf16", "fp16")
EA_CODE = {"bf16": 0, "fp16": 1}


class _Out:
    """A NaN-prefilled fp32 output with a NaN guard of 64 floats behind it."""

    def __init__(self, *shape):
        n = 1
        for s_ in shape:
            n *= s_
        self.n = n
        self.flat = torch.full((n + GUARD,), NAN, dtype=torch.float32, device="cuda")
        self.bits = self.flat[n:].view(torch.int32).clone()
        self.t = self.flat[:n].view(*shape)

    def guard_ok(self, name):
        assert bool((self.flat[self.n:].view(torch.int32) == self.bits).all()), "%s: the guard behind it was written" % name

    def check(self, name):
        assert bool(torch.isfinite(self.t).all()), "%s holds elements no launch wrote (or non-finite values)" % name
        self.guard_ok(name)


def _f(t, mul=None):
    if t is None:
        return None
    return (t.float() if mul is None else t.float() * mul).contiguous().cuda()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _buffer(slots, nslots, c, td, seed, time_first, nan_slots=()):
    """[B,N,nslots,h,D] device buffer of dtype td: `slots` {index: [B,h,N,D] fp32 rows}, the others seeded filler; time_first: the
    same values stored [N,B,...] and handed out as a permuted view."""
    B, h, N, D = c["B"], c["h"], c["N"], c["D"]
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B, N, nslots, h, D, generator=g).to(td)
    for i, rows in slots.items():
        buf[:, :, i] = rows.permute(0, 2, 1, 3).to(td)
    for i in nan_slots:
        buf[:, :, i] = NAN
    if time_first:
        return buf.permute(1, 0, 2, 3, 4).contiguous().cuda().permute(1, 0, 2, 3, 4)
    return buf.cuda()


def _view(buf, slot):
    return buf[:, :, slot].permute(0, 2, 1, 3)                                       # [B,h,N,D], D contiguous


def _rows(buf, slot):
    return _view(buf, slot).float().cpu().contiguous()


class _Run:
    """Device tensors of one case and its launches.  gmul: factor on the incoming gradients (a power of two or 0)."""

    def __init__(self, name, dt, gmul=None, same_b=False, time_first=False, zero_uq=False, entry=None):
        from efficient_attention import _native as nv
        self.nv, self.name, self.dt, self.td = nv, name, dt, sc.DTYPES[dt]
        self.c, self.o = c, o = sc.operands(name, dt, same_b=same_b)
        B, h, N, D = c["B"], c["h"], c["N"], c["D"]
        fam = self.fam = c["fam"]
        self.entry = entry or ("bwd_fin" if fam == "F" else "bwd")
        self.out = {}
        td, s0 = self.td, sc.seed(name)
        if fam == "P":
            L = c["side"] ** 2
            self.src = _buffer({0: o["x"]}, 3, c, td, s0, time_first)
            self.grad = _buffer({0: o["base"]}, 3, c, td, s0 + 1, time_first)
            self.d_mean = _f(o["d_mean"], gmul)
            self.out["mean"] = _Out(B, h, L, D)
            self.keep = (1, 2)
        else:
            L = c["L"]
            self.geom = nv.make_geom(B, h, N, D, EA_CODE[dt], False, (N,), 0, 0, 0, L)
            self.d_qbar, self.d_kbar = _f(o["d_qbar"], gmul), _f(o["d_kbar"], gmul)
            self.out.update(qbar=_Out(B, h, L, D), kbar=_Out(B, h, L, D))
        if fam == "G":
            self.src = _buffer({3: o["xq"], 4: o["xk"]}, 5, c, td, s0, time_first)
            self.grad = _buffer({}, 5, c, td, s0 + 1, time_first, nan_slots=(3, 4))      # written, not accumulated: NaN must go
            self.mask = None if o["mask"] is None else o["mask"].to(torch.uint8).contiguous().cuda()
            self.ps = [_f(o[n_]) for n_ in ("bias_q", "bias_k", "mbias_q", "mbias_k", "gq", "cq", "gk", "ck")]
            if c["part"]:
                self.out["part"] = _Out(B, h, L, 2, 4, D)
            self.keep = (0, 1, 2)
        if fam in ("H", "F"):
            self.src = _buffer({0: o["xq"], 1: o["xk"]}, 3, c, td, s0, time_first)
            self.grad = _buffer({0: o["base_q"], 1: o["base_k"]}, 3, c, td, s0 + 1, time_first)
            self.ps = [_f(o[n_]) for n_ in ("Gq", "gbq", "Gk", "gbk", "lwq", "lbq", "lwk", "lbk")]
            self.groups = int(nv.lib().ea_lara_seglin_groups(ctypes.byref(self.geom)))
            assert self.groups == sr.seglin_groups(B * h, L)[0]
            self.out.update(part=_Out(B * h * self.groups, 2, 4, 64), dG_part=_Out(B * h * self.groups, 2, 64, 64))
            self.stats = _Out(B * h * 2 * N * 4)
            assert self.stats.flat.data_ptr() % 16 == 0
            if fam == "F":
                self.fin = [_f(o["fin_qbar"]), _f(o["fin_uq"], 0.0 if zero_uq else None), _f(o["fin_lse"])]
            self.keep = (2,)
        self.prefill = self.grad.clone()

    def forward(self):
        nv, p, c = self.nv, self.nv.ptr, self.c
        if self.fam == "P":
            t = nv.t4(_view(self.src, 0))
            return nv.lib().ea_adaptive_pool2d_fwd(EA_CODE[self.dt], c["B"], c["h"], c["gh"], c["gw"], c["side"], c["D"], ctypes.byref(t),
                                                   p(self.out["mean"].t), nv.stream())
        if self.fam == "G":
            tq, tk = nv.t4(_view(self.src, 3)), nv.t4(_view(self.src, 4))
            return nv.lib().ea_lara_segment_fwd(ctypes.byref(self.geom), ctypes.byref(tq), ctypes.byref(tk), p(self.mask), *[p(t) for t in self.ps],
                                                p(self.out["qbar"].t), p(self.out["kbar"].t), nv.stream())
        tq, tk = nv.t4(_view(self.src, 0)), nv.t4(_view(self.src, 1))
        return nv.lib().ea_lara_seglin_fwd(ctypes.byref(self.geom), ctypes.byref(tq), ctypes.byref(tk), *[p(t) for t in self.ps],
                                           p(self.out["qbar"].t), p(self.out["kbar"].t), nv.stream())

    def backward(self):
        nv, p, c = self.nv, self.nv.ptr, self.c
        if self.fam == "P":
            t = nv.t4(_view(self.grad, 0))
            return nv.lib().ea_adaptive_pool2d_bwd(EA_CODE[self.dt], c["B"], c["h"], c["gh"], c["gw"], c["side"], c["D"], p(self.d_mean),
                                                   ctypes.byref(t), nv.stream())
        if self.fam == "G":
            ts = [nv.t4(_view(self.src, 3)), nv.t4(_view(self.src, 4)), nv.t4(_view(self.grad, 3)), nv.t4(_view(self.grad, 4))]
            part = p(self.out["part"].t) if "part" in self.out else None
            return nv.lib().ea_lara_segment_bwd(ctypes.byref(self.geom), ctypes.byref(ts[0]), ctypes.byref(ts[1]), p(self.mask),
                                                *[p(t) for t in self.ps], p(self.d_qbar), p(self.d_kbar), ctypes.byref(ts[2]),
                                                ctypes.byref(ts[3]), part, nv.stream())
        ts = [nv.t4(_view(self.src, 0)), nv.t4(_view(self.src, 1)), nv.t4(_view(self.grad, 0)), nv.t4(_view(self.grad, 1))]
        common = [ctypes.byref(self.geom), ctypes.byref(ts[0]), ctypes.byref(ts[1]), *[p(t) for t in self.ps], p(self.d_qbar), p(self.d_kbar),
                  ctypes.byref(ts[2]), ctypes.byref(ts[3]), p(self.out["part"].t), p(self.out["dG_part"].t), p(self.stats.t)]
        if self.entry == "bwd_fin":
            return nv.lib().ea_lara_seglin_bwd_fin(*common, *[p(t) for t in self.fin], c["C"], float(c["scale"]), nv.stream())
        return nv.lib().ea_lara_seglin_bwd(*common, nv.stream())

    def results(self):
        """Checks what every run must hold (finite outputs, guards, untouched slots) and -> the compared tensors on the CPU
        (+ the raw partials and the raw 16-bit buffers under `raw_*`)."""
        torch.cuda.synchronize()
        c, B, h = self.c, self.c["B"], self.c["h"]
        for n_, b in self.out.items():
            b.check(n_)
        for s_ in self.keep:
            assert torch.equal(_bits(self.grad[:, :, s_]), _bits(self.prefill[:, :, s_])), "%s: slot %d of the gradient buffer changed" % (self.name, s_)
        res = {n_: self.out[n_].t.detach().cpu().clone() for n_ in self.out if n_ in ("qbar", "kbar", "mean")}
        if self.fam == "P":
            res["dx"] = _rows(self.grad, 0)
            res["dx_inc"] = res["dx"] - self.o["base"]
            res["raw_dx"] = _bits(_view(self.grad, 0)).cpu()
            return res
        if self.fam == "G":
            res["dq"], res["dk"] = _rows(self.grad, 3), _rows(self.grad, 4)
            assert bool(torch.isfinite(res["dq"]).all()) and bool(torch.isfinite(res["dk"]).all()), "a token of dq / dk was not written"
            if "part" in self.out:
                raw = res["raw_part"] = self.out["part"].t.detach().cpu().clone()             # [B,h,L,2,4,D]
                res["part"] = raw.double().sum(2)
                if self.mask is None:
                    assert bool((raw[..., 3, :] == 0).all()), "no mask, but the d mbias plane is not zero"
            res["raw_dq"], res["raw_dk"] = _bits(_view(self.grad, 3)).cpu(), _bits(_view(self.grad, 4)).cpu()
            return res
        self.stats.guard_ok("stats")
        res["dq"], res["dk"] = _rows(self.grad, 0), _rows(self.grad, 1)
        res["dq_inc"], res["dk_inc"] = res["dq"] - self.o["base_q"], res["dk"] - self.o["base_k"]
        raw = res["raw_part"] = self.out["part"].t.detach().cpu().view(B, h, self.groups, 2, 4, 64).clone()
        assert bool((raw[..., 3, :] == 0).all()), "the fourth plane of seglin's part is not zero"
        res["part"] = raw.double().sum(2)[..., :3, :]
        rawg = res["raw_dG"] = self.out["dG_part"].t.detach().cpu().view(B, h, self.groups, 2, 64, 64).clone()
        res["dG"] = rawg.double().sum(2)
        res["raw_dq"], res["raw_dk"] = _bits(_view(self.grad, 0)).cpu(), _bits(_view(self.grad, 1)).cpu()
        return res


def _run_case(name, dt, **kw):
    r = _Run(name, dt, **kw)
    assert r.forward() == 0 and r.backward() == 0, (name, dt)
    return r.results()


_GOT, _REF = {}, {}


def _got(name, dt):
    if (name, dt) not in _GOT:
        _GOT[name, dt] = _run_case(name, dt)
    return _GOT[name, dt]


def _ref(name, dt):
    """(R, M) of a case, computed once and shared."""
    if (name, dt) not in _REF:
        c, o = sc.operands(name, dt)
        _REF[name, dt] = (sr.reference(c, o), sr.model(c, o, sc.DTYPES[dt]))
    return _REF[name, dt]


def _compared(got):
    return sorted(n_ for n_ in got if not n_.startswith("raw_"))


def _same_bits(a, b, tag):
    assert set(a) == set(b)
    for n_ in a:
        assert torch.equal(a[n_], b[n_]), tag + (n_,)


def _hold_to_bound(tag, got, R, M, td, names):
    bad, lines, worst, worst_ratio = [], [], 0.0, (0.0, "")
    for n_ in names:
        ok, txt, ratio = sr.bound_report(n_, got[n_], M[n_], R[n_], td)
        f = sr.floor_for(n_, td)
        used = max(g_ / (sr.FACTOR * m_ + f) for g_, m_ in zip((sr.a_err(got[n_], R[n_]),) + sr.norm_errs(got[n_], R[n_]),
                                                               (sr.a_err(M[n_], R[n_]),) + sr.norm_errs(M[n_], R[n_])))
        worst = max(worst, used)
        if sr.a_err(M[n_], R[n_]) > 0 and ratio > worst_ratio[0]:
            worst_ratio = (ratio, n_)
        lines.append("%s %s  bound used %.2f" % (tag, txt, used))
        if not ok:
            bad.append(n_)
    print("\n" + "\n".join(lines) + "\n%s worst a(HIP) / a(M) %.2f (%s), worst share of the bound %.2f" % ((tag,) + worst_ratio + (worst,)))
    assert not bad, "%s: %s exceed 4 a(M) + f\n%s" % (tag, bad, "\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.NAMES)
def test_segment_kernels_match_fp64_same_operand_reference(name, dt):
    c = sc.CASES[name]
    if name == "H4":
        # a condition of the case, not a check of the kernel: several segments per wave in both column passes on this device
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        fw, bw = sr.col_groups(c["B"], c["h"], c["L"], cus, False), sr.col_groups(c["B"], c["h"], c["L"], cus, True)
        print("\nH4 on %d CUs: (per, cgroups, segments per group) forward %s, dq / dk pass %s; dG pass %s" % (
            cus, fw, bw, sr.seglin_groups(c["B"] * c["h"], c["L"])))
        assert fw[0] >= 2 and bw[0] >= 2
    got = _got(name, dt)                                              # (finite everywhere, guards and foreign slots intact: _Run.results)
    R, M = _ref(name, dt)
    names = _compared(got)
    assert set(names) == set(R) - (set() if c.get("part", True) else {"part"})
    _hold_to_bound("%s %s" % (name, dt), got, R, M, sc.DTYPES[dt], names)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.NAMES)
def test_two_runs_are_bit_identical(name, dt):
    _same_bits(_got(name, dt), _run_case(name, dt), (name, dt))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.SAME_B)
def test_batch_rows_are_independent(name, dt):
    """Every batch row holds the same data: the rows of every result must agree bit for bit."""
    got = _run_case(name, dt, same_b=True)
    for n_, t in got.items():
        assert t.shape[0] == sc.CASES[name]["B"] and bool((t == t[:1]).all()), (name, dt, n_)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", ["G1", "H1"])
def test_time_first_storage_gives_the_same_bits(name, dt):
    """The same values stored [N,B,...] and passed as permuted views (other batch / token strides)."""
    _same_bits(_got(name, dt), _run_case(name, dt, time_first=True), (name, dt))


ZERO_SCALE = ("G1", "G2", "G5", "H1", "H3", "H4")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", ZERO_SCALE)
def test_zero_cotangents_give_exact_zeros(name, dt):
    """d_qbar = d_kbar = 0: the segment kernel writes exact zeros, seglin leaves dq / dk bit-identical to the base; every partial is
    exactly 0."""
    r = _Run(name, dt, gmul=0.0)
    assert r.forward() == 0 and r.backward() == 0
    got = r.results()
    if r.fam == "G":
        assert bool((got["dq"] == 0).all()) and bool((got["dk"] == 0).all())
        assert bool((got["raw_part"] == 0).all())
    else:
        assert torch.equal(_bits(r.grad), _bits(r.prefill)), "seglin changed dq / dk under zero cotangents"
        assert bool((got["raw_part"] == 0).all()) and bool((got["raw_dG"] == 0).all())
    _same_bits({n_: got[n_] for n_ in ("qbar", "kbar")}, {n_: _got(name, dt)[n_] for n_ in ("qbar", "kbar")}, (name, dt))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, -8], ids=["x2^8", "x2^-8"])
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", ZERO_SCALE)
def test_backward_is_homogeneous_under_loss_scaling(name, dt, k):
    """Both cotangents times 2^k: every fp32 partial is the unscaled one times 2^k bit for bit, and so is the segment kernel's
    written dq / dk -- where the I/O dtype can say so: an element whose value or whose scaled value lies below fp16's normal range
    (2^-14) is a multiple of 2^-24 there, so the two roundings may differ by 2^-24 max(1, 2^k) (half a spacing for either run);
    bf16 has no such element.  For the same reason seglin's dG, whose dz operand is rounded to the element type before the
    product, scales exactly in bf16, and in fp16 to within sum_n 2^-24 max(1, 2^k) |x_n| per input channel (every dz element
    at most that far off) plus the fp32 floor 2^-20 |dG|."""
    base, scaled = _got(name, dt), _run_case(name, dt, gmul=2.0 ** k)
    m = 2.0 ** k
    c, o = sc.operands(name, dt)
    _same_bits({n_: scaled[n_] for n_ in ("qbar", "kbar")}, {n_: base[n_] for n_ in ("qbar", "kbar")}, (name, dt))
    assert torch.equal(scaled["raw_part"], base["raw_part"] * m), (name, dt, "part")
    if c["fam"] == "G":
        tiny = float(torch.finfo(sc.DTYPES[dt]).tiny)
        for n_ in ("dq", "dk"):
            want = base[n_] * m
            normal = ((base[n_].abs() >= tiny) & (want.abs() >= tiny)) | (base[n_] == 0)
            diff = (scaled[n_] - want).abs()
            print("\n%s %s %s x2^%d: %d of %d elements outside the normal range, largest difference there %.3e" % (
                name, dt, n_, k, int((~normal).sum()), normal.numel(), float(diff[~normal].max()) if bool((~normal).any()) else 0.0))
            assert bool((diff[normal] == 0).all()), (name, dt, n_)
            assert dt == "fp16" or bool(normal.all())
            assert bool((diff[~normal] <= 2.0 ** -24 * max(1.0, m)).all()), (name, dt, n_)
    elif dt == "bf16":
        assert torch.equal(scaled["raw_dG"], base["raw_dG"] * m), (name, dt, "dG")
    else:
        want = base["dG"] * m
        ax = torch.stack([o["xq"].double().abs().sum(2), o["xk"].double().abs().sum(2)], 2)           # [B,h,2,64 (in)]
        tol = 2.0 ** -24 * max(1.0, m) * ax[:, :, :, None, :] + 2.0 ** -20 * want.abs()
        diff = (scaled["dG"] - want).abs()
        print("\n%s fp16 dG x2^%d: largest difference / tolerance %.3f" % (name, k, float((diff / tol.clamp_min(1e-300)).max())))
        assert bool((diff <= tol).all()), (name, dt, "dG")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sc.F_NAMES)
def test_fused_finish_touches_only_dq(name, dt):
    """dk and the partials of the k side do not depend on the finish: bit-identical to ea_lara_seglin_bwd's.  With u qbar = 0 (F1,
    F2) the whole result is."""
    fin, plain = _got(name, dt), _run_case(name, dt, entry="bwd")
    for n_ in ("raw_dk", "qbar", "kbar"):
        assert torch.equal(fin[n_], plain[n_]), (name, dt, n_)
    assert torch.equal(fin["raw_part"][:, :, :, 1], plain["raw_part"][:, :, :, 1]) and torch.equal(fin["raw_dG"][:, :, :, 1], plain["raw_dG"][:, :, :, 1])
    # the q side's partials do not read dq either
    assert torch.equal(fin["raw_part"], plain["raw_part"]) and torch.equal(fin["raw_dG"], plain["raw_dG"])
    assert not torch.equal(fin["raw_dq"], plain["raw_dq"])
    if name in ("F1", "F2"):
        _same_bits(_run_case(name, dt, zero_uq=True), plain, (name, dt, "u qbar = 0"))
