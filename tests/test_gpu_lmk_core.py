"""-m gpu: the landmark pipeline lmk2_kernel<D, BWD> (csrc/ea_lmk2.hip) -- Linear + LayerNorm, the softmax mixing of k_bar, mu, omega,
the [C x L] proposal densities and the whole backward with its per-(b,h) parameter partials -- called through the C ABI
(ea_lara_landmarks_fwd / _bwd / _bwd_parts / _fwd_cb / _bwd_cb) on the test's own fp32 tensors, against an fp64 evaluation of the
SAME operands (tests/lmk_reference.py), one case per branch of the kernel (tests/lmk_cases.py; the reference, the model and the
input conditions are held on the CPU by tests/test_lmk_reference_cpu.py).

Bound, per compared tensor X with the exact reference R and the rounding model M (the kernel's arithmetic in fp32 with its fp16
operand roundings): a(X) = max_i |X_i - R_i| / (rms(R) + |R_i|) must satisfy a(HIP) <= 4 a(M) + f, and so must the two norm-wise
figures (max / max, rms / rms); every result is fp32, so f = 2^-20.  The factor and the floor are window_reference's, fixed before
anything was measured; M and R are computed at test time: no recorded constants.  `pytest -s` prints a(HIP) / a(M) and the share
of the bound used per tensor; DESIGN.md 4b carries the worst figures observed.

Every output is prefilled with NaN and followed by a 64-float guard: after the call every element is finite and the guard is
still NaN bit for bit."""
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

import lmk_cases as lc                  # noqa: E402
import lmk_reference as lr              # noqa: E402

NAN = float("nan")
GUARD = 64
EA_E_BADARG = -1
FWD_OUT = ("omega", "qbar_rows", "bhv", "lp")
BWD_OUT = ("dpq", "dpk", "dW_part", "dvec_part", "d_colbias")


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

    def check(self, name):
        assert bool(torch.isfinite(self.t).all()), "%s holds elements no launch wrote (or non-finite values)" % name
        assert bool((self.flat[self.n:].view(torch.int32) == self.bits).all()), "%s: the guard behind it was written" % name


def _dev(t, mul=None):
    if t is None:
        return None
    t = t.float() if mul is None else t.float() * mul
    return t.contiguous().cuda()


def _geom(c, **over):
    from efficient_attention import _native as nv
    f = dict(BH=c["BH"], L=c["L"], C=c["C"], D=c["D"], has_mlp=c["has_mlp"], mixed=c["mixed"], mis=lc.MIS_CODE[c["mis"]], dup=c["dup"],
             scale=c["scale"], eva=c["eva"])
    f.update(over)
    return nv.ea_lmk_geom(f["BH"], f["L"], f["C"], f["D"], f["has_mlp"], f["mixed"], f["mis"], f["dup"], float(f["scale"]), f["eva"])


class _Run:
    """Device tensors of one case and the two launches.  gmul: factor on every incoming gradient (a power of two or 0)."""

    def __init__(self, c, o, gmul=None, saved=None):
        from efficient_attention import _native as nv
        self.nv, self.c = nv, c
        BH, L, C, D = c["BH"], c["L"], c["C"], c["D"]
        R = L if c["eva"] else C
        self.geom = _geom(c)
        self.pq, self.pk = _dev(o["pq"]), _dev(o["pk"])
        self.params = [_dev(o[n_]) for n_ in lr.PARAMS]
        self.noise, self.colbias = _dev(o["noise"]), _dev(o["colbias"])
        use = c["use"]
        self.g_omega = _dev(o["g_omega"], gmul)
        self.g_qrows = _dev(o["g_qrows"], gmul) if "g_qrows" in use else None
        self.g_bhv = _dev(o["g_bhv"], gmul) if "g_bhv" in use else None
        self.g_lp = _dev(o["g_lp"], gmul)
        self.parts = _dev(o["parts"], gmul)
        mis = c["mis"]
        self.out = dict(omega=_Out(BH, R, D))
        if c["eva"] or mis != "bh":
            self.out["qbar_rows"] = _Out(BH, R, D)
        if not c["eva"]:
            self.out["lp"] = _Out(BH, C)
            if mis == "opt":
                self.out["bhv"] = _Out(BH, C)
        self.out.update(dpq=_Out(BH, L, D), dpk=_Out(BH, L, D))
        if c["has_mlp"]:
            self.out.update(dW_part=_Out(BH, 2, D, D), dvec_part=_Out(BH, 2, 3, D))
        if c["cb"]:
            self.out["d_colbias"] = _Out(BH, L)
        n_saved = int(nv.lib().ea_lara_landmarks_saved_floats(ctypes.byref(self.geom)))
        assert n_saved == BH * (3 * L * D + 64 * L + 128)
        want = (c["saved_fwd"], c["saved_bwd"]) if saved is None else saved
        self.saved = _Out(n_saved) if any(want) else None           # (a workspace: only its guard is looked at)
        self.saved_fwd = self.saved.t if want[0] else None
        self.saved_bwd = self.saved.t if want[1] else None

    def _p(self, name):
        return self.nv.ptr(self.out[name].t) if name in self.out else None

    def forward(self):
        nv, p = self.nv, self.nv.ptr
        head = [ctypes.byref(self.geom), p(self.pq), p(self.pk)] + [p(t) for t in self.params] + [p(self.noise)]
        tail = [self._p("omega"), self._p("qbar_rows"), self._p("bhv"), self._p("lp"), p(self.saved_fwd), nv.stream()]
        if self.c["cb"]:
            return nv.lib().ea_lara_landmarks_fwd_cb(*head, p(self.colbias), *tail)
        return nv.lib().ea_lara_landmarks_fwd(*head, *tail)

    def backward(self, entry=None, d_omega=None, S=None, noise="case"):
        """entry: None = the case's own (`_bwd_cb` with a column bias, `_bwd_parts` with parts, else `_bwd`)."""
        nv, p, c = self.nv, self.nv.ptr, self.c
        entry = entry or ("bwd_cb" if c["cb"] else "bwd_parts" if c["S"] else "bwd")
        head = [ctypes.byref(self.geom), p(self.pq), p(self.pk)] + [p(t) for t in self.params] + [p(self.noise if noise == "case" else noise)]
        dom = self.g_omega if d_omega is None else d_omega
        gr = [p(self.g_qrows), p(self.g_bhv), p(self.g_lp), self._p("dpq"), self._p("dpk"), self._p("dW_part"), self._p("dvec_part")]
        if entry == "bwd_cb":
            return nv.lib().ea_lara_landmarks_bwd_cb(*head, p(self.colbias), p(dom), *gr, self._p("d_colbias"), p(self.saved_bwd), nv.stream())
        if entry == "bwd_parts":
            return nv.lib().ea_lara_landmarks_bwd_parts(*head, p(dom), c["S"] if S is None else S, p(self.parts), float(c["dom_scale"]), *gr,
                                                        p(self.saved_bwd), nv.stream())
        return nv.lib().ea_lara_landmarks_bwd(*head, p(dom), *gr, p(self.saved_bwd), nv.stream())

    def results(self, names=None):
        torch.cuda.synchronize()
        for n_, b in self.out.items():
            if names is None or n_ in names:
                b.check(n_)
        if self.saved is not None:
            assert bool((self.saved.flat[self.saved.n:].view(torch.int32) == self.saved.bits).all()), "the guard behind `saved` was written"
        return {n_: b.t.detach().cpu().clone() for n_, b in self.out.items() if names is None or n_ in names}


def _run_case(name, **kw):
    c, o = lc.operands(name, same_bh=kw.pop("same_bh", False))
    r = _Run(c, o, **kw)
    assert r.forward() == 0 and r.backward() == 0, name
    return r.results()


_GOT, _REF = {}, {}


def _got(name):
    if name not in _GOT:
        _GOT[name] = _run_case(name)
    return _GOT[name]


def _ref(name):
    """(R, M) of a case, computed once and shared."""
    if name not in _REF:
        c, o = lc.operands(name)
        _REF[name] = (lr.reference(c, o, use=c["use"]), lr.model(c, o, use=c["use"]))
    return _REF[name]


def _hold_to_bound(tag, got, R, M, names=None):
    bad, lines, worst, worst_ratio = [], [], 0.0, (0.0, "")
    for n_ in R:
        if names is not None and n_ not in names:
            continue
        ok, txt, ratio = lr.bound_report(n_, got[n_], M[n_], R[n_], lr.H16)
        f = lr.floor_for(n_, lr.H16)
        used = max(g_ / (lr.FACTOR * m_ + f) for g_, m_ in zip((lr.a_err(got[n_], R[n_]),) + lr.norm_errs(got[n_], R[n_]),
                                                               (lr.a_err(M[n_], R[n_]),) + lr.norm_errs(M[n_], R[n_])))
        worst = max(worst, used)
        if lr.a_err(M[n_], R[n_]) > 0 and ratio > worst_ratio[0]:
            worst_ratio = (ratio, n_)
        lines.append("%s %s  bound used %.2f" % (tag, txt, used))
        if not ok:
            bad.append(n_)
    print("\n" + "\n".join(lines) + "\n%s worst a(HIP) / a(M) %.2f (%s), worst share of the bound %.2f" % ((tag,) + worst_ratio + (worst,)))
    assert not bad, "%s: %s exceed 4 a(M) + f\n%s" % (tag, bad, "\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("name", lc.NAMES)
def test_landmark_kernels_match_fp64_same_operand_reference(name):
    got = _got(name)                                                  # (finite everywhere, guards intact: _Run.results)
    R, M = _ref(name)
    assert set(got) == set(R)
    _hold_to_bound(name, got, R, M)


@pytest.mark.gpu
@pytest.mark.parametrize("name", lc.NAMES)
def test_two_runs_are_bit_identical(name):
    a, b = _got(name), _run_case(name)
    for n_ in a:
        assert torch.equal(a[n_], b[n_]), (name, n_)


@pytest.mark.gpu
@pytest.mark.parametrize("name", lc.NAMES)
def test_bh_slices_are_independent(name):
    """Every (b,h) holds the same data: all (b,h) slices of every result must be bit-identical."""
    got = _run_case(name, same_bh=True)
    for n_, t in got.items():
        assert bool((t == t[:1]).all()), (name, n_)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["G8a", "G8b", "G8c"])
def test_bwd_parts_is_bwd_on_ea_slice_sum(name):
    """ea_lara_landmarks_bwd_parts(d_omega, parts, dom_S, s) against ea_lara_landmarks_bwd on ea_slice_sum(d_omega, parts, s): the
    header claims ea_slice_sum's order of additions, so the results are bit-identical; both lie within the bound of R on
    s (d_omega + sum parts)."""
    c, o = lc.operands(name)
    folded = _got(name)
    r = _Run(c, o)
    nv = r.nv
    BH, C, D, S = c["BH"], c["C"], c["D"], c["S"]
    summed = torch.full((BH, C, D), NAN, dtype=torch.float32, device="cuda")
    nv.call("ea_slice_sum", BH, S, C * D, float(c["dom_scale"]), nv.ptr(r.g_omega), nv.ptr(r.parts), nv.ptr(summed), nv.stream())
    assert r.forward() == 0 and r.backward(entry="bwd", d_omega=summed) == 0
    plain = r.results()
    for n_ in BWD_OUT[:4]:
        assert torch.equal(plain[n_], folded[n_]), (name, n_)
    R, M = _ref(name)
    _hold_to_bound(name + " via ea_slice_sum", plain, R, M, names=BWD_OUT)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, -16], ids=["x2^16", "x2^-16"])
@pytest.mark.parametrize("name", lc.HOMOGENEITY)
def test_backward_is_homogeneous_under_loss_scaling(name, k):
    """Every incoming gradient times 2^k: every backward result is the unscaled one times 2^k, bit for bit -- pow2_scale is an exact
    power of two, so the fp16 images of the gradient-side operands do not change."""
    base, scaled = _got(name), _run_case(name, gmul=2.0 ** k)
    for n_ in BWD_OUT:
        if n_ in base:
            assert torch.equal(scaled[n_], base[n_] * 2.0 ** k), (name, n_, float((scaled[n_] - base[n_] * 2.0 ** k).abs().max()))
    for n_ in FWD_OUT:
        if n_ in base:
            assert torch.equal(scaled[n_], base[n_]), (name, n_)


@pytest.mark.gpu
def test_all_zero_gradients_give_all_zero_results():
    """pow2_scale's m == 0 branch: a scale of 1, no 0 * inf."""
    got = _run_case("G1o", gmul=0.0)
    for n_ in BWD_OUT[:4]:
        assert bool((got[n_] == 0).all()), n_                        # (finite: _Run.results)


@pytest.mark.gpu
def test_saved_workspace_does_not_change_the_unparametrised_case():
    """G5 (no MLP, no mixing) with a `saved` workspace supplied both ways: the same forward bits, a backward within the bound.
    Whether the backward is bit-identical too is printed, not asserted."""
    base, with_ws = _got("G5"), _run_case("G5", saved=(True, True))
    for n_ in FWD_OUT:
        assert torch.equal(base[n_], with_ws[n_]), n_
    R, M = _ref("G5")
    _hold_to_bound("G5 with saved", with_ws, R, M)
    print("G5 backward with `saved` bit-identical to the run without: %s" % {n_: torch.equal(base[n_], with_ws[n_]) for n_ in ("dpq", "dpk")})


@pytest.mark.gpu
def test_entry_level_refusals_next_to_the_accepted_call():
    """On real device tensors, so that only the refused argument differs from a call that runs: `_cb` on an unmixed geometry,
    dom_S = 0 and 5, antithetic noise NULL -- each EA_E_BADARG with no output written."""
    c, o = lc.operands("G8b")
    r = _Run(c, o)
    assert r.forward() == 0
    for S in (0, 5):
        assert r.backward(S=S) == EA_E_BADARG
    c6, o6 = lc.operands("G6")
    r6 = _Run(c6, o6)
    r6.geom = _geom(c6, mixed=0)
    assert r6.forward() == EA_E_BADARG and r6.backward() == EA_E_BADARG
    c2, o2 = lc.operands("G2")
    r2 = _Run(c2, o2)
    r2.noise = None
    assert r2.forward() == EA_E_BADARG and r2.backward() == EA_E_BADARG
    torch.cuda.synchronize()
    for run, names in ((r, BWD_OUT), (r6, None), (r2, None)):
        for n_, b in run.out.items():
            if names is None or n_ in names:
                assert bool(torch.isnan(b.flat).all()), "a refused call wrote %s" % n_
