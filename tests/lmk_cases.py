"""Case table of the landmark-pipeline core tests (tests/test_lmk_reference_cpu.py checks the reference, the model and the input
conditions on the CPU, tests/test_gpu_lmk_core.py runs lmk2_kernel<D, BWD> of csrc/ea_lmk2.hip through the C ABI): one case per
branch of the kernel.  BH is 4 to 6, so a launch is a few workgroups.  Operands are drawn in fp32 from a per-case seed.

Input scales: LayerNorm rows have |x|^2 = D gamma^2, so gamma ~ 0.7 (q side) keeps s |mu|^2 at a few units (D^-1/2 D 0.5 = 4 at
D = 64); without the MLP pq / pk take that role.  The fractions in the comments are properties of R alone (fp64), asserted by
tests/test_lmk_reference_cpu.py: `bhv` = share of bhv in [0.05, 0.95] (mis-opt, >= 0.5 required), `A` = share of the rows of the
mixing matrix whose largest entry is below 0.9 (mixed, >= 0.5 required)."""
import torch

MIS_CODE = {"opt": 0, "biased": 1, "bh": 2}


def _c(D, L, dup, has_mlp, mixed, mis, BH=5, eva=0, cb=False, noise=True, saved=(True, True), like=None, S=0, use=None,
       sp=1.0, gq=0.7, gk=0.6, sn=0.5):
    C = L * (2 if dup else 1)
    return dict(D=D, L=L, C=C, dup=dup, has_mlp=has_mlp, mixed=mixed, mis=mis, BH=BH, eva=eva, cb=cb, noise=noise,
                saved_fwd=saved[0], saved_bwd=saved[1], like=like, S=S, dom_scale=(float(D) ** -0.5 if S else 1.0),
                use=use or ("g_omega", "g_qrows", "g_bhv", "g_lp"), scale=float(D) ** -0.5, sp=sp, gq=gq, gk=gk, sn=sn)


CASES = {
    # the benchmark's geometry: L % 16 = 1 (one valid row in the fourth strip, 15 masked columns); the three estimators; qbar_rows
    # NULL for bh.  Observed: bhv share 1.00 (0.27 .. 0.75), A share 1.00 in all three (largest entry of A 0.35), s |mu|^2 4.4 .. 4.7
    "G1o": _c(64, 49, 0, 1, 1, "opt", BH=6),
    "G1b": _c(64, 49, 0, 1, 1, "biased", BH=6),
    "G1h": _c(64, 49, 0, 1, 1, "bh", BH=6),
    # antithetic sign and c % L noise rows, nrep = 2 in the normaliser, the fold of rows l + L onto l, dqs over both copies
    # (unmixed MLP).  gamma 0.45 / 0.4: with 0.7 / 0.6 the diagonal took 0.98 of its row at L = 16 (bhv 0.49 of at most 0.5).
    # Observed: bhv share 1.00 (0.19 .. 0.38 of at most 0.5), s |mu|^2 3.2
    "G2": _c(64, 16, 1, 1, 0, "opt", gq=0.45, gk=0.4),
    # independent noise [BH, C, D]; C = 64 with no padded sample row; k0 read from pk (mixed without the MLP), `saved` required
    # Observed: bhv share 1.00 (0.08 .. 0.30 of at most 0.5), A share 1.00 in both (largest entry 0.60), s |mu|^2 2.8
    "G3o": _c(64, 32, 2, 0, 1, "opt", sp=0.55),
    "G3b": _c(64, 32, 2, 0, 1, "biased", sp=0.55),
    # D = 32 (NT = 2, KD = 1, only waves 0 and 1 own dW rows); L = 64 with no masked column.  Observed: A share 1.00 (largest
    # entry 0.15), s |mu|^2 3.3
    "G4": _c(32, 64, 0, 1, 1, "biased", BH=4),
    # the have_mu == false backward (mu rebuilt from pq + pk; `saved` NULL both ways); three waves with no valid row
    # Observed: bhv share 1.00 (0.17 .. 0.43 of at most 0.5), s |mu|^2 2.5
    "G5": _c(32, 7, 1, 0, 0, "opt", saved=(False, False), sp=0.45),
    # the _cb entries: column bias and d_colbias; one row in the third strip.  Observed: A share 1.00 (largest entry 0.66)
    "G6": _c(64, 33, 0, 1, 1, "bh", cb=True),
    # the eval forward and a backward with noise == NULL.  Observed: bhv share 1.00 (0.42 .. 0.70), A share 1.00 (largest entry 0.35)
    "G7": _c(64, 49, 0, 1, 1, "opt", noise=False),
    # _bwd_parts on G1o's operands: the fold of ea_slice_sum on load, dom_S = 1, 3, 4, dom_scale = s
    "G8a": _c(64, 49, 0, 1, 1, "opt", BH=6, like="G1o", S=1),
    "G8b": _c(64, 49, 0, 1, 1, "opt", BH=6, like="G1o", S=3),
    "G8c": _c(64, 49, 0, 1, 1, "opt", BH=6, like="G1o", S=4),
    # the optional gradient inputs d_qbar_rows and d_bhv NULL, on G1o's operands
    "G9": _c(64, 49, 0, 1, 1, "opt", BH=6, like="G1o", use=("g_omega", "g_lp")),
    # EVA: the early return of the forward, the d rf_k_bar input, the shared tail; noise given / NULL
    "E1": _c(64, 49, 0, 1, 0, "opt", eva=1),
    "E2": _c(32, 16, 0, 1, 0, "opt", eva=1, BH=4, noise=False),
}

NAMES = sorted(CASES)
OPT = [n_ for n_ in NAMES if CASES[n_]["mis"] == "opt" and not CASES[n_]["eva"]]
MIXED = [n_ for n_ in NAMES if CASES[n_]["mixed"]]
HOMOGENEITY = ("G1o", "G3b", "G6", "E1")


def seed(name):
    return 7000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def operands(name, same_bh=False):
    """(c, o): geometry and fp32 CPU operands of a case.  pq, pk [BH,L,D]; the eight parameters (shared by every (b,h), as the
    kernel gets them); noise [BH,L,D] (dup 0, 1) | [BH,C,D] (dup 2) | None; colbias [BH,L]; the incoming gradients g_omega, g_qrows
    [BH,C,D] (EVA: [BH,L,D]), g_bhv, g_lp [BH,C]; parts [BH,S,C,D].  same_bh: every (b,h) gets the data of the first."""
    c = CASES[name]
    D, L, C, BH = c["D"], c["L"], c["C"], c["BH"]
    g = torch.Generator().manual_seed(seed(c["like"] or name))
    n = 1 if same_bh else BH

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    o = dict(pq=c["sp"] * rn(n, L, D), pk=c["sp"] * rn(n, L, D))
    o.update(Wq=rn(D, D) / D ** 0.5, bq=0.1 * rn(D), gq=c["gq"] * (1 + 0.1 * rn(D)), cq=0.1 * rn(D),
             Wk=rn(D, D) / D ** 0.5, bk=0.1 * rn(D), gk=c["gk"] * (1 + 0.1 * rn(D)), ck=0.1 * rn(D))
    nrows = C if c["dup"] == 2 else L
    noise = c["sn"] * rn(n, nrows, D)
    o["noise"] = noise if c["noise"] else None
    colbias = 0.5 * rn(n, L)
    o["colbias"] = colbias if c["cb"] else None
    R = L if c["eva"] else C
    o.update(g_omega=rn(n, R, D), g_qrows=rn(n, R, D), g_bhv=rn(n, R), g_lp=rn(n, R))
    o["parts"] = rn(n, c["S"], C, D) if c["S"] else None               # (drawn last: the cases `like` G1o share all the rest)
    if not c["has_mlp"]:
        for n_ in ("Wq", "bq", "gq", "cq", "Wk", "bk", "gk", "ck"):
            o[n_] = None
    if c["eva"]:
        o["g_bhv"] = o["g_lp"] = None
    elif c["mis"] != "opt":
        o["g_bhv"] = None
        if c["mis"] == "bh":
            o["g_qrows"] = None
    if same_bh:
        o = {k_: (t if (t is None or k_ in ("Wq", "bq", "gq", "cq", "Wk", "bk", "gk", "ck")) else t.expand(BH, *t.shape[1:]).contiguous())
             for k_, t in o.items()}
    return c, o
