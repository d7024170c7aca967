"""Case table of the 16-bit LARA estimator core tests (tests/test_lara_reference_cpu.py pins the plans on the CPU,
tests/test_gpu_lara_core.py runs the kernels): the smallest shapes that reach each host-selected variant of the token passes.
PINS holds what the library answers for every case -- ea_lara_parts (slices of the token-row passes: forward statistics, two-pass
backward), ea_lara_fused_parts (slices of the fused backward; -2 = refused, C > 64), whether the merge is folded into its consumer
on each side (_ops.lara_fold), NCT = ceil(C / 16) and the `lh1` switch of lara_fq_kernel -- so that a planner change cannot
silently move a case off its plan."""
import torch

KAPPA = 0.25
MIS_CODE = {"opt": 0, "biased": 1, "bh": 2}


def _c(B, h, N, d, C, mis=("opt",), mask_tail=0, fold=True, time_first=False):
    return dict(B=B, h=h, N=N, d=d, C=C, mis=tuple(mis), mask_tail=mask_tail, fold=fold, time_first=time_first)


CASES = {
    # NCT 4, LH 1, parts 1 / fused 2, both folded, two slices at token 64, N tail of 4 -- in all three estimator variants
    "A1": _c(2, 3, 100, 64, 49, mis=("opt", "biased", "bh")),
    # key-padding mask: the last 37 keys of batch row 1 are padded
    "A1m": _c(2, 3, 100, 64, 49, mask_tail=37),
    # EA_LARA_FOLD=0: ea_lara_merge_fwd / _bwd and the unmerged out_fwd / bwd_k_fused on the operands of A1
    "A1u": _c(2, 3, 100, 64, 49, fold=False),
    # LH 2, no padded landmark slot
    "A2": _c(2, 3, 100, 64, 64),
    # d = 32, NCT 1 in the NCT <= 2 template, parts 8 / fused 8: unfolded both ways
    "A3": _c(2, 3, 200, 32, 16),
    # one slice (nsplit 1), parts 2 / fused 2
    "A4": _c(2, 3, 64, 32, 32, mis=("biased",)),
    # the two sides of the lh1 switch (C - 48 <= 2)
    "A5": _c(2, 3, 100, 64, 50),
    "A6": _c(2, 3, 100, 64, 51),
    # one landmark in the second tile; parts 4 (folded forward), fused 6 (unfolded backward)
    "A7": _c(2, 3, 150, 32, 17),
    # NCT 3 in the NCT 4 template, three slices, fused 3 folded
    "A8": _c(2, 3, 130, 64, 33, mis=("bh",)),
    # C > 64: the two-pass ea_lara_bwd_q / _qstats / _k / _kstats / _qcorr, NCT 7 in the 8 template
    "T1": _c(2, 3, 200, 64, 98),
    # the same route at d = 32, one landmark in the fifth tile
    "T2": _c(2, 3, 200, 32, 65, mis=("biased",)),
    # 16 slices (parts 8, fused 16); time-first storage: qkv5 is a view of [N,B,3,h,d]
    "O1": _c(1, 3, 1000, 64, 49, time_first=True),
    # cfg2's plan.  B h = 384: with 384 < slots < 768 (256 CUs x 2 workgroups of lara_fq_kernel) lara_f_plan (F = 160) gives the
    # query side an EMPTY second slice (512 slots: rb = 3, b = ((196 - 2 * 160) / 4 + 32) / 64 * 64 = 0 < 16) and the key side, where
    # both slices of every (b,h) are resident (3 per CU: slots >= 768), 192 + 4 (last_extra = 128: ((196 + 128) / 2 + 32) / 64 * 64 = 192; 128 + 68 when
    # they are not).  Expected, not asserted: occupancy x CUs has no host query, and the bound holds whichever branch runs
    "E1": _c(128, 3, 196, 64, 49),
    # the unequal-halves plan: for 512 slots rb = 3, b = ((450 - 2 * 160) / 4 + 32) / 64 * 64 = 64 -> 386 + 64 on the query side;
    # lara_y_plan's uneven forward slices (F = 112); a masked tail on batch row 1.  Expected, not asserted (as E1)
    "E2": _c(128, 3, 450, 32, 49, mask_tail=70),
}

PIN_NAMES = ("parts", "fused", "fold_fwd", "fold_bwd", "nct", "lh1")
PINS = {
    "A1": (1, 2, True, True, 4, True),
    "A1m": (1, 2, True, True, 4, True),
    "A1u": (1, 2, False, False, 4, True),
    "A2": (1, 2, True, True, 4, False),
    "A3": (8, 8, False, False, 1, False),
    "A4": (2, 2, True, True, 2, False),
    "A5": (1, 2, True, True, 4, True),
    "A6": (1, 2, True, True, 4, False),
    "A7": (4, 6, True, False, 2, False),
    "A8": (2, 3, True, True, 3, True),
    "T1": (2, -2, False, False, 7, False),
    "T2": (2, -2, False, False, 5, False),
    "O1": (8, 16, False, False, 4, True),
    "E1": (2, 2, True, True, 4, True),
    "E2": (2, 2, True, True, 4, True),
}

# (case, mis) of every run
RUNS = [(n_, m) for n_ in sorted(CASES) for m in CASES[n_]["mis"]]


def nct(C):
    return (C + 15) // 16


def lh1(C):
    """launch_f (ea_lara_f.hip): the NCT = 4 template with at most two samples in its last tile (or none: NCT = 3)."""
    return 2 < nct(C) <= 4 and C - 48 <= 2


def seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def operands(name, mis, io, same_rows=False):
    """CPU operands of a case (seeded per case; A1u gets A1's), 16-bit values held in fp32: q, k, v, dout = randn rounded to the
    I/O dtype; fp32 landmark tensors omega = randn, qbar = 0.5 randn, bhv = softmax_c(0.25 randn), lp = randn.  mask [B,N] bool or
    None.  same_rows: every batch row gets the data of row 0 (and no mask)."""
    c = CASES[name]
    B, h, N, d, C = (1 if same_rows else c["B"]), c["h"], c["N"], c["d"], c["C"]
    g = torch.Generator().manual_seed(seed("A1" if name == "A1u" else name))

    def r16(t):
        return t.to(io).float()
    o = dict(q=r16(torch.randn(B, h, N, d, generator=g)), k=r16(torch.randn(B, h, N, d, generator=g)),
             v=r16(torch.randn(B, h, N, d, generator=g)), dout=r16(torch.randn(B, h, N, d, generator=g)),
             omega=torch.randn(B, h, C, d, generator=g), qbar=0.5 * torch.randn(B, h, C, d, generator=g),
             bhv=torch.softmax(0.25 * torch.randn(B, h, C, generator=g), -1), lp=torch.randn(B, h, C, generator=g))
    if mis == "bh":
        o["qbar"] = None
    if mis != "opt":
        o["bhv"] = None
    if same_rows:
        o = {k_: (t if t is None else t.expand(c["B"], *t.shape[1:]).contiguous()) for k_, t in o.items()}
    o["mask"] = None
    if c["mask_tail"] and not same_rows:
        o["mask"] = torch.zeros(B, N, dtype=torch.bool)
        o["mask"][1, N - c["mask_tail"]:] = True
    return c, o
