"""Case table of the 16-bit softmax core tests (tests/test_softmax_reference_cpu.py pins the plans on the CPU,
tests/test_gpu_softmax_core.py runs the kernels): one case per kernel variant of csrc/ea_softmax.hip, at the smallest shape that
reaches it.  PINS holds the tile counts (QT of the forward, QT = KT of the two backward kernels) that ea_softmax_tiles answers for
a device of 256 compute units -- B h ceil(N / 128) >= 512 for two tiles, B h ceil(N / 256) >= 512 (D <= 64, no keep mask) for
four -- so that a change of the rule cannot silently move a case off its variant."""
import torch

CUS = 256
KEEP_P = 0.2                      # attention dropout of the D / Q2d / Q2c cases
KEEP_SCALE = 1.0 / (1.0 - KEEP_P)


def _c(B, h, N, d, mask=False, keep=False, kb=False, views="fused", v_is_k=False):
    return dict(B=B, h=h, N=N, d=d, mask=mask, keep=keep, kb=kb, views=views, v_is_k=v_is_k)


CASES = {
    # fwd / bwd QT 1; three PL chunks, then a tail chunk of 8 keys in the additive body; a query tail (200 = 3 x 64 + 8)
    "S1": _c(2, 3, 200, 64),
    # PL body only: no tail chunk, no query tail
    "S2": _c(2, 3, 128, 64),
    # a tail chunk only (N < 64): the PL loop is empty
    "S3": _c(1, 2, 40, 64),
    # a mask: the additive body throughout (nfull = 0).  Row 0 pads its last 40 keys, row 1 its FIRST 70: the first whole 64-key
    # chunk of row 1 is dead, the running maximum is still -inf after it (msafe, alpha = exp2(-inf - 0))
    "S4": _c(2, 3, 200, 64, mask=True),
    # NSL 1 (d = 32: 256 staging slots, one per thread) and NSL 4 (d = 128); 130 = 2 x 64 + 2: two keys in the last chunk
    "S5": _c(2, 2, 150, 32, mask=True),
    "S6": _c(1, 2, 130, 128, mask=True),
    # DR in all three kernels; the keep rows are 64 ceil(N / 64) > N bytes apart and read as 32-bit words at kc + 16 tt + 4 g
    "D1": _c(2, 2, 200, 64, keep=True),
    "D1m": _c(2, 2, 200, 64, keep=True, mask=True),
    "D2": _c(1, 2, 100, 128, keep=True),
    "D3": _c(2, 2, 90, 32, keep=True),
    # B h = 256, ceil(200 / 128) = 2: fwd QT 2, bwd QT 2; the second query block (128 queries per workgroup) holds 72
    "Q2": _c(64, 4, 200, 64),
    # the additive body at QT 2, kdead at KT 2
    "Q2m": _c(64, 4, 200, 64, mask=True),
    # ceil(300 / 256) = 2: fwd QT 4 (256 queries per workgroup; the second block holds 44: three waves idle), bwd QT 2
    "Q4": _c(64, 4, 300, 64),
    "Q4m": _c(64, 4, 300, 64, mask=True),
    # fwd QT 4 at d = 32 with a single partial block (B h = 512, one block of 100 queries)
    "Q4s": _c(128, 4, 100, 32),
    # d = 128: fwd QT 2, bwd QT 1 (the backward has no two-tile variant above d = 64)
    "Q2w": _c(64, 4, 200, 128),
    # DR at QT 2 both ways; Q2c: the rule says four tiles (B h = 512), the keep mask clamps them to two
    "Q2d": _c(64, 4, 200, 64, keep=True),
    "Q2c": _c(128, 4, 100, 64, keep=True),
    # the key-norm term and its dk gradient (dscol), QT 1, at the three head sizes; q, k, v are views of separate tensors
    "K1": _c(2, 3, 200, 64, kb=True, views="separate"),
    "K1s": _c(2, 2, 150, 32, kb=True, views="separate"),
    "K1w": _c(1, 2, 130, 128, kb=True, views="separate"),
    # KB at fwd / bwd QT 2, and at fwd QT 4
    "K2": _c(64, 4, 200, 64, kb=True, views="separate"),
    "K4": _c(64, 4, 300, 64, kb=True, views="separate"),
    # RA's first softmax: q, k are [B,h,N,d] views of separate [B,N,h,d] tensors, v IS k, no key-norm term
    "V1": _c(2, 3, 200, 64, views="separate", v_is_k=True),
}

# name -> (forward QT, backward QT) at CUS compute units
PINS = {
    "S1": (1, 1), "S2": (1, 1), "S3": (1, 1), "S4": (1, 1), "S5": (1, 1), "S6": (1, 1),
    "D1": (1, 1), "D1m": (1, 1), "D2": (1, 1), "D3": (1, 1),
    "Q2": (2, 2), "Q2m": (2, 2), "Q4": (4, 2), "Q4m": (4, 2), "Q4s": (4, 2), "Q2w": (2, 1), "Q2d": (2, 2), "Q2c": (2, 2),
    "K1": (1, 1), "K1s": (1, 1), "K1w": (1, 1), "K2": (2, 2), "K4": (4, 2),
    "V1": (1, 1),
}

# every batch row the same data: S4 with the dead-leading-chunk mask on all rows, and Q4
BATCH_INDEPENDENCE = ("S4", "Q4")

# the sampler: (B, h, N, d), every shape in bf16 and fp16 and with both seeds (one above 2^32)
SAMPLER_SHAPES = ((2, 3, 200, 64), (1, 2, 40, 32), (1, 2, 130, 128))
SAMPLER_SEEDS = (0x5EED1234, (0x9E3779B9 << 32) | 0x7F4A7C15)


def seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def case_mask(c, B=None, same_rows=False):
    """[B,N] bool, True = padded key: even rows pad their last 40 keys, odd rows their FIRST 70.  same_rows: the odd rows' mask
    on every row."""
    B, N = c["B"] if B is None else B, c["N"]
    m = torch.zeros(B, N, dtype=torch.bool)
    m[0::2, N - 40:] = True
    m[1::2, :70] = True
    if same_rows:
        m[:] = False
        m[:, :70] = True
    return m


def operands(name, io, same_rows=False):
    """CPU operands of a case (seeded per case), 16-bit values held in fp32: q, k, v, dout [B,h,N,d] standard normal, drawn in
    fp32 and rounded once to the I/O dtype (v = k where the case says so); mask [B,N] bool or None; keep [B,h,N,N] uint8 0/1 or
    None.  same_rows: every batch row gets the data of row 0."""
    c = CASES[name]
    B, h, N, d = (1 if same_rows else c["B"]), c["h"], c["N"], c["d"]
    g = torch.Generator().manual_seed(seed(name))

    def r16(t):
        return t.to(io).float()
    o = dict(q=r16(torch.randn(B, h, N, d, generator=g)), k=r16(torch.randn(B, h, N, d, generator=g)),
             v=r16(torch.randn(B, h, N, d, generator=g)), dout=r16(torch.randn(B, h, N, d, generator=g)))
    if c["v_is_k"]:
        o["v"] = o["k"]
    o["keep"] = (torch.rand(B, h, N, N, generator=g) >= KEEP_P).to(torch.uint8) if c["keep"] else None
    if same_rows:
        o = {k_: (t if t is None else t.expand(c["B"], *t.shape[1:]).contiguous()) for k_, t in o.items()}
    o["mask"] = case_mask(c, same_rows=same_rows) if c["mask"] else None
    return c, o


def reference_kw(c, o):
    """The keyword arguments of softmax_reference.softmax_grads for a case's operands."""
    return dict(mask=o["mask"], keep=o["keep"], keep_scale=KEEP_SCALE if c["keep"] else 1.0, key_norm_bias=c["kb"],
                scale=c["d"] ** -0.5)
