"""Cases, operands and the runner of tests/test_gpu_wgrad_stages.py, shared with the two child processes it starts (one per
setting of EA_WGRAD_STAGES, which the library reads once per process).

The stage loop of wgrad_kernel can go wrong at the first two and the last two 64-row stages of a token slice, so the cases are
slices of 1 .. 7 stages whose last stage holds 1, 63 or 64 rows.  With two stages in flight the loop has a steady part that
runs while two further whole stages exist (slices of >= 256 rows) and a drain of one to four stages, hence the row counts
beyond the five-stage ones: 193 / 256 (four stages, drain only), 321 (one steady trip, drain of four), 385 (two trips)."""
import sys

ROWS_PER_SLICE = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 319, 320, 321, 385)
# op -> the (out, in) sizes of its products; "pair": ea_wgrad_pair, both products over the same token rows in one launch
OPS = {"w192": ((192, 192),), "w576": ((576, 192),), "pair": ((576, 192), (192, 192))}
DTYPES = ("bf16", "fp16")


def slice_query(op):
    """rows -> slice count of the op's launch, asked of the library (ea_wgrad_parts / ea_wgrad_pair_parts)."""
    from efficient_attention import _native as nv
    shapes = OPS[op]
    if len(shapes) == 1:
        return lambda rows: int(nv.lib().ea_wgrad_parts(rows, *shapes[0]))
    return lambda rows: int(nv.lib().ea_wgrad_pair_parts(rows, *shapes[0], *shapes[1]))


def rows_for(op, n):
    """(rows, S): a row count that the library cuts into S slices of exactly n rows each."""
    query = slice_query(op)
    for S in range(1, 513):                    # the smallest such count (8 slices below 256 rows each, one per CU from there)
        if query(S * n) == S:
            return S * n, S
    raise AssertionError("no row count with slices of %d rows for %s" % (n, op))


def operands(op, n, dtype):
    """[(dy, x)] per product, on the GPU: random, with the first and the last row of every 64-row stage of every slice (and the
    slice's last row) 8 times larger -- a row taken from the wrong stage, dropped or counted twice moves the result by far
    more than the bound."""
    import torch
    td = torch.bfloat16 if dtype == "bf16" else torch.float16
    rows, S = rows_for(op, n)
    g = torch.Generator(device="cuda").manual_seed(1000 * n + len(op) + (7 if dtype == "fp16" else 0))
    local = torch.arange(rows, device="cuda") % n
    edge = ((local % 64 == 0) | (local % 64 == 63) | (local == n - 1)).float() * 7.0 + 1.0
    out = []
    for M, K in OPS[op]:
        dy = (torch.randn(rows, M, device="cuda", generator=g) * 0.5 + 0.1) * edge[:, None]
        x = torch.randn(rows, K, device="cuda", generator=g) * edge[:, None]
        out.append((dy.to(td), x.to(td)))
    return out


def run(op, n, dtype, bias):
    """[(dW, db | None)] per product, fp32 on the CPU."""
    from efficient_attention import _ops
    ab = operands(op, n, dtype)
    if len(ab) == 1:
        res = [_ops.wgrad(ab[0][0], ab[0][1], bias)]
    else:
        (p1, m1), (p2, m2) = _ops.wgrad_pair(ab[0][0], ab[0][1], bias, ab[1][0], ab[1][1], bias)
        s1, s2 = _ops.multi_sum([p1, p2])
        res = [_ops._wgrad_split(s1, m1), _ops._wgrad_split(s2, m2)]
    return [(dw.cpu(), None if db is None else db.cpu()) for dw, db in res]


def key(op, n, dtype, bias):
    return "%s/%s/%s/%d" % (op, dtype, "bias" if bias else "nobias", n)


def run_all():
    return {key(op, n, dt, b): run(op, n, dt, b) for op in OPS for dt in DTYPES for b in (True, False) for n in ROWS_PER_SLICE}


if __name__ == "__main__":        # child process: <package directory> <output file>
    sys.path.insert(0, sys.argv[1])
    import torch
    torch.save(run_all(), sys.argv[2])
