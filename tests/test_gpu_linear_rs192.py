"""ea_linear_rs192 (ea_linear_rs192.hip): the 192 -> 192 projection with its weight resident in registers, against ea_linear (the
lin_kernel path) on the same operands in the same process: Y must be bit-identical -- the raw 16-bit words compared.

Rows: 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 383, 384, 385 and 32 x CUs + 33 (some workgroups get one step more than others) --
the smallest counts at which a tail tile, a clamped row or a tile boundary can go wrong (tiles of 32 tokens, 16 per wave);
bf16 and fp16; with and without bias; row strides of 192, and of 576 with a column offset (views into a qkv-shaped buffer, whose
other columns must stay untouched); the plain image (W_proj: the output projection) and the transposed one (W_proj^T: its input
gradient).

One case per dtype against the fp64 product of the same rounded operands, in the model-relative bound of the same-operand core
tests (tests/window_reference.py bound_report: a(HIP) <= 4 a(M) + f, and the same for max / max and rms / rms, with M the fp32
product rounded to the element type and f half an ulp of a 16-bit output: 2^-9 for bf16, 2^-12 for fp16)."""
import pytest

EA_E_UNSUPPORTED = -2
ROWS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 383, 384, 385)
_CACHE = {}


def _td(dtype):
    import torch
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def _layer(dtype):
    """(bias fp32 [192], images of prepare_w192_rs) of one random layer per dtype, made once."""
    import torch
    from efficient_attention import _ops
    if dtype not in _CACHE:
        g = torch.Generator(device="cuda").manual_seed(11 if dtype == "bf16" else 12)
        wq = torch.randn(576, 192, device="cuda", generator=g) * 0.05
        wp = torch.randn(192, 192, device="cuda", generator=g) * 0.08
        bias = torch.randn(192, device="cuda", generator=g) * 0.3
        _CACHE[dtype] = (bias, _ops.prepare_w192_rs(wq, wp, _td(dtype)))
    return _CACHE[dtype]


def _rs192(a, image, bias, y, rows, td):
    from efficient_attention import _native as nv
    from efficient_attention import _ops
    nv.call("ea_linear_rs192", _ops._ELEM[td], nv.ptr(a), a.stride(0), nv.ptr(image), nv.ptr(bias), nv.ptr(y), y.stride(0), rows,
            nv.stream())


@pytest.mark.gpu
@pytest.mark.parametrize("image", ["plain", "transposed"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bits_of_ea_linear(dtype, image):
    import torch
    from efficient_attention import _ops
    td = _td(dtype)
    bias, imgs = _layer(dtype)
    assert imgs[5] is not None, "EA_LIN_RS192=0: the images are not made"
    w16, img = (imgs[2], imgs[5]) if image == "plain" else (imgs[3], imgs[6])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cuda").manual_seed(5)
    bad = []
    for rows in ROWS + (32 * cus + 33,):
        for wide in (False, True):
            if wide:
                abuf = (torch.randn(rows, 576, device="cuda", generator=g)).to(td)
                a = abuf[:, 192:384]
                ybuf = torch.full((rows, 576), 3.0, dtype=td, device="cuda")
                y = ybuf[:, 384:576]
            else:
                a = torch.randn(rows, 192, device="cuda", generator=g).to(td)
                ybuf = y = torch.empty(rows, 192, dtype=td, device="cuda")
            for b in (bias, None):
                ref = _ops.ea_linear(a, w16, b, td)[0]
                y.fill_(-7.0)
                _rs192(a, img, b, y, rows, td)
                differ = int((y.contiguous().view(torch.int16) != ref.view(torch.int16)).sum())
                if wide and not bool((ybuf[:, :384] == 3.0).all()):
                    bad.append("rows %d: columns outside the view were written" % rows)
                if differ:
                    bad.append("rows %d ld %d bias %s: %d words differ" % (rows, 576 if wide else 192, b is not None, differ))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_prepared_images_are_w16p_and_its_transpose_in_register_order(dtype):
    """the two new images against tests/rs192_reference.py (held to the documented map by tests/test_linear_rs192_cpu.py); the other five
    are what ea_linear_w192_prepare_t writes"""
    import torch
    import rs192_reference
    from efficient_attention import _ops
    td = _td(dtype)
    g = torch.Generator(device="cuda").manual_seed(21)
    wq = torch.randn(576, 192, device="cuda", generator=g) * 0.05
    wp = torch.randn(192, 192, device="cuda", generator=g) * 0.05
    seven, five = _ops.prepare_w192_rs(wq, wp, td), _ops.prepare_w192_t(wq, wp, td)
    assert len(seven) == 7 and len(five) == 5
    for a, b in zip(seven, five):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(seven[2], wp.to(td)) and torch.equal(seven[3], wp.to(td).t().contiguous())
    assert torch.equal(seven[5].view(torch.int16), rs192_reference.rs192_image(seven[2]).view(torch.int16))
    assert torch.equal(seven[6].view(torch.int16), rs192_reference.rs192_image(seven[3]).view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_against_the_fp64_product_of_the_same_operands(dtype):
    import torch
    import window_reference as wr
    td = _td(dtype)
    bias, imgs = _layer(dtype)
    rows = 385
    g = torch.Generator(device="cuda").manual_seed(6)
    a = torch.randn(rows, 192, device="cuda", generator=g).to(td)
    lines, bad = [], []
    for name, w16, img in (("plain", imgs[2], imgs[5]), ("transposed", imgs[3], imgs[6])):
        y = torch.empty(rows, 192, dtype=td, device="cuda")
        _rs192(a, img, bias, y, rows, td)
        b16 = bias.to(td)
        R = a.double() @ w16.double().t() + b16.double()
        M = (a.float() @ w16.float().t() + b16.float()).to(td)
        ok, txt, _ = wr.bound_report("out", y.cpu(), M.cpu(), R.cpu(), td)
        lines.append("%-10s %s" % (name, txt))
        if not ok:
            bad.append(lines[-1])
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_rows_the_entry_would_refuse_stay_on_ea_linear():
    """a broadcast row (stride 0) passes ea_linear's row test but not the one in front of ea_linear_rs192"""
    import torch
    from efficient_attention import _ops
    td = torch.bfloat16
    row = torch.randn(1, 192, device="cuda").to(td)
    full = torch.randn(64, 192, device="cuda").to(td)
    assert _ops._lin_rows_ok(row.expand(64, 192), td) and not _ops._rs192_rows_ok(row.expand(64, 192), td)
    assert _ops._rs192_rows_ok(full, td) and _ops._rs192_rows_ok(torch.zeros(64, 576, dtype=td, device="cuda")[:, 192:384], td)
    assert not _ops._rs192_rows_ok(full.float(), td) and not _ops._rs192_rows_ok(full[:, :128], td)


@pytest.mark.gpu
def test_arguments_it_cannot_serve_are_refused_before_any_launch():
    import torch
    from efficient_attention import _native as nv
    from efficient_attention import _ops
    td = torch.bfloat16
    bias, imgs = _layer("bf16")
    lib = nv.lib()
    buf = torch.zeros(64 * 200 + 16, dtype=td, device="cuda")
    y = torch.zeros(64, 192, dtype=td, device="cuda")
    e = _ops._ELEM[td]

    def call(a_ptr, lda, y_ptr, ldy, rows):
        return lib.ea_linear_rs192(e, a_ptr, lda, nv.ptr(imgs[5]), None, y_ptr, ldy, rows, None)
    assert call(buf.data_ptr(), 192, y.data_ptr(), 192, 0) == 0                      # EA_OK, nothing to do
    unsupported = EA_E_UNSUPPORTED
    assert call(buf.data_ptr(), 184, y.data_ptr(), 192, 64) == unsupported           # ld below 192
    assert call(buf.data_ptr(), 196, y.data_ptr(), 192, 64) == unsupported           # ld no multiple of 8
    assert call(buf.data_ptr(), 192, y.data_ptr(), 196, 64) == unsupported
    assert call(buf.data_ptr() + 8, 192, y.data_ptr(), 192, 64) == unsupported       # 8-byte alignment
    assert call(buf.data_ptr(), 192, y.data_ptr() + 8, 192, 64) == unsupported
    torch.cuda.synchronize()
    assert not bool(y.any())
