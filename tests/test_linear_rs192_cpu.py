"""-m "not gpu": the host side of ea_linear_rs192 (ea_linear_rs192.hip), the 192 -> 192 projection with its weight in registers.

  * The LDS tile of lin_rs192_kernel in the bank model of MI355X (tools/lds_bank_model.cpp rs192, the sibling of
    tests/test_lds_swizzle_model.py): under psi the row-operand reads take 4 cycles per ds_read_b128 and the commit stores 8 per
    ds_write_b128 -- the conflict-free counts; under phi2 the reads would take 8.
  * The weight image is a pure permutation of the weight's 16-byte chunks: tests/rs192_reference.py against the documented
    (pair, j, ks, lane) -> (row, column) map computed here in numpy (tests/test_gpu_linear_rs192.py holds the prepare kernel
    to the same function on the GPU).
  * The two entries are declared, bound with the header's arguments, and refuse what they cannot serve on the host."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "efficient-attention_amd")
HEADER = os.path.join(ROOT, "include", "ea_hip.h")
EA_E_BADARG, EA_E_UNSUPPORTED = -1, -2


def _hipcc():
    spec = importlib.util.spec_from_file_location("ea_build_for_rs192_model", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_model_rs192") / "lds_bank_model")
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tools", "lds_bank_model.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([exe, "rs192"], stdout=subprocess.PIPE, text=True, check=True).stdout
    print(out)
    res = {}
    for m in re.finditer(r"^(\w+) (\w+) max=(\d+) sum=(\d+) n=(\d+)$", out, flags=re.M):
        res[(m.group(1), m.group(2))] = dict(max=int(m.group(3)), sum=int(m.group(4)), n=int(m.group(5)))
    assert len(res) == 4, out
    return res


def _all(r, cycles, n):
    return r["max"] == cycles and r["sum"] == cycles * r["n"] and r["n"] == n


def test_tile_reads_and_commit_stores_are_conflict_free_under_psi(model):
    # reads: 2 token halves x 6 k-steps; stores: one per wave
    assert _all(model[("rs192_row_read", "psi")], 4, 12)          # ds_read_b128: 4 lane groups, one cycle each
    assert _all(model[("rs192_commit_store", "psi")], 8, 12)      # ds_write_b128: 8 groups of 8 lanes
    assert _all(model[("rs192_row_read", "phi2")], 8, 12)         # control: phi2 is 2-way conflicted here


def _expected_image(w):
    """numpy, from the documented map: piece ((pair * 2 + j) * 6 + ks) * 64 + 16 g + li = w[32 pair + 8 (li >> 2) + (li & 3) + 4 j,
    32 ks + 8 g .. + 7]."""
    out = np.empty((6 * 2 * 6 * 64, 8), dtype=w.dtype)
    for pair in range(6):
        for j in range(2):
            for ks in range(6):
                for g in range(4):
                    for li in range(16):
                        row = 32 * pair + 8 * (li >> 2) + (li & 3) + 4 * j
                        out[((pair * 2 + j) * 6 + ks) * 64 + 16 * g + li] = w[row, 32 * ks + 8 * g:32 * ks + 8 * g + 8]
    return out.reshape(-1)


def test_image_is_the_documented_permutation_of_the_weight_bits():
    import torch
    import rs192_reference
    bits = np.arange(192 * 192, dtype=np.uint16).reshape(192, 192)       # every element its own 16-bit pattern
    for td in (torch.bfloat16, torch.float16):
        w16 = torch.from_numpy(bits.view(np.int16).copy()).view(td)
        for w, wb in ((w16, bits), (w16.t().contiguous(), np.ascontiguousarray(bits.T))):
            img = rs192_reference.rs192_image(w).view(torch.int16).numpy().view(np.uint16)
            assert img.shape == (192 * 192,)
            assert np.array_equal(img, _expected_image(wb))
            assert np.array_equal(np.sort(img), np.arange(192 * 192, dtype=np.uint16))      # a permutation: nothing lost or doubled
    # every row of the pair's two MFMA tiles: rows 8 a + b (tile 0) and 8 a + b + 4 (tile 1) of the pair's 32, b < 4
    rows = {32 * p + 8 * (li >> 2) + (li & 3) + 4 * j for p in range(6) for j in range(2) for li in range(16)}
    assert rows == set(range(192))


@pytest.fixture(scope="module")
def nv():
    from efficient_attention import _native
    if not os.path.exists(os.path.join(PKG, "lib", "libea_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    _native.lib()
    return _native


def test_entries_are_declared_and_bound_with_the_headers_arguments(nv):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def declared(name):
        decl = re.search(r"\bint %s\(([^)]*)\);" % name, text).group(1)
        return [" ".join(a.split()) for a in decl.split(",")]
    assert declared("ea_linear_rs192") == ["int32_t dtype", "const void* a", "int64_t lda", "const void* image", "const float* bias",
                                           "void* y", "int64_t ldy", "int32_t rows", "void* stream"]
    prep = declared("ea_linear_w192_prepare_rs")
    assert prep[:-1] == declared("ea_linear_w192_prepare_t")[:-1] + ["void* wp_rs", "void* wpT_rs"] and prep[-1] == "void* stream"
    code = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name in ("ea_linear_rs192", "ea_linear_w192_prepare_rs"):
        assert nv.SIGNATURES[name] == [code.get(a.rsplit(" ", 1)[0], ctypes.c_void_p) for a in declared(name)], name
        assert hasattr(nv.lib(), name)
    assert nv.lib().ea_abi_version() == nv.ABI_VERSION
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ea_linear_rs192" in doc and "ea_linear_w192_prepare_rs" in doc


def test_refusals_on_the_host(nv):
    """never-dereferenced host addresses: every call here returns before any HIP call"""
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    f = nv.lib().ea_linear_rs192

    def call(dtype=0, a=base, lda=192, image=base, bias=None, y=base, ldy=192, rows=64):
        return f(dtype, a, lda, image, bias, y, ldy, rows, None)
    assert call(rows=0) == 0 and call(rows=-3) == 0
    assert call(dtype=7) == EA_E_BADARG
    assert call(a=None) == EA_E_BADARG and call(image=None) == EA_E_BADARG and call(y=None) == EA_E_BADARG
    for over in (dict(a=base + 8), dict(image=base + 8), dict(y=base + 8), dict(bias=base + 4), dict(lda=184), dict(ldy=184),
                 dict(lda=196), dict(ldy=204), dict(rows=(1 << 30) + 1), dict(lda=1 << 20, rows=1 << 20)):
        assert call(**over) == EA_E_UNSUPPORTED, over
    g = nv.lib().ea_linear_w192_prepare_rs
    ptrs = [base] * 9
    for i in range(9):
        for bad in (None, base + 8):
            assert g(0, *(ptrs[:i] + [bad] + ptrs[i + 1:]), None) == EA_E_BADARG, (i, bad)
