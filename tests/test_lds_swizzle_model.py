"""-m "not gpu": the chunk swizzle of the 32-token activation tiles of the register-resident projection kernels
(ea_proj_rs.hip, ea_dgrad_rs.hip) in the LDS bank model of MI355X.  tools/lds_bank_model.cpp -- a host program that
includes csrc/ea_lds_swizzle.h, the header the kernels address their tiles with -- prints LDS-array cycles per
wave-instruction for every access those kernels make to such a tile; the layout is checked here, before any GPU time."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "efficient-attention_amd")


def _hipcc():
    spec = importlib.util.spec_from_file_location("ea_build_for_model", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_model") / "lds_bank_model")
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tools", "lds_bank_model.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    print(out)
    res = {}
    for m in re.finditer(r"^(\w+) (\w+) max=(\d+) sum=(\d+) n=(\d+)$", out, flags=re.M):
        res[(m.group(1), m.group(2))] = dict(max=int(m.group(3)), sum=int(m.group(4)), n=int(m.group(5)))
    assert len(res) == 16, out
    return res


def _all(r, cycles):
    """every instruction of the pattern takes exactly `cycles` LDS cycles"""
    return r["max"] == cycles and r["sum"] == cycles * r["n"]


def test_phi2_is_conflicted_for_the_contiguous_k_step(model):
    """Control: under phi2 the 4 (ks & 1) + g row read is 2-way conflicted in every lane group (8 cycles, not 4) -- the
    SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of 0.38 / 0.32 in the two kernels -- while the mapping phi2 was chosen for is clean."""
    assert _all(model[("row_read_4ks_g", "phi2")], 8)
    assert _all(model[("row_read_2g_ks", "phi2")], 4)


def test_psi_is_conflict_free_for_both_row_mappings_tr_reads_and_commit_stores(model):
    assert _all(model[("row_read_4ks_g", "psi")], 4)          # ds_read_b128: 4 lane groups, one cycle each
    assert _all(model[("row_read_2g_ks", "psi")], 4)
    assert _all(model[("tr_read", "psi")], 2)                 # ds_read_b64_tr_b16: 2 groups
    assert _all(model[("commit_store_24", "psi")], 8)         # ds_write_b128: 8 groups of 8 lanes
    assert _all(model[("commit_store_72", "psi")], 8)


def test_psi_is_no_worse_than_phi2_elsewhere(model):
    """the 8-byte read-modify-write of the corrected dq piece and the 16-byte slot-order read of the write-back"""
    for pat in ("rmw_read", "rmw_write", "writeback_read_24"):
        a, b = model[(pat, "psi")], model[(pat, "phi2")]
        assert a["n"] == b["n"] and a["sum"] <= b["sum"] and a["max"] <= b["max"], (pat, a, b)
    assert _all(model[("rmw_read", "psi")], 2)
