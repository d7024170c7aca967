"""-m "not gpu": ea_lara_layer_plan / ea_eva_layer_plan (ABI 31) lay the composite entries' workspaces out exactly as the numbered
selectors of the two size queries they replace did (ABI 30).  tests/golden/layer_plans.json holds, per configuration, what the
ABI 30 library answered to every selector, and which selector each field of the new structs took over.  Host functions only:
nothing is launched."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "layer_plans.json")))
COUNTS = ("bias_ld", "dbias_part_rows")          # every other field is a size or an offset in floats, 16-byte aligned


@pytest.fixture(scope="module")
def nv():
    from efficient_attention import _native
    if not os.path.exists(os.path.join(ROOT, "efficient-attention_amd", "lib", "libea_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    _native.lib()
    return _native


def _plan(nv, family, cfg):
    """-> (return code, sizes struct) of ea_<family>_layer_plan for one recorded configuration."""
    spec = GOLDEN[family]
    assert [f for f, _ in getattr(nv, "ea_%s_layer" % family)._fields_] == spec["config"]
    c = getattr(nv, "ea_%s_layer" % family)(*cfg)
    out = getattr(nv, "ea_%s_layer_sizes" % family)()
    return getattr(nv.lib(), "ea_%s_layer_plan" % family)(ctypes.byref(c), ctypes.byref(out)), out


def _as_dict(sizes):
    return {f: int(getattr(sizes, f)) for f, _ in sizes._fields_}


def _cases(kind):
    return [(fam, i) for fam in ("lara", "eva") for i in range(len(GOLDEN[fam][kind]))]


@pytest.mark.parametrize("family,i", _cases("accepted"))
def test_every_field_equals_the_recorded_selector(nv, family, i):
    spec, row = GOLDEN[family], GOLDEN[family]["accepted"][i]
    rc, sizes = _plan(nv, family, row["cfg"])
    assert rc == 0
    got = _as_dict(sizes)
    assert set(got) == set(spec["fields"])          # the structs have no field the selectors did not answer
    assert got == {f: row["selectors"][sel] for f, sel in spec["fields"].items()}, row["cfg"]
    assert not [f for f, v in got.items() if f not in COUNTS and v % 4], got


def test_every_recorded_selector_has_a_field_but_the_constant_one():
    """LARA: all twelve; EVA: all thirteen but selector 1, the forward scratch it never had (0 for every configuration)."""
    assert sorted(GOLDEN["lara"]["fields"].values()) == list(range(12))
    assert sorted(GOLDEN["eva"]["fields"].values()) == [0] + list(range(2, 13))
    assert all(row["selectors"][1] == 0 for row in GOLDEN["eva"]["accepted"])


@pytest.mark.parametrize("family,i", _cases("refused"))
def test_refused_configurations_keep_their_codes(nv, family, i):
    row = GOLDEN[family]["refused"][i]
    rc, sizes = _plan(nv, family, row["cfg"])
    assert rc == row["code"] < 0
    assert not any(_as_dict(sizes).values())         # a refused plan writes nothing


def test_lara_fold_switch_changes_no_size(nv, monkeypatch):
    """EA_LARA_FOLD=0 restores the merge launches but must not move the plan: callers memoise it per geometry."""
    row = GOLDEN["lara"]["accepted"][0]
    monkeypatch.delenv("EA_LARA_FOLD", raising=False)
    on = _as_dict(_plan(nv, "lara", row["cfg"])[1])
    monkeypatch.setenv("EA_LARA_FOLD", "0")
    off = _as_dict(_plan(nv, "lara", row["cfg"])[1])
    assert on == off == {f: row["selectors"][sel] for f, sel in GOLDEN["lara"]["fields"].items()}
