"""The per-layer precision plan (c3_model_set_layer_precision, include/c3hip.h), the part that needs no GPU: the entries are declared,
bound and exported, c3_layer_precision_check accepts exactly the names of the handle's network and names the entry it refuses, and
``layer_precision()`` checks its arguments before anything reaches a handle."""
import ctypes

import pytest

from clair3_amd import _lib
from clair3_amd.model import Clair3_F, Clair3_P, _HipModel
from tests.test_abi import HEADER, _has_gpu, declared_symbols

ENTRIES = ("c3_model_set_layer_precision", "c3_model_layer_precision", "c3_layer_precision_check")
NAMES = {_lib.KIND_PILEUP: ("lstm1", "proj2", "lstm2", "l4"),
         _lib.KIND_FULL_ALIGNMENT: ("conv1", "res1a", "res1b", "conv3", "res2a", "res2b", "conv5", "res3a", "res3b", "l4")}


def check(kind, names):
    """(return code, error text) of c3_layer_precision_check"""
    L = _lib.lib()
    rc = L.c3_layer_precision_check(kind, names if names is None else names.encode())
    return rc, L.c3_last_error().decode()


def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    comment = src[:src.index("int c3_model_set_layer_precision")].rsplit("/*", 1)[1]
    for kind in NAMES:  # the header lists every name of both networks, and the two variables
        for n in NAMES[kind]:
            assert n in comment, n
    assert "C3HIP_FP32_LAYERS" in comment and "C3HIP_AUTO_FP32_LAYERS" in comment and "DESIGN.md 1" in comment


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_valid_plans(kind):
    mine = NAMES[kind]
    for n in mine:
        assert check(kind, n)[0] == 0, n
    assert check(kind, "")[0] == 0
    assert check(kind, "all")[0] == 0
    assert check(kind, ",".join(mine))[0] == 0
    assert check(kind, ",".join(reversed(mine)))[0] == 0  # any order
    assert check(kind, f"{mine[0]},{mine[0]}")[0] == 0 and check(kind, f"{mine[1]},l4,{mine[1]},l4")[0] == 0  # naming a layer twice


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_invalid_plans_name_the_entry(kind):
    mine = NAMES[kind]
    other = NAMES[_lib.KIND_FULL_ALIGNMENT if kind == _lib.KIND_PILEUP else _lib.KIND_PILEUP]
    for bad in ("lstm3", "fa.conv1", "p.lstm2", "ALL", "all", " l4", "l4 ", "act3", "tail"):
        rc, err = check(kind, f"{mine[0]},{bad}")
        assert rc != 0 and f'"{bad}"' in err and "unknown layer" in err, (bad, err)
    for foreign in other:
        if foreign in mine:  # (l4: both networks have one)
            continue
        rc, err = check(kind, foreign)
        assert rc != 0 and f'"{foreign}"' in err, (foreign, err)
        assert ("full-alignment network" if kind == _lib.KIND_PILEUP else "pileup network") in err, err
        assert mine[0] in err  # ... and says which names this network has
    for empty in (f"{mine[2]},,l4", f",{mine[0]}", f"{mine[0]},", ","):
        rc, err = check(kind, empty)
        assert rc != 0 and "empty entry" in err and f'"{empty}"' in err, (empty, err)
    rc, err = check(kind, None)
    assert rc != 0 and "null" in err


def test_the_issue_s_own_example():
    rc, err = check(_lib.KIND_PILEUP, "lstm2,,l4")
    assert rc != 0 and "empty entry" in err and "lstm2,,l4" in err
    rc, err = check(7, "l4")
    assert rc != 0 and "kind 7" in err


def test_python_arguments():
    ok = _HipModel._layer_names
    assert ok("") == "" and ok("all") == "all" and ok("lstm2,l4") == "lstm2,l4" and ok(b"l4") == "l4"
    assert ok(["lstm1", "proj2"]) == "lstm1,proj2" and ok(("l4",)) == "l4" and ok([]) == "" and ok(n for n in ("res2a", "res2b")) == "res2a,res2b"
    for bad in (3, 1.5, ["l4", 3], ["l4", ""], ["lstm1,proj2"], [None], [b"l4"]):
        with pytest.raises(_lib.C3Error, match="layer names"):
            ok(bad)


def test_null_handles_are_errors_not_aborts():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    assert L.c3_model_set_layer_precision(None, b"l4") != 0 and b"null" in L.c3_last_error()
    assert L.c3_model_layer_precision(None, buf, 64) != 0 and b"null" in L.c3_last_error()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a GPU-less host")
def test_fails_loudly_without_a_gpu():
    """a bad name is refused before the missing handle is (the check is plain host code); nothing is left for a later .to(device)"""
    for cls, good, bad in ((Clair3_P, "lstm2", "res2a"), (Clair3_F, ["res2a", "res2b"], "lstm2")):
        m = cls(predict=True)
        with pytest.raises(_lib.C3Error, match=f'"{bad}"'):
            m.layer_precision(bad)
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.layer_precision(good)
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.layer_precision()
        assert m._layer_precision is None
