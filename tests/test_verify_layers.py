"""Layer records of verify mode (c3_model_set_verify_layers, csrc/c3_verify.h), the part that needs no GPU: the entries are declared,
bound and exported, ``verify(layers=...)`` and C3HIP_VERIFY_LAYERS are checked and passed on, the summary lines mark what the suite's
layer gate would, and the ctypes struct is the header's."""
import ctypes
import inspect
import re

import pytest

from clair3_amd import _lib, predict
from clair3_amd.model import Clair3_F, Clair3_P, _HipModel
from tests.test_abi import HEADER, _has_gpu, declared_symbols

ENTRIES = ("c3_model_set_verify_layers", "c3_model_verify_layers")


def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    for value, word in _lib.VERIFY_LAYER_STATUS.items():
        assert f"#define C3_VERIFY_LAYER_{word.upper()} {value}" in src, word


def test_layer_struct_matches_the_header():
    """field for field, in the header's order"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} c3_verify_layer;", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, name = decl.split(None, 1)
        m = re.match(r"(\w+)\[(\d+)\]", name.strip())
        fields.append((m.group(1), ctype, int(m.group(2))) if m else (name.strip(), ctype, 1))
    ct = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "char": ctypes.c_char}
    want = [(n, ct[t] * k if k > 1 else ct[t]) for n, t, k in fields]
    assert [(n, t) for n, t in _lib.VerifyLayer._fields_] == want
    assert ctypes.sizeof(_lib.VerifyLayer) == 80


def test_verify_takes_layers_and_keeps_its_defaults():
    from tests import util
    sig = inspect.signature(_HipModel.verify)
    assert list(sig.parameters) == ["self", "every", "tol", "near_tie", "escalate", "layers"]
    assert sig.parameters["layers"].default is False
    assert sig.parameters["every"].default == 1 and sig.parameters["escalate"].default is False
    assert sig.parameters["tol"].default == util.PROB_TOL and sig.parameters["near_tie"].default == util.NEAR_TIE


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a GPU-less host")
def test_arguments_are_checked_before_the_handle():
    for cls in (Clair3_P, Clair3_F):
        m = cls(predict=True)
        for bad in (1, 0, "yes", None):
            with pytest.raises(_lib.C3Error, match="layers must be True or False"):
                m.verify(layers=bad)
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.verify(layers=True)
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.verify_layers()
        assert m._verify is None and m._verify_layers is False  # a call that failed leaves nothing for a later .to(device)


def test_environment_adds_layers_only_when_set(monkeypatch):
    calls = []

    class Model:
        _handle = object()

        def verify(self, **kw):
            calls.append(kw)

    for k in ("C3HIP_VERIFY", "C3HIP_VERIFY_TOL", "C3HIP_VERIFY_LAYERS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(predict, "_VERIFIED", [])
    monkeypatch.setattr("atexit.register", lambda fn: None)
    monkeypatch.setenv("C3HIP_VERIFY_LAYERS", "1")
    assert predict.verify_from_env(Model()) is False and not calls, "without C3HIP_VERIFY nothing is switched on"
    monkeypatch.setenv("C3HIP_VERIFY", "8,escalate")
    assert predict.verify_from_env(Model()) is True and calls.pop() == dict(every=8, escalate=True, layers=True)
    for off in ("0", "", "off"):
        monkeypatch.setenv("C3HIP_VERIFY_LAYERS", off)
        assert predict.verify_from_env(Model()) is True and calls.pop() == dict(every=8, escalate=True)
    monkeypatch.delenv("C3HIP_VERIFY_LAYERS")
    monkeypatch.setenv("C3HIP_VERIFY_TOL", "2e-5")
    assert predict.verify_from_env(Model()) is True and calls.pop() == dict(every=8, escalate=True, tol=2e-5), "the existing dict, unchanged"
    # the parser itself knows nothing of layers
    assert predict.parse_verify_env("8,escalate", "2e-5") == dict(every=8, escalate=True, tol=2e-5)


def _layer(name, status="compared", d=0.0, ref=1.0, **kw):
    e = dict(name=name, status=status, batches=3, windows=120, worst_batch=2, worst_window=7, worst_index=4242, max_abs_diff=d, ref_max_abs=ref,
             test_max_abs=ref, rel=d / max(1.0, ref))
    e.update(kw)
    return e


def test_summary_lines_mark_layers_beyond_the_suites_gate():
    from tests.test_caller_inputs_gpu import LAYER_TOL
    assert predict.LAYER_TOL == LAYER_TOL == 2e-5
    table = [_layer("act0", "fused", batches=0, windows=0, worst_batch=-1), _layer("act1", d=1e-6, ref=0.5), _layer("act2", d=2e-5, ref=1.0),
             _layer("act3", d=2.1e-5, ref=1.0), _layer("act4", d=2.1e-3, ref=200.0), _layer("spp", d=float("inf"), ref=3.0),
             _layer("l4_out", "none", batches=0, windows=0, worst_batch=-1)]
    lines = predict.verify_layer_lines(table)
    assert len(lines) == len(table) and all(ln.startswith("[clair3_amd] verify layer ") for ln in lines)
    assert [ln.split()[3] for ln in lines] == [e["name"] for e in table], "network order"
    by = dict(zip((e["name"] for e in table), lines))
    assert "fused" in by["act0"] and "batches=" not in by["act0"] and "<<" not in by["act0"]
    assert "no batch" in by["l4_out"]
    assert [name for name, ln in by.items() if ln.endswith(" <<")] == ["act3", "spp"], "rel > LAYER_TOL, and rel is relative to max(1, max |ref|)"
    assert "batches=3 windows=120" in by["act1"] and "worst=(batch 2, window 7, index 4242)" in by["act1"] and "max_abs_diff=1e-06" in by["act1"]
    assert "rel=1.05e-05" in by["act4"]


def test_null_handles_are_errors_not_aborts():
    L = _lib.lib()
    buf = (_lib.VerifyLayer * 2)()
    assert L.c3_model_set_verify_layers(None, 1) != 0 and b"null" in L.c3_last_error()
    assert L.c3_model_verify_layers(None, buf, 2) < 0 and b"null" in L.c3_last_error()
