"""Verify mode (c3_model_set_verify, csrc/c3_verify.h), the part that needs no GPU: the entry points are declared, bound and exported, the
arguments of ``verify()`` and of C3HIP_VERIFY / C3HIP_VERIFY_TOL are checked before anything reaches the library, and without a device the
calls fail the way the other entries do."""
import ctypes
import re

import numpy as np
import pytest

from clair3_amd import _lib, predict
from clair3_amd.model import Clair3_F, Clair3_P, _HipModel
from tests.test_abi import HEADER, _has_gpu, declared_symbols

ENTRIES = ("c3_model_set_verify", "c3_model_verify_stats", "c3_model_verify_reset")


def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    assert "#define C3_VERIFY_REPORT 0" in src and "#define C3_VERIFY_ESCALATE 1" in src
    assert (_lib.VERIFY_REPORT, _lib.VERIFY_ESCALATE) == (0, 1)
    # the comment of the entries says what they are for and where the question comes from
    comment = src[:src.index("#define C3_VERIFY_REPORT")].rsplit("/*", 1)[1]
    assert "DESIGN.md 4" in comment and "c3_predict_device" in comment and "never verified" in comment


def test_stats_struct_matches_the_header():
    """field for field, in the header's order: fixed-width integers first, then the floats"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} c3_verify_stats;", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            n = n.strip()
            m = re.match(r"(\w+)\[(\d+)\]", n)
            fields.append((m.group(1), ctype, int(m.group(2))) if m else (n, ctype, 1))
    ct = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    want = [(n, ct[t] * k if k > 1 else ct[t]) for n, t, k in fields]
    assert [(n, t) for n, t in _lib.VerifyStats._fields_] == want
    assert ctypes.sizeof(_lib.VerifyStats) == 168


def test_verify_arguments_are_checked():
    ok = _HipModel._verify_args
    assert ok(1, 1e-4, 1e-6, False) == (1, 1e-4, 1e-6, _lib.VERIFY_REPORT)
    assert ok(16, 0.5, 0.0, True) == (16, 0.5, 0.0, _lib.VERIFY_ESCALATE)
    assert ok(0, 1e-4, 1e-6, False)[0] == 0
    assert ok(np.int64(3), np.float32(1e-3), 0, False)[0] == 3
    for bad in (dict(every=-1), dict(every=1.5), dict(every="2"), dict(every=True), dict(every=2 ** 31), dict(tol=0.0), dict(tol=-1e-4),
                dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=1e-60), dict(tol="x"), dict(near_tie=-1e-9), dict(near_tie=float("nan")),
                dict(near_tie=None)):
        kw = dict(every=1, tol=1e-4, near_tie=1e-6, escalate=False)
        kw.update(bad)
        with pytest.raises(_lib.C3Error):
            ok(**kw)


def test_defaults_are_the_projects_own_gates():
    import inspect
    from tests import util
    sig = inspect.signature(_HipModel.verify)
    assert sig.parameters["every"].default == 1 and sig.parameters["escalate"].default is False
    assert sig.parameters["tol"].default == util.PROB_TOL and sig.parameters["near_tie"].default == util.NEAR_TIE


def test_environment_parsing():
    p = predict.parse_verify_env
    assert p(None) is None and p("") is None and p("  ") is None and p("0") is None and p("0,escalate") is None
    assert p("1") == dict(every=1, escalate=False)
    assert p(" 16 ") == dict(every=16, escalate=False)
    assert p("4,escalate") == dict(every=4, escalate=True)
    assert p("4, Escalate") == dict(every=4, escalate=True)
    assert p("4,report") == dict(every=4, escalate=False)
    assert p("2", "1e-5") == dict(every=2, escalate=False, tol=1e-5)
    assert p("2", "") == dict(every=2, escalate=False)
    for bad in ("x", "1,2", "1,escalate,3", "-1", "1.5", "escalate", ",escalate"):
        with pytest.raises(_lib.C3Error, match="C3HIP_VERIFY"):
            p(bad)
    for bad in ("0", "-1e-4", "tol"):
        with pytest.raises(_lib.C3Error, match="C3HIP_VERIFY_TOL"):
            p("1", bad)


def test_environment_reaches_the_model_where_it_is_built(monkeypatch):
    """verify_from_env: unset = the model is left alone; set = model.verify(...) with what the variables say"""
    calls = []

    class Model:
        _handle = object()

        def verify(self, **kw):
            calls.append(kw)

    monkeypatch.delenv("C3HIP_VERIFY", raising=False)
    monkeypatch.delenv("C3HIP_VERIFY_TOL", raising=False)
    monkeypatch.setattr(predict, "_VERIFIED", [])
    monkeypatch.setattr("atexit.register", lambda fn: None)
    assert predict.verify_from_env(Model()) is False and not calls
    monkeypatch.setenv("C3HIP_VERIFY", "8,escalate")
    monkeypatch.setenv("C3HIP_VERIFY_TOL", "2e-5")
    m = Model()
    assert predict.verify_from_env(m) is True and calls == [dict(every=8, escalate=True, tol=2e-5)]
    assert predict._VERIFIED == [m]
    monkeypatch.setenv("C3HIP_VERIFY", "often")
    with pytest.raises(_lib.C3Error):
        predict.verify_from_env(Model())


def test_null_handles_are_errors_not_aborts():
    L = _lib.lib()
    st = _lib.VerifyStats()
    assert L.c3_model_set_verify(None, 1, 1e-4, 1e-6, 0) != 0 and b"null" in L.c3_last_error()
    assert L.c3_model_verify_stats(None, ctypes.byref(st)) != 0 and b"null" in L.c3_last_error()
    assert L.c3_model_verify_reset(None) != 0 and b"null" in L.c3_last_error()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a GPU-less host")
def test_fails_loudly_without_a_gpu():
    for cls in (Clair3_P, Clair3_F):
        m = cls(predict=True)
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.verify()
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.verify_stats()
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.verify_reset()
        with pytest.raises(_lib.C3Error, match="every"):
            m.verify(every=-2)
        assert m._verify is None  # a call that failed has set nothing that a later .to(device) would apply
        with pytest.raises(_lib.C3Error, match="no HIP device|no CPU"):
            m.to("cuda:0")
