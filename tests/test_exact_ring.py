"""The exact form on the submit / wait ring without a device: the new entries in the header and the library, their refusals of a null
handle, the ctypes mirror of c3_verify_extra, the keywords of model.verify / model.answer, and what the environment asks of a model where
it is built (C3HIP_ANSWER, C3HIP_VERIFY_REF, the `replace` word of C3HIP_VERIFY)."""
import ctypes
import inspect
import os
import re

import pytest

from clair3_amd import _lib, predict
from clair3_amd.model import Clair3_F, Clair3_P, _HipModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "c3hip.h")
ENTRIES = ("c3_model_set_answer", "c3_model_set_verify_reference", "c3_model_verify_extra")
ENV = ("C3HIP_VERIFY", "C3HIP_VERIFY_TOL", "C3HIP_VERIFY_LAYERS", "C3HIP_VERIFY_REF", "C3HIP_ANSWER", "C3HIP_EXACT")


def test_the_header_declares_the_entries_and_the_library_exports_them():
    src = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(c3_model \*m, ", src, re.M), f"{name} is not declared in include/c3hip.h"
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    for define in ("C3_ANSWER_PRODUCT 0", "C3_ANSWER_EXACT 1", "C3_VERIFY_REF_FP32 0", "C3_VERIFY_REF_EXACT 1", "C3_VERIFY_REPLACE 2"):
        assert re.search(rf"^#define {define}\b", src, re.M), define
    assert (_lib.VERIFY_REPORT, _lib.VERIFY_ESCALATE, _lib.VERIFY_REPLACE) == (0, 1, 2)
    assert _lib.ANSWER == {"product": 0, "exact": 1} and _lib.VERIFY_REF == {"fp32": 0, "exact": 1}
    # the comment says what is refused and what the device-resident entries keep doing
    comment = src[:src.index("#define C3_ANSWER_PRODUCT")].rsplit("/*", 1)[1]
    for words in ("c3_predict_device and c3_predict_device_checked stay exactly what they are", "Refused unless", "bit-identical", "batches_skipped"):
        assert words in comment, words
    assert _lib.lib().c3_version().decode().startswith("c3hip 0.5.6 ")


def test_the_extra_record_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} c3_verify_extra;", src).group(1)
    ct = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    want = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.strip().split(None, 1)
            want += [(n.strip(), ct[ctype]) for n in names.split(",")]
    assert [(n, t) for n, t in _lib.VerifyExtra._fields_] == want
    assert ctypes.sizeof(_lib.VerifyExtra) == 32
    assert ctypes.sizeof(_lib.VerifyStats) == 168, "c3_verify_stats keeps its size"


def test_null_handles_are_refused_with_a_message():
    L = _lib.lib()
    ex = _lib.VerifyExtra()
    assert L.c3_model_set_answer(None, 1) != 0 and "null model" in _lib.last_error() and "c3_model_set_answer" in _lib.last_error()
    assert L.c3_model_set_verify_reference(None, 1) != 0 and "null model" in _lib.last_error() and "c3_model_set_verify_reference" in _lib.last_error()
    assert L.c3_model_verify_extra(None, ctypes.byref(ex)) != 0 and "null" in _lib.last_error()
    assert L.c3_model_set_verify(None, 1, 1e-4, 1e-6, _lib.VERIFY_REPLACE) != 0 and "null" in _lib.last_error()


def test_verify_signature_keeps_todays_call_and_adds_the_keywords_behind_it():
    base = inspect.signature(_HipModel.verify)
    for cls in (Clair3_P, Clair3_F):  # (the classes a caller builds; the base they share keeps the call it had)
        sig = inspect.signature(cls.verify)
        assert list(sig.parameters) == list(base.parameters) + ["reference", "replace"]
        assert all(sig.parameters[k].default == base.parameters[k].default for k in list(base.parameters)[1:])
        assert sig.parameters["reference"].default == "fp32" and sig.parameters["replace"].default is False
        bound = sig.bind(None, 4, 2e-5, 1e-6, True, False)  # the old positional call
        assert bound.arguments["escalate"] is True and "reference" not in bound.arguments
        sig.bind(None, every=4, tol=1e-4, near_tie=0.0, escalate=False, layers=True)  # ... and the old keyword call
    ok = _HipModel._verify_args
    assert ok(1, 1e-4, 1e-6, False) == (1, 1e-4, 1e-6, _lib.VERIFY_REPORT)
    assert ok(1, 1e-4, 1e-6, True) == (1, 1e-4, 1e-6, _lib.VERIFY_ESCALATE)
    assert ok(2, 1e-4, 1e-6, False, True) == (2, 1e-4, 1e-6, _lib.VERIFY_REPLACE)
    with pytest.raises(_lib.C3Error, match="escalate and replace"):
        ok(1, 1e-4, 1e-6, True, True)
    assert inspect.signature(_HipModel.answer).parameters["form"].default == "exact"


def test_python_refuses_before_any_device_call():
    for cls in (Clair3_P, Clair3_F):
        m = cls(predict=True)
        with pytest.raises(_lib.C3Error, match="escalate and replace"):
            m.verify(escalate=True, replace=True)
        with pytest.raises(_lib.C3Error, match="reference must be"):
            m.verify(reference="fp64")
        with pytest.raises(_lib.C3Error, match="replace must be"):
            m.verify(replace=1)
        with pytest.raises(_lib.C3Error, match="form must be"):
            m.answer("fp32")
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.answer("exact")
        with pytest.raises(_lib.C3Error, match="no device/weights"):
            m.verify_extra()
        assert m._answer == "product" and m._verify_ref == "fp32" and m._verify is None


def test_environment_parsing():
    p = predict.parse_verify_env
    assert p("4,escalate") == dict(every=4, escalate=True), "no new key unless a new word is used"
    assert p("4") == dict(every=4, escalate=False) and p("4,report") == dict(every=4, escalate=False)
    assert p("2,replace") == dict(every=2, escalate=False, replace=True)
    assert p("2, Replace", "1e-5") == dict(every=2, escalate=False, replace=True, tol=1e-5)
    assert p("0,replace") is None
    for bad in ("1,escalate,3", "1,replace,escalate", "1,repair", "replace"):
        with pytest.raises(_lib.C3Error, match="C3HIP_VERIFY"):
            p(bad)
    assert predict.parse_answer_env(None) is None and predict.parse_answer_env(" ") is None
    assert predict.parse_answer_env("exact") == "exact" and predict.parse_answer_env(" Product ") == "product"
    with pytest.raises(_lib.C3Error, match="C3HIP_ANSWER"):
        predict.parse_answer_env("bad")
    assert predict.parse_verify_ref_env("") is None and predict.parse_verify_ref_env("exact") == "exact" and predict.parse_verify_ref_env("FP32") == "fp32"
    with pytest.raises(_lib.C3Error, match="C3HIP_VERIFY_REF"):
        predict.parse_verify_ref_env("bad")


class Stub:
    """records what the environment makes of a model where it is built"""
    _handle = object()

    def __init__(self):
        self.calls, self._exact = [], False

    def verify(self, **kw):
        self.calls.append(("verify", kw))

    def exact(self, enable):
        self.calls.append(("exact", enable))
        self._exact = bool(enable)

    def answer(self, form):
        self.calls.append(("answer", form))


def from_env(m):
    """the three steps in the order _load_torch_checkpoint and build_model take them"""
    predict.verify_from_env(m)
    predict.exact_from_env(m)
    predict.answer_from_env(m)
    return m.calls


def test_environment_reaches_the_model_where_it_is_built(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(predict, "_VERIFIED", [])
    monkeypatch.setattr("atexit.register", lambda fn: None)
    assert from_env(Stub()) == [], "nothing set: the model is left alone"
    monkeypatch.setenv("C3HIP_VERIFY", "8,escalate")
    monkeypatch.setenv("C3HIP_EXACT", "1")
    assert from_env(Stub()) == [("verify", dict(every=8, escalate=True)), ("exact", True)], "today's variables: today's calls"
    monkeypatch.setenv("C3HIP_VERIFY_REF", "fp32")
    assert from_env(Stub()) == [("verify", dict(every=8, escalate=True)), ("exact", True)], "the default reference adds no keyword"
    monkeypatch.delenv("C3HIP_EXACT")
    monkeypatch.setenv("C3HIP_VERIFY", "2,replace")
    monkeypatch.setenv("C3HIP_VERIFY_REF", "exact")
    assert from_env(Stub()) == [("exact", True), ("verify", dict(every=2, escalate=False, replace=True, reference="exact"))], \
        "the exact reference implies the exact form, placed before verify mode asks for it"
    monkeypatch.delenv("C3HIP_VERIFY")
    assert from_env(Stub()) == [], "a reference without verify mode asks for nothing"
    monkeypatch.delenv("C3HIP_VERIFY_REF")
    monkeypatch.setenv("C3HIP_ANSWER", "exact")
    assert from_env(Stub()) == [("exact", True), ("answer", "exact")], "C3HIP_ANSWER=exact implies the exact form, as C3HIP_EXACT=1 does"
    monkeypatch.setenv("C3HIP_ANSWER", "product")
    assert from_env(Stub()) == []
    for name, value in (("C3HIP_ANSWER", "bad"), ("C3HIP_VERIFY_REF", "bad")):
        monkeypatch.setenv("C3HIP_ANSWER", "product")
        monkeypatch.setenv("C3HIP_VERIFY", "1")
        monkeypatch.setenv(name, value)
        with pytest.raises(_lib.C3Error, match=name):
            from_env(Stub())
        monkeypatch.delenv(name)


def test_the_summary_line_ends_on_the_reference_only_when_it_is_exact():
    class M:
        def __init__(self, ref):
            self.ref = ref

        def describe(self):
            return "sharing=1 precision=fp16x3 verify=every:2,policy:replace"

        def verify_stats(self):
            return dict(every=2, policy="replace", tol=1e-4, batches_submitted=4, batches_checked=2, batches_skipped=0, windows_checked=10,
                        max_abs_diff=1e-5, head_max_abs_diff=[1e-5, 0, 0, 0], worst_batch=0, worst_row=3, rows_over_tol=1, label_diffs=[0] * 4,
                        near_ties=[0] * 4, escalations=0)

        def verify_extra(self):
            return dict(reference=self.ref, rows_replaced=3, batches_with_replacements=1, max_abs_diff_f64=1e-5)

    fp32, exact = predict.verify_summary(M("fp32")), predict.verify_summary(M("exact"))
    assert "submitted=4 checked=2 skipped=0 windows=10" in fp32 and fp32.endswith("escalations=0")
    assert exact == fp32 + " ref=exact replaced=3"
