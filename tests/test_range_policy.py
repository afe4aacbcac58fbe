"""The range-guard policy (c3_model_set_range_policy and the entries around it), the parts that need no device: the text of a policy, the
three entries in header, binding and library, null handles, and the line a worker leaves on stderr."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from clair3_amd import _lib, predict
from tests import util

NEW = ("c3_model_set_range_policy", "c3_range_policy_check", "c3_model_range_stats")


@pytest.mark.parametrize("text", ["sticky", "recalibrate", "recalibrate:3", "recalibrate:0", "recalibrate:12"])
def test_policy_texts_that_are_accepted(text):
    assert _lib.lib().c3_range_policy_check(text.encode()) == 0, _lib.last_error()


@pytest.mark.parametrize("text", ["", "stick", "Sticky", "recalibrate:", "recalibrate:-1", "recalibrate:3x", "recalibrate:3 ", " recalibrate", "recalibrate,3",
                                  "recalibrate:+3", "recalibrate:99999999", "sticky:1", "fp32"])
def test_policy_texts_that_are_refused(text):
    L = _lib.lib()
    assert L.c3_range_policy_check(text.encode()) != 0
    err = _lib.last_error()
    assert "sticky" in err and "recalibrate:<n>" in err, err
    assert L.c3_range_policy_check(None) != 0 and "null" in _lib.last_error()


def test_header_binding_and_library_agree_on_the_new_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(util.ROOT, "include", "c3hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(c3_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "neither nm nor llvm-nm at hand"
    dyn = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in dyn.stdout.splitlines() if line.strip()}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    assert re.search(r"#define\s+C3_RANGE_STICKY\s+0\b", header) and re.search(r"#define\s+C3_RANGE_RECALIBRATE\s+1\b", header)
    assert (_lib.RANGE_STICKY, _lib.RANGE_RECALIBRATE) == (0, 1)


def test_the_binding_lays_the_stats_out_as_the_header_does():
    """c3_range_stats: four int64, five int32, 96 characters -- 8-byte aligned, no padding inside"""
    header = open(os.path.join(util.ROOT, "include", "c3hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} c3_range_stats;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            n = n.strip()
            m = re.fullmatch(r"(\w+)\[(\d+)\]", n)
            fields.append((m.group(1), ctype, int(m.group(2))) if m else (n, ctype, 0))
    want = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "char": ctypes.c_char}
    got = _lib.RangeStats._fields_
    assert [f[0] for f in fields] == [g[0] for g in got]
    for (name, ctype, count), (_, bound) in zip(fields, got):
        assert bound == (want[ctype] * count if count else want[ctype]), name
    assert ctypes.sizeof(_lib.RangeStats) == 4 * 8 + 5 * 4 + 96 + 4  # (the tail pads to the int64 alignment)


def test_null_handles_are_errors():
    L = _lib.lib()
    st = _lib.RangeStats()
    for policy in (_lib.RANGE_STICKY, _lib.RANGE_RECALIBRATE):
        assert L.c3_model_set_range_policy(None, policy, 4) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_model_range_stats(None, ctypes.byref(st)) != 0 and b"null model" in L.c3_last_error()


class _Tripped:
    KIND = _lib.KIND_FULL_ALIGNMENT
    _handle = object()

    def __init__(self, **over):
        self.st = dict(trips=2, recalibrations=1, reruns=1, census_windows=256, channels_lowered=256, cap_log2=10, policy="recalibrate",
                       max_recalibrations=4, fell_back="")
        self.st.update(over)

    def range_stats(self):
        return self.st

    def describe(self):
        return "sharing=1 precision=fp16x3 pack_rows=0 range_guard=recalibrate,recalibrations:1"


def test_the_workers_line():
    line = predict.range_guard_summary(_Tripped())
    assert line.startswith("[clair3_amd] range guard: policy=recalibrate:4 precision=fp16x3 trips=2 recalibrations=1 reruns=1 ")
    assert "channels_lowered=256 cap_log2=10 census_windows=256 fell_back=no" in line and "\n" not in line
    assert predict.range_guard_summary(_Tripped(trips=0, recalibrations=0)) is None, "a handle that never tripped says nothing"
    assert "fell_back='census not finite'" in predict.range_guard_summary(_Tripped(fell_back="census not finite"))


def test_range_guard_from_env_only_notes_full_alignment_models(monkeypatch):
    class P(_Tripped):
        KIND = _lib.KIND_PILEUP
    monkeypatch.setattr(predict, "_GUARDED", [object()])  # (not empty: no atexit hook is registered by this test)
    monkeypatch.delenv("C3HIP_RANGE_GUARD", raising=False)
    assert predict.range_guard_from_env(_Tripped()) is False
    monkeypatch.setenv("C3HIP_RANGE_GUARD", "recalibrate")
    assert predict.range_guard_from_env(P()) is False
    m = _Tripped()
    assert predict.range_guard_from_env(m) is True and predict._GUARDED[-1] is m
    assert predict.range_guard_from_env(m) is False and len(predict._GUARDED) == 2, "noted once"
