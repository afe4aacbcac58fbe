"""Calibration of the full-alignment channel exponents, the parts that need no device: the entries of the C ABI, the rule
(c3_calibration_rule) against a numpy statement of it, the calibration file and C3HIP_CALIBRATION."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from clair3_amd import _lib, calibrate as cal, predict
from tests import util

NEW = ("c3_model_calibrate", "c3_model_calibrate_reset", "c3_model_calibration_census", "c3_model_calibration_solve",
       "c3_model_set_channel_lowering", "c3_model_set_calibration_origin", "c3_model_channel_exps", "c3_calibration_rule")


def rule_numpy(s, cap_log2):
    """include/c3hip.h c3_calibration_rule, stated in numpy: s[c] = f * 2^e with f in [0.5, 1) is what np.frexp returns"""
    s = np.asarray(s, dtype=np.float64)
    live = s > 0
    d = np.where(live, np.maximum(0, np.frexp(s)[1] - cap_log2), 0)
    d_group = int(np.sort(d[live])[(live.sum() - 1) // 2]) if live.any() else 0
    return np.maximum(d, d_group).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the ABI
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
    assert b"c3hip 0.5." in _lib.lib().c3_version()


def test_null_handles_and_arguments_are_errors():
    L = _lib.lib()
    buf = np.zeros(9 * 256, np.float32)
    low = np.zeros(cal.CHANNELS, np.uint8)
    n = ctypes.c_int64(0)
    for rc in (L.c3_model_calibrate(None, None, _lib.DTYPE_I8, 0, None), L.c3_model_calibrate_reset(None),
               L.c3_model_calibration_census(None, buf.ctypes.data, ctypes.byref(n)), L.c3_model_calibration_solve(None, 10, low.ctypes.data),
               L.c3_model_set_channel_lowering(None, low.ctypes.data), L.c3_model_set_calibration_origin(None, 10, 5),
               L.c3_model_channel_exps(None, None, None)):
        assert rc != 0 and b"null model" in L.c3_last_error()
    s = np.ones(4, np.float32)
    assert L.c3_calibration_rule(None, 4, 10, low.ctypes.data) != 0 and b"null" in L.c3_last_error()
    assert L.c3_calibration_rule(s.ctypes.data, 4, 10, None) != 0 and b"null" in L.c3_last_error()
    assert L.c3_calibration_rule(s.ctypes.data, 0, 10, low.ctypes.data) != 0 and b"at least one channel" in L.c3_last_error()
    for cap in (3, 14, -1):
        assert L.c3_calibration_rule(s.ctypes.data, 4, cap, low.ctypes.data) != 0 and b"cap_log2" in L.c3_last_error()
    for cap in (4, 13):
        assert L.c3_calibration_rule(s.ctypes.data, 4, cap, low.ctypes.data) == 0


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("cap", [4, 10, 13])
def test_rule_matches_its_numpy_statement(cap):
    rng = np.random.default_rng(1000 + cap)
    groups = []
    for n in (1, 2, 3, 64, 128, 256):
        groups.append(np.exp2(rng.uniform(-30, 30, n)).astype(np.float32))                    # random, over sixty powers of two
        g = np.exp2(rng.uniform(0, 24, n)).astype(np.float32)
        g[rng.random(n) < 0.4] = 0.0                                                           # ... with silent channels
        groups.append(g)
        groups.append(np.zeros(n, np.float32))                                                 # all silent
        one = np.zeros(n, np.float32)
        one[rng.integers(n)] = 3.0e7
        groups.append(one)                                                                     # one active channel
        groups.append(np.full(n, 5000.0, np.float32))                                          # all equal
        edge = np.full(n, 1.0, np.float32)
        edge[0] = np.float32(2.0 ** cap)                                                       # exactly the cap: one power of two down
        groups.append(edge)
        below = np.full(n, 1.0, np.float32)
        below[0] = np.nextafter(np.float32(2.0 ** cap), np.float32(0))                         # the largest value that stays
        groups.append(below)
    groups.append(np.array([np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1e-45, 1.0], np.float32))  # the ends of the format, a subnormal
    for s in groups:
        got, want = cal.rule(s, cap), rule_numpy(s, cap)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (s, got, want)
        scaled = np.ldexp(s.astype(np.float64), -got.astype(np.int64))
        assert (scaled < 2.0 ** cap).all(), "what was seen stays below the cap"
    assert cal.rule(np.array([2.0 ** cap, 1.0], np.float32), cap).tolist() == [1, 0]
    assert cal.rule(np.array([0.0, 0.0, 2.0 ** (cap + 5)], np.float32), cap).tolist() == [6, 6, 6], "silent channels follow the group"
    assert cal.rule(np.array([1.0, 2.0, 2.0 ** (cap + 5)], np.float32), cap).tolist() == [0, 0, 6], "one hot channel moves alone"


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan, -1.0])
def test_rule_refuses_values_that_are_no_maximum(bad):
    s = np.ones(8, np.float32)
    s[5] = bad
    with pytest.raises(_lib.C3Error, match="channel 5"):
        cal.rule(s, 10)


def test_the_issues_figures_on_the_oracle():
    """the rule on the fp64 oracle's layer outputs of the suite's out-of-range recipe (tests/test_parity_gpu.py), load-time exponents
    recomputed here: stage 2 of the recipe (group stage1) 116 of 128 channels over the cap, group shift 13, every exponent moved, the
    sample's maximum 3.58e7 -> 1022; the other stages untouched"""
    from clair3_amd import synthetic as syn
    from oracle import oracle
    sd = recipe_state_dict()
    _, d = oracle.fa_forward(sd, syn.make_fa_windows(5, seed=62), True, debug=True)
    census = np.zeros((9, 256))
    for l in range(9):
        a = np.abs(d[f"act{l}"])
        census[l, :a.shape[-1]] = a.reshape(-1, a.shape[-1]).max(0)
    k0 = load_time_exps(sd)
    lowering = np.concatenate([cal.rule(np.ldexp(cal.group_maxima(census)[at:at + n], k0[at:at + n]), 10) for _, at, n, _ in cal.GROUPS])
    s = {g["name"]: g for g in cal.summary(census, k0, lowering)["groups"]}
    assert (s["stage1"]["lowered"], s["stage1"]["shift"]) == (128, 13) and s["stage1"]["max_before"] > 3.5e7 and 1000 < s["stage1"]["max_after"] < 1024
    assert (s["inner1"]["lowered"], s["inner1"]["shift"]) == (128, 3) and s["inner1"]["max_before"] > 16000 and s["inner1"]["max_after"] < 1024
    for name in ("stage0", "inner0", "stage2", "inner2"):
        assert s[name]["lowered"] == 0 and s[name]["max_before"] == s[name]["max_after"] < 32


def recipe_state_dict(hot_channel=None):
    """seed 61 with a stage at ~1e7 behind BatchNorm statistics that do not follow (tests/test_parity_gpu.py); hot_channel: that one channel only"""
    from clair3_amd import synthetic as syn
    sd = {k: np.array(v, copy=True) for k, v in syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=61).items()}
    if hot_channel is None:
        for k in ("conv3.conv.weight", "conv3.conv.bias", "conv3.bn.running_mean"):
            sd[k] *= 4.0e6
        for k in ("res_block2.0.conv1.weight", "res_block2.0.conv2.weight"):
            sd[k] /= 2.0e3
        sd["conv5.conv.weight"] /= 4.0e6
    else:
        c = hot_channel
        for k in ("conv3.conv.weight", "conv3.conv.bias", "conv3.bn.running_mean"):
            sd[k][c] *= 4.0e6
        sd["res_block2.0.conv1.weight"][:, c] /= 4.0e6
        sd["conv5.conv.weight"][:, c] /= 4.0e6
    return sd


def load_time_exps(sd):
    """c3_pack.h fa_channel_exps in numpy: |gamma| + |beta| of a channel's BatchNorm (a stage: the larger of its two) times 2^k0 in [1, 2)"""
    from clair3_amd import synthetic as syn
    out = []
    mag = lambda l: (np.abs(sd[syn.FA_CONV_LAYERS[l][1] + ".weight"].astype(np.float64)) + np.abs(sd[syn.FA_CONV_LAYERS[l][1] + ".bias"].astype(np.float64)))
    for s in range(3):
        for m in (np.maximum(mag(3 * s), mag(3 * s + 2)), mag(3 * s + 1)):
            k = np.zeros(len(m), np.int64)
            ok = (m > 0) & np.isfinite(m)
            k[ok] = np.clip(1 - np.frexp(m[ok])[1], -40, 40)
            out.append(k)
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ the file
def good_file(tmp_path, **over):
    rng = np.random.default_rng(5)
    doc = dict(channels=8, depth=89, cap_log2=10, windows=5, k0=rng.integers(-3, 4, cal.CHANNELS), lowering=rng.integers(0, 14, cal.CHANNELS))
    doc.update(over)
    path = str(tmp_path / "cal.json")
    cal.write_file(path, **doc)
    return path, doc


def test_file_round_trip(tmp_path):
    path, doc = good_file(tmp_path)
    f = cal.read_file(path)
    assert {k: f[k] for k in ("channels", "depth", "cap_log2", "windows")} == dict(channels=8, depth=89, cap_log2=10, windows=5)
    assert f["k0"].dtype == np.int8 and np.array_equal(f["k0"], doc["k0"])
    assert f["lowering"].dtype == np.uint8 and np.array_equal(f["lowering"], doc["lowering"])
    raw = json.load(open(path))
    assert sorted(raw) == sorted(["format", "channels", "depth", "cap_log2", "windows", "k0", "lowering"]) and raw["format"] == cal.FORMAT
    assert len(raw["k0"]) == len(raw["lowering"]) == 896


@pytest.mark.parametrize("change, match", [
    (dict(format="something-else"), "format"), (dict(format=None), "format"), (dict(channels=0), "channels"), (dict(channels="8"), "channels"),
    (dict(depth=-1), "depth"), (dict(cap_log2=14), "cap_log2"), (dict(cap_log2=True), "cap_log2"), (dict(windows=-1), "windows"),
    (dict(k0=[0] * 895), "k0"), (dict(k0=[41] + [0] * 895), "k0"), (dict(k0=None), "k0"), (dict(lowering=[0] * 897), "lowering"),
    (dict(lowering=[-1] + [0] * 895), "lowering"), (dict(lowering=[0.5] + [0] * 895), "lowering"), (dict(lowering=[256] + [0] * 895), "lowering"),
    (dict(k0=[-40] + [0] * 895, lowering=[1] + [0] * 895), "-40")])
def test_file_rejections(tmp_path, change, match):
    path, _ = good_file(tmp_path)
    raw = json.load(open(path))
    raw.update(change)
    if change.get("format", "") is None:
        del raw["format"]
    json.dump(raw, open(path, "w"))
    with pytest.raises(_lib.C3Error, match=match):
        cal.read_file(path)


def test_file_that_is_missing_or_no_json(tmp_path):
    with pytest.raises(_lib.C3Error, match="absent.json"):
        cal.read_file(str(tmp_path / "absent.json"))
    for text in ("", "not json", "[1, 2]"):
        p = tmp_path / "bad.json"
        p.write_text(text)
        with pytest.raises(_lib.C3Error, match="bad.json"):
            cal.read_file(str(p))
    with pytest.raises(_lib.C3Error, match="896"):
        cal.write_file(str(tmp_path / "x.json"), channels=8, depth=89, cap_log2=10, windows=1, k0=np.zeros(896, int), lowering=np.zeros(5, int))
    with pytest.raises(_lib.C3Error, match="896"):
        cal.as_lowering(np.zeros(896, np.float32))


# ------------------------------------------------------------------------------------------------ C3HIP_CALIBRATION
class _Model:
    """what predict.calibration_from_env touches of a model"""

    def __init__(self, kind, sd=None):
        self.KIND, self._pending_sd, self._calibration_file, self.loaded = kind, sd, None, []

    def load_calibration(self, path):
        self.loaded.append(path)


def test_calibration_from_env(tmp_path, monkeypatch):
    monkeypatch.delenv("C3HIP_CALIBRATION", raising=False)
    m = _Model(_lib.KIND_FULL_ALIGNMENT, sd={})
    assert predict.calibration_from_env(m) is False and not m.loaded, "unset: the model is left alone"
    monkeypatch.setenv("C3HIP_CALIBRATION", "  ")
    assert predict.calibration_from_env(m) is False and not m.loaded
    path, _ = good_file(tmp_path)
    monkeypatch.setenv("C3HIP_CALIBRATION", path)
    assert predict.calibration_from_env(m) is True and m.loaded == [path]
    p = _Model(_lib.KIND_PILEUP, sd={})
    assert predict.calibration_from_env(p) is False and not p.loaded, "a pileup model ignores it"
    late = _Model(_lib.KIND_FULL_ALIGNMENT)  # built without a checkpoint: checked now, applied by its first load_state_dict
    assert predict.calibration_from_env(late) is True and not late.loaded and late._calibration_file == path
    monkeypatch.setenv("C3HIP_CALIBRATION", str(tmp_path / "typo.json"))
    with pytest.raises(_lib.C3Error, match="typo.json"):
        predict.calibration_from_env(_Model(_lib.KIND_FULL_ALIGNMENT))
    assert predict.calibration_from_env(_Model(_lib.KIND_PILEUP)) is False


def test_a_model_without_a_device_says_so():
    from clair3_amd.model import Clair3_F
    m = Clair3_F(add_indel_length=True, predict=True)
    for call in (lambda: m.calibrate(np.zeros((1, 89, 33, 8), np.int8)), m.calibration, lambda: m.set_calibration(None), m.calibration_reset,
                 lambda: m.load_calibration("x.json")):
        with pytest.raises(_lib.C3Error, match="no device/weights yet"):
            call()
    with pytest.raises(_lib.C3Error, match="no calibration is set"):
        m.save_calibration("x.json")
