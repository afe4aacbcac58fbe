"""Wave priority between the two workgroups of a CU (clair3_amd/csrc/c3_conv3.h wave_prio_masks, c3_forward.h run_fa_planes; needs an
MI355X).  A scheme only changes which wave the issue arbiter of a SIMD prefers: no arithmetic, no tile shape, no form.  So a handle
created with C3HIP_WAVE_PRIO=0 and one with the default (and one with =1, whatever the default is) give EQUAL rows and planes on the same
weights and windows, at the batch sizes that put every kernel form that takes a scheme to work:
  305 windows  every F(2,3) layer paired, both stride-2 layers in the pair form, res1a / res1b / res3b persistent with several tiles per workgroup
  150 windows  res2a / res2b paired with one tile per workgroup, res3a on transform waves, both stride-2 layers with one workgroup per CU
    5 windows  fewer workgroups than CUs everywhere: no two share a CU
The scheme is on only while the handle has the chip to itself: describe() names the convolutions that ran one in `wave_prio=`, and "-"
under C3HIP_WAVE_PRIO=0 and after sharing(3)."""
import numpy as np
import pytest

from clair3_amd import synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model, oracle_mod  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_ALL = 305
SIZES = (305, 150, 5)
# the convolutions that run a scheme while C3HIP_WAVE_PRIO is on and the handle is alone, per batch size: the stride-1 launches that put two
# workgroups on a CU (c3_forward.h kPrio*; 256 CUs) except res1a -- not the transform-waves form (res3a at 150) and not the stride-2 layers,
# which keep no scheme
NAMED = {305: "res1b/res2a/res2b/res3a/res3b", 150: "res1b/res2a/res2b/res3b", 5: "-"}
ENV = ("C3HIP_WAVE_PRIO", "C3HIP_FP32", "C3HIP_WINO", "C3HIP_KEEP_ACTIVATIONS", "C3HIP_CONV1_FUSED", "C3HIP_SPP_FUSED", "C3HIP_FA_TAIL", "C3HIP_FP32_LAYERS")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def field(m):
    d = m.describe()
    assert " wave_prio=" in d and d.index(" wave_prio=") < d.index(" rows_windows="), d
    return d.split(" wave_prio=")[1].split()[0]


def run(m, x):
    return m.wait(m.submit(x, slot=0))


def handles(monkeypatch, channels, sd, **kw):
    """{switch: handle} on the same weights: off, the default, on (the switch is read when a handle is created)"""
    out = {}
    for name, value in (("off", "0"), ("default", None), ("on", "1")):
        if value is None:
            monkeypatch.delenv("C3HIP_WAVE_PRIO", raising=False)
        else:
            monkeypatch.setenv("C3HIP_WAVE_PRIO", value)
        out[name] = make_model(syn.FULL_ALIGNMENT, channels, True, sd, **kw)
    monkeypatch.delenv("C3HIP_WAVE_PRIO", raising=False)
    return out


@pytest.fixture(scope="module")
def pool8():
    """C = 8 weights and windows, the three handles, and the rows of the 305-window pass with the switch off, computed once"""
    mp = pytest.MonkeyPatch()
    for k in ENV:
        mp.delenv(k, raising=False)
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=141)
    x = syn.make_fa_windows(N_ALL, seed=821)
    ms = handles(mp, 8, sd)
    mp.undo()
    y = run(ms["off"], x).copy()
    y.setflags(write=False)
    return sd, x, ms, y


@pytest.mark.parametrize("n", SIZES)
def test_rows_do_not_depend_on_the_switch(pool8, n):
    sd, x, ms, y_off = pool8
    y0 = y_off if n == N_ALL else run(ms["off"], x[:n])
    for name in ("default", "on"):
        y = run(ms[name], x[:n])
        assert np.array_equal(y, y0), (name, n, float(np.abs(y - y0).max()))
    run(ms["off"], x[:n])
    assert field(ms["on"]) == NAMED[n] and field(ms["off"]) == "-", (n, ms["on"].describe(), ms["off"].describe())
    assert field(ms["default"]) in (NAMED[n], "-"), ms["default"].describe()


def test_first_rows_against_the_oracle(pool8, oracle_mod):  # noqa: F811
    sd, x, ms, _ = pool8
    y = run(ms["on"], x)
    assert field(ms["on"]) == NAMED[N_ALL], ms["on"].describe()
    util.assert_rows_match(y[:8], oracle_mod.fa_forward(sd, x[:8], True), what="wave priority on, first 8 rows of 305")


def test_planes_per_layer(monkeypatch, pool8):
    """the planes of res2a, res2b and res3a of the first 7 windows of the 305-window pass, word for word"""
    sd, x, _, y_off = pool8
    taps = {"act4": (23, 9, 128), "act5": (23, 9, 128), "act7": (12, 5, 256)}
    ms = handles(monkeypatch, 8, sd)
    got = {}
    for name, m in ms.items():
        m.tap(tuple(taps))
        y = run(m, x)
        assert np.array_equal(y, y_off), name
        got[name] = {t: m.tap_fetch(t, 0, (7,) + tail) for t, tail in taps.items()}
    for t in taps:
        assert np.abs(got["off"][t]).max() > 0
        for name in ("default", "on"):
            assert np.array_equal(got[name][t].view(np.uint32), got["off"][t].view(np.uint32)), (name, t)


def test_the_dwell_network(monkeypatch):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 9, True, seed=142, trained_like=True)
    x = syn.make_fa_windows(N_ALL, seed=822, channels=9)
    ms = handles(monkeypatch, 9, sd)
    for n in (N_ALL, 9):
        y0 = run(ms["off"], x[:n])
        for name in ("default", "on"):
            assert np.array_equal(run(ms[name], x[:n]), y0), (name, n)


def test_the_field_follows_switch_and_sharing(pool8):
    sd, x, ms, y_off = pool8
    m = ms["on"]
    y = run(m, x)
    assert field(m) == NAMED[N_ALL], m.describe()
    try:
        m.sharing(3)
        y3 = run(m, x)
        assert field(m) == "-", m.describe()
    finally:
        m.sharing(1)
    assert np.array_equal(y3, y) and np.array_equal(y, y_off)
    run(ms["off"], x)
    assert field(ms["off"]) == "-", ms["off"].describe()
