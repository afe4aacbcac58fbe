"""The transform-waves form of the F(2,3)-along-H convolutions (c3_conv3w.h conv3x3_wino_tw_kernel; needs an MI355X): launches with no
more tiles than the chip has CUs, on a chip the handle has to itself, run one 512-thread workgroup per tile whose waves 4-7 transform
the next slab under the tap loop of waves 0-3.  It computes every value with the paired kernel's instructions in the paired kernel's
order, so rows and planes are compared for EQUALITY with a 305-window pass, where every F(2,3) layer (res3a 292 tiles, res2a / res2b 524,
on 256 CUs) is on the paired form.  The form is selected by the batch size alone: res3a up to 268 windows (256 tiles), res2a / res2b up
to 149 (256 tiles)."""
import numpy as np
import pytest

from clair3_amd import synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model, oracle_mod  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_ALL = 305
SUBS = ((0, 1), (77, 5), (5, 130), (37, 268), (100, 149))  # (first window, windows)
RES2_MAX = 149  # windows up to which res2a / res2b have no more tiles than CUs


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("C3HIP_FP32", "C3HIP_WINO", "C3HIP_KEEP_ACTIVATIONS", "C3HIP_CONV1_FUSED", "C3HIP_SPP_FUSED"):
        monkeypatch.delenv(k, raising=False)


def forms(m):
    """{layer: form} of the F(2,3) layers of the last pass (the wino_form field of describe())"""
    d = m.describe()
    assert "wino_form=" in d, d
    field = d.split("wino_form=")[1].split()[0]
    return dict(item.split(":") for item in field.split("/"))


def run(m, x):
    return m.wait(m.submit(x, slot=0))


@pytest.fixture(scope="module")
def pool8():
    """C = 8 weights and windows, and the rows of all 305 windows in one pass (every F(2,3) layer paired), computed once"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=131)
    x = syn.make_fa_windows(N_ALL, seed=811)
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    y = run(m, x).copy()
    assert forms(m) == {"res2a": "paired", "res2b": "paired", "res3a": "paired"}, m.describe()
    y.setflags(write=False)
    return sd, x, m, y


def test_rows_do_not_depend_on_the_form(pool8):
    sd, x, m, y_all = pool8
    for first, n in SUBS:
        y = run(m, x[first:first + n])
        f = forms(m)
        assert f["res3a"] == "transform-waves", (n, f)
        for layer in ("res2a", "res2b"):
            assert f[layer] == ("transform-waves" if n <= RES2_MAX else "paired"), (n, f)
        assert np.array_equal(y, y_all[first:first + n]), (first, n, float(np.abs(y - y_all[first:first + n]).max()))


def test_first_rows_against_the_oracle(pool8, oracle_mod):  # noqa: F811
    sd, x, m, _ = pool8
    y = run(m, x[:100])
    assert set(forms(m).values()) == {"transform-waves"}, m.describe()
    util.assert_rows_match(y[:24], oracle_mod.fa_forward(sd, x[:24], True), what="transform waves, first 24 rows")


def test_planes_per_layer(pool8):
    """the outputs of res2a, res2b (residual path) and res3a (eight slabs, 256 channels) of 7 windows: alone (transform waves; a full tile
    and ragged ones) and as the first rows of the 305-window pass (paired), word for word"""
    sd, x, _, y_all = pool8
    taps = {"act4": (23, 9, 128), "act5": (23, 9, 128), "act7": (12, 5, 256)}  # res2a, res2b, res3a
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd).tap(tuple(taps))
    y7 = run(m, x[:7])
    assert set(forms(m).values()) == {"transform-waves"}, m.describe()
    alone = {name: m.tap_fetch(name, 0, (7,) + tail) for name, tail in taps.items()}
    y = run(m, x)
    assert set(forms(m).values()) == {"paired"}, m.describe()
    assert np.array_equal(y, y_all) and np.array_equal(y7, y_all[:7])
    for name, tail in taps.items():
        paired = m.tap_fetch(name, 0, (7,) + tail)
        assert np.abs(paired).max() > 0
        assert np.array_equal(alone[name].view(np.uint32), paired.view(np.uint32)), name


def test_the_dwell_network():
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 9, True, seed=132, trained_like=True)
    x = syn.make_fa_windows(N_ALL, seed=812, channels=9)
    m = make_model(syn.FULL_ALIGNMENT, 9, True, sd)
    y_all = run(m, x)
    assert set(forms(m).values()) == {"paired"}, m.describe()
    y9 = run(m, x[:9])
    assert set(forms(m).values()) == {"transform-waves"}, m.describe()
    assert np.array_equal(y9, y_all[:9])


def test_beside_other_handles_the_paired_form_stays(pool8):
    sd, x, m, y_all = pool8
    y = run(m, x[:100])
    assert set(forms(m).values()) == {"transform-waves"}, m.describe()
    try:
        m.sharing(3)
        y3 = run(m, x[:100])
        assert set(forms(m).values()) == {"paired"}, m.describe()
    finally:
        m.sharing(1)
    assert np.array_equal(y3, y) and np.array_equal(y, y_all[:100])
