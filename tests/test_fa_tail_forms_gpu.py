"""The forms of full alignment's FC chain (C3HIP_FA_TAIL, clair3_amd/csrc/c3_tail.h; needs an MI355X): `split` is L4 -> split-K sum -> tail
in three launches, `w4` / `w8` / `w16` run the sum inside fc_tail_sum_kernel<W> (W windows per workgroup), `auto` picks among them by batch
size and by whether the batch has the chip to itself.  The sum's order of additions and every matrix instruction's operands are the same in all of them, so the rows and the `l4_out` tap
are compared for EQUALITY with `split` on the same windows: 1, 3, 4, 5, 17 and 67 windows are one partial group, ragged last groups for
every W (3 | 4: full | 5, 17, 67: 1 or 3 left over) and several groups, with four and two branches and nine input channels.  The first rows
of the longest batch go through the suite's own gate against the fp64 oracle."""
import os

import numpy as np
import pytest

from clair3_amd import synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model, oracle_mod  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 17, 67)
FORMS = {"split": "split", "w4": "fused-w4", "w8": "fused-w8", "w16": "fused-w16"}
CONFIGS = {"c8_indel": (8, True, 0), "c8_plain": (8, False, 10), "c9_indel": (9, True, 20)}  # channels, add_indel_length, seed offset
SWITCHES = ("C3HIP_FA_TAIL", "C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_KEEP_ACTIVATIONS")


def handle(form, ch, indel, sd):
    """a handle on this form: the switch is read when the handle is created"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ["C3HIP_FA_TAIL"] = form
    try:
        return make_model(syn.FULL_ALIGNMENT, ch, indel, sd)
    finally:
        del os.environ["C3HIP_FA_TAIL"]
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def tail_field(d):
    assert " fa_tail=" in d, d
    return d.split(" fa_tail=")[1].split()[0]


@pytest.fixture(scope="module")
def runs():
    """per configuration: weights, windows and, per form and batch size, (rows, l4_out of the first and the last window, fa_tail of
    describe()), computed once"""
    out = {}
    for name, (ch, indel, off) in CONFIGS.items():
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, indel, seed=611 + off)
        x = syn.make_fa_windows(max(SIZES), seed=612 + off, channels=ch)
        res = {}
        for form in tuple(FORMS) + ("auto",):
            m = handle(form, ch, indel, sd).tap("l4_out")
            for n in SIZES:
                y = m.wait(m.submit(x[:n], slot=0)).copy()
                res[form, n] = (y, m.tap_fetch("l4_out", 0, (1, 256)), m.tap_fetch("l4_out", n - 1, (1, 256)), tail_field(m.describe()))
        out[name] = (sd, x, res)
    return out


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_form_gives_the_rows_of_the_three_launches(runs, config):
    sd, x, res = runs[config]
    nout = 90 if CONFIGS[config][1] else 24
    for n in SIZES:
        y0, first0, last0, d0 = res["split", n]
        assert d0 == "split" and y0.shape == (n, nout), (n, d0, y0.shape)
        assert np.isfinite(y0).all() and np.abs(first0).max() > 0 and np.abs(last0).max() > 0
        for form, field in FORMS.items():
            y, first, last, d = res[form, n]
            assert d == field, (config, form, n, d)
            assert np.array_equal(y, y0), (config, form, n, float(np.abs(y - y0).max()))
            assert np.array_equal(first.view(np.uint32), first0.view(np.uint32)), (config, form, n, "l4_out of the first window")
            assert np.array_equal(last.view(np.uint32), last0.view(np.uint32)), (config, form, n, "l4_out of the last window")
        y, first, last, d = res["auto", n]
        assert d in FORMS.values() and np.array_equal(y, y0), (config, n, d)
        assert np.array_equal(first.view(np.uint32), first0.view(np.uint32)) and np.array_equal(last.view(np.uint32), last0.view(np.uint32))
    assert res["auto", 67][3] == "fused-w4", res["auto", 67][3]


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_first_rows_against_the_oracle(runs, config, oracle_mod):  # noqa: F811
    sd, x, res = runs[config]
    y_o = oracle_mod.fa_forward(sd, x[:8], CONFIGS[config][1])
    util.assert_rows_match(res["auto", 67][0][:8], y_o, what=f"{config}: fa_tail=auto, first 8 rows of 67")


def test_decoder_columns_behind_the_rows(runs):
    """rows wider than the probabilities (row > nout): the tail writes with the row's stride, the decoder columns follow in every form"""
    sd, x, _ = runs["c8_indel"]
    ys = {}
    for form in FORMS:
        m = handle(form, 8, True, sd)
        m.decode_columns(True)
        ys[form] = m.wait(m.submit(x[:17], slot=0)).copy()
        assert tail_field(m.describe()) == FORMS[form] and ys[form].shape == (17, m.row_size) and m.row_size > 90
    for form in FORMS:
        assert np.array_equal(ys[form].view(np.uint32), ys["split"].view(np.uint32)), form


def test_auto_keeps_the_three_launches_beside_other_batches(runs):
    """a workgroup of the fused form needs a CU to itself: with the caller's hint that other handles share the chip, or another batch of
    the ring in flight, `auto` stays on the three launches; the rows are the same either way"""
    sd, x, res = runs["c8_indel"]
    m = handle("auto", 8, True, sd)
    m.sharing(3)
    y = m.wait(m.submit(x, slot=0))
    assert tail_field(m.describe()) == "split" and np.array_equal(y, res["split", 67][0])
    m.sharing(1)
    t0, t1 = m.submit(x[:17], slot=0), m.submit(x[:5], slot=1)  # the second one is enqueued while the first is in flight
    y0, y1 = m.wait(t0), m.wait(t1)
    assert tail_field(m.describe()) == "split", m.describe()
    assert np.array_equal(y0, res["split", 17][0]) and np.array_equal(y1, res["split", 5][0])
    y = m.wait(m.submit(x, slot=0))
    assert tail_field(m.describe()) == "fused-w4" and np.array_equal(y, res["split", 67][0])


def test_a_value_that_names_no_form_fails_the_creation():
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=611)
    with pytest.raises(Exception, match="C3HIP_FA_TAIL"):
        handle("w5", 8, True, sd)
