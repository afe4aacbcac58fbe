"""The one buffer of the three variant instruments on the device (needs an MI355X): jackknife, subsample and occlusion mode stage every
pass of every call in the same buffer of the handle (csrc/c3_variants.h), which is regrown when a call needs more and reused when it needs
less.  Here the modes run one after another on ONE handle, every call cut into three passes of different size, a smaller call behind larger
ones; every array a call returns is compared bitwise with the same call on a fresh handle that runs that mode alone, and the shared handle
must be left as it was.  (What a mode computes is held against a plain handle and the numpy rule by the three modes' own GPU files.)"""
import numpy as np
import pytest

from clair3_amd import synthetic as syn
from tests.test_jackknife import same, same_drops
from tests.test_jackknife_gpu import CASES, forced, make_fa
from tests.test_occlude_gpu import make_p

pytestmark = pytest.mark.gpu

CHUNKS = ("C3HIP_JACKKNIFE_CHUNK", "C3HIP_SUBSAMPLE_CHUNK", "C3HIP_OCCLUDE_CHUNK")
FIGURES = ("on_fp32", "passes", "bytes_staged", "variants", "channels", "bands", "band", "replicates", "seed")


@pytest.fixture(autouse=True)
def passes_of_two_windows(monkeypatch):
    for k in ("C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_PACK_ROWS", "C3HIP_REFINE", "C3HIP_VERIFY", "C3HIP_EXACT", "C3HIP_RANGE_GUARD"):
        monkeypatch.delenv(k, raising=False)
    for k in CHUNKS:
        monkeypatch.setenv(k, "2")


def same_call(a, b):
    """every array of two results of the same call bitwise equal -- records field by field, drops with a NaN for a NaN --, every figure equal"""
    assert a.keys() == b.keys()
    for k, v in a.items():
        if k == "drops":
            assert same_drops(v, b[k]), k
        elif isinstance(v, np.ndarray) and v.dtype.names:
            assert v.dtype == b[k].dtype and all(same(v[f], b[k][f]) for f in v.dtype.names), k
        elif isinstance(v, np.ndarray):
            assert same(v, b[k]), k
        elif k in FIGURES:
            assert v == b[k], (k, v, b[k])
        else:
            assert k in ("expand_us", "reduce_us"), k
    return True


def test_the_three_modes_share_one_buffer_on_a_full_alignment_handle():
    ch, depth, indel, seed = CASES["c8_d55"]
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, indel, seed=seed)
    rows, counts = forced(syn.make_fa_windows(5, seed=seed + 100, channels=ch, depth=depth), [0, 1, 2, 17, 55])
    few = (rows[:int(counts[:2].sum())], counts[:2])
    calls = [
        ("occlude", 3, lambda m: m.occlude_rows(rows, counts, what="both", band=8, drops=True, variant_rows=True)),
        ("jackknife", 3, lambda m: m.jackknife_rows(rows, counts, drops=True, variant_rows=True)),
        ("subsample", 3, lambda m: m.subsample_rows(rows, counts, depths=(1, 4, 16), replicates=2, masks=True, variant_rows=True)),
        ("jackknife", 1, lambda m: m.jackknife_rows(*few, drops=True, variant_rows=True)),  # a smaller need behind larger ones
        ("occlude", 3, lambda m: m.occlude_rows(rows, counts, what="both", band=8, drops=True, variant_rows=True)),
    ]
    shared = make_fa(sd, ch, depth, indel)
    before = (shared.describe(), shared.range_status())
    got = [call(shared) for _, _, call in calls]
    assert (shared.describe(), shared.range_status()) == before, "the handle is left as it was"
    alone = {}  # one fresh handle per mode, which runs that mode alone
    for (mode, passes, call), g in zip(calls, got):
        if mode not in alone:
            alone[mode] = make_fa(sd, ch, depth, indel)
        want = call(alone[mode])
        assert g["passes"] == passes and not g["on_fp32"] and same_call(g, want), mode
    # the calls' sizes differ, so the buffer was grown and then reused: 5 * (8 + 5) occlusion variants, 75 reads, 2 replicates at the levels below
    assert [len(g["variant_rows"]) for g in got] == [65, 75, 2 * (0 + 0 + 1 + 3 + 3), 1, 65]
    assert got[2]["masks"].shape == (14, 2) and got[0]["drops"].shape == (5, 13, 4) and got[1]["drops"].shape == (75, 4)


def test_occlusion_and_predictions_take_turns_on_a_pileup_handle():
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=42)
    x = syn.make_pileup_windows(3, seed=52, dtype=np.int8)
    occlude = lambda m: m.occlude(x, what="both", band=8, drops=True, variant_rows=True)  # noqa: E731
    shared, alone, plain = (make_p(sd) for _ in range(3))
    first = shared.predict_numpy(x)  # (what a description says of the last prediction is there before the mode runs)
    before = (shared.describe(), shared.range_status())
    got = [occlude(shared), shared.predict_numpy(x), occlude(shared), shared.predict_numpy(x)]
    assert (shared.describe(), shared.range_status()) == before, "the handle is left as it was"
    want, y = occlude(alone), plain.predict_numpy(x)
    assert got[0]["passes"] == 2 and same_call(got[0], want) and same_call(got[2], want)
    assert same(first, y) and same(got[1], y) and same(got[3], y) and same(got[0]["base_rows"], y)
    assert len(got[0]["variant_rows"]) == 3 * (18 + 5)
