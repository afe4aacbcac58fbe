"""The store policy of what one launch of the product forward pass hands to the next (C3_PLANE_STORE_AUX, clair3_amd/csrc/c3_gemm.h; needs
an MI355X): plane activations, the pooled tensor and the split-K sum of L4 leave write-through.  A cache policy changes no stored bit, so the
rows of 1, 5 and 150 windows are compared for EQUALITY with the rows of the same windows in one 305-window pass.  Together the four batches
take every touched store site in both of its forms: F(2,3) layers as transform waves (1, 5; res3a of 150) and paired (305; res2a / res2b
of 150), the stride-2 layers with one (1, 5, 150) and two (305) workgroups per CU, a partial last tile everywhere.  The first rows of the
long pass go through the suite's own gate against the fp64 oracle."""
import numpy as np
import pytest

from clair3_amd import synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model, oracle_mod  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_ALL = 305
SUBS = ((0, 1), (77, 5), (100, 150))  # (first window, windows)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("C3HIP_FP32", "C3HIP_WINO", "C3HIP_KEEP_ACTIVATIONS", "C3HIP_CONV1_FUSED", "C3HIP_SPP_FUSED"):
        monkeypatch.delenv(k, raising=False)


def run(m, x):
    return m.wait(m.submit(x, slot=0))


@pytest.fixture(scope="module")
def pool8():
    """C = 8 weights and windows, one handle, and the rows of all 305 windows in one pass, computed once"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=141)
    x = syn.make_fa_windows(N_ALL, seed=821)
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    y = run(m, x).copy()
    y.setflags(write=False)
    return sd, x, m, y, m.describe()


def test_describe_names_the_policy(pool8):
    assert " plane_stores=write-through " in pool8[4], pool8[4]
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=142)
    p = make_model(syn.PILEUP, 18, False, sd)
    p.predict_numpy(syn.make_windows(syn.PILEUP, 24, seed=822))
    assert " plane_stores=write-through " in p.describe(), p.describe()


def test_rows_do_not_depend_on_the_batch(pool8):
    sd, x, m, y_all, d_all = pool8
    assert "wino_form=res2a:paired/res2b:paired/res3a:paired" in d_all and "conv3=two-workgroups-per-cu" in d_all, d_all
    for first, n in SUBS:
        y = run(m, x[first:first + n])
        d = m.describe()
        assert "res3a:transform-waves" in d and "conv3=one-workgroup-per-cu" in d, (n, d)
        assert ("res2a:paired/res2b:paired" if n == 150 else "res2a:transform-waves/res2b:transform-waves") in d, (n, d)
        assert np.array_equal(y, y_all[first:first + n]), (first, n, float(np.abs(y - y_all[first:first + n]).max()))


def test_first_rows_against_the_oracle(pool8, oracle_mod):  # noqa: F811
    sd, x, _, y_all, _ = pool8
    util.assert_rows_match(y_all[:8], oracle_mod.fa_forward(sd, x[:8], True), what="write-through plane stores, first 8 rows of 305")
