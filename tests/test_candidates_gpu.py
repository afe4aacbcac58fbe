"""Window selection from candidate positions on the device (csrc/c3_select.h; need an MI355X): statuses and kept count against the fixture
the reference's CreateTensorPileup wrote and against the numpy rule, rows against the entry that already exists -- predict_numpy on the
materialised windows, bit for bit -- and against the fp64 oracle; the ring, the range guard's re-run, empty and refused calls."""
import json
import os

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "fp32": {"C3HIP_FP32": "1"}}
MODES = (("main", False), ("head_tail", True))


def fixture():
    z = np.load(os.path.join(util.GOLDEN, "pileup_candidates.npz"))
    return z, json.loads(str(z["meta"]))


def _env(monkeypatch, env):
    for k in ("C3HIP_FP32", "C3HIP_AUTO_FP32"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)


def _kept(status):
    return np.isin(status, syn.CAND_KEPT)


def _deep(depths, max_depth=144):
    return int(((depths > 0) & (depths > 1.5 * max_depth)).sum())


def _big_region(n_cols=200000, n_chunks=6, n_cand=21000, seed=501, depth=None):
    region, major = syn.make_pileup_region(n_cols, n_chunks, seed=seed, empty_fraction=0.01, depth=depth)
    rng = np.random.default_rng(seed + 2)
    cand = np.unique(rng.integers(major[0] - 30, major[-1] + 30, size=n_cand + n_cand // 8))[:n_cand]
    depths = rng.choice(np.array([40, 150, 216, 217, 400, 3000], np.int32), size=len(cand)).astype(np.int32)
    return region, major, cand, depths


# ------------------------------------------------------------------------------------------------ 1: the fixture
@pytest.mark.parametrize("mode,head_tail", MODES)
def test_fixture_through_predict_candidates(mode, head_tail, monkeypatch):
    from oracle import oracle
    _env(monkeypatch, "default")
    z, _ = fixture()
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=511)
    m = make_model(syn.PILEUP, 18, False, sd)
    cand, depth, windows = z["cand"], z["depth"], z[f"windows_{mode}"]
    want_status, _ = syn.select_pileup_windows(z["matrix"], z["major"], cand, head_tail)
    assert np.array_equal(cand[_kept(want_status)], z[f"kept_{mode}"])
    want = m.predict_numpy(windows)
    want_d = m.predict_numpy(windows, depths=depth[_kept(want_status)])
    assert not np.array_equal(want, want_d), "the fixture holds a rescaled window among the kept"
    y_o = oracle.pileup_forward(sd, windows, False)
    for region in (z["matrix"].astype(np.int32), z["matrix"]):
        rows, status = m.predict_candidates(region, z["major"], cand, head_tail=head_tail)
        assert np.array_equal(status, want_status), f"{mode} {region.dtype}: statuses"
        assert rows.shape == (len(windows), 24), f"{mode}: n_rows {len(rows)} for {len(windows)} kept"
        assert np.array_equal(rows, want), f"{mode} {region.dtype}: rows differ from predict_numpy on the fixture's windows"
        err = util.assert_rows_match(rows, y_o, what=f"candidates {mode} vs oracle")
        print(f"{mode} {region.dtype}: max |dY| vs the oracle = {err:.2e}")
        assert err < 2e-5
        d = m.describe()
        assert f"candidates={len(cand)} kept={len(windows)} chunks=9" in d and "rescaled=0" in d, d
        rows_d, status_d = m.predict_candidates(region, z["major"], cand, depths=depth, head_tail=head_tail)
        assert np.array_equal(status_d, want_status) and np.array_equal(rows_d, want_d), f"{mode} {region.dtype}: with depths"
        assert f"rescaled={_deep(depth[_kept(want_status)])} " in m.describe(), m.describe()


# ------------------------------------------------------------------------------------------------ 2: a large region
@pytest.mark.parametrize("decode", [False, True])
@pytest.mark.parametrize("env", list(ENVS))
def test_large_region_more_than_one_micro_batch(env, decode, monkeypatch):
    _env(monkeypatch, env)
    region, major, cand, depths = _big_region()
    assert len(region) >= 200000 and len(syn.pileup_chunks(major)[0]) >= 5 and len(cand) >= 20000 > 16384
    assert 0.005 < float((region == 0).all(axis=1).mean()) < 0.02
    m = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=521))
    m.decode_columns(decode)
    for head_tail in (False, True):
        want_status, windows = syn.select_pileup_windows(region, major, cand, head_tail)
        n_kept = len(windows)
        assert n_kept > 10000 and (want_status == syn.CAND_EMPTY_COLUMN).sum() > 3000 and (want_status == syn.CAND_NO_WINDOW).any()
        if head_tail:
            assert (want_status == syn.CAND_HEAD).any() and (want_status == syn.CAND_TAIL).any()
        rows, status = m.predict_candidates(region, major, cand, head_tail=head_tail)
        assert np.array_equal(status, want_status) and rows.shape == (n_kept, m.row_size)
        assert np.array_equal(rows, m.predict_numpy(windows)), f"{env} decode={decode} head_tail={head_tail}"
        assert ("on_fp32=1" in m.describe()) == (env == "fp32")
        kd = depths[_kept(want_status)]
        rows, status = m.predict_candidates(region.astype(np.int64), major, cand, depths=depths, head_tail=head_tail)
        assert np.array_equal(status, want_status)
        assert np.array_equal(rows, m.predict_numpy(windows, depths=kd)), f"{env} decode={decode} head_tail={head_tail} with depths"
        assert f"rescaled={_deep(kd)} candidates={len(cand)} kept={n_kept}" in m.describe(), m.describe()


# ------------------------------------------------------------------------------------------------ 3: the ring
def test_ring_candidate_batches_between_other_batches():
    m = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=531))
    z, _ = fixture()
    region, major, cand, depths = _big_region(30000, 5, 1500, seed=532)
    xa = syn.make_pileup_windows(700, seed=533, dtype=np.int32)
    starts = np.arange(0, 20000, 41, dtype=np.int32)
    want = [m.predict_candidates(region, major, cand, head_tail=True), m.predict_candidates(z["matrix"], z["major"], z["cand"], depths=z["depth"]),
            m.predict_candidates(region, major, cand[::3], depths=depths[::3], head_tail=False)]
    want_x, want_r = m.predict_numpy(xa), m.predict_region(region, starts)
    _, w0 = syn.select_pileup_windows(region, major, cand, True)
    assert np.array_equal(want[0][0], m.predict_numpy(w0))
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        t = [m.submit_candidates(region, major, cand, slot=0, head_tail=True),
             m.submit_candidates(z["matrix"], z["major"], z["cand"], slot=1, depths=z["depth"]),
             m.submit_candidates(region, major, cand[::3], slot=2, depths=depths[::3])]
        for k in order:
            rows, status = m.wait(t[k])
            assert np.array_equal(status, want[k][1]) and np.array_equal(rows, want[k][0]), (order, k)
    # interleaved with ordinary window and region batches
    t0 = m.submit_candidates(region, major, cand, slot=0, head_tail=True)
    t1 = m.submit(xa, slot=1)
    t2 = m.submit_candidates(z["matrix"], z["major"], z["cand"], slot=2, depths=z["depth"])
    t3 = m.submit_region(region, starts, slot=3)
    with pytest.raises(_lib.C3Error, match="still in flight"):
        m.submit_candidates(region, major, cand, slot=2)
    assert np.array_equal(m.wait(t1), want_x) and np.array_equal(m.wait(t3), want_r)
    for tk, w in ((t2, want[1]), (t0, want[0])):
        rows, status = m.wait(tk)
        assert np.array_equal(status, w[1]) and np.array_equal(rows, w[0])
    # the inputs may be reused as soon as submit returns
    r2, j2, c2, d2 = region.copy(), major.copy(), cand.copy(), depths.copy()
    tk = m.submit_candidates(r2, j2, c2[::3], slot=1, depths=d2[::3])
    r2[:] = 0
    j2[:] = 0
    c2[:] = 0
    d2[:] = 0
    rows, status = m.wait(tk)
    assert np.array_equal(status, want[2][1]) and np.array_equal(rows, want[2][0])


# ------------------------------------------------------------------------------------------------ 4: the range guard's re-run
def _overflowing_weights(seed):
    """pileup weights whose fp16 pieces overflow (an LSTM2 recurrent weight beyond 65504 becomes inf as an fp16 piece) while the fp32 forms
    stay finite (tests/test_deep_rescale_gpu.py trips the guard the same way)"""
    sd = {k: np.array(v, copy=True) for k, v in syn.make_state_dict(syn.PILEUP, 18, False, seed=seed).items()}
    for name in ("LSTM2.weight_hh_l0", "LSTM2.weight_hh_l0_reverse"):
        sd[name][5, 7] = 1.0e5
        sd[name][200, 3] = -2.0e5
    return sd


def test_guard_rerun_keeps_the_selection(monkeypatch, capfd):
    _env(monkeypatch, "default")
    sd = _overflowing_weights(541)
    region, major, cand, depths = _big_region(30000, 5, 1200, seed=542)
    want_status, windows = syn.select_pileup_windows(region, major, cand, True)
    monkeypatch.setenv("C3HIP_FP32", "1")
    m32 = make_model(syn.PILEUP, 18, False, sd)
    want = m32.predict_numpy(windows, depths=depths[_kept(want_status)])
    assert np.isfinite(want).all()
    monkeypatch.delenv("C3HIP_FP32")
    monkeypatch.setenv("C3HIP_AUTO_FP32", "0")  # (the load-time escalation would start such weights on fp32: keep the fp16x3 kernels)
    capfd.readouterr()
    m = make_model(syn.PILEUP, 18, False, sd)
    assert "precision=fp16x3" in m.describe(), m.describe()
    rows, status = m.predict_candidates(region, major, cand, depths=depths, head_tail=True)
    assert "continues on fp32" in capfd.readouterr().err, "the guard did not trip: this test needs weights that overflow the fp16 pieces"
    assert "precision=fp32-range-guard" in m.describe()
    assert np.array_equal(status, want_status) and np.array_equal(rows, want), "the re-run's rows differ from a handle started on fp32"
    # two batches in flight when the first wait notices
    m2 = make_model(syn.PILEUP, 18, False, sd)
    t0 = m2.submit_candidates(region, major, cand, slot=0, depths=depths, head_tail=True)
    t1 = m2.submit_candidates(region.astype(np.int64), major, cand, slot=1, depths=depths, head_tail=True)
    for tk in (t0, t1):
        rows, status = m2.wait(tk)
        assert np.array_equal(status, want_status) and np.array_equal(rows, want)
    assert capfd.readouterr().err.count("continues on fp32") == 1


# ------------------------------------------------------------------------------------------------ 5: empty calls, refusals, describe
def test_empty_and_all_dropped_calls_and_refusals():
    m = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=551))
    region, major = syn.make_pileup_region(500, 2, seed=552)
    none = np.zeros(0, np.int64)
    rows, status = m.predict_candidates(region, major, none)
    assert rows.shape == (0, 24) and status.shape == (0,) and "candidates=0 kept=0 chunks=2" in m.describe()
    rows, status = m.wait(m.submit_candidates(region, major, none, slot=2, head_tail=True))
    assert rows.shape == (0, 24) and status.shape == (0,)
    # every candidate dropped: outside the region, and in a region too short for a window
    far = np.array([5, major[-1] + 100, major[0] - 1], np.int64)
    for ht in (False, True):
        rows, status = m.predict_candidates(region, major, far, head_tail=ht)
        assert rows.shape == (0, 24) and status.tolist() == [0, 0, 0] and "candidates=3 kept=0" in m.describe()
    short, smajor = region[:20], major[:20]
    rows, status = m.predict_candidates(short, smajor, smajor[[0, 10, 19]])
    assert rows.shape == (0, 24) and status.tolist() == [0, 0, 0]
    rows, status = m.predict_candidates(short, smajor, smajor[[0, 10, 19]], head_tail=True)
    want_status, windows = syn.select_pileup_windows(short, smajor, smajor[[0, 10, 19]], True)
    assert np.array_equal(status, want_status) and np.array_equal(rows, m.predict_numpy(windows))
    rows, status = m.predict_candidates(region[:0], major[:0], far, head_tail=True)
    assert rows.shape == (0, 24) and status.tolist() == [0, 0, 0] and "chunks=0" in m.describe()
    # a region whose every column is empty: every main window is dropped, the forward ran on surplus windows only
    cand = major[40:200:7]
    rows, status = m.predict_candidates(np.zeros_like(region), major, cand)
    want_status, _ = syn.select_pileup_windows(np.zeros_like(region), major, cand)
    assert rows.shape == (0, 24) and np.array_equal(status, want_status) and (status == syn.CAND_EMPTY_COLUMN).any()
    # refusals
    L = _lib.lib()
    with pytest.raises(_lib.C3Error, match="int8"):
        m.predict_candidates(region.astype(np.int8), major, cand)
    with pytest.raises(_lib.C3Error, match="strictly increasing"):
        m.predict_candidates(region, np.r_[major[:-1], major[-2]], cand)
    with pytest.raises(_lib.C3Error, match="one entry per column"):
        m.predict_candidates(region, major[:-1], cand)
    with pytest.raises(_lib.C3Error, match="one entry per window"):
        m.predict_candidates(region, major, cand, depths=np.array([400], np.int32))
    import ctypes as C
    y, st, n = np.empty((len(cand), 24), np.float32), np.empty(len(cand), np.uint8), C.c_int64(-1)
    args = (m._handle, region.ctypes.data, _lib.DTYPE_I32, len(region), major.ctypes.data)
    assert L.c3_predict_pileup_candidates(*args, None, None, len(cand), 0, y.ctypes.data, st.ctypes.data, C.byref(n)) != 0 and b"null buffer" in L.c3_last_error()
    assert L.c3_predict_pileup_candidates(*args, cand.ctypes.data, None, len(cand), 0, y.ctypes.data, None, C.byref(n)) != 0 and b"null buffer" in L.c3_last_error()
    assert L.c3_predict_pileup_candidates(*args, cand.ctypes.data, None, len(cand), 0, y.ctypes.data, st.ctypes.data, None) != 0 and b"null buffer" in L.c3_last_error()
    assert L.c3_predict_pileup_candidates(m._handle, None, _lib.DTYPE_I32, len(region), None, cand.ctypes.data, None, len(cand), 0, y.ctypes.data, st.ctypes.data,
                                          C.byref(n)) != 0 and b"null buffer" in L.c3_last_error()
    assert L.c3_predict_pileup_candidates(*args, cand.ctypes.data, None, -1, 0, y.ctypes.data, st.ctypes.data, C.byref(n)) != 0 and b"negative" in L.c3_last_error()
    assert L.c3_predict_submit_candidates(*args, cand.ctypes.data, None, len(cand), 0, y.ctypes.data, st.ctypes.data, C.byref(n), 9) != 0 and b"slot" in L.c3_last_error()
    mf = make_model(syn.FULL_ALIGNMENT, 8, True, syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=553))
    assert L.c3_predict_pileup_candidates(mf._handle, region.ctypes.data, _lib.DTYPE_I32, len(region), major.ctypes.data, cand.ctypes.data, None, len(cand), 0,
                                          y.ctypes.data, st.ctypes.data, C.byref(n)) != 0 and b"pileup" in L.c3_last_error()
    # nothing was left in flight and the handle still works
    want_status, windows = syn.select_pileup_windows(region, major, cand)
    rows, status = m.predict_candidates(region, major, cand)
    assert np.array_equal(status, want_status) and np.array_equal(rows, m.predict_numpy(windows)) and len(rows) > len(cand) // 2
    assert f"candidates={len(cand)} kept={len(rows)} chunks=2" in m.describe(), m.describe()
