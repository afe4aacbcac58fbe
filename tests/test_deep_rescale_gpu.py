"""The rescaling rule for pileup windows of very deep coverage on the device (csrc/c3_rescale.h; need an MI355X): the *_depth entries and
the region entry on the ring against the same windows rescaled on the host (bit for bit: after the integer step the same kernels see
the same int32 counts), against the rows the reference module gave for the fixture, on the ring, through the range guard's re-run, and
their argument errors."""
import json
import os

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "fp32": {"C3HIP_FP32": "1"}}


def fixture(name="pileup_deep_rescaled"):
    z = np.load(os.path.join(util.GOLDEN, f"{name}.npz"))
    return z, json.loads(str(z["meta"]))


def _env(monkeypatch, env):
    for k in ("C3HIP_FP32", "C3HIP_AUTO_FP32"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)


def _deep(depths, max_depth=144):
    return int(((depths > 0) & (depths > 1.5 * max_depth)).sum())


def _drawn(n, depth, seed):
    """n int32 windows drawn at `depth` with the depths the recipe drew; every fifth window (from the third on) at ordinary coverage, so
    that a batch mixes rescaled and untouched windows"""
    x, d = syn.make_pileup_windows(n, seed=seed, dtype=np.int32, depth=depth, return_depth=True)
    xs, ds = syn.make_pileup_windows(n, seed=seed + 1, dtype=np.int32, depth=60, return_depth=True)
    x[2::5], d[2::5] = xs[2::5], ds[2::5]
    return x, d


# ------------------------------------------------------------------------------------------------ 1: same rows as host rescaling
@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("decode", [False, True])
def test_device_rescaling_equals_host_rescaling(env, decode, monkeypatch):
    _env(monkeypatch, env)
    z, meta = fixture()
    m = make_model(syn.PILEUP, 18, True, syn.make_state_dict(syn.PILEUP, 18, True, seed=meta["weight_seed"]))
    m.decode_columns(decode)
    cases = [("fixture", z["x"], z["depth"])]
    for depth in (500, 3000, 30000):
        for n in (1, 48, 1100):
            x, d = _drawn(n, depth, seed=400 + n)
            cases.append((f"depth {depth} batch {n}", x, d))
    for what, x, d in cases:
        host = syn.rescale_deep_windows(x, d)
        assert (host != x).any() and (len(x) < 3 or _deep(d) < len(x)), what
        want = m.predict_numpy(host)
        got = m.predict_numpy(x, depths=d)
        assert got.shape == (len(x), m.row_size) and np.isfinite(got).all()
        assert np.array_equal(got, want), f"{env} decode={decode} {what}: device-rescaled rows differ from host-rescaled rows"
        assert f"rescaled={_deep(d)}" in m.describe() and "max_depth=144" in m.describe(), m.describe()
        assert ("on_fp32=1" in m.describe()) == (env == "fp32")
        # the unscaled windows really give other rows: the comparison above is not vacuous
        assert not np.array_equal(m.predict_numpy(x), want), what


def test_blocking_call_in_pieces_and_micro_batches():
    """a batch the blocking call cuts into pieces of the ring (>= 2 chunks of 4096), and one forward pass beyond the workspace's micro-batch
    (16384 windows): depths travel with their windows"""
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=431)
    m = make_model(syn.PILEUP, 18, False, sd)
    bx, bd = _drawn(96, 3000, seed=432)
    y96 = m.predict_numpy(syn.rescale_deep_windows(bx, bd))
    n = 16384 + 96 + 37
    reps = -(-n // 96)
    x, d = np.concatenate([bx] * reps)[:n], np.concatenate([bd] * reps)[:n]
    got = m.predict_numpy(x, depths=d)
    assert f"rescaled={_deep(d)}" in m.describe(), m.describe()
    one = m.wait(m.submit(x, slot=1, depths=d))  # one forward pass: two micro-batches
    for i in range(0, n, 96):
        k = min(96, n - i)
        assert np.array_equal(got[i:i + k], y96[:k]) and np.array_equal(one[i:i + k], y96[:k]), f"block at {i}"


def test_max_depth_moves_the_threshold():
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=433)
    m = make_model(syn.PILEUP, 18, False, sd)
    x, d = _drawn(64, 180, seed=434)
    assert _deep(d) == 0 and _deep(d, 89) > 32
    assert np.array_equal(m.predict_numpy(x, depths=d), m.predict_numpy(x)) and "rescaled=0" in m.describe()
    m.set_max_depth(89)
    want = m.predict_numpy(syn.rescale_deep_windows(x, d, max_depth=89))
    assert np.array_equal(m.predict_numpy(x, depths=d), want)
    assert f"max_depth=89 rescaled={_deep(d, 89)}" in m.describe(), m.describe()


def test_taps_see_the_rescaled_input():
    from oracle import oracle
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=435)
    m = make_model(syn.PILEUP, 18, False, sd)
    m.tap("lstm1_out")
    x, d = _drawn(40, 3000, seed=436)
    m.predict_numpy(x, depths=d)
    a = m.tap_fetch("lstm1_out", 0, (40, 33, 256))
    _, dbg = oracle.pileup_forward(sd, syn.rescale_deep_windows(x, d), False, debug=True)
    assert float(np.abs(a - dbg["lstm1_out"]).max()) < 2e-5


# ------------------------------------------------------------------------------------------------ 2: region entry
def _region_case():
    """neighbouring candidates at depths 150, 400 and 3000 whose windows share columns, then a stretch of deep candidates"""
    n_cols = 1200
    region = syn.make_pileup_windows(n_cols // 33 + 1, seed=441, dtype=np.int32, depth=400).reshape(-1, 18)[:n_cols].copy()
    region[40:80] = syn.make_pileup_windows(2, seed=442, dtype=np.int32, depth=3000).reshape(-1, 18)[:40]
    region[300, 1], region[300, 10], region[301, 0] = 217, 217, -217  # a planted pair for depth 248 (125, not 126)
    starts = np.r_[[10, 11, 12, 13, 30, 45, 0, n_cols - 33], np.arange(280, 320), np.arange(100, 1100, 9)].astype(np.int32)
    rng = np.random.default_rng(443)
    depths = rng.choice(np.array([150, 400, 3000, 248, 216, 217, 0], np.int32), size=len(starts)).astype(np.int32)
    depths[:6] = [150, 400, 3000, 150, 3000, 400]
    depths[8:48] = 248
    return region, starts, depths


@pytest.mark.parametrize("env", list(ENVS))
def test_region_entry_rescales_every_window_by_its_own_factor(env, monkeypatch):
    _env(monkeypatch, env)
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=444)
    m = make_model(syn.PILEUP, 18, False, sd)
    region, starts, depths = _region_case()
    windows = np.stack([region[s:s + 33] for s in starts])
    host = syn.rescale_deep_windows(windows, depths)
    assert starts[8] == 280 and depths[8] == 248 and windows[8, 20, 1] == 217 and host[8, 20, 1] == 125  # the planted pair (exact: 126)
    want = m.predict_numpy(host)
    plain = m.predict_numpy(windows)
    assert not np.array_equal(want, plain)
    for reg in (region, region.astype(np.int64)):
        got = m.predict_region(reg, starts, depths)
        assert np.array_equal(got, want), f"{env} {reg.dtype}: region rows with depths differ from the host path"
        assert f"rescaled={_deep(depths)}" in m.describe(), m.describe()
        assert np.array_equal(m.predict_region(reg, starts), plain), f"{env} {reg.dtype}: depths=None must stay today's entry"
        assert "rescaled=0" in m.describe()
    assert np.array_equal(m.predict_numpy(windows, depths=depths), want)
    assert m.predict_region(region, np.zeros(0, np.int32), np.zeros(0, np.int32)).shape == (0, 24)
    with pytest.raises(_lib.C3Error, match="outside"):
        m.predict_region(region, np.array([len(region) - 32], np.int32), np.array([400], np.int32))


# ------------------------------------------------------------------------------------------------ 3: against the reference
@pytest.mark.parametrize("name,indel", [("pileup_deep_rescaled", True), ("pileup_deep_rescaled_noindel", False)])
@pytest.mark.parametrize("env", list(ENVS))
def test_fixture_rows_against_the_reference(name, indel, env, monkeypatch):
    _env(monkeypatch, env)
    z, _ = fixture()
    zy, meta = fixture(name)
    m = make_model(syn.PILEUP, 18, indel, syn.make_state_dict(syn.PILEUP, 18, indel, seed=meta["weight_seed"]))
    y = m.predict_numpy(z["x"], depths=z["depth"])
    y_ref = zy["y_ref"]
    err = float(np.abs(y.astype(np.float64) - y_ref).max())
    print(f"{name} {env}: max |dY| vs the reference = {err:.2e}")
    util.assert_rows_match(y, y_ref, tol=util.PROB_TOL, what=f"{name} {env}")
    for lo, hi in util.HEAD_SLICES[: 4 if indel else 2]:  # no near-tie in the fixture: labels identical on EVERY window
        assert np.array_equal(y[:, lo:hi].argmax(1), y_ref[:, lo:hi].argmax(1)), (name, env, lo)
    # and the region form of the same call: the fixture's windows laid end to end
    yr = m.predict_region(z["x"].reshape(-1, 18), np.arange(len(y), dtype=np.int32) * 33, z["depth"])
    assert np.array_equal(yr, y)


# ------------------------------------------------------------------------------------------------ 4: the ring
def test_ring_batches_with_depths_in_any_wait_order():
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=451)
    m = make_model(syn.PILEUP, 18, False, sd)
    region, starts, rdepths = _region_case()
    xa, da = _drawn(1024, 500, seed=452)
    xb, db = _drawn(300, 30000, seed=453)
    want = [m.predict_numpy(xa, depths=da), m.predict_region(region, starts, rdepths), m.predict_numpy(xb, depths=db),
            m.predict_region(region, starts)]
    assert np.array_equal(want[0], m.predict_numpy(syn.rescale_deep_windows(xa, da)))
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        t = [m.submit(xa, slot=0, depths=da), m.submit_region(region, starts, slot=1, depths=rdepths), m.submit(xb, slot=2, depths=db)]
        got = {}
        for k in order:
            got[k] = m.wait(t[k])
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (order, k)
    # region batches in three slots, with and without depths, int64 too
    t = [m.submit_region(region, starts, slot=2), m.submit_region(region.astype(np.int64), starts, slot=0, depths=rdepths),
         m.submit_region(region, starts, slot=1, depths=rdepths)]
    assert np.array_equal(m.wait(t[1]), want[1]) and np.array_equal(m.wait(t[0]), want[3]) and np.array_equal(m.wait(t[2]), want[1])
    # no window above 216: the plain entry's rows, and the handle says so
    xs, ds = syn.make_pileup_windows(200, seed=454, dtype=np.int32, depth=150, return_depth=True)
    ds = np.minimum(ds, 216)
    y_plain = m.predict_numpy(xs)
    assert np.array_equal(m.wait(m.submit(xs, slot=3, depths=ds)), y_plain)
    assert "rescaled=0" in m.describe(), m.describe()
    assert np.array_equal(m.predict_numpy(xs, depths=ds), y_plain) and "rescaled=0" in m.describe()
    # depths and windows may be reused as soon as submit returns
    x2, d2 = xb.copy(), db.copy()
    tk = m.submit(x2, slot=0, depths=d2)
    x2[:] = 0
    d2[:] = 0
    assert np.array_equal(m.wait(tk), want[2])


# ------------------------------------------------------------------------------------------------ 5: the range guard's re-run
def _overflowing_weights(seed):
    """pileup weights whose fp16 pieces overflow (an LSTM2 recurrent weight beyond 65504 becomes inf as an fp16 piece) while the fp32 forms stay
    finite: the gates it feeds saturate"""
    sd = {k: np.array(v, copy=True) for k, v in syn.make_state_dict(syn.PILEUP, 18, False, seed=seed).items()}
    for name in ("LSTM2.weight_hh_l0", "LSTM2.weight_hh_l0_reverse"):
        sd[name][5, 7] = 1.0e5
        sd[name][200, 3] = -2.0e5
    return sd


def test_guard_rerun_rescales_again_from_the_original_counts(monkeypatch, capfd):
    """c3_predict_wait runs a batch again on the fp32 forms from the slot's staged input when the fp16x3 rows come back non-finite: the
    re-run must see the ORIGINAL counts and rescale them once -- rows equal to C3HIP_FP32=1 rows of the host-rescaled windows, bit for bit,
    for sliced windows and for a region batch"""
    from oracle import oracle
    _env(monkeypatch, "default")
    sd = _overflowing_weights(461)
    x, d = _drawn(200, 3000, seed=462)
    host = syn.rescale_deep_windows(x, d)
    y_o = oracle.pileup_forward(sd, host, False)
    assert np.isfinite(y_o).all(), "the fp64 oracle must stay finite on these weights"
    region, starts, rdepths = _region_case()
    rwin = syn.rescale_deep_windows(np.stack([region[s:s + 33] for s in starts]), rdepths)
    monkeypatch.setenv("C3HIP_FP32", "1")
    m32 = make_model(syn.PILEUP, 18, False, sd)
    want, rwant = m32.predict_numpy(host), m32.predict_numpy(rwin)
    assert np.isfinite(want).all() and np.isfinite(rwant).all()
    monkeypatch.delenv("C3HIP_FP32")
    monkeypatch.setenv("C3HIP_AUTO_FP32", "0")  # (the load-time escalation would start such weights on fp32: keep the fp16x3 kernels)
    capfd.readouterr()
    m = make_model(syn.PILEUP, 18, False, sd)
    assert "precision=fp16x3" in m.describe(), m.describe()
    got = m.predict_numpy(x, depths=d)
    assert "continues on fp32" in capfd.readouterr().err, "the guard did not trip: this test needs weights that overflow the fp16 pieces"
    assert "precision=fp32-range-guard" in m.describe()
    assert np.array_equal(got, want), "the re-run's rows differ from fp32 rows of the host-rescaled windows (rescaled twice, or not at all?)"
    assert np.array_equal(m.predict_numpy(x, depths=d), want)
    # a region batch through the guard: a fresh handle, two batches in flight when the first wait notices
    m2 = make_model(syn.PILEUP, 18, False, sd)
    t0 = m2.submit_region(region, starts, slot=0, depths=rdepths)
    t1 = m2.submit(x, slot=1, depths=d)
    assert np.array_equal(m2.wait(t0), rwant) and np.array_equal(m2.wait(t1), want)
    assert capfd.readouterr().err.count("continues on fp32") == 1
    # ... and the blocking region entry without depths has the guard now
    m3 = make_model(syn.PILEUP, 18, False, sd)
    plain = np.stack([region[s:s + 33] for s in starts])
    assert np.array_equal(m3.predict_region(region, starts), m32.predict_numpy(plain))
    assert "continues on fp32" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------ 6: errors
def test_argument_errors_leave_the_process_alive():
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=471)
    m = make_model(syn.PILEUP, 18, False, sd)
    x, d = _drawn(8, 500, seed=472)
    L = _lib.lib()
    y = np.empty((8, 24), np.float32)
    starts = (np.arange(8) * 33).astype(np.int32)
    # int8 counts: refused, and the message says why
    with pytest.raises(_lib.C3Error, match="int8.*GPU branch.*wrapped"):
        m.predict_numpy(x.astype(np.int8), depths=d)
    with pytest.raises(_lib.C3Error, match="int8"):
        m.submit(x.astype(np.int8), slot=0, depths=d)
    with pytest.raises(_lib.C3Error, match="int8"):
        m.predict_region(x.astype(np.int8).reshape(-1, 18), starts, d)
    with pytest.raises(_lib.C3Error, match="int8"):
        m.submit_region(x.astype(np.int8).reshape(-1, 18), starts, slot=0, depths=d)
    # null depths are not a synonym for the old entries
    assert L.c3_predict_depth(m._handle, x.ctypes.data, _lib.DTYPE_I32, 8, None, y.ctypes.data) != 0 and b"null depths" in L.c3_last_error()
    assert L.c3_predict_submit_depth(m._handle, x.ctypes.data, _lib.DTYPE_I32, 8, None, y.ctypes.data, 0) != 0 and b"null depths" in L.c3_last_error()
    assert L.c3_predict_pileup_region_depth(m._handle, x.ctypes.data, _lib.DTYPE_I32, 8 * 33, starts.ctypes.data, 8, None, y.ctypes.data) != 0
    assert b"null depths" in L.c3_last_error()
    # sizes, max_depth
    assert L.c3_predict_depth(m._handle, x.ctypes.data, _lib.DTYPE_I32, -1, d.ctypes.data, y.ctypes.data) != 0 and b"negative" in L.c3_last_error()
    assert L.c3_predict_pileup_region_depth(m._handle, x.ctypes.data, _lib.DTYPE_I32, -5, starts.ctypes.data, 8, d.ctypes.data, y.ctypes.data) != 0
    assert b"negative" in L.c3_last_error()
    for bad in (0, -144):
        with pytest.raises(_lib.C3Error, match="positive"):
            m.set_max_depth(bad)
    with pytest.raises(_lib.C3Error, match="one entry per window"):
        m.predict_numpy(x, depths=d[:5])
    # a full-alignment handle has no such rule
    mf = make_model(syn.FULL_ALIGNMENT, 8, True, syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=473))
    xf = syn.make_fa_windows(2, seed=474)
    with pytest.raises(_lib.C3Error, match="pileup"):
        mf.predict_numpy(xf, depths=np.array([500, 500], np.int32))
    with pytest.raises(_lib.C3Error, match="pileup"):
        mf.submit(xf, slot=0, depths=np.array([500, 500], np.int32))
    assert L.c3_model_set_max_depth(mf._handle, 144) != 0 and b"pileup" in L.c3_last_error()
    yf = np.empty((2, 90), np.float32)
    assert L.c3_predict_submit_region(mf._handle, xf.ctypes.data, _lib.DTYPE_I32, 66, starts.ctypes.data, 2, d.ctypes.data, yf.ctypes.data, 0) != 0
    # nothing was left in flight and both handles still work
    assert np.array_equal(m.predict_numpy(x, depths=d), m.predict_numpy(syn.rescale_deep_windows(x, d)))
    assert np.isfinite(mf.predict_numpy(xf)).all()
