"""Full-alignment windows handed over as their occupied read rows, padded on the device (csrc/c3_expand.h; need an MI355X): the rows
entries against the dense entry on the padded windows -- bit for bit, the same kernels see the same int8 windows -- against the rows the
reference module gave for the fixture, on the ring, through the range guard's re-run, under C3HIP_PACK_ROWS=1, with caller buffers at
odd addresses, and their argument errors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn, worker
from tests import util
from tests.test_parity_gpu import make_model

pytestmark = pytest.mark.gpu

SWITCHES = ("C3HIP_FP32", "C3HIP_CONV1_FUSED", "C3HIP_SPP_FUSED", "C3HIP_PACK_ROWS", "C3HIP_AUTO_FP32")
# "decode": the default forms with the decoder columns behind every row
MODES = {"default": {}, "fp32": {"C3HIP_FP32": "1"}, "conv1_unfused": {"C3HIP_CONV1_FUSED": "0"}, "spp_unfused": {"C3HIP_SPP_FUSED": "0"},
         "decode": {}}
SHAPES = {"c8": (8, 89), "c9": (9, 89), "depth55": (8, 55)}
PATTERN = 0x5B


def fixture(name="fa_rows"):
    z = np.load(os.path.join(util.GOLDEN, f"{name}.npz"))
    return z, json.loads(str(z["meta"]))


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_pool = {}


def ragged(n, channels, depth, seed, explicit=False):
    """n windows as rows: counts drawn over 0 .. depth (the first ones 0, 1, depth - 1, depth), rows drawn out of a pool of read rows of
    the realistic recipe.  explicit: also firsts drawn over everything that fits, the first ones touching row 0 and row depth - 1"""
    if channels not in _pool:
        rows = syn.pack_fa_rows(syn.make_fa_windows(24, seed=900 + channels, channels=channels))[0]
        _pool[channels] = rows[(rows != 0).any(axis=(1, 2))]
    pool = _pool[channels]
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, depth + 1, size=n).astype(np.int32)
    forced = [0, 1, depth - 1, depth, 2, depth // 2][:n] if n > 1 else [depth // 3]
    counts[:len(forced)] = forced
    rows = pool[rng.integers(0, len(pool), size=int(counts.sum()))]
    if not explicit:
        return rows, counts, None
    firsts = rng.integers(0, depth - counts + 1).astype(np.int32)
    if n > 6:
        counts_l = counts.tolist()
        firsts[4], firsts[5] = 0, depth - counts_l[5]  # a two-row run at the top, a run that ends on the last row
    return rows, counts, firsts


# ------------------------------------------------------------------------------------------------ 4: rows entry == dense entry on the padded windows
@pytest.mark.parametrize("indel", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", list(MODES))
def test_rows_entry_equals_dense_entry_on_padded_windows(mode, shape, indel, monkeypatch):
    _env(monkeypatch, MODES[mode])
    channels, depth = SHAPES[shape]
    m = make_model(syn.FULL_ALIGNMENT, channels, indel, syn.make_state_dict(syn.FULL_ALIGNMENT, channels, indel, seed=510 + channels), depth=depth)
    m.decode_columns(mode == "decode")
    for n in (1, 7, 256, 2500):  # (2500 crosses the 2048-window micro-batch)
        for explicit in (False, True):
            rows, counts, firsts = ragged(n, channels, depth, seed=520 + n + explicit, explicit=explicit)
            x = syn.pad_fa_rows(rows, counts, firsts, depth=depth)
            want = m.predict_numpy(x)
            got = m.predict_rows(rows, counts, firsts)
            what = f"{mode} {shape} indel={indel} B={n} explicit={explicit}"
            assert got.shape == (n, m.row_size) and got.dtype == np.float32 and np.isfinite(got).all(), what
            assert np.array_equal(got, want), f"{what}: rows differ from the dense entry on the padded windows"
            d = m.describe()
            assert f"rows_windows={n} rows_shipped={len(rows)} pack_rows=0" in d, d
            assert ("on_fp32=1" in d) == (mode == "fp32"), d
            if explicit and n >= 7:  # where the run sits matters: the comparison above is not vacuous
                assert not np.array_equal(m.predict_rows(rows, counts), want), what
    assert m.predict_rows(np.zeros((0, 33, channels), np.int8), np.zeros(0, np.int32)).shape == (0, m.row_size)


# ------------------------------------------------------------------------------------------------ 5: the reference's rows for the fixture
@pytest.mark.parametrize("name", ["fa_rows", "fa_rows_dwell"])
def test_fixture_rows_within_the_golden_gate(name):
    z, meta = fixture(name)
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, meta["channels"], True, seed=meta["weight_seed"])
    m = make_model(syn.FULL_ALIGNMENT, meta["channels"], True, sd)
    y = m.predict_rows(z["rows"], z["counts"])
    y_ref = z["y_ref"]
    err = util.assert_rows_match(y, y_ref, what=name)
    print(f"{name}: max|dY| vs reference = {err:.2e}")
    assert err < 2e-5  # the gate tests/test_parity_gpu.py test_golden_rows applies to the other full-alignment goldens
    gap = min(float(np.diff(np.sort(y_ref[:, lo:hi], axis=1)[:, -2:], axis=1).min()) for lo, hi in util.HEAD_SLICES)
    assert gap >= 1e-5  # (make_golden_fa_rows.py: weights re-drawn until it holds)
    for lo, hi in util.HEAD_SLICES:
        assert np.array_equal(y[:, lo:hi].argmax(1), y_ref[:, lo:hi].argmax(1)), f"{name}: labels of head [{lo}, {hi})"
    assert np.array_equal(y, m.predict_numpy(z["x"]))
    if name == "fa_rows":  # the 55-row set: its rows come from the dense entry on the tensor the reference generator padded
        m55 = make_model(syn.FULL_ALIGNMENT, 8, True, sd, depth=55)
        assert np.array_equal(m55.predict_rows(z["rows55"], z["counts55"]), m55.predict_numpy(z["x55"]))


# ------------------------------------------------------------------------------------------------ 6: the ring, and what it refuses
def test_ring_of_rows_and_dense_batches():
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=531)
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    batches = []
    for i, (n, kind) in enumerate(((96, "rows"), (40, "dense"), (300, "rows"), (17, "explicit"), (600, "dense"), (1, "rows"), (64, "explicit"))):
        rows, counts, firsts = ragged(n, 8, 89, seed=540 + i, explicit=kind == "explicit")
        batches.append((kind, rows, counts, firsts, syn.pad_fa_rows(rows, counts, firsts)))
    blocking = [m.predict_numpy(b[4]) for b in batches]

    def submit(i, slot):
        kind, rows, counts, firsts, x = batches[i]
        return m.submit(x, slot) if kind == "dense" else m.submit_rows(rows, counts, firsts, slot=slot)

    for order in ((2, 0, 1), (1, 2, 0)):
        done = 0
        for i0 in range(0, len(batches), 3):
            idx = list(range(i0, min(i0 + 3, len(batches))))
            tickets = {i: submit(i, i % 3) for i in idx}
            for k in order:
                if i0 + k in tickets:
                    assert np.array_equal(m.wait(tickets[i0 + k]), blocking[i0 + k]), f"batch {i0 + k} ({batches[i0 + k][0]}) waited in order {order}"
                    done += 1
        assert done == len(batches)


def test_rows_entries_refuse_what_they_cannot_run():
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, False, seed=532)
    m = make_model(syn.FULL_ALIGNMENT, 8, False, sd)
    rows, counts, _ = ragged(12, 8, 89, seed=550)
    want = m.predict_rows(rows, counts)
    L = _lib.lib()
    y = np.empty((12, m.row_size), np.float32)

    def refused(match, r=rows, f=None, c=counts, n=12, yy=y, slot=1):
        rc = L.c3_predict_submit_rows(m._handle, None if r is None else r.ctypes.data, None if f is None else f.ctypes.data,
                                      None if c is None else c.ctypes.data, n, None if yy is None else yy.ctypes.data, slot)
        assert rc != 0 and match in _lib.last_error(), (match, _lib.last_error())
        # nothing was queued and the slot is free: the same slot takes the batch at once
        assert np.array_equal(m.wait(m.submit_rows(rows, counts, slot=slot if 0 <= slot < 4 else 1)), want), match

    bad = counts.copy()
    bad[3] = -1
    refused("negative row_count", c=bad)
    bad = counts.copy()
    bad[5] = 90
    refused("beyond the depth", c=bad)
    firsts = ((89 - counts) // 2).astype(np.int32)
    f = firsts.copy()
    f[2] = -1
    refused("negative row_first", f=f)
    f = firsts.copy()
    f[4] = 89 - counts[4] + 1
    refused("beyond the depth", f=f)
    refused("null buffer", r=None)
    refused("null buffer", c=None)
    refused("null buffer", yy=None)
    refused("negative batch", n=-1)
    refused("slot must be", slot=4)
    t = m.submit_rows(rows, counts, slot=2)
    with pytest.raises(_lib.C3Error, match="slot 2 still in flight"):
        m.submit_rows(rows, counts, slot=2)
    assert np.array_equal(m.wait(t), want)
    with pytest.raises(_lib.C3Error, match="counts add up"):
        m.predict_rows(rows[:-1], counts)
    with pytest.raises(_lib.C3Error, match="rows must be"):
        m.predict_rows(rows.astype(np.int32), counts)
    # a pileup handle has no zero rows to restore
    p = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=533))
    yp = np.empty((1, 24), np.float32)
    one = np.ones(1, np.int32)
    assert L.c3_predict_rows(p._handle, rows.ctypes.data, None, one.ctypes.data, 1, yp.ctypes.data) != 0
    assert "pileup" in _lib.last_error()
    x = syn.make_pileup_windows(9, seed=534)
    assert np.isfinite(p.predict_numpy(x)).all()


# ------------------------------------------------------------------------------------------------ 7: the range guard's re-run
def _overflowing_weights():
    """the weight set of tests/test_parity_gpu.py's range-guard tests: a stage at ~1e7 that the fp16 pieces of its readers cannot hold"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=61)
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    for k in ("conv3.conv.weight", "conv3.conv.bias", "conv3.bn.running_mean"):
        sd[k] *= 4.0e6
    for k in ("res_block2.0.conv1.weight", "res_block2.0.conv2.weight"):
        sd[k] /= 2.0e3
    sd["conv5.conv.weight"] /= 4.0e6
    return sd


def test_range_guard_expands_again_from_the_staged_rows(capfd):
    sd = _overflowing_weights()
    rows, counts, firsts = ragged(9, 8, 89, seed=560, explicit=True)
    x = syn.pad_fa_rows(rows, counts, firsts)
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    assert "precision=fp16x3" in m.describe(), m.describe()
    y = m.predict_rows(rows, counts, firsts)
    assert "continues on fp32" in capfd.readouterr().err
    assert "precision=fp32-range-guard" in m.describe() and "on_fp32=1" in m.describe(), m.describe()
    m2 = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    want = m2.predict_numpy(x)  # trips the same way: fp16x3 first, then the re-run on fp32
    assert "continues on fp32" in capfd.readouterr().err and "precision=fp32-range-guard" in m2.describe()
    assert np.isfinite(y).all() and np.array_equal(y, want)
    # two rows batches in flight when the first wait notices: both are expanded and run again
    m3 = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    ta, tb = m3.submit_rows(rows, counts, firsts, slot=0), m3.submit_rows(rows[:counts[0] + counts[1] + counts[2]], counts[:3], firsts[:3], slot=1)
    assert np.array_equal(m3.wait(ta), want) and np.array_equal(m3.wait(tb), want[:3])


# ------------------------------------------------------------------------------------------------ 8: C3HIP_PACK_ROWS=1
def _launches(m):
    return {r["name"]: r["launches"] for r in m.profile_read()}


def test_pack_rows_switch(monkeypatch, tmp_path):
    from tests.test_worker import write_chunk_files
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=571)
    _env(monkeypatch, {})
    plain = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    _env(monkeypatch, {"C3HIP_PACK_ROWS": "1"})
    packed = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    _env(monkeypatch, {})
    assert "pack_rows=0" in plain.describe() and "pack_rows=1" in packed.describe()
    lst, xs = write_chunk_files(tmp_path, [130, 1, 77], kind=syn.FULL_ALIGNMENT, seed=572)
    cases = [syn.make_fa_windows(n, seed=573 + n) for n in (1, 30, 256, 1000)]
    cases += [syn.make_fa_windows(50, seed=574, recipe="uniform"), np.zeros((3, 89, 33, 8), np.int8)]
    odd = syn.make_fa_windows(20, seed=575)
    odd[3, 40:44] = 0  # interior zero rows
    odd[4, :50] = 0    # an off-centre run
    odd[5] = 0
    cases.append(odd)
    for x in cases:
        want = plain.predict_numpy(x)
        d = plain.describe()
        assert "rows_windows=0 rows_shipped=0 pack_rows=0" in d, d
        shipped = len(syn.pack_fa_rows(x)[0])
        assert np.array_equal(packed.predict_numpy(x), want), f"predict_numpy of {len(x)} windows under C3HIP_PACK_ROWS=1"
        d = packed.describe()
        assert f"rows_windows={len(x)} rows_shipped={shipped} pack_rows=1" in d, d
        tickets = [packed.submit(x, slot=s) for s in (2, 0)]
        for t in tickets:
            assert np.array_equal(packed.wait(t), want)
        assert f"rows_windows={len(x)} rows_shipped={shipped} pack_rows=1" in packed.describe()
    got, ref = [], []
    assert worker.predict_file_list(packed, lst, lambda p, a, y: got.append(y), batch_size=64) == 208
    assert worker.predict_file_list(plain, lst, lambda p, a, y: ref.append(y), batch_size=64) == 208
    assert np.array_equal(np.concatenate(got), np.concatenate(ref))
    assert np.array_equal(np.concatenate(ref), plain.predict_numpy(np.concatenate(xs)))
    # the switch unset: a dense batch queues no pre-pass; a rows batch one per micro-batch
    x = syn.make_fa_windows(40, seed=576)
    plain.profile(True)
    plain.profile_reset()
    plain.predict_numpy(x)
    names = _launches(plain)
    assert names and "fa.expand" not in names and "fa.l4" in names, names
    rows, counts, _ = ragged(2500, 8, 89, seed=577)
    plain.profile_reset()
    y = plain.predict_rows(rows, counts)
    names = _launches(plain)
    assert names.get("fa.expand") == 2 and names.get("fa.l4") == 2, names
    plain.profile_reset()
    plain.predict_rows(rows[:int(counts[:40].sum())], counts[:40])
    assert _launches(plain).get("fa.expand") == 1
    plain.profile(False)
    plain.profile_reset()
    assert np.array_equal(plain.predict_rows(rows, counts), y)
    # a pileup handle ignores the switch
    _env(monkeypatch, {"C3HIP_PACK_ROWS": "1"})
    p = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=578))
    _env(monkeypatch, {})
    q = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=578))
    xp = syn.make_pileup_windows(70, seed=579)
    assert np.array_equal(p.predict_numpy(xp), q.predict_numpy(xp))


# ------------------------------------------------------------------------------------------------ 9: buffers the library does not control
@pytest.mark.parametrize("channels", [8, 9])
def test_rows_and_tables_at_odd_host_addresses(channels):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, channels, True, seed=581)
    m = make_model(syn.FULL_ALIGNMENT, channels, True, sd)
    L = _lib.lib()
    for n, explicit in ((5, False), (5, True), (300, True)):
        rows, counts, firsts = ragged(n, channels, 89, seed=582 + n + explicit, explicit=explicit)
        want = m.predict_numpy(syn.pad_fa_rows(rows, counts, firsts))
        for off in (1, 3, 7):
            guard = 64

            def guarded(a):
                buf = np.full(guard + off + a.nbytes + guard, PATTERN, dtype=np.uint8)
                buf[guard + off:guard + off + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
                return buf, buf.ctypes.data + guard + off

            rbuf, rp = guarded(rows)
            cbuf, cp = guarded(counts)
            fbuf, fp = guarded(firsts) if explicit else (None, None)
            ybuf = np.full(16 + n * m.row_size + 16, np.float32(-77.25), dtype=np.float32)
            befores = [b.copy() for b in (rbuf, cbuf) + ((fbuf,) if explicit else ())]
            for entry in ("blocking", "ring"):
                ybuf[:] = np.float32(-77.25)
                yp = ybuf.ctypes.data + 16 * 4
                if entry == "blocking":
                    _lib.check(L.c3_predict_rows(m._handle, rp, fp, cp, n, yp), "c3_predict_rows")
                else:
                    _lib.check(L.c3_predict_submit_rows(m._handle, rp, fp, cp, n, yp, 3), "c3_predict_submit_rows")
                    rbuf[guard + off:guard + off + rows.nbytes] = 0  # (the buffers may be reused as soon as submit returns)
                    cbuf[guard + off:guard + off + counts.nbytes] = 0
                    _lib.check(L.c3_predict_wait(m._handle, 3), "c3_predict_wait")
                    rbuf[:], cbuf[:] = befores[0], befores[1]
                what = f"C={channels} n={n} explicit={explicit} offset {off} {entry}"
                assert np.array_equal(ybuf[16:16 + n * m.row_size].reshape(n, m.row_size), want), what
                assert (ybuf[:16] == np.float32(-77.25)).all() and (ybuf[16 + n * m.row_size:] == np.float32(-77.25)).all(), what
                for b, before in zip((rbuf, cbuf) + ((fbuf,) if explicit else ()), befores):
                    assert np.array_equal(b, before), f"{what}: a caller buffer was written"
