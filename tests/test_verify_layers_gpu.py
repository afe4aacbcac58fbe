"""Layer records of verify mode on the device (csrc/c3_verify.h layer_compare_kernel; need an MI355X): a verified batch also compares the
output of every layer on the fp16x3 form with the fp32 form's, both from the same staged input.

  1  the record is the truth: recomputed in numpy float32 from the tapped tensors of two more handles (C3HIP_FP32=0 and =1), no tolerance;
  2  beyond the micro-batch cap, and a candidate batch with dropped candidates;
  3  nothing else moves: rows, verify_stats(), describe(), the selection rule;
  4  off means off; user taps, keep mode and profiling are left alone; reload and verify_reset; three slots in flight; the worker command.
Every weight set and window comes from clair3_amd/synthetic.py."""
import numpy as np
import pytest

from clair3_amd import synthetic as syn
from tests.test_parity_gpu import make_model
from tests.test_verify_gpu import _tile, _worker

pytestmark = pytest.mark.gpu

FA_LAYERS = [f"act{i}" for i in range(9)] + ["spp", "l4_out"]
P_LAYERS = ["lstm1_out", "gx2", "lstm2_out", "l4_out"]
ENV = ("C3HIP_FP32", "C3HIP_AUTO_FP32", "C3HIP_VERIFY", "C3HIP_VERIFY_TOL", "C3HIP_VERIFY_LAYERS", "C3HIP_KEEP_ACTIVATIONS", "C3HIP_PACK_ROWS",
       "C3HIP_CONV1_FUSED", "C3HIP_SPP_FUSED")


def _model(monkeypatch, kind, ch, indel, sd, fp32=None, env=None, **kw):
    """a handle created under C3HIP_FP32=<fp32> (None: the library's own decision) and the switches of ``env``"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if fp32 is not None:
        monkeypatch.setenv("C3HIP_FP32", str(fp32))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    m = make_model(kind, ch, indel, sd, **kw)
    for k in env or {}:
        monkeypatch.delenv(k)
    return m


def _three_handles(monkeypatch, kind, ch, indel, sd, **kw):
    """(the handle under verify, forced to the fp16x3 kernels; a plain fp16x3 handle; a handle on the fp32 forms): same weights"""
    return (_model(monkeypatch, kind, ch, indel, sd, fp32=0, **kw), _model(monkeypatch, kind, ch, indel, sd, fp32=0, **kw),
            _model(monkeypatch, kind, ch, indel, sd, fp32=1, **kw))


def layer_shapes(kind, depth=syn.FA_DEPTH_ONT):
    """per-window shape of every layer in network order, as c3_debug_tap_fetch lays it out"""
    if kind == syn.PILEUP:
        return {"lstm1_out": (33, 256), "gx2": (33, 1280), "lstm2_out": (33, 320), "l4_out": (128,)}
    shapes, h, w = {}, depth, 33
    for i, (stride, cout) in enumerate(zip((2, 1, 1, 2, 1, 1, 2, 1, 1), (64, 64, 64, 128, 128, 128, 256, 256, 256))):
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
        shapes[f"act{i}"] = (h, w, cout)
    shapes["spp"], shapes["l4_out"] = (14, 256), (256,)
    return shapes


def np_layer(a, b):
    """what the device reports for a layer's tensor a (fp16x3 form) against b (fp32 form), both (windows, ...) float32"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    d = np.abs(a - b)
    assert d.dtype == np.float32 and d.size
    k, pw = int(d.argmax()), d[0].size  # the first maximum in C order: the lowest (window, index)
    return dict(max_abs_diff=np.float32(d.max()), ref_max_abs=np.float32(np.abs(b).max()), test_max_abs=np.float32(np.abs(a).max()),
                worst_window=k // pw, worst_index=k % pw, windows=len(a))


def assert_layer(e, rec, what, batches=1, worst_batch=0):
    print(f"{what} {e['name']}: device max_abs_diff {e['max_abs_diff']:.3e} ref {e['ref_max_abs']:.4g} test {e['test_max_abs']:.4g} rel {e['rel']:.2e} "
          f"worst (window {e['worst_window']}, index {e['worst_index']}) windows {e['windows']}")
    assert e["status"] == "compared", (what, e)
    for key in ("max_abs_diff", "ref_max_abs", "test_max_abs"):  # floats as floats
        assert np.float32(e[key]) == rec[key], (what, e["name"], key, e[key], rec[key])
    for key in ("worst_window", "worst_index", "windows"):  # integers as integers
        assert e[key] == rec[key], (what, e["name"], key, e[key], rec[key])
    assert (e["batches"], e["worst_batch"]) == (batches, worst_batch), (what, e)
    assert rec["ref_max_abs"] > 0, (what, e["name"], "a layer of zeros")
    assert np.float32(e["rel"]) == np.float32(rec["max_abs_diff"] / max(np.float32(1), rec["ref_max_abs"]))


def _tapped(m, call, names, shapes, n, chunk=1024):
    """the first n windows of every tensor of ``names`` of call(m), fetched in chunks of at most ``chunk`` windows"""
    m.tap(names)
    call(m)
    out = {k: np.concatenate([m.tap_fetch(k, i, (min(chunk, n - i),) + shapes[k]) for i in range(0, n, chunk)]) for k in names}
    m.tap("")
    return out


def _check_truth(what, handles, call, kind, n, fused=(), depth=syn.FA_DEPTH_ONT):
    """call(model) -> rows; n: the windows that count.  Every layer's record against numpy; returns the device's table"""
    mv, m16, m32 = handles
    shapes = layer_shapes(kind, depth)
    names = list(shapes)
    mv.verify(every=1, layers=True)
    mv.verify_reset()
    y = call(mv)
    table = mv.verify_layers()
    assert [e["name"] for e in table] == names
    assert [e["name"] for e in table if e["status"] == "fused"] == list(fused), (what, [(e["name"], e["status"]) for e in table])
    compared = [k for k in names if k not in fused]
    a, b = _tapped(m16, call, compared, shapes, n), _tapped(m32, call, compared, shapes, n)
    assert "on_fp32=0" in m16.describe() and "on_fp32=1" in m32.describe()
    for e in table:
        if e["name"] in fused:
            assert (e["batches"], e["windows"], e["max_abs_diff"], e["worst_batch"]) == (0, 0, 0.0, -1), e
        else:
            assert_layer(e, np_layer(a[e["name"]], b[e["name"]]), what)
    assert any(e["max_abs_diff"] > 0 for e in table), f"{what}: the two forms agree to the bit in every layer"
    st = mv.verify_stats()
    assert st["batches_checked"] == 1 and st["windows_checked"] == n, st
    return y, table


# ------------------------------------------------------------------------------------------------ 1: the record is the truth
@pytest.mark.parametrize("batch", [1, 37, 65])
def test_record_pileup_int8(batch, monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=811)
    x = syn.make_pileup_windows(batch, seed=812)
    _check_truth(f"pileup int8 B={batch}", _three_handles(monkeypatch, syn.PILEUP, 18, False, sd), lambda m: m.predict_numpy(x), syn.PILEUP, batch)


def test_record_pileup_int32_region_with_depths(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=813)
    region, _ = syn.make_pileup_region(2000, seed=814, depth=300)
    rng = np.random.default_rng(815)
    starts = rng.integers(0, len(region) - 33, size=37).astype(np.int32)
    depths = rng.choice(np.array([40, 217, 400, 3000], np.int32), size=37).astype(np.int32)
    assert int((depths > 216).sum()) > 5
    _check_truth("pileup region int32", _three_handles(monkeypatch, syn.PILEUP, 18, True, sd),
                 lambda m: m.predict_region(region, starts, depths=depths), syn.PILEUP, 37)


@pytest.mark.parametrize("ch,batch", [(8, 1), (8, 5), (9, 3)])
def test_record_full_alignment(ch, batch, monkeypatch):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=821)
    x = syn.make_fa_windows(batch, seed=822, channels=ch)
    _check_truth(f"full alignment C={ch} B={batch}", _three_handles(monkeypatch, syn.FULL_ALIGNMENT, ch, True, sd), lambda m: m.predict_numpy(x),
                 syn.FULL_ALIGNMENT, batch, fused=("act0", "act8"))


def test_record_depth55_compares_act8_and_spp(monkeypatch):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=823)
    x = syn.make_fa_windows(3, seed=824, depth=55)
    _check_truth("depth 55", _three_handles(monkeypatch, syn.FULL_ALIGNMENT, 8, True, sd, depth=55), lambda m: m.predict_numpy(x),
                 syn.FULL_ALIGNMENT, 3, fused=("act0",), depth=55)


def test_record_unfused_forms_compare_act0_and_act8(monkeypatch):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=825)
    x = syn.make_fa_windows(3, seed=826)
    env = {"C3HIP_CONV1_FUSED": "0", "C3HIP_SPP_FUSED": "0"}
    _, unfused = _check_truth("unfused", _three_handles(monkeypatch, syn.FULL_ALIGNMENT, 8, True, sd, env=env), lambda m: m.predict_numpy(x),
                              syn.FULL_ALIGNMENT, 3)
    m = _model(monkeypatch, syn.FULL_ALIGNMENT, 8, True, sd, fp32=0)  # without the switches both report "fused"
    m.verify(every=1, layers=True)
    m.predict_numpy(x)
    table = m.verify_layers()
    assert [e["name"] for e in table if e["status"] == "fused"] == ["act0", "act8"]
    # the layers behind a fused one are the same tensors on either form of the product pass
    for e, u in zip(table, unfused):
        if e["name"] in ("spp", "l4_out"):
            assert (e["ref_max_abs"], e["windows"]) == (u["ref_max_abs"], u["windows"]), (e, u)


# ------------------------------------------------------------------------------------------------ 2: beyond the micro-batch cap; candidates
@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_beyond_the_microbatch_cap(kind, monkeypatch):
    ch, indel, n, big = (18, False, 16500, "lstm2_out") if kind == syn.PILEUP else (8, True, 2100, "act7")
    sd = syn.make_state_dict(kind, ch, indel, seed=831)
    x = _tile(syn.make_windows(kind, 150, seed=832, channels=ch), n)
    mv, m16, m32 = _three_handles(monkeypatch, kind, ch, indel, sd)
    shapes = layer_shapes(kind)

    def call(m):  # ONE batch of the ring: the forward pass cuts it into micro-batches
        return m.wait(m.submit(x, slot=1))
    mv.verify(every=1, layers=True)
    call(mv)
    table = {e["name"]: e for e in mv.verify_layers()}
    for e in table.values():
        assert e["status"] == ("fused" if e["name"] in ("act0", "act8") else "compared") and e["windows"] == (0 if e["status"] == "fused" else n), e
    a, b = _tapped(m16, call, ["l4_out", big], shapes, n), _tapped(m32, call, ["l4_out", big], shapes, n)
    for k in ("l4_out", big):
        assert_layer(table[k], np_layer(a[k], b[k]), f"{n} windows")
    assert table[big]["max_abs_diff"] > 0


def test_candidates_only_kept_windows(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=841)
    region, major = syn.make_pileup_region(6000, 3, seed=842, empty_fraction=0.01, depth=260)
    rng = np.random.default_rng(843)
    cand = np.unique(rng.integers(major[0] - 30, major[-1] + 30, size=330))[:300]
    want_status, windows = syn.select_pileup_windows(region, major, cand, True)
    kept = len(windows)
    assert 0 < kept < len(cand) - 20, "candidates are dropped"

    def call(m):
        rows, status = m.predict_candidates(region, major, cand, head_tail=True)
        assert np.array_equal(status, want_status) and len(rows) == kept
        return rows
    _check_truth("candidates", _three_handles(monkeypatch, syn.PILEUP, 18, False, sd), call, syn.PILEUP, kept)


# ------------------------------------------------------------------------------------------------ 3: nothing else moves
@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_nothing_else_moves(kind, monkeypatch):
    ch, indel = (18, False) if kind == syn.PILEUP else (8, True)
    sd = syn.make_state_dict(kind, ch, indel, seed=851)
    sizes = (300, 17, 1025, 1, 64) if kind == syn.PILEUP else (77, 5, 130, 1, 20)
    batches = [syn.make_windows(kind, n, seed=852 + i, channels=ch) for i, n in enumerate(sizes)]
    m = _model(monkeypatch, kind, ch, indel, sd, fp32=0)

    def run():
        return [m.wait(m.submit(x, slot=i % 2)) for i, x in enumerate(batches)]
    plain = run()
    for every in (1, 3):
        m.verify(every=every)
        m.verify_reset()
        rows0, st0, d0 = run(), m.verify_stats(), m.describe()
        assert every != 1 or m.verify_layers() == [], "never enabled: no layers"
        m.verify(every=every, layers=True)
        m.verify_reset()
        rows1, st1, d1 = run(), m.verify_stats(), m.describe()
        for i, (p, a, b) in enumerate(zip(plain, rows0, rows1)):
            assert np.array_equal(p, a) and np.array_equal(p, b), f"every={every}: batch {i} is not the fp16x3 rows bit for bit"
        assert st0 == st1, (st0, st1)
        assert d1 == d0 + ",layers:1", (d0, d1)
        selected = [i for i in range(len(batches)) if i % every == 0]
        for e in m.verify_layers():
            if e["status"] == "compared":
                assert (e["batches"], e["windows"]) == (len(selected), sum(sizes[i] for i in selected)), (every, e)
                assert e["worst_batch"] in selected and e["ref_max_abs"] > 0
            else:
                assert e["name"] in ("act0", "act8") and e["batches"] == 0
        m.verify(every=every)  # (back to a handle whose switch is off: the layers stay listed, nothing is added)
        before = m.verify_layers()
        run()
        assert m.verify_layers() == before and "layers" not in m.describe()


# ------------------------------------------------------------------------------------------------ 4: off, skips, resets, the ring, the worker
def test_off_means_off(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=861)
    x = syn.make_pileup_windows(40, seed=862)
    m = _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=0)
    y0 = m.predict_numpy(x)
    assert m.verify_layers() == [] and "verify" not in m.describe()
    m.verify(every=0, layers=True)  # no effect while every == 0
    assert np.array_equal(m.predict_numpy(x), y0)
    table = m.verify_layers()
    assert [e["name"] for e in table] == P_LAYERS and all(e["status"] == "none" and e["batches"] == 0 and e["worst_batch"] == -1 for e in table), table
    assert m.verify_stats()["batches_submitted"] == 0 and "verify" not in m.describe()


def test_user_taps_keep_mode_and_profiling_are_left_alone(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=863)
    x = syn.make_pileup_windows(40, seed=864)
    plain, m = _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=0), _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=0)
    m.verify(every=1, layers=True)
    for h in (plain, m):
        h.tap("lstm1_out,lstm2_out")
    y0, y1 = plain.predict_numpy(x), m.predict_numpy(x)
    assert np.array_equal(y0, y1)
    for name, shape in (("lstm1_out", (40, 33, 256)), ("lstm2_out", (40, 33, 320))):
        assert np.array_equal(plain.tap_fetch(name, 0, shape), m.tap_fetch(name, 0, shape)), f"{name}: the user's tapped tensor"
    assert all(e["batches"] == 0 for e in m.verify_layers()) and m.verify_stats()["batches_skipped"] == 1
    m.tap("")
    m.profile(True)
    m.predict_numpy(x)
    names = [r["name"] for r in m.profile_read()]
    m.profile(False)
    assert names and all(e["batches"] == 0 for e in m.verify_layers()) and m.verify_stats()["batches_skipped"] == 2
    kept = _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=0, keep=True)
    kept.verify(every=1, layers=True)
    assert np.array_equal(kept.predict_numpy(x), y0)
    assert all(e["batches"] == 0 for e in kept.verify_layers()) and kept.verify_stats()["batches_skipped"] == 1
    m.predict_numpy(x)  # nothing in the way any more
    assert all(e["batches"] == 1 and e["windows"] == 40 for e in m.verify_layers()), m.verify_layers()


def test_reload_and_reset_zero_the_totals_and_keep_the_setting(monkeypatch):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=871)
    x = syn.make_fa_windows(6, seed=872)
    m = _model(monkeypatch, syn.FULL_ALIGNMENT, 8, True, sd, fp32=0)
    m.verify(every=1, layers=True)
    m.predict_numpy(x)
    first = m.verify_layers()
    assert [e["batches"] for e in first] == [0] + [1] * 7 + [0, 1, 1]
    for zero in (m.verify_reset, lambda: m.load_state_dict(sd)):
        zero()
        table = m.verify_layers()
        assert all((e["batches"], e["windows"], e["max_abs_diff"], e["ref_max_abs"], e["worst_batch"], e["status"]) == (0, 0, 0.0, 0.0, -1, "none")
                   for e in table), table
        assert m.describe().endswith(",layers:1")
        m.predict_numpy(x)
        assert m.verify_layers() == first, "the same batch gives the same record"


@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_three_slots_in_flight_match_blocking_calls(kind, monkeypatch):
    ch, indel = (18, False) if kind == syn.PILEUP else (8, True)
    sd = syn.make_state_dict(kind, ch, indel, seed=881)
    sizes = (300, 256, 17, 500, 64, 256, 129) if kind == syn.PILEUP else (40, 64, 17, 70, 64, 30, 33)
    batches = [syn.make_windows(kind, n, seed=882 + i, channels=ch) for i, n in enumerate(sizes)]
    ring, blocking = _model(monkeypatch, kind, ch, indel, sd, fp32=0), _model(monkeypatch, kind, ch, indel, sd, fp32=0)
    for m in (ring, blocking):
        m.verify(every=2, layers=True)
    want = [blocking.predict_numpy(x) for x in batches]
    got, tickets = [], []
    for i, x in enumerate(batches):
        if len(tickets) == 3:
            got.append(ring.wait(tickets.pop(0)))
        tickets.append(ring.submit(x, slot=i % 3))
    got += [ring.wait(t) for t in tickets]
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    lr, lb = ring.verify_layers(), blocking.verify_layers()
    assert lr == lb, (lr, lb)
    assert all((e["batches"], e["windows"]) == (4, sum(sizes[0::2])) for e in lr if e["status"] == "compared") and any(e["max_abs_diff"] > 0 for e in lr)


def test_worker_process_leaves_the_layer_lines_behind_its_summary(tmp_path):
    import os
    from tests import refloop
    ref = refloop.reference_root()
    if ref is None:
        pytest.skip("no reference modules (oracle/_ref is staged by the build)")
    d = str(tmp_path)
    sizes = [1300, 41]
    lst = refloop.write_job(d, syn.PILEUP, sizes, channels=18)
    ck = os.path.join(d, "model")
    refloop.write_checkpoint(ck + ".pt", syn.PILEUP, 18, False)
    ver = _worker(ref, d, lst, ck, os.path.join(d, "verify.vcf"), {"C3HIP_VERIFY": "2"})
    lay = _worker(ref, d, lst, ck, os.path.join(d, "layers.vcf"), {"C3HIP_VERIFY": "2", "C3HIP_VERIFY_LAYERS": "1"})
    assert ver.returncode == 0 and lay.returncode == 0, (lay.stdout + lay.stderr)[-3000:]
    print(lay.stderr[-2000:])
    lines = lay.stderr.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("[clair3_amd] verify:")]
    assert len(at) == 1, lay.stderr[-3000:]
    tail = lines[at[0] + 1:at[0] + 1 + len(P_LAYERS)]
    assert [ln.split()[3] for ln in tail] == P_LAYERS and all(ln.startswith("[clair3_amd] verify layer ") and " batches=" in ln for ln in tail), tail
    assert not [ln for ln in ver.stderr.splitlines() if "verify layer" in ln]
    assert len(lines) == len(ver.stderr.splitlines()) + len(P_LAYERS) and lines[at[0]] == [ln for ln in ver.stderr.splitlines() if "verify:" in ln][0]
    assert lay.stdout == ver.stdout, "stdout is the loop's own"
    assert refloop.vcf_records(os.path.join(d, "layers.vcf")) == refloop.vcf_records(os.path.join(d, "verify.vcf"))
