"""Inputs the library does not control (need an MI355X).  The rest of the suite stages host windows into the library's own aligned
buffers, draws pileup counts from int8-sized recipes and loads every handle once.  A caller does not:
  * device-resident windows on buffers the library did not allocate -- a torch slice xd[k:] starts k windows into its allocation, an odd
    address for 9-channel (dwell) windows, and the raw ABI takes any byte address -- and rows written into the middle of a caller's tensor;
  * int32 pileup windows with the counts of real coverage (hundreds to tens of thousands, beyond int8), which drive the LSTM gates far
    into saturation;
  * a second c3_model_load into a handle whose range guard has tripped.
Each is held to the fp64 oracle (oracle/c3_oracle.c) and to the library's own staged path, bit for bit where the arithmetic is the same."""
import ctypes as C

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from tests import util
from tests.test_parity_gpu import describe, make_model

pytestmark = pytest.mark.gpu

LAYER_TOL = 2e-5  # the suite's layer gate: max |d| / max(1, max |ref|)
PATTERN = 0x5B    # what fills every byte around a view: a read outside the view changes the rows


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------------------------------------ A: offset views, foreign bases

# name -> (kind, channels, window dtype, add_indel, a size past a form threshold: conv3's two-workgroups form / the weights-resident projection)
SHAPES = {
    "pileup_i8": (syn.PILEUP, 18, np.int8, False, 300),
    "pileup_i32": (syn.PILEUP, 18, np.int32, False, 300),
    "fa_c8": (syn.FULL_ALIGNMENT, 8, np.int8, True, 200),
    "fa_c9": (syn.FULL_ALIGNMENT, 9, np.int8, True, 200),
}
ENVS = {"default": {}, "conv1_unfused": {"C3HIP_CONV1_FUSED": "0"}, "fp32": {"C3HIP_FP32": "1"}}
_CASES = [(s, n, e) for s in SHAPES for e in ENVS for n in (1, 5, SHAPES[s][4])
          if not (e == "conv1_unfused" and SHAPES[s][0] == syn.PILEUP)]  # (conv1 is a full-alignment layer)
_oracle_cache = {}


def _windows(shape, n, seed):
    """n windows whose bytes are non-zero up to the last pixel of the last window (the realistic full-alignment recipe leaves the last
    rows empty, which would hide a zeroed end): the uniform recipe for full alignment, realistic pileup windows ending in a uniform one"""
    kind, ch, dt, _, _ = SHAPES[shape]
    if kind == syn.FULL_ALIGNMENT:
        return syn.make_fa_windows(n, seed=seed, recipe="uniform", channels=ch)
    x = syn.make_pileup_windows(n, seed=seed, dtype=dt)
    x[-1] = syn.make_pileup_windows(1, seed=seed + 1, recipe="uniform", dtype=dt)[0]
    return x


def _env(monkeypatch, env):
    for k in ("C3HIP_CONV1_FUSED", "C3HIP_FP32"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)


def _model_and_rows(shape, n, env, monkeypatch, oracle_mod):
    """a handle under env, n windows, their rows through the staged host path, and the first / last 4 of them held to the oracle"""
    kind, ch, dt, indel, _ = SHAPES[shape]
    _env(monkeypatch, env)
    sd = syn.make_state_dict(kind, ch, indel, seed=301 + ch)
    m = make_model(kind, ch, indel, sd)
    x = _windows(shape, n, seed=302 + n)
    y = m.predict_numpy(x)
    assert ("on_fp32=1" in describe(m)) == (env == "fp32"), describe(m)
    sel = np.unique(np.r_[0:min(4, n), max(0, n - 4):n])
    key = (shape, n)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle_mod.forward(kind, sd, x[sel], indel)
    util.assert_rows_match(y[sel], _oracle_cache[key], what=f"{shape} n={n} {env}: first / last windows vs oracle")
    return m, x, y


@pytest.mark.parametrize("shape,n,env", _CASES)
def test_device_entries_on_offset_views(shape, n, env, monkeypatch, oracle_mod):
    """xd[k:k + n] of one device tensor of n + 3 windows (k = 0..3: the view's base k windows into the allocation; k = 3 ends it), every
    other byte of the tensor the fill pattern: the unchecked entry, the checked one and forward(checked=True) return the staged path's
    rows bit for bit"""
    import torch
    m, x, y = _model_and_rows(shape, n, env, monkeypatch, oracle_mod)
    tdt = torch.int8 if x.dtype == np.int8 else torch.int32
    wbytes = x[0].nbytes
    for k in range(4):
        xd = torch.full((n + 3,) + x.shape[1:], PATTERN if tdt == torch.int8 else PATTERN * 0x01010101, dtype=tdt, device="cuda:0")
        xd[k:k + n] = torch.from_numpy(x).cuda()
        view = xd[k:k + n]
        assert view.is_contiguous() and view.data_ptr() == xd.data_ptr() + k * wbytes
        got = {"unchecked": m(view), "forward(checked=True)": m.forward(view, checked=True)}
        yc = torch.empty((n, m.row_size), dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().c3_predict_device_checked(m._handle, C.c_void_p(view.data_ptr()), _lib.DTYPE_I8 if tdt == torch.int8 else _lib.DTYPE_I32,
                                                        n, C.c_void_p(yc.data_ptr()), C.c_void_p(stream)), "c3_predict_device_checked")
        got["c3_predict_device_checked"] = yc
        torch.cuda.synchronize()
        for what, yd in got.items():
            assert np.array_equal(yd.cpu().numpy(), y), f"{shape} n={n} {env}: {what} on xd[{k}:{k + n}] (base + {k * wbytes} B) differs from the staged rows"
    assert m.range_status() == (0, env == "fp32")


@pytest.mark.parametrize("shape,env", [(s, e) for s in ("pileup_i8", "fa_c8", "fa_c9") for e in ENVS
                                       if not (e == "conv1_unfused" and SHAPES[s][0] == syn.PILEUP)])
def test_raw_entries_at_odd_byte_addresses(shape, env, monkeypatch, oracle_mod):
    """int8 window blocks that start 1, 3 and 7 bytes into a torch.empty allocation (what a caller's own packing may hand over through
    the C ABI): rows equal to the aligned call's"""
    import torch
    n = 5 if SHAPES[shape][0] == syn.FULL_ALIGNMENT else SHAPES[shape][4]
    m, x, y = _model_and_rows(shape, n, env, monkeypatch, oracle_mod)
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for off in (1, 3, 7):
        buf = torch.empty(x.nbytes + 64, dtype=torch.int8, device="cuda:0")
        buf.fill_(PATTERN)
        buf[off:off + x.nbytes] = torch.from_numpy(x.reshape(-1)).cuda()
        for name in ("c3_predict_device", "c3_predict_device_checked"):
            yd = torch.full((n, m.row_size), -3.0, dtype=torch.float32, device="cuda:0")
            _lib.check(getattr(L, name)(m._handle, C.c_void_p(buf.data_ptr() + off), _lib.DTYPE_I8, n, C.c_void_p(yd.data_ptr()), stream), name)
            torch.cuda.synchronize()
            assert np.array_equal(yd.cpu().numpy(), y), f"{shape} {env}: {name} on a block at byte offset {off}"


@pytest.mark.parametrize("kind,env", [(k, e) for k in (syn.PILEUP, syn.FULL_ALIGNMENT) for e in ENVS
                                      if not (e == "conv1_unfused" and k == syn.PILEUP)])
@pytest.mark.parametrize("decode", [False, True])
def test_submit_dev_writes_only_its_rows(kind, env, decode, monkeypatch):
    """c3_predict_submit_dev with y_dev at row k of a larger device tensor (decoder columns on: 55 / 121-float rows, no 16-byte multiple):
    the n rows are the staged path's, every float outside them keeps its value"""
    import torch
    _env(monkeypatch, env)
    ch = 18 if kind == syn.PILEUP else 9
    indel = kind == syn.FULL_ALIGNMENT
    m = make_model(kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=311))
    m.decode_columns(decode)
    n = 7
    x = syn.make_windows(kind, n, seed=312, channels=ch)
    y = m.predict_numpy(x)
    assert y.shape == (n, (90 if indel else 24) + (31 if decode else 0))
    for k in range(4):
        yd = torch.full((n + 6, m.row_size), -7.25, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert m.wait(m.submit_dev(x, yd.data_ptr() + k * m.row_size * 4, slot=0)) is None
        got = yd.cpu().numpy()
        assert np.array_equal(got[k:k + n], y), f"{kind} {env} decode={decode}: rows at row {k}"
        outside = np.r_[0:k, k + n:n + 6]
        assert (got[outside] == np.float32(-7.25)).all(), f"{kind} {env} decode={decode}: rows outside [{k}, {k + n}) were written"


# ------------------------------------------------------------------------------------------------ B: int32 counts beyond int8

DEPTHS = (128, 500, 3000, 30000)


def _extreme_windows(seed):
    """int32 windows at +-2^15 and +-2^20: constant, signs alternating over positions and channels, the sign pattern of realistic windows,
    sparse and dense random values"""
    rng = np.random.default_rng(seed)
    T, ch = syn.NO_OF_POSITIONS, 18
    alt = (-1) ** (np.arange(T)[:, None] + np.arange(ch)[None, :])
    base = syn.make_pileup_windows(2, seed=seed, dtype=np.int32)
    w = []
    for mag in (2 ** 15, 2 ** 20):
        w += [np.full((T, ch), mag), np.full((T, ch), -mag), mag * alt, -mag * alt, np.sign(base[0]) * mag,
              np.where(base[1] != 0, np.sign(base[1]) * mag, 0), rng.integers(-mag, mag + 1, size=(T, ch)),
              np.where(rng.random((T, ch)) < 0.1, mag, 0) * alt]
    return np.stack(w).astype(np.int32)


def _batch(which):
    if which == "extremes":
        return _extreme_windows(321)
    x = syn.make_pileup_windows(48, seed=322, dtype=np.int32, depth=which)
    if which > 128:
        assert (x.astype(np.int8) != x).any()  # int8 would have wrapped these counts
    return x


def _fp32_reference_errors(sd, x, d):
    """how far the reference's own fp32 arithmetic (the same ATen operators, oracle/torch_port.py) lands from the fp64 oracle, per layer"""
    import torch
    import torch.nn.functional as F
    from oracle import torch_port
    st = torch_port.to_torch(sd)
    lstms = torch_port.make_lstms(st)
    with torch.inference_mode():
        h1, _ = lstms[0](torch.as_tensor(x).float())
        h2, _ = lstms[1](h1)
        l4 = F.selu(F.linear(torch.flatten(h2, start_dim=1), st["L4.weight"], st["L4.bias"]))
    got = {"lstm1_out": h1, "lstm2_out": h2, "l4_out": l4}
    return {k: float(np.abs(v.numpy() - d[k]).max()) for k, v in got.items()}


@pytest.mark.parametrize("which", list(DEPTHS) + ["extremes"])
def test_int32_counts_of_real_coverage(which, monkeypatch, oracle_mod):
    """int32 pileup windows (the fp32 projection of LSTM1) at depths of 128 - 30000 and at +-2^15 / +-2^20: LSTM1, LSTM2 and L4 against the
    oracle at the layer gate, rows at the parity gate, under the default tile choice (half tiles at this batch), full tiles and the fp32
    forms; the region entry with int32 and int64 matrices of the same counts gives the same rows bit for bit.  Where the fp32 reference
    itself is further than the layer gate from the exact values (cancellation in the input projection of +-2^20 counts), the gate is eight
    times the reference's own error."""
    from clair3_amd.model import Clair3_P
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=323)
    x = _batch(which)
    y_o, d = oracle_mod.pileup_forward(sd, x, False, debug=True)
    if not np.isfinite(y_o).all():  # (not expected: the gates saturate, the oracle's softmax is stable)
        pytest.fail(f"oracle rows not finite at {which}")
    ref_err = _fp32_reference_errors(sd, x, d)
    worst = {}
    for env in ({}, {"C3HIP_HALF_TILES": "0"}, {"C3HIP_FP32": "1"}):
        for k in ("C3HIP_HALF_TILES", "C3HIP_FP32"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = make_model(syn.PILEUP, 18, False, sd, keep=True)
        y = m.predict_numpy(x)
        assert np.isfinite(y).all(), f"{which} {env}: non-finite rows"
        for key in ("lstm1_out", "lstm2_out", "l4_out"):
            a = m.debug_fetch(key, d[key].shape)
            assert np.isfinite(a).all(), f"{which} {env}: {key} not finite"
            scale = max(1.0, float(np.abs(d[key]).max()))
            err = float(np.abs(a - d[key]).max()) / scale
            worst[key] = max(worst.get(key, 0.0), err)
            tol = max(LAYER_TOL, 8.0 * ref_err[key] / scale)
            assert err < tol, f"{which} {env}: {key} err {err:.3e} (gate {tol:.1e}; fp32 reference {ref_err[key]:.1e})"
        util.assert_rows_match(y, y_o, what=f"{which} {env} vs oracle")
        m2 = make_model(syn.PILEUP, 18, False, sd)  # (no kept activations: the forms of an ordinary handle)
        y2 = m2.predict_numpy(x)
        util.assert_rows_match(y2, y_o, what=f"{which} {env} vs oracle, ordinary handle")
        if not env:
            tiles = describe(m2)
            assert "lstm1=fused-f16x3" in tiles and "on_fp32=0" in tiles, tiles
        elif "C3HIP_FP32" in env:
            assert "lstm1=fused-fp32-mfma" in describe(m2)
        else:
            assert "lstm1=fused-f16x3-full-tiles" in describe(m2)
        # the region entry: the windows laid end to end in one matrix, int32 and the size_t (int64) matrix of the same counts
        region32 = np.ascontiguousarray(x.reshape(-1, 18))
        region64 = region32.astype(np.int64)
        starts = np.arange(len(x), dtype=np.int32) * syn.NO_OF_POSITIONS
        assert isinstance(m2, Clair3_P)
        yr32, yr64 = m2.predict_region(region32, starts), m2.predict_region(region64, starts)
        assert np.array_equal(yr32, y2) and np.array_equal(yr64, y2), f"{which} {env}: region rows differ from the windows'"
    print(f"int32 counts at {which} (max |x| {int(np.abs(x).max())}): worst layer errors "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + "; fp32 reference " + ", ".join(f"{k} {v:.2e}" for k, v in ref_err.items()))


# ------------------------------------------------------------------------------------------------ C: the range guard across a reload

def _fa_beyond_fp16(seed=61):
    """test_parity_gpu's recipe: a stage at ~1e7 that overflows the fp16 pieces of the layers that read it"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=seed)
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    for k in ("conv3.conv.weight", "conv3.conv.bias", "conv3.bn.running_mean"):
        sd[k] *= 4.0e6
    for k in ("res_block2.0.conv1.weight", "res_block2.0.conv2.weight"):
        sd[k] /= 2.0e3
    sd["conv5.conv.weight"] /= 4.0e6
    return sd


def _pileup_beyond_fp16(seed=331):
    """one LSTM1 input weight of 1000: int8 windows take LSTM1's projection on fp16 pieces of 128 W_ih (c3_pack.h), and 128000 is beyond
    the fp16 range -- the pieces overflow, the rows come back NaN.  (The load-time precision decision does not look at LSTM1's W_ih, and
    the FC chain cannot overflow: L4 packs every feature row times its own power of two and the heads run on fp32.)"""
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=seed)
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    sd["LSTM1.weight_ih_l0"][5, 3] = 1000.0
    return sd


def _all_entries(m, x, xd):
    """rows of the host call, of a ring batch and of the checked device entry"""
    y_host = m.predict_numpy(x)
    y_ring = m.wait(m.submit(x, slot=1))
    y_dev = m.forward(xd, checked=True).cpu().numpy()
    return y_host, y_ring, y_dev


@pytest.mark.parametrize("kind", [syn.FULL_ALIGNMENT, syn.PILEUP])
def test_reload_ends_what_the_range_guard_decided(kind, monkeypatch, capfd, oracle_mod):
    """a handle whose guard has tripped (and whose sticky device flag is set) gets ordinary weights: it is back on fp16x3 with a clear
    flag, says nothing about fp32 over the next host, ring and checked device calls, and returns the rows of a fresh handle bit for bit"""
    import torch
    monkeypatch.delenv("C3HIP_FP32", raising=False)
    monkeypatch.delenv("C3HIP_AUTO_FP32", raising=False)
    ch, indel = (8, True) if kind == syn.FULL_ALIGNMENT else (18, False)
    bad = _fa_beyond_fp16() if kind == syn.FULL_ALIGNMENT else _pileup_beyond_fp16()
    x = syn.make_windows(kind, 6, seed=332, channels=ch)
    xd = torch.from_numpy(x).cuda()
    if kind == syn.PILEUP:  # confirm the recipe first: non-finite rows on fp16x3 (unchecked entry: no re-run), finite on the oracle
        y_o = oracle_mod.forward(kind, bad, x, indel)
        assert np.isfinite(y_o).all(), "the oracle overflows too: not a recipe for the range guard"
        probe = make_model(kind, ch, indel, bad)
        y_probe = probe(xd).cpu().numpy()
        flag, _ = probe.range_status()
        assert flag != 0 or not np.isfinite(y_probe).all(), "the large LSTM1 weight stays inside the fp16x3 range"
        del probe
    m = make_model(kind, ch, indel, bad)
    # trip it: full alignment through the host call (the conv kernels raise the device flag), pileup through the checked device entry
    # (its scan of the rows raises the flag; the host call finds the NaN rows on the host and leaves the flag alone)
    y_bad = m.predict_numpy(x) if kind == syn.FULL_ALIGNMENT else m.forward(xd, checked=True).cpu().numpy()
    assert np.isfinite(y_bad).all()
    util.assert_rows_match(y_bad, oracle_mod.forward(kind, bad, x, indel), what="re-run on fp32")
    assert "continues on fp32" in capfd.readouterr().err
    flag, on_fp32 = m.range_status()
    assert flag != 0 and on_fp32 and "on_fp32=1" in describe(m)
    good = syn.make_state_dict(kind, ch, indel, seed=333)
    m.load_state_dict(good)
    assert m.range_status() == (0, False), "a reload keeps the range guard's decision about the weights before"
    assert "on_fp32=0" in describe(m)
    fresh = make_model(kind, ch, indel, good)
    got, want = _all_entries(m, x, xd), _all_entries(fresh, x, xd)
    for what, a, b in zip(("host", "ring", "checked device"), got, want):
        assert np.array_equal(a, b), f"{kind}: {what} rows of the reloaded handle differ from a fresh one's"
    util.assert_rows_match(got[0], oracle_mod.forward(kind, good, x, indel), what="reloaded handle vs oracle")
    assert "continues on fp32" not in capfd.readouterr().err
    assert m.range_status() == (0, False) and "on_fp32=0" in describe(m)


@pytest.mark.parametrize("forced", ["0", "1"])
def test_reload_keeps_a_forced_precision(forced, monkeypatch):
    """C3HIP_FP32 is an explicit choice: =1 stays on fp32 across reloads; =0 comes back on fp16x3 after the guard tripped"""
    import torch
    monkeypatch.setenv("C3HIP_FP32", forced)
    x = syn.make_fa_windows(4, seed=341)
    good = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=342)
    m = make_model(syn.FULL_ALIGNMENT, 8, True, _fa_beyond_fp16())
    m.forward(torch.from_numpy(x).cuda(), checked=True)
    assert m.range_status()[1]
    m.load_state_dict(good)
    assert m.range_status() == (0, forced == "1"), describe(m)
    y = m.predict_numpy(x)
    assert m.range_status() == (0, forced == "1") and ("on_fp32=1" in describe(m)) == (forced == "1")
    assert np.array_equal(y, make_model(syn.FULL_ALIGNMENT, 8, True, good).predict_numpy(x))
    # the pileup handle: forced precision wins over the load-time decision too
    p = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=343))
    p.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, False, seed=344))
    assert p.range_status() == (0, forced == "1"), describe(p)


def test_reload_is_refused_while_a_batch_is_in_flight():
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=351)
    m = make_model(syn.PILEUP, 18, False, sd)
    x = syn.make_pileup_windows(16, seed=352)
    t = m.submit(x, slot=0)
    with pytest.raises(_lib.C3Error, match="in flight"):
        m.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, False, seed=353))
    y = m.wait(t)
    assert np.array_equal(y, m.predict_numpy(x))  # the refused load changed nothing
