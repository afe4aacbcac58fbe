"""The full-alignment kernels at other window geometries than 89 x 33 and 55 x 33 (needs an MI355X).  The library takes any
(depth, positions) -- c3_model_set_geometry asks for >= 1 x 1 and Clair3_F follows the tensor -- and feeds it into the fused conv1 of
res1a / res1b (even input extents, the unaligned 9-channel fetches), the halo tile, the F(2,3) row pairs, the stride-2 kernels, the
division magics, the table-driven pooling, the switch to the fp32 stack for windows wider than 34, the exact form and the rows pre-pass.
Nine shapes, chosen for what each reaches (tests/test_geometry.py pins the fp64 oracle at them against the reference module):

    depth x positions   stages behind conv1 / conv3 / conv5
    90 x 34             45x17, 23x9, 12x5   even H and W at conv1 only; the rest is the ONT product path (pooling inside res3b); C = 8 and 9
    64 x 33             32x17, 16x9,  8x5   even H into every stride-2 layer and F(2,3) row pair; table pooling
    144 x 33            72x17, 36x9, 18x5   tall: the most pixels per window, pooling bins of 6 rows
    41 x 20             21x10, 11x5,  6x3   even W at conv1's input and at the 64-channel block, final W = 3; C = 8 and 9
    33 x 23             17x12,  9x6,  5x3   even W at the first two stages
    17 x 17              9x9,   5x5,  3x3   the smallest 14-bin window: several windows and all their borders inside one 128-pixel tile
    18 x 24              9x12,  5x6,  3x3   the same with even extents
    55 x 41             28x21, 14x11, 7x6   wider than the halo tile is sized for: the call takes the fp32 stack by itself
    23 x 35             12x18,  6x9,  3x5   the narrowest window that does so

Bounds are the project's own (test_product_layers_gpu.py): 2e-5 of a tensor's range and of a channel's scale, no worse than 5x the fp32
forms' error (+3e-7 per tensor, +1e-6 per channel), rows within 2e-5 of the oracle, labels identical outside near-ties; the exact form
at test_exact_gpu.py's bounds.  Batch sizes: 1, 3, 17 and big_batch() -- the smallest batch at which every convolution launch of the
shape has more tiles than the chip has CUs, so that the persistent walks, the paired forms and both stride-2 forms run."""
import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from tests import util
from tests.test_exact_gpu import check_layer, check_rows
from tests.test_parity_gpu import make_model
from tests.test_product_layers_gpu import FA_TAPS, Oracle, sample, tapped

pytestmark = pytest.mark.gpu

SHAPES = [(90, 34), (64, 33), (144, 33), (41, 20), (33, 23), (17, 17), (18, 24), (55, 41), (23, 35)]
DWELL = [(90, 34), (41, 20)]
REFUSED = [(89, 31), (25, 33), (3, 3)]  # 11, 11 and 3 pyramid bins
ENTRIES = [(d, p, 8) for d, p in SHAPES] + [(d, p, 9) for d, p in DWELL]
WIDE = [(55, 41), (23, 35)]
# the weight seeds of test_product_layers_gpu.py; a shape whose activations trip the fp16 range guard with them takes "peaked" (43)
SEEDS = {"plain": 41, "peaked": 43, "trained_like": 141}
WEIGHTS_AT = {}  # (depth, positions, channels, weights) -> the weights used instead

CUS = 256                             # compute units of an MI355X: a launch with more tiles takes the forms for a full chip
K_PL_BM, K_WTM, K_S2_BM = 128, 126, 128  # kPlBM (c3_conv3.h), kWTM (c3_conv3w.h), kS2BM (c3_conv3s2.h): pixels per tile
TABLE, FORMS_SEEN = [], set()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("C3HIP_FP32", "C3HIP_WINO", "C3HIP_KEEP_ACTIVATIONS", "C3HIP_CONV1_FUSED", "C3HIP_SPP_FUSED"):
        monkeypatch.delenv(k, raising=False)


def stages(depth, positions):
    out, h, w = [], depth, positions
    for _ in range(3):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def tile_counts(n, depth, positions):
    """tiles of every convolution launch behind conv1 as run_fa_planes counts them (c3_forward.h), whichever form a stride-1 layer takes:
    direct ceil(M / kPlBM) x Cout / 64 with M = n H W; F(2,3) ceil(n Hj W / kWTM) x Cout / 64 with Hj = (H + 1) / 2; stride 2
    ceil(M / kS2BM) x Cout / 128"""
    out = []
    for s, (h, w) in enumerate(stages(depth, positions)):
        cout = 64 << s
        out.append(-(-n * h * w // K_PL_BM) * (cout // 64))
        out.append(-(-n * ((h + 1) // 2) * w // K_WTM) * (cout // 64))
        if s:
            out.append(-(-n * h * w // K_S2_BM) * (cout // 128))
    return out


def big_batch(depth, positions):
    """the smallest batch at which every launch has more tiles than CUs: 1821 windows at 17 x 17 (conv5: 9 pixels a window, two column
    tiles), 183 at 144 x 33, under the 2048 of a micro-batch everywhere"""
    n = 1
    while min(tile_counts(n, depth, positions)) <= CUS:
        n += 1
    return n


def weights_of(depth, positions, ch, weights):
    w = WEIGHTS_AT.get((depth, positions, ch, weights), weights)
    return syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=SEEDS[w], peaked=w != "plain", trained_like=w == "trained_like")


def model(ch, depth, positions, sd, taps="", keep=False):
    return make_model(syn.FULL_ALIGNMENT, ch, True, sd, keep=keep, depth=depth, positions=positions).tap(taps)


def run(m, x):
    return m.wait(m.submit(x, slot=0))


def field(form, name):
    return form.split(name + "=")[1].split()[0]


def _print_table(title):
    print(f"\n{title}: worst error per tensor / worst channel (x1e-6)")
    for what, whole, chan in TABLE:
        print(f"  {what:44s} " + " ".join(f"{k}={whole[k] * 1e6:.2f}" + (f"/{chan[k] * 1e6:.2f}" if k in chan else "") for k in whole))
    TABLE.clear()


def test_big_batches_are_what_the_launch_code_gives():
    """big_batch() against numbers worked out by hand from c3_forward.h: 17 x 17 -- conv5 has 9 n pixels in tiles of 128 and two column
    tiles, 2 ceil(9 n / 128) > 256 first at n = 1821; 90 x 34 -- res3a on F(2,3) has 6 x 5 tile-pixels a window and four column tiles,
    4 ceil(30 n / 126) > 256 first at n = 269, and conv5 2 ceil(60 n / 128) > 256 first at n = 274"""
    assert big_batch(17, 17) == 1821 and big_batch(90, 34) == 274
    assert all(big_batch(d, p) <= 2048 for d, p in SHAPES)


# ------------------------------------------------------------------------------------------ the product forms, layer by layer
@pytest.mark.parametrize("weights", ["plain", "trained_like"])
@pytest.mark.parametrize("depth,positions,ch", ENTRIES)
def test_product_layers_at_shape(depth, positions, ch, weights, monkeypatch):
    sd = weights_of(depth, positions, ch, weights)
    wide = (depth, positions) in WIDE
    n_big = big_batch(depth, positions)
    x = syn.make_fa_windows(n_big, seed=SEEDS[weights] + 1, channels=ch, depth=depth, positions=positions)
    oracle = Oracle(syn.FULL_ALIGNMENT, sd, x, True)
    plan = [({}, n) for n in (1, 3, 17, n_big)]
    if (depth, positions, ch) == (41, 20, 8):  # every stride-1 layer on the direct kernel, once
        plan += [({"C3HIP_WINO": "0"}, 17), ({"C3HIP_WINO": "0"}, n_big)]
    every = np.array(sorted(set().union(*[set(sample(n).tolist()) for _, n in plan])))
    y_all, d_all = oracle(every)
    pos = {int(i): j for j, i in enumerate(every)}
    # the comparison form: fp32 MFMA on fp32 activations, every layer written, one pass over the pool
    monkeypatch.setenv("C3HIP_FP32", "1")
    m32 = model(ch, depth, positions, sd, FA_TAPS)
    monkeypatch.delenv("C3HIP_FP32")
    run(m32, x)
    assert "conv_stack=fp32-mfma" in m32.describe()
    f32 = {name: tapped(m32, name, every, d_all[name].shape[1:]) for name in FA_TAPS}
    handles = {}
    for env, n in plan:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        key = tuple(sorted(env.items()))
        if key not in handles:  # one handle per environment: its workspace grows from batch to batch
            handles[key] = model(ch, depth, positions, sd, FA_TAPS)
        m = handles[key]
        for k in env:
            monkeypatch.delenv(k)
        y = run(m, x[:n])
        form = m.describe()
        FORMS_SEEN.add(f"{depth}x{positions} " + form.split(" ring_lanes")[0].split("plane_stores=")[1].split(" ", 1)[1])
        what = f"{depth}x{positions} C={ch} {weights} n={n} {env or ''}"
        names = list(FA_TAPS)
        if wide:  # the fp32 stack, taken by the call itself: no switch, no range trip
            assert "conv_stack=fp32-mfma" in form and "on_fp32=0" in form, (what, form)
        else:
            assert "conv_stack=planes-f16x3" in form and "on_fp32=0" in form, (what, form)
            stride1 = field(form, "stride1")
            assert stride1[:2] == "dd" and (set(stride1) == {"d"} if env else stride1[2:5] == "www"), (what, form)
            with pytest.raises(Exception, match="act0 is computed inside res1a"):
                m.tap_fetch("act0", 0, (1,) + d_all["act0"].shape[1:])
            names.remove("act0")
            if stages(depth, positions)[2] == (12, 5):
                with pytest.raises(Exception, match="act8 is pooled inside res3b"):
                    m.tap_fetch("act8", 0, (1,) + d_all["act8"].shape[1:])
                names.remove("act8")
            if n == n_big:  # more tiles than CUs in every launch: both stride-2 layers paired, no F(2,3) layer on the one-tile-per-CU form
                assert field(form, "conv3") == field(form, "conv5") == "two-workgroups-per-cu", (what, form)
                assert "transform-waves" not in field(form, "wino_form"), (what, form)
            if n == 1:
                assert field(form, "conv3") == field(form, "conv5") == "one-workgroup-per-cu", (what, form)
        idx = sample(n)
        y_o, d = oracle(idx)
        sel = [pos[int(i)] for i in idx]
        mine = {name: tapped(m, name, idx, d[name].shape[1:]) for name in names}
        whole, chan = util.layer_errors(lambda k: mine[k], d, names, sd)
        w32, c32 = util.layer_errors(lambda k: f32[k][sel], d, names, sd)
        whole["y"] = util.assert_rows_match(y[idx], y_o, tol=2e-5, what=what)
        TABLE.append((what, whole, chan))
        TABLE.append(("   fp32 forms, same windows", w32, c32))
        for k in names:
            assert whole[k] <= 2e-5 and whole[k] <= 5 * w32[k] + 3e-7, (what, k, whole[k], w32[k])
            if k in chan:
                assert chan[k] <= 2e-5 and chan[k] <= 5 * c32[k] + 1e-6, (what, k, chan[k], c32[k])
    _print_table(f"full alignment {depth} x {positions}, C={ch}, {weights} weights")


def test_forms_seen(monkeypatch):
    """the sweep above ran every form of the stack (after it in file order; run alone, its calls are repeated for their forms)"""
    if not FORMS_SEEN:
        for depth, positions, ch in ENTRIES:
            sd = weights_of(depth, positions, ch, "plain")
            n_big = big_batch(depth, positions)
            x = syn.make_fa_windows(n_big, seed=SEEDS["plain"] + 1, channels=ch, depth=depth, positions=positions)
            for env in ({}, {"C3HIP_WINO": "0"}) if (depth, positions, ch) == (41, 20, 8) else ({},):
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                m = model(ch, depth, positions, sd)
                for k in env:
                    monkeypatch.delenv(k)
                for n in (1, 17, n_big):
                    run(m, x[:n])
                    FORMS_SEEN.add(f"{depth}x{positions} " + m.describe().split(" ring_lanes")[0].split("plane_stores=")[1].split(" ", 1)[1])
    seen = " | ".join(sorted(FORMS_SEEN))
    print("forms seen:\n  " + "\n  ".join(sorted(FORMS_SEEN)))
    for want in ("conv3=one-workgroup-per-cu", "conv3=two-workgroups-per-cu", "conv5=one-workgroup-per-cu", "conv5=two-workgroups-per-cu",
                 "stride1=dddddd"):
        assert want in seen, (want, seen)
    stride1 = {field(f, "stride1") for f in FORMS_SEEN if "planes-f16x3" in f}
    assert any("w" in s for s in stride1) and any(set(s) == {"d"} for s in stride1), stride1
    for depth, positions in SHAPES:
        mine = [f for f in FORMS_SEEN if f.startswith(f"{depth}x{positions} ")]
        assert mine, (depth, positions)
        if positions <= 34:
            assert all("conv_stack=planes-f16x3" in f and "on_fp32=0" in f for f in mine), mine
        else:
            assert all("conv_stack=fp32-mfma" in f and "on_fp32=0" in f for f in mine), mine


# ------------------------------------------------------------------------------------------ keep mode: the unfused forms
@pytest.mark.parametrize("depth,positions,ch", ENTRIES)
def test_keep_mode_layers_at_shape(depth, positions, ch):
    """keep mode runs conv1 as its own launch (conv1_i8_f16_kernel; Conv1Loader for 9 channels) and the table-driven spp_planes_kernel:
    all nine convolution outputs, the pooled vector and the rows against the oracle, as test_other_window_geometry does for 55 x 33"""
    from oracle import oracle
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=101)
    x = syn.make_fa_windows(5, seed=102, channels=ch, depth=depth, positions=positions)
    m = model(ch, depth, positions, sd, keep=True)
    y = m.predict_numpy(x)
    form = m.describe()
    assert ("conv_stack=fp32-mfma" if positions > 34 else "conv_stack=planes-f16x3") in form and "on_fp32=0" in form, form
    y_o, d = oracle.fa_forward(sd, x, True, debug=True)
    errs = {}
    for name in [f"act{l}" for l in range(9)] + ["spp", "l4_out"]:
        a = m.debug_fetch(name, d[name].shape)
        assert np.isfinite(a).all(), name
        errs[name] = float(np.abs(a - d[name]).max()) / max(1.0, float(np.abs(d[name]).max()))
    errs["y"] = util.assert_rows_match(y, y_o, tol=2e-5, what=f"keep mode {depth}x{positions} C={ch}")
    print(f"keep mode {depth}x{positions} C={ch} (x1e-6): " + " ".join(f"{k}={v * 1e6:.2f}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e < 2e-5, (name, e)


# ------------------------------------------------------------------------------------------ windows wider than the halo tile
@pytest.mark.parametrize("depth,positions", WIDE)
def test_wide_windows_take_the_fp32_stack_by_themselves(depth, positions, capfd):
    from oracle import oracle
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=41)
    xw = syn.make_fa_windows(9, seed=42, depth=depth, positions=positions)
    x89 = syn.make_fa_windows(9, seed=43)
    want89 = make_model(syn.FULL_ALIGNMENT, 8, True, sd).predict_numpy(x89)
    capfd.readouterr()
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)  # the default geometry: the handle follows the tensor
    y = m.predict_numpy(xw)
    form = m.describe()
    assert "conv_stack=fp32-mfma" in form and "on_fp32=0" in form and "precision=fp16x3" in form, form
    assert m.range_status() == (0, False)
    err = util.assert_rows_match(y, oracle.fa_forward(sd, xw, True), tol=2e-5, what=f"wide {depth}x{positions}")
    # back to 89 x 33 on the same handle: the plane kernels again, and the rows of a handle that never saw a wide window
    y89 = m.predict_numpy(x89)
    form = m.describe()
    assert "conv_stack=planes-f16x3" in form and "on_fp32=0" in form, form
    assert np.array_equal(y89, want89)
    assert np.array_equal(m.predict_numpy(xw), y)
    said = capfd.readouterr().err
    assert "activations beyond the range" not in said and "continues on fp32" not in said, said
    print(f"wide {depth}x{positions}: rows max|dY| = {err:.2e}")


# ------------------------------------------------------------------------------------------ the exact form
@pytest.mark.parametrize("depth,positions,ch", [(90, 34, 9), (41, 20, 8), (17, 17, 8)])
def test_exact_form_at_shape(depth, positions, ch):
    from oracle import oracle
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=61)
    x = syn.make_fa_windows(2, seed=62, channels=ch, depth=depth, positions=positions)
    y_o, d = oracle.fa_forward(sd, x, True, debug=True)
    m = model(ch, depth, positions, sd).exact(True)
    what = f"exact {depth}x{positions} C={ch}"
    check_rows(m.predict_exact(x), y_o, what)
    for name in [f"act{i}" for i in range(9)] + ["spp", "l4_out"]:
        check_layer(m.exact_fetch(name, 0, d[name].shape), d[name], f"{what} {name}")


# ------------------------------------------------------------------------------------------ the rows entry
@pytest.mark.parametrize("depth,positions,ch", [(64, 33, 8), (41, 20, 8), (41, 20, 9)])
def test_rows_entry_at_shape(depth, positions, ch):
    """windows handed over as their occupied rows (c3_expand.h: 8-byte pieces for an even channel count, bytes for 9) give the rows of the
    dense entry on the padded windows, bit for bit -- centred runs, runs placed by ``firsts``, and through the ring on two slots"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=71)
    x = syn.make_fa_windows(23, seed=72, channels=ch, depth=depth, positions=positions)
    x[5] = 0  # a window without reads
    rows, firsts, counts = syn.pack_fa_rows(x)
    assert np.array_equal(syn.pad_fa_rows(rows, counts, depth=depth), x)  # the recipe centres its reads
    m = model(ch, depth, positions, sd)
    dense = m.predict_numpy(x)
    assert np.array_equal(m.predict_rows(rows, counts), dense)
    rng = np.random.default_rng(73)
    moved = rng.integers(0, depth - counts + 1).astype(np.int32)  # anywhere the run fits, the two ends included
    moved[0], moved[1] = 0, depth - counts[1]
    x_moved = syn.pad_fa_rows(rows, counts, moved, depth=depth)
    dense_moved = m.predict_numpy(x_moved)
    assert not np.array_equal(dense_moved, dense)
    assert np.array_equal(m.predict_rows(rows, counts, moved), dense_moved)
    t0 = m.submit_rows(rows, counts, slot=0)
    t1 = m.submit_rows(rows, counts, moved, slot=1)
    assert np.array_equal(m.wait(t0), dense) and np.array_equal(m.wait(t1), dense_moved)
    assert "rows_windows=23" in m.describe(), m.describe()


# ------------------------------------------------------------------------------------------ one handle, many shapes
SEQUENCE = [(17, 17), (144, 33), (41, 20), (89, 33), (55, 41), (17, 17)]


def test_one_handle_many_shapes():
    """a single handle fed six batches of five shapes, following the tensor: every step gives the rows of a fresh handle of that shape
    (workspaces freed and regrown, weights packed again, the census reset), and further passes over the sequence leave no more device
    memory in use than the first.  c3_mem_info counts whole 2 MiB fragments -- the runtime hands out allocations below that size from
    blocks of it, and which block a regrown buffer lands in moves the figure by one fragment either way (measured after passes 1 - 4:
    10, 12, 10, 12 MiB over the loaded handle) -- so "no growth" is held to that resolution over THREE further passes: anything the
    sequence frees and regrows (the 144 x 33 workspace alone is 6.6 MB, a set of packed weights more) would add at least 18 MB"""
    fragment = 2 << 20
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=81)
    xs = {s: syn.make_fa_windows(7, seed=82 + i, depth=s[0], positions=s[1]) for i, s in enumerate(sorted(set(SEQUENCE)))}
    want = {}
    for (d, p), x in xs.items():
        fresh = model(8, d, p, sd)
        want[(d, p)] = fresh.predict_numpy(x)
        fresh._destroy()
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    used = []
    for rounds in range(4):
        for step, s in enumerate(SEQUENCE):
            y = m.predict_numpy(xs[s])
            assert np.array_equal(y, want[s]), (rounds, step, s, float(np.abs(y - want[s]).max()))
            assert ("conv_stack=fp32-mfma" if s[1] > 34 else "conv_stack=planes-f16x3") in m.describe(), (s, m.describe())
        m.synchronize()
        free_b, total_b = _lib.mem_info(0)
        used.append(total_b - free_b)
    print(f"device memory in use after passes 1 - 4: {used} bytes")
    assert max(used[1:]) - used[0] <= fragment, used


# ------------------------------------------------------------------------------------------ refusals
def test_refused_shapes():
    """shapes whose last stage pools into other than 14 bins are refused by name; the handle then answers 89 x 33 as before, and a load
    behind a refused shape leaves a handle that is whole: it follows the next tensor, and still refuses the shape"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=91)
    x89 = syn.make_fa_windows(6, seed=92)
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    y89 = m.predict_numpy(x89)
    for depth, positions in REFUSED:
        x = syn.make_fa_windows(3, seed=93, recipe="uniform", depth=depth, positions=positions)
        with pytest.raises(_lib.C3Error, match="unsupported geometry"):
            m.predict_numpy(x)
        with pytest.raises(_lib.C3Error, match="unsupported geometry"):  # ... through the ring as well, and the slot stays free
            m.submit(x, slot=0)
        assert np.array_equal(m.predict_numpy(x89), y89), (depth, positions)
        assert "conv_stack=planes-f16x3" in m.describe() and "on_fp32=0" in m.describe()
    x = syn.make_fa_windows(3, seed=93, recipe="uniform", depth=25, positions=33)
    with pytest.raises(_lib.C3Error, match="unsupported geometry: 11 pyramid bins"):
        m.predict_numpy(x)
    m.load_state_dict(sd)  # loaded at 25 x 33: one geometry, everywhere
    assert m._geometry == (25, 33) and _lib.lib().c3_model_window_bytes(m._handle, _lib.DTYPE_I8) == 25 * 33 * 8
    with pytest.raises(_lib.C3Error, match="unsupported geometry: 11 pyramid bins"):
        m.predict_numpy(x)
    assert np.array_equal(m.predict_numpy(x89), y89)
    assert _lib.lib().c3_model_window_bytes(m._handle, _lib.DTYPE_I8) == 89 * 33 * 8
    keep = model(8, 3, 3, sd, keep=True)  # the unfused forms get as far as the pooling table too
    with pytest.raises(_lib.C3Error, match="unsupported geometry: 3 pyramid bins"):
        keep.predict_numpy(syn.make_fa_windows(2, seed=94, recipe="uniform", depth=3, positions=3))


# ------------------------------------------------------------------------------------------ a geometry change under a batch in flight
def test_geometry_change_is_refused_while_a_batch_is_in_flight():
    """c3_model_set_geometry frees every lane's workspace and drops the weights: with a batch in flight it is refused on the host, before
    it touches anything, like c3_model_load and c3_model_set_decode_columns; the geometry the handle already has is no change"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=95)
    x89, x55 = syn.make_fa_windows(40, seed=96), syn.make_fa_windows(24, seed=97, depth=55)
    want89 = make_model(syn.FULL_ALIGNMENT, 8, True, sd).predict_numpy(x89)
    want55 = make_model(syn.FULL_ALIGNMENT, 8, True, sd, depth=55).predict_numpy(x55)
    m = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
    t0 = m.submit(x89, slot=0)
    with pytest.raises(_lib.C3Error, match="a prediction is in flight: call c3_predict_wait first"):
        m.submit(x55, slot=1)
    assert m._geometry in (None, (89, 33))
    assert _lib.lib().c3_model_window_bytes(m._handle, _lib.DTYPE_I8) == 89 * 33 * 8
    # the geometry it has: not refused, at either level, and the weights stay
    assert _lib.lib().c3_model_set_geometry(m._handle, 89, 33) == 0
    m.set_geometry(89, 33)
    t1 = m.submit(x89[:7], slot=1)
    assert np.array_equal(m.wait(t0), want89)
    assert np.array_equal(m.wait(t1), want89[:7])
    assert np.array_equal(m.wait(m.submit(x55, slot=1)), want55)  # nothing in flight: the change goes through
    assert m._geometry == (55, 33)
    assert np.array_equal(m.predict_numpy(x89), want89)


# ------------------------------------------------------------------------------------------ pileup windows of other lengths
def _pileup_case(T, n):
    """weights whose L4 takes 320 T inputs and (n, T, 18) windows: the realistic counts laid end to end and cut into windows of T columns"""
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=51)
    k = 1.0 / np.sqrt(320 * T)
    sd["L4.weight"] = (4.0 * np.random.default_rng(5100 + T).uniform(-k, k, size=(128, 320 * T))).astype(np.float32)
    cols = syn.make_pileup_windows(-(-n * T // syn.NO_OF_POSITIONS), seed=52).reshape(-1, syn.PILEUP_CHANNELS)
    return sd, np.ascontiguousarray(cols[:n * T].reshape(n, T, syn.PILEUP_CHANNELS))


@pytest.mark.parametrize("T", [16, 40])
def test_pileup_positions(T):
    """c3_model_set_geometry takes a pileup ``positions`` other than 33 (K4 = 320 T, T steps in both recurrences): batch 17 and the
    1024 of the half tiles against the fp64 oracle, which takes T from the tensor, at the rows bound of test_pileup_product_layers"""
    from oracle import oracle
    sd, x = _pileup_case(T, 1024)
    m = make_model(syn.PILEUP, 18, True, sd, positions=T)
    idx = np.union1d(sample(17), sample(1024))
    y_o = oracle.pileup_forward(sd, x[idx], True)
    for n in (17, 1024):
        y = run(m, x[:n])
        form = m.describe()
        assert "on_fp32=0" in form and "precision=fp16x3" in form, form
        if n == 1024:
            assert field(form, "lstm1") == "fused-f16x3-half-tiles" and field(form, "lstm2") == "f16x3-half-tiles", form
        sel = idx < n
        err = util.assert_rows_match(y[idx[sel]], y_o[sel], tol=2e-5, what=f"pileup T={T} n={n}")
        print(f"pileup T={T} n={n}: {field(form, 'lstm1')} {field(form, 'proj2')} {field(form, 'lstm2')} rows max|dY| = {err:.2e}")
    with pytest.raises(_lib.C3Error, match="shape"):
        m.predict_numpy(x[:2, :T - 1])
