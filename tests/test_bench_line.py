"""The ONE line bench.py prints must stay short enough for the driver to parse (round 3's 21 KB line was not) and keep value,
ms_per_step and roofline on the same leg (one batch in flight)."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_short_line_from_a_committed_full_record():
    import bench
    with open(os.path.join(ROOT, "profiles", "r03_final_bench20.json")) as fh:
        full = json.load(fh)
    names = ["full_alignment", "pileup", "full_alignment_dwell"]
    line = bench.short_line(full, names, os.path.join(ROOT, "gpurun_out", "bench_full.json"))
    text = json.dumps(line)
    assert len(text) <= 4096, len(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "host_inclusive", "gt_concordance"):
        assert key in line, key
    assert line["config"]["batches_in_flight"] == 1
    one = full["one_batch_in_flight"]
    assert abs(line["value"] / one["value"] - 1) < 1e-4 and abs(line["ms_per_step"] / one["ms_per_step"] - 1) < 1e-4
    roof = line["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "mfma_util", "avg_launch_us", "launches"):
        assert key in roof, key
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    # the step the roofline's kernels belong to is the step `value` is computed from
    assert abs(roof["step_us_one_batch_in_flight"] / (1e3 * line["ms_per_step"]) - 1) < 1e-3
    assert line["cpu_baseline"]["kind"] in ("reference", "port") and line["cpu_baseline"]["cores"] >= 1
    assert line["pileup"]["batches_in_flight"] == 1 and "roofline" in line["pileup"]
    assert line["full_record"] == os.path.join("gpurun_out", "bench_full.json")


def test_the_committed_final_collection_is_consistent():
    """profiles/r04_final_*: the line the bench printed on the GPU box is one parseable line under 4 KB whose value / ms_per_step / roofline
    describe the same leg; the roofline fraction recomputed from the rocprofv3 kernel statistics of the same box agrees within 3 %
    (tools/roofline_check.py); the PMC traffic the line quotes is the committed pmc_traffic.json"""
    import csv
    for name in ("r04_final_bench.json", "r04_final_bench20.json"):
        raw = open(os.path.join(ROOT, "profiles", name)).read().strip()
        assert len(raw.splitlines()) == 1 and len(raw) <= 4096, (name, len(raw))
        line = json.loads(raw)
        assert line["n_gpus"] == 1 and line["config"]["batches_in_flight"] == 1 and line["higher_is_better"] is True
        assert abs(line["value"] * line["ms_per_step"] / 1e3 / line["config"]["windows_per_step"] - 1) < 1e-3  # value = windows per step / step time
        roof = line["roofline"]
        assert roof["bound"] == "mfma" and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
        assert abs(roof["step_us_one_batch_in_flight"] / (1e3 * line["ms_per_step"]) - 1) < 1e-3
        assert line["cpu_baseline"]["kind"] == "reference" and line["gt_concordance"]["gt21_differ"] == 0
    line = json.loads(open(os.path.join(ROOT, "profiles", "r04_final_bench.json")).read())
    traffic = json.load(open(os.path.join(ROOT, "profiles", "r04_final_pmc_traffic.json")))
    assert abs(line["roofline"]["traffic"] / traffic.get("fabric_bytes_per_launch", traffic.get("hbm_bytes_per_launch")) - 1) < 1e-3
    # the same fraction from the profiler's averages: algorithmic FLOP of the convolution family / its launches' durations
    stats = {r["Name"]: (int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(os.path.join(ROOT, "profiles", "r04_final_kernel_stats_fa_one_in_flight.csv")))}
    conv = {k: v for k, v in stats.items() if "conv3x3_planes_kernel" in k or "conv3x3_s2_planes_kernel" in k}
    assert len(conv) == 8 and len({c for c, _ in conv.values()}) == 1  # eight launches per step, each once
    conv_us = sum(avg for _, avg in conv.values()) / 1e3
    flop = 449_418_240 * line["config"]["windows_per_step"]  # algorithmic FLOP of the convolution family per window (C = 8)
    frac_csv = flop / (conv_us * 1e-6) / 2500e12
    assert abs(frac_csv / line["roofline"]["frac"] - 1) < 0.03, (frac_csv, line["roofline"]["frac"])


def test_family_time_is_a_share_of_the_free_running_step():
    """round 4's line carried kernel_us_per_step 341.96 > step 336.6 us (eight bracketed launches read longer than the whole free-running
    step): the family's time is now its SHARE of the bracketed kernel time applied to the free-running step"""
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_final_bench_full.json")))
    r = full["roofline"]
    ev_family, ev_all, step = r["kernel_us_per_step"], r["step_us_sum_of_kernels"], r["step_us_one_batch_in_flight"]
    share, fam = bench.family_time(ev_family, ev_all, step)
    assert 0.9 < share <= 1.0 and fam <= step and abs(fam - ev_family / ev_all * step) < 1e-9
    import pytest
    with pytest.raises(ValueError, match="inconsistent profile"):  # a share above one is an error, not something to clamp
        bench.family_time(10.0, 5.0, 100.0)
    # and every line committed from round 5 on keeps the inequality
    for name in sorted(os.listdir(os.path.join(ROOT, "profiles"))):
        if name.startswith("r05_") and name.endswith(("bench.json", "bench20.json")):
            raw = open(os.path.join(ROOT, "profiles", name)).read().strip()
            if len(raw.splitlines()) != 1:
                continue
            line = json.loads(raw)
            roof = line["roofline"]
            assert roof["kernel_us_per_step"] <= roof["step_us_one_batch_in_flight"] * (1 + 1e-9), name
            assert "fabric_bytes_per_step" in roof and "hbm_frac" not in roof, name
            assert abs(roof["whole_network_frac"] - line["value"] * 451538432 / 2500e12) < 2e-3, name


def test_the_round_6_line_carries_what_round_5s_review_asked_for():
    """profiles/r06_final_bench*.json: the raw event-based family time and fraction next to the share-based ones, and the host-to-host
    ring timed over exactly the driver's --steps next to the >= 100-step figure"""
    for name, steps in (("r06_final_bench.json", 200), ("r06_final_bench20.json", 20)):
        line = json.loads(open(os.path.join(ROOT, "profiles", name)).read())
        roof, host = line["roofline"], line["host_inclusive"]
        ev = roof["events"]
        assert ev["family_us_per_step"] >= roof["kernel_us_per_step"] and abs(ev["frac"] * ev["family_us_per_step"] / (roof["frac"] * roof["kernel_us_per_step"]) - 1) < 1e-3
        assert line["steps"] == steps and host["at_driver_steps"]["steps"] == steps and host["steps"] == max(steps, 100)
        assert 0.8 < host["at_driver_steps"]["value"] / host["value"] < 1.2
        assert "page_locked" not in json.dumps(line) and "registered_source" not in json.dumps(line)  # no page-locked legs any more


def test_the_round_5_collections_are_consistent():
    """profiles/r05_g_*, r05_final_* and r06_final_* (round 6 changed no kernel of the product path): one parseable line under 4 KB, value / ms_per_step / roofline on the
    same leg, the family's time inside the step, fabric-byte names, and the roofline fraction recomputed from the rocprofv3 kernel statistics
    of the same box within 3 % (eight convolution launches per step: five direct / stride-2 kernels and three on the F(2,3) form)"""
    import csv
    for tag in ("r05_g", "r05_final", "r06_final"):
        for name in (f"{tag}_bench.json", f"{tag}_bench20.json"):
            raw = open(os.path.join(ROOT, "profiles", name)).read().strip()
            assert len(raw.splitlines()) == 1 and len(raw) <= 4096, (name, len(raw))
            line = json.loads(raw)
            assert line["n_gpus"] == 1 and line["config"]["batches_in_flight"] == 1 and line["higher_is_better"] is True
            assert abs(line["value"] * line["ms_per_step"] / 1e3 / line["config"]["windows_per_step"] - 1) < 1e-3
            roof = line["roofline"]
            assert roof["bound"] == "mfma" and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
            assert abs(roof["step_us_one_batch_in_flight"] / (1e3 * line["ms_per_step"]) - 1) < 1e-3
            assert roof["kernel_us_per_step"] <= roof["step_us_one_batch_in_flight"]
            assert abs(roof["whole_network_frac"] - line["value"] * 451538432 / 2500e12) < 1e-3
            assert line["cpu_baseline"]["kind"] == "reference" and line["gt_concordance"]["gt21_differ"] == 0
        line = json.loads(open(os.path.join(ROOT, "profiles", f"{tag}_bench.json")).read())
        traffic = json.load(open(os.path.join(ROOT, "profiles", f"{tag}_pmc_traffic.json")))
        assert 0.5 < traffic["l2_hit_rate"] < 1.0 and traffic["fabric_bytes_per_step"] > 0
        stats = {r["Name"]: (int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(os.path.join(ROOT, "profiles", f"{tag}_kernel_stats_fa_one_in_flight.csv")))}
        conv = {k: v for k, v in stats.items() if "conv3x3_planes_kernel" in k or "conv3x3_wino_planes_kernel" in k or "conv3x3_s2_planes_kernel" in k}
        assert len(conv) == 8 and len({c for c, _ in conv.values()}) == 1 and sum("wino" in k for k in conv) == 3
        conv_us = sum(avg for _, avg in conv.values()) / 1e3
        frac_csv = 449_418_240 * line["config"]["windows_per_step"] / (conv_us * 1e-6) / 2500e12
        # a traced run is a slower run (2 - 3 % lower clocks under the profiler): the like-for-like figure is the CSV's fraction scaled to the
        # un-traced step (tools/roofline_check.py).  Round 6's box (a fast one: 790 k) is 3.5 % apart unscaled, 1 % scaled; and the CSV must lie
        # between the line's raw event-based fraction (every launch bracketed: too long) and its share-based one
        all_us = sum(c * avg for k, (c, avg) in stats.items() if k.startswith(("void c3::", "c3::"))) / next(iter(conv.values()))[0] / 1e3
        scaled = frac_csv * all_us / (1e3 * line["ms_per_step"])
        assert min(abs(frac_csv / line["roofline"]["frac"] - 1), abs(scaled / line["roofline"]["frac"] - 1)) < 0.03, (tag, frac_csv, scaled, line["roofline"]["frac"])
        if "events" in line["roofline"]:
            assert line["roofline"]["events"]["frac"] < frac_csv < line["roofline"]["frac"] * 1.01, (tag, line["roofline"]["events"]["frac"], frac_csv)


@pytest.mark.gpu
def test_a_plain_run_times_the_headline_alone_and_dumps_its_rows(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: one block of exactly K steps of the headline workload, the line
    without the legs that belong to --full, no record file; --dump-outputs writes the rows of the last timed step, which are the
    oracle's rows of the seeded weights and windows"""
    import subprocess
    import sys
    import numpy as np
    from clair3_amd import synthetic as syn
    from oracle import oracle
    env = dict(os.environ, C3_BENCH_FULL=str(tmp_path / "full.json"))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "candidate-windows/sec" and line["unit"] == "candidate-windows/s" and line["higher_is_better"] is True
    assert line["steps"] == 7 and line["warmup"] == 2 and line["value_stats"]["repeats"] == 1 and line["dtype"] == "f32(fp16x3)"
    assert abs(line["value"] * line["ms_per_step"] / 1e3 / line["config"]["windows_per_step"] - 1) < 1e-3
    for key in ("roofline", "host_inclusive", "cpu_baseline", "gt_concordance", "pileup", "full_alignment_dwell", "3_batches_in_flight"):
        assert key not in line, key
    assert line["full_record"] is None and not (tmp_path / "full.json").exists()
    assert sorted(os.listdir(tmp_path / "out")) == ["full_alignment.npy"]
    y = np.load(tmp_path / "out" / "full_alignment.npy")
    assert y.dtype == np.float32 and y.shape == (256, 90)
    kind = syn.FULL_ALIGNMENT
    x = syn.make_windows(kind, 256, seed=1000, channels=8)[:16]  # rows are per window: a slice keeps the fp64 oracle quick
    y_ref = oracle.forward(kind, syn.make_state_dict(kind, 8, True, seed=0), x, True)
    assert float(np.abs(y[:16] - y_ref).max()) < 1e-4
