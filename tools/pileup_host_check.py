#!/usr/bin/env python3
"""The host form of pileup from reads under AddressSanitizer and UndefinedBehaviorSanitizer, on a CPU.

    python tools/pileup_host_check.py [--cxx g++]

Builds tools/pileup_host_check.cpp (the checks, the rule and the alt-info printer of csrc/c3_pileup_rule.h with a main of their own) with
-fsanitize=address,undefined into a temporary directory, replays the three golden read sets (tests/golden/pileup_reads.npz) and a generated
one with N ops, non-ACGT bases and D / I neighbours through it, and compares what it writes with the fixture's columns and with the library's
own c3_pileup_reads_host; then runs the program's refused inputs.  Nothing here touches a GPU, and nothing is loaded into Python under a
sanitizer: the program is a process of its own, started in the environment this tool was started in.  It is meant for the CPU build box:
where that environment preloads a library into every process, the sanitizer's runtime refuses to start and the tool fails with its
message.  Exit status 0: every case agreed and the sanitizers reported nothing.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clair3_amd import pileup_reads as pr, synthetic as syn  # noqa: E402

FIELDS = ("pos", "flag", "mapq", "cigar_first", "cigar", "seq_first", "seq")


def dump(rs, path):
    arrays = {name: np.ascontiguousarray(rs[name], dtype=dt) for name, dt in pr.ReadSet.FIELDS}
    ref = np.ascontiguousarray(rs["ref_bytes"], dtype=np.uint8)
    head = np.array([len(arrays["pos"]), len(arrays["cigar"]), len(arrays["seq"]), rs["start"], rs["end"], rs["ref_first"], len(ref)], np.int64)
    with open(path, "wb") as fh:
        fh.write(head.tobytes())
        for name in FIELDS:
            fh.write(arrays[name].tobytes())
        fh.write(ref.tobytes())


def load(path):
    blob = open(path, "rb").read()
    n_cols, n_cand = np.frombuffer(blob[:16], np.int64)
    at = 16
    matrix = np.frombuffer(blob[at:at + n_cols * 72], np.int32).reshape(-1, 18)
    at += n_cols * 72
    major = np.frombuffer(blob[at:at + n_cols * 8], np.int64)
    return matrix, major, blob[at + n_cols * 8:], int(n_cand)


def main():
    cxx = sys.argv[sys.argv.index("--cxx") + 1] if "--cxx" in sys.argv else os.environ.get("CXX", "g++")
    cases = []
    with np.load(os.path.join(ROOT, "tests", "golden", "pileup_reads.npz")) as z:
        for k in range(int(z["n_sets"])):
            rs = {name: z[f"{k}_{name}"] for name in FIELDS}
            rs.update(start=int(z[f"{k}_start"]), end=int(z[f"{k}_end"]), ref_bytes=z[f"{k}_ref"], ref_first=int(z[f"{k}_ref_first"]))
            cases.append((f"golden set {k}", rs, (100, 1), z[f"{k}_channels"], z[f"{k}_major"]))
    odd = syn.make_read_set(n_sites=500, depth=30, read_len=(150, 600), seed=41, n_op=0.003, non_acgt=0.03, d_then_i=0.004, i_then_d=0.004, pad=0.2,
                            eqx=True, gaps=2, ref_other=0.03)
    cases.append(("generated, every kind of op", odd, (3, 0), None, None))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pileup_host_check")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tools", "pileup_host_check.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        for what, rs, (max_indel, call_ht), channels, major in cases:
            dump(rs, os.path.join(tmp, "case.bin"))
            subprocess.check_call([exe, os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin"), str(max_indel), str(call_ht)], env=env)
            got_m, got_major, got_text, n_cand = load(os.path.join(tmp, "out.bin"))
            want = pr.pileup_counts(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], path="host", max_indel_length=max_indel, call_ht=bool(call_ht))
            assert np.array_equal(got_m, want[0]) and np.array_equal(got_major, want[1]), what
            assert got_text.decode() == "".join(x + "\n" for x in want[2]) and n_cand == len(want[2]), what
            if channels is not None:
                assert np.array_equal(got_m, channels) and np.array_equal(got_major, major), what + ": the fixture's columns"
            print(f"{what}: {len(got_major)} columns, {n_cand} candidates, {len(got_text)} bytes of text: equal, no report")
        subprocess.check_call([exe, "--errors"], env=env)
    print("pileup host form under -fsanitize=address,undefined: clean")
    return 0


if __name__ == "__main__":
    sys.exit(main())
