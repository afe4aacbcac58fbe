#!/usr/bin/env python3
"""Serve mode's rate from client to client (clair3_amd/serve.py; needs an MI355X): one server child with both networks, K client processes
that each send the CPU branch's batches -- predictBatchSize x threads = 800 windows, one blocking call per batch, as the reference's loop makes
them (clair3/CallVariantsFromCffi.py:266,276-296) -- and windows/s over all clients from the first request sent to the last answer read.
Behind every K: the per-request times a client sees (segment, answer, rows) and where the server's own time went (map, stage, wait, reply).

usage: serve_throughput.py [REQUESTS=40 per full-alignment client, five times as many per pileup client] [K ...=1 4 12]          (the rates of bench.py --full's host_inclusive leg stand next to these in
profiles/serve_mode.txt: same job, parent commit, alternating)"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from clair3_amd import client  # noqa: E402

BATCH = 800
TIMEOUT = 300


def client_main(sock, name, requests, go_at):
    """one CPU worker's model calls: warm up, wait for the common start, then `requests` blocking calls"""
    from clair3_amd import synthetic as syn
    kind = syn.PILEUP if name == "pileup" else syn.FULL_ALIGNMENT
    x = syn.make_windows(kind, BATCH, seed=os.getpid() % 1000)
    if name == "pileup":
        x = x.astype(np.int32)  # the CPU branch's pileup tensors are int32 (the Triton branch: INT32)
    m = client.RemoteModel(sock, name)
    for _ in range(2):
        m.predict_numpy(x)
    while time.time() < go_at:
        time.sleep(0.0005)
    t = dict(segment=0.0, answer=0.0, rows=0.0)
    t_start = time.time()
    for _ in range(requests):
        t0 = time.perf_counter()
        pending = m.send(x)
        t1 = time.perf_counter()
        m._conn.receive("predict")
        t2 = time.perf_counter()
        seg, n, yoff = pending
        y = seg.array(np.float32, (n, m.row_size), yoff).copy()
        seg.close()
        t3 = time.perf_counter()
        t["segment"] += t1 - t0
        t["answer"] += t2 - t1
        t["rows"] += t3 - t2
    assert np.isfinite(y).all()
    print(json.dumps(dict(start=t_start, end=time.time(), **t)), flush=True)


def main():
    requests = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    ks = [int(a) for a in sys.argv[2:]] or [1, 4, 12]
    from clair3_amd import synthetic as syn
    from tests import refloop
    with tempfile.TemporaryDirectory() as d:
        sock = os.path.join(d, "c3.sock")
        for name, kind, channels in (("pileup", syn.PILEUP, 18), ("alignment", syn.FULL_ALIGNMENT, 8)):
            refloop.write_checkpoint(os.path.join(d, name + ".pt"), kind, channels, True)
        env = dict(os.environ, PYTHONPATH=ROOT)
        server = subprocess.Popen([sys.executable, "-m", "clair3_amd.serve", "--socket", sock, "--model", f"pileup={d}/pileup", "--model",
                                   f"alignment={d}/alignment", "--add_indel_length"], env=env)
        try:
            end = time.time() + 120
            while True:
                assert server.poll() is None and time.time() < end, "the server did not come up"
                try:
                    client.control(sock, "hello", timeout=5)
                    break
                except client.ServerError:
                    time.sleep(0.05)
            for name in ("pileup", "alignment"):
                for k in ks:
                    n_each = requests * (5 if name == "pileup" else 1)  # (a pileup request takes a tenth of the time: the timed window stays long enough)
                    before = client.control(sock, "stats")["stats"][name]
                    go_at = time.time() + 3.0 + 0.1 * k
                    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--client", sock, name, str(n_each), repr(go_at)],
                                              env=env, stdout=subprocess.PIPE, text=True) for _ in range(k)]
                    outs = []
                    for p in procs:
                        out, _ = p.communicate(timeout=TIMEOUT)
                        assert p.returncode == 0, out
                        outs.append(json.loads(out.strip().splitlines()[-1]))
                    after = client.control(sock, "stats")["stats"][name]
                    span = max(o["end"] for o in outs) - min(o["start"] for o in outs)
                    n_req = k * n_each
                    sec = {key: after["seconds"][key] - before["seconds"][key] for key in after["seconds"]}
                    per = {key: 1e6 * sum(o[key] for o in outs) / n_req for key in ("segment", "answer", "rows")}
                    print(f"{name:9s} K={k:2d}: {n_req * BATCH / span:10.0f} windows/s  ({n_req} requests of {BATCH} in {span * 1e3:.1f} ms; passes for "
                          f"the timed requests and warm-ups: {after['passes'] - before['passes']}, largest pass {after['max_parts']} parts)\n"
                          f"    client, us per request: segment+send {per['segment']:.0f}  answer {per['answer']:.0f}  rows+unmap {per['rows']:.0f}\n"
                          f"    server, us per request (warm-ups included): map {1e6 * sec['map'] / (n_req + 2 * k):.0f}  stage {1e6 * sec['stage'] / (n_req + 2 * k):.0f}  "
                          f"wait {1e6 * sec['wait'] / (n_req + 2 * k):.0f}  reply {1e6 * sec['reply'] / (n_req + 2 * k):.0f}", flush=True)
        finally:
            try:
                client.control(sock, "shutdown", timeout=10)
                server.wait(timeout=30)
            except Exception:  # noqa: BLE001
                server.terminate()
                server.wait(timeout=30)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--client":
        client_main(sys.argv[2], sys.argv[3], int(sys.argv[4]), float(sys.argv[5]))
    else:
        main()
