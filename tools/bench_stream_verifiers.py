#!/usr/bin/env python3
"""Launch cost of the per-stream custom verifiers.

131,072 streams x 3 heads (alexa, hey_mycroft, hey_jarvis); every stream's alexa column is verified, by
  wide     one verifier handle-wide (oww_set_verifier -> verifier_kernel: the yardstick),
  pool1    the same verifier assigned to every stream from a pool of one (stream_verifier_kernel),
  pool1024 1,024 distinct verifiers, stream s assigned verifier s % 1024 (stream_verifier_kernel).
The audio is the 8-stream Gaussian PCM of tests/test_stream_verifiers_gpu.py tiled over the streams; 40 steps, the first 10 discarded.

  python tools/bench_stream_verifiers.py run --mode pool1024 --thr 0.5        (run under rocprofv3 --kernel-trace --stats)
  python tools/bench_stream_verifiers.py summarize OUT.jsonl DIR:MODE:THR ...  (one rocprofv3 output directory per run)

`run` prints one JSON line: evaluations per timed step (counted by the pool kernel; the handle-wide runs take the count of the pool
runs on the same inputs).  `summarize` reads each directory's kernel trace, takes the verifier kernel's durations of the timed steps and
writes one JSON line per run with the bytes model: extra bytes = evaluations x T x 96 x 4 over the yardstick's time at 6.3 TB/s."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np                                           # noqa: E402

S, STEPS, SKIP, T = 131072, 40, 10, 16
HBM = 6.3e12                                                 # achievable HBM bytes/s
KERNELS = {"wide": "verifier_kernel", "pool1": "stream_verifier_kernel", "pool1024": "stream_verifier_kernel"}


def verifiers(n):
    from openwakeword_amd.model import fold_verifier
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
    from verifier_fixture import trained_verifier
    base = [fold_verifier(trained_verifier(seed)) for seed in range(min(n, 8))]
    return [((base[i % len(base)][0] * np.float32(1.0 + i / 4096.0)).astype(np.float32), base[i % len(base)][1]) for i in range(n)]


def run(mode, thr):
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
    from golden import cases
    heads = {n: W.synthetic_head(n, cases.SEED_WEIGHTS) for n in ("alexa", "hey_mycroft", "hey_jarvis")}
    n_ver = {"wide": 1, "pool1": 1, "pool1024": 1024}[mode]
    pool = verifiers(n_ver)
    e = StreamEngine(S, heads, W.synthetic_embedding(cases.SEED_WEIGHTS), verifier_capacity=0 if mode == "wide" else n_ver)
    if mode == "wide":
        e.set_verifier(0, pool[0][0], pool[0][1], thr)
    else:
        ids = np.array([e.verifier_add(w, b) for w, b in pool], np.int32)
        e.assign_verifiers(0, np.arange(S), ids[np.arange(S) % n_ver], np.full(S, thr, np.float32))
    base = W.synthetic_pcm(8, STEPS * 1280, seed=0xA11CE, rms=3000.0)
    evals = []
    for t in range(STEPS):
        x = np.ascontiguousarray(np.tile(base[:, t * 1280:(t + 1) * 1280], (S // 8, 1)))
        e.step(x)
        if t >= SKIP:
            evals.append(e.verifier_stats()[1])
    e.close()
    print(json.dumps({"mode": mode, "thr": thr, "evals_per_step": float(np.mean(evals)) if mode != "wide" else None}))


def kernel_durations(d, name):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"{d}: no kernel trace")
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                kn = r.get("Kernel_Name", "")
                if name + "(" in kn or kn.endswith(name) or ("::" + name) in kn:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    return [ns for _, ns in rows]


def summarize(out, runs):
    recs = []
    for spec in runs:
        d, mode, thr, evals = spec.split(":")
        ns = kernel_durations(d, KERNELS[mode])
        timed = ns[-(STEPS - SKIP):]
        recs.append({"mode": mode, "thr": float(thr), "kernel": KERNELS[mode], "launches": len(ns),
                     "mean_us": float(np.mean(timed)) / 1e3, "min_us": float(np.min(timed)) / 1e3, "evals_per_step": float(evals)})
    for r in recs:
        wide = [w["mean_us"] for w in recs if w["mode"] == "wide" and w["thr"] == r["thr"]]
        extra = r["evals_per_step"] * T * 96 * 4
        r["wide_mean_us"] = [round(x, 3) for x in wide]
        r["wide_spread_us"] = round(max(wide) - min(wide), 3) if wide else None
        r["extra_weight_bytes"] = extra
        r["allowed_us"] = round(max(wide) + extra / HBM * 1e6, 3) if wide else None
        r["bytes_model_tb_s"] = round(2 * extra / (r["mean_us"] * 1e-6) / 1e12, 3)     # feature rows + weights per re-scored pair
        r["within_margin"] = (r["mean_us"] <= r["allowed_us"]) if wide and r["mode"] != "wide" else None
    with open(out, "a") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--mode", choices=sorted(KERNELS), required=True)
    r.add_argument("--thr", type=float, required=True)
    s = sub.add_parser("summarize")
    s.add_argument("out")
    s.add_argument("runs", nargs="+", help="DIR:MODE:THR:EVALS_PER_STEP")
    a = ap.parse_args()
    if a.cmd == "run":
        run(a.mode, a.thr)
    else:
        summarize(a.out, a.runs)
