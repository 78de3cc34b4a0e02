"""Cost of detection events (include/owwhip.h: oww_events_*) per step at 131,072 streams x 3 heads, capacity 4,096, 16 snapshot rows:
  off        the same handle shape without events -- the launches and the step time of a handle that never asked
  yardstick  postproc_kernel alone: a handle whose post-processing does not ride in the heads launch (a handle-wide verifier whose
             threshold no raw score reaches keeps it a launch of its own); it reads the same raw scores plus the 30-deep ring
  rare       events on, thresholds at the 0.995 quantile of each label's scores: <= 1 % of the pairs hit
  half       events on, thresholds at the median: 50 % of the pairs hit (far beyond the capacity: n_stored = 4,096 < n_total)
  rare0, half0  the same two without snapshots (feature_rows = 0): what is left of events_write_kernel is the base reduction, the
             ranking and the record stores, so the difference to rare / half is the snapshot walk
Time = kernel class 7 (post-processing; the two event launches are counted there) of oww_kernel_times over --steps steps, per step;
on the default three sigmoid heads post-processing rides in the heads launch, so class 7 of `rare` / `half` is the two event kernels
alone.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_events.py` (a run of its own, no counters) the trace names
events_count_kernel, events_write_kernel and postproc_kernel separately.  Bytes model per step: pairs x 4 B read by each of the two
kernels + (32 + rows x 384) B written and rows x 384 B read per stored hit.  Prints one JSON line per setting."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["alexa", "hey_mycroft", "weather"]
QUANTILE = {"rare": 0.995, "half": 0.5, "rare0": 0.995, "half0": 0.5}


def run(setting: str, S: int, steps: int, warmup: int, capacity: int, rows: int) -> dict:
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    heads = {n: W.synthetic_head(n, 1234) for n in NAMES}
    events = setting in QUANTILE
    if setting.endswith("0"):
        rows = 0
    eng = StreamEngine(S, heads, W.synthetic_embedding(3), **(dict(event_capacity=capacity, event_features=rows) if events else {}))
    if setting == "yardstick":
        eng.set_verifier(0, np.zeros(16 * 96, np.float32), 0.0, threshold=2.0)
    rng = np.random.default_rng(1)
    pcm = [(rng.standard_normal((S, 1280)) * 3000).astype(np.int16) for _ in range(4)]
    # past the five zeroed predictions and until the 16-row feature rings hold rows of this audio only: the scores drift until then,
    # and thresholds taken earlier would not give the hit rate asked for.  Then one pass over the PCM pool for the quantiles.
    for i in range(max(warmup, 24)):
        eng.step(pcm[i % 4])
    thr = None
    if events:
        pool = np.concatenate([eng.step(pcm[i % 4]).copy() for i in range(4)])
        thr = np.quantile(pool, QUANTILE[setting], axis=0).astype(np.float32)
        eng.set_event_thresholds(thr)
    eng.sync()
    eng.kernel_times()
    eng.enable_timing(True)
    hits, stored = [], []
    t0 = time.perf_counter()
    for i in range(steps):
        eng.step(pcm[i % 4])
        if events:
            rec, total = eng.events()
            hits.append(total)
            stored.append(len(rec))
    eng.sync()
    wall = (time.perf_counter() - t0) / steps
    kt = eng.kernel_times()
    pairs = S * len(NAMES)
    res = {"setting": setting, "streams": S, "pairs": pairs, "steps": steps,
           "class7_ms_per_step": round(kt["postproc"]["ms"] / steps, 5), "class7_launches_per_step": kt["postproc"]["launches"] / steps,
           "launches_per_step": {k: v["launches"] / steps for k, v in kt.items() if v["launches"]},
           "kernel_ms_per_step": round(sum(v["ms"] for v in kt.values()) / steps, 4), "wall_ms_per_step_timed": round(wall * 1e3, 3),
           "build": eng._lib.oww_build_info().decode()}
    if events:
        n_st = float(np.mean(stored))
        res.update({"capacity": capacity, "feature_rows": rows, "thresholds": [float(v) for v in thr],
                    "hit_fraction": round(float(np.mean(hits)) / pairs, 5), "n_total_mean": float(np.mean(hits)), "n_stored_mean": n_st,
                    "bytes_model": {"score_reads": 2 * pairs * 4, "hit_writes": int(n_st * (32 + rows * 384)), "hit_reads": int(n_st * rows * 384)}})
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--settings", default="off,yardstick,rare,half,rare0,half0")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for s in a.settings.split(","):
        line = json.dumps(run(s, a.streams, a.steps, a.warmup, a.capacity, a.rows))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
