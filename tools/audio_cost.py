"""Cost of the per-stream audio rings (include/owwhip.h: oww_audio_configure) per step, PCM and scores resident on the device:
  off          the same handle shape without audio and without events -- the step of a handle that never asked
  ring         audio_chunks = --ring: one audio_append_kernel launch behind every step
  events       events without audio (capacity --capacity, no feature rows), thresholds at the 0.995 quantile: 0.5 % of the pairs hit
  ring_events  ring + events + event_audio = --ring: the append, the two event launches and events_audio_kernel
Two figures per setting.  Wall: a host clock around --steps asynchronous oww_step calls that ends in a device synchronise, timing
off, --repeats windows with the settings alternating inside every repeat, so that a drift of the box lands on all of them.  Class 7:
oww_kernel_times over --steps further steps with timing on; on the default sigmoid heads post-processing rides in the heads launch,
so class 7 is the append (ring), the two event launches (events) or all four (ring_events): snapshot launch = ring_events - ring -
events.  Bytes model: the append reads and writes 2,560 B per stream and step, a snapshot launch reads and writes event_audio x
2,560 B per stored event.  Prints one JSON line per setting and shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["alexa", "hey_mycroft", "weather"]
SETTINGS = ("off", "ring", "events", "ring_events")


def make(setting, S, n_heads, ring, capacity):
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    heads = {n: W.synthetic_head(n, 1234) for n in NAMES[:n_heads]}
    kw = {}
    if setting in ("ring", "ring_events"):
        kw["audio_chunks"] = ring
    if setting in ("events", "ring_events"):
        kw["event_capacity"] = capacity
    if setting == "ring_events":
        kw["event_audio"] = ring
    return StreamEngine(S, heads, W.synthetic_embedding(3), **kw)


def run_shape(S, n_heads, a):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    host = [(rng.standard_normal((S, 1280)) * 3000).astype(np.int16) for _ in range(4)]
    pool = [torch.from_numpy(x).to(dev) for x in host]
    engines, scores, stats = {}, {}, {}
    for s in a.settings.split(","):
        eng = make(s, S, n_heads, a.ring, a.capacity)
        for i in range(max(a.warmup, 24)):                   # past the zeroed predictions, the feature rings full of this audio
            eng.step(host[i % 4])
        if s in ("events", "ring_events"):
            seen = np.concatenate([eng.step(host[i % 4]).copy() for i in range(4)])
            eng.set_event_thresholds(np.quantile(seen, 0.995, axis=0).astype(np.float32))
        scores[s] = torch.empty((S, eng.n_labels), dtype=torch.float32, device=dev)
        engines[s] = eng
        stats[s] = {"wall_ms": [], "hits": [], "stored": []}
    torch.cuda.synchronize()

    def window(eng, sc, steps):
        t0 = time.perf_counter()
        for i in range(steps):
            eng.step_device(pool[i % 4].data_ptr(), 1, sc.data_ptr())
        eng.sync()
        return (time.perf_counter() - t0) / steps * 1e3

    for s, eng in engines.items():                           # every shape warm on the device path
        window(eng, scores[s], 8)
    for _ in range(a.repeats):
        for s, eng in engines.items():
            stats[s]["wall_ms"].append(round(window(eng, scores[s], a.steps), 4))
    out = []
    for s, eng in engines.items():
        eng.kernel_times()
        eng.enable_timing(True)
        for i in range(a.steps):
            eng.step_device(pool[i % 4].data_ptr(), 1, scores[s].data_ptr())
            if s in ("events", "ring_events"):
                rec, total = eng.events()
                stats[s]["hits"].append(total)
                stats[s]["stored"].append(len(rec))
        eng.sync()
        kt = eng.kernel_times()
        eng.enable_timing(False)
        w = stats[s]["wall_ms"]
        res = {"setting": s, "streams": S, "heads": n_heads, "steps": a.steps, "repeats": a.repeats,
               "wall_ms_per_step": w, "wall_ms_mean": round(float(np.mean(w)), 4),
               "class7_ms_per_step": round(kt["postproc"]["ms"] / a.steps, 5), "class7_launches_per_step": kt["postproc"]["launches"] / a.steps,
               "kernel_ms_per_step": round(sum(v["ms"] for v in kt.values()) / a.steps, 4), "build": eng._lib.oww_build_info().decode()}
        if s in ("ring", "ring_events"):
            res.update({"ring_chunks": a.ring, "ring_bytes": S * a.ring * 2560, "append_bytes_per_step": 2 * 2560 * S})
        if s in ("events", "ring_events"):
            n_st = float(np.mean(stats[s]["stored"]))
            res.update({"capacity": a.capacity, "hit_fraction": round(float(np.mean(stats[s]["hits"])) / (S * n_heads), 5), "n_stored_mean": n_st})
            if s == "ring_events":
                res["snapshot_bytes_per_step"] = int(2 * n_st * a.ring * 2560)
        out.append(res)
    by = {r["setting"]: r for r in out}
    if "ring" in by:
        r = by["ring"]
        r["append_tb_per_s"] = round(r["append_bytes_per_step"] / (r["class7_ms_per_step"] * 1e-3) / 1e12, 3) if r["class7_ms_per_step"] else None
        if "off" in by:
            r["wall_over_off_ms"] = round(r["wall_ms_mean"] - by["off"]["wall_ms_mean"], 4)
    if {"ring", "events", "ring_events"} <= set(by):
        r = by["ring_events"]
        snap = r["class7_ms_per_step"] - by["ring"]["class7_ms_per_step"] - by["events"]["class7_ms_per_step"]
        r["snapshot_ms_per_step"] = round(snap, 5)
        r["snapshot_tb_per_s"] = round(r["snapshot_bytes_per_step"] / (snap * 1e-3) / 1e12, 3) if snap > 0 else None
    for eng in engines.values():
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="131072x3,4096x1", help="streams x heads, comma separated")
    ap.add_argument("--ring", type=int, default=25)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        S, n_heads = (int(v) for v in shape.split("x"))
        for res in run_shape(S, n_heads, a):
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
