"""Routed head-bank launch alone (include/owwhip.h: oww_bank_*), per step, at 131,072 streams:
  fixed3  the fixed 3-head launch (alexa, hey_mycroft, weather as fixed heads, no bank) -- the yardstick of (a)
  a       1 slot, subscriptions spread over the same 3 nets in the bank (bank-only handle)
  b       1,024 heads x 128 streams
  c       4,096 heads x 32 streams
  d       the routing of (b) issued as one launch per head (library built with -DOWH_BANK_PER_HEAD=1; --per-head-lib)
Time = kernel class 6 (heads) of oww_kernel_times over --steps steps after --warmup, per step.  Bytes model per step: first-layer
weights streamed once per tile (oww_bank_routing) + every entry's T x 96 fp32 feature rows; the tail weights (w2 and the per-unit
arrays, < 70 KB per head) are left out.  Prints one JSON line per setting."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(setting: str, S: int, steps: int, warmup: int) -> dict:
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    emb = W.synthetic_embedding(3)
    names = ["alexa", "hey_mycroft", "weather"]
    t0 = time.time()
    if setting == "fixed3":
        eng = StreamEngine(S, {n: W.synthetic_head(n, 1234) for n in names}, emb)
    else:
        n_heads = {"a": 3, "b": 1024, "c": 4096, "d": 1024}[setting]
        eng = StreamEngine(S, {}, emb, bank_slots=1, bank_capacity=n_heads)
        for i in range(n_heads):
            h = W.synthetic_head(names[i], 1234) if setting == "a" else W.synthetic_head(f"bank{i}", 100 + i)
            eng.bank_add(h)
        eng.subscribe(np.arange(S), (np.arange(S) % n_heads)[:, None].astype(np.int32))
    t_setup = time.time() - t0
    rng = np.random.default_rng(1)
    pcm = [(rng.standard_normal((S, 1280)) * 3000).astype(np.int16) for _ in range(4)]
    for i in range(warmup):
        eng.step(pcm[i % 4])
    eng.sync()
    eng.kernel_times()
    eng.enable_timing(True)
    for i in range(steps):
        eng.step(pcm[i % 4], out=None)
    eng.sync()
    kt = eng.kernel_times()
    ms = kt["heads"]["ms"] / steps
    res = {"setting": setting, "streams": S, "steps": steps, "heads_ms_per_step": round(ms, 4),
           "launches_per_step": kt["heads"]["launches"] / steps, "setup_s": round(t_setup, 1),
           "build": eng._lib.oww_build_info().decode()}
    if setting != "fixed3":
        r = eng.bank_routing()
        entries, tiles, wg = sum(r["entries"]), sum(r["tiles"]), max(r["waves_per_tile"])
        feat_bytes = entries * 16 * 96 * 4
        res.update({"tiles": r["tiles"], "waves_per_tile": r["waves_per_tile"], "entries": entries,
                    "tile_occupancy": round(entries / max(1, sum(t * 32 * w for t, w in zip(r["tiles"], r["waves_per_tile"]))), 3),
                    "weight_bytes": r["weight_bytes"], "feature_bytes": feat_bytes,
                    "bytes_model_GBps": round((r["weight_bytes"] + feat_bytes) / (ms * 1e-3) / 1e9, 1)})
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settings", default="fixed3,a,b,c,d")
    ap.add_argument("--per-head-lib", default=os.path.join(ROOT, "openwakeword_amd", "libowwhip_bank_per_head.so"))
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run(a.one, a.streams, a.steps, a.warmup)), flush=True)
        return
    for s in a.settings.split(","):
        env = dict(os.environ)
        if s == "d":
            if not os.path.exists(a.per_head_lib):
                from openwakeword_amd import _build
                _build.build(out=a.per_head_lib, defines=("OWH_BANK_PER_HEAD=1",))
            env["OWW_LIB"] = a.per_head_lib
        # one process per setting (a fresh device context; (d) loads the per-head build)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", s, "--streams", str(a.streams), "--steps", str(a.steps),
                            "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
