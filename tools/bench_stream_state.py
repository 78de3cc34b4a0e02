"""Stream state records on one MI355X: what export and move cost against a plain device copy of the same
records, and what a compaction pass buys a masked step at 50 % participation.

    python tools/bench_stream_state.py [--streams 131072] [--n 16384] [--out profiles/stream_state_bench.jsonl]

1. Throughput.  `oww_state_export` into a device buffer and `oww_move_streams`, for (a) n random streams and (b) n streams as whole
   32-stream blocks.  Yardstick, same process: hipMemcpyAsync device-to-device of n x record_bytes (what park_state does).  Allowed
   time = yardstick x (bytes the call must touch / 2 n record_bytes) + the yardstick's own spread over the five alternating rounds.
   The bytes come from the layout (history lengths and streams per group block are read from csrc/owwhip_layout.h) with 128-byte
   requests: a listed stream drags in its whole group block for every grouped array unless its group mates are listed too.
   Times are GPU times: events on the handle's stream behind a filler that keeps the stream busy while the host builds and queues
   the call, so the host's list building is not in them; `wall_ms` is the whole call from the host, synchronised either side.
2. Compaction.  A masked step with a fixed random half of the streams taking part; the same number of participants in whole blocks
   (the fan-in server's cohort placement) as the second yardstick; then one `oww_move_streams` call that swaps the participants
   into the blocks that already hold most of them, and the masked step again."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

LINE = 128                     # bytes per memory request


def layout_constants():
    src = open(os.path.join(ROOT, "openwakeword_amd", "csrc", "owwhip_layout.h")).read()

    def arr(name):
        m = re.search(name + r"\[N_STATE\]\s*=\s*\{([^}]*)\}", src)
        return [int(x) for x in m.group(1).split(",")]
    return arr("kStateLenRr"), arr("kStateSpgRr")


def bytes_model(ids, n_labels, feature_ring):
    """(live bytes touched, useful live bytes) of one export of the listed streams: a grouped array is touched by whole group blocks
    (every block that holds a listed stream, once), everything else by the stream's own bytes in 128-byte requests."""
    lens, spg = layout_constants()
    ids = np.asarray(ids, dtype=np.int64)
    up = lambda b: (b + LINE - 1) // LINE * LINE
    whole_lines = len(np.unique(ids // 32)) * 32 == len(ids)              # neighbours share the partly used requests
    touched = useful = 0
    for n, g in zip(lens, spg):
        useful += 4 * n * len(ids)
        touched += 4 * n * g * len(np.unique(ids // g)) if g > 1 else up(4 * n) * len(ids)
    for b in [960, 4 * 96 * feature_ring, 4 * 30 * n_labels, 4 * n_labels, 4 * n_labels, 4, 4, 32, 4]:
        useful += b * len(ids)
        touched += (b if whole_lines else up(b)) * len(ids)
    return touched, useful


def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    return C.CDLL("libamdhip64.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=131072)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_state_bench.jsonl"))
    args = ap.parse_args()
    import torch
    from openwakeword_amd import _lib, weights as W
    from openwakeword_amd.engine import StreamEngine
    S, n = args.streams, args.n
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    heads = {k: W.synthetic_head(k, 1234) for k in ("alexa", "hey_mycroft", "hey_jarvis")}
    eng = StreamEngine(S, heads, W.synthetic_embedding(1234), use_mfma=3, hip_stream=stream.cuda_stream)
    lib = _lib.load()
    build = lib.oww_build_info().decode()
    nb, fp = eng.state_info()
    rng = np.random.default_rng(16)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rec = torch.zeros(n * nb, dtype=torch.uint8, device=dev)
    rec2 = torch.zeros(n * nb, dtype=torch.uint8, device=dev)
    filler = torch.empty(1 << 30, dtype=torch.float32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pcm = (torch.randn(2, S, 1280, device=dev) * 3000).to(torch.int16)
    scores = torch.zeros(S, eng.n_labels, device=dev)
    for i in range(4):
        eng.step_device(pcm[i % 2].data_ptr(), 1, scores.data_ptr())
    torch.cuda.synchronize(dev)

    def gpu_ms(fn):
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            for _ in range(3):
                filler.zero_()
            e0.record(stream)
        fn()
        with torch.cuda.stream(stream):
            e1.record(stream)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def wall_ms(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0)

    lone = rng.choice(S, n, replace=False).astype(np.int32)
    lone_dst = rng.permutation(np.setdiff1d(np.arange(S), lone))[:n].astype(np.int32)
    blocks = rng.choice(S // 32, 2 * (n // 32), replace=False)
    whole = (blocks[: n // 32, None] * 32 + np.arange(32)).ravel().astype(np.int32)
    whole_dst = (blocks[n // 32:, None] * 32 + np.arange(32)).ravel().astype(np.int32)
    legs = {
        "memcpy_d2d": lambda: hip.hipMemcpyAsync(rec2.data_ptr(), rec.data_ptr(), n * nb, 3, stream.cuda_stream),
        "export_lone": lambda: eng.export_state_device(lone, rec.data_ptr()),
        "export_blocks": lambda: eng.export_state_device(whole, rec.data_ptr()),
        "move_lone": lambda: eng.move_streams(lone, lone_dst),
        "move_blocks": lambda: eng.move_streams(whole, whole_dst),
    }
    for fn in legs.values():                               # first use: layout table, staging buffers
        fn()
    torch.cuda.synchronize(dev)
    times = {k: {"gpu_ms": [], "wall_ms": []} for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k]["gpu_ms"].append(round(gpu_ms(fn), 4))
            times[k]["wall_ms"].append(round(wall_ms(fn), 4))
    yard = times["memcpy_d2d"]["gpu_ms"]
    spread = max(yard) - min(yard)
    t1, u1 = bytes_model(lone, eng.n_labels, eng.feature_ring)
    t32, u32 = bytes_model(whole, eng.n_labels, eng.feature_ring)
    out = {"what": "throughput", "build": build, "streams": S, "n": n, "record_bytes": nb, "fingerprint": f"{fp:016x}",
           "live_bytes": {"lone": {"touched": t1, "useful": u1}, "whole_blocks": {"touched": t32, "useful": u32}},
           "yardstick_gpu_ms": {"mean": round(float(np.mean(yard)), 4), "min": min(yard), "max": max(yard)}, "legs": {}}
    for k in legs:
        if k == "memcpy_d2d":
            out["legs"][k] = times[k]
            continue
        touched = t1 if k.endswith("lone") else t32
        ratio = (touched + n * nb) / (2.0 * n * nb) * (2 if k.startswith("move") else 1)      # a move gathers and scatters
        g = times[k]["gpu_ms"]
        allowed = float(np.mean(yard)) * ratio + spread
        out["legs"][k] = dict(times[k], mean_gpu_ms=round(float(np.mean(g)), 4), bytes_ratio=round(ratio, 4), allowed_ms=round(allowed, 4),
                              met=bool(np.mean(g) <= allowed), gb_per_s=round((touched + n * nb) * (2 if k.startswith("move") else 1) / np.mean(g) / 1e6, 1))
    lines = [out]
    print(json.dumps(out))

    # ---- 2. what compaction buys a masked step at 50 % participation
    eng.reset()
    on = np.zeros(S, np.uint8)
    on[rng.choice(S, S // 2, replace=False)] = 1
    cohort = np.zeros(S, np.uint8)
    cohort[(rng.choice(S // 32, S // 64, replace=False)[:, None] * 32 + np.arange(32)).ravel()] = 1

    def masked_ms(mask, steps=20):
        for i in range(5):
            eng.step_masked_device(pcm[i % 2].data_ptr(), mask, scores.data_ptr())
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(steps):
            eng.step_masked_device(pcm[i % 2].data_ptr(), mask, scores.data_ptr())
        torch.cuda.synchronize(dev)
        return round(1e3 * (time.perf_counter() - t0) / steps, 4)

    before = [masked_ms(on)]
    yard_cohort = [masked_ms(cohort)]
    before.append(masked_ms(on))
    yard_cohort.append(masked_ms(cohort))
    # participants into the blocks that hold most of them: every participant outside swaps with a non-participant inside
    per_block = on.reshape(-1, 32).sum(1)
    takers = np.zeros(S // 32, bool)
    takers[np.argsort(-per_block, kind="stable")[: S // 64]] = True
    inside = np.repeat(takers, 32)
    out_part = np.nonzero((on == 1) & ~inside)[0]
    in_idle = np.nonzero((on == 0) & inside)[0]
    assert len(out_part) == len(in_idle)
    src = np.concatenate([out_part, in_idle]).astype(np.int32)
    dst = np.concatenate([in_idle, out_part]).astype(np.int32)
    move_wall = wall_ms(lambda: eng.move_streams(src, dst))
    after_mask = inside.astype(np.uint8)
    after = [masked_ms(after_mask), masked_ms(after_mask)]
    gain = float(np.mean(before) - np.mean(after))
    out2 = {"what": "compaction", "build": build, "streams": S, "participation": 0.5,
            "masked_step_ms": {"random_before": before, "cohort_yardstick": yard_cohort, "after_compaction": after},
            "move": {"streams_moved": int(len(src)), "wall_ms": round(move_wall, 4)},
            "steps_to_pay_back": round(move_wall / gain, 1) if gain > 0 else None,
            "scores_valid": bool(torch.isfinite(scores).all().item()) and not eng.range_status()}
    lines.append(out2)
    print(json.dumps(out2))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
