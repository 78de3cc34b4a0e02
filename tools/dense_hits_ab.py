#!/usr/bin/env python3
"""Ordered hit lists of dense scoring on one MI355X: what oww_bank_score_hits costs per call against the two entries
a caller had before it, on the bank shapes of tools/dense_bank_ab.py -- 256 narrow bank heads (T = 16, 64 hidden units) over eight
sequences of 45,000 windows (eight hours), features resident on the device.

Three arms per hit rate (0, 1e-4 and 1e-2 of a head's windows; the thresholds are taken per head from the score matrix):
  hits    oww_bank_score_hits, cap 4096, windows into a device buffer: wall clock, class 6 (heads launches, the re-score included) and
          class 7 (mask compaction, gathers, score passes) of oww_kernel_times.
  stats   oww_bank_score_stats with the same thresholds: wall clock and class 6.
  matrix  oww_bank_score_features + the copy of its matrix into pinned host memory + numpy's nonzero on it: wall clock of each part.
tools/dense_bank_ab.py's protocol: warm-up rounds first, the arms alternating inside every repeat, medians.  At hit rate 0 no gather
and no re-score runs, so class 7 of the hits arm is the compaction pass alone and class 6 is the heads launch in its MASK mode.
The totals are checked against the statistics entry's counts.  Prints one JSON line; --out writes it to a file.

usage: python tools/dense_hits_ab.py [--heads 256] [--reps 5] [--out profiles/dense_hits_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

T = 16
RATES = (0.0, 1e-4, 1e-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=256)
    ap.add_argument("--windows", type=int, default=45000)
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from openwakeword_amd import _build, _lib
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import DENSE_HIT, KERNEL_CLASSES, StreamEngine, _ptr
    if not torch.cuda.is_available():
        raise SystemExit("dense_hits_ab.py measures on the GPU; none is visible")
    for k in ("OWW_DENSE_PATH", "OWW_DENSE_BANK_HPW", "OWW_DENSE_SLAB_MB"):
        os.environ.pop(k, None)

    H, B, NW, cap = args.heads, args.seqs, args.windows, args.cap
    bank = StreamEngine(B, {}, W.synthetic_embedding(1234), bank_slots=1, bank_capacity=H)
    ids = np.array([bank.bank_add(W.synthetic_head(f"bank{i}", 7000 + i, kind="binary", T=T, hidden=64, n_out=1, layernorm=True)) for i in range(H)],
                   np.int32)
    bank.enable_timing(True)
    lib = bank._lib
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    n_rows, N = NW + T - 1, B * NW
    feats = torch.randn(B, n_rows, 96, device="cuda", generator=gen)
    out = torch.zeros(B, NW, H, device="cuda")
    host = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
    off = bank.score_hits_layout(cap, ids)
    windows = torch.empty(int(off[-1]), device="cuda")
    hits = np.zeros((H, cap), DENSE_HIT)
    ns, nt = np.zeros(H, np.int32), np.zeros(H, np.int64)
    cnt, mx, am = np.zeros((B, H), np.int32), np.zeros((B, H), np.float32), np.zeros((B, H), np.int32)

    def classes():
        t = bank.kernel_times()
        return t[KERNEL_CLASSES[6]], t[KERNEL_CLASSES[7]]

    def run_matrix():
        t0 = time.perf_counter()
        _lib.check(lib.oww_bank_score_features(bank._h, feats.data_ptr(), 1, B, n_rows, _ptr(ids), H, out.data_ptr(), 1))
        return time.perf_counter() - t0

    def run_hits(thr):
        bank.kernel_times()
        t0 = time.perf_counter()
        _lib.check(lib.oww_bank_score_hits(bank._h, feats.data_ptr(), 1, B, n_rows, _ptr(ids), H, _ptr(thr), cap, hits.ctypes.data, _ptr(ns), _ptr(nt),
                                           windows.data_ptr(), 1))
        w = time.perf_counter() - t0
        c6, c7 = classes()
        return w, c6, c7

    def run_stats(thr):
        bank.kernel_times()
        t0 = time.perf_counter()
        _lib.check(lib.oww_bank_score_stats(bank._h, feats.data_ptr(), 1, B, n_rows, _ptr(ids), H, _ptr(thr), _ptr(cnt), _ptr(mx), _ptr(am)))
        w = time.perf_counter() - t0
        return w, classes()[0]

    run_matrix()
    flat = out.reshape(N, H)
    per_rate = {}
    for rate in RATES:
        k = int(round(rate * N))
        thr = np.full(H, 2.0, np.float32) if k == 0 else torch.topk(flat, k, dim=0).values[-1].cpu().numpy().astype(np.float32)
        for _ in range(args.warmup):
            run_hits(thr); run_stats(thr); run_matrix(); host.copy_(out); torch.cuda.synchronize()
        r = {"hits_wall": [], "hits_c6": [], "hits_c7": [], "stats_wall": [], "stats_c6": [], "matrix_wall": [], "copy_wall": [], "nonzero_wall": []}
        launches = {}
        for _ in range(args.reps):
            w, c6, c7 = run_hits(thr)
            r["hits_wall"].append(w * 1e3); r["hits_c6"].append(c6["ms"]); r["hits_c7"].append(c7["ms"]); launches["hits"] = [c6["launches"], c7["launches"]]
            w, c6 = run_stats(thr)
            r["stats_wall"].append(w * 1e3); r["stats_c6"].append(c6["ms"]); launches["stats"] = [c6["launches"], 0]
            r["matrix_wall"].append(run_matrix() * 1e3)
            t0 = time.perf_counter(); host.copy_(out); torch.cuda.synchronize(); r["copy_wall"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); where = np.nonzero(host.numpy() >= thr[None, None, :]); r["nonzero_wall"].append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(nt, cnt.sum(axis=0)) and int(nt.sum()) == where[0].size and np.array_equal(ns, np.minimum(nt, cap)))
        med = {k2: round(statistics.median(v), 3) for k2, v in r.items()}
        med.update(threshold_rank=k, hits_total=int(nt.sum()), hits_stored=int(ns.sum()), launches_class_6_7=launches, totals_equal_stats_and_nonzero=same,
                   hits_over_stats_wall=round(med["hits_wall"] / med["stats_wall"], 3),
                   hits_over_stats_class6=round(med["hits_c6"] / med["stats_c6"], 3),
                   matrix_route_over_hits_wall=round((med["matrix_wall"] + med["copy_wall"] + med["nonzero_wall"]) / med["hits_wall"], 3),
                   class7_share_of_hits_kernels=round(med["hits_c7"] / (med["hits_c6"] + med["hits_c7"]), 4),
                   spread={k2: [round(min(v), 3), round(max(v), 3)] for k2, v in r.items()})
        per_rate[str(rate)] = med
    flag = bank.range_status()
    bank.close()
    ok = all(v["totals_equal_stats_and_nonzero"] for v in per_rate.values()) and not flag
    res = {"metric": "dense hit lists: oww_bank_score_hits against oww_bank_score_stats and against matrix + D2H + host nonzero, ms per call",
           "bank_heads": H, "T": T, "hidden": 64, "sequences": B, "windows_per_sequence": NW, "windows": N, "cap": cap,
           "mask_bytes": int(H * ((B * ((NW + 31) // 32) + 3) // 4 * 4) * 4), "matrix_bytes": N * H * 4, "rates": per_rate, "range_flag": bool(flag),
           "timing": f"wall = host clock around a call that ends in a stream synchronise; c6 / c7 = oww_kernel_times classes 6 and 7 (hipEvents); "
                     f"{args.warmup} warm-up round(s), {args.reps} alternating repeats, medians with [min, max]",
           "source_hash": _build.source_hash(), "build_info": lib.oww_build_info().decode() if hasattr(lib, "oww_build_info") else "",
           "device": torch.cuda.get_device_name(0), "data": "N(0, 1) features, synthetic bank heads (seeds 7000 ..)"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the totals differ from the statistics entry's or numpy's, or the range flag is up")


if __name__ == "__main__":
    main()
