#!/usr/bin/env python3
"""Dense scoring over the head bank on one MI355X: 256 narrow bank heads (T = 16, 64 hidden units) over a corpus.

Three comparisons, tools/dense_score_ab.py's protocol (features and outputs resident, warm-up rounds first, the arms alternating
inside every repeat, medians of oww_kernel_times class 6 -- hipEvents around the heads launches):
  large   eight sequences of 45,000 windows (eight hours).  Time per (window x head) of the one-call launch of
          oww_bank_score_features against time per (window x net) of the fixed-head sliding kernel: oww_score_features with the three
          benchmark heads (four nets) on the same features in the same session.  The bank kernel streams the same weight bytes per
          tile and stages rows less often, so it must not be slower than that figure by more than the fixed-head kernel's own
          min-max spread over its repeats.
  short   one sequence of 7,500 windows (ten minutes): one call with 256 ids against 256 calls with one id each -- why the grid spans
          heads.  Class 6 sums and wall clock.
  stats   oww_bank_score_stats on the large shape against oww_bank_score_features plus the device-to-host copy of its matrix
          (0.37 GB): wall clock around each, and the kernels' class 6 time.
The statistics are checked against torch's on the matrix.  Prints one JSON line; --out writes it to a file.

usage: python tools/dense_bank_ab.py [--heads 256] [--reps 7] [--out profiles/dense_bank_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

FIXED = ("alexa", "hey_mycroft", "hey_jarvis")
T = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=256)
    ap.add_argument("--windows", type=int, default=45000)
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--short-windows", type=int, default=7500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from openwakeword_amd import _build, _lib
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import KERNEL_CLASSES, StreamEngine, _ptr
    if not torch.cuda.is_available():
        raise SystemExit("dense_bank_ab.py measures on the GPU; none is visible")
    os.environ.pop("OWW_DENSE_PATH", None)
    os.environ.pop("OWW_DENSE_BANK_HPW", None)

    emb = W.synthetic_embedding(1234)
    H, B, NW = args.heads, args.seqs, args.windows
    bank = StreamEngine(B, {}, emb, bank_slots=1, bank_capacity=H)
    fixed = StreamEngine(B, {n: W.synthetic_head(n, 1234) for n in FIXED}, emb)
    ids = np.array([bank.bank_add(W.synthetic_head(f"bank{i}", 7000 + i, kind="binary", T=T, hidden=64, n_out=1, layernorm=True)) for i in range(H)],
                   np.int32)
    n_nets = 4                                                  # alexa, hey_mycroft, hey_jarvis (a gated pair)
    bank.enable_timing(True); fixed.enable_timing(True)
    lib = bank._lib
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    n_rows = NW + T - 1
    feats = torch.randn(B, n_rows, 96, device="cuda", generator=gen)
    out_bank = torch.zeros(B, NW, H, device="cuda")
    out_fixed = torch.zeros(B, NW, fixed.n_labels, device="cuda")
    cnt, mx, am = np.zeros((B, H), np.int32), np.zeros((B, H), np.float32), np.zeros((B, H), np.int32)

    def heads_ms(eng):
        return eng.kernel_times()[KERNEL_CLASSES[6]]

    def run_bank():
        bank.kernel_times()
        t0 = time.perf_counter()
        _lib.check(lib.oww_bank_score_features(bank._h, feats.data_ptr(), 1, B, n_rows, _ptr(ids), H, out_bank.data_ptr(), 1))
        return heads_ms(bank), time.perf_counter() - t0

    def run_fixed():
        fixed.kernel_times()
        _lib.check(lib.oww_score_features(fixed._h, feats.data_ptr(), 1, B, n_rows, out_fixed.data_ptr(), 1))
        return heads_ms(fixed)

    def run_stats():
        bank.kernel_times()
        t0 = time.perf_counter()
        _lib.check(lib.oww_bank_score_stats(bank._h, feats.data_ptr(), 1, B, n_rows, _ptr(ids), H, None, _ptr(cnt), _ptr(mx), _ptr(am)))
        return heads_ms(bank), time.perf_counter() - t0

    # ---- large shape: the bank launch, the fixed-head launches and the statistics entry alternate
    host = torch.empty(out_bank.shape, dtype=torch.float32, pin_memory=True)
    for _ in range(args.warmup):
        run_bank(); run_fixed(); run_stats(); host.copy_(out_bank); torch.cuda.synchronize()
    ms = {"bank": [], "fixed": [], "stats": []}
    wall = {"bank_matrix": [], "copy": [], "stats": []}
    launches = {}
    for _ in range(args.reps):
        t, w = run_bank(); ms["bank"].append(t["ms"]); wall["bank_matrix"].append(w); launches["bank"] = t["launches"]
        t0 = time.perf_counter(); host.copy_(out_bank); torch.cuda.synchronize(); wall["copy"].append(time.perf_counter() - t0)
        t = run_fixed(); ms["fixed"].append(t["ms"]); launches["fixed"] = t["launches"]
        t, w = run_stats(); ms["stats"].append(t["ms"]); wall["stats"].append(w); launches["stats"] = t["launches"]
    torch.cuda.synchronize()
    thr = torch.tensor(0.5, device="cuda")
    stats_same = bool(np.array_equal(cnt, (out_bank >= thr).sum(dim=1).cpu().numpy().astype(np.int32)) and
                      np.array_equal(mx.view(np.int32), out_bank.max(dim=1).values.cpu().numpy().view(np.int32)))
    widx = torch.arange(NW, device="cuda", dtype=torch.int32)[None, :, None]
    first = torch.where(out_bank == out_bank.max(dim=1, keepdim=True).values, widx, NW).min(dim=1).values.cpu().numpy().astype(np.int32)
    stats_same = stats_same and bool(np.array_equal(am, first))
    finite = bool(torch.isfinite(out_bank).all().item())
    mid = float(((out_bank > 0.05) & (out_bank < 0.95)).float().mean().item())
    del host

    # ---- short shape: one call with every id against one call per id
    SW = args.short_windows
    s_rows = SW + T - 1
    out_all = torch.zeros(1, SW, H, device="cuda")
    out_one = torch.zeros(1, SW, 1, device="cuda")
    one_id = [np.array([i], np.int32) for i in ids]

    def short_all():
        bank.kernel_times()
        t0 = time.perf_counter()
        _lib.check(lib.oww_bank_score_features(bank._h, feats.data_ptr(), 1, 1, s_rows, _ptr(ids), H, out_all.data_ptr(), 1))
        return heads_ms(bank), time.perf_counter() - t0

    def short_each():
        bank.kernel_times()
        t0 = time.perf_counter()
        for a in one_id:
            _lib.check(lib.oww_bank_score_features(bank._h, feats.data_ptr(), 1, 1, s_rows, _ptr(a), 1, out_one.data_ptr(), 1))
        return heads_ms(bank), time.perf_counter() - t0

    for _ in range(args.warmup):
        short_all(); short_each()
    sms = {"all": [], "each": []}
    swall = {"all": [], "each": []}
    for _ in range(args.reps):
        t, w = short_all(); sms["all"].append(t["ms"]); swall["all"].append(w); launches["short_all"] = t["launches"]
        t, w = short_each(); sms["each"].append(t["ms"]); swall["each"].append(w); launches["short_each"] = t["launches"]
    torch.cuda.synchronize()
    short_same = bool(torch.equal(out_all[:, :, -1:], out_one))           # (the last single call scored the last id)
    flag = bank.range_status()
    bank.close(); fixed.close()

    N = B * NW
    med = {k: statistics.median(v) for k, v in ms.items()}
    per_bank = med["bank"] * 1e6 / (N * H)                              # ns per (window x head)
    per_fixed = med["fixed"] * 1e6 / (N * n_nets)                       # ns per (window x net)
    spread = (max(ms["fixed"]) - min(ms["fixed"])) * 1e6 / (N * n_nets)
    r3 = lambda v: [round(x, 3) for x in v]
    res = {
        "metric": "dense scoring over the head bank: one launch for every listed head (heads_dense_bank_kernel)",
        "bank_heads": H, "T": T, "hidden": 64,
        "large": {"sequences": B, "windows_per_sequence": NW, "windows": N, "audio_hours": round(N * 0.08 / 3600, 2),
                  "bank_ms_median": round(med["bank"], 3), "bank_ms": r3(ms["bank"]),
                  "fixed_ms_median": round(med["fixed"], 3), "fixed_ms": r3(ms["fixed"]), "fixed_heads": list(FIXED), "fixed_nets": n_nets,
                  "bank_ns_per_window_head": round(per_bank, 5), "fixed_ns_per_window_net": round(per_fixed, 5),
                  "fixed_min_max_spread_ns": round(spread, 5), "bank_minus_fixed_ns": round(per_bank - per_fixed, 5),
                  "within_fixed_spread": bool(per_bank - per_fixed <= spread),
                  "launches_class6": {k: launches[k] for k in ("bank", "fixed", "stats")}},
        "short": {"sequences": 1, "windows": SW, "audio_minutes": round(SW * 0.08 / 60, 1),
                  "one_call_ms_median": round(statistics.median(sms["all"]), 3), "one_call_ms": r3(sms["all"]),
                  "call_per_head_ms_median": round(statistics.median(sms["each"]), 3), "call_per_head_ms": r3(sms["each"]),
                  "class6_ratio_per_head_over_one_call": round(statistics.median(sms["each"]) / statistics.median(sms["all"]), 3),
                  "one_call_wall_ms_median": round(statistics.median(swall["all"]) * 1e3, 3),
                  "call_per_head_wall_ms_median": round(statistics.median(swall["each"]) * 1e3, 3),
                  "wall_ratio_per_head_over_one_call": round(statistics.median(swall["each"]) / statistics.median(swall["all"]), 3),
                  "launches_class6": {"one_call": launches["short_all"], "call_per_head": launches["short_each"]},
                  "last_column_bit_identical": short_same},
        "stats_vs_matrix": {"stats_class6_ms_median": round(med["stats"], 3), "stats_class6_ms": r3(ms["stats"]),
                            "stats_wall_ms_median": round(statistics.median(wall["stats"]) * 1e3, 3),
                            "matrix_wall_ms_median": round(statistics.median(wall["bank_matrix"]) * 1e3, 3),
                            "matrix_d2h_wall_ms_median": round(statistics.median(wall["copy"]) * 1e3, 3),
                            "matrix_bytes": N * H * 4, "d2h": "into pinned host memory",
                            "matrix_plus_copy_over_stats_wall": round((statistics.median(wall["bank_matrix"]) + statistics.median(wall["copy"])) /
                                                                      statistics.median(wall["stats"]), 3),
                            "stats_equal_torch_on_matrix": stats_same},
        "finite": finite, "range_flag": bool(flag), "share_of_scores_in_0.05_0.95": round(mid, 3),
        "timing": f"oww_kernel_times class 6 (hipEvents), {args.warmup} warm-up rounds, {args.reps} alternating repeats, medians; wall = "
                  "host clock around a call that ends in a stream synchronise",
        "source_hash": _build.source_hash(), "device": torch.cuda.get_device_name(0),
        "data": "N(0, 1) features, synthetic weights (bank heads seeds 7000 .., fixed heads seed 1234)",
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not (stats_same and finite and short_same) or flag:
        raise SystemExit("the statistics differ from the matrix's, a score is not finite, or the one-call and per-head routes disagree")


if __name__ == "__main__":
    main()
