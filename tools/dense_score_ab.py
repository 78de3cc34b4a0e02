#!/usr/bin/env python3
"""Dense scoring A/B on one MI355X: every window of eight hours of features through the three benchmark heads.

  A = the only device route before oww_score_features: the heads' external-features launch over the N materialised windows, features
      resident (OWW_DENSE_PATH=ext sends oww_score_features down its gather fallback, and OWW_DENSE_SLAB_MB makes its slab large enough
      for all N windows: they are gathered on the device once and scored by the one launch oww_head would issue for them).  Timed: that
      heads launch (kernel class 6); the gather (class 7) is reported beside it and is not part of A.  A_slabs: the same with the
      library's own 256 MiB slabs, what the fallback costs a head form the sliding kernel does not cover.
  B = the sliding-window launch over the same N windows (kernel class 6).
Both from oww_kernel_times (hipEvents around the launches), features and scores on the device, warm-up first, A and B alternating
inside every repeat, medians.  The outputs of the two routes are compared bit for bit.  Then what a user feels: score_clips on one hour
of audio end to end, beside utils.bulk_predict's streaming loop on the same hour as WAV files.  The box is named by the configs[1]
probe of tools/class_probe.sh (4,096 x hey_jarvis step: first class below 0.42 ms).  Prints one JSON line; --out writes it to a file.

usage: python tools/dense_score_ab.py [--windows 45000] [--seqs 8] [--reps 7] [--hour-seqs 8] [--out profiles/dense_score_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

HEADS = ("alexa", "hey_mycroft", "hey_jarvis")


def box_probe(torch, W, StreamEngine, steps=600, warmup=200):
    S = 4096
    eng = StreamEngine(S, {"hey_jarvis": W.synthetic_head("hey_jarvis", 1234)}, W.synthetic_embedding(1234))
    try:
        pcm = (torch.randn(S, 1280, device="cuda") * 3000.0).round().clamp(-32768, 32767).to(torch.int16)
        for _ in range(warmup):
            eng.step_device(pcm.data_ptr())
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step_device(pcm.data_ptr())
        eng.sync()
        return (time.perf_counter() - t0) / steps * 1e3
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=45000, help="windows per sequence (45,000 x 80 ms = one hour)")
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hour-seqs", type=int, default=8, help="the end-to-end hour of audio is split into this many clips / files")
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from openwakeword_amd import _build, _lib, utils
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import KERNEL_CLASSES, StreamEngine
    from openwakeword_amd.model import BatchedModel
    if not torch.cuda.is_available():
        raise SystemExit("dense_score_ab.py measures on the GPU; none is visible")

    probe_ms = box_probe(torch, W, StreamEngine)
    heads = {n: W.synthetic_head(n, 1234) for n in HEADS}
    eng = StreamEngine(args.seqs, heads, W.synthetic_embedding(1234))
    T = max(int(h["T"]) for h in heads.values())
    n_rows = args.windows + T - 1
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    feats = torch.randn(args.seqs, n_rows, 96, device="cuda", generator=gen)
    out = {k: torch.zeros(args.seqs, args.windows, eng.n_labels, device="cuda") for k in "AB"}
    eng.enable_timing(True)

    one_slab_mb = args.seqs * args.windows * T * 384 // (1 << 20) + 1

    def run(which):
        os.environ.pop("OWW_DENSE_PATH", None)
        os.environ.pop("OWW_DENSE_SLAB_MB", None)
        if which != "B":
            os.environ["OWW_DENSE_PATH"] = "ext"
        if which == "A":
            os.environ["OWW_DENSE_SLAB_MB"] = str(one_slab_mb)
        eng.kernel_times()
        _lib.check(eng._lib.oww_score_features(eng._h, feats.data_ptr(), 1, args.seqs, n_rows, out[which[0]].data_ptr(), 1))
        t = eng.kernel_times()
        return t[KERNEL_CLASSES[6]], t[KERNEL_CLASSES[7]]

    for _ in range(args.warmup):
        run("A"); run("B"); run("A_slabs")
    ms = {"A": [], "B": [], "A_slabs": []}
    gather_ms, launches = [], {}
    for _ in range(args.reps):
        for which in ("A", "B", "A_slabs"):
            heads_t, gather_t = run(which)
            ms[which].append(heads_t["ms"])
            launches[which] = (heads_t["launches"], gather_t["launches"])
            if which == "A":
                gather_ms.append(gather_t["ms"])
    os.environ.pop("OWW_DENSE_PATH", None)
    os.environ.pop("OWW_DENSE_SLAB_MB", None)
    torch.cuda.synchronize()
    same = bool(torch.equal(out["A"], out["B"]))
    finite = bool(torch.isfinite(out["B"]).all().item())
    mid = float(((out["B"] > 0.05) & (out["B"] < 0.95)).float().mean().item())
    eng.close()

    n_windows = args.seqs * args.windows
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "metric": "dense scoring: heads launch time over every window, ext route (A) against the sliding-window kernel (B)",
        "heads": list(HEADS), "T": T, "sequences": args.seqs, "windows_per_sequence": args.windows, "windows": n_windows,
        "audio_hours": round(n_windows * 0.08 / 3600, 2),
        "A_ext_ms_median": round(med["A"], 3), "B_sliding_ms_median": round(med["B"], 3),
        "A_ext_ms": [round(x, 3) for x in ms["A"]], "B_sliding_ms": [round(x, 3) for x in ms["B"]],
        "A_slabs_ms_median": round(med["A_slabs"], 3),
        "A_over_B": round(med["A"] / med["B"], 3),
        "A_gather_ms_median_not_in_A": round(statistics.median(gather_ms), 3),
        "launches_heads_gather": launches,
        "B_windows_per_second": round(n_windows / (med["B"] * 1e-3), 0),
        # A: every window's T rows; B: each of its launches (passes of at most two nets) stages 256 + T - 1 rows per tile of 256 windows
        "feature_bytes_read": {"A": n_windows * T * 384,
                               "B": launches["B"][0] * args.seqs * ((args.windows + 255) // 256) * (256 + T - 1) * 384},
        "bit_identical": same, "finite": finite, "share_of_scores_in_0.05_0.95": round(mid, 3),
        "timing": f"oww_kernel_times class 6 (hipEvents), {args.warmup} warm-up pairs, {args.reps} alternating repeats, medians",
        "source_hash": _build.source_hash(), "box": {"device": torch.cuda.get_device_name(0), "configs1_step_ms": round(probe_ms, 3),
                                                     "class": 1 if probe_ms < 0.42 else 2},
        "data": "N(0, 1) features, synthetic weights seed 1234",
    }

    if not args.no_end_to_end:
        # one hour of audio, end to end: PCM on the host in, scores on the host out
        k = args.hour_seqs
        n = 3600 * 16000 // k
        pcm = W.synthetic_pcm(k, n, seed=5, rms=3000.0)
        bm = BatchedModel(k, list(HEADS), weights="synthetic")
        bm.score_clips(pcm[:, :16000 * 20])                               # warm-up
        t0 = time.perf_counter()
        dense = bm.score_clips(pcm)
        clips_s = time.perf_counter() - t0
        n_pos = next(iter(dense.values())).shape[1]
        bm.close()
        with tempfile.TemporaryDirectory() as d:
            paths = []
            for i in range(k):
                paths.append(os.path.join(d, f"hour_{i}.wav"))
                with wave.open(paths[-1], "wb") as w:
                    w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                    w.writeframes(pcm[i].tobytes())
            t0 = time.perf_counter()
            stream = utils.bulk_predict(paths, list(HEADS), weights="synthetic", padding=0)
            bulk_s = time.perf_counter() - t0
        res["end_to_end_one_hour"] = {
            "clips": k, "samples_per_clip": n, "score_clips_s": round(clips_s, 3), "score_clips_positions_per_clip": n_pos,
            "score_clips_audio_hours_per_second": round(1.0 / clips_s, 3),
            "bulk_predict_s": round(bulk_s, 3), "bulk_predict_frames_per_file": len(stream[paths[0]]),
            "bulk_predict_audio_hours_per_second": round(1.0 / bulk_s, 3),
            "note": "wall clock around each call, host PCM / WAV files in, host scores out; bulk_predict includes reading the files, "
                    "building its model and one host round trip per 80 ms chunk; score_clips excludes building the model"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not (same and finite):
        raise SystemExit("the two routes disagree or a score is not finite")


if __name__ == "__main__":
    main()
