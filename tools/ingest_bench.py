#!/usr/bin/env python3
"""Device time of the stateful stream ingest (oww_ingest / oww_step_ingest) on the flagship shape: S streams x 3 heads, 8 kHz mu-law
messages of 640 codes resident in HBM.

    python tools/ingest_bench.py [--streams 131072] [--rounds 5] [--iters 20] [--out FILE.json]

Reports, as one JSON line (and to --out):
  ingest_ms        hipEvent time of the ingest launch alone (device codes -> the handle's staging buffer), its bytes (codes in, 16 kHz
                   samples out, history in and out) over that time, and that rate as a fraction of the 8 TB/s HBM peak
  step_ingest_ms   oww_step_ingest on the resident codes, against
  step_pcm16k_ms   oww_step on resident 16 kHz PCM, same build, same process
  host_8k_ms       predict_batch(pcm_8k, sample_rate=8000) from host memory (host clock around a blocking call): the stateless host-fed path
  mixed_one_class_ms   the ingest-classes launch (oww_ingest_mixed) on a second handle whose table holds the one class (8000, "ulaw"):
                   the same codes, the same row pitch, to be read against ingest_ms -- what the class lookup costs
  mixed_thirds_ms  oww_ingest_mixed on a third handle with the table [(8000, "ulaw"), (16000, "pcm16"), (48000, "pcm16")] and a third of
                   the streams in each (stream s in class s % 3), rows 7,680 bytes apart: workgroups of 640, 1,280 and 3,840 input
                   samples in one launch, and the 48 kHz class's LDS allocation for all of them -- what the imbalance costs
All device variants alternate inside every round (warm-up first); every figure is the median over rounds with its min..max.
--no-mixed leaves the two extra handles out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from openwakeword_amd import _lib, resample as R, weights as W
from openwakeword_amd.model import BatchedModel

PEAK_HBM_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-mixed", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs the GPU: there is nothing to time without one")
    S, rate, n_in = args.streams, 8000, 640
    names = ("alexa", "hey_mycroft", "hey_jarvis")
    wts = {"heads": {n: W.synthetic_head(n, 1234) for n in names}, "embedding": W.synthetic_embedding(1234)}
    st = torch.cuda.Stream()
    bm = BatchedModel(S, list(names), weights=wts, hip_stream=st.cuda_stream)
    eng, lib = bm.engine, bm.engine._lib
    bm.configure_ingest(rate, "ulaw")
    p, q, taps = R.design(rate)
    hpad = (taps.shape[1] - 1 + 7) // 8 * 8
    gen = torch.Generator(device="cuda").manual_seed(7)
    codes = torch.randint(0, 256, (S, n_in), device="cuda", dtype=torch.uint8, generator=gen)
    pcm16k = (torch.randn(S, 1280, device="cuda", generator=gen) * 3000).to(torch.int16)
    pcm8k_host = (np.random.default_rng(7).standard_normal((S, n_in)) * 3000).astype(np.int16)
    torch.cuda.synchronize()
    cp, pp = C.c_void_p(codes.data_ptr()), C.c_void_p(pcm16k.data_ptr())

    def ingest():
        _lib.check(lib.oww_ingest(eng._h, cp, 1, n_in, None, 0, None, 1))

    def step_ingest():
        _lib.check(lib.oww_step_ingest(eng._h, cp, 1, n_in, None, 0, None, 1))

    def step_pcm():
        _lib.check(lib.oww_step(eng._h, pp, 1, 1, None, 1))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(args.iters):
            fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    variants = {"ingest_ms": ingest, "step_ingest_ms": step_ingest, "step_pcm16k_ms": step_pcm}
    thirds = [(8000, "ulaw"), (16000, "pcm16"), (48000, "pcm16")]
    if not args.no_mixed:
        bm_one = BatchedModel(S, list(names), weights=wts, hip_stream=st.cuda_stream)
        bm_one.configure_ingest_classes([(rate, "ulaw")])
        bm_mix = BatchedModel(S, list(names), weights=wts, hip_stream=st.cuda_stream)
        bm_mix.configure_ingest_classes(thirds)
        bm_mix.assign_ingest(np.arange(S), np.arange(S) % 3)
        rb = bm_mix.engine.ingest_row_bytes()
        rows = torch.randint(0, 256, (S, rb), device="cuda", dtype=torch.uint8, generator=gen)
        torch.cuda.synchronize()
        rp = C.c_void_p(rows.data_ptr())
        assert bm_one.engine.ingest_row_bytes() == n_in

        def mixed_one():
            _lib.check(lib.oww_ingest_mixed(bm_one.engine._h, cp, 1, n_in, 1280, None, 0, None, 1))

        def mixed_thirds():
            _lib.check(lib.oww_ingest_mixed(bm_mix.engine._h, rp, 1, rb, 1280, None, 0, None, 1))
        variants["mixed_one_class_ms"] = mixed_one
        variants["mixed_thirds_ms"] = mixed_thirds
    for fn in variants.values():
        for _ in range(3):
            fn()
    eng.sync()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    # the stateless host-fed path (unchanged by the ingest): host PCM at 8 kHz in, scores out, blocking
    bm.predict_batch(pcm8k_host, sample_rate=rate)
    host = []
    for _ in range(args.host_iters):
        t0 = time.perf_counter()
        bm.predict_batch(pcm8k_host, sample_rate=rate)
        host.append((time.perf_counter() - t0) * 1e3)
    # what was timed is what the tests hold: the first streams of one more launch against the host restatement
    bm.configure_ingest(rate, "ulaw")
    out = torch.empty(S, 1280, device="cuda", dtype=torch.int16)
    torch.cuda.synchronize()
    _lib.check(lib.oww_ingest(eng._h, cp, 1, n_in, None, 0, C.c_void_p(out.data_ptr()), 1))
    eng.sync()
    n_chk = min(S, 8)
    y, _ = R.ingest_numpy(R.decode_ulaw(codes[:n_chk].cpu().numpy()), rate)
    want = np.clip(np.rint(y), -32768, 32767).astype(np.int64)
    max_diff = int(np.abs(out[:n_chk].cpu().numpy().astype(np.int64) - want).max())

    def stat(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    bytes_launch = S * (n_in + 1280 * 2 + 2 * hpad * 2)
    t = statistics.median(ms["ingest_ms"]) * 1e-3
    res = {"build": lib.oww_build_info().decode(), "device": torch.cuda.get_device_name(0), "streams": S, "heads": len(names),
           "rate_in": rate, "encoding": "ulaw", "n_in": n_in, "n_taps": int(taps.shape[1]), "rounds": args.rounds, "iters": args.iters,
           "ingest_ms": stat(ms["ingest_ms"]), "step_ingest_ms": stat(ms["step_ingest_ms"]), "step_pcm16k_ms": stat(ms["step_pcm16k_ms"]),
           "step_ingest_minus_step_ms": round(statistics.median(ms["step_ingest_ms"]) - statistics.median(ms["step_pcm16k_ms"]), 4),
           "host_8k_predict_batch_ms": stat(host),
           "ingest_bytes_per_launch": bytes_launch, "ingest_GB_s": round(bytes_launch / t / 1e9, 1),
           "ingest_frac_of_hbm_peak": round(bytes_launch / t / 1e9 / PEAK_HBM_GBS, 4),
           "ingest_fma_per_launch": S * 1280 * ((int(taps.shape[1]) + 3) // 4 * 4),
           "max_abs_diff_vs_numpy_first_streams": max_diff}
    if not args.no_mixed:
        # the one-class mixed launch computes what the single-format launch computes: first streams, one more launch each from silence
        bm_one.configure_ingest_classes([(rate, "ulaw")])
        out2 = torch.empty(S, 1280, device="cuda", dtype=torch.int16)
        torch.cuda.synchronize()
        _lib.check(lib.oww_ingest_mixed(bm_one.engine._h, cp, 1, n_in, 1280, None, 0, C.c_void_p(out2.data_ptr()), 1))
        bm_one.engine.sync()
        hp = [(R.class_params(r, e)[3] - 1 + 7) // 8 * 8 if r != 16000 else 0 for r, e in thirds]
        per_class = [R.class_n_in(r) * (2 if e == "pcm16" else 1) + 1280 * 2 + 2 * h * 2 for (r, e), h in zip(thirds, hp)]
        n_cls = [len(range(c, S, 3)) for c in range(3)]
        bytes_mix = sum(n * b for n, b in zip(n_cls, per_class))
        t_mix = statistics.median(ms["mixed_thirds_ms"]) * 1e-3
        res.update({"mixed_one_class_ms": stat(ms["mixed_one_class_ms"]), "mixed_thirds_ms": stat(ms["mixed_thirds_ms"]),
                    "mixed_one_class_over_ingest": round(statistics.median(ms["mixed_one_class_ms"]) / statistics.median(ms["ingest_ms"]), 4),
                    "mixed_one_class_equals_ingest_bit_for_bit": bool(torch.equal(out, out2)),
                    "mixed_thirds_classes": [list(c) for c in thirds], "mixed_thirds_row_bytes": int(rb),
                    "mixed_thirds_bytes_per_launch": bytes_mix, "mixed_thirds_GB_s": round(bytes_mix / t_mix / 1e9, 1),
                    "mixed_thirds_fma_per_launch": sum(n * 1280 * ((R.class_params(r, e)[3] + 3) // 4 * 4) for n, (r, e) in zip(n_cls, thirds))})
        bm_one.close()
        bm_mix.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    bm.close()


if __name__ == "__main__":
    main()
