#!/usr/bin/env python3
"""
bench.py -- throughput of the streaming wake-word hot path on N MI355X GPUs of one node.

A "step" is one 80 ms frame (1280 new int16 samples) for EVERY stream of the job through
mel -> incremental speech-embedding CNN -> wake-word heads -> post-processing, i.e. one
`openwakeword.Model.predict` per stream (/root/reference/openwakeword/model.py:232-386).
Metric (BASELINE.json): frames/sec = stream-steps completed per second, whole job.

Workload: per GPU `--streams` concurrent streams (default 131072 = the per-GPU shard of BASELINE
configs[3] "8 GPU, 1M streams, 3 heads"; configs[2] is --streams 65536, configs[1] is
--streams 4096 --heads hey_jarvis), 3 heads (alexa, hey_mycroft, hey_jarvis), synthetic Gaussian PCM
(RMS 3000) already resident in HBM, random-init weights of the reference's shapes (no model files exist
offline).  Streams are sharded by contiguous range over ranks (weak scaling: fixed streams per GPU);
the only collective is the gather of fp32 scores [S, n_labels] to rank 0 over RCCL (every step, or every
--gather-every K steps).

A plain run sets up, warms up, times exactly --steps steps and prints the JSON line (contract fields, config, scores_valid);
`parity`, `roofline` and `cpu_baseline` are null in it.  With --full the line also carries:
  parity       64 probe streams x 16 frames placed at random ids of the SAME full-size engine, compared with the CPU
               oracle before the timed region (oracle/parity_sample.py; the timed configuration carries its own parity evidence)
  roofline     dominant kernel, from hipEvents on the library's stream in a separate pass after the timed steps
  cpu_baseline the reference's algorithm on the host cores (torch-CPU port), timed by rank 0 before it joins the process group (every N)
  sustained    100 warm-up + 250 timed steps of the same configuration (N = 1 only)
  fp32_exact   the same workload on the exact-fp32 kernel family (use_mfma = 1), the reference's arithmetic type
  resident_1m  1,048,576 streams resident in ONE handle on one GPU (run in a child process): ms per step must stay < 80
  (and the other BASELINE configurations, masked steps, host PCM, embed_clips; the --no-* switches thin a --full run out)

--dump-outputs DIR writes the scores of the last timed step, all ranks' streams in global order, as DIR/scores.npy (fp32
[streams x gpus, n_labels]; a fixed, seeded sample of rows when that exceeds 64 MB).  The inputs depend only on the arguments.

  python bench.py --gpus 1 --steps 50 --warmup 10
  python bench.py --gpus 1 --steps 50 --warmup 10 --full
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P \\
         bench.py --gpus 8 --steps 50 --warmup 10
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# executed algorithmic flops per stream-step of each CNN stage (2 x MACs of the incremental form)
STAGE_FLOPS = {"stageA": 1_880_064, "stageB": 3_096_576, "stageC": 3_649_536, "stageD": 1_658_880, "stageE": 940_032}
MFLOP_CNN_STEP = sum(STAGE_FLOPS.values()) / 1e6      # 11.225 MFLOP: one incremental step of the embedding CNN
MEL_BYTES = 3584            # 2560 B new PCM + 1024 B mel rows per stream-step
PEAK_FP32_TFLOPS = 157.3    # MI355X_MICROARCH.md: fp32 MFMA dense peak
PEAK_F16_TFLOPS = 2500.0    # MI355X_MICROARCH.md: f16 / bf16 MFMA dense peak
# f16 MFMAs (v_mfma_f32_16x16x32_f16, 16384 flop each) the fp16-split kernels execute per stream-step, channel padding included
# (round 2: the layers with a 72-channel input run K-merged -- 7 instead of 9 k-steps per output tile -- i.e. layers b, c, d of
#  stage C: 810 instead of 990, and layer a of stage D: 306 instead of 324; layer a of stage C, 48 channels in, 5 instead of 6: 780)
#  round 3: stage A's conv0 is one K-folded MFMA per output tile instead of three, and the half tiles of conv1 / conv2 stack a
#  second tap / output row in their free rows: 512 instead of 672; stage B's remainder k-step in two MFMAs: 648 instead of 756)
HX_MFMAS = {"stageA": 512, "stageB": 648, "stageC": 780, "stageD": 306, "stageE": 182}
MEL_FLOPS = 100_000         # FFT form of the log-mel front end per stream-step, executed by the fused launch's VALU
PEAK_CLOCK_GHZ = 2.4        # MI355X_MICROARCH.md: peak engine clock; 256 CUs x 4 SIMDs
N_SIMD = 1024
PEAK_HBM_GBS = 8000.0
REALTIME_STEPS_PER_S = 12.5  # one 80 ms frame per stream every 80 ms


def head_flops(heads) -> int:
    n = 0
    for h in heads.values():
        per = h["T"] * 96 * h["hidden"] + h["hidden"] * h["hidden"] + h["hidden"] * h["n_out"]
        n += 2 * per * (2 if h["kind"] == "gated" else 1)
    return n


_PROFILE_CACHE = {}


def loaded_build() -> str:
    """The source hash compiled into the libowwhip.so this process runs (oww_build_info: "src=<sha16> arch=...")."""
    from openwakeword_amd import _lib
    info = _lib.load().oww_build_info().decode()
    return dict(kv.split("=", 1) for kv in info.split()).get("src", "unknown")


def committed_profile(kind: str):
    """(table, file name, None) of the newest committed rocprofv3 counter summary profiles/rNN_<kind>.json that was taken ON THE BUILD
    THIS PROCESS RUNS -- tools/pmc.sh stores the library's source hash with every summary ("_csrc_sha16") -- else (None, None, why).
    A kernel change without a fresh PMC pass must not price new times with old instruction counts."""
    if kind in _PROFILE_CACHE:
        return _PROFILE_CACHE[kind]
    import glob
    have = loaded_build()
    res = (None, None, f"no profiles/r*_{kind}.json was taken on the loaded build (src={have}): run tools/pmc.sh on it")
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_{kind}.json")), reverse=True):
        try:
            t = json.load(open(path))
        except Exception:
            continue
        if t.get("_csrc_sha16") == have:
            res = (t, os.path.basename(path), None)
            break
    _PROFILE_CACHE[kind] = res
    return res


def pmc_traffic(kernel: str, streams: int, args):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC pass of THIS build (FETCH_SIZE x2 + WRITE_SIZE, produced by
    tools/pmc.sh on the same workload); None when no pass matches this configuration or this build."""
    if args.valu or args.lds_mfma or streams != 131072:
        return None
    key = kernel + ("_rr" if args.fp32 else "_hx")
    t, name, _why = committed_profile("traffic")
    if t is None or key not in t:
        return None
    return {"hbm_bytes_per_launch": t[key]["hbm_bytes"], "source": f"profiles/{name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, build src={t['_csrc_sha16']})"}


def issue_bound(kernel: str, streams: int, avg_ms: float, args):
    """Composite bound of one launch from the committed PMC pass of the loaded build (profiles/rNN_instr.json, tools/pmc.sh on this workload): wave
    instructions per stream-step by pipe and the SIMD cycles they need at issue.  On this part a wave's VALU and MFMA work add up on
    its SIMD (tools/ubench/overlap_ubench.hip: a VALU instruction issues in 4 cycles, v_mfma_f32_16x16x32_f16 in 16, no overlap between
    the waves of a SIMD), so issue cycles = 4 VALU + 16 MFMA per stream-step; LDS and HBM are priced beside it and the largest of the
    fractions names what binds."""
    if args.valu or args.lds_mfma or args.fp32 or streams != 131072:
        return None
    tab, src, why = committed_profile("instr")
    if tab is None:
        return {"unavailable": why}
    t = tab.get(kernel + "_hx")
    if t is None:
        return None
    per = lambda c: t[c] / streams
    mfma, valu, lds = per("SQ_INSTS_MFMA"), per("SQ_INSTS_VALU") - per("SQ_INSTS_MFMA"), per("SQ_INSTS_LDS")
    avail = avg_ms * 1e-3 * PEAK_CLOCK_GHZ * 1e9 * N_SIMD / streams          # SIMD cycles per stream-step at the peak clock
    issue = 4 * valu + 16 * mfma
    lds_frac = t["SQ_LDS_IDX_ACTIVE"] / (avg_ms * 1e-3 * PEAK_CLOCK_GHZ * 1e9 * 256)     # LDS-active cycles of the 256 CUs / CU cycles of the launch
    hbm = pmc_traffic(kernel, streams, args)
    fr = {"mfma_issue": 16 * mfma / avail, "valu_issue": 4 * valu / avail, "valu_plus_mfma_issue": issue / avail,
          "lds": lds_frac,
          "hbm": (hbm["hbm_bytes_per_launch"] / (avg_ms * 1e-3) / 1e9 / PEAK_HBM_GBS) if hbm else None}
    binds = max((k for k in ("valu_plus_mfma_issue", "lds", "hbm") if fr[k] is not None), key=lambda k: fr[k])
    return {"wave_instructions_per_stream_step": {"valu": round(valu, 1), "mfma": round(mfma, 1), "lds": round(lds, 1)},
            "simd_cycles_per_stream_step": {"available_at_2.4GHz": round(avail, 0), "mfma_issue": round(16 * mfma, 0), "valu_issue": round(4 * valu, 0)},
            "frac_of_available": {k: (round(v, 4) if v is not None else None) for k, v in fr.items()}, "binds": binds,
            "lds_bank_conflict_frac": round(t["SQ_LDS_BANK_CONFLICT"] / max(t["SQ_LDS_IDX_ACTIVE"], 1.0), 4),
            "source": f"profiles/{src} (rocprofv3 --pmc passes of tools/pmc.sh on this workload and this build, src={tab['_csrc_sha16']}); the chip sits at its power cap in this regime "
                      "(profiles/r05_power.jsonl: 1,372 W of 1,400 W, sclk 1.99 of 2.4 GHz), so ~0.83 of 'available' is the practical ceiling"}


def make_pcm_pool(torch, dev, S, n_pool, kind, gen, rank):
    """Synthetic PCM int16 [S, 1280] x n_pool resident in HBM (generated in row blocks: S may be a million)."""
    pool = []
    if kind == "wav":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ref_streaming.npz"))
        wav = torch.from_numpy(np.concatenate([z["pcm/" + k] for k in ("alexa_test", "hey_mycroft_test", "hey_jane")])).to(dev)
        phase = (torch.arange(S, device=dev, dtype=torch.int64) + rank * S) * 997
    for i in range(n_pool):
        buf = torch.empty(S, 1280, device=dev, dtype=torch.int16)
        for lo in range(0, S, 131072):
            hi = min(S, lo + 131072)
            if kind == "noise":
                buf[lo:hi] = (torch.randn(hi - lo, 1280, device=dev, generator=gen) * 3000.0).round().clamp(-32768, 32767).to(torch.int16)
            elif kind == "uniform":
                buf[lo:hi] = torch.randint(-1000, 1000, (hi - lo, 1280), device=dev, generator=gen, dtype=torch.int32).to(torch.int16)
            else:
                buf[lo:hi] = wav[((phase[lo:hi, None] + (i * 1280 + torch.arange(1280, device=dev))[None, :]) % wav.numel())]
        pool.append(buf)
    return pool


def timed_run(torch, dist, eng, pool, scores, steps, warmup, dev, world, gatherer=None, timing=True):
    """`warmup` untimed + exactly `steps` timed device-resident steps, barrier + synchronize either side; max over ranks.
    Returns (seconds, kernel_times or None)."""
    def one(i):
        eng.step_device(pool[i % len(pool)].data_ptr(), 1, scores.data_ptr())
        if gatherer is not None:
            gatherer.gather(scores)                    # RCCL over xGMI: the path's only exchange

    def fence():
        if gatherer is not None:
            gatherer.flush()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for i in range(warmup):
        one(i)
    fence()
    if timing:
        eng.enable_timing(True)
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    fence()
    dt = time.perf_counter() - t0
    kt = eng.kernel_times() if timing else None
    eng.enable_timing(False)
    t = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item()), kt


def all_scores(torch, dist, scores, world, rank, backend):
    """Every rank's scores [S, n_labels] of the last step, in global stream order, as a host array on rank 0 (None elsewhere)."""
    if world == 1:
        return scores.cpu().numpy()
    local = scores if backend == "nccl" else scores.cpu()          # gloo gathers host tensors
    blocks = [torch.empty_like(local) for _ in range(world)] if rank == 0 else None
    dist.gather(local, blocks, dst=0)
    return torch.cat(blocks).cpu().numpy() if rank == 0 else None


def dump_scores(out_dir, rows, budget=60 << 20):
    """out_dir/scores.npy, fp32 [rows, n_labels]; above `budget` bytes (64 MB with room to spare) a fixed, seeded sample of the
    rows, kept in row order, so that two builds run with the same arguments compare output for output."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    if a.nbytes > budget:
        keep = budget // (a.nbytes // a.shape[0])
        a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "scores.npy"), a)


def parity_check(torch, eng, pool, scores, dev, head_names, ref, rank, vad=False):
    """The oracle-sampled parity check on the engine that is about to be timed: the 64 probe streams replace random rows
    of the synthetic batch for 16 frames (oracle/parity_sample.py); max |score - oracle| over the 1,024 (stream, step) pairs.
    With `vad` (BASELINE configs[4]) the reference side is OracleModel behind the voice-activity gate of model.py:366-381 and a gate
    decision whose compared value lies within 1e-3 of the threshold is skipped (and counted)."""
    from oracle import parity_sample as PS
    S = eng.n_streams
    ids = PS.probe_stream_ids(S, seed=7 + rank)
    ids_t = torch.from_numpy(ids).to(dev)
    pcm = torch.from_numpy(PS.probe_pcm()).to(dev)
    ref_labels = [str(x) for x in ref["labels"]]
    cols = [ref_labels.index(l) for l in PS.labels_of(head_names)]       # the engine's score columns (a multiclass head: n_out of them)
    want = torch.from_numpy(ref["scores"][:, :, cols]).to(dev)
    keep = torch.ones(PS.N_PROBE, PS.N_FRAMES, dtype=torch.bool, device=dev)
    if vad:
        g = ref["vad_window_max"]
        keep = torch.from_numpy(~(np.abs(g - PS.VAD_THRESHOLD) < 1e-3)).to(dev)
    eng.reset(None, ref["init_features"][-eng.feature_ring:])
    if vad:
        eng.reset_vad()
    worst = 0.0
    finite = True
    n_open = 0
    for t in range(PS.N_FRAMES):
        buf = pool[t % len(pool)].clone()
        buf[ids_t] = pcm[:, t * 1280:(t + 1) * 1280]
        eng.step_device(buf.data_ptr(), 1, scores.data_ptr())
        torch.cuda.synchronize(dev)
        got = scores[ids_t].double()
        finite = finite and bool(torch.isfinite(scores).all().item())
        k = keep[:, t]
        if bool(k.any().item()):
            worst = max(worst, float((got[k] - want[:, t][k]).abs().max().item()))
            n_open += int((want[:, t][k] != 0).any(dim=1).sum().item())
    eng.reset()
    if vad:
        eng.reset_vad()
    n_pairs = int(keep.sum().item())
    out = {"n_pairs": n_pairs, "max_abs_err": worst, "tolerance": 1e-4, "ok": bool(worst <= 1e-4 and finite),
           "streams_in_batch": S, "checker": "oracle/parity_sample.py: 64 probe streams (fixture WAVs, silence, LSB / full-scale noise, "
           "square waves, Gaussian RMS 30..12000) at random stream ids of this engine x 16 frames vs OracleModel (numpy fp32)"}
    if vad:
        out.update({"vad_gate": f"OracleModel(vad_threshold={PS.VAD_THRESHOLD}, vad_session=StandinVadSession): model.py:366-381 around the stand-in network",
                    "skipped_near_threshold": int(PS.N_PROBE * PS.N_FRAMES - n_pairs), "pairs_gate_open": n_open,
                    "pairs_gated_to_zero": n_pairs - n_open})
        out["ok"] = bool(out["ok"] and n_open > 0 and n_pairs - n_open > 0)
    return out


def quick_config(torch, dev, stream, S, head_names, steps, warmup, vad=False, host=False, parity_ref=None):
    """One more configuration timed inside the default run (driver-timed): HBM-resident PCM unless `host` (pinned host buffers through
    the pipelined oww_submit / oww_collect path); returns ms per step and frames/s."""
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    heads = {n: W.synthetic_head(n, 1234) for n in head_names}
    kw = dict(vad=W.synthetic_vad(1234), vad_threshold=0.5) if vad else {}
    eng = StreamEngine(S, heads, W.synthetic_embedding(1234), device=dev.index, use_mfma=3, hip_stream=stream.cuda_stream, **kw)
    try:
        eng.reset()
        gen = torch.Generator(device=dev)
        gen.manual_seed(0xA11CE + 17)
        pool = make_pcm_pool(torch, dev, S, 2, "noise", gen, 0)
        scores = torch.empty(S, eng.n_labels, device=dev, dtype=torch.float32)
        parity = None
        if parity_ref is not None:
            try:
                parity = parity_check(torch, eng, pool, scores, dev, head_names, parity_ref, 0, vad=vad)
            except Exception as e:
                parity = {"error": repr(e)[:300], "ok": False}
        if not host:
            dt, _ = timed_run(torch, None, eng, pool, scores, steps, warmup, dev, 1, timing=False)
        else:
            host_pool = [torch.empty(S, 1280, dtype=torch.int16, pin_memory=True).copy_(t).numpy() for t in pool]
            host_scores = torch.empty(S, eng.n_labels, dtype=torch.float32, pin_memory=True).numpy()
            n_in = 0
            def pump(n):
                nonlocal n_in
                for i in range(n):
                    eng.submit(host_pool[i % 2])
                    n_in += 1
                    if n_in == 2:
                        eng.collect(host_scores); n_in -= 1
                while n_in:
                    eng.collect(host_scores); n_in -= 1
                torch.cuda.synchronize(dev)
            pump(warmup)
            t0 = time.perf_counter()
            pump(steps)
            dt = time.perf_counter() - t0
            scores = torch.from_numpy(host_scores).to(dev)
        ok = bool(torch.isfinite(scores).all().item()) and bool(((scores >= 0) & (scores <= 1)).all().item()) and not eng.range_status()
        rec = {"streams": S, "heads": list(head_names), "steps": steps, "warmup": warmup, "ms_per_step": round(1e3 * dt / steps, 4),
               "value": round(S * steps / dt, 1), "unit": "frames/s", "scores_valid": ok}
        if parity_ref is not None:
            rec["parity"] = parity
        return rec
    finally:
        eng.close()


def masked_leg(torch, dev, stream, S, head_names):
    """oww_step_masked at 10 / 25 / 50 / 100 % participation (mask on the host, PCM resident in HBM): the serving edge's step for the
    connections that have a full chunk (examples/web/streaming_server.py:49-66).  Two placements of the same number of participants:
    `random` = connections sit at arbitrary stream slots (every 8-stream group holds somebody at 50 %), `packed` = slots handed out by
    serve.SlotAllocator from each connection's cohort key (80 ms messages, random arrival times), the participants of a step being
    the connections whose phase bins fall due in that pump round -- what FanInServer's placement produces for real-time clients."""
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    from openwakeword_amd import serve
    heads = {n: W.synthetic_head(n, 1234) for n in head_names}
    eng = StreamEngine(S, heads, W.synthetic_embedding(1234), device=dev.index, use_mfma=3, hip_stream=stream.cuda_stream)
    try:
        eng.reset()
        gen = torch.Generator(device=dev)
        gen.manual_seed(0xA11CE + 23)
        pool = make_pcm_pool(torch, dev, S, 2, "noise", gen, 0)
        scores = torch.zeros(S, eng.n_labels, device=dev, dtype=torch.float32)
        rng = np.random.default_rng(17)
        # packed placement: S connections arriving at random times, one 80 ms message each
        al = serve.SlotAllocator(S, group=32, distance=serve.cohort_distance)
        keys = [serve.cohort_key(0.080, t) for t in rng.random(S) * 600.0]
        slot = np.fromiter((al.alloc(k) for k in keys), dtype=np.int64, count=S)
        phase = np.fromiter((k[1] for k in keys), dtype=np.int64, count=S)
        NB = serve.N_PHASE_BINS

        def packed_masks(frac):
            width = max(1, int(round(frac * NB)))                      # phase bins due per pump round
            out = []
            for r in range(4):
                m = np.zeros(S, np.uint8)
                bins = [(r * width + j) % NB for j in range(width)]
                m[slot[np.isin(phase, bins)]] = 1
                out.append(m)
            return out

        def run(masks):
            for i in range(5):
                eng.step_masked_device(pool[i % 2].data_ptr(), masks[i % 4], scores.data_ptr())
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            n = 20
            for i in range(n):
                eng.step_masked_device(pool[i % 2].data_ptr(), masks[i % 4], scores.data_ptr())
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            part = sum(int(m.sum()) for m in masks) / 4
            g8 = float(np.mean([m[: S // 8 * 8].reshape(-1, 8).any(axis=1).mean() for m in masks]))
            return {"ms_per_step": round(1e3 * dt / n, 4), "stream_steps_per_s": round(part * n / dt, 1),
                    "participation": round(part / S, 4), "groups_of_8_touched": round(g8, 4)}

        out = {}
        for frac in (0.1, 0.25, 0.5, 1.0):
            out[f"participation_{int(frac * 100)}pct"] = run([(rng.random(S) < frac).astype(np.uint8) for _ in range(4)])
        out["packed"] = {f"participation_{int(frac * 100)}pct": run(packed_masks(frac)) for frac in (0.125, 0.25, 0.5)}
        out["packed"]["placement"] = ("serve.SlotAllocator: 32-stream blocks per cohort key (message period, arrival phase in 8 bins); a round's "
                                      "participants = the connections of the phase bins due")
        out["streams"] = S
        out["scores_valid"] = bool(torch.isfinite(scores).all().item()) and not eng.range_status()
        out["note"] = ("host-side list building included; below 7/8 participation only the stage groups that hold a participating stream are "
                       "launched, so the cost follows the groups touched: 'random' placement touches nearly all of them at 50 %")
        return out
    finally:
        eng.close()


def leg_resident_1m(args):
    """Child-process leg: 1,048,576 streams resident in one handle on one GPU (north star: >= 1 M concurrent streams on a
    node; this shows the whole million also FITS one GPU and what a step of it costs)."""
    import torch
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S = args.streams
    free0, total = torch.cuda.mem_get_info(dev)
    heads = {n: W.synthetic_head(n, 1234) for n in args.heads.split(",") if n}
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    eng = StreamEngine(S, heads, W.synthetic_embedding(1234), device=0, use_mfma=3, hip_stream=stream.cuda_stream)
    eng.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xA11CE)
    pool = make_pcm_pool(torch, dev, S, 2, "noise", gen, 0)
    scores = torch.empty(S, eng.n_labels, device=dev, dtype=torch.float32)
    # the oracle-sampled parity check inside the resident million: 64 probe streams at random ids of THIS
    # engine x 16 frames; the reference was computed (and cached) by the parent before it touched HIP
    parity = None
    if set(heads) <= {"alexa", "hey_mycroft", "hey_jarvis"} and not args.no_parity:
        try:
            from oracle import parity_sample as PS
            parity = parity_check(torch, eng, pool, scores, dev, list(heads), PS.oracle_reference(), 0)
        except Exception as e:
            parity = {"error": repr(e)[:200]}
    dt, _ = timed_run(torch, None, eng, pool, scores, args.steps, args.warmup, dev, 1, timing=False)
    free1, _ = torch.cuda.mem_get_info(dev)
    ok = bool(torch.isfinite(scores).all().item()) and bool(((scores >= 0) & (scores <= 1)).all().item())
    ms = 1e3 * dt / args.steps
    print(json.dumps({"streams": S, "heads": list(heads), "handles": 1, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(ms, 3), "value": round(S * args.steps / dt, 1), "unit": "frames/s",
                      "realtime": bool(ms < 80.0), "realtime_budget_ms": 80.0,
                      "device_memory_used_gb": round((free0 - free1) / 2**30, 2), "device_memory_total_gb": round(total / 2**30, 1),
                      "scores_valid": ok, "parity": parity}))


def _embed_cpu_worker(a):
    seed, budget_s, n = a
    import torch
    torch.set_num_threads(1)
    from openwakeword_amd import weights as W
    from oracle.oww_oracle_torch import TorchCpuPort
    port = TorchCpuPort(W.synthetic_embedding(1234), {}, threads=1)
    clip = W.synthetic_pcm(1, n, seed=seed)
    done, t0 = 0, time.perf_counter()
    while True:
        spec = port.mel(clip)[0]
        port.embed(torch.stack([spec[i:i + 76] for i in range(0, spec.shape[0] - 75, 8)]))      # utils.py:354-385: every window, full CNN
        done += 1
        if time.perf_counter() - t0 >= budget_s:
            break
    return done, time.perf_counter() - t0


def leg_embed_clips(args):
    """Child-process leg, SURVEY §8(f)1: bulk clip embedding (AudioFeatures.embed_clips / compute_features_from_generator,
    /root/reference/openwakeword/utils.py:354-385, 542-601) -- `--streams` clips of 2 s, PCM and embeddings resident in HBM, one
    oww_embed_clips call per repetition.  Reports clips/s, the flops the incremental CNN EXECUTES (9 lead-in steps + one step per
    window, 11.225 MFLOP each) against the f16 MFMA peak, the per-kernel times of one call, parity against the vectors the reference's
    own AudioFeatures.embed_clips produced on the exporter-written files (tests/golden/ref_onnx_files.npz: embed/*), and the
    reference's algorithm (torch-CPU port: mel per clip, every 76-row window through the full CNN) timed on the host cores."""
    import multiprocessing as mp
    n = 32000
    cpu = None
    if not args.no_cpu_baseline:                        # forked workers: before HIP is touched
        from oracle.parity_sample import effective_cpus
        cores = effective_cpus()
        with mp.get_context("fork").Pool(cores) as pool:
            res = pool.map(_embed_cpu_worker, [(50 + i, args.cpu_seconds, n) for i in range(cores)])
        clips, wall = sum(r[0] for r in res), max(r[1] for r in res)
        cpu = {"value": round(clips / wall, 2), "unit": "clips/s", "cores": cores, "kind": "port",
               "sample": f"{clips} clips of 2 s in {wall:.1f} s on {cores} single-threaded processes (the reference's form: full-window CNN per embedding, torch-CPU)"}
    import torch
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = args.streams
    frames = (n - 512) // 160 + 1
    n_out = (frames - 76) // 8 + 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    pcm = (torch.randn(B, n, device=dev, generator=gen) * 3000.0).round().clamp(-32768, 32767).to(torch.int16)
    out = torch.empty(B, n_out, 96, device=dev, dtype=torch.float32)
    eng = StreamEngine(B, {}, W.synthetic_embedding(1234), device=0, use_mfma=3)
    try:
        # parity: the reference's own embed_clips on the exporter-written files (4 clips of 2 s) through the same entry point
        parity = None
        try:
            z = np.load(os.path.join(ROOT, "tests", "golden", "ref_onnx_files.npz"))
            got = eng.embed_clips(np.ascontiguousarray(z["embed/pcm"]))
            want = z["embed/embed_clips"]
            err = float(np.abs(got - want).max())
            parity = {"n_clips": int(want.shape[0]), "windows": int(want.shape[1]), "max_abs_err": err, "tolerance": 2e-4 * max(1.0, float(np.abs(want).max())),
                      "ok": bool(err <= 2e-4 * max(1.0, float(np.abs(want).max()))),
                      "checker": "tests/golden/ref_onnx_files.npz embed/*: /root/reference's AudioFeatures.embed_clips on model files written by "
                                 "PyTorch's exporter from the same weights (tests/golden/make_golden_onnx.py)"}
        except Exception as e:                          # noqa: BLE001
            parity = {"error": repr(e)[:300], "ok": False}
        eng.embed_clips_device(pcm.data_ptr(), B, n, out.data_ptr())                   # warm-up (the call synchronises)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.embed_clips_device(pcm.data_ptr(), B, n, out.data_ptr())
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        ok = bool(torch.isfinite(out).all().item())
        eng.enable_timing(True)
        eng.embed_clips_device(pcm.data_ptr(), B, n, out.data_ptr())
        kt = {k: round(v["ms"], 3) for k, v in eng.kernel_times().items() if v["launches"]}
        eng.enable_timing(False)
    finally:
        eng.close()
    steps = 9 + n_out
    flops = B * steps * MFLOP_CNN_STEP * 1e6
    tf = flops / dt / 1e12
    cnn_ms = sum(v for k, v in kt.items() if k.startswith("stage"))
    rec = {"metric": "clip embeddings (AudioFeatures.embed_clips), clips/s on 1 GPU", "value": round(B / dt, 1), "unit": "clips/s",
           "clips": B, "clip_seconds": 2.0, "windows_per_clip": n_out, "ms_per_call": round(dt * 1e3, 2), "calls_timed": args.steps,
           "audio_seconds_per_second": round(B * 2.0 / dt, 1), "embeddings_per_second": round(B * n_out / dt, 1),
           "kernel_ms_per_call": kt,
           "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_F16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_F16_TFLOPS, 4),
                        "cnn_kernels_only": round(flops / (cnn_ms * 1e-3) / 1e12 / PEAK_F16_TFLOPS, 4) if cnn_ms else None,
                        "flops_per_clip": round(steps * MFLOP_CNN_STEP * 1e6), "traffic": None,
                        "note": f"executed flops only: {steps} incremental CNN steps of {MFLOP_CNN_STEP} MFLOP per clip (9 lead-in + one per window); "
                                f"the reference's full-window form would execute {n_out} x 83.9 MFLOP for the same output"},
           "finite": ok, "parity": parity, "data": "synthetic Gaussian int16 PCM (RMS 3000), synthetic weights seed 1234", "cpu_baseline": cpu}
    if cpu:
        rec["x_cpu_host"] = round(rec["value"] / cpu["value"], 1)
    print(json.dumps(rec))


def self_launch(n: int) -> None:
    """A bare `python bench.py --gpus N` (N > 1, no torchrun environment): re-execute this command line under
    torch.distributed.run -- one rank per GPU, rendezvous on 127.0.0.1 at a free port -- and pass the ranks' output through
    (rank 0 prints the one JSON line).  The driver's explicit `python -m torch.distributed.run ... bench.py --gpus N` form
    never gets here: it sets RANK / WORLD_SIZE."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    sys.stdout.flush()
    raise SystemExit(subprocess.run(cmd, env=env, cwd=os.getcwd()).returncode)


class CAbiGather:
    """Delivery of the scores through the C ABI's own exchange (include/owwhip.h: oww_comm_init / oww_gather_scores -- one grouped
    ncclSend (every rank) / ncclRecv x world (rank 0) on the handle's stream per step) instead of torch.distributed.  The
    communicator id travels over the process group here; any side channel will do.  Same interface as shard.ScoreGather."""

    def __init__(self, torch, dist, eng, S, NL, dev, world, rank):
        from openwakeword_amd.engine import StreamEngine
        box = [StreamEngine.comm_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(box, src=0)
        eng.comm_init(box[0], rank, world)
        self.eng, self.rank, self.world = eng, rank, world
        self.ranks = eng.comm_count()                      # ncclCommCount
        self.out = torch.full((S * world, NL), -1.0, device=dev, dtype=torch.float32) if rank == 0 else None
        self.counts = [S] * world
        self.collectives = 0

    def gather(self, scores):
        self.eng.gather_scores(self.out.data_ptr() if self.rank == 0 else 0, self.counts)
        self.collectives += 1
        return self.out

    def flush(self):
        self.eng.sync()

    def close(self):
        self.eng.comm_destroy()


def c_abi_gather_pass(torch, dist, eng, pool, scores, dev, world, rank, steps, warmup):
    """The headline steps once more with the scores delivered by CAbiGather; rank 0 then checks what arrived against a
    torch.distributed gather of the same scores.  Returns the record for the JSON line."""
    S, NL = scores.shape
    g = CAbiGather(torch, dist, eng, S, NL, dev, world, rank)
    try:
        dt, _ = timed_run(torch, dist, eng, pool, scores, steps, warmup, dev, world, g, False)
        if world > 1:
            blocks = [torch.empty_like(scores) for _ in range(world)] if rank == 0 else None
            dist.gather(scores, blocks, dst=0)
            equal = bool(torch.equal(g.out, torch.cat(blocks))) if rank == 0 else None
        else:
            equal = bool(torch.equal(g.out, scores))
        return {"exchange": "oww_gather_scores: grouped ncclSend (every rank) / ncclRecv x world (rank 0) on the handle's stream, every step",
                "rccl_ranks": g.ranks, "steps": steps, "warmup": warmup, "ms_per_step": round(1e3 * dt / steps, 4),
                "value": round(S * world * steps / dt, 1), "unit": "frames/s", "bytes_per_rank_and_step": int(S * NL * 4),
                "gathered_equals_scores": equal}
    finally:
        g.close()


def with_watchdog(seconds, on_timeout, fn):
    """Run fn(); if it has not returned after `seconds` (a collective that never completes cannot be cancelled from the host),
    call on_timeout() and end the process with exit code 0 -- the headline record must not be lost to an extra one."""
    import threading
    done = threading.Event()

    def guard():
        if not done.wait(seconds):
            try:
                on_timeout()
            finally:
                sys.stdout.flush()
                os._exit(0)
    threading.Thread(target=guard, daemon=True).start()
    try:
        return fn()
    finally:
        done.set()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--streams", type=int, default=131072, help="streams per GPU")
    ap.add_argument("--heads", default="alexa,hey_mycroft,hey_jarvis")
    ap.add_argument("--valu", action="store_true", help="plain-VALU kernels instead of MFMA (A/B only)")
    ap.add_argument("--lds-mfma", action="store_true", help="LDS-tiled MFMA kernels instead of the register-resident ones (A/B only)")
    ap.add_argument("--fp32", action="store_true", help="exact-fp32 MFMA form of the register-resident kernels instead of the default "
                    "fp16-split form (three f16 MFMAs per fp32 product)")
    ap.add_argument("--f16x3", action="store_true", help="(default) fp16-split form; kept for A/B scripts")
    ap.add_argument("--graph", action="store_true", help="replay the step from a hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="wall-clock budget of the cpu_baseline leg")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle-sampled parity check of the timed engine")
    ap.add_argument("--no-extras", action="store_true", help="skip the sustained / fp32_exact / resident_1m records")
    ap.add_argument("--sustained-steps", type=int, default=250)
    ap.add_argument("--sustained-warmup", type=int, default=100)
    ap.add_argument("--gather-every", type=int, default=1, help="N > 1: gather scores to rank 0 every K steps (one K-times larger collective)")
    ap.add_argument("--gather", choices=("dist", "c_abi"), default="dist",
                    help="delivery of the scores to rank 0 inside the timed region: dist = torch.distributed gather (backend nccl = RCCL); "
                         "c_abi = the library's own grouped ncclSend / ncclRecv exchange (oww_comm_init / oww_gather_scores; also runs "
                         "with one rank, as a send-to-self through RCCL)")
    ap.add_argument("--vad", action="store_true", help="BASELINE configs[4]: the voice-activity stand-in network + gate fused into the step")
    ap.add_argument("--leg", default="", help="(internal) run one extra record in this process and print its JSON: resident_1m | embed_clips")
    ap.add_argument("--pcm-pool", type=int, default=4, help="distinct PCM buffers cycled through")
    ap.add_argument("--pcm", choices=("noise", "uniform", "wav"), default="noise",
                    help="synthetic input (SURVEY 8d): noise = Gaussian RMS 3000 (default); uniform = the reference tests' "
                         "randint(-1000, 1000) (tests/test_models.py:57); wav = the reference's three fixture clips tiled end to end, "
                         "stream s starting at sample (s * 997) mod length")
    ap.add_argument("--host-pcm", action="store_true", help="PCIe-inclusive variant (NOT the headline number): PCM handed over as pinned "
                    "host buffers and scores returned to the host every step through the pipelined oww_submit / oww_collect path "
                    "(upload of step t+1 overlaps the kernels of step t)")
    ap.add_argument("--host-pcm-blocking", action="store_true", help="the same through the blocking oww_step(host, host) call (no overlap)")
    ap.add_argument("--full", action="store_true", help="besides the headline steps: CPU baseline, oracle-sampled parity, per-kernel "
                    "timing pass and roofline, and the extra records (the --no-* switches thin these out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the scores of the last timed step to DIR/scores.npy")
    args = ap.parse_args()

    if args.leg == "resident_1m":
        return leg_resident_1m(args)
    if args.leg == "embed_clips":
        return leg_embed_clips(args)

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank0 = rank == 0
    head_names = [n for n in args.heads.split(",") if n]
    cpu_base = None
    t_pre = time.perf_counter()
    if rank0 and args.full and not args.no_cpu_baseline:
        # forked single-threaded workers: must run before this process touches HIP.  Rank 0 times it at EVERY N (the other ranks sit
        # in the rendezvous below meanwhile, so the host cores are free): an N > 1 line without it would read "unmeasured".
        from oracle import cpu_baseline
        cpu_base = cpu_baseline.run(head_names, budget_s=args.cpu_seconds)
    parity_ref = None
    family_ok = not (args.valu or args.lds_mfma)
    PS6 = ("alexa", "hey_mycroft", "hey_jarvis", "hey_rhasspy", "timer", "weather")        # (= oracle.parity_sample.HEADS6)
    want_parity = (args.full and not args.no_parity and family_ok and set(head_names) <= set(PS6)
                   and not (args.host_pcm or args.host_pcm_blocking))
    vad_parity_ref = default6_ref = None
    if want_parity and rank0:
        from oracle import parity_sample as PS
        # computed once by a child interpreter, cached under $TMPDIR (the three-head sample unless the run names other catalogue heads)
        parity_ref = PS.oracle_reference(vad=args.vad, head_names=PS.HEADS3 if set(head_names) <= set(PS.HEADS3) else tuple(head_names))
        if world == 1 and not args.no_extras and not args.vad and set(head_names) == set(PS.HEADS3):
            vad_parity_ref = PS.oracle_reference(vad=True)     # for the vad_fused record (BASELINE configs[4])
            default6_ref = PS.oracle_reference(head_names=PS.HEADS6)      # for configs.default6 (the reference's default six models)

    t_pre_done = time.perf_counter()
    import torch
    import torch.distributed as dist
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine

    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    # (testing aid: OWW_BENCH_ONE_GPU=1 puts every rank on device 0 with the gloo backend, to exercise the N > 1 code path on a
    #  single-GPU box; never used for reported numbers)
    one_gpu = os.environ.get("OWW_BENCH_ONE_GPU") == "1"
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # rank 0 arrives late by design: it has timed the CPU baseline (--cpu-seconds) and computed the oracle reference of the parity
        # sample (a child interpreter, 20-60 s on a loaded host) before it joins, so the rendezvous and the first collective get an
        # explicit, generous timeout instead of whatever the backend defaults to
        from datetime import timedelta
        pg_timeout = timedelta(seconds=max(1800.0, 20.0 * args.cpu_seconds + 600.0))
        if one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world, timeout=pg_timeout)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=pg_timeout)
        if want_parity:
            dist.barrier()                               # rank 0 wrote the cache file before it joined
            if not rank0:
                from oracle import parity_sample as PS
                parity_ref = PS.oracle_reference(vad=args.vad, head_names=PS.HEADS3 if set(head_names) <= set(PS.HEADS3) else tuple(head_names))

    S = args.streams
    emb = W.synthetic_embedding(1234)
    heads = {n: W.synthetic_head(n, 1234) for n in head_names}
    # one side stream carries the engine's kernels AND the RCCL gather, so they are ordered without host syncs
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    family = 0 if args.valu else 2 if args.lds_mfma else 1 if args.fp32 else 3
    vad_kw = dict(vad=W.synthetic_vad(1234), vad_threshold=0.5) if args.vad else {}
    eng = StreamEngine(S, heads, emb, device=local_rank, use_mfma=family, hip_stream=stream.cuda_stream, **vad_kw)
    NL = eng.n_labels
    eng.reset()
    if args.graph:
        eng.use_graph(True)

    # synthetic PCM resident in HBM: a different seed per rank (independent streams)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xA11CE + rank)
    pool = make_pcm_pool(torch, dev, S, max(1, args.pcm_pool), args.pcm, gen, rank)
    scores = torch.empty(S, NL, device=dev, dtype=torch.float32)
    from openwakeword_amd.shard import ScoreGather
    if args.gather == "c_abi":
        if one_gpu and world > 1:
            raise SystemExit("--gather c_abi needs one GPU per rank (RCCL refuses two ranks on one device); OWW_BENCH_ONE_GPU runs use --gather dist")
        if args.gather_every != 1:
            raise SystemExit("--gather c_abi delivers every step (--gather-every applies to --gather dist)")
        gatherer = CAbiGather(torch, dist, eng, S, NL, dev, world, rank)
    else:
        gatherer = ScoreGather(S * world, NL, dev, every=args.gather_every) if world > 1 else None      # rank r owns global streams [r*S, (r+1)*S)
    backend = dist.get_backend() if world > 1 else None
    rccl_ranks = gatherer.ranks if args.gather == "c_abi" else (dist.get_world_size() if backend == "nccl" else 0)

    parity = None
    if parity_ref is not None:
        parity = parity_check(torch, eng, pool, scores, dev, head_names, parity_ref, rank, vad=args.vad)
        if world > 1:
            t = torch.tensor([parity["max_abs_err"]], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            parity["max_abs_err"] = float(t.item())
            n = torch.tensor([parity["n_pairs"], int(parity["ok"])], device=dev, dtype=torch.int64)
            dist.all_reduce(n[:1], op=dist.ReduceOp.SUM)
            dist.all_reduce(n[1:], op=dist.ReduceOp.MIN)
            parity["n_pairs"] = int(n[0].item())
            parity["ok"] = bool(n[1].item()) and bool(parity["max_abs_err"] <= parity["tolerance"])

    host = args.host_pcm or args.host_pcm_blocking
    timing = args.full and not args.no_kernel_timing and not args.graph
    extras_on = args.full and not args.no_extras
    kpass = None
    if host:
        host_pool = [torch.empty(S, 1280, dtype=torch.int16, pin_memory=True).copy_(t).numpy() for t in pool]
        host_scores = torch.empty(S, NL, dtype=torch.float32, pin_memory=True).numpy()
        inflight = [0]

        def one_step(i):
            if args.host_pcm_blocking:
                eng.step(host_pool[i % len(host_pool)], out=host_scores)     # H2D + kernels + D2H, blocking
                return
            eng.submit(host_pool[i % len(host_pool)])                        # step i's upload overlaps step i-1's kernels
            inflight[0] += 1
            if inflight[0] == 2:
                eng.collect(host_scores)
                inflight[0] -= 1

        def fence():
            while inflight[0]:
                eng.collect(host_scores)
                inflight[0] -= 1
            torch.cuda.synchronize(dev)

        for i in range(args.warmup):
            one_step(i)
        fence()
        if timing:
            eng.enable_timing(True)
        t0 = time.perf_counter()
        for i in range(args.steps):
            one_step(i)
        fence()
        dt_max = time.perf_counter() - t0
        ktimes = eng.kernel_times() if timing else None
        eng.enable_timing(False)
        scores = torch.from_numpy(host_scores).to(dev)
    else:
        # the timed K steps run WITHOUT per-kernel hipEvents (the optional block-pipelined step, OWW_BLOCKS > 1, is switched off by
        # the library while kernels are being timed one by one; the default is one block, so both passes run the same launches)
        dt_max, _ = timed_run(torch, dist, eng, pool, scores, args.steps, args.warmup, dev, world, gatherer, False)
        ktimes = None
    if args.dump_outputs:                       # before any later pass overwrites the last timed step's scores
        rows = all_scores(torch, dist, scores, world, rank, backend)
        if rank0:
            dump_scores(args.dump_outputs, rows)
    if timing and not host:
        n_k = max(4, min(args.steps, 10))
        dt_k, ktimes = timed_run(torch, dist, eng, pool, scores, n_k, 2, dev, world, gatherer, True)
        kpass = {"steps": n_k, "launches": int(sum(v["launches"] for v in ktimes.values())), "ms_per_step": round(1e3 * dt_k / n_k, 4),
                 "note": "separate pass after the timed steps: per-kernel hipEvents on, block pipelining off (kernels run one after the other)"}
    ok = bool(torch.isfinite(scores).all().item()) and bool(((scores >= 0) & (scores <= 1)).all().item())
    range_flag = eng.range_status() if family == 3 else False

    extras = {}
    if rank0 and world == 1 and extras_on and not host:
        # ---- c_abi_gather with ONE rank: the C ABI's RCCL exchange as a send-to-self on the handle's stream (what a 1-GPU box can show)
        if args.gather == "dist" and family == 3:
            try:
                extras["c_abi_gather"] = c_abi_gather_pass(torch, dist, eng, pool, scores, dev, 1, 0, 20, 5)
            except Exception as e:
                extras["c_abi_gather"] = {"error": repr(e)[:400]}
        # ---- sustained: the same configuration for 100 warm-up + 250 timed steps (the part is power-limited: a 20-step burst reads low)
        dt_s, _ = timed_run(torch, dist, eng, pool, scores, args.sustained_steps, args.sustained_warmup, dev, 1, None, timing=False)
        extras["sustained"] = {"steps": args.sustained_steps, "warmup": args.sustained_warmup,
                               "ms_per_step": round(1e3 * dt_s / args.sustained_steps, 4),
                               "value": round(S * args.sustained_steps / dt_s, 1), "unit": "frames/s"}
        # ---- fp32_exact: the reference's own arithmetic type (exact fp32 MFMA family), same workload
        if family == 3:
            eng.close()
            eng32 = StreamEngine(S, heads, emb, device=local_rank, use_mfma=1, hip_stream=stream.cuda_stream, **vad_kw)
            eng32.reset()
            dt_f, kt_f = timed_run(torch, dist, eng32, pool, scores, 20, 5, dev, 1, None, timing=True)
            extras["fp32_exact"] = {"kernels": "mfma_rr_fp32", "steps": 20, "warmup": 5, "ms_per_step": round(1e3 * dt_f / 20, 4),
                                    "value": round(S * 20 / dt_f, 1), "unit": "frames/s", "dtype": "f32"}
            # this family still runs the log-mel front end as its own launch: the HBM figure the north star asks for on "the mel
            # kernel" (in the default family its rows never reach HBM, see fused_front).  Algorithmic bytes per stream-step
            # (SURVEY 8d): 2,560 B of new PCM + 960 B tail read + 960 B tail written + 1,024 B of mel rows written
            if kt_f and kt_f["mel"]["launches"]:
                mel_ms = kt_f["mel"]["ms"] / kt_f["mel"]["launches"]
                gbs = S * 5504 / (mel_ms * 1e-3) / 1e9
                extras["fp32_exact"]["mel_kernel"] = {"avg_ms": round(mel_ms, 4), "bytes_per_stream_step": 5504, "achieved": round(gbs, 1),
                                                      "unit": "GB/s", "peak": PEAK_HBM_GBS, "frac": round(gbs / PEAK_HBM_GBS, 4),
                                                      "fp32_valu_tflops": round(S * 0.10e6 / (mel_ms * 1e-3) / 1e12, 2),
                                                      "note": "separate mel launch (fp32 kernel families, multi-chunk calls, clip embedding); "
                                                              "FFT butterflies and LDS transposes bound it, not HBM"}
            eng32.close()
            eng = None
        # ---- the other BASELINE configurations and the serving-edge forms of the headline one, driver-timed:
        #      configs[1] 4,096 x hey_jarvis, configs[2] 65,536 x 3 heads, configs[4] = + the VAD stand-in fused into every step,
        #      and the headline batch with its PCM arriving over PCIe every step (pipelined oww_submit / oww_collect)
        del pool
        if eng is not None:
            eng.close()
            eng = None
        torch.cuda.empty_cache()
        if family == 3 and not args.vad:
            try:
                extras["configs"] = {
                    # (a 0.3 ms step: 1,000 timed steps after 300 of warm-up = 0.4 s -- a 50-step burst is over before a lightly
                    #  loaded chip has left its low-power clocks, which is what made this figure swing 0.35 .. 0.75 ms box to box)
                    "c1_4096x1": quick_config(torch, dev, stream, 4096, ["hey_jarvis"], 1000, 300),
                    "c2_65536x3": quick_config(torch, dev, stream, 65536, head_names, 50, 10),
                    # the reference's default Model(): all six pretrained models (model.py:84-87) -- five 64-unit heads (six nets: two
                    # launches of the f16-split heads kernel) + the multiclass `timer` (T = 34, 128 units, 7 classes: its wide form);
                    # 12 score columns per stream, held to the oracle on the same 1,024 (stream, step) pairs
                    "default6_131072x6": quick_config(torch, dev, stream, S, list(PS6), 20, 5, parity_ref=default6_ref),
                }
                extras["vad_fused"] = quick_config(torch, dev, stream, S, head_names, 20, 5, vad=True, parity_ref=vad_parity_ref)
                extras["masked_step"] = masked_leg(torch, dev, stream, S, head_names)
                extras["host_pcm"] = dict(quick_config(torch, dev, stream, S, head_names, 20, 5, host=True),
                                          note="PCIe-inclusive (pinned host PCM in, scores out, two steps in flight): never the headline value")
            except Exception as e:
                extras["configs_error"] = repr(e)[:400]
            torch.cuda.empty_cache()
        # ---- embed_clips: SURVEY §8(f)1, bulk clip embedding on the same kernels (child process: its CPU leg forks before HIP)
        try:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "embed_clips", "--streams", "16384", "--steps", "5", "--cpu-seconds", "6"]
            cmd += ["--no-cpu-baseline"] if args.no_cpu_baseline else []
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            extras["embed_clips"] = json.loads(line[-1]) if (r.returncode == 0 and line) else {"error": (r.stderr or r.stdout)[-400:]}
        except Exception as e:
            extras["embed_clips"] = {"error": repr(e)[:400]}
        # ---- resident_1m: a million streams in ONE handle on this GPU, in a child process (own 73 GB of state)
        try:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "resident_1m", "--streams", str(1 << 20), "--heads", args.heads,
                   "--steps", "10", "--warmup", "3"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            extras["resident_1m"] = json.loads(line[-1]) if (r.returncode == 0 and line) else {"error": (r.stderr or r.stdout)[-400:]}
        except Exception as e:                      # never let an extra record take the headline down
            extras["resident_1m"] = {"error": repr(e)[:400]}

    if rank == 0:
        total_frames = S * world * args.steps
        value = total_frames / dt_max
        out = {
            "metric": "real-time audio frames/sec (80 ms frame, 3 wakewords), whole job; real-time streams = value/12.5",
            "value": round(value, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt_max / args.steps, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": ("f32" if family != 3 else "f32 as 3xf16 split MFMA, fp32 accumulate"), "data": "synthetic" if args.pcm != "wav" else "synthetic (reference fixture clips tiled)",
            "config": {"workload": f"{S} concurrent 16 kHz streams per GPU x {len(heads)} heads ({','.join(heads)}), "
                                   "80 ms frames, BASELINE configs[3] per-GPU shard" if S == 131072 else
                                   f"{S} concurrent 16 kHz streams per GPU x {len(heads)} heads ({','.join(heads)}), 80 ms frames",
                       "streams_per_gpu": S, "heads": list(heads), "frame_samples": 1280, "sharding": f"stream-range x{world}",
                       "collective": ("oww_gather_scores (C ABI: grouped ncclSend / ncclRecv over RCCL) every step" if args.gather == "c_abi" else
                                      (f"RCCL gather of scores every {args.gather_every} step(s)" if not one_gpu else
                                       f"gloo gather every {args.gather_every} step(s) (OWW_BENCH_ONE_GPU testing aid: all ranks on device 0)") if world > 1 else "none"),
                       "gather": args.gather if (world > 1 or args.gather == "c_abi") else "none",
                       "rccl_ranks": int(rccl_ranks),
                       "pcm_distribution": {"noise": "Gaussian, RMS 3000", "uniform": "randint(-1000, 1000)", "wav": "fixture WAVs tiled, phase 997*s"}[args.pcm],
                       "pcm": ("pinned host buffers, PCIe-inclusive, " + ("blocking oww_step" if args.host_pcm_blocking else "pipelined oww_submit/oww_collect") +
                               " (not the headline configuration)") if host else "resident in HBM",
                       "kernels": "valu" if args.valu else ("mfma_lds" if args.lds_mfma else ("mfma_rr_fp32" if args.fp32 else "mfma_rr_f16x3")), "graph": bool(args.graph),
                       "vad": "stand-in network + gate fused into the step" if args.vad else "off", "weights": "synthetic seed 1234",
                       "step_blocks": int(os.environ.get("OWW_BLOCKS", "1")) if (family == 3 and S >= 16384 and not args.graph) else 1},
            "realtime_streams_extrapolated": round(value / REALTIME_STEPS_PER_S, 1),
            "realtime_streams_note": f"value / 12.5, extrapolated from the measured batch of {S * world} streams; see resident_1m for a resident million",
            "frames_per_sec_per_gpu": round(value / world, 1),
            "scores_valid": ok, "f16_range_flag": bool(range_flag),
            "parity": parity,
        }
        if ktimes:
            per = {k: (v["ms"] / max(v["launches"], 1)) for k, v in ktimes.items()}
            out["kernel_ms"] = {k: round(v, 4) for k, v in per.items()}
            out["kernel_timing_pass"] = kpass
            # launches of the pass the events were recorded in, per step of THAT pass (the host-PCM form records during the timed steps)
            out["launches_per_step"] = round(sum(v["launches"] for v in ktimes.values()) / max(kpass["steps"] if kpass else args.steps, 1), 2)
            # Roofline kernel = the LONGEST launch of the step (not the longest "matrix-bound" one).  With the mel front end
            # fused into stage A (default: the mel class has no launches) that launch also carries the FFT / log-mel work; its
            # algorithmic flops are stage A's + the FFT form of the front end, priced against the matrix peak like every stage, and
            # "composite" names what actually binds it (VALU + MFMA issue cycles, LDS cycles, HBM bytes).
            fused_front = per["mel"] == 0 and per["stageA"] > 0
            dom = max(STAGE_FLOPS, key=lambda k: per[k])
            # (the fused front end and stage C run within a few percent of each other and swap places from box to box: the front end is
            #  named whenever it is within 3 % of the longest launch, so that the headline roofline tracks one kernel -- VERDICT r04 weak 8)
            if fused_front and per["stageA"] >= 0.97 * per[dom]:
                dom = "stageA"
            f16 = family == 3
            peak = PEAK_F16_TFLOPS if f16 else PEAK_FP32_TFLOPS

            def stage_flops(k):
                return STAGE_FLOPS[k] + (MEL_FLOPS if (fused_front and k == "stageA") else 0)

            def stage_roof(k):
                if per[k] <= 0:
                    return None
                tf = stage_flops(k) * S / (per[k] * 1e-3) / 1e12          # algorithmic (fp32-equivalent) flops only
                r = {"achieved": round(tf, 2), "unit": "TFLOP/s", "frac": round(tf / peak, 4), "avg_ms": round(per[k], 4)}
                if f16:
                    ex = HX_MFMAS[k] * 16384 * S / (per[k] * 1e-3) / 1e12  # what the matrix pipe executes: 3 MFMAs per product + padding
                    r.update({"executed_f16_tflops": round(ex, 1), "executed_frac_of_f16_peak": round(ex / peak, 4),
                              "x_fp32_mfma_peak": round(tf / PEAK_FP32_TFLOPS, 3)})
                return r

            d = stage_roof(dom)
            out["roofline"] = {"bound": "mfma", "kernel": dom + (" (mel front end + stage A, one launch)" if fused_front and dom == "stageA" else ""),
                               "achieved": d["achieved"], "peak": peak, "unit": "TFLOP/s",
                               "frac": d["frac"], "traffic": pmc_traffic(dom, S, args),
                               "flops_per_launch": stage_flops(dom) * S, "avg_ms": round(per[dom], 4),
                               "composite": issue_bound(dom, S, per[dom], args)}
            if f16:
                out["roofline"].update({k: d[k] for k in ("executed_f16_tflops", "executed_frac_of_f16_peak", "x_fp32_mfma_peak")})
                out["roofline"]["note"] = ("fp32 products evaluated as 3 f16 MFMAs (hi/lo operand split, fp32 accumulate): 'achieved' counts the "
                                           "algorithmic fp32 flops once, against the dense f16 MFMA peak; the scheme's own ceiling is peak/3")
            if fused_front:
                a = stage_roof("stageA")
                front_bytes = 2560 + 960 + 960                            # PCM in + 480-sample tail read and rewritten (the mel rows stay in LDS)
                out["fused_front"] = {"kernel": "mel front end + stage A in one launch (owwhip_fused.h)", "avg_ms": round(per["stageA"], 4),
                                      "share_of_step": round(per["stageA"] / sum(per.values()), 3),
                                      "mfma": a, "mel_hbm_bytes_per_stream_step": front_bytes,
                                      "mel_rows_to_hbm": 0, "composite": issue_bound("stageA", S, per["stageA"], args),
                                      "note": "FFT / log-mel phases are VALU + LDS work on the same waves that then run stage A's MFMAs"}
            cnn_ms = sum(per[k] for k in STAGE_FLOPS)
            cnn_tf = sum(STAGE_FLOPS.values()) * S / (cnn_ms * 1e-3) / 1e12
            hf = head_flops(heads) * S / (per["heads"] * 1e-3) / 1e12 if per["heads"] > 0 else 0.0
            mel_ms = per["mel"] if per["mel"] > 0 else None               # fused into stage A when the mel class has no launches
            out["roofline_all"] = {
                "cnn_all_stages": {"achieved": round(cnn_tf, 2), "unit": "TFLOP/s", "frac": round(cnn_tf / peak, 4),
                                   "x_fp32_mfma_peak": round(cnn_tf / PEAK_FP32_TFLOPS, 3)},
                **{k: dict(stage_roof(k) or {}, composite=issue_bound(k, S, per[k], args)) for k in STAGE_FLOPS},
                "heads": {"achieved": round(hf, 2), "unit": "TFLOP/s", "frac": round(hf / peak, 4)},
                "mel": ({"bound": "hbm", "achieved": round(MEL_BYTES * S / (mel_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS,
                         "unit": "GB/s", "frac": round(MEL_BYTES * S / (mel_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)} if mel_ms else
                        {"fused_into": "stageA", "note": "mel rows never reach HBM (BASELINE configs[2] 'mel+embedding fused')"}),
            }
        else:
            out["roofline"] = None
        out.update(extras)
        out["cpu_baseline"] = cpu_base
        out["pre_rendezvous_s"] = round(t_pre_done - t_pre, 1)      # rank 0: CPU baseline + oracle reference, before HIP / the process group
    else:
        out = None
    if world > 1 and args.gather == "dist" and backend == "nccl" and not one_gpu and extras_on and not host and eng is not None:
        # ---- c_abi_gather: the same steps delivered through the library's own RCCL exchange (the binder-without-torch path), every rank.
        #      Under a watchdog: a collective that never completes cannot be cancelled, and the headline line must survive it.
        def lost():
            if rank == 0:
                print(json.dumps(dict(out, c_abi_gather={"error": "did not complete within 120 s; the process was ended by the watchdog"})))
        try:
            rec = with_watchdog(120.0, lost, lambda: c_abi_gather_pass(torch, dist, eng, pool, scores, dev, world, rank,
                                                                      min(args.steps, 20), min(args.warmup, 5)))
        except Exception as e:
            rec = {"error": repr(e)[:400]}
        if rank == 0:
            out["c_abi_gather"] = rec
        if "error" in rec:                                  # a rank that failed alone leaves its peers in a collective: do not join them
            if rank == 0:
                print(json.dumps(out))
            sys.stdout.flush()
            os._exit(0)
    if rank == 0:
        print(json.dumps(out))
    if args.gather == "c_abi":
        gatherer.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
