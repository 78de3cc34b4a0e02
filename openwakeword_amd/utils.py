"""
Bulk feature extraction on the device: the `openwakeword.utils` functions that sit on `AudioFeatures.embed_clips`
(SURVEY.md section 8f rank 1).  `compute_features_from_generator` is the training pipeline's feature writer
(/root/reference/openwakeword/utils.py:542-601): clips from a generator -> embeddings -> one `.npy` file of shape
(N, n_windows, 96) float32 written through a memory map, trimmed to the rows actually produced
(/root/reference/openwakeword/data.py:856-892).
"""
from __future__ import annotations

import os
from typing import Iterator, Optional

import numpy as np
from numpy.lib.format import open_memmap

from .model import AudioFeatures  # noqa: F401  (re-export: the reference exposes it from this module)
from .engine import EMB_DIM, StreamEngine


def trim_mmap(mmap_path: str, n_rows: Optional[int] = None) -> int:
    """Drop the unused rows at the end of a feature file (data.py:856-892: the rows after the last one that is not all
    zero, or everything after `n_rows` when the writer knows its count).  The file is rewritten through a second map in
    blocks, then renamed over the original.  Returns the number of rows kept."""
    src = np.load(mmap_path, mmap_mode="r")
    if n_rows is None:
        n_rows = src.shape[0]
        while n_rows > 0 and not src[n_rows - 1].any():
            n_rows -= 1
    n_rows = int(min(max(n_rows, 0), src.shape[0]))
    if n_rows == src.shape[0]:
        return n_rows
    tmp = mmap_path[:-4] + ".trim.npy" if mmap_path.endswith(".npy") else mmap_path + ".trim"
    dst = open_memmap(tmp, mode="w+", dtype=src.dtype, shape=(n_rows,) + src.shape[1:])
    for lo in range(0, n_rows, 1024):
        dst[lo:min(lo + 1024, n_rows)] = src[lo:min(lo + 1024, n_rows)]
    dst.flush()
    del dst, src
    os.replace(tmp, mmap_path)
    return n_rows


def _embedding_weights(weights) -> dict:
    """The embedding model's parameters: the caller's ({"embedding": ...} as for `Model`, or the path of an embedding_model.onnx),
    else the .onnx file where the reference keeps it, else (opt-in, weights="synthetic") random-init ones."""
    from . import weights as W
    from .model import FEATURE_MODELS
    if isinstance(weights, dict):
        return weights["embedding"] if "embedding" in weights else weights
    path = FEATURE_MODELS["embedding"]["model_path"]
    if isinstance(weights, str) and weights != "synthetic":
        if not os.path.exists(weights):
            raise ValueError(f"{weights} does not exist")
        path = weights
    if os.path.exists(path):
        from . import onnx_ingest
        return onnx_ingest.load_embedding(path)
    if weights == "synthetic":
        return W.synthetic_embedding(1234)
    raise ValueError(f"{path} does not exist; pass weights='synthetic' for random-init weights of the same architecture")


def compute_features_from_generator(generator: Iterator[np.ndarray], n_total: int, clip_duration: int, output_file: str,
                                    device: str = "gpu", ncpu: int = 1, engine: Optional[StreamEngine] = None,
                                    weights=None) -> int:
    """utils.py:542-601 with the embedding work on the MI355X.

    `generator` yields int16 arrays [batch, clip_duration]; the first batch fixes the batch size (ValueError when it
    exceeds `n_total`, utils.py:581-583); rows beyond `n_total` are dropped; the file is trimmed to the rows written.
    `device` / `ncpu` exist for signature compatibility (there is no CPU path here).  `engine`: an existing
    `StreamEngine` to run on; otherwise one is created with as many streams as the batch.  `weights`: None = the embedding model
    file where the reference keeps it; the path of an embedding_model.onnx; a weight dict as for `Model`; 'synthetic' opts into
    random-init weights when the file is absent.  Returns the rows written."""
    n_cols = AudioFeatures.get_embedding_shape(None, clip_duration / 16000)
    if n_cols[0] < 1:
        raise ValueError("clips are shorter than one 76-frame embedding window (12512 samples, 782 ms)")
    fp = open_memmap(output_file, mode="w+", dtype=np.float32, shape=(int(n_total), n_cols[0], n_cols[1]))
    own = None
    rows = 0
    try:
        first = True
        for audio in generator:
            audio = np.asarray(audio)
            if first:
                first = False
                if audio.shape[0] > n_total:
                    raise ValueError(f"The value of 'n_total' ({n_total}) is less than the batch size ({audio.shape[0]})."
                                     " Please increase 'n_total' to be >= batch size.")
                if engine is None:
                    own = engine = StreamEngine(max(int(audio.shape[0]), 1), {}, _embedding_weights(weights))
            if rows >= n_total:
                break
            if audio.dtype != np.int16 or audio.ndim != 2:
                raise ValueError("the generator must yield 2-D int16 arrays [batch, samples]")
            cap = engine.n_streams_padded
            for lo in range(0, audio.shape[0], cap):
                feats = engine.embed_clips(audio[lo:lo + cap])[: n_total - rows]
                fp[rows:rows + feats.shape[0]] = feats
                rows += feats.shape[0]
                if rows >= n_total:
                    break
            fp.flush()
    finally:
        del fp
        if own is not None:
            own.close()
        elif engine is not None:
            engine.reset()
    trim_mmap(output_file, rows)
    return rows


def bulk_predict(file_paths, wakeword_models, prediction_function: str = "predict_clip", ncpu: int = 1,
                 inference_framework: str = "hip", **kwargs) -> dict:
    """`openwakeword.utils.bulk_predict` (utils.py:466-536) with the GPU as the pool of workers.

    The reference forks `ncpu` processes, each streaming its share of the files through one `Model`; here every file is one
    stream of a `BatchedModel` and all files advance together, 80 ms per device step (equivalent to the reference with one
    fresh process per file: no state is carried from one clip to the next).  `predict_clip` keyword arguments (`padding`,
    `chunk_size` -- a multiple of 1280 --, `patience`, `threshold`, `debounce_time`) and `Model` keyword arguments
    (`weights`, `device`) are taken from **kwargs like the reference filters them by name.  Other prediction functions, or
    chunk sizes that are not whole 80 ms frames, run file by file through a single `Model`.
    Returns {file path: value of the prediction function}, for `predict_clip` a list of {label: score} per chunk."""
    import wave
    from .model import BatchedModel, Model
    if inference_framework != "hip":
        raise ValueError("openwakeword_amd only provides inference_framework='hip'")
    file_paths = list(file_paths)
    model_kw = {k: v for k, v in kwargs.items() if k in ("weights", "device", "class_mapping_dicts", "vad_threshold", "vad_session",
                                                         "custom_verifier_models", "custom_verifier_threshold",
                                                         "enable_speex_noise_suppression")}
    chunk = int(kwargs.get("chunk_size", 1280))
    batched_ok = prediction_function == "predict_clip" and chunk % 1280 == 0 and chunk > 0 and \
        not (set(model_kw) - {"weights", "device"})
    if not batched_ok:
        mdl = Model(wakeword_models=wakeword_models, **model_kw)
        try:
            fn = getattr(mdl, prediction_function)
            names = fn.__code__.co_varnames
            takes_kw = bool(fn.__code__.co_flags & 0x08)
            out = {}
            for f in file_paths:
                out[f] = fn(f, **{k: v for k, v in kwargs.items() if (k in names or takes_kw) and k not in model_kw})
                mdl.reset()
            return out
        finally:
            mdl.close()

    padding = int(kwargs.get("padding", 1))
    clips = []
    for f in file_paths:
        with wave.open(f, mode="rb") as w:
            data = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16)
        if padding:
            z = np.zeros(16000 * padding, dtype=np.int16)
            data = np.concatenate((z, data, z))
        clips.append(data)
    if not clips:
        return {}
    k = chunk // 1280
    n_calls = [len(range(0, c.shape[0] - chunk, chunk)) for c in clips]              # model.py:421-426
    S = len(clips)
    bm = BatchedModel(S, list(wakeword_models), weights=model_kw.get("weights"),
                      device=int(model_kw.get("device", 0)), max_chunks=k)
    try:
        seed_stream = AudioFeatures(bm.engine, 0)                                     # seeds a feature ring like a fresh Model
        init = seed_stream.get_features(bm.engine.feature_ring)[0]
        ring = np.zeros((bm.engine.feature_ring, EMB_DIM), np.float32)
        ring[ring.shape[0] - init.shape[0]:] = init
        bm.reset(None, ring)
        bm.set_postproc(kwargs.get("patience", {}), kwargs.get("threshold", {}), float(kwargs.get("debounce_time", 0.0)), chunk)
        results = [[] for _ in range(S)]
        pcm = np.zeros((S, chunk), np.int16)
        for t in range(max(n_calls)):
            pcm[:] = 0
            for s, c in enumerate(clips):
                if t < n_calls[s]:
                    pcm[s] = c[t * chunk:(t + 1) * chunk]
            scores = bm.predict_batch(pcm)
            for s in range(S):
                if t < n_calls[s]:
                    results[s].append({lab: scores[s, i] for i, lab in enumerate(bm.labels)})
        return {f: results[s] for s, f in enumerate(file_paths)}
    finally:
        bm.close()


def _dense_model(wakeword_models, n_streams: int, **kw):
    """(BatchedModel-like scorer, owned): `wakeword_models` is a list of model names / paths (a BatchedModel is built and owned), or an
    object that already scores densely (a BatchedModel, or anything with its `engine`, `labels`, `_keep` and `_model_T`)."""
    if hasattr(wakeword_models, "engine"):
        return wakeword_models, False
    from .model import BatchedModel
    return BatchedModel(max(int(n_streams), 1), list(wakeword_models), weights=kw.get("weights"), device=int(kw.get("device", 0))), True


def dense_chunks(n_rows: int, t_max: int, chunk_rows: int):
    """The chunks `score_feature_file` walks: (first window, one past the last window, first row, one past the last row) of each.
    Consecutive chunks overlap by t_max - 1 rows, so every window lies whole in exactly one of them."""
    n_rows, t_max, chunk_rows = int(n_rows), int(t_max), int(chunk_rows)
    if chunk_rows < t_max:
        raise ValueError(f"chunk_rows = {chunk_rows} holds no window (t_max = {t_max})")
    n_win = n_rows - t_max + 1
    step = chunk_rows - (t_max - 1)
    return [(lo, min(lo + step, n_win), lo, min(lo + step, n_win) + t_max - 1) for lo in range(0, max(n_win, 0), step)]


def score_feature_file(path_or_array, wakeword_models, chunk_rows: int = 1 << 18, **kw) -> dict:
    """The scan of train.py:874-879 on the device: every T-row window (stride 1) of precomputed features `[N, 96]` -- a `.npy` path, read
    through a memmap, or an array -- through the models -> {label: [n_win] raw scores}, n_win = N - t_max + 1.  Window w ends at row
    w + t_max - 1 and each model reads its own last T rows; train.py:875's `range(0, N - T, 1)` drops the last window, so `[:-1]` of a
    model's scores is the reference's set.  The array is scored `chunk_rows` rows at a time, chunks overlapping by t_max - 1 rows:
    a window's scores depend on its rows alone, so the result does not depend on `chunk_rows`.
    `wakeword_models`: model names / paths (keyword arguments `weights`, `device` as for `Model`), or a `BatchedModel`."""
    feats = np.load(path_or_array, mmap_mode="r") if isinstance(path_or_array, (str, os.PathLike)) else np.asarray(path_or_array)
    if feats.ndim != 2 or feats.shape[1] != EMB_DIM:
        raise ValueError(f"features must be [N, 96], got {feats.shape}")
    bm, own = _dense_model(wakeword_models, 1, **kw)
    try:
        n_win, t_max = bm.engine.score_shape(feats.shape[0])
        raw = np.empty((n_win, bm.engine.n_labels), dtype=np.float32)
        for w0, w1, r0, r1 in dense_chunks(feats.shape[0], t_max, chunk_rows):
            raw[w0:w1] = bm.engine.score_features(np.ascontiguousarray(feats[r0:r1], dtype=np.float32)[None])[0]
        return {lab: raw[:, c] for lab, c in zip(bm.labels, bm._keep)}
    finally:
        if own:
            bm.close()


def mine_windows(clips, wakeword_models, threshold: float = 0.5, **kw) -> dict:
    """The feature windows of equally long clips `int16 [B, n]` that score at least `threshold` -> {label: [N, T, 96]}, the shape
    `Model._get_positive_prediction_frames(return_type="features")` returns (model.py:428-479; examples/mine_false_positives.py).
    Scores come from `score_clips`; the windows are cut on the host from the embeddings that call returns: window w of a model with
    window length T is rows [w + t_max - T, w + t_max) of its clip.  These are embed_clips-path scores -- one mel clamp floor per
    clip, no seeded feature ring -- not the streaming path's, so a clip's first t_max - 1 positions (which the reference scores on a
    ring still holding its seed) are not scored.  Multiclass models: a window is kept under every class label that reaches the threshold."""
    clips = np.ascontiguousarray(np.atleast_2d(clips))
    bm, own = _dense_model(wakeword_models, min(clips.shape[0], 64), **kw)
    try:
        scores, emb = bm.score_clips(clips, return_features=True)
        t_max = max(bm._model_T.values())
        out = {}
        for lab, c in zip(bm.labels, bm._keep):
            T = bm._model_T[bm._parent[c]]
            b, w = np.nonzero(scores[lab] >= threshold)
            idx = (w + (t_max - T))[:, None] + np.arange(T)[None, :]
            out[lab] = emb[b[:, None], idx] if b.size else np.zeros((0, T, EMB_DIM), dtype=np.float32)
        return out
    finally:
        if own:
            bm.close()


def mine_clip_hits(clips, wakeword_models, threshold: float = 0.5, cap: int = 4096, **kw) -> dict:
    """`mine_windows` with the search on the device: the feature windows of equally long clips `int16 [B, n]` that score at least
    `threshold` -> {label: [N, T, 96]}, at most `cap` per label (the first in (clip, window) order).  Neither the score matrix nor the
    embeddings come to the host: `BatchedModel.score_clip_hits` returns the hits and their windows alone.  Where nothing overflows the
    result is bit for bit `mine_windows`'."""
    clips = np.ascontiguousarray(np.atleast_2d(clips))
    bm, own = _dense_model(wakeword_models, min(clips.shape[0], 64), **kw)
    try:
        return {lab: col["windows"] for lab, col in bm.score_clip_hits(clips, threshold, cap).items()}
    finally:
        if own:
            bm.close()


def mine_feature_file(path_or_array, model, threshold=0.5, ids=None, cap: int = 4096, chunk_rows: int = 1 << 18) -> dict:
    """The chunked scan of `score_feature_file` / `validate_bank` that returns hits instead of scores or counts: every T-row window
    (stride 1) of precomputed features `[N, 96]` -- a `.npy` path, read through a memmap, or an array -- through the fixed models of
    `model` (a `BatchedModel`; `threshold` a number or {label: value}) or, with `ids`, through its bank heads (`threshold` a number or
    one per id) -> {label or id: {"window", "score", "windows", "n_total"}}: the windows (counted over the whole array) that score at
    least the threshold, in ascending order and at most `cap` of them, their scores, their own [T, 96] feature rows, and the number
    of hits without the cap.  Chunks overlap by t_max - 1 rows and a window's score depends on its rows alone, so the result does not
    depend on `chunk_rows`."""
    feats = np.load(path_or_array, mmap_mode="r") if isinstance(path_or_array, (str, os.PathLike)) else np.asarray(path_or_array)
    if feats.ndim != 2 or feats.shape[1] != EMB_DIM:
        raise ValueError(f"features must be [N, 96], got {feats.shape}")
    if ids is None:
        _, t_max = model.engine.score_shape(feats.shape[0])
        keys = list(model.labels)
    else:
        ids = [int(i) for i in ids]
        _, t_max = model.bank_score_shape(ids, feats.shape[0])
        keys = ids
        thr = None if threshold is None else np.broadcast_to(np.asarray(threshold, dtype=np.float32), (len(ids),))
    acc = [None] * len(keys)
    for w0, _, r0, r1 in dense_chunks(feats.shape[0], t_max, chunk_rows):
        chunk = np.ascontiguousarray(feats[r0:r1], dtype=np.float32)[None]
        if ids is None:
            got = model.score_hits(chunk, threshold, cap)
            cols = [got[lab] for lab in keys]
        else:
            cols = model.bank_score_hits(chunk, ids, thr, cap)
        for k, col in enumerate(cols):
            col = {"window": col["window"].astype(np.int64) + w0, "score": col["score"], "windows": col["windows"], "n_total": col["n_total"]}
            if acc[k] is None:
                acc[k] = col
                continue
            room = max(int(cap) - acc[k]["window"].size, 0)
            for f in ("window", "score", "windows"):
                acc[k][f] = np.concatenate([acc[k][f], col[f][:room]], axis=0)
            acc[k]["n_total"] += col["n_total"]
    return dict(zip(keys, acc)) if ids is None else {i: acc[k] for k, i in enumerate(ids)}


def validate_bank(path_or_array, model, ids, thresholds=None, chunk_rows: int = 1 << 18, hours: float = None) -> dict:
    """The scan of train.py:225-258 (`_select_best_model`) for bank heads: every T-row window (stride 1) of precomputed negative
    features `[N, 96]` -- a `.npy` path, read through a memmap, or an array -- through the bank heads `ids` of `model` (a `BatchedModel`
    or `StreamEngine` with a head bank), counted on the device -> {id: {"n_false_positives": windows with score >= its threshold
    (`thresholds` None = 0.5, train.py:100), "false_positives_per_hour", "max_score", "argmax_window": the first window that attains
    it}}.  Window w ends at row w + t_max - 1, t_max the longest window of the listed heads, and each head reads its own last T rows.
    The array is scored `chunk_rows` rows at a time, chunks overlapping by t_max - 1 rows: counts add, and of two chunks with the
    same maximum the earlier one keeps the argmax, so the result does not depend on `chunk_rows`.  The hours are n_win * 0.08 / 3600
    unless `hours` is given (train.py:245 divides by a caller-given `val_set_hrs`).  train.py:875's `range(0, N - T, 1)` drops the
    last window; this scan does not, so a hit on the very last window is counted here and not there."""
    feats = np.load(path_or_array, mmap_mode="r") if isinstance(path_or_array, (str, os.PathLike)) else np.asarray(path_or_array)
    if feats.ndim != 2 or feats.shape[1] != EMB_DIM:
        raise ValueError(f"features must be [N, 96], got {feats.shape}")
    ids = [int(i) for i in ids]
    n_win, t_max = model.bank_score_shape(ids, feats.shape[0])
    count = np.zeros(len(ids), dtype=np.int64)
    best = np.full(len(ids), -np.inf, dtype=np.float32)
    where = np.zeros(len(ids), dtype=np.int64)
    for w0, _, r0, r1 in dense_chunks(feats.shape[0], t_max, chunk_rows):
        st = model.bank_score_stats(np.ascontiguousarray(feats[r0:r1], dtype=np.float32)[None], ids, thresholds)
        count += st["count"][0]
        better = st["max"][0] > best                    # (strictly: a tie stays with the earlier chunk)
        best = np.where(better, st["max"][0], best)
        where = np.where(better, st["argmax"][0].astype(np.int64) + w0, where)
    hrs = n_win * 0.08 / 3600.0 if hours is None else float(hours)
    return {i: {"n_false_positives": int(count[k]), "false_positives_per_hour": float(count[k] / hrs), "max_score": float(best[k]),
                "argmax_window": int(where[k])} for k, i in enumerate(ids)}
