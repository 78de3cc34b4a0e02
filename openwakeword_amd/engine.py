"""
StreamEngine: S concurrent audio streams advanced one 80 ms frame per call on one MI355X.

This is the batched form of the reference's per-object hot loop
(`openwakeword.Model.predict`, /root/reference/openwakeword/model.py:232-386, which drives
`utils.AudioFeatures.__call__`, utils.py:409-463): the reference keeps one Python object per stream and
calls onnxruntime 2+H times per frame; here every stream's state lives in HBM and one `step()` runs the
mel / embedding / head / post-processing kernels of libowwhip.so over all of them.

Thin by design: blob packing + ctypes calls.  All arithmetic happens in the HIP library.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, weights as W

CHUNK = 1280
EMB_DIM = 96
_KIND = {"binary": 0, "gated": 1, "multiclass": 2, "rnn": 3}
# rows x mel-width x channels that each CNN layer produces per 80 ms step (incremental form)
LAYER_NEW_SHAPES = ([(8, 32, 24)] * 3 + [(4, 16, 48)] * 4 + [(4, 8, 72)] * 4 + [(2, 4, 96)] * 4 +
                    [(2, 2, 96)] * 4 + [(1, 1, 96)])
# oww_event of include/owwhip.h (32 bytes): what events() returns
EVENT_DTYPE = np.dtype([("stream", np.int32), ("column", np.int32), ("bank_id", np.int32), ("score", np.float32),
                        ("frame", np.uint32), ("feature_index", np.int32), ("reserved", np.int32, (2,))])
EVENT_CAPACITY_MAX = 1 << 20
# oww_dense_hit of include/owwhip.h (16 bytes): one record of a dense hit list
DENSE_HIT = np.dtype([("seq", np.int32), ("window", np.int32), ("score", np.float32), ("reserved", np.int32)])
DENSE_HIT_CAP_MAX = 1 << 20
AUDIO_RING_MAX = 1024    # oww_audio_configure: ring_chunks 1 .. 1024
KERNEL_CLASSES = ["mel", "stageA", "stageB", "stageC", "stageD", "stageE", "heads", "postproc", "vad_front", "vad_lstm"]


def pack_mel_blob() -> np.ndarray:
    start, taps, lo, hi = W.mel_sparse_taps()
    assert lo == 2 and hi == 121, "the mel kernel keeps FFT bins 2..121 only"
    return np.concatenate([W.hann_window().view(np.uint8), start.astype(np.int32).view(np.uint8),
                           taps.astype(np.float32).ravel().view(np.uint8)])


def pack_embedding_blob(emb: dict) -> np.ndarray:
    parts = []
    for li, w in enumerate(emb["conv"]):
        kh, kw, ci, co, _ = W.CNN_TOPOLOGY[li]
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (kh, kw, ci, co):
            raise ValueError(f"conv {li}: expected HWIO {(kh, kw, ci, co)}, got {w.shape}")
        parts.append(w.ravel())
        if li < len(emb["conv"]) - 1:
            scale, shift = W.bn_scale_shift(emb["bn"][li])
            parts += [scale, shift]
    return np.concatenate(parts).astype(np.float32)


def pack_head_blob(head: dict) -> np.ndarray:
    T, H, O = int(head["T"]), int(head["hidden"]), int(head["n_out"])
    if head["kind"] == "rnn":
        # train.py:85-98: hdr = {3, T, 64, n_out, 0, 0, 0, 0}; per layer, per direction: w [in + 64][256] (rows x ; h, columns i | f | g | o),
        # b [256]; then w_out [128][n_out], b_out [n_out]
        if H != W.RNN_HID or len(head["lstm"]) != 2 or any(len(layer) != 2 for layer in head["lstm"]):
            raise ValueError("an rnn head is a 2-layer bidirectional LSTM(64) (train.py:88)")
        parts = [np.array([3, T, H, O, 0, 0, 0, 0], dtype=np.int32).view(np.float32)]
        for li, layer in enumerate(head["lstm"]):
            n_in = EMB_DIM if li == 0 else 2 * H
            for w, b in layer:
                if w.shape != (n_in + H, 4 * H) or b.shape != (4 * H,):
                    raise ValueError("rnn head weight shapes do not match train.py:85-98")
                parts += [w.ravel(), b]
        if head["w_out"].shape != (2 * H, O) or head["b_out"].shape != (O,):
            raise ValueError("rnn head output layer shape")
        parts += [head["w_out"].ravel(), head["b_out"]]
        return np.concatenate([np.ascontiguousarray(p, dtype=np.float32).ravel() for p in parts])
    has_ln = head["net"].get("ln1") is not None
    n_blocks = len(W.net_blocks(head["net"]))             # train.py:73; hdr[5] counts the blocks beyond the released models' one
    hdr = np.array([_KIND[head["kind"]], T, H, O, int(has_ln), n_blocks - 1, 0, 0], dtype=np.int32)
    parts = [hdr.view(np.float32)]
    nets = [head["net"]] + ([head["net2"]] if head["kind"] == "gated" else [])
    for net in nets:
        blocks = W.net_blocks(net)
        if net["w1"].shape != (T * EMB_DIM, H) or net["w3"].shape != (H, O) or len(blocks) != n_blocks or \
                any(w.shape != (H, H) or b.shape != (H,) or (ln is not None) != has_ln for w, b, ln in blocks):
            raise ValueError("head weight shapes do not match its header")
        parts += [net["w1"].ravel(), net["b1"]]
        if has_ln:
            parts += list(net["ln1"])
        for w, b, ln in blocks:
            parts += [w.ravel(), b]
            if has_ln:
                parts += list(ln)
        parts += [net["w3"].ravel(), net["b3"]]
    return np.concatenate([np.ascontiguousarray(p, dtype=np.float32).ravel() for p in parts])


def pack_vad_blob(vad: dict) -> np.ndarray:
    """Blob of oww_load_vad for the voice-activity stand-in network (weights.synthetic_vad layout)."""
    hdr = np.array([1, W.VAD_N_FFT, W.VAD_HOP, W.VAD_BINS, W.VAD_HID, 0, 0, 0], dtype=np.int32)
    parts = [hdr.view(np.float32), np.array([W.VAD_MAG_GAIN], np.float32), W.vad_hann()]
    for (w, b), (cin, cout, _s) in zip(vad["enc"], W.VAD_ENC):
        if w.shape != (3, cin, cout) or b.shape != (cout,):
            raise ValueError(f"VAD encoder layer: expected w {(3, cin, cout)}, b {(cout,)}, got {w.shape}, {b.shape}")
        parts += [w.ravel(), b]
    for w, b in vad["lstm"]:
        if w.shape != (2 * W.VAD_HID, 4 * W.VAD_HID) or b.shape != (4 * W.VAD_HID,):
            raise ValueError("VAD LSTM layer: expected w [128, 256] (rows x ; h, columns i | f | g | o), b [256]")
        parts += [w.ravel(), b]
    wd, bd = vad["dec"]
    parts += [np.asarray(wd, np.float32).ravel(), np.array([bd], np.float32)]
    return np.concatenate([np.ascontiguousarray(p, dtype=np.float32).ravel() for p in parts])


def events_from_scores(scores, bank_scores=None, bank_sub=None, thresholds=0.5, bank_thr=0.5, participating=None):
    """The definition of a call's detection events (include/owwhip.h: oww_get_events), restated on host arrays: for users and tests
    without a GPU, and the reference the device path is held to.

    scores [S, n_labels] and bank_scores [S, K] are the call's post-processed scores (either may be None), bank_sub [S, K] the bank id
    subscribed to each slot (< 0 = empty), thresholds one value or [n_labels] (NaN = the column never reports), bank_thr the bank
    slots' threshold, participating [S] which streams took part in the call (None = all).  A pair is a hit when its stream took part,
    the pair exists and score >= threshold.  Returns [(stream, column, bank_id, score)] in the library's order: ascending stream, then
    the fixed columns ascending, then the slots ascending; a fixed hit carries (column, -1), a bank hit (~slot, bank id)."""
    sc = None if scores is None else np.asarray(scores, dtype=np.float32)
    bs = None if bank_scores is None else np.asarray(bank_scores, dtype=np.float32)
    if sc is None and bs is None:
        return []
    if sc is not None and sc.ndim != 2 or bs is not None and bs.ndim != 2:
        raise ValueError("scores and bank_scores are 2-D [streams, columns] arrays")
    S = (sc if sc is not None else bs).shape[0]
    NL = 0 if sc is None else sc.shape[1]
    K = 0 if bs is None else bs.shape[1]
    if sc is not None and bs is not None and bs.shape[0] != S:
        raise ValueError("scores and bank_scores must cover the same streams")
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (NL,))
    sub = None
    if K:
        if bank_sub is None:
            raise ValueError("bank_scores need bank_sub, the bank id subscribed to every slot")
        sub = np.asarray(bank_sub)
        if sub.shape != (S, K):
            raise ValueError(f"bank_sub must be [{S}, {K}], got {sub.shape}")
    on = np.ones(S, dtype=bool) if participating is None else np.asarray(participating) != 0
    if on.shape != (S,):
        raise ValueError(f"participating must be [{S}], got {on.shape}")
    bank_thr = np.float32(bank_thr)
    out = []
    for s in np.flatnonzero(on):
        for c in range(NL):
            if sc[s, c] >= thr[c]:                    # (False for a NaN threshold)
                out.append((int(s), c, -1, np.float32(sc[s, c])))
        for k in range(K):
            if sub[s, k] >= 0 and bs[s, k] >= bank_thr:
                out.append((int(s), ~k, int(sub[s, k]), np.float32(bs[s, k])))
    return out


class audio_ring_model:
    """The definition of the per-stream audio rings (include/owwhip.h: oww_audio_configure / oww_get_audio / oww_get_event_audio),
    restated on host arrays: for users and tests without a GPU, and the reference the device path is held to -- never used by the
    product path.  Per stream the last ring_chunks chunks of 1280 samples and a uint32 counter of the chunks received since its reset."""

    def __init__(self, n_streams: int, ring_chunks: int):
        self.n_streams, self.ring_chunks = int(n_streams), int(ring_chunks)
        self.buf = np.zeros((self.n_streams, self.ring_chunks * CHUNK), dtype=np.int16)      # oldest sample first
        self.counts = np.zeros(self.n_streams, dtype=np.uint32)

    def append(self, pcm, participating=None) -> None:
        """One call: pcm int16 [S, k * 1280]; participating [S] (None = every stream).  Streams that sit out keep every bit."""
        pcm = np.asarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 2 or pcm.shape[0] != self.n_streams or pcm.shape[1] == 0 or pcm.shape[1] % CHUNK:
            raise ValueError(f"pcm must be int16 [{self.n_streams}, 1280*k], got {pcm.dtype} {pcm.shape}")
        on = np.ones(self.n_streams, dtype=bool) if participating is None else np.asarray(participating) != 0
        joined = np.concatenate([self.buf[on], pcm[on]], axis=1)
        self.buf[on] = joined[:, -self.ring_chunks * CHUNK:]                     # of a call longer than the ring the last ring_chunks
        self.counts[on] += np.uint32(pcm.shape[1] // CHUNK)

    def reset(self, stream_ids=None) -> None:
        ids = slice(None) if stream_ids is None else np.asarray(stream_ids, dtype=np.int64)
        self.buf[ids] = 0
        self.counts[ids] = 0

    def last(self, stream_ids, n_chunks: int) -> np.ndarray:
        """int16 [n, n_chunks * 1280]: the newest n_chunks chunks of the listed streams, oldest first; what a stream has not received
        since its reset reads as zero (the buffer starts, and resets to, zeros)."""
        if not 1 <= int(n_chunks) <= self.ring_chunks:
            raise ValueError(f"n_chunks must lie in 1 .. {self.ring_chunks}, got {n_chunks}")
        return self.buf[np.asarray(stream_ids, dtype=np.int64)][:, -int(n_chunks) * CHUNK:].copy()


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def C_void(address) -> C.c_void_p:
    """a device address (int, or anything with data_ptr(), e.g. a torch tensor) as a pointer argument"""
    return C.c_void_p(int(address.data_ptr()) if hasattr(address, "data_ptr") else int(address))


_CAL_CLIPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resources", "calibration_clips.npz")


def default_calibration_pcm() -> Optional[np.ndarray]:
    """Speech for the commit-time calibration / self-test of the fp16-split kernels (oww_set_calibration): int16 [12, 16 * 1280].
    The three 16 kHz clips are the reference's own test fixtures (/root/reference/tests/data/{alexa_test,hey_mycroft_test,hey_jane}.wav,
    2.4 s of speech in all; shipped as resources/calibration_clips.npz), each tiled to 16 frames as recorded, peak-normalised to full
    scale, and 20 dB down, plus one half-period-shifted copy of each: the loudness range a microphone front end delivers, with the
    spectral and temporal structure noise and square waves do not have.  None when the resource file is absent."""
    if not os.path.exists(_CAL_CLIPS):
        return None
    z = np.load(_CAL_CLIPS)
    n = 16 * CHUNK
    rows = []
    for k in sorted(z.files):
        x = z[k].astype(np.float64)
        full = x * (32767.0 / max(1.0, np.abs(x).max()))
        for y in (x, full, 0.1 * x, np.roll(full, len(x) // 2)):
            rows.append(np.clip(np.rint(np.resize(y, n)), -32768, 32767).astype(np.int16))
    return np.stack(rows)


def check_event_config(event_capacity, event_features, feature_ring: int) -> Tuple[int, int]:
    """The limits of oww_events_configure, checked before the library is touched -> (capacity, rows)."""
    for name, v in (("event_capacity", event_capacity), ("event_features", event_features)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    cap, rows = int(event_capacity), int(event_features)
    if cap < 0 or cap > EVENT_CAPACITY_MAX:
        raise ValueError(f"event_capacity must lie in 0 .. {EVENT_CAPACITY_MAX} (0 = no events), got {cap}")
    if rows < 0 or rows > int(feature_ring):
        raise ValueError(f"event_features must lie in 0 .. {int(feature_ring)} (the feature ring), got {rows}")
    if rows > 0 and cap == 0:
        raise ValueError("event_features needs event_capacity > 0")
    return cap, rows


def check_audio_config(audio_chunks, event_audio, event_capacity) -> Tuple[int, int]:
    """The limits of oww_audio_configure, checked before the library is touched -> (ring_chunks, event_chunks)."""
    for name, v in (("audio_chunks", audio_chunks), ("event_audio", event_audio)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    ring, ev = int(audio_chunks), int(event_audio)
    if ring < 0 or ring > AUDIO_RING_MAX:
        raise ValueError(f"audio_chunks must lie in 0 .. {AUDIO_RING_MAX} (0 = no audio), got {ring}")
    if ev < 0 or ev > ring:
        raise ValueError(f"event_audio must lie in 0 .. audio_chunks = {ring}, got {ev}")
    if ev > 0 and int(event_capacity) <= 0:
        raise ValueError("event_audio needs event_capacity > 0")
    return ring, ev


class StreamEngine:
    """One GPU, S streams.  `heads` maps model name -> head dict (see weights.synthetic_head).

    use_mfma selects the kernel family of the embedding CNN / heads (include/owwhip.h): 3 = register-resident kernels with
    every fp32 product evaluated as three f16 MFMAs (hi/lo operand split, fp32 accumulation; default, same tolerances as
    fp32), 1 = the same kernels on the exact-fp32 MFMA, 2 = LDS-tiled fp32 MFMA kernels, 0 = plain VALU."""

    def __init__(self, n_streams: int, heads: Dict[str, dict], embedding: Optional[dict] = None,
                 device: int = 0, max_chunks: int = 1, use_mfma: int = 3, debug_layers: bool = False,
                 feature_ring: int = 0, hip_stream: int = 0, vad: Optional[dict] = None, vad_threshold: float = 0.0,
                 calibration_pcm: Union[np.ndarray, str, None] = "default", bank_slots: int = 0, bank_capacity: int = 0,
                 verifier_capacity: int = 0, event_capacity: int = 0, event_features: int = 0, audio_chunks: int = 0,
                 event_audio: int = 0):
        """`vad`: weights of the on-device voice-activity stand-in network (weights.synthetic_vad layout); when given, every
        step also runs it on the frame's two 640-sample sub-frames and gates the scores with `vad_threshold` (model.py:366-381).
        `calibration_pcm` (use_mfma = 3): audio of the deployment's domain, int16 [n, k * 1280], that oww_commit adds to its built-in
        probes when it calibrates the activation scales and holds the fp16-split kernels to the exact-fp32 ones; "default" = speech
        (default_calibration_pcm), None = the synthetic probes only.
        `bank_slots` > 0 (use_mfma = 3): a head bank of `bank_capacity` heads, every stream subscribed to up to `bank_slots` of them
        (oww_bank_configure; bank_add / subscribe / bank_scores below).
        `verifier_capacity` > 0: a pool of that many per-stream custom verifiers (oww_verifier_configure; verifier_add /
        assign_verifiers below).
        `event_capacity` > 0: detections are reported as ordered device-side events, up to that many per call, each with a snapshot of
        the stream's last `event_features` feature rows (oww_events_configure; set_event_thresholds / events / event_features below).
        `audio_chunks` > 0: every stream's last `audio_chunks` chunks of 16 kHz audio stay on the device (the reference's
        raw_data_buffer: 125), and every event carries its stream's last `event_audio` chunks (oww_audio_configure; audio /
        event_audio below)."""
        self.event_capacity, self.event_rows = check_event_config(event_capacity, event_features,
                                                                  max([16] + [int(h["T"]) for h in heads.values()] + [int(feature_ring)]))
        self.audio_chunks, self.event_audio_chunks = check_audio_config(audio_chunks, event_audio, event_capacity)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self._inflight: List[np.ndarray] = []
        self.n_streams = int(n_streams)
        self.max_chunks = int(max_chunks)
        self.head_names = list(heads.keys())
        self.heads = heads
        self._embedding = embedding
        self._cfg = dict(device=int(device), use_mfma=int(use_mfma))
        cfg = _lib.Config(int(device), self.n_streams, self.max_chunks, int(feature_ring), int(use_mfma),
                          int(bool(debug_layers)), C.c_void_p(hip_stream) if hip_stream else None)
        _lib.check(self._lib.oww_create(C.byref(cfg), C.byref(self._h)))
        try:
            blob = pack_mel_blob()
            _lib.check(self._lib.oww_load_mel(self._h, _ptr(blob), blob.nbytes))
            blob = pack_embedding_blob(embedding if embedding is not None else W.synthetic_embedding())
            _lib.check(self._lib.oww_load_embedding(self._h, _ptr(blob), blob.nbytes))
            self.head_cols = {}
            col = 0
            for name, head in heads.items():
                blob = pack_head_blob(head)
                _lib.check(self._lib.oww_add_head(self._h, _ptr(blob), blob.nbytes))
                self.head_cols[name] = (col, col + int(head["n_out"]))
                col += int(head["n_out"])
            self.has_vad = vad is not None
            if vad is not None:
                blob = pack_vad_blob(vad)
                _lib.check(self._lib.oww_load_vad(self._h, _ptr(blob), blob.nbytes))
            if isinstance(calibration_pcm, str):
                calibration_pcm = default_calibration_pcm() if calibration_pcm == "default" else None
            if calibration_pcm is not None and int(use_mfma) == 3:
                cal = np.asarray(calibration_pcm)
                if cal.dtype.kind not in "iu":
                    # (float audio in [-1, 1] would be truncated to silence and the scale ladder calibrated on nothing)
                    raise ValueError(f"Input data must be 16-bit integers (i.e., 16-bit PCM audio). You provided {cal.dtype} data.")
                if cal.size and (int(cal.min()) < -32768 or int(cal.max()) > 32767):      # wider integer types: valid 16-bit PCM only
                    raise ValueError(f"calibration_pcm holds values outside the 16-bit PCM range ({int(cal.min())} .. {int(cal.max())})")
                cal = np.ascontiguousarray(cal, dtype=np.int16)
                if cal.ndim != 2 or cal.shape[1] < CHUNK:
                    raise ValueError("calibration_pcm must be int16 [n_streams, n_frames * 1280]")
                n_frames = cal.shape[1] // CHUNK
                cal = np.ascontiguousarray(cal[:, :n_frames * CHUNK])
                _lib.check(self._lib.oww_set_calibration(self._h, _ptr(cal), cal.shape[0], n_frames))
            self.bank_slots = int(bank_slots)
            if self.bank_slots > 0:
                _lib.check(self._lib.oww_bank_configure(self._h, self.bank_slots, int(bank_capacity) or 1024))
            self.verifier_capacity = int(verifier_capacity)
            if self.verifier_capacity > 0:
                _lib.check(self._lib.oww_verifier_configure(self._h, self.verifier_capacity))
            if self.event_capacity > 0:
                _lib.check(self._lib.oww_events_configure(self._h, self.event_capacity, self.event_rows))
            if self.audio_chunks > 0:
                _lib.check(self._lib.oww_audio_configure(self._h, self.audio_chunks, self.event_audio_chunks))
            _lib.check(self._lib.oww_commit(self._h))
            if vad_threshold:
                _lib.check(self._lib.oww_set_vad_threshold(self._h, float(vad_threshold)))
        except Exception:
            self.close()
            raise
        self.n_labels = self._lib.oww_n_labels(self._h)
        self.n_streams_padded = (self.n_streams + 31) // 32 * 32
        self.feature_ring = max([16] + [int(h["T"]) for h in heads.values()] + [int(feature_ring)])

    # ---- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.oww_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state
    def reset(self, stream_ids: Optional[Sequence[int]] = None, init_features: Optional[np.ndarray] = None):
        ids = None
        n = 0
        if stream_ids is not None:
            ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
            n = ids.size
        feat = None
        if init_features is not None:
            feat = np.ascontiguousarray(init_features, dtype=np.float32)
            if feat.shape != (self.feature_ring, EMB_DIM):
                raise ValueError(f"init_features must be [{self.feature_ring}, 96] (oldest row first), got {feat.shape}")
        _lib.check(self._lib.oww_reset(self._h, _ptr(ids), n, _ptr(feat)))

    def set_postproc(self, patience: Optional[Sequence[int]] = None, threshold: Optional[Sequence[float]] = None,
                     debounce_frames: int = 0):
        pat = None if patience is None else np.ascontiguousarray(patience, dtype=np.int32)
        thr = None if threshold is None else np.ascontiguousarray(threshold, dtype=np.float32)
        for a in (pat, thr):
            if a is not None and a.size != self.n_labels:
                raise ValueError(f"need one value per label ({self.n_labels})")
        _lib.check(self._lib.oww_set_postproc(self._h, _ptr(pat), _ptr(thr), int(debounce_frames)))

    # ---- hot loop
    def step(self, pcm: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """pcm int16 [S, 1280*k] (host) -> scores fp32 [S, n_labels] (host, blocking)."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16:
            raise ValueError(f"Input data must be 16-bit integers (i.e., 16-bit PCM audio). You provided {pcm.dtype} data.")
        if pcm.ndim != 2 or pcm.shape[0] != self.n_streams or pcm.shape[1] % CHUNK or pcm.shape[1] == 0:
            raise ValueError(f"pcm must be [n_streams={self.n_streams}, 1280*k], got {pcm.shape}")
        k = pcm.shape[1] // CHUNK
        if out is None:
            out = np.empty((self.n_streams, self.n_labels), dtype=np.float32)
        _lib.check(self._lib.oww_step(self._h, _ptr(pcm), 0, k, _ptr(out), 0))
        return out

    def step_masked(self, pcm: np.ndarray, stream_on: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """One 1280-sample step for the streams with stream_on != 0 only (oww_step_masked): the others keep every bit of their
        state and repeat their previous scores -- the batched form of a client that simply does not call predict() while it has
        no audio (examples/web/streaming_server.py:49-66)."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16:
            raise ValueError(f"Input data must be 16-bit integers (i.e., 16-bit PCM audio). You provided {pcm.dtype} data.")
        if pcm.shape != (self.n_streams, CHUNK):
            raise ValueError(f"pcm must be [n_streams={self.n_streams}, 1280], got {pcm.shape}")
        on = np.ascontiguousarray(np.asarray(stream_on) != 0, dtype=np.uint8)
        if on.shape != (self.n_streams,):
            raise ValueError(f"stream_on must be [n_streams={self.n_streams}], got {on.shape}")
        if out is None:
            out = np.empty((self.n_streams, self.n_labels), dtype=np.float32)
        _lib.check(self._lib.oww_step_masked(self._h, _ptr(pcm), 0, _ptr(on), 0, _ptr(out), 0))
        return out

    def step_masked_device(self, pcm_dev_ptr: int, stream_on: np.ndarray, scores_dev_ptr: int = 0) -> None:
        """oww_step_masked on device-resident PCM / scores with the participation mask on the host (asynchronous); with at most
        7/8 of the streams taking part only their groups are launched."""
        on = np.ascontiguousarray(stream_on, dtype=np.uint8)
        if on.shape != (self.n_streams,):
            raise ValueError(f"stream_on must be [{self.n_streams}]")
        _lib.check(self._lib.oww_step_masked(self._h, C.c_void_p(int(pcm_dev_ptr)), 1, _ptr(on), 0,
                                             C.c_void_p(int(scores_dev_ptr)) if scores_dev_ptr else None, 1))

    def resample(self, pcm: np.ndarray, sample_rate: int) -> np.ndarray:
        """int16 [S, n_in] at `sample_rate` Hz -> int16 [S, n_in * 16000 // sample_rate] at 16 kHz on the device (oww_resample with the
        filter bank of resample.design; stateless per call, like the per-message resampy call of examples/web/streaming_server.py:57-58)."""
        from . import resample as R
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 2 or pcm.shape[0] != self.n_streams:
            raise ValueError(f"pcm must be int16 [n_streams={self.n_streams}, n], got {pcm.dtype} {pcm.shape}")
        if int(sample_rate) == 16000:
            return pcm
        p, q, taps = R.design(int(sample_rate))
        n_out = (pcm.shape[1] * q) // p
        out = np.empty((self.n_streams, n_out), dtype=np.int16)
        _lib.check(self._lib.oww_resample(self._h, _ptr(pcm), 0, pcm.shape[1], p, q, _ptr(taps), taps.shape[1], _ptr(out), 0, n_out))
        return out

    # ---- stateful stream ingest (include/owwhip.h: oww_ingest_configure / oww_ingest / oww_step_ingest) ----
    def configure_ingest(self, sample_rate: int, encoding: str = "pcm16") -> None:
        """Per-stream decode ("pcm16", "ulaw", "alaw") and CONTINUOUS conversion of `sample_rate` Hz to 16 kHz on the device with the
        bank of resample.design; 16000 Hz = decode only.  Zeroes every stream's filter history; may be called again."""
        from . import resample as R
        if encoding not in R.ENCODINGS:
            raise ValueError(f"unknown encoding {encoding!r} (one of {sorted(R.ENCODINGS)})")
        if int(sample_rate) == 16000:
            p, q, taps, n_taps = 1, 1, None, 0
        else:
            p, q, taps = R.design(int(sample_rate))
            n_taps = taps.shape[1]
        _lib.check(self._lib.oww_ingest_configure(self._h, R.ENCODINGS[encoding], p, q, _ptr(taps), n_taps))
        self._ingest = (encoding, p, q, n_taps)
        self._ingest_classes = None

    def _ingest_mask(self, stream_on):                   # as the library takes it: contiguous uint8 [S] of 0 / 1, or None
        if stream_on is None:
            return None
        on = np.ascontiguousarray(np.asarray(stream_on) != 0, dtype=np.uint8)
        if on.shape != (self.n_streams,):
            raise ValueError(f"stream_on must be [n_streams={self.n_streams}], got {on.shape}")
        return on

    def _ingest_out(self, out, n_out):                   # the caller's 16 kHz buffer, checked, or a fresh one of zeros
        if out is None:
            return np.zeros((self.n_streams, n_out), dtype=np.int16)
        if out.dtype != np.int16 or out.shape != (self.n_streams, n_out) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous int16 [{self.n_streams}, {n_out}] array")
        return out

    def _ingest_args(self, data: np.ndarray, stream_on):
        if getattr(self, "_ingest", None) is None:
            raise _lib.OwwError("ingest is not configured: call configure_ingest(sample_rate, encoding) first")
        encoding, p, q, _ = self._ingest
        data = np.ascontiguousarray(data)
        want = np.int16 if encoding == "pcm16" else np.uint8
        if data.dtype != want or data.ndim != 2 or data.shape[0] != self.n_streams or data.shape[1] == 0:
            raise ValueError(f"{encoding} data must be {np.dtype(want).name} [n_streams={self.n_streams}, n], got {data.dtype} {data.shape}")
        if (data.shape[1] * q) % p:
            raise ValueError(f"a message must hold a whole number of output samples: {data.shape[1]} * {q} is no multiple of {p}")
        return data, self._ingest_mask(stream_on), (data.shape[1] * q) // p

    def ingest(self, data: np.ndarray, stream_on: Optional[np.ndarray] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """One message per stream, [S, n_in] in the configured encoding -> 16 kHz int16 [S, n_in * q / p], continuous with the stream's
        earlier messages (host, blocking).  A stream with stream_on[s] == 0 is not read, keeps its history and its row of `out` is not
        written (a fresh `out` holds zeros there)."""
        data, on, n_out = self._ingest_args(data, stream_on)
        out = self._ingest_out(out, n_out)
        _lib.check(self._lib.oww_ingest(self._h, _ptr(data), 0, data.shape[1], _ptr(on), 0, _ptr(out), 0))
        return out

    def step_ingest(self, data: np.ndarray, stream_on: Optional[np.ndarray] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """ingest + step without the 16 kHz audio leaving the device (oww_step_ingest): scores fp32 [S, n_labels].  The message must
        convert to 1280 * k samples (k = 1 with `stream_on`, which is step_masked's mask)."""
        data, on, n_out = self._ingest_args(data, stream_on)
        if out is None:
            out = np.empty((self.n_streams, self.n_labels), dtype=np.float32)
        _lib.check(self._lib.oww_step_ingest(self._h, _ptr(data), 0, data.shape[1], _ptr(on), 0, _ptr(out), 0))
        return out

    def ingest_dev_ptr(self) -> int:
        """Device address of the 16 kHz staging buffer the last ingest without `out` wrote (16-byte aligned; 0 before configure_ingest)."""
        return int(self._lib.oww_ingest_dev(self._h) or 0)

    # ---- ingest classes: every stream its own rate and encoding (include/owwhip.h: oww_ingest_configure_classes ... ) ----
    def configure_ingest_classes(self, formats) -> None:
        """`formats`: a list of (sample_rate, encoding), at most 16.  Every stream starts in class 0 with a zero history; replaces any
        earlier ingest configuration.  Banks come from resample.design; 16000 Hz means decode only."""
        from . import resample as R
        formats = [(int(r), str(e)) for r, e in formats]
        arr = (_lib.IngestClass * max(len(formats), 1))()
        keep = []
        for i, (rate, enc) in enumerate(formats):
            p, q, taps, n_taps = R.class_params(rate, enc)
            keep.append(taps)
            arr[i] = _lib.IngestClass(R.ENCODINGS[enc], p, q, n_taps, None if taps is None else taps.ctypes.data)
        _lib.check(self._lib.oww_ingest_configure_classes(self._h, len(formats), arr))
        self._ingest = None
        self._ingest_classes = formats

    def _classes(self):
        if getattr(self, "_ingest_classes", None) is None:
            raise _lib.OwwError("ingest classes are not configured: call configure_ingest_classes(formats) first")
        return self._ingest_classes

    def assign_ingest(self, stream_ids, class_ids) -> None:
        """Streams `stream_ids` take the classes `class_ids` and start from silence (oww_ingest_assign)."""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).reshape(-1)
        cls = np.asarray(class_ids).reshape(-1)
        if cls.size != ids.size or (cls.size and (cls.min() < 0 or cls.max() > 255)):
            raise ValueError(f"class_ids must be {ids.size} values in [0, 255]")
        cls = np.ascontiguousarray(cls, dtype=np.uint8)
        _lib.check(self._lib.oww_ingest_assign(self._h, _ptr(ids), ids.size, _ptr(cls)))

    def ingest_row_bytes(self, n_out: int = CHUNK) -> int:
        """Row pitch of `rows` for messages of n_out outputs: the widest configured class's message, rounded up to 16 bytes."""
        from . import resample as R
        return R.class_row_bytes(self._classes(), n_out)

    def pack_ingest_rows(self, per_stream_arrays, class_ids, n_out: int = CHUNK, out: Optional[np.ndarray] = None) -> np.ndarray:
        """uint8 [S, row_bytes] from one int16 / uint8 array per stream (None: the stream sits out); lengths and dtypes are checked
        against each stream's class (resample.pack_ingest_rows with this engine's classes)."""
        from . import resample as R
        if len(per_stream_arrays) != self.n_streams:
            raise ValueError(f"{len(per_stream_arrays)} arrays for n_streams={self.n_streams}")
        return R.pack_ingest_rows(per_stream_arrays, class_ids, self._classes(), n_out, out)

    def _mixed_args(self, rows, n_out, stream_on):
        self._classes()
        if not isinstance(rows, np.ndarray) or rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[0] != self.n_streams \
                or not rows.flags["C_CONTIGUOUS"]:
            raise ValueError(f"rows must be a C-contiguous uint8 [n_streams={self.n_streams}, row_bytes] array")
        return rows, self._ingest_mask(stream_on), int(n_out)

    def ingest_mixed(self, rows: np.ndarray, n_out: int = CHUNK, stream_on: Optional[np.ndarray] = None,
                     out: Optional[np.ndarray] = None) -> np.ndarray:
        """One message per stream in the stream's own class, rows uint8 [S, row_bytes] (resample.pack_ingest_rows) -> 16 kHz int16
        [S, n_out], continuous with each stream's earlier messages.  Masked streams as in ingest()."""
        rows, on, n_out = self._mixed_args(rows, n_out, stream_on)
        out = self._ingest_out(out, n_out)
        _lib.check(self._lib.oww_ingest_mixed(self._h, _ptr(rows), 0, rows.shape[1], n_out, _ptr(on), 0, _ptr(out), 0))
        return out

    def step_ingest_mixed(self, rows: np.ndarray, n_out: int = CHUNK, stream_on: Optional[np.ndarray] = None,
                          out: Optional[np.ndarray] = None) -> np.ndarray:
        """ingest_mixed + step without the 16 kHz audio leaving the device (oww_step_ingest_mixed): scores fp32 [S, n_labels]."""
        rows, on, n_out = self._mixed_args(rows, n_out, stream_on)
        if out is None:
            out = np.empty((self.n_streams, self.n_labels), dtype=np.float32)
        _lib.check(self._lib.oww_step_ingest_mixed(self._h, _ptr(rows), 0, rows.shape[1], n_out, _ptr(on), 0, _ptr(out), 0))
        return out

    def submit_ingest_mixed(self, rows: np.ndarray, stream_on: Optional[np.ndarray] = None) -> None:
        """Pipelined step_ingest_mixed of one chunk (oww_submit_ingest_mixed): returns at once, collect() brings the scores.  `rows`
        must stay alive and unmodified until then (use `pinned_empty(shape, np.uint8)` for an asynchronous upload)."""
        rows, on, _ = self._mixed_args(rows, CHUNK, stream_on)
        _lib.check(self._lib.oww_submit_ingest_mixed(self._h, _ptr(rows), rows.shape[1], _ptr(on)))
        self._inflight.append(rows)

    def step_raw(self, pcm: np.ndarray) -> np.ndarray:
        """Like step(), but returns the head outputs before post-processing (model.py:313-317)."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16:
            raise ValueError(f"Input data must be 16-bit integers (i.e., 16-bit PCM audio). You provided {pcm.dtype} data.")
        if pcm.ndim != 2 or pcm.shape[0] != self.n_streams or pcm.shape[1] % CHUNK or pcm.shape[1] == 0:
            raise ValueError(f"pcm must be [n_streams={self.n_streams}, 1280*k], got {pcm.shape}")
        _lib.check(self._lib.oww_step(self._h, _ptr(pcm), 0, pcm.shape[1] // CHUNK, None, 0))
        out = np.empty((self.n_streams, self.n_labels), dtype=np.float32)
        _lib.check(self._lib.oww_get_raw(self._h, _ptr(out)))
        return out

    def step_device(self, pcm_dev_ptr: int, n_chunks: int = 1, scores_dev_ptr: int = 0):
        """Asynchronous step on device pointers (e.g. torch tensors' data_ptr())."""
        _lib.check(self._lib.oww_step(self._h, C.c_void_p(pcm_dev_ptr), 1, int(n_chunks),
                                      C.c_void_p(scores_dev_ptr) if scores_dev_ptr else None, 1))

    # ---- host-fed pipeline: upload of step t+1 overlaps the kernels of step t (oww_submit / oww_collect) ----
    def submit(self, pcm: np.ndarray, stream_on: Optional[np.ndarray] = None) -> None:
        """Enqueue one step on host PCM int16 [S, 1280*k] and return at once.  At most two steps in flight; the array
        must stay alive and unmodified until the matching collect() (use `pinned_empty` buffers for an asynchronous
        upload).  Same results as step(); with `stream_on` ([S], one chunk) as step_masked()."""
        if not isinstance(pcm, np.ndarray) or pcm.dtype != np.int16 or not pcm.flags["C_CONTIGUOUS"]:
            raise ValueError("submit expects a C-contiguous int16 ndarray")
        if pcm.ndim != 2 or pcm.shape[0] != self.n_streams or pcm.shape[1] % CHUNK or pcm.shape[1] == 0:
            raise ValueError(f"pcm must be [n_streams={self.n_streams}, 1280*k], got {pcm.shape}")
        if stream_on is None:
            _lib.check(self._lib.oww_submit(self._h, _ptr(pcm), pcm.shape[1] // CHUNK))
        else:
            on = np.ascontiguousarray(np.asarray(stream_on) != 0, dtype=np.uint8)
            if on.shape != (self.n_streams,) or pcm.shape[1] != CHUNK:
                raise ValueError(f"a masked submit takes pcm [n_streams, 1280] and stream_on [n_streams], got {pcm.shape}, {on.shape}")
            _lib.check(self._lib.oww_submit_masked(self._h, _ptr(pcm), _ptr(on)))
        self._inflight.append(pcm)                      # keeps the buffer alive until collected

    def collect(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Scores fp32 [S, n_labels] of the oldest submitted step (blocks until they have arrived)."""
        if out is None:
            out = np.empty((self.n_streams, self.n_labels), dtype=np.float32)
        _lib.check(self._lib.oww_collect(self._h, _ptr(out)))
        if self._inflight:
            self._inflight.pop(0)
        return out

    def pinned_empty(self, shape, dtype=np.int16) -> np.ndarray:
        """A page-locked host array (hipHostMalloc) for PCM / score buffers; freed when the array is collected."""
        import weakref
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        _lib.check(self._lib.oww_host_alloc(C.byref(p), max(nbytes, 1)))
        buf = (C.c_byte * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
        weakref.finalize(buf, self._lib.oww_host_free, C.c_void_p(p.value))
        return arr

    def calibration_info(self) -> Dict[str, object]:
        """What oww_commit measured on its probe set (fp16-split family): per-layer |activation| maxima, the power-of-two scale
        exponents (CNN layers and the heads' feature scale), the number of probe streams and the commit-time self-test errors."""
        absmax = np.zeros(20, np.float32)
        exps = np.zeros(21, np.int32)
        n = C.c_int32(0)
        st = np.zeros(3, np.float32)
        _lib.check(self._lib.oww_calibration_info(self._h, _ptr(absmax), _ptr(exps), C.byref(n), _ptr(st)))
        return {"absmax": absmax, "layer_exp": exps[:20].copy(), "feature_exp": int(exps[20]), "n_probe_streams": int(n.value),
                "selftest_embedding_err": float(st[0]), "selftest_embedding_max": float(st[1]), "selftest_score_err": float(st[2])}

    def self_test(self, n_frames: int = 24, pcm: Optional[np.ndarray] = None, tol: float = 1e-3) -> Dict[str, float]:
        """Deploy-time check of the default f16-split kernels against the exact-fp32 family on THIS engine's weights.

        The f16-split family carries activations as f16 hi/lo pairs; a network whose activations leave the f16 range
        (|x| > 65504) would not fail loudly -- max/ReLU stages swallow the resulting NaNs -- it would silently score
        differently.  This runs `n_frames` frames of 32 probe streams (silence, quiet and full-scale noise, full-scale
        square waves, or the rows of `pcm` [32, 1280*n]) through a scratch engine of this family and one with
        use_mfma=1 and compares raw scores and embeddings.  Returns the maxima; raises OwwError beyond `tol`
        (the north-star score tolerance).  Does not touch this engine's streams."""
        S = 32
        if pcm is None:
            r = np.random.default_rng(2024)
            pcm = np.zeros((S, CHUNK * n_frames), np.int16)
            for i in range(1, S):
                amp = (30, 300, 3000, 12000, 32767)[i % 5]
                if i % 3 == 0:
                    t = np.arange(CHUNK * n_frames)
                    pcm[i] = np.where((t // (8 << (i % 4))) % 2, amp, -amp)
                else:
                    pcm[i] = np.clip(np.round(r.normal(0.0, amp, CHUNK * n_frames)), -32768, 32767)
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        if pcm.shape[0] != S or pcm.shape[1] % CHUNK:
            raise ValueError("self_test expects pcm [32, 1280*n]")
        outs = []
        for fam in (self._cfg["use_mfma"], 1):
            eng = StreamEngine(S, self.heads, self._embedding, device=self._cfg["device"], use_mfma=fam,
                               feature_ring=self.feature_ring)
            try:
                raw = [eng.step_raw(pcm[:, CHUNK * t: CHUNK * (t + 1)]) for t in range(pcm.shape[1] // CHUNK)]
                feats = np.stack([eng.get_features(s, 16) for s in range(S)])
                outs.append((np.stack(raw), feats))
            finally:
                eng.close()
        res = {"max_abs_score_diff": float(np.max(np.abs(outs[0][0] - outs[1][0]))) if outs[0][0].size else 0.0,
               "max_abs_embedding_diff": float(np.max(np.abs(outs[0][1] - outs[1][1]))),
               "max_abs_embedding": float(np.max(np.abs(outs[1][1])))}
        bad = not np.isfinite(outs[0][1]).all() or res["max_abs_score_diff"] > tol or \
            res["max_abs_embedding_diff"] > tol * max(1.0, res["max_abs_embedding"])
        if bad:
            raise _lib.OwwError(f"kernel family {self._cfg['use_mfma']} disagrees with the exact-fp32 family on these weights "
                                f"({res}): create the engine with use_mfma=1")
        return res

    def set_verifier(self, label: int, w: Optional[np.ndarray], bias: float = 0.0, threshold: float = 0.1) -> None:
        """Custom verifier of score column `label` on the device: sigmoid(w . last-T-feature-rows + bias) replaces the head
        output wherever that is >= threshold (model.py:320-328).  w = None removes it."""
        if w is None:
            _lib.check(self._lib.oww_set_verifier(self._h, int(label), None, 0, 0.0, 0.0))
            return
        w = np.ascontiguousarray(w, dtype=np.float32).ravel()
        _lib.check(self._lib.oww_set_verifier(self._h, int(label), _ptr(w), int(w.size), float(bias), float(threshold)))

    # ---- per-stream custom verifiers (include/owwhip.h: oww_verifier_*) ----
    def verifier_add(self, w: np.ndarray, bias: float) -> int:
        """Folded verifier (w [T*96], bias) into the pool -> id (needs verifier_capacity > 0)."""
        w = np.ascontiguousarray(w, dtype=np.float32).ravel()
        rc = self._lib.oww_verifier_add(self._h, _ptr(w), int(w.size), float(bias))
        _lib.check(rc)
        return int(rc)

    def verifier_remove(self, verifier_id: int) -> None:
        _lib.check(self._lib.oww_verifier_remove(self._h, int(verifier_id)))

    def assign_verifiers(self, label: int, stream_ids, verifier_ids, thresholds, bank: bool = False) -> None:
        """Per-stream verifier ids (>= 0 pool, -1 default, -2 none) and thresholds for score column `label` (bank: bank slot)."""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).ravel()
        v = np.ascontiguousarray(verifier_ids, dtype=np.int32).ravel()
        t = np.ascontiguousarray(thresholds, dtype=np.float32).ravel()
        fn = self._lib.oww_bank_assign_verifiers if bank else self._lib.oww_assign_verifiers
        _lib.check(fn(self._h, int(label), _ptr(ids), ids.size, _ptr(v), _ptr(t)))

    def verifier_fit(self, windows, offsets, labels, T: int, C: float = 0.001, on_device: bool = False) -> List[dict]:
        """oww_verifier_fit: problem u = windows offsets[u] .. offsets[u+1]-1 of `windows` ([n, T, 96] fp32 on the host, or a device
        address of such a buffer with on_device) with `labels` [n] in {0, 1} -> one dict per problem (status, id, n_pos, n_neg,
        iterations, residual); an OK problem's verifier is live in the pool under its id."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        lab = np.ascontiguousarray(labels, dtype=np.uint8).ravel()
        U = off.size - 1
        if U < 0 or (U >= 0 and lab.size < int(off[-1])):
            raise ValueError(f"offsets [U+1] and {int(off[-1]) if off.size else 0} labels expected, got {off.size} offsets and {lab.size} labels")
        if on_device:
            wp = C_void(windows)
        else:
            w = np.ascontiguousarray(windows, dtype=np.float32)
            if w.size < int(off[-1]) * int(T) * 96:
                raise ValueError(f"{int(off[-1])} windows of {T} x 96 floats expected, got {w.size} floats")
            wp = _ptr(w)
        out = (_lib.FitResult * max(U, 1))()
        _lib.check(self._lib.oww_verifier_fit(self._h, wp, int(bool(on_device)), _ptr(off), _ptr(lab), U, int(T), float(C), out))
        return [dict(status=int(r.status), id=int(r.id), n_pos=int(r.n_pos), n_neg=int(r.n_neg), iterations=int(r.iterations),
                     residual=float(r.residual)) for r in out[:U]]

    def verifier_get(self, verifier_id: int, T: int) -> Tuple[np.ndarray, float]:
        """Pool verifier `verifier_id` (of T feature rows) read back: (w [T*96] fp32, bias)."""
        w = np.empty(int(T) * 96, dtype=np.float32)
        b = C.c_float(0.0)
        _lib.check(self._lib.oww_verifier_get(self._h, int(verifier_id), _ptr(w), int(w.size), C.byref(b)))
        return w, float(b.value)

    # ---- training bank heads (include/owwhip.h: oww_train_*) ----
    def train_param_count(self, T: int, hidden: int) -> int:
        return int(self._lib.oww_train_param_count(int(T), int(hidden)))

    def train_begin(self, params: np.ndarray, T: int, hidden: int) -> None:
        """oww_train_begin: params [U, oww_train_param_count(T, hidden)] fp32, the initial flat records."""
        p = np.ascontiguousarray(params, dtype=np.float32)
        n = self.train_param_count(T, hidden)
        if p.ndim != 2 or (n and p.shape[1] != n):
            raise ValueError(f"params must be [U, {n}] for T = {T}, hidden = {hidden}, got {p.shape}")
        _lib.check(self._lib.oww_train_begin(self._h, p.shape[0], int(T), int(hidden), _ptr(p)))
        self._train_U = int(p.shape[0])              # the session's problems: what train_steps sizes its tables and records by

    def train_set_pool(self, pool, n_windows: Optional[int] = None, on_device: bool = False) -> None:
        """oww_train_set_pool: `pool` [P, T, 96] fp32 on the host, or a device address of such a buffer of n_windows windows."""
        if on_device:
            _lib.check(self._lib.oww_train_set_pool(self._h, C_void(pool), 1, int(n_windows)))
            return
        w = np.ascontiguousarray(pool, dtype=np.float32)
        _lib.check(self._lib.oww_train_set_pool(self._h, _ptr(w), 0, int(w.shape[0]) if n_windows is None else int(n_windows)))

    def train_steps(self, n_problems: int, idx, y, lr, neg_weight, on_device: bool = False, shape=None) -> Tuple[np.ndarray, np.ndarray]:
        """oww_train_steps: idx / y [U, K, n] (or [K, n]: one table for all problems) on the host, or device addresses with
        on_device and shape = their shape; lr, neg_weight [K] -> (loss [U, K] fp32, NaN where no optimizer step was taken; m [U, K]).
        n_problems must be the open session's U: the library reads U tables and writes U x K records."""
        U = getattr(self, "_train_U", None)
        if U is None:
            raise ValueError("train_steps: no training session on this engine (train_begin first)")
        if int(n_problems) != U:
            raise ValueError(f"train_steps: n_problems = {n_problems}, the open session trains {U} problems")
        if on_device:
            shp = tuple(int(s) for s in shape)
            ip, yp = C_void(idx), C_void(y)
        else:
            i = np.ascontiguousarray(idx, dtype=np.int32)
            yy = np.ascontiguousarray(y, dtype=np.uint8)
            if i.shape != yy.shape:
                raise ValueError(f"idx {i.shape} and y {yy.shape} differ in shape")
            shp, ip, yp = i.shape, _ptr(i), _ptr(yy)
        if len(shp) not in (2, 3) or (len(shp) == 3 and shp[0] != int(n_problems)):
            raise ValueError(f"tables must be [K, n] or [{n_problems}, K, n], got {shp}")
        K, n = shp[-2], shp[-1]
        l = np.ascontiguousarray(lr, dtype=np.float64).ravel()
        w = np.ascontiguousarray(neg_weight, dtype=np.float32).ravel()
        if l.size != K or w.size != K:
            raise ValueError(f"lr and neg_weight must have one entry per step ({K}), got {l.size} and {w.size}")
        out = (_lib.TrainRecord * (int(n_problems) * max(K, 1)))()
        _lib.check(self._lib.oww_train_steps(self._h, K, n, ip, yp, int(len(shp) == 2), int(bool(on_device)), _ptr(l), _ptr(w), out))
        rec = np.frombuffer(out, dtype=np.dtype([("loss", np.float32), ("m", np.int32)])).reshape(int(n_problems), K)
        return rec["loss"].copy(), rec["m"].copy()

    def train_get(self, u: int, n_params: int) -> np.ndarray:
        p = np.empty(int(n_params), dtype=np.float32)
        _lib.check(self._lib.oww_train_get(self._h, int(u), _ptr(p), int(p.size)))
        return p

    def train_end(self) -> None:
        _lib.check(self._lib.oww_train_end(self._h))
        self._train_U = None
        self._train_C = 0

    # ---- validation, checkpoints and merge of a session's heads (include/owwhip.h: oww_train_new_sequence ..) ----
    def _train_open_U(self, what: str) -> int:
        U = getattr(self, "_train_U", None)
        if U is None:
            raise ValueError(f"{what}: no training session on this engine (train_begin first)")
        return U

    def train_new_sequence(self) -> None:
        _lib.check(self._lib.oww_train_new_sequence(self._h))

    def train_set_eval_pool(self, pool, n_windows: Optional[int] = None, on_device: bool = False) -> None:
        """oww_train_set_eval_pool: `pool` [P, T, 96] fp32 on the host, or a device address of such a buffer of n_windows windows."""
        if on_device:
            _lib.check(self._lib.oww_train_set_eval_pool(self._h, C_void(pool), 1, int(n_windows)))
            return
        w = np.ascontiguousarray(pool, dtype=np.float32)
        _lib.check(self._lib.oww_train_set_eval_pool(self._h, _ptr(w), 0, int(w.shape[0]) if n_windows is None else int(n_windows)))

    def train_eval(self, idx, y, source: int = -1, scores: bool = False, on_device: bool = False, shape=None):
        """oww_train_eval: idx / y [U, n] (or [n]: one table for all problems) on the host, or device addresses with on_device and
        shape = their shape -> (counts [U, 5] int32: n_pos, n_neg, pos_gt, neg_gt, neg_ge; scores [U, n] fp32 or None)."""
        U = self._train_open_U("train_eval")
        if on_device:
            shp = tuple(int(s) for s in shape)
            ip, yp = C_void(idx), C_void(y)
        else:
            i = np.ascontiguousarray(idx, dtype=np.int32)
            yy = np.ascontiguousarray(y, dtype=np.uint8)
            if i.shape != yy.shape:
                raise ValueError(f"idx {i.shape} and y {yy.shape} differ in shape")
            shp, ip, yp = i.shape, _ptr(i), _ptr(yy)
        if len(shp) not in (1, 2) or (len(shp) == 2 and shp[0] != U):
            raise ValueError(f"tables must be [n] or [{U}, n], got {shp}")
        n = shp[-1]
        counts = np.zeros((U, 5), dtype=np.int32)
        sc = np.empty((U, max(n, 1)), dtype=np.float32) if scores else None
        _lib.check(self._lib.oww_train_eval(self._h, int(source), n, ip, yp, int(len(shp) == 1), int(bool(on_device)),
                                            _ptr(sc) if scores else None, _ptr(counts)))
        return counts, sc

    def train_checkpoints(self, C_: int) -> None:
        _lib.check(self._lib.oww_train_checkpoints(self._h, int(C_)))
        self._train_C = int(C_)

    def train_snapshot(self, slots) -> None:
        """oww_train_snapshot: slots [U] int32, -1 = none."""
        U = self._train_open_U("train_snapshot")
        s = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        if s.size != U:
            raise ValueError(f"train_snapshot: {s.size} slot numbers for {U} problems")
        _lib.check(self._lib.oww_train_snapshot(self._h, _ptr(s)))

    def train_average(self, sel, dst: int) -> None:
        """oww_train_average: sel [U, C] (nonzero = selected), dst the slot that receives the result."""
        U = self._train_open_U("train_average")
        Cn = getattr(self, "_train_C", 0)
        s = np.ascontiguousarray(np.asarray(sel) != 0, dtype=np.uint8)
        if Cn and s.shape != (U, Cn):
            raise ValueError(f"train_average: sel must be [{U}, {Cn}], got {s.shape}")
        _lib.check(self._lib.oww_train_average(self._h, _ptr(s), int(dst)))

    def train_get_slot(self, u: int, slot: int, n_params: int) -> np.ndarray:
        p = np.empty(int(n_params), dtype=np.float32)
        _lib.check(self._lib.oww_train_get_slot(self._h, int(u), int(slot), _ptr(p), int(p.size)))
        return p

    def verifier_stats(self) -> Tuple[int, int]:
        """(pairs with a per-stream assignment, verifier evaluations of the last step)."""
        out = np.zeros(2, dtype=np.int64)
        _lib.check(self._lib.oww_verifier_stats(self._h, _ptr(out)))
        return int(out[0]), int(out[1])

    def set_vad_threshold(self, threshold: float) -> None:
        """VAD gate of model.py:366-381 on the device (0 = off); the scores come from push_vad()."""
        _lib.check(self._lib.oww_set_vad_threshold(self._h, float(threshold)))

    def push_vad(self, vad_scores: np.ndarray) -> None:
        """One voice-activity score per stream for the frame about to be stepped (what VAD.__call__ appends, vad.py:129-130)."""
        v = np.ascontiguousarray(vad_scores, dtype=np.float32)
        if v.shape != (self.n_streams,):
            raise ValueError(f"need one VAD score per stream ({self.n_streams})")
        _lib.check(self._lib.oww_push_vad(self._h, _ptr(v), 0))

    def get_vad(self) -> np.ndarray:
        """Voice-activity scores [S] the on-device network pushed for the last step (what VAD.__call__ appended, vad.py:129-130)."""
        out = np.empty(self.n_streams, dtype=np.float32)
        _lib.check(self._lib.oww_get_vad(self._h, _ptr(out)))
        return out

    def reset_vad(self, stream_ids: Optional[Sequence[int]] = None) -> None:
        """Zero the VAD state (recurrent h, c and score ring) of the listed streams (None = all).  reset() leaves it alone, like
        Model.reset() leaves Model.vad alone (model.py:226-230); call this when a stream slot is handed to a new caller."""
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        _lib.check(self._lib.oww_reset_vad(self._h, _ptr(ids), 0 if ids is None else ids.size))

    # ---- head bank (include/owwhip.h: oww_bank_*) ----
    def bank_add(self, head: dict) -> int:
        """Add a head (weights.synthetic_head / onnx_ingest.load_head layout) to the bank -> bank id."""
        blob = pack_head_blob(head)
        rc = self._lib.oww_bank_add(self._h, _ptr(blob), blob.nbytes)
        _lib.check(rc)
        return int(rc)

    def bank_remove(self, bank_id: int) -> None:
        _lib.check(self._lib.oww_bank_remove(self._h, int(bank_id)))

    def bank_set_postproc(self, bank_id: int, patience: int = 0, threshold: float = float("nan")) -> None:
        _lib.check(self._lib.oww_bank_set_postproc(self._h, int(bank_id), int(patience), float(threshold)))

    def subscribe(self, stream_ids: Sequence[int], bank_ids: np.ndarray) -> None:
        """bank_ids: int [n, bank_slots] (-1 = empty slot) for the n streams of stream_ids."""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).ravel()
        b = np.ascontiguousarray(bank_ids, dtype=np.int32).reshape(ids.size, self.bank_slots)
        _lib.check(self._lib.oww_subscribe(self._h, _ptr(ids), ids.size, _ptr(b)))

    def bank_scores(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is None:
            out = np.empty((self.n_streams, self.bank_slots), dtype=np.float32)
        _lib.check(self._lib.oww_bank_scores(self._h, _ptr(out)))
        return out

    def bank_scores_dev_ptr(self) -> int:
        return int(self._lib.oww_bank_scores_dev(self._h) or 0)

    def bank_routing(self) -> Dict[str, object]:
        info = np.zeros(6, dtype=np.int32)
        wb = C.c_double(0.0)
        _lib.check(self._lib.oww_bank_routing(self._h, _ptr(info), C.byref(wb)))
        return {"tiles": [int(info[0]), int(info[3])], "waves_per_tile": [int(info[1]), int(info[4])],
                "entries": [int(info[2]), int(info[5])], "weight_bytes": float(wb.value)}

    # ---- detection events (include/owwhip.h: oww_events_*) ----
    def set_event_thresholds(self, fixed: Optional[Sequence[float]] = None, bank: Optional[float] = None) -> None:
        """Event thresholds of the score columns ([n_labels]; NaN = the column never reports; None = keep) and of the bank slots."""
        thr = None
        if fixed is not None:
            thr = np.ascontiguousarray(fixed, dtype=np.float32)
            if thr.shape != (self.n_labels,):
                raise ValueError(f"need one event threshold per label ({self.n_labels})")
        _lib.check(self._lib.oww_events_set_thresholds(self._h, _ptr(thr), float("nan") if bank is None else float(bank)))

    def events(self) -> Tuple[np.ndarray, int]:
        """(records, n_total) of the last step / step_masked / collect: records is a structured array (EVENT_DTYPE) of the stored events
        in ascending (stream, column, slot) order, n_total counts every hit; len(records) < n_total = the call overflowed the capacity."""
        rec = np.zeros(self.event_capacity, dtype=EVENT_DTYPE)
        n_stored, n_total = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.oww_get_events(self._h, _ptr(rec), rec.size, C.byref(n_stored), C.byref(n_total)))
        return rec[:n_stored.value].copy(), int(n_total.value)

    def event_features(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """float32 [n, event_features, 96]: the feature rows (oldest first) behind stored events first .. first + n - 1 of the call
        events() refers to, as the ring held them right after the detecting step; n = None: up to the last stored event."""
        if n is None:
            n_stored = C.c_int32(0)
            _lib.check(self._lib.oww_get_events(self._h, None, 0, C.byref(n_stored), None))
            n = max(0, n_stored.value - int(first))
        out = np.empty((int(n), self.event_rows, EMB_DIM), dtype=np.float32)
        _lib.check(self._lib.oww_get_event_features(self._h, int(first), int(n), _ptr(out), 0))
        return out

    def events_dev_ptrs(self) -> Tuple[int, int, int]:
        """Device addresses (records, {n_stored, n_total}, snapshots) of the last synchronous step's events; 0 where there is none."""
        cnt = C.c_void_p()
        rec = self._lib.oww_events_dev(self._h, C.byref(cnt))
        return int(rec or 0), int(cnt.value or 0), int(self._lib.oww_event_features_dev(self._h) or 0)

    # ---- per-stream audio rings (include/owwhip.h: oww_audio_configure / oww_get_audio / oww_get_event_audio) ----
    check_audio_config = staticmethod(check_audio_config)

    def audio(self, stream_ids: Sequence[int], n_chunks: int) -> Tuple[np.ndarray, np.ndarray]:
        """(int16 [n, n_chunks * 1280], uint32 counts [n]): the newest n_chunks chunks of the listed streams, oldest first, zero where
        a stream has received less since its reset, and each stream's chunk counter.  Runs behind every queued step."""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).ravel()
        out = np.empty((ids.size, max(int(n_chunks), 0) * CHUNK), dtype=np.int16)
        counts = np.zeros(ids.size, dtype=np.uint32)
        _lib.check(self._lib.oww_get_audio(self._h, _ptr(ids), ids.size, int(n_chunks), _ptr(out), 0, _ptr(counts)))
        return out, counts

    def event_audio(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """int16 [n, event_audio * 1280]: the audio behind stored events first .. first + n - 1 of the call events() refers to, ending
        with the detecting chunk; n = None: up to the last stored event."""
        if n is None:
            n_stored = C.c_int32(0)
            _lib.check(self._lib.oww_get_events(self._h, None, 0, C.byref(n_stored), None))
            n = max(0, n_stored.value - int(first))
        out = np.empty((int(n), self.event_audio_chunks * CHUNK), dtype=np.int16)
        _lib.check(self._lib.oww_get_event_audio(self._h, int(first), int(n), _ptr(out), 0))
        return out

    def event_audio_dev_ptr(self) -> int:
        """Device address of the last synchronous step's audio snapshots; 0 where there is none."""
        return int(self._lib.oww_event_audio_dev(self._h) or 0)

    def event_label(self, record) -> Union[str, int]:
        """The score column's name for a fixed-head event ("name" or "name:j" for output j of a multi-output head), the bank id for a
        bank event."""
        col = int(record["column"])
        if col < 0:
            return int(record["bank_id"])
        for name, (lo, hi) in self.head_cols.items():
            if lo <= col < hi:
                return name if hi - lo == 1 else f"{name}:{col - lo}"
        raise ValueError(f"no score column {col}")

    # ---- stream state records (include/owwhip.h: oww_state_*, oww_move_streams) ----
    def state_info(self) -> Tuple[int, int]:
        """(bytes of one stream state record, 64-bit fingerprint of what a record's bits depend on)."""
        nb, fp = C.c_size_t(0), C.c_uint64(0)
        _lib.check(self._lib.oww_state_info(self._h, C.byref(nb), C.byref(fp)))
        return int(nb.value), int(fp.value)

    def export_state(self, stream_ids: Sequence[int], out: Optional[np.ndarray] = None) -> np.ndarray:
        """Records of the listed streams -> uint8 [n, record_bytes] (host, complete on return)."""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).ravel()
        nb = self.state_info()[0]
        if out is None:
            out = np.empty((ids.size, nb), dtype=np.uint8)
        elif out.dtype != np.uint8 or out.shape != (ids.size, nb) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint8 [{ids.size}, {nb}] array")
        _lib.check(self._lib.oww_state_export(self._h, _ptr(ids), ids.size, _ptr(out), 0))
        return out

    def import_state(self, stream_ids: Sequence[int], records: np.ndarray) -> None:
        """Put records (export_state of a handle with the same fingerprint) into the listed streams."""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).ravel()
        rec = np.ascontiguousarray(records)
        if rec.dtype != np.uint8 or rec.ndim != 2 or rec.shape[0] != ids.size:
            raise ValueError(f"records must be uint8 [{ids.size}, record_bytes], got {rec.dtype} {rec.shape}")
        nb = self.state_info()[0]
        if rec.shape[1] != nb:
            raise ValueError(f"records are {rec.shape[1]} bytes each, this handle's records have {nb}")
        _lib.check(self._lib.oww_state_import(self._h, _ptr(ids), ids.size, _ptr(rec), 0))

    def export_state_device(self, stream_ids: Sequence[int], out_dev_ptr: int) -> None:
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).ravel()
        _lib.check(self._lib.oww_state_export(self._h, _ptr(ids), ids.size, C.c_void_p(out_dev_ptr), 1))

    def import_state_device(self, stream_ids: Sequence[int], in_dev_ptr: int) -> None:
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).ravel()
        _lib.check(self._lib.oww_state_import(self._h, _ptr(ids), ids.size, C.c_void_p(in_dev_ptr), 1))

    def move_streams(self, src: Sequence[int], dst: Sequence[int]) -> None:
        """Stream src[i] becomes stream dst[i], with every bit of its state, its subscriptions and its verifier assignments."""
        s = np.ascontiguousarray(src, dtype=np.int32).ravel()
        d = np.ascontiguousarray(dst, dtype=np.int32).ravel()
        if s.size != d.size:
            raise ValueError(f"src and dst must have the same length ({s.size} != {d.size})")
        _lib.check(self._lib.oww_move_streams(self._h, _ptr(s), _ptr(d), s.size))

    def sync(self):
        _lib.check(self._lib.oww_sync(self._h))

    def range_status(self, clear: bool = False) -> bool:
        """True when the fp16-split kernels (use_mfma=3) have seen an activation beyond the f16 range since the flag was
        last cleared (sticky; every step / collect / sync raises `OwwRangeError` while it is up).  Waits for the stream."""
        rc = self._lib.oww_range_status(self._h, int(bool(clear)))
        if rc == _lib.ERANGE:
            return True
        _lib.check(rc)
        return False

    def range_where(self):
        """(first_stream, n_streams) of a wave that saw the out-of-range value behind OwwRangeError -- the offender is among these
        streams -- or (-1, 0) when the flag is down / the position is unknown (include/owwhip.h: oww_range_where)."""
        a, b = C.c_int32(-1), C.c_int32(0)
        _lib.check(self._lib.oww_range_where(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @property
    def scores_dev_ptr(self) -> int:
        return int(self._lib.oww_scores_dev(self._h) or 0)

    # ---- stage-level entry points (the reference's per-stage closures)
    def mel(self, pcm: np.ndarray) -> np.ndarray:
        """melspec_model_predict (utils.py:87): int16 [B, n] -> dB [B, F, 32]."""
        pcm = np.ascontiguousarray(np.atleast_2d(pcm))
        if pcm.dtype != np.int16:
            raise ValueError(f"Input data must be 16-bit integers (i.e., 16-bit PCM audio). You provided {pcm.dtype} data.")
        B, n = pcm.shape
        out = np.empty((B, (n - 512) // 160 + 1, 32), dtype=np.float32)
        _lib.check(self._lib.oww_mel(self._h, _ptr(pcm), B, n, _ptr(out)))
        return out

    def mel_clips(self, pcm: np.ndarray) -> np.ndarray:
        """Like mel(), but every clip gets its own clamp floor (the reference's per-clip CPU path, utils.py:243-290)."""
        pcm = np.ascontiguousarray(np.atleast_2d(pcm))
        if pcm.dtype != np.int16:
            raise ValueError(f"Input data must be 16-bit integers (i.e., 16-bit PCM audio). You provided {pcm.dtype} data.")
        B, n = pcm.shape
        if B > self.n_streams_padded:
            raise ValueError(f"at most {self.n_streams_padded} clips per call (the handle's stream count)")
        out = np.empty((B, (n - 512) // 160 + 1, 32), dtype=np.float32)
        _lib.check(self._lib.oww_mel_clips(self._h, _ptr(pcm), B, n, _ptr(out)))
        return out

    def embed_clips(self, pcm: np.ndarray) -> np.ndarray:
        """AudioFeatures.embed_clips on the device (utils.py:354-385): int16 [B, n] -> [B, n_windows, 96], mel, window
        walk and CNN without leaving HBM.  Borrows the streaming machinery of streams [0, B) (B rounded up to 8): their state is
        parked for the call and put back, so live streams continue bit for bit (ABI 2)."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 2:
            raise ValueError("embed_clips expects a 2-D int16 array [B, samples]")
        B, n = pcm.shape
        if B > self.n_streams_padded:
            raise ValueError(f"at most {self.n_streams_padded} clips per call (the handle's stream count)")
        F = (n - 512) // 160 + 1
        if n < 512 or F < 76:
            raise ValueError("clips are shorter than one 76-frame embedding window (12512 samples, 782 ms)")
        out = np.empty((B, (F - 76) // 8 + 1, EMB_DIM), dtype=np.float32)
        _lib.check(self._lib.oww_embed_clips(self._h, _ptr(pcm), 0, B, n, _ptr(out), 0))
        return out

    def embed_clips_device(self, pcm_ptr: int, B: int, n: int, out_ptr: int) -> None:
        """The same on device buffers (int16 [B, n] -> f32 [B, n_windows, 96]); pointers are raw device addresses."""
        _lib.check(self._lib.oww_embed_clips(self._h, C.c_void_p(pcm_ptr), 1, int(B), int(n), C.c_void_p(out_ptr), 1))

    def embed(self, mel_rows: np.ndarray) -> np.ndarray:
        """embedding_model_predict over sliding windows (utils.py:229-236): [B, 76+8j, 32] -> [B, j+1, 96].
        Borrows the streaming machinery of streams [0, B) (B rounded up to 8): their state is parked for the call and put back, so
        live streams continue bit for bit (ABI 2)."""
        m = np.ascontiguousarray(mel_rows, dtype=np.float32)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[2] != 32:
            raise ValueError(f"embed expects mel rows [B, 76 + 8 j, 32], got {m.shape}")
        B, rows, _ = m.shape
        if rows < 76 or (rows - 76) % 8:
            raise ValueError(f"embed expects 76 + 8 j mel rows per clip (whole windows), got {rows}")
        if B < 1 or B > self.n_streams_padded:
            raise ValueError(f"between 1 and {self.n_streams_padded} clips per call (the handle's stream count)")
        out = np.empty((B, (rows - 76) // 8 + 1, EMB_DIM), dtype=np.float32)
        _lib.check(self._lib.oww_embed(self._h, _ptr(m), B, rows, _ptr(out)))
        return out

    def head(self, head: Union[int, str], features: np.ndarray) -> np.ndarray:
        """model_prediction_function[name] (model.py:137-138): [B, T, 96] -> [B, n_out]."""
        idx = self.head_names.index(head) if isinstance(head, str) else int(head)
        f = np.ascontiguousarray(features, dtype=np.float32)
        if f.ndim == 2:
            f = f[None]
        hd = self.heads[self.head_names[idx]]
        if f.shape[1:] != (hd["T"], EMB_DIM):
            raise ValueError(f"features must be [B, {hd['T']}, 96], got {f.shape}")
        out = np.empty((f.shape[0], hd["n_out"]), dtype=np.float32)
        _lib.check(self._lib.oww_head(self._h, idx, _ptr(f), f.shape[0], _ptr(out)))
        return out

    # ---- dense scoring (include/owwhip.h: oww_score_shape / oww_score_features / oww_score_clips)
    def score_shape(self, n_rows: int) -> Tuple[int, int]:
        """(n_win, t_max) for sequences of n_rows feature rows: t_max = the largest window length over the fixed heads,
        n_win = n_rows - t_max + 1."""
        n_win, t_max = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.oww_score_shape(self._h, int(n_rows), C.byref(n_win), C.byref(t_max)))
        return int(n_win.value), int(t_max.value)

    def score_features(self, feats: np.ndarray) -> np.ndarray:
        """Every window of feature sequences through the fixed heads (train.py:874-879): [B, n_rows, 96] -> raw head outputs
        [B, n_win, n_labels].  Window w ends at row w + t_max - 1 and each head reads its own last T rows; all n_rows - t_max + 1
        windows are returned (out[:, :-1] is the set train.py:875 scores).  No post-processing, no stream state touched."""
        f = np.ascontiguousarray(feats, dtype=np.float32)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != EMB_DIM:
            raise ValueError(f"score_features expects [B, n_rows, 96], got {f.shape}")
        B, n_rows, _ = f.shape
        n_win, _ = self.score_shape(n_rows)
        out = np.empty((B, n_win, self.n_labels), dtype=np.float32)
        _lib.check(self._lib.oww_score_features(self._h, _ptr(f), 0, B, n_rows, _ptr(out), 0))
        return out

    def score_clips(self, pcm: np.ndarray, return_features: bool = False):
        """int16 clips [B, n] -> [B, n_win, n_labels]: score_features over the clips' embed_clips embeddings, which stay on the device
        (with return_features: also the embeddings [B, n_out, 96], exactly what embed_clips returns).  Borrows streams [0, B) as
        embed_clips does.  These are embed_clips-path scores (one mel clamp floor per clip, no seeded feature ring)."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 2:
            raise ValueError("score_clips expects a 2-D int16 array [B, samples]")
        B, n = pcm.shape
        if B < 1 or B > self.n_streams_padded:
            raise ValueError(f"between 1 and {self.n_streams_padded} clips per call (the handle's stream count)")
        F = (n - 512) // 160 + 1
        if n < 512 or F < 76:
            raise ValueError("clips are shorter than one 76-frame embedding window (12512 samples, 782 ms)")
        n_rows = (F - 76) // 8 + 1
        n_win, _ = self.score_shape(n_rows)
        out = np.empty((B, n_win, self.n_labels), dtype=np.float32)
        emb = np.empty((B, n_rows, EMB_DIM), dtype=np.float32) if return_features else None
        _lib.check(self._lib.oww_score_clips(self._h, _ptr(pcm), 0, B, n, _ptr(out), 0, _ptr(emb) if return_features else None, 0))
        return (out, emb) if return_features else out

    # ---- dense scoring over the head bank (include/owwhip.h: oww_bank_score_shape / oww_bank_score_features / oww_bank_score_stats)
    @staticmethod
    def _bank_ids(ids) -> np.ndarray:
        a = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if a.size < 1:
            raise ValueError("need at least one bank id")
        return a

    @staticmethod
    def _bank_feats(feats) -> np.ndarray:
        f = np.ascontiguousarray(feats, dtype=np.float32)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != EMB_DIM:
            raise ValueError(f"bank scoring expects [B, n_rows, 96], got {f.shape}")
        return f

    def bank_score_shape(self, ids: Sequence[int], n_rows: int) -> Tuple[int, int]:
        """(n_win, t_max) for sequences of n_rows feature rows scored with the listed bank heads: t_max = their largest window
        length, n_win = n_rows - t_max + 1."""
        a = self._bank_ids(ids)
        n_win, t_max = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.oww_bank_score_shape(self._h, _ptr(a), a.size, int(n_rows), C.byref(n_win), C.byref(t_max)))
        return int(n_win.value), int(t_max.value)

    def bank_score_features(self, feats: np.ndarray, ids: Sequence[int]) -> np.ndarray:
        """Every window of feature sequences [B, n_rows, 96] through the listed bank heads -> raw sigmoid outputs [B, n_win, n_ids]
        (column i: bank head ids[i]; duplicates allowed).  Window w ends at row w + t_max - 1 and each head reads its own last T rows.
        No post-processing; subscriptions, bank scores and every other piece of live state stay as they are."""
        f, a = self._bank_feats(feats), self._bank_ids(ids)
        B, n_rows, _ = f.shape
        n_win, _ = self.bank_score_shape(a, n_rows)
        out = np.empty((B, n_win, a.size), dtype=np.float32)
        _lib.check(self._lib.oww_bank_score_features(self._h, _ptr(f), 0, B, n_rows, _ptr(a), a.size, _ptr(out), 0))
        return out

    def bank_score_stats(self, feats: np.ndarray, ids: Sequence[int], thresholds: Optional[Sequence[float]] = None) -> Dict[str, np.ndarray]:
        """What a validation scan wants of bank_score_features' matrix, reduced on the device (the matrix is never written):
        {"count": int32 [B, n_ids] windows with score >= thresholds[i] (None = 0.5, train.py:100), "max": float32 [B, n_ids],
        "argmax": int32 [B, n_ids] the first window that attains the maximum} -- bit for bit numpy's on the matrix."""
        f, a = self._bank_feats(feats), self._bank_ids(ids)
        B, n_rows, _ = f.shape
        thr = None
        if thresholds is not None:
            thr = np.ascontiguousarray(thresholds, dtype=np.float32).ravel()
            if thr.shape != (a.size,):
                raise ValueError(f"need one threshold per listed head ({a.size})")
        count, mx, arg = (np.empty((B, a.size), dtype=t) for t in (np.int32, np.float32, np.int32))
        _lib.check(self._lib.oww_bank_score_stats(self._h, _ptr(f), 0, B, n_rows, _ptr(a), a.size, _ptr(thr), _ptr(count), _ptr(mx), _ptr(arg)))
        return {"count": count, "max": mx, "argmax": arg}

    # ---- dense scoring: ordered hit lists (include/owwhip.h: oww_score_hits_layout / oww_score_hits / oww_score_clip_hits /
    #      oww_bank_score_hits)
    def score_hits_layout(self, cap: int, ids: Optional[Sequence[int]] = None) -> np.ndarray:
        """int64 [n_cols + 1]: where each column's windows start in the flat windows buffer (floats), and the buffer's size; column
        c holds [cap, T_c, 96].  ids None = the fixed score columns, else the listed bank heads."""
        a = None if ids is None else self._bank_ids(ids)
        off = np.zeros((self.n_labels if a is None else a.size) + 1, dtype=np.int64)
        _lib.check(self._lib.oww_score_hits_layout(self._h, _ptr(a), 0 if a is None else a.size, int(cap), _ptr(off)))
        return off

    def _thresholds(self, thresholds, n_cols: int) -> Optional[np.ndarray]:
        if thresholds is None:
            return None
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (n_cols,)) if np.ndim(thresholds) == 0
                                   else thresholds, dtype=np.float32).ravel()
        if thr.shape != (n_cols,):
            raise ValueError(f"need one threshold per column ({n_cols})")
        return thr

    def _hits_raw(self, call, n_cols: int, cap: int, off: Optional[np.ndarray], hits_buf=None, windows_buf=None) -> dict:
        """Runs one of the three entries (call(hits_ptr, n_stored_ptr, n_total_ptr, windows_ptr)) on buffers of its own, or the
        caller's, and returns them as they are: {"hits": DENSE_HIT [n_cols, cap], "n_stored", "n_total", "windows" flat or None,
        "win_offset"}."""
        hits = np.zeros((n_cols, cap), dtype=DENSE_HIT) if hits_buf is None else hits_buf
        n_stored, n_total = np.zeros(n_cols, dtype=np.int32), np.zeros(n_cols, dtype=np.int64)
        windows = None
        if off is not None:
            windows = np.empty(int(off[-1]), dtype=np.float32) if windows_buf is None else windows_buf
        _lib.check(call(hits.ctypes.data_as(C.c_void_p), _ptr(n_stored), _ptr(n_total), _ptr(windows)))
        return {"hits": hits, "n_stored": n_stored, "n_total": n_total, "windows": windows, "win_offset": off}

    @staticmethod
    def _hits_columns(raw: dict) -> List[dict]:
        """The raw buffers of a hit-list call, per column and trimmed to n_stored."""
        cols = []
        off = raw["win_offset"]
        for c in range(raw["hits"].shape[0]):
            n = int(raw["n_stored"][c])
            rec = raw["hits"][c, :n]
            col = {"seq": rec["seq"].copy(), "window": rec["window"].copy(), "score": rec["score"].copy(), "n_total": int(raw["n_total"][c]),
                   "windows": None}
            if raw["windows"] is not None:
                cap = raw["hits"].shape[1]
                T = int(off[c + 1] - off[c]) // (cap * EMB_DIM)
                col["windows"] = raw["windows"][off[c]: off[c] + n * T * EMB_DIM].reshape(n, T, EMB_DIM).copy()
            cols.append(col)
        return cols

    def score_hits(self, feats: np.ndarray, thresholds=None, cap: int = 4096, return_windows: bool = True) -> List[dict]:
        """The hits of score_features' matrix without the matrix (Model._get_positive_prediction_frames, model.py:428-479): per
        fixed score column a dict {"seq", "window", "score", "n_total", "windows"} -- the (sequence, window) positions with
        score >= thresholds[c] (None = 0.5; one number = every column; a NaN column never reports) in ascending order, the first
        `cap` of them; their scores, bit for bit the matrix's; n_total, the count without the cap; and windows [n, T_c, 96], each
        hit's own T_c feature rows."""
        f = self._bank_feats(feats)
        B, n_rows, _ = f.shape
        thr = self._thresholds(thresholds, self.n_labels)
        off = self.score_hits_layout(cap) if return_windows else None
        raw = self._hits_raw(lambda hp, ns, nt, wp: self._lib.oww_score_hits(self._h, _ptr(f), 0, B, n_rows, _ptr(thr), int(cap), hp, ns, nt, wp, 0),
                             self.n_labels, int(cap), off)
        return self._hits_columns(raw)

    def score_clip_hits(self, pcm: np.ndarray, thresholds=None, cap: int = 4096, return_windows: bool = True) -> List[dict]:
        """score_hits over the clips' embed_clips embeddings [B, n] int16 -> per column the hits of score_clips' matrix.  The
        embeddings never leave the device: only hits and their windows come back.  Borrows streams [0, B) as embed_clips does."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 2:
            raise ValueError("score_clip_hits expects a 2-D int16 array [B, samples]")
        B, n = pcm.shape
        thr = self._thresholds(thresholds, self.n_labels)
        off = self.score_hits_layout(cap) if return_windows else None
        raw = self._hits_raw(lambda hp, ns, nt, wp: self._lib.oww_score_clip_hits(self._h, _ptr(pcm), 0, B, n, _ptr(thr), int(cap), hp, ns, nt, wp, 0),
                             self.n_labels, int(cap), off)
        return self._hits_columns(raw)

    def bank_score_hits(self, feats: np.ndarray, ids: Sequence[int], thresholds=None, cap: int = 4096, return_windows: bool = True) -> List[dict]:
        """score_hits over the listed bank heads: per listed id (duplicates allowed) the hits of bank_score_features' matrix, which
        is never written.  n_total of column i is the sum over sequences of bank_score_stats' count[:, i]."""
        f, a = self._bank_feats(feats), self._bank_ids(ids)
        B, n_rows, _ = f.shape
        thr = self._thresholds(thresholds, a.size)
        off = self.score_hits_layout(cap, a) if return_windows else None
        raw = self._hits_raw(lambda hp, ns, nt, wp: self._lib.oww_bank_score_hits(self._h, _ptr(f), 0, B, n_rows, _ptr(a), a.size, _ptr(thr), int(cap),
                                                                                  hp, ns, nt, wp, 0), a.size, int(cap), off)
        return self._hits_columns(raw)

    # ---- introspection
    def get_features(self, sid: int, T: int = 16) -> np.ndarray:
        out = np.empty((T, EMB_DIM), dtype=np.float32)
        _lib.check(self._lib.oww_get_features(self._h, int(sid), int(T), _ptr(out)))
        return out

    def get_mel(self, sid: int, n_rows: int = 8) -> np.ndarray:
        out = np.empty((n_rows, 32), dtype=np.float32)
        _lib.check(self._lib.oww_get_mel(self._h, int(sid), _ptr(out), int(n_rows)))
        return out

    def debug_layer(self, sid: int, layer: int) -> np.ndarray:
        """New rows of CNN layer `layer` (0..19) for stream sid from the last chunk: [rows, F, C]."""
        r, f, c = LAYER_NEW_SHAPES[layer]
        out = np.empty(r * f * c, dtype=np.float32)
        _lib.check(self._lib.oww_debug_read(self._h, int(sid), int(layer), _ptr(out), out.size))
        return out.reshape(r, f, c)

    def debug_profile(self) -> np.ndarray:
        """Shader-clock phase stamps [stage B..E][wave][mark] of workgroup $OWW_PROF_BLOCK (development aid)."""
        out = np.zeros((4, 16, 16), dtype=np.int64)
        _lib.check(self._lib.oww_debug_profile(self._h, _ptr(out), out.size))
        return out

    def enable_timing(self, on: bool = True):
        _lib.check(self._lib.oww_enable_timing(self._h, int(on)))

    def kernel_times(self) -> Dict[str, Dict[str, float]]:
        k = len(KERNEL_CLASSES)
        ms = (C.c_double * k)()
        n = (C.c_int64 * k)()
        _lib.check(self._lib.oww_kernel_times(self._h, ms, n))
        return {KERNEL_CLASSES[i]: {"ms": ms[i], "launches": int(n[i])} for i in range(k)}

    # ---- multi-GPU delivery of the scores over RCCL without torch.distributed (include/owwhip.h: oww_comm_*)
    @staticmethod
    def comm_id() -> bytes:
        """Rank 0: the 128 bytes every rank passes to comm_init (ncclGetUniqueId); ship them by any side channel."""
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().oww_comm_id(buf))
        return buf.raw

    def comm_init(self, comm_id: bytes, rank: int, world: int) -> None:
        if len(comm_id) != 128:
            raise ValueError("comm_id must be the 128 bytes of StreamEngine.comm_id()")
        _lib.check(self._lib.oww_comm_init(self._h, C.c_char_p(comm_id), int(rank), int(world)))

    def gather_scores(self, out_dev_ptr: int, counts: Sequence[int]) -> None:
        """Enqueue the gather of every rank's [S_r, n_labels] scores to rank 0's device buffer `out_dev_ptr` (asynchronous)."""
        c = np.ascontiguousarray(counts, dtype=np.int32)
        _lib.check(self._lib.oww_gather_scores(self._h, C.c_void_p(int(out_dev_ptr)), _ptr(c)))

    def comm_count(self) -> int:
        """Ranks the handle's RCCL communicator itself reports (ncclCommCount)."""
        n = C.c_int32(0)
        _lib.check(self._lib.oww_comm_count(self._h, C.byref(n)))
        return int(n.value)

    def comm_destroy(self) -> None:
        _lib.check(self._lib.oww_comm_destroy(self._h))

    def use_graph(self, on: bool = True):
        _lib.check(self._lib.oww_use_graph(self._h, int(on)))
