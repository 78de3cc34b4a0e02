"""Rate conversion to 16 kHz for whole batches of streams on the device (SURVEY §8f-3 "on-device resample").

The reference's serving example converts every websocket message with `resampy.resample(data, sample_rate, 16000)` before
`predict()` (examples/web/streaming_server.py:57-58): a stateless, band-limited (Kaiser-windowed sinc) interpolation per
message.  This module designs the equivalent polyphase filter bank once per input rate; `oww_resample` (include/owwhip.h) applies
it to [S, n_in] int16 on the GPU, `apply_numpy` is the host restatement the tests check it against.

    p / q = rate_in / 16000 in lowest terms; output sample j sits at input position j * p / q:
    i0 = (j * p) // q, phase = (j * p) % q,   out[j] = sat_int16(rint(sum_k taps[phase, k] * x[i0 + k - half + 1]))
with x = 0 outside the message.  taps[phase, k] = window((k - half + 1 - phase / q) / (ZC * s)) * sinc((k - half + 1 - phase / q) / s) / s,
s = max(1, rate_in / 16000) (the pass band ends at the lower of the two Nyquist rates), ZC zero crossings each side, every phase
normalised to unit DC gain.
"""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache
from typing import Tuple

import numpy as np

ZERO_CROSSINGS = 12
KAISER_BETA = 8.0
ROLLOFF = 0.945          # pass band edge as a fraction of the lower Nyquist rate (resampy's kaiser_best uses ~0.9476)


@lru_cache(maxsize=32)
def design(rate_in: int, rate_out: int = 16000) -> Tuple[int, int, np.ndarray]:
    """(p, q, taps float32 [q, 2 * half]) for rate_in -> rate_out."""
    if not 1000 <= int(rate_in) <= 384000:
        raise ValueError(f"sample rate {rate_in} Hz is outside [1000, 384000]")
    r = Fraction(int(rate_in), int(rate_out))
    p, q = r.numerator, r.denominator
    s = max(1.0, rate_in / rate_out) / ROLLOFF
    half = int(np.ceil(ZERO_CROSSINGS * s))
    k = np.arange(2 * half, dtype=np.float64) - (half - 1)                  # tap offsets relative to i0
    ph = np.arange(q, dtype=np.float64)[:, None] / q
    d = k[None, :] - ph                                                     # distance of the tap from the output position, in input samples
    u = d / (ZERO_CROSSINGS * s)
    win = np.where(np.abs(u) < 1.0, np.i0(KAISER_BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, 1.0))) / np.i0(KAISER_BETA), 0.0)
    taps = win * np.sinc(d / s) / s
    taps /= taps.sum(axis=1, keepdims=True)
    return p, q, np.ascontiguousarray(taps, dtype=np.float32)


def n_out_for(n_in: int, rate_in: int, rate_out: int = 16000) -> int:
    p, q, _ = design(rate_in, rate_out)
    return (int(n_in) * q) // p


def apply_numpy(x: np.ndarray, rate_in: int) -> np.ndarray:
    """Host restatement of oww_resample (float64 accumulation): int16 [..., n_in] -> int16 [..., n_out]."""
    p, q, taps = design(rate_in)
    x = np.asarray(x)
    if rate_in == 16000:
        return x.copy()
    n_in = x.shape[-1]
    n_out = (n_in * q) // p
    half = taps.shape[1] // 2
    j = np.arange(n_out)
    i0 = (j * p) // q
    ph = (j * p) % q
    idx = i0[:, None] + np.arange(2 * half)[None, :] - (half - 1)            # [n_out, taps]
    ok = (idx >= 0) & (idx < n_in)
    xs = np.where(ok, x[..., np.clip(idx, 0, n_in - 1)].astype(np.float64), 0.0)
    y = (xs * taps[ph].astype(np.float64)).sum(-1)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


# ---- stateful stream ingest (include/owwhip.h: oww_ingest_configure / oww_ingest): G.711 decode and continuous conversion ----------
ENCODINGS = {"pcm16": 0, "ulaw": 1, "alaw": 2}          # OWW_ENC_PCM16 / OWW_ENC_ULAW / OWW_ENC_ALAW


def decode_ulaw(codes) -> np.ndarray:
    """G.711 mu-law bytes -> int16 (audioop.ulaw2lin): u = ~b; t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7); 0x84 - t if u & 0x80 else t - 0x84."""
    u = (~np.asarray(codes).astype(np.int32)) & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def decode_alaw(codes) -> np.ndarray:
    """G.711 A-law bytes -> int16 (audioop.alaw2lin): a = b ^ 0x55; t = (a & 15) << 4; seg = (a >> 4) & 7; seg 0: t + 8, seg 1: t + 0x108,
    else (t + 0x108) << (seg - 1); positive if a & 0x80."""
    a = (np.asarray(codes).astype(np.int32) ^ 0x55) & 0xFF
    t = (a & 15) << 4
    seg = (a >> 4) & 7
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t).astype(np.int16)


def decode(data, encoding: str) -> np.ndarray:
    """A message in one of ENCODINGS -> int16."""
    if encoding not in ENCODINGS:
        raise ValueError(f"unknown encoding {encoding!r} (one of {sorted(ENCODINGS)})")
    if encoding == "pcm16":
        return np.asarray(data).astype(np.int16)
    return decode_ulaw(data) if encoding == "ulaw" else decode_alaw(data)


def ingest_numpy(x_decoded: np.ndarray, rate: int, history: np.ndarray = None) -> Tuple[np.ndarray, np.ndarray]:
    """Host restatement of one oww_ingest message in float64, BEFORE rounding: decoded samples [..., n_in] at `rate` Hz and the
    stream's history [..., n_taps - 1] (the decoded samples before this message, oldest first; None = a fresh stream: zeros) ->
    (y float64 [..., n_in * q / p], new history).  The caller rounds: np.clip(np.rint(y), -32768, 32767).  With X = history | message,
    y[j] = sum_k taps[(j p) % q][k] * X[(j p) // q + k]: every message starts at phase 0, so n_in * q must be a multiple of p."""
    p, q, taps = design(rate)
    x = np.asarray(x_decoded, dtype=np.float64)
    n_in, n_taps = x.shape[-1], taps.shape[1]
    if (n_in * q) % p:
        raise ValueError(f"a message must hold a whole number of output samples: n_in * q = {n_in} * {q} is no multiple of p = {p}")
    if history is None:
        history = np.zeros(x.shape[:-1] + (n_taps - 1,), np.float64)
    ext = np.concatenate([np.asarray(history, np.float64), x], axis=-1)
    jp = np.arange((n_in * q) // p, dtype=np.int64) * p
    idx = (jp // q)[:, None] + np.arange(n_taps)[None, :]                  # [n_out, n_taps] into ext
    y = (ext[..., idx] * taps[jp % q].astype(np.float64)).sum(-1)
    return y, ext[..., ext.shape[-1] - (n_taps - 1):]


# ---- ingest classes (include/owwhip.h: oww_ingest_configure_classes / oww_ingest_mixed): every stream its own rate and encoding ------
def class_params(rate: int, encoding: str):
    """(p, q, taps or None, n_taps) of the class (rate, encoding): 16000 Hz means decode only (p = q = 1, no filter, no history)."""
    if encoding not in ENCODINGS:
        raise ValueError(f"unknown encoding {encoding!r} (one of {sorted(ENCODINGS)})")
    if int(rate) == 16000:
        return 1, 1, None, 0
    p, q, taps = design(int(rate))
    return p, q, taps, taps.shape[1]


def class_n_in(rate: int, n_out: int = 1280) -> int:
    """Input samples of one message of `n_out` 16 kHz samples at `rate` Hz; ValueError when that is no whole number."""
    r = Fraction(int(rate), 16000)
    if (int(n_out) * r.numerator) % r.denominator:
        raise ValueError(f"{n_out} output samples are no whole number of input samples at {rate} Hz")
    return int(n_out) * r.numerator // r.denominator


def class_row_bytes(classes, n_out: int = 1280) -> int:
    """Bytes of the widest class's message of n_out outputs, rounded up to 16: the row pitch oww_ingest_mixed wants."""
    widest = max(class_n_in(rate, n_out) * (2 if enc == "pcm16" else 1) for rate, enc in classes)
    return (widest + 15) // 16 * 16


def pack_ingest_rows(per_stream_arrays, class_ids, classes, n_out: int = 1280, out: np.ndarray = None) -> np.ndarray:
    """uint8 [S, row_bytes] for oww_ingest_mixed from one array per stream: int16 for a "pcm16" class, uint8 for "ulaw" / "alaw", each
    exactly class_n_in(rate, n_out) long (ValueError otherwise).  None leaves a stream's row as it is (zeros in a fresh array): for
    streams that sit out.  `classes` is the list given to configure_ingest_classes, class_ids[s] the class of stream s."""
    S = len(per_stream_arrays)
    if len(class_ids) != S:
        raise ValueError(f"{S} arrays but {len(class_ids)} class ids")
    rb = class_row_bytes(classes, n_out)
    if out is None:
        out = np.zeros((S, rb), np.uint8)
    elif out.dtype != np.uint8 or out.shape != (S, rb) or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous uint8 [{S}, {rb}] array")
    for s, (x, c) in enumerate(zip(per_stream_arrays, class_ids)):
        if not 0 <= int(c) < len(classes):
            raise ValueError(f"stream {s}: unknown class {c}")
        if x is None:
            continue
        rate, enc = classes[int(c)]
        want = np.int16 if enc == "pcm16" else np.uint8
        x = np.asarray(x)
        n = class_n_in(rate, n_out)
        if x.dtype != want:
            raise ValueError(f"stream {s}: class {c} ({rate} Hz {enc}) takes {np.dtype(want).name}, got {x.dtype}")
        if x.shape != (n,):
            raise ValueError(f"stream {s}: class {c} ({rate} Hz {enc}) takes {n} samples for {n_out} outputs, got shape {x.shape}")
        out[s, :x.nbytes] = np.ascontiguousarray(x).view(np.uint8)
    return out


def ingest_mixed_numpy(rows: np.ndarray, class_ids, classes, histories, n_out: int = 1280, stream_on=None) -> np.ndarray:
    """Host definition of one oww_ingest_mixed message: rows uint8 [S, row_bytes], class_ids[s] the class of stream s, `classes` the
    list of (rate, encoding), `histories` a list of S arrays (None = silence) that is updated in place.  Per stream this is decode +
    ingest_numpy + the device's rounding; a 16 kHz class is decode only.  -> int16 [S, n_out]; a stream with stream_on[s] == 0 is not
    read, keeps its history and has a zero row."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2:
        raise ValueError(f"rows must be uint8 [S, row_bytes], got {rows.dtype} {rows.shape}")
    out = np.zeros((rows.shape[0], int(n_out)), np.int16)
    for s in range(rows.shape[0]):
        if stream_on is not None and not stream_on[s]:
            continue
        rate, enc = classes[int(class_ids[s])]
        n = class_n_in(rate, n_out)
        raw = rows[s, :n * (2 if enc == "pcm16" else 1)]
        x = decode(raw.view(np.int16) if enc == "pcm16" else raw, enc)
        if int(rate) == 16000:
            out[s] = x
            continue
        y, histories[s] = ingest_numpy(x, int(rate), histories[s])
        out[s] = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    return out
