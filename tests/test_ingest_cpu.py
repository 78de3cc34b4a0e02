"""CPU tier of the stateful stream ingest (oww_ingest_configure / oww_ingest / oww_step_ingest): the G.711 expansions, the float64
restatement of one message (`resample.ingest_numpy`) against the header's definition on the whole recording, and the ABI surface.

The definition: with X = every decoded sample of the stream, out[J] = sum_k taps[(J p) % q][k] * X[(J p) / q + k - (n_taps - 1)],
X[i] = 0 for i < 0 -- `resample_ref.ref64` (oww_resample's definition, written from the header) on zeros(n_taps / 2) | X.  The
tolerance before rounding, 1e-9, is float64 round-off of a 26..74-term sum of products below 2^15 * 1.5 (n_taps * 2^-53 * A < 1e-10)."""
import os
import re

import numpy as np
import pytest

import resample_ref as RR
from openwakeword_amd import _lib
from openwakeword_amd import resample as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RATES = (8000, 11025, 44100, 48000)
FRAME = {8000: 640, 11025: 882, 44100: 3528, 48000: 3840}                   # the 80 ms message of each rate
N_FRAMES = 4
NOISE6000 = RR.SIGNALS.index("noise6000")


def test_g711_decoders_equal_audioop_on_all_256_codes():
    codes = np.arange(256, dtype=np.uint8)
    try:
        import audioop
        want_u = np.frombuffer(audioop.ulaw2lin(codes.tobytes(), 2), np.int16)
        want_a = np.frombuffer(audioop.alaw2lin(codes.tobytes(), 2), np.int16)
    except ImportError:
        tab = np.load(os.path.join(ROOT, "tests", "golden", "g711_tables.npz"))
        want_u, want_a = tab["ulaw"], tab["alaw"]
    got_u, got_a = R.decode_ulaw(codes), R.decode_alaw(codes)
    assert got_u.dtype == np.int16 and got_a.dtype == np.int16
    assert (got_u == want_u).all() and (got_a == want_a).all()
    assert (R.decode_ulaw(codes.reshape(16, 16)) == want_u.reshape(16, 16)).all()      # any shape


def test_committed_g711_table_is_the_decoders():
    tab = np.load(os.path.join(ROOT, "tests", "golden", "g711_tables.npz"))
    codes = np.arange(256, dtype=np.uint8)
    assert tab["ulaw"].dtype == np.int16 and tab["ulaw"].shape == (256,) and tab["alaw"].shape == (256,)
    assert (tab["ulaw"] == R.decode_ulaw(codes)).all() and (tab["alaw"] == R.decode_alaw(codes)).all()
    assert tab["ulaw"][0xFF] == 0 and tab["ulaw"][0x00] == -32124 and tab["alaw"][0x55] == -8 and tab["alaw"][0xD5] == 8


def _chain(x, rate, sizes):
    """ingest_numpy message after message (sizes in turn) -> float64 [rows, n_out]"""
    hist, outs, at, i = None, [], 0, 0
    while at < x.shape[-1]:
        n = sizes[i % len(sizes)]
        y, hist = R.ingest_numpy(x[..., at:at + n], rate, hist)
        outs.append(y)
        at += n
        i += 1
    assert at == x.shape[-1]
    return np.concatenate(outs, axis=-1)


def _per_message_zero_padded(x, rate, n):
    """the restatement NOT to write: every message converted on its own from a zero history (and with its own latency)"""
    return np.concatenate([R.ingest_numpy(x[..., a:a + n], rate, None)[0] for a in range(0, x.shape[-1], n)], axis=-1)


@pytest.mark.parametrize("rate", RATES)
def test_ingest_numpy_chained_equals_the_definition_on_the_whole_recording(rate):
    p, q, taps = R.design(rate)
    n_taps, half = taps.shape[1], taps.shape[1] // 2
    x = RR.signals(rate, FRAME[rate] * N_FRAMES)
    whole = np.concatenate([np.zeros((x.shape[0], half), np.int16), x], axis=1)
    y_ref, A = RR.ref64(whole, p, q, taps)
    n_out = x.shape[1] * q // p
    y_ref, A = y_ref[:, :n_out], A[:, :n_out]
    # 80 ms messages
    y = _chain(x, rate, [FRAME[rate]])
    assert y.shape == y_ref.shape
    assert np.abs(y - y_ref).max() <= 1e-9, f"{rate} Hz, 80 ms messages: {np.abs(y - y_ref).max():.3e}"
    # messages shorter than n_taps - 1: the smallest message that holds whole outputs, and two and three of them in turn
    unit = p                                                                 # n_in * q % p == 0 with gcd(p, q) = 1 <=> p | n_in
    short = [unit * k for k in (1, 2, 3) if unit * k < n_taps - 1] or [unit]
    if short[0] < n_taps - 1:
        ys = _chain(x[:, :unit * 6 * (FRAME[rate] // (unit * 6))], rate, short)
        assert np.abs(ys - y_ref[:, :ys.shape[1]]).max() <= 1e-9, f"{rate} Hz, messages of {short}: {np.abs(ys - y_ref[:, :ys.shape[1]]).max():.3e}"
    else:
        assert rate in (11025, 44100)                                       # p = 441 exceeds every bank here: no shorter message exists
    # rounded, the chained form holds the project's budget; the per-message zero-padded form does not
    got = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    assert (RR.excess(got, y_ref, A, n_taps) <= 0).all()
    bad = np.clip(np.rint(_per_message_zero_padded(x, rate, FRAME[rate])), -32768, 32767).astype(np.int16)
    over = RR.excess(bad[NOISE6000], y_ref[NOISE6000], A[NOISE6000], n_taps)
    assert (over > 0).any(), f"{rate} Hz: the budget admits per-message zero padding on the noise6000 row"
    first = FRAME[rate] * q // p
    assert (over[first:first + 4] > 0).any()                               # at the first message edge already


def test_ingest_numpy_refuses_a_fractional_message():
    with pytest.raises(ValueError):
        R.ingest_numpy(np.zeros(100, np.int16), 44100)
    y, h = R.ingest_numpy(np.zeros((3, 4), np.int16), 8000)
    assert y.shape == (3, 8) and h.shape == (3, R.design(8000)[2].shape[1] - 1)


ENTRIES = ("oww_ingest_configure", "oww_ingest", "oww_step_ingest")


def test_entries_declared_in_the_header_and_bound():
    with open(os.path.join(ROOT, "include", "owwhip.h")) as f:
        header = f.read()
    assert "#define OWW_ABI_VERSION 6" in header and "#define OWW_N_KERNEL_CLASSES 10" in header
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(oww_ctx\* h,", header, re.M), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"^const int16_t\* oww_ingest_dev\(const oww_ctx\* h\);", header, re.M)
    assert "oww_ingest_dev" in _lib.SYMBOLS
    for k, v in R.ENCODINGS.items():
        assert re.search(r"#define OWW_ENC_" + k.upper() + r"\s+" + str(v) + r"\b", header), k
    assert len(_lib.SYMBOLS["oww_ingest"][1]) == 8 and len(_lib.SYMBOLS["oww_step_ingest"][1]) == 8
    assert len(_lib.SYMBOLS["oww_ingest_configure"][1]) == 6
    assert _lib.ABI_VERSION == 6
