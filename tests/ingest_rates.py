"""Case table, coverage guard, float64 reference and fp32 emulation for the stateful stream ingest (`ingest_stream<ENC>` behind
`ingest_kernel` and `ingest_mixed_kernel`; host arithmetic in openwakeword_amd/csrc/owwhip_ingest.h) at every rate and class table the
server serves.  HIP-free and shared by tests/test_ingest_rates_cpu.py (CPU tier: the table reaches every branch, a correct fp32 chain
holds the budget at the new rates, six wrong kernels do not) and tests/test_ingest_rates_gpu.py (device tier).

The definition is include/owwhip.h's: with X every decoded sample of the stream since its reset,
    out[J] = sat_int16(rint(sum_k taps[(J p) % q][k] * X[(J p) / q + k - (n_taps - 1)])),   X[i] = 0 for i < 0,
which is `RR.ref64` on zeros(n_taps / 2) | X.  The only tolerances are tests/resample_ref.py's derived `0.5 + gamma * A` per output
sample (`RR.excess <= 0`) and bit equality."""
from __future__ import annotations

import functools

import numpy as np

import resample_ref as RR
from openwakeword_amd import resample as R
from openwakeword_amd.serve import RATES

S = RR.ROWS
N_MSG, N_OUT = 6, 1280                     # six 80 ms frames per recording
TOTAL = N_MSG * N_OUT
IG_TILE = 2048                             # owk::IG_TILE = owi::kTile
LDS_STAGE, LDS_WITH_TAPS = 96 * 1024, 150 * 1024          # owi::kLdsStage, owi::kLdsWithTaps
# the staging edge at the longest served history (96 kHz, H = 153): the largest whole message that stages and the first that does not,
# as tests/ingest_rates_check.cpp prints them from owwhip_ingest.h (the CPU tier holds these two numbers to that program)
EDGE96 = (24408, 24414)

# every class of the server's default table, then the sliding form (p = 1) at q = 4 and q = 8, which resample.design reaches at 4 and 2 kHz
CLASSES = tuple((rate, "pcm16") for rate in RATES) + ((8000, "ulaw"), (8000, "alaw")) + ((4000, "pcm16"), (2000, "pcm16"), (4000, "ulaw"))


def params(rate: int, enc: str):
    """(p, q, taps or None, n_taps) of resample.class_params"""
    return R.class_params(rate, enc)


def frame(rate: int) -> int:
    """input samples of one 80 ms frame"""
    return R.class_n_in(rate, N_OUT)


def unit(rate: int, enc: str) -> int:
    """the class's smallest legal message: the least n_in with n_in * q % p == 0 (p / q is in lowest terms)"""
    return params(rate, enc)[0]


def server_default_classes():
    """the class list `serve.FanInServer(ingest="device")` builds when it is given no table: asked of the server itself, on a model
    that only records what it is configured with"""
    from openwakeword_amd import serve

    class _Engine:
        def pinned_empty(self, shape, dtype=np.int16):
            return np.zeros(shape, dtype)

        def submit_ingest_mixed(self, rows, on):
            raise AssertionError("nothing is submitted here")

    class _Model:
        n_streams, labels, engine, configured = 2, ["a"], _Engine(), None

        def configure_ingest_classes(self, formats):
            self.configured = list(formats)

    m = _Model()
    srv = serve.FanInServer(m, ingest="device")
    assert m.configured == srv.classes
    return [(int(r), str(e)) for r, e in srv.classes]


# ---- the launch arithmetic, restated ------------------------------------------------------------------------------------------------
def geometry_n_in(rate: int, enc: str, n_in: int) -> dict:
    """Python mirror of owwhip_ingest.h::class_geometry, the table row (ntp, Hpad, slide) and the launch flags for one message of n_in
    input samples.

    A COVERAGE GUARD FOR THE CASE TABLE ONLY, like RR.launch_geometry: it answers "which branch does this case reach", so that a case
    is in the table for a stated reason.  It is not a check of the library (tests/ingest_rates_check.cpp prints the library's own
    numbers and the CPU tier holds this mirror to them) -- if the host code changes, this mirror is what has to follow."""
    p, q, _, n_taps = params(rate, enc)
    assert n_in >= 1 and (n_in * q) % p == 0, f"{rate} Hz: {n_in} samples are no whole number of outputs"
    n_out = n_in * q // p
    ntp = (n_taps + 3) // 4 * 4
    H = n_taps - 1 if n_taps else 0
    Hoff = (H + 3) // 4 * 4
    xs_len = (Hoff + n_in + 8 + 3) // 4 * 4
    stage = xs_len * 4
    lds_bare = stage + IG_TILE * 2
    lds_with_taps = lds_bare + q * ntp * 4
    n_bytes = n_in * (2 if enc == "pcm16" else 1)
    return dict(n_in=n_in, n_out=n_out, p=p, q=q, n_taps=n_taps, ntp=ntp, H=H, Hpad=(H + 7) // 8 * 8 if n_taps else 0, x0=Hoff - H,
                slide=int(bool(n_taps) and p == 1 and q in (1, 2, 4, 8)), ntp_is_n_taps=bool(n_taps) and ntp == n_taps,
                vec_in=n_bytes % 16 == 0, vec_out=n_out % 8 == 0, xs_len=xs_len, stage=stage, refused=stage > LDS_STAGE,
                lds_bare=lds_bare, lds_with_taps=lds_with_taps, taps_in_lds=int(bool(n_taps) and lds_with_taps <= LDS_WITH_TAPS),
                n_tiles=(n_out + IG_TILE - 1) // IG_TILE, short=n_in < H)


def geometry(rate: int, enc: str, n_out: int = N_OUT) -> dict:
    """`geometry_n_in` for the message that produces n_out outputs (a coverage guard for the table only, see there)"""
    p, q, _, _ = params(rate, enc)
    assert (n_out * p) % q == 0
    return geometry_n_in(rate, enc, n_out * p // q)


# ---- the cuts the device tier feeds ---------------------------------------------------------------------------------------------------
def _plans(rate: int, enc: str) -> dict:
    """name -> message sizes in input samples, in the order they are fed; every plan is a prefix of the six-frame recording"""
    F, u, total = frame(rate), unit(rate, enc), frame(rate) * N_MSG
    p, q, _, n_taps = params(rate, enc)
    H = n_taps - 1 if n_taps else 0
    plans = {"six": [F] * N_MSG}
    k = next(k for k in (6, 3, 2, 1) if not geometry_n_in(rate, enc, k * F)["refused"])      # the largest whole-frame message that stages
    plans["whole"] = [k * F] * (N_MSG // k)
    if k > 2 and not geometry_n_in(rate, enc, 2 * F)["refused"]:
        plans["two_frames"] = [2 * F] * 3                                                     # two tiles at every rate
    assert F % 2 == 0 and (F // 2 * q) % p == 0
    plans["half"] = [F // 2] * (2 * N_MSG)
    left = total // u                                                                         # (12 units in all at 11.025 kHz)
    plans["tiny"] = [u] * min(16, left // 2)
    left -= len(plans["tiny"])
    for m in (3, 1, 2, 5, 1, 7):
        if m <= left:
            plans["tiny"].append(m * u)
            left -= m
    if H >= 77 and u < H:                                                                     # the old history moves down
        m = (H - 1) // u                                                                      # the most units below H
        plans["short_history"] = [u, m * u, 2 * u, (m - 1) * u, m // 2 * u, u, m * u, 3 * u, F, u, m * u]
        assert max(n for n in plans["short_history"] if n != F) < H
    if p == 1 and q in (4, 8):                                                                # groups of four positions straddle a tile edge
        plans["tile_edge"] = [2 * F, 3 * F, F]
    for name, sizes in plans.items():
        assert sum(sizes) <= total and all(n >= 1 and (n * q) % p == 0 for n in sizes), (rate, enc, name)
    return plans


MESSAGE_PLANS = {c: _plans(*c) for c in CLASSES}


# ---- recordings and the float64 reference ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def codes_for(n: int, seed: int = 0) -> np.ndarray:
    """uint8 [S, n]: rows 0..3 the constant codes 0x00, 0xFF, 0x7F, 0x55, every other row uniform random codes (as
    tests/test_ingest_gpu.py::codes_for)."""
    c = np.random.default_rng([711, n, seed]).integers(0, 256, (S, n)).astype(np.uint8)
    for r, v in enumerate((0x00, 0xFF, 0x7F, 0x55)):
        c[r] = v
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def recording(rate: int, enc: str):
    """(what is fed [S, 6 frames], its decoded int16), read-only: RR.signals for PCM16 (DC at both rails, alt6, full-scale uniform, the
    band-edge square wave, first and last impulses, ...), the codes of `codes_for` for G.711"""
    n = frame(rate) * N_MSG
    fed = RR.signals(rate, n) if enc == "pcm16" else codes_for(n, seed=rate)
    dec = R.decode(fed, enc)
    dec.setflags(write=False)
    return fed, dec


@functools.lru_cache(maxsize=None)
def reference(rate: int, enc: str):
    """(prefixed recording, y64, A) of the definition: RR.ref64 on zeros(n_taps // 2) | decoded whole, cut to the outputs the stream has
    produced.  Decode only (16 kHz): the decoded recording itself with A = 0."""
    p, q, taps, n_taps = params(rate, enc)
    _, dec = recording(rate, enc)
    if not n_taps:
        y = dec.astype(np.float64)
        out = (dec, y, np.zeros_like(y))
    else:
        pre = np.concatenate([np.zeros((S, n_taps // 2), np.int16), dec], axis=1)
        y, A = RR.ref64(pre, p, q, taps)
        n = dec.shape[1] * q // p
        out = (pre, y[:, :n], A[:, :n])
    for a in out:
        a.setflags(write=False)
    return out


def holds_budget(got, rate: int, enc: str, rows=None):
    """RR.excess of `got` (a prefix of the recording's outputs; `rows` picks streams) against the definition -> (excess, worst ratio)"""
    _, y, A = reference(rate, enc)
    n_taps = params(rate, enc)[3]
    rows = slice(None) if rows is None else rows
    y, A = y[rows, :got.shape[1]], A[rows, :got.shape[1]]
    return RR.excess(got, y, A, n_taps), RR.worst_ratio(got, y, A, n_taps)


# ---- the kernel's chain on the CPU, and six ways to get the stream wrong --------------------------------------------------------------
MUTATIONS = ("history_dropped", "history_shifted", "phase_plus_one", "last_tap_skipped", "tile_edge_group", "history_not_moved_down")


def emulate(rate: int, enc: str, sizes, mutation: str = "") -> np.ndarray:
    """numpy float32 emulation of `ingest_stream` over the recording's messages `sizes`: per message X = history | message, every output
    the k-ordered chain acc = float32(acc + w * x) from 0 over the ntp terms of the padded row (the sum formed in float64, then rounded:
    the product of a float32 and an int16 is exact there), rint, clamp; the history goes from message to message as int16.
    `mutation` names one deliberate defect (MUTATIONS); "" is the kernel as documented.  -> int16 [S, outputs of the messages]"""
    assert mutation in ("",) + MUTATIONS
    p, q, taps, n_taps = params(rate, enc)
    _, dec = recording(rate, enc)
    if not n_taps:
        return dec[:, :sum(sizes)].copy()
    ntp, H = (n_taps + 3) // 4 * 4, n_taps - 1
    bank = np.zeros((q, ntp), np.float64)
    bank[:, :n_taps] = taps
    n_terms = ntp - 1 if (mutation == "last_tap_skipped" and ntp == n_taps) else ntp      # (a row without padding: k < ntp - 1 loses a real tap)
    Hoff = (H + 3) // 4 * 4
    x0 = Hoff - H
    hist = np.zeros((S, H), np.int16)
    outs, at = [], 0
    for m, n_in in enumerate(sizes):
        msg = dec[:, at:at + n_in]
        at += n_in
        used = hist
        if mutation == "history_dropped" and m == 1:
            used = np.zeros_like(hist)
        elif mutation == "history_shifted":
            used = np.concatenate([hist[:, 1:], np.zeros((S, 1), np.int16)], axis=1)
        X = np.concatenate([used, msg, np.zeros((S, ntp + 8), np.int16)], axis=1).astype(np.float64)
        n_out = n_in * q // p
        jp = np.arange(n_out, dtype=np.int64) * p
        pos, row = jp // q, ((jp + 1) % q if mutation == "phase_plus_one" else jp % q)
        acc = np.zeros((S, n_out), np.float32)
        for k in range(n_terms):
            acc = (acc.astype(np.float64) + bank[row, k] * X[:, pos + k]).astype(np.float32)
        y = np.clip(np.rint(acc), -32768, 32767).astype(np.int16)
        if mutation == "tile_edge_group" and p == 1 and q in (1, 2, 4, 8):
            # a group of four positions that straddles a tile edge is left to the earlier tile: the later tile's positions before its
            # first whole group keep what the staging tile held at their place (the earlier tile's outputs)
            tp = IG_TILE // q
            for pos0 in range(tp, n_in, tp):
                first_whole = (pos0 + x0 + 3) // 4 * 4 - x0
                for ps in range(pos0, min(first_whole, n_in)):
                    y[:, ps * q:(ps + 1) * q] = y[:, (ps - tp) * q:(ps - tp + 1) * q]
        outs.append(y)
        new = np.concatenate([hist, msg], axis=1)[:, n_in:n_in + H] if n_in < H else msg[:, n_in - H:]
        if mutation == "history_not_moved_down" and n_in < H:
            new = np.concatenate([hist[:, :H - n_in], msg], axis=1)
        hist = np.ascontiguousarray(new, dtype=np.int16)
    return np.concatenate(outs, axis=1)
