"""Float64 reference, error budget and case table for the device resampler (`resample_kernel` / `oww_resample`).

Shared by tests/test_resample_budget_cpu.py (CPU tier: pins the design, admits every case, shows the budget rejects wrong kernels)
and tests/test_resample_edges.py (GPU tier).  Nothing here imports `openwakeword_amd.resample.apply_numpy` or copies its index
arithmetic: `ref64` is written from the definition in include/owwhip.h,

    out[s][j] = sat_int16(rint(sum_k taps[(j p) % q][k] * in[s][(j p) / q + k - n_taps / 2 + 1])),   samples outside the message = 0,

for any bank [q][n_taps], and `independent_taps` restates the Kaiser-windowed sinc of resample.py's module docstring with its own
Bessel series and its own sinc.

The budget.  The kernel is a k-ordered fp32 `fmaf` chain over ntp = n_taps rounded up to 4 terms (the padded terms are exact zeros),
started at 0.  int16 samples and float32 taps are exact operands, so the only roundings are the ntp roundings of the chain, and the
standard bound for recursive summation holds with A = sum_k |taps * x|:

    |acc32 - y64| <= gamma * A,     gamma = ntp * u / (1 - ntp * u),     u = 2^-24.

rint moves the value by at most 0.5 and the clamp is 1-Lipschitz, so ONE assertion covers every output, saturated ones included:

    |got - clip(y64, -32768, 32767)| <= 0.5 + gamma * A + 1e-9          per output sample

(1e-9 absorbs the float64 reference's own rounding where A is small; where A is large that rounding, n_taps * 2^-53 * A, is 2^-29
of gamma * A).  There is no mismatch-share cap and no measured constant.  At full scale A is about 1.5 * 32768, so gamma * A stays
below 0.55 LSB for rates up to 96 kHz (154 taps); at 192 and 384 kHz (306 and 610 taps) it reaches 1.1 and 2.1 LSB.  That is what an fp32 chain of that length
allows, not a slack: a kernel that wanted less would have to accumulate in pairs or in higher precision.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24
ROWS = 37                      # stream count of the GPU tier's engine

# (rate Hz, n_in): the geometries of the GPU tier.  `launch_geometry` says which branch each one is here for
# (test_resample_budget_cpu.py::test_case_table_covers_every_branch holds the table to that list).
CASES = (
    (8000, 3),          # n_out 6 < 256; p < q; ntp = n_taps + 2
    (8000, 640),        # one whole chunk out, one workgroup
    (11025, 1000),      # n_out 1451: 2 workgroups, fractional j0 * p / q, n_out % 256 != 0
    (12000, 2880),      # p / q = 3 / 4, n_out 3840 = 3 * opb
    (22050, 1764),      # ntp = n_taps = 36
    (24000, 3847),      # ntp = n_taps = 40, n_out 2564: 3 workgroups, the last one 4 outputs
    (32000, 2562),      # q = 1, n_out 1281: the second workgroup produces one output
    (44100, 7056),      # n_out 2560 = 2 * opb
    (48000, 11520),     # q = 1, 3 workgroups
    (88200, 14112),     # p / q = 441 / 80, 140 taps
    (96000, 7680),      # q = 1, 154 taps
    (192000, 30720),    # opb reduced to 768, 4 workgroups
    (384000, 30720),    # opb reduced to 256, 5 workgroups
    (16001, 1300),      # 1.79 MB bank: taps read from global memory, 2 workgroups
    (15999, 2600),      # the same with p < q, 3 workgroups
)


def gamma(n_taps: int) -> float:
    ntp = (int(n_taps) + 3) // 4 * 4
    return ntp * U32 / (1.0 - ntp * U32)


def ratio(rate: int, rate_out: int = 16000):
    r = Fraction(int(rate), int(rate_out))
    return r.numerator, r.denominator


# ---- the definition of include/owwhip.h in float64 --------------------------------------------------------------------------------
def ref64(x, p: int, q: int, taps):
    """x int16 [..., n_in], taps float [q][n_taps] -> (y64, A), both float64 [..., n_in * q // p]: the unrounded sum of the header's
    definition and A = sum_k |taps * x|.  One pass per tap over a zero-extended copy of the message (a strided gather)."""
    x = np.asarray(x)
    taps = np.asarray(taps)
    assert taps.ndim == 2 and taps.shape[0] == q and taps.shape[1] % 2 == 0
    n_in, n_taps = x.shape[-1], taps.shape[1]
    n_out = (n_in * q) // p
    t64 = taps.astype(np.float64)
    ext = np.zeros(x.shape[:-1] + (n_in + 2 * n_taps,), np.float64)           # "samples outside the message = 0"
    ext[..., n_taps:n_taps + n_in] = x
    jp = np.arange(n_out, dtype=np.int64) * p
    first = jp // q - n_taps // 2 + 1 + n_taps                                 # position of tap 0's sample in ext
    row = jp % q
    y = np.zeros(x.shape[:-1] + (n_out,), np.float64)
    A = np.zeros_like(y)
    for k in range(n_taps):
        term = t64[row, k] * ext[..., first + k]
        y += term
        A += np.abs(term)
    return y, A


def budget(A, n_taps: int):
    return 0.5 + gamma(n_taps) * A + 1e-9


def excess(got, y64, A, n_taps: int):
    """|got - clip(y64)| - budget per output: <= 0 everywhere is THE assertion."""
    return np.abs(np.asarray(got, np.float64) - np.clip(y64, -32768.0, 32767.0)) - budget(A, n_taps)


def worst_ratio(got, y64, A, n_taps: int) -> float:
    """max (|got - clip(y64)| - 0.5)+ / (gamma * A): how much of the chain's allowance the worst output used (reported, never
    asserted; the rounding's own 0.5 is taken off first, so 0 means "explained by rint alone")."""
    err = np.abs(np.asarray(got, np.float64) - np.clip(y64, -32768.0, 32767.0)) - 0.5
    ga = gamma(n_taps) * A
    ok = ga > 0
    return float(np.max(np.where(ok, np.maximum(err, 0.0) / np.where(ok, ga, 1.0), 0.0))) if err.size else 0.0


# ---- host launch arithmetic, restated -----------------------------------------------------------------------------------------------
RS_NT = 256


def launch_geometry(n_in: int, p: int, q: int, n_taps: int) -> dict:
    """Python mirror of the opb / span / taps_in_lds / refusal arithmetic of `oww_resample`.

    A COVERAGE GUARD FOR THE CASE TABLE ONLY: it answers "which branch does this case reach", so that a case is in the table for a
    stated reason.  It is not a check of the library -- if the host code changes, this mirror is what has to follow."""
    n_out = (n_in * q) // p
    ntp = (n_taps + 3) // 4 * 4

    def span_of(o):
        return ((o - 1) * p) // q + 1 + n_taps + 4

    opb = RS_NT * 5
    while opb > RS_NT and span_of(opb) * 4 > 48 * 1024:
        opb -= RS_NT
    opb_rate = opb
    opb = min(opb, (n_out + RS_NT - 1) // RS_NT * RS_NT)
    span = span_of(opb)
    lds_x = (span + 3) // 4 * 4 * 4
    lds_t = q * ntp * 4
    n_wg = (n_out + opb - 1) // opb if opb > 0 else 0
    frac = any((w * opb * p) % q for w in range(1, n_wg))
    return dict(n_out=n_out, ntp=ntp, opb=opb, opb_rate=opb_rate, span=span, lds_x=lds_x, lds_t=lds_t, refused=lds_x > 96 * 1024,
                taps_in_lds=int(lds_x + lds_t <= 150 * 1024), n_wg=n_wg, fractional_start=frac)


# ---- the filter of resample.py's docstring, a second time -------------------------------------------------------------------------
ZC, BETA, ROLLOFF = 12, 8.0, 0.945


def _bessel_i0(x):
    """I0 by its power series, sum_m ((x / 2)^m / m!)^2; x <= 8 here, the terms fall below 1e-17 of the sum by m = 32."""
    h = np.asarray(x, np.float64) / 2.0
    term = np.ones_like(h)
    tot = np.ones_like(h)
    for m in range(1, 40):
        term = term * h / m
        tot = tot + term * term
    return tot


@functools.lru_cache(maxsize=None)
def independent_taps(rate: int):
    """(p, q, taps float64 [q][2 * half]) of the docstring's formula: taps[phase, k] = window(d / (ZC * s)) * sinc(d / s) / s with
    d = k - half + 1 - phase / q, s = max(1, rate / 16000) / ROLLOFF, a Kaiser(beta = 8) window of ZC = 12 zero crossings a side,
    every phase normalised to unit DC gain."""
    p, q = ratio(rate)
    s = max(1.0, rate / 16000.0) / ROLLOFF
    half = int(math.ceil(ZC * s))
    out = np.zeros((q, 2 * half), np.float64)
    i0b = float(_bessel_i0(BETA))
    for k in range(2 * half):
        d = (k - half + 1) - np.arange(q, dtype=np.float64) / q
        u = d / (ZC * s)
        inside = np.abs(u) < 1.0
        win = np.where(inside, _bessel_i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / i0b, 0.0)
        a = math.pi * d / s
        snc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
        out[:, k] = win * snc / s
    out /= np.array([math.fsum(r) for r in out])[:, None]
    out.setflags(write=False)
    return p, q, out


# ---- signals ------------------------------------------------------------------------------------------------------------------------
SIGNALS = ("silence", "dc_pos", "dc_neg", "alt6", "uniform_fs", "noise6000", "noise30", "square_edge", "impulse_first", "impulse_last")


@functools.lru_cache(maxsize=None)
def signals(rate: int, n_in: int, rows: int = ROWS) -> np.ndarray:
    """int16 [rows, n_in], read-only, fixed by (rate, n_in): the ten named rows of SIGNALS, then further seeds of the three noises and
    other phases of the square wave in turn."""
    rng = np.random.default_rng([rate, n_in])
    t = np.arange(n_in)
    f_edge = 0.9 * ROLLOFF * 0.5 * min(rate, 16000)                           # just inside the pass band: the ringing stays in the output
    x = np.zeros((rows, n_in), np.int16)
    for r in range(rows):
        kind = SIGNALS[r] if r < len(SIGNALS) else ("uniform_fs", "noise6000", "noise30", "square_edge")[r % 4]
        if kind == "dc_pos":
            x[r] = 32767
        elif kind == "dc_neg":
            x[r] = -32768
        elif kind == "alt6":                                                   # three samples up, three down: mean -0.5
            x[r] = np.where((t // 3) % 2 == 0, 32767, -32768)
        elif kind == "uniform_fs":
            x[r] = rng.integers(-32768, 32768, n_in)
        elif kind == "noise6000":
            x[r] = np.clip(np.rint(rng.standard_normal(n_in) * 6000.0), -32768, 32767)
        elif kind == "noise30":
            x[r] = np.rint(rng.standard_normal(n_in) * 30.0)
        elif kind == "square_edge":
            x[r] = np.where(np.sin(2 * np.pi * f_edge * t / rate + 0.3 + 0.7 * r) >= 0, 32767, -32768)
        elif kind == "impulse_first":
            x[r, 0] = 32767
        elif kind == "impulse_last":
            x[r, n_in - 1] = -32768
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case_reference(rate: int, n_in: int, rows: int = ROWS):
    """(p, q, taps float32 of resample.design, x, y64, A) of one case, computed once and shared (all read-only)."""
    from openwakeword_amd import resample as R
    p, q, taps = R.design(rate)
    x = signals(rate, n_in, rows)
    y, A = ref64(x, p, q, taps)
    y.setflags(write=False)
    A.setflags(write=False)
    return p, q, taps, x, y, A


def saturated(y64) -> np.ndarray:
    """Outputs whose value the clamp changes (beyond the int16 range by more than the rounding)."""
    return (y64 > 32767.5) | (y64 < -32768.5)


def near_tie(y64, A, n_taps: int) -> np.ndarray:
    """Outputs within gamma * A of a rounding tie: the chain's error may legitimately decide which way they round."""
    return np.abs(y64 - np.floor(y64) - 0.5) <= gamma(n_taps) * A


# ---- the fp32 chain on the CPU, and five ways to get it wrong ---------------------------------------------------------------------
VARIANTS = ("phase_plus_one", "window_shift", "row_stride_n_taps", "edge_clamp", "truncate")


def emulate32(x, p: int, q: int, taps, variant: str = "") -> np.ndarray:
    """numpy emulation of the kernel's chain: acc = float32(acc + w * x) term by term in k order over the padded row (the sum formed
    in float64, then rounded to float32: the product of a float32 and an int16 is exact there), rint, clamp -> int16.
    `variant` names one deliberate defect (VARIANTS); "" is the kernel as documented."""
    assert variant in ("",) + VARIANTS
    x = np.asarray(x)
    taps = np.asarray(taps, np.float32)
    n_in, n_taps = x.shape[-1], taps.shape[1]
    ntp = (n_taps + 3) // 4 * 4
    n_out = (n_in * q) // p
    bank = np.zeros((q, ntp), np.float64)
    bank[:, :n_taps] = taps
    flat = np.concatenate([bank.ravel(), np.zeros(ntp)])
    jp = np.arange(n_out, dtype=np.int64) * p
    row = (jp + 1) % q if variant == "phase_plus_one" else jp % q
    w0 = row * (n_taps if variant == "row_stride_n_taps" else ntp)
    first = jp // q - n_taps // 2 + 1 + (1 if variant == "window_shift" else 0)
    xf = x.astype(np.float64)
    acc = np.zeros(x.shape[:-1] + (n_out,), np.float32)
    for k in range(ntp):
        g = first + k
        inside = (g >= 0) & (g < n_in)
        v = xf[..., np.clip(g, 0, n_in - 1)]
        if variant != "edge_clamp":
            v = np.where(inside, v, 0.0)
        acc = (acc.astype(np.float64) + flat[w0 + k] * v).astype(np.float32)
    r = np.trunc(acc) if variant == "truncate" else np.rint(acc)
    return np.clip(r, -32768, 32767).astype(np.int16)
