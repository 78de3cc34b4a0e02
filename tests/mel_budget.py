"""The level-aware error budget of the log-mel front end, its float64 reference and the signal regimes (helper module, no tests).

Both device forms (owk::mel_kernel, the mel phase of owf::hmelA_kernel) are compared with oracle.oww_oracle's float64 tables.  A flat
tolerance cannot work: the fp32 reference itself (the DFT-matrix recipe, oracle.oww_oracle.mel_stage in float32) is 2e-5 dB from
float64 on noise and 1.8 dB on a full-scale Nyquist alternation.  Its error grows with the distance D between a value and the energy
of its frame,

    R_f       = 10 log10(fbmax * sum_k P_k)        all 257 float64 power bins of frame f, fbmax = the largest filterbank weight
    u         = the unclamped float64 dB value     (u <= R_f always)
    budget_dB = T0 + T1 * 10^((D - 80) / 20),      D = R_pair - u >= 0

R_pair is the larger R_f of frames (2j, 2j + 1) in the KERNEL's frame numbering: both kernels transform such a pair as one complex
FFT (z = a + i b), so a quiet frame's spectrum carries round-off relative to its louder partner.  The pairs lie within each 8-frame
group of a call; a last odd frame's partner is cut from the zero-extended input, as the kernel does.  The budget comes from the
unclamped u and is applied to the clamped comparison (a value below the floor can only rise above it by its own error).  Streaming
rows are in mel units (dB / 10 + 2): a tenth of the dB budget.

T0 = 2e-4 dB is 5 x the device figure the project records (about 4e-6 mel units, tests/test_gpu_parity.py) and 10 x the bound the
db10 comment gives for the hardware-log2 form.  T1 = 4 x E32, where E32 is the fp32 REFERENCE's own envelope over REGIMES,
max (err - T0)+ * 10^((80 - D) / 20) with D to the value's own frame; the factor 4 covers another operation order (radix-8 FFT,
sincospif twiddles, a 1-ulp log2).  The margin is measured against the reference, never against the device:
tests/test_mel_budget_cpu.py re-measures E32 and holds the fp32 oracle to T0 + (T1 / 4) * ... for every regime."""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import oww_oracle as O

T0 = 2e-4                # dB
E32 = 1.5e-3             # dB: the fp32 oracle's envelope over REGIMES at 1,999 / 4,320 / 6,400 samples.  Measured 1.27e-3 on
                         # tone700_noise3 and 1.19e-3 on tone60; frozen with headroom, because the oracle's matrix products are
                         # the BLAS library's and another build of it sums the 512 terms in another order
T1 = 4 * E32             # dB
CHUNK, HIST, N_FFT, HOP = O.CHUNK, 480, O.N_FFT, O.HOP
N = 5 * CHUNK            # samples per regime
N_CLIP = 3 * CHUNK + HIST        # 4,320 samples = 24 frames: the clip-mode call, and the set E32 and the conditions are taken over
LEAKAGE = ("tone5000", "nyquist")    # no energy inside the 60-3800 Hz bank: every row is leakage, D > 100
SWITCH = 2700            # silence <-> noise
ONSET_ODD = 160 * 13 + 400       # the onset enters with the last 160 samples of clip frame 13 (streaming frames lie 3 later: even)
ONSET_EVEN = 160 * 12 + 400      # ... of clip frame 12 (streaming: odd)


def _i16(x):
    x = np.clip(np.round(np.asarray(x, dtype=np.float64)), -32768, 32767).astype(np.int16)
    assert x.shape == (N,)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def regimes():
    """name -> int16 [N], read-only, from one fixed seeded generator (dict order is the regime order everywhere)."""
    r = np.random.default_rng(20261018)
    n = np.arange(N)
    t = n / O.SR
    tone = lambda hz, amp: amp * np.sin(2 * np.pi * hz * t)
    loud = r.normal(0, 12000, N)
    quiet_tone = tone(440.0, 40)
    out = {
        "noise30": r.normal(0, 30, N),
        "noise3000": r.normal(0, 3000, N),
        "noise12000": r.normal(0, 12000, N),
        "uniform_fs": r.integers(-32768, 32768, N),
        "lsb": r.integers(-1, 2, N),
        "zeros": np.zeros(N),
        "last_one": np.where(n == N_CLIP - 1, 1, 0),                 # the last sample of the 4,320-sample call
        "dc_pos": np.full(N, 32767),
        "dc_neg": np.full(N, -32768),
        "dc_one": np.full(N, 1),
        "nyquist": np.where(n % 2, -32768, 32767),
        "square16": np.where((n // 8) % 2, -32768, 32767),           # period 16 samples
        "tone1000": tone(1000.0, 30000),                             # bin 32 exactly
        "tone1017": tone(1017.3, 30000),
        "tone60": tone(60.0, 30000),
        "tone3800": tone(3800.0, 30000),
        "tone5000": tone(5000.0, 30000),
        "tone440_quiet": quiet_tone,
        "tone700_noise3": tone(700.0, 30000) + r.normal(0, 3, N),
        "impulse": np.where(n == 1000, 32767, 0),
        "impulse_train": np.where(n % 160 == 37, 32767, 0),
        "chirp": 30000 * np.sin(2 * np.pi * (50.0 * t + 0.5 * (4000.0 - 50.0) / (N / O.SR) * t * t)),
        "step": np.where(n < 1500, -20000, 20000),
        "silence_noise": np.where(n < SWITCH, 0, loud),
        "noise_silence": np.where(n < SWITCH, loud, 0),
        "onset_odd": np.where(n < ONSET_ODD, quiet_tone, loud),
        "onset_even": np.where(n < ONSET_EVEN, quiet_tone, loud),
    }
    return {k: _i16(v) for k, v in out.items()}


REGIMES = tuple(regimes())


class Ref(NamedTuple):
    clamped: np.ndarray      # [B, F, 32] float64, clamped at the floor (dB; mel units for streaming calls, masked rows 1.0)
    u: np.ndarray            # [B, F, 32] float64 dB, unclamped
    budget: np.ndarray       # [B, F, 32] allowed |device - clamped| in the units of `clamped` (0 for masked rows)
    R: np.ndarray            # [B, F] float64 dB, R_pair of every frame
    floor: np.ndarray        # [B] dB


def _unclamped(x, n_frames):
    """int16 [B, n] -> (u [B, F, 32], R_f [B, F2]) in float64, F2 = n_frames rounded up to even, the input zero-extended for it."""
    t = O._tables(np.float64)
    F2 = n_frames + (n_frames & 1)
    need = (F2 - 1) * HOP + N_FFT
    x = np.asarray(x, dtype=np.float64)
    if x.shape[1] < need:
        x = np.pad(x, ((0, 0), (0, need - x.shape[1])))
    idx = (np.arange(F2) * HOP)[:, None] + np.arange(N_FFT)[None, :]
    frames = x[:, idx]
    re, im = frames @ t.re, frames @ t.im
    power = re * re + im * im
    u = 10.0 * np.log10(np.maximum(power @ t.fb, O.AMIN))
    R = 10.0 * np.log10(np.maximum(t.fb.max() * power.sum(axis=2), O.AMIN))
    return u[:, :n_frames], R


def reference(x, n_frames: Optional[int] = None, per_clip: bool = False, masked: int = 0, floor_max=None) -> Ref:
    """The float64 rows and budget (dB) of ONE kernel call whose frames are cut from int16 x [B, n] ([n] = one row): a clip-mode
    call (x = the PCM), or a streaming call (x = 480-sample tail ++ PCM).  The floor is max - 80 dB over the whole call (per row
    with per_clip), the first `masked` frames excluded; floor_max [B] overrides the maximum (a slice of a longer call)."""
    x = np.atleast_2d(np.asarray(x))
    assert x.dtype == np.int16
    if n_frames is None:
        n_frames = O.n_mel_frames(x.shape[1])
    u, Rf = _unclamped(x, n_frames)
    R = np.repeat(np.maximum(Rf[:, 0::2], Rf[:, 1::2]), 2, axis=1)[:, :n_frames]
    if floor_max is None:
        floor_max = u[:, masked:].max(axis=(1, 2))
        if not per_clip:
            floor_max = np.full_like(floor_max, floor_max.max())
    floor = np.asarray(floor_max, dtype=np.float64) - O.TOP_DB
    D = np.maximum(R[:, :, None] - u, 0.0)
    budget = T0 + T1 * 10.0 ** ((D - 80.0) / 20.0)
    return Ref(np.maximum(u, floor[:, None, None]), u, budget, R, floor)


def stream_reference(x, calls) -> list:
    """One stream after a reset, fed int16 x [n] in calls of `calls` chunks each -> one Ref per call in mel units (dB / 10 + 2), rows
    as oww_get_mel orders them.  The first call masks its first three frames (they read 1.0 and are excluded from the floor)."""
    x = np.asarray(x)
    tail, pos, out = np.zeros(HIST, np.int16), 0, []
    for i, k in enumerate(calls):
        pcm = x[pos:pos + k * CHUNK]
        assert pcm.size == k * CHUNK
        pos += k * CHUNK
        masked = 3 if i == 0 else 0
        ref = reference(np.concatenate([tail, pcm]), 8 * k, masked=masked)
        clamped, budget = ref.clamped / 10.0 + 2.0, ref.budget / 10.0
        clamped[:, :masked], budget[:, :masked] = 1.0, 0.0
        out.append(Ref(clamped, ref.u, budget, ref.R, ref.floor))
        tail = pcm[-HIST:]
    return out


def worst_ratio(got, ref: Ref):
    """max |got - clamped| / budget over one call (masked rows: 0 when they read exactly 1.0, inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref.clamped)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ref.budget > 0, err / ref.budget, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max())
