"""The clips, lengths and float64 references of the bulk clip-embedding path (helper module, no tests, no GPU).

oww_embed_clips / oww_embed (openwakeword_amd/csrc/owwhip.hip) are compared in two stages, each with the budget the project already
has: the clip-mode mel rows against tests/mel_budget.py, and the window walk + CNN against tests/cnn_budget.py on the DEVICE'S OWN
mel rows.  No tolerance is defined here; tests/test_clip_budget_cpu.py shows that both budgets admit these clips at clip length.

Clips are int16 rows of N = 35,072 samples from one seeded generator, cut to the case's length with clips(n): the first n samples,
except that loud_tail keeps its loud part in the LAST 1,000 samples of the cut (the clip is built for that length).  ORDER is the
mixed batch: square_fs stands directly before zeros, and directly before lsb in the reversed batch, so the loudest clip's last four
mel rows are the lead-in rows the walk reads in front of the two quietest clips."""
import functools

import numpy as np

import mel_budget as MB
from oracle import oww_oracle as O

SEED = 20261019
N = 35072                                   # samples per clip: 217 frames, 18 windows
LOUD = 1000                                 # samples of the loud part of loud_tail / loud_head
ORDER = ("noise3000", "speechlike", "loud_head", "lsb", "square_fs", "zeros", "loud_tail")
# n -> (F frames, windows)
LENGTHS = {12512: (76, 1),                  # the minimum
           12671: (76, 1),                  # 159 samples unused
           12672: (77, 1),                  # odd F: the last FFT pair is half empty
           13632: (83, 1),                  # 7 rows unused
           13792: (84, 2),
           35072: (217, 18)}                # 5 rows unused; more windows than the 16 feature-ring rows
N_MIN, N_TWO, N_LONG = 12512, 13792, 35072
SHIFT_CLIPS = ("noise3000", "lsb", "speechlike")        # the clips of the off-by-one-row condition
FLOOR_BATCH = ("square_fs", "lsb", "zeros", "loud_tail")


def n_frames(n):
    return (n - O.N_FFT) // O.HOP + 1


def n_windows(F):
    return (F - O.MEL_WINDOW) // O.MEL_HOP + 1


@functools.lru_cache(maxsize=None)
def _parts():
    r = np.random.default_rng(SEED)
    k = np.arange(N)
    t = k / O.SR
    fm = 2.0 * np.pi * (200.0 * t - (40.0 / (2.0 * np.pi * 2.5)) * np.cos(2.0 * np.pi * 2.5 * t))     # 200 +- 40 Hz, 2.5 Hz vibrato
    return {
        "noise3000": r.normal(0, 3000, N),
        # fifteen harmonics at 1 / h, 4 Hz tremolo.  (The fundamental alone at 6,000 left the fp32 oracle's mel envelope at 35,072
        # samples -- 1.06 x, a lone tone 57 dB above its skirts -- and was replaced by the harmonic stack; the envelope stays.)
        "speechlike": 4000.0 * (0.55 + 0.45 * np.sin(2.0 * np.pi * 4.0 * t)) * sum(np.sin(h * fm) / h for h in range(1, 16))
                      + r.normal(0, 50, N),
        "lsb": r.integers(-1, 2, N),
        "zeros": np.zeros(N),
        "square_fs": np.where((k // 8) % 2, -32768, 32767),
        "tone": 40.0 * np.sin(2.0 * np.pi * 440.0 * t),
        "loud": r.normal(0, 12000, LOUD),
    }


def _i16(x):
    x = np.clip(np.round(np.asarray(x, dtype=np.float64)), -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def clip(name, n=N):
    """int16 [n], read-only."""
    assert 0 < n <= N
    p = _parts()
    if name in ("loud_tail", "loud_head"):
        x = p["tone"][:n].copy()
        if name == "loud_tail":
            x[n - LOUD:] = p["loud"]
        else:
            x[:LOUD] = p["loud"][::-1]
        return _i16(x)
    return _i16(p[name][:n])


@functools.lru_cache(maxsize=None)
def clips(n=N, names=ORDER):
    """int16 [len(names), n], read-only: the mixed batch (or the named clips) at one length."""
    x = np.stack([clip(name, n) for name in names])
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------------------------- references
def mel_ref(x) -> MB.Ref:
    """The float64 dB rows and the level-aware budget of one clip-mode call, one floor per clip."""
    return MB.reference(x, per_clip=True)


def windows(spec):
    """The walk of the reference (utils.py:229-236): rows [F, 32] -> [n_windows, 76, 32], a window every 8 rows while 76 rows remain."""
    spec = np.asarray(spec)
    return np.stack([spec[i:i + O.MEL_WINDOW] for i in range(0, spec.shape[0], O.MEL_HOP) if spec[i:i + O.MEL_WINDOW].shape[0] == O.MEL_WINDOW])


def cnn64(rows, emb):
    """Windows [W, 76, 32] -> float64 [W, 96]."""
    rows = np.asarray(rows)
    return O.embedding_stage(rows[..., None], emb, np.float64).reshape(rows.shape[0], O.EMB_DIM)


def mel_units32(db32, floor=None):
    """fmaf(fmaxf(db, floor), 0.1f, 2.0f) as the kernels evaluate it: the product of two fp32 values is exact in float64, so one
    float64 sum and one rounding to fp32 give the fused result (a double rounding needs a float64 sum that ends exactly on an fp32
    tie).  floor None: the rows are clamped already (what oww_mel_clips returns)."""
    db = np.asarray(db32)
    assert db.dtype == np.float32
    if floor is not None:
        db = np.maximum(db, np.float32(floor))
    return (db.astype(np.float64) * np.float64(np.float32(0.1)) + 2.0).astype(np.float32)


def spec64(x):
    """int16 [n] -> float64 [F, 32] in mel units, the floor this clip's own."""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1
    return O.mel_transform(O.mel_stage(x, np.float64)[0, 0])


def clip_embeddings64(x, emb):
    """int16 [B, n] -> float64 [B, n_windows, 96], float64 end to end: mel_stage(float64) of every clip alone (one floor PER CLIP),
    / 10 + 2, windows, CNN.  (OracleAudioFeatures.clip_embeddings casts the window batch to float32.)"""
    return np.stack([cnn64(windows(spec64(c)), emb) for c in np.atleast_2d(x)])


def window_movement(a, b):
    """[W]: max |a - b| / max |b| of every window, for [W, 96] arrays (the normalisation of cnn_budget.ratios)."""
    import cnn_budget as CB
    return CB.ratios(a, b)


def same_floor_at(n_short, n_long, margin_db=1e-2):
    """The clips whose per-clip float64 maximum is the same value at both lengths: either every frame beyond the short cut lies at
    least margin_db below it, or all frames are alike (a stationary clip: the maximum is every frame's).  Their first windows must carry
    the same bits at both lengths."""
    out = []
    for name in ORDER:
        a, b = mel_ref(clip(name, n_short)), mel_ref(clip(name, n_long))
        Fs = a.u.shape[1]
        stationary = float(np.ptp(b.u[0], axis=0).max()) < 1e-9
        if a.u.max() == b.u.max() and (stationary or b.u[0, Fs:].max() <= a.u.max() - margin_db):
            out.append(name)
    return tuple(out)
