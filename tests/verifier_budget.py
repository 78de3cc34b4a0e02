"""The custom-verifier kernels against float64: restatement, reference, budget, weight regimes, faults and the pair-list mirror
(helper module, no tests; tests/test_verifier_budget_cpu.py derives every number here, tests/test_verifier_regimes.py spends them).

verifier_kernel and stream_verifier_kernel (csrc/owwhip_kernels.h) re-score a head output with sigmoid(sum_i w_i x_i + b) over the
stream's last T ring rows: 64 lane accumulators, element i on lane i % 64 in ascending i, one fmaf per element, the xor butterfly
32 .. 1, + b, 1 / (1 + expf(-z)).  restate32 is that order in numpy, ref64 the same map in float64 on the fp32 (w, b) the device is
given.  A flat tolerance says little about a sum whose terms cancel against b (the folded StandardScaler centring), so the budget of a
re-scored score is relative to the mass kappa = sum |w_i x_i| + |b|:

    budget = 0.25 * MARGIN * E32[T] * kappa + MARGIN * A

0.25 is the sigmoid's largest slope; E32[T] = max |z_restate32 - z_ref64| / kappa of the fp32 RESTATEMENT over every regime and window
set of the CPU tier; A = max |score_restate32 - sigmoid64(z_restate32)| (expf, the division, the last rounding); MARGIN = 4 is what
tests/cnn_budget.py and tests/mel_budget.py give a device over its CPU restatement (another expf, another contraction).  Nothing here
is measured on a device.

Windows are taken from RINGS, float32 [n, TR, 96] oldest row first with the newest row at index TR - 1 -- what get_features(s, TR)
returns after a call -- because the faults of FAULTS are faults of the ring walk: a start one slot early reads, when T = TR, the row
just written."""
import functools
import warnings
from typing import NamedTuple

import numpy as np

from openwakeword_amd.model import VerifierFoldWarning, fold_verifier

LANES = 64
EMB = 96
MARGIN = 4
T_VALUES = (1, 5, 16, 34, 120)
REGIMES = ("reference", "unit", "offset", "lowvar", "sparse_rows", "alternating")
FAULTS = ("early", "late", "reversed", "tail32", "no_bias", "stride")
LOWVAR_SCALE = 1e-3
U24 = 2.0 ** -24

# max |z_restate32 - z_ref64| / kappa per T, over every regime of REGIMES on the oracle rings and `lowvar` on the near-constant windows:
# tests/test_verifier_budget_cpu.py::test_e32_and_a_are_the_measured_envelope measures them and holds each frozen figure between the
# measurement and twice the measurement.
E32 = {1: 1.35 * U24, 5: 0.55 * U24, 16: 0.68 * U24, 34: 0.86 * U24, 120: 0.95 * U24}     # measured 1.170, 0.473, 0.588, 0.749, 0.827
# max |score_restate32 - sigmoid64(z_restate32)|, same test
A = 1.2e-7                                                                                # measured 8.63e-8


def ring_rows(T):
    """Rows of the feature ring the GPU tier runs window length T on (H34 / H120 of tests/test_verifier_regimes.py)."""
    return 34 if T <= 34 else 120


def budget(T, kappa):
    return 0.25 * MARGIN * E32[T] * np.asarray(kappa, np.float64) + MARGIN * A


# ------------------------------------------------------------------------------------------------ the two evaluations
def restate32(window, w, b):
    """(logit, score) float32 of the kernels' arithmetic; window [..., n] float32, w [n] float32, b a float (rounded to fp32)."""
    x = np.asarray(window, np.float32)
    w = np.asarray(w, np.float32).ravel()
    lead, n = x.shape[:-1], x.shape[-1]
    assert w.size == n, (w.size, n)
    x = x.reshape(-1, n)
    steps = -(-n // LANES)
    xp = np.zeros((x.shape[0], steps * LANES), np.float32)      # fmaf(0, 0, acc) = acc: the idle lanes of a last half pass
    xp[:, :n] = x
    wp = np.zeros(steps * LANES, np.float32)
    wp[:n] = w
    xp = xp.reshape(-1, steps, LANES).astype(np.float64)
    wp = wp.reshape(steps, LANES).astype(np.float64)
    acc = np.zeros((x.shape[0], LANES), np.float32)
    for k in range(steps):                                       # fp32 x fp32 is exact in float64; one rounding to fp32 per step
        acc = (xp[:, k] * wp[k] + acc.astype(np.float64)).astype(np.float32)
    o = LANES // 2
    while o:                                                     # lanes l and l ^ o add the same pair: one value per pair survives
        acc = (acc[:, :o] + acc[:, o:2 * o]).astype(np.float32)
        o //= 2
    z = (acc[:, 0] + np.float32(b)).astype(np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(-z, dtype=np.float32)
        score = (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)
    return z.reshape(lead), score.reshape(lead)


def sigmoid64(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def ref64(window, w, b):
    """(logit, score, kappa) in float64 of the fp32 (w, b) the device holds; kappa = sum |w_i x_i| + |b|."""
    x = np.asarray(window, np.float32).astype(np.float64)
    w = np.asarray(w, np.float32).astype(np.float64).ravel()
    b = float(np.float32(b))
    p = x * w
    z = p.sum(axis=-1) + b
    return z, sigmoid64(z), np.abs(p).sum(axis=-1) + abs(b)


# ------------------------------------------------------------------------------------------------ windows and faults
def windows(rings, T, fault=None):
    """float32 [n, T * 96]: the last T rows of each ring [n, TR, 96], or what a faulty walk of the ring slots reads instead."""
    rings = np.asarray(rings, np.float32)
    TR = rings.shape[1]
    assert 1 <= T <= TR and rings.shape[2] == EMB
    idx = TR - T + np.arange(T)
    if fault == "early":
        idx = idx - 1
    elif fault == "late":
        idx = idx + 1
    elif fault == "reversed":
        idx = idx[::-1]
    return np.ascontiguousarray(rings[:, idx % TR].reshape(rings.shape[0], T * EMB))


def faulty(fault, rings, T, w, b):
    """(window, w, b) as a kernel with `fault` would combine them."""
    w = np.asarray(w, np.float32)
    if fault in ("early", "late", "reversed"):
        return windows(rings, T, fault), w, b
    x = windows(rings, T)
    if fault == "tail32":                        # the half-wave tail of an odd T never runs
        w = w.copy()
        w[-32:] = 0
    elif fault == "no_bias":
        b = 0.0
    elif fault == "stride":                      # a table of rows 96 (T + 1) apart read where they are 96 T apart, at label 1: every weight
        w = np.concatenate([w[EMB:], np.zeros(EMB, np.float32)])     # one ring row off, the last row on the table's zero padding
    else:
        raise ValueError(fault)
    return x, w, b


# ------------------------------------------------------------------------------------------------ regimes
class Triple(NamedTuple):
    """A fitted scikit-learn pipeline flatten -> StandardScaler -> LogisticRegression, as numbers (float64)."""
    coef: np.ndarray
    mean: np.ndarray
    scale: np.ndarray
    intercept: float


class StandardScaler:                            # (fold_verifier goes by the class names of the reference's pipeline)
    def __init__(self, mean, scale):
        self.mean_, self.scale_ = mean, scale


class LogisticRegression:
    def __init__(self, coef, intercept):
        self.coef_, self.intercept_ = coef[None, :], np.array([intercept])


class Pipeline:
    def __init__(self, t: Triple):
        self.steps = [("standardscaler", StandardScaler(t.mean, t.scale)), ("logisticregression", LogisticRegression(t.coef, t.intercept))]


def pipeline_logit(t: Triple, window):
    """The unfolded pipeline in float64: sum coef (x - mean) / scale + intercept."""
    x = np.asarray(window, np.float32).astype(np.float64)
    return ((x - t.mean) / t.scale) @ t.coef + t.intercept


def kappa_hat(t: Triple, w=None, b=None):
    """sum |w_i| (|mean_i| + scale_i) + |b|: the mass of the folded map on data the scaler was fitted to."""
    if w is None:
        w, b = fold_verifier(Pipeline(t))
    return float(np.sum(np.abs(np.asarray(w, np.float64)) * (np.abs(t.mean) + t.scale)) + abs(b))


def _normalised(coef, mean, scale, X):
    """Coefficients scaled for a logit standard deviation of 2 over the windows X, the intercept for a median of 0."""
    u = ((X.astype(np.float64) - mean) / scale) @ coef
    c = 2.0 / float(np.std(u))
    return Triple(coef * c, mean, scale, -float(np.median(u * c)))


def _fixture_triple(T, seed):
    """The fixture's recipe (tests/verifier_fixture.py) at window length T; T = 16 is the fixture itself."""
    from verifier_fixture import flatten_features, trained_verifier
    if T == 16:
        pipe = trained_verifier(seed)
    else:
        from sklearn.linear_model import LogisticRegression as LR
        from sklearn.pipeline import make_pipeline
        from sklearn.preprocessing import FunctionTransformer, StandardScaler as SS
        r = np.random.default_rng(seed)
        X = r.normal(0, 4.0, (60, T, EMB)).astype(np.float32)
        y = (X[:, :, :8].mean(axis=(1, 2)) > 0).astype(int)
        if y.min() == y.max():
            y[0] = 1 - y[0]
        pipe = make_pipeline(FunctionTransformer(flatten_features), SS(), LR(random_state=0, max_iter=2000, C=0.001))
        pipe.fit(X, y)
    sc, clf = pipe.steps[1][1], pipe.steps[2][1]
    return Triple(np.asarray(clf.coef_, np.float64)[0], np.asarray(sc.mean_, np.float64), np.asarray(sc.scale_, np.float64),
                  float(clf.intercept_[0]))


def lowvar_columns(n):
    return np.arange(n) % 8 == 3


# seeds other than 0: chosen on the FLOAT64 reference alone, so that every fault of FAULTS moves it by a hundred budgets in 95 % of
# the oracle windows with |z64| <= 4 (tests/test_verifier_budget_cpu.py asserts 90 %); dropping 32 of 11,520 products is the faint one
SEEDS = {("unit", 34): 1, ("unit", 120): 2, ("lowvar", 120): 1, ("alternating", 120): 3}


def triple(regime, T, X, seed=None):
    """The regime's pipeline at window length T, calibrated on the windows X [n, T * 96] (never on a verifier's output)."""
    n = T * EMB
    seed = SEEDS.get((regime, T), 0) if seed is None else seed
    assert X.shape[1] == n
    r = np.random.default_rng([20261019, REGIMES.index(regime), T, seed])
    g = r.standard_normal(n)
    zero, one = np.zeros(n), np.ones(n)
    col_mean = X.astype(np.float64).mean(axis=0)
    if regime == "reference":
        return _fixture_triple(T, seed)
    if regime == "unit":
        return _normalised(g, zero, one, X)
    near_mean = col_mean * (1.0 + 0.01 * r.standard_normal(n))
    col_std = X.astype(np.float64).std(axis=0)
    if regime == "offset":                       # a StandardScaler fitted to data like X
        return _normalised(g, near_mean, col_std, X)
    if regime == "lowvar":
        lv = lowvar_columns(n)
        return _normalised(g, np.where(lv, col_mean, near_mean), np.where(lv, LOWVAR_SCALE, col_std), X)
    if regime == "sparse_rows":
        keep = np.zeros((T, EMB), bool)
        keep[[0, T - 1]] = True
        return _normalised(np.where(keep.ravel(), g, 0.0), zero, one, X)
    if regime == "alternating":
        # one column pattern v on every row, the sign flipping from row to row; the amplitude rises towards the newest row, so that
        # neither a reversed walk of an odd T nor the static part of the features cancels
        v = r.standard_normal(EMB)
        rows = np.where(np.arange(T) % 2 == 0, 1.0, -1.0) * (0.5 + np.arange(T) / T)
        return _normalised((rows[:, None] * v[None, :]).ravel(), zero, one, X)
    raise ValueError(regime)


def folded(t: Triple):
    """(w float32 [T * 96], b) of the project's own fold (its warning is test_verifier_budget_cpu.py::test_fold_warning's subject)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", VerifierFoldWarning)
        return fold_verifier(Pipeline(t))


def near_constant(X, seed=0):
    """X with one feature in eight replaced by a nearly constant column: its mean plus N(0, LOWVAR_SCALE).  The device's features hold
    no such column, so this set exists in the CPU tier only -- it is what `lowvar` was named for."""
    X = np.array(X, np.float32)
    lv = lowvar_columns(X.shape[1])
    r = np.random.default_rng([20261019, 77, seed])
    m = X[:, lv].astype(np.float64).mean(axis=0)
    X[:, lv] = (m + LOWVAR_SCALE * r.standard_normal((X.shape[0], int(lv.sum())))).astype(np.float32)
    return X


# ------------------------------------------------------------------------------------------------ audio
def case_pcm(S, n_frames, seed=0x5EED):
    """int16 [S, n_frames * 1280]: five kinds of stream (s % 5) so that the feature rows differ between streams and from row to row --
    white noise, low-passed noise, bursts between silence, quiet noise, a swept tone in noise."""
    n = n_frames * 1280
    r = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    out = np.zeros((S, n))
    for s in range(S):
        x = r.normal(0.0, 1.0, n)
        kind = s % 5
        if kind == 0:
            x = 3000.0 * x
        elif kind == 1:
            x = 6000.0 * np.convolve(x, np.ones(12) / 12.0, mode="same")
        elif kind == 2:
            gate = ((np.arange(n) // (1280 * 3 + 400 * (s // 5 + 1))) % 2).astype(np.float64)
            x = 8000.0 * x * gate
        elif kind == 3:
            x = 30.0 * x
        else:
            x = 300.0 * x + 9000.0 * np.sin(2 * np.pi * (300.0 + 900.0 * (1 + np.sin(2 * np.pi * 0.7 * t))) * t)
        out[s] = x
    return np.clip(np.rint(out), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def oracle_rows():
    """float32 [3, R, 96], read-only: oracle.oww_oracle clip embeddings of case_pcm streams 0..2 (the CPU tier's feature rows)."""
    from openwakeword_amd import weights as W
    from oracle import oww_oracle as O
    af = O.OracleAudioFeatures(W.synthetic_embedding(1234), init_noise=np.zeros(16000, np.int16))
    pcm = case_pcm(3, 200)
    rows = np.stack([af.clip_embeddings(pcm[s]) for s in range(3)]).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def oracle_rings(TR):
    """float32 [n, TR, 96]: every run of TR consecutive oracle rows of every stream."""
    rows = oracle_rows()
    out = np.stack([rows[s, e - TR + 1:e + 1] for s in range(rows.shape[0]) for e in range(TR - 1, rows.shape[1])])
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the pair list
DEFAULT, NONE = -1, -2
SV_PAIRS, SV_WAVES = 16, 4


class Entry(NamedTuple):
    s: int
    col: int             # >= 0 fixed score column; < 0: bank slot ~col
    T: int
    v: int               # >= 0 pool verifier; < 0: the handle-wide verifier of column ~v
    thr: float


def sv_list(fix, fix_thr, bank, bank_thr, pool_T, ver_T, ver_thr):
    """Mirror of owwhip_verifier_host.h::sv_list (owsv), to which test_verifier_budget_cpu.py holds it field by field.
    fix [S, NL] / bank [S, K]: pool ids, DEFAULT or NONE; pool_T: id -> T; ver_T [NL]: T of each column's handle-wide verifier (0 = none; empty: the handle has none at all).  Stream-major; per stream the fixed columns, then the bank slots; empty while every pair
    is at the default (verifier_kernel then serves the handle-wide verifiers)."""
    fix, bank = np.asarray(fix), np.asarray(bank)
    out = []
    if int(np.sum(fix != DEFAULT)) + int(np.sum(bank != DEFAULT)) == 0:
        return out
    for s in range(fix.shape[0]):
        for c in range(fix.shape[1]):
            v = int(fix[s, c])
            if v >= 0:
                out.append(Entry(s, c, pool_T[v], v, float(fix_thr[s, c])))
            elif v == DEFAULT and len(ver_T) and ver_T[c] > 0:
                out.append(Entry(s, c, ver_T[c], ~c, float(ver_thr[c])))
        for k in range(bank.shape[1]):
            v = int(bank[s, k])
            if v >= 0:
                out.append(Entry(s, ~k, pool_T[v], v, float(bank_thr[s, k])))
    return out


def wave_of(i):
    return i // SV_PAIRS


def n_waves(n):
    return -(-n // SV_PAIRS)


def n_workgroups(n):
    return -(-n // (SV_PAIRS * SV_WAVES))


# ------------------------------------------------------------------------------------------------ list shapes of the GPU tier (handle HL)
HL_S, HL_T = 33, (16, 5, 34)     # fixed columns 0 and 1 (T = 16, 5) are verified; the bank slot's head (T = 34) is also fixed column 2, unverified
HL_POOL = {0: 16, 1: 5, 2: 34}   # pool id -> T: one verifier per verified column and one for the slot
ENTRY_COUNTS = (1, 15, 16, 17, 63, 64, 65)
ALL_HIT_WAVE, NO_HIT_WAVE, MIXED_WAVE = 0, 1, 2
MASK_OFF = (2, 13, 15, 17, 20)   # streams the masked step of the list-shape case switches off


class Layout:
    """Assignment tables of handle HL and their pair list."""

    def __init__(self):
        self.fix = np.full((HL_S, 3), DEFAULT)
        self.fix_thr = np.zeros((HL_S, 3), np.float32)
        self.bank = np.full((HL_S, 1), DEFAULT)
        self.bank_thr = np.zeros((HL_S, 1), np.float32)
        self.ver_T = [0, 0, 0]
        self.ver_thr = [0.0, 0.0, 0.0]

    def put(self, s, where, thr):
        """where 0 / 1: the fixed column's pool verifier; 2: the slot's."""
        if where < 2:
            self.fix[s, where], self.fix_thr[s, where] = where, thr
        else:
            self.bank[s, 0], self.bank_thr[s, 0] = 2, thr

    def entries(self):
        return sv_list(self.fix, self.fix_thr, self.bank, self.bank_thr, HL_POOL, self.ver_T, self.ver_thr)


def count_layout(n, mid=0.5):
    """The first n (stream, column 0 / column 1 / slot) pairs carry their pool verifier; every third stream at threshold 0, the others at
    mid (one value, or one per column 0 / column 1 / slot)."""
    lay = Layout()
    mid = np.broadcast_to(np.asarray(mid, np.float64), (3,))
    for i in range(n):
        lay.put(i // 3, i % 3, 0.0 if (i // 3) % 3 == 0 else float(mid[i % 3]))
    return lay


def mixed_layout(mid=0.5):
    """63 entries in one workgroup: wave 0 hits on all 16 (threshold 0), wave 1 on none (1.5), wave 2 mixes pool entries on column 0
    (T = 16), the handle-wide verifier of column 1 on pairs left at the default (T = 5) and slot entries (T = 34), wave 3 holds the 15
    default entries of the remaining streams."""
    lay = Layout()
    lay.ver_T[1], lay.ver_thr[1] = 5, mid
    for base, thr in ((0, 0.0), (6, 1.5)):
        for s in range(base, base + 5):
            for where in range(3):
                lay.put(s, where, thr)
        lay.put(base + 5, 0, thr)
        lay.fix[base + 5, 1] = NONE
    for s in range(12, 17):
        lay.put(s, 0, mid)
        lay.put(s, 2, mid)
    lay.put(17, 0, mid)
    lay.fix[17, 1] = NONE
    return lay
