"""Shared by tests/test_rnn_regimes_cpu.py and tests/test_rnn_regimes_gpu.py: the recurrent head kernel (owk::heads_rnn_kernel, the
2-layer bidirectional LSTM(64) head of train.py's model_type "rnn") across gate regimes.

The other files that run this kernel draw weights of one temperament (weights.synthetic_rnn_head: gates near the middle, recurrent
gain 0.8 / sqrt(64), biases N(0, 0.3)).  This file holds the regimes -- each one draw of weights.synthetic_head(kind="rnn") changed in
place so that one LSTM quantity decides the score --, the inputs, the admission rule on the reference (fp32 oracle against float64
oracle under four summation orders), a numpy fp32 restatement of what the kernel computes with nine selectable defects, and the case
table that says which admitted (regime, T, n_out) goes into which handle.  No expectation is computed from the emulation; it exists to
show that the cases tell a right kernel from a wrong one.  HIP-free, no tests."""
import copy
import functools

import numpy as np

from oracle import oww_oracle as O
from openwakeword_amd import weights as W

import head_windows as HW
from test_head_regimes import FP32_CAP, LOUD_ROW, N_ROWS, TOL_SCORE, ZERO_ROW          # noqa: F401  (the project's tolerances, not new ones)

H = W.RNN_HID                        # 64 hidden units per direction; gate columns i | f | g | o in blocks of H
T_ALL = (1, 2, 16, 64)               # 64 = RNN_TMAX (owwhip_layout.h), the largest LDS footprint
N_OUTS = (1, 8)                      # sigmoid; ReLU + softmax
MAX_HEADS, MAX_LABELS = 16, 32       # include/owwhip.h: OWW_MAX_HEADS, OWW_MAX_LABELS
N_ORDERS = 4                         # summation orders of the admission rule: the natural one and three feature-column permutations
MIN_SPREAD = 0.05                    # np.ptp of the float64 scores of a case: the comparison is not vacuous (tests/test_rnn_heads.py)

I_COLS, F_COLS, G_COLS, O_COLS = (slice(k * H, (k + 1) * H) for k in range(4))
windows = HW.windows                 # float32 [37, T, 96]: N(0, 1), row 5 all zero, row 20 at 30 x, fixed seed, read-only


# ------------------------------------------------------------------------------------------------ regimes
def _directions(head):
    """(layer, direction, w, b) of both layers x both directions; w [n_in + 64, 256] rows (x ; h)."""
    for li, layer in enumerate(head["lstm"]):
        for di, (w, b) in enumerate(layer):
            yield li, di, w, b


def _bias(cols, delta):
    def change(head):
        for _l, _d, _w, b in _directions(head):
            for c, d in zip(cols, delta):
                b[c] += np.float32(d)
    return change


def _scale(rows, factor, layers=(0, 1)):
    """rows: "all", "rec" (the 64 recurrent rows), "in" (the input rows)."""
    def change(head):
        for li, _d, w, _b in _directions(head):
            if li not in layers:
                continue
            n_in = w.shape[0] - H
            sl = {"all": slice(None), "rec": slice(n_in, None), "in": slice(0, n_in)}[rows]
            w[sl] *= np.float32(factor)
    return change


def _out(factor=1.0, shift=0.0):
    def change(head):
        head["w_out"] *= np.float32(factor)
        head["b_out"] += np.float32(shift)
    return change


# regime -> (seed offset of the draw, change in place, what it exercises)
REGIMES = {
    "seed1": (0, None, "baseline"),
    "seed2": (1000, None, "baseline"),
    "seed3": (2000, None, "baseline"),
    "remember": (0, _bias((F_COLS,), (6.0,)), "forget gate at 1: c carried across all T steps"),
    "forget": (0, _bias((F_COLS,), (-6.0,)), "memoryless cell: the first-step shortcut equals the general step with c = 0"),
    "closed": (0, _bias((I_COLS,), (-20.0,)), "input gate shut: c = h = 0 up to tiny terms, the score is sigmoid(b_out)"),
    "cell_big": (0, _bias((F_COLS, I_COLS), (8.0, 8.0)), "|c| grows to order T, tanh(c) saturates"),
    "gates_x4": (0, _scale("all", 4.0), "all four gates saturate; expf(-v) overflows to inf inside the sigmoid"),
    "rec_x4": (0, _scale("rec", 4.0), "error amplification through h"),
    "rec_x2": (0, _scale("rec", 2.0), "error amplification through h at T = 64"),
    "in_cold": (0, _scale("in", 2.0 ** -10, layers=(0,)), "the output is governed by biases and the recurrence"),
    "out_x16": (0, _out(16.0), "logits beyond +- 40"),
    "out_x50": (0, _out(50.0), "softmax with one dominant class, the others down to 1e-80 in float64"),
    "relu_dead": (0, _out(shift=-200.0), "every logit clipped by the ReLU: 1/8 bit for bit; n_out = 1: score 0 in fp32"),
    "gates_x16": (0, _scale("all", 16.0), "chaotic: not admitted"),
}
UNCENTRED = ("closed", "relu_dead")              # their score IS the output bias
# the regimes whose spread is small by construction, with the np.ptp of the float64 scores that the construction allows at most:
#   closed     sigmoid(b_out) on every row; what is left of i = sigmoid(-20 + .) moves the logit by less than 1e-6
#   relu_dead  n_out = 8: exactly 1/8 everywhere (spread 0); n_out = 1: sigmoid(-200 + .) < 1e-60
#   in_cold    the features reach layer 0 at 2^-10: every row but the loud one (30 x) scores the zero row's value within 1e-2;
#              the spread of the whole table comes from the loud row alone and has no lower bound
SPREAD_AT_MOST = {"closed": 1e-6, "relu_dead": 1e-60}
NO_SPREAD_FLOOR = ("closed", "in_cold", "relu_dead")
IN_COLD_QUIET_SPREAD = 1e-2                      # (stated, like the two above, by the construction: a logit moves by |x| 2^-10 |w| ~ 3e-3)


def applies(regime, T, n_out):
    """The cases the regime table asks for, before admission."""
    if regime == "out_x50":
        return n_out == 8
    if regime == "rec_x4":
        return T <= 16
    if regime == "rec_x2":
        return T == 64
    if regime == "gates_x16":
        return T >= 16                           # (at T <= 2 nothing can be amplified: the figures of the table are T = 16 and 64)
    return True


ALL_CASES = tuple((r, T, n) for r in REGIMES for T in T_ALL for n in N_OUTS if applies(r, T, n))
# (regime, T, n_out) -> worst |fp32 oracle - float64 oracle| over the four summation orders, centred, as measured by
# tests/test_rnn_regimes_cpu.py (which re-derives the table and holds each figure within a factor of 2)
NOT_ADMITTED = {
    ("gates_x16", 16, 1): 0.33, ("gates_x16", 16, 8): 0.67, ("gates_x16", 64, 1): 0.99, ("gates_x16", 64, 8): 1.0,
}
ADMITTED = tuple(c for c in ALL_CASES if c not in NOT_ADMITTED)


def name_of(case):
    r, T, n = case
    return f"{r}_t{T}_o{n}"


@functools.lru_cache(maxsize=None)
def _head(case):
    regime, T, n_out = case
    off, change, _ = REGIMES[regime]
    h = W.synthetic_head(f"rnn_o{n_out}", 5000 + T + off, kind="rnn", n_out=n_out, T=T)
    if change is not None:
        change(h)
    if regime not in UNCENTRED:
        HW.centre(h, windows(T))                 # (n_out = 1 only: b_out moved by minus the median float64 logit)
    return h


def head(case):
    """The head of one (regime, T, n_out): a fresh copy, centred on windows(T) where the regime allows it."""
    return copy.deepcopy(_head(case))


@functools.lru_cache(maxsize=None)
def _want(case, dtype):
    with np.errstate(over="ignore"):             # (fp32 exp(-z) overflows to inf where a gate or the output saturates: 1 / inf = 0)
        w = O.head_stage(windows(case[1]), _head(case), np.dtype(dtype).type).astype(np.float64)
    w.setflags(write=False)
    return w


def want(case, dtype=np.float64):
    """[37, n_out] of one case from the oracle in `dtype` (computed once, read-only)."""
    return _want(case, np.dtype(dtype).name)


def logits64(case):
    """The float64 output layer before its activation, [37, n_out]."""
    hd = _head(case)
    a = np.asarray(windows(case[1]), np.float64)
    with np.errstate(over="ignore"):
        for layer in hd["lstm"]:
            a = np.concatenate([O._lstm_direction(a, layer[0][0], layer[0][1], False, np.float64),
                                O._lstm_direction(a, layer[1][0], layer[1][1], True, np.float64)], axis=2)
    return a[:, -1] @ hd["w_out"].astype(np.float64) + hd["b_out"].astype(np.float64)


# ------------------------------------------------------------------------------------------------ admission
def permuted(ft, hd, order):
    """The same computation in another summation order: the 96 feature columns permuted together with layer 0's input rows."""
    if order == 0:
        return ft, hd
    perm = np.random.default_rng(9000 + order).permutation(96)
    hd = copy.deepcopy(hd)
    for d in range(2):
        w, b = hd["lstm"][0][d]
        hd["lstm"][0][d] = (np.concatenate([w[:96][perm], w[96:]], axis=0), b)
    return np.ascontiguousarray(ft[:, :, perm]), hd


@functools.lru_cache(maxsize=None)
def fp32_error(case):
    """Worst |fp32 oracle - float64 oracle| on windows(T), one figure per summation order."""
    ft, hd, ref = windows(case[1]), _head(case), want(case)
    out = []
    for order in range(N_ORDERS):
        f, h = permuted(ft, hd, order)
        with np.errstate(over="ignore"):
            got = O.head_stage(f, h, np.float32).astype(np.float64)
        out.append(float(np.abs(got - ref).max()))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ emulation
DEFECTS = {
    1: "gate blocks read in ONNX order (i o f c) without the conversion",
    2: "layer 1's reverse direction stepped at t = 0 instead of t = T - 1",
    3: "layer 1's reverse direction run over all T steps, its final state taken (h_n instead of out[:, -1])",
    4: "a direction's first step does not skip the previous direction's leftover hidden vector",
    5: "tanh(c) replaced by c in h = o tanh(c)",
    6: "layer 1 fed the forward half of layer 0 twice",
    7: "a sigmoid with a relative error of 1e-3",
    8: "the first step uses c = f c_stale + i g with the previous direction's cell",
    9: "tanh(v) computed as (e^2v - 1) / (e^2v + 1): inf / inf beyond v = 44",
}
VANISH_AT_T1 = (2, 3)                # by construction: at T = 1, t = 0 IS t = T - 1 and "all T steps" is the one step.  (Defects 4 and 8
                                     # do not vanish there: layer 0's reverse direction already follows a direction that left a state.)


def emulate(ft, hd, defect=None):
    """What heads_rnn_kernel computes, in numpy fp32: per direction the accumulator starts at the bias, takes x W_x, then h W_h except
    on the direction's first step; c = i g on the first step; layer 1's reverse direction takes ONE step from a zero state at t = T - 1;
    Linear(128, n_out) on [fwd_last | bwd_first]; sigmoid, or ReLU then max-subtracted softmax.  -> float32 [rows, n_out]"""
    f32 = np.float32
    x0 = np.asarray(ft, f32)
    B, T, _ = x0.shape

    def sig(v):
        with np.errstate(over="ignore"):
            s = f32(1.0) / (f32(1.0) + np.exp(-v))
        return s * f32(1.001) if defect == 7 else s

    def tanh(v):
        if defect != 9:
            return np.tanh(v)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(f32(2.0) * v)
            return (e - f32(1.0)) / (e + f32(1.0))

    h_stale, c_stale = np.zeros((B, H), f32), np.zeros((B, H), f32)     # what the previous direction left behind
    src, last = x0, None
    for li in range(2):
        outs = []
        for di in range(2):
            w, b = hd["lstm"][li][di]
            n_in = w.shape[0] - H
            wx, wh = w[:n_in], w[n_in:]
            xin = src
            if li == 1 and defect == 6:
                xin = np.concatenate([src[:, :, :H], src[:, :, :H]], axis=2)
            one_step = li == 1 and di == 1 and defect != 3
            ts = list(range(T)) if di == 0 else list(range(T - 1, -1, -1))
            if one_step:
                ts = [0 if defect == 2 else T - 1]
            h, c = h_stale, c_stale
            out = np.zeros((B, T, H), f32)
            for it, t in enumerate(ts):
                first = it == 0
                z = b[None, :] + xin[:, t] @ wx
                if not first or defect == 4:
                    z = z + h @ wh
                blocks = [z[:, k * H:(k + 1) * H] for k in range(4)]
                if defect == 1:
                    i, o, f, g = blocks
                else:
                    i, f, g, o = blocks
                i, f, g, o = sig(i), sig(f), tanh(g), sig(o)
                c = i * g if first and defect != 8 else f * c + i * g
                h = (o * (c if defect == 5 else tanh(c))).astype(f32)
                out[:, t] = h
            h_stale, c_stale = h, c
            outs.append(out)
        if li == 0:
            src = np.concatenate(outs, axis=2)
        else:
            t_bwd = 0 if defect in (2, 3) else T - 1
            last = np.concatenate([outs[0][:, T - 1], outs[1][:, t_bwd]], axis=1)
    z = hd["b_out"][None, :].astype(f32) + last @ hd["w_out"].astype(f32)
    if int(hd["n_out"]) == 1:
        return sig(z).astype(f32)
    z = np.maximum(z, f32(0))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(f32)


# ------------------------------------------------------------------------------------------------ the existing mild-weight inputs
def mild_inputs():
    """The inputs of tests/test_rnn_heads.py at 37 streams: its two heads, features N(0, 0.3) and N(0, 2) -> [(label, head, ft)]."""
    heads = {"rnn1": W.synthetic_head("rnn1", 61, kind="rnn", n_out=1), "rnn5": W.synthetic_head("rnn5", 62, kind="rnn", n_out=5, T=34)}
    rng = np.random.default_rng(4)
    out = []
    for name, h in heads.items():
        for scale in (0.3, 2.0):
            out.append((f"{name} N(0, {scale})", h, rng.normal(0, scale, (N_ROWS, h["T"], 96)).astype(np.float32)))
    return out


# ------------------------------------------------------------------------------------------------ the case table
FAMILY_REGIMES = ("seed1", "remember", "gates_x4")       # also run in the exact-fp32 and the plain families (the kernel is the same one)
SLOT_T = (16, 64)                                        # slot and neighbour invariance: FAMILY_REGIMES at these T, both n_out
SLOT_ROWS = (0, 3, ZERO_ROW, 11, LOUD_ROW, 36)


def pack(cases):
    """Handles for `cases` in order, first fit: at most MAX_HEADS heads and MAX_LABELS score columns each -> [[case, ...], ...]"""
    handles = []
    for c in cases:
        for hnd in handles:
            if len(hnd) < MAX_HEADS and sum(k[2] for k in hnd) + c[2] <= MAX_LABELS:
                hnd.append(c)
                break
        else:
            handles.append([c])
    return handles


@functools.lru_cache(maxsize=None)
def handles(family=3):
    """The device table: every admitted case of a family, one T per handle -> ((T, (case, ...)), ...)"""
    out = []
    for T in T_ALL:
        cases = [c for c in ADMITTED if c[1] == T and (family == 3 or c[0] in FAMILY_REGIMES)]
        out += [(T, tuple(hnd)) for hnd in pack(cases)]
    return tuple(out)


def check_table():
    """The coverage guard: every admitted (regime, T, n_out) is placed exactly once in the default family's handles, the three family
    regimes exactly once in the others', and every handle keeps the library's limits."""
    for family in (3, 1, 0):
        placed = [c for _T, hnd in handles(family) for c in hnd]
        expect = [c for c in ADMITTED if family == 3 or c[0] in FAMILY_REGIMES]
        assert sorted(placed) == sorted(expect), (family, set(expect) ^ set(placed))
        assert len(placed) == len(set(placed))
        for _T, hnd in handles(family):
            assert len(hnd) <= MAX_HEADS and sum(c[2] for c in hnd) <= MAX_LABELS, hnd
    assert not set(NOT_ADMITTED) & set(ADMITTED) and set(NOT_ADMITTED) <= set(ALL_CASES)
    for r in REGIMES:                                    # every regime of the table reaches the device or is recorded as left out
        assert any(c[0] == r for c in ADMITTED) or any(c[0] == r for c in NOT_ADMITTED), r
    return True


def handle_heads(hnd):
    return {name_of(c): head(c) for c in hnd}


# ------------------------------------------------------------------------------------------------ call routes: the oracle model's side
CALL_S, CALL_ORACLE, CALL_MAX_CHUNKS, CALL_WARMUP = 9, 4, 3, 5
CALL_SIZES = (1, 2, 3, 5, 1, 3)                          # chunks per call after the warm-up; 5 > max_chunks: the sliced long call
CALL_LABELS = ("rnn1",) + tuple(f"rnn5#{i}" for i in range(5)) + ("alexa",)
CALL_RNN_COLS = 6                                        # the first six score columns belong to the two recurrent heads
CALL_LEVELS = (2.0, 9000.0)                              # rms of a chunk, drawn per stream and chunk: the level changes inside the calls
CALL_PCM_SEED = 7101                                     # (levels and seed picked on the oracle alone until early_max_share held; then fixed)
EARLY_MARGIN, EARLY_SHARE = 1e-2, 0.25                   # non-vacuity of the max over a call's chunks (asserted on the oracle alone)
# the plain schedule, and one with masked one-chunk steps between the multi-chunk calls: (chunks, streams that sit out)
PLAIN_CALLS = tuple((1, ()) for _ in range(CALL_WARMUP)) + tuple((k, ()) for k in CALL_SIZES)
MASKED_CALLS = tuple((1, ()) for _ in range(CALL_WARMUP)) + ((3, ()), (1, (1, 3, 4, 8)), (2, ()), (1, (0, 2, 5, 6, 7)), (3, ()))


def call_heads():
    """The heads of tests/test_rnn_heads.py: a sigmoid recurrent head (T = 16), a five-class one (T = 34), and the MLP head alexa."""
    import cases
    return {"rnn1": W.synthetic_head("rnn1", 61, kind="rnn", n_out=1), "rnn5": W.synthetic_head("rnn5", 62, kind="rnn", n_out=5, T=34),
            "alexa": W.synthetic_head("alexa", cases.SEED_WEIGHTS)}


def call_emb():
    import cases
    return W.synthetic_embedding(cases.SEED_WEIGHTS)


@functools.lru_cache(maxsize=None)
def call_pcm(n_chunks):
    """int16 [CALL_S, 1280 n_chunks]: Gaussian noise whose rms is drawn anew for every stream and chunk (fixed seed, read-only)."""
    rng = np.random.default_rng(CALL_PCM_SEED)
    rms = rng.choice(CALL_LEVELS, size=(CALL_S, n_chunks))
    x = rng.normal(0.0, 1.0, (CALL_S, n_chunks, 1280)) * rms[:, :, None]
    pcm = np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(CALL_S, -1)
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def oracle_calls(schedule):
    """The oracle model of streams 0 .. CALL_ORACLE - 1 through `schedule` ((chunks, streams that sit out), ...) ->
    (init_features [CALL_ORACLE][ring, 96], [per call: dict(k, off, scores [CALL_ORACLE, 7] -- NaN rows for streams that sat out --,
    chunk_raw [CALL_ORACLE, k, 7] the head outputs of each chunk of the call, oldest first)]).  Computed once per schedule."""
    heads, emb = call_heads(), call_emb()
    pcm = call_pcm(sum(k for k, _ in schedule))
    ring = max(int(h["T"]) for h in heads.values())
    models, inits, seen = [], [], []
    for s in range(CALL_ORACLE):
        log = {n: [] for n in heads}
        fns = {n: (lambda x, _h=h, _l=log[n]: (_l.append(O.head_stage(x, _h, np.float32)), [_l[-1]])[1]) for n, h in heads.items()}
        m = O.OracleModel(heads, emb, init_noise=W.synthetic_pcm(1, 64000, seed=500 + s, rms=600.0)[0], head_fns=fns,
                          class_mapping={"rnn5": {str(i): f"rnn5#{i}" for i in range(5)}})
        models.append(m)
        seen.append(log)
        inits.append(np.array(m.preprocessor.features[-ring:], np.float32))
    out, at = [], 0
    for k, off in schedule:
        x = pcm[:, 1280 * at:1280 * (at + k)]
        scores = np.full((CALL_ORACLE, len(CALL_LABELS)), np.nan)
        chunk_raw = np.full((CALL_ORACLE, k, len(CALL_LABELS)), np.nan)
        for s, m in enumerate(models):
            if s in off:
                continue
            for log in seen[s].values():
                log.clear()
            p = m.predict(x[s])
            scores[s] = [p[n] for n in CALL_LABELS]
            per = np.concatenate([np.concatenate(seen[s][n], axis=0).reshape(k, -1) for n in heads], axis=1)
            chunk_raw[s] = per
        out.append(dict(k=k, off=off, at=at, scores=scores, chunk_raw=chunk_raw))
        at += k
    return tuple(inits), tuple(out)


def early_max_share(calls):
    """Of the (call of more than one chunk, oracle stream that took part, recurrent column) triples: the share whose maximum over the
    call's chunks is taken before the last chunk and exceeds the last chunk's value by more than EARLY_MARGIN."""
    n = hit = 0
    for c in calls:
        if c["k"] == 1:
            continue
        for s in range(CALL_ORACLE):
            if s in c["off"]:
                continue
            r = c["chunk_raw"][s][:, :CALL_RNN_COLS]
            n += r.shape[1]
            hit += int((r[:-1].max(axis=0) > r[-1] + EARLY_MARGIN).sum())
    return hit / max(n, 1), n
