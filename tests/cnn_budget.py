"""The relative error budget of the embedding CNN, its float64 layer chain, the case table and a numpy emulation of the f16-split
kernels (helper module, no tests, no GPU).

Every comparison of a CNN activation with float64 has ONE form.  For stream s and layer l, over the rows compared,

    |got - y64| <= T * M,        M = max |y64| over those rows of that stream

and the same for an embedding window with M = the window's max |e64|.  The budget is relative to the layer's own largest activation:
a network whose embeddings are of order 1e-4 is held as tightly as one whose embeddings are of order 1e+5.

T = 4 * E32.  E32 is the fp32 REFERENCE's own envelope in that normalisation (oracle.oww_oracle's chain in float32 against the same chain
in float64) over the whole case table below, frozen with headroom because the oracle's matrix products are the BLAS library's and another
build sums in another order.  The factor 4 is the f16 split's operand width: x = xh + xl carries 22 mantissa bits, 4 x the fp32 unit
round-off; the exact-fp32 family (use_mfma = 1) has to fit the same T.  T moves with E32 only; tests/test_cnn_budget_cpu.py re-measures
E32 and shows with emulate_split() that kernels which are wrong in one constant, one term or one exponent leave the budget.

Rows compared: the rows of a layer that are new in one 80 ms step (8 mel rows -> 8, 4, 4, 2, 2, 1 rows in stages A..E and conv19), before
pooling -- what oww_debug_read returns.  A [76 + 16]-row input holds three such steps (windows)."""
import copy
import functools

import numpy as np

from oracle import oww_oracle as O
from openwakeword_amd import weights as W

E32 = 2.5e-6             # the fp32 oracle's envelope over REGIMES x (mel_inputs, the oracle's mel rows of pcm_rows) x 20 layers x 3 steps:
                         # measured 1.94e-6 (seed1234 / tiny / huge_embedding, the N(10, 1.5) input, layer 14), every other regime
                         # <= 1.70e-6; frozen with 1.29 x headroom for another BLAS summation order
T = 4 * E32              # 1.0e-5 of the layer's (the window's) largest float64 value

N_LAYERS = len(O.CNN_LAYERS)
N_STREAMS = 9
ROWS = O.MEL_WINDOW + 16                 # mel rows per stream of an embed() input: three windows
N_STEPS = 12                             # one-chunk steps of the PCM rows; layers are compared after steps 10 and 12
STEPS_COMPARED = (10, 12)
SEEDS = ("seed1234", "seed1", "seed2")
MODIFIED = ("hot", "cold", "conv_1e-3", "negative_bn", "tiny_embedding", "huge_embedding", "channel_cold")
REGIMES = SEEDS + MODIFIED
# Not admitted to the f16-split (use_mfma = 3) table: the FAITHFUL emulation leaves T there, so a correct kernel would too.
# channel_cold: one power of two per LAYER carries channels 2^8 apart; the cold channels' low halves fall into the f16 subnormal range
# (spacing 2^-24) and the next layer's 2^8 x weights bring that error back to full size -- 3.4 T at layer 18, above T from layer 9 on.
# The exact family (use_mfma = 1) is held to T in this regime like in every other.
NOT_ADMITTED = {"channel_cold": 3.4}      # regime -> the emulation's worst fraction of T (tests/test_cnn_budget_cpu.py re-derives both)
ADMITTED = tuple(n for n in REGIMES if n not in NOT_ADMITTED)
STAGE_LAST = (2, 6, 10, 14, 18)          # the layers whose pooled output is handed to the next stage (conv19 after 18)
STAGE_FIRST = (0, 3, 7, 11, 15)


def _new_rows():
    rows, out = 8, []
    for *_, pool in O.CNN_LAYERS:
        out.append(rows)
        if pool:
            rows //= pool[0]
    return tuple(out)


NEW_ROWS = _new_rows()                   # rows per step of every layer, before its pooling


# ------------------------------------------------------------------------------------------------------------------ weight regimes
def _rescale_pairs(emb, layers, f):
    emb = copy.deepcopy(emb)
    for l in layers:
        g, b, m, v = emb["bn"][l]
        emb["bn"][l] = ((g * f).astype(np.float32), (b * f).astype(np.float32), m, v)
        emb["conv"][l + 1] = (emb["conv"][l + 1] / f).astype(np.float32)
    return emb


def regime(name):
    """name -> (embedding weights, head seed).  Everything but channel_cold restates tests/test_weight_regimes.py::_regime (the CPU tier
    holds the two to each other)."""
    if name.startswith("seed"):
        return W.synthetic_embedding(int(name[4:])), int(name[4:])
    base = W.synthetic_embedding(1234)
    if name == "hot":
        return _rescale_pairs(base, (1, 5, 9, 13, 17), 3.0e3), 1234
    if name == "cold":
        return _rescale_pairs(base, (1, 5, 9, 13, 17), 1.0e-4), 1234
    if name == "conv_1e-3":
        emb = copy.deepcopy(base)
        emb["conv"] = [(w * 1e-3).astype(np.float32) for w in emb["conv"]]
        return emb, 1234
    if name == "negative_bn":
        emb = copy.deepcopy(base)
        for l in (0, 2, 3, 8, 12, 18):
            g, b, m, v = emb["bn"][l]
            sgn = np.where(np.arange(g.size) % 3 == 0, -1.0, 1.0).astype(np.float32)
            emb["bn"][l] = (g * sgn, b, m, v)
        return emb, 1234
    if name in ("tiny_embedding", "huge_embedding"):
        emb = copy.deepcopy(base)
        f = 1e-4 if name == "tiny_embedding" else 1e4
        emb["conv"][19] = (emb["conv"][19] * f).astype(np.float32)
        return emb, 1234
    if name == "channel_cold":
        # every fourth channel of layers 4, 8, 12, 16 lives 2^-8 below its neighbours: one scale per LAYER has to carry both
        emb = copy.deepcopy(base)
        for l in (4, 8, 12, 16):
            g, b, m, v = emb["bn"][l]
            f = np.where(np.arange(g.size) % 4 == 0, 2.0 ** -8, 1.0).astype(np.float32)
            emb["bn"][l] = ((g * f).astype(np.float32), (b * f).astype(np.float32), m, v)
            w = emb["conv"][l + 1].copy()
            w[:, :, np.arange(g.size) % 4 == 0, :] *= np.float32(2.0 ** 8)
            emb["conv"][l + 1] = w
        return emb, 1234
    raise KeyError(name)


def heads_for(name, hseed, names=("alexa",)):
    """Heads whose first layer undoes the embedding's scale in tiny / huge_embedding (tests/test_weight_regimes.py::_heads_for)."""
    heads = {n: W.synthetic_head(n, hseed) for n in names}
    if name in ("tiny_embedding", "huge_embedding"):
        f = 1e4 if name == "tiny_embedding" else 1e-4
        for h in heads.values():
            for net in ("net", "net2"):
                if net in h:
                    h[net]["w1"] = (h[net]["w1"] * f).astype(np.float32)
    return heads


# ---------------------------------------------------------------------------------------------------------------------- inputs
PCM_NAMES = ("silence", "noise1", "noise30", "noise3000", "noise12000", "uniform_fs", "square32", "alexa", "silence_then_fs")
MEL_NAMES = ("normal", "ones", "const-6", "const12", "impulse0", "checker", "impulse15", "impulse16", "impulse31")
IMPULSE_ROW = 61                         # the row of the +8 impulse: inside all three windows, off every pooling seam of 8


def pcm_rows(alexa):
    """int16 [9, 12 * 1280], read-only: the streaming inputs.  `alexa` = the golden file's pcm/alexa_test clip."""
    r = np.random.default_rng(20261019)
    n = N_STEPS * O.CHUNK
    k = np.arange(n)
    rows = [np.zeros(n), r.normal(0, 1, n), r.normal(0, 30, n), r.normal(0, 3000, n), r.normal(0, 12000, n),
            r.integers(-32768, 32768, n), np.where((k // 16) % 2, 32767, -32767), np.resize(np.asarray(alexa, dtype=np.float64), n),
            np.where(k < 6 * O.CHUNK, 0, r.integers(-32768, 32768, n))]
    x = np.clip(np.round(np.stack(rows)), -32768, 32767).astype(np.int16)
    assert x.shape == (N_STREAMS, n) and len(PCM_NAMES) == N_STREAMS
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def mel_inputs():
    """float32 [9, 92, 32], read-only: the embed() inputs.  The checkerboard stream sits between impulse streams, so a value that
    leaks across a stream edge inside a shared tile shows in a neighbour whose own oracle is smooth."""
    r = np.random.default_rng(20261020)
    x = np.empty((N_STREAMS, ROWS, O.N_MELS), np.float64)
    x[0] = r.normal(10.0, 1.5, (ROWS, O.N_MELS))
    x[1] = 1.0
    x[2] = -6.0
    x[3] = 12.0
    x[5] = np.where((np.arange(ROWS)[:, None] + np.arange(O.N_MELS)[None, :]) % 2, 12.0, -6.0)
    for s, b in ((4, 0), (6, 15), (7, 16), (8, 31)):      # bins 15 | 16: the tile seam; 0 and 31: the two DPP zero-fill edges
        x[s] = 2.0
        x[s, IMPULSE_ROW, b] += 8.0
    assert MEL_NAMES[5] == "checker" and [MEL_NAMES[s] for s in (4, 6, 7, 8)] == ["impulse0", "impulse15", "impulse16", "impulse31"]
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def oracle_mel_of_pcm(pcm):
    """float32 [S, 92, 32]: the float64 oracle's streaming mel rows of pcm_rows() (every stream with its own clamp floor), the last 92
    of the 96 rows of the 12 steps.  The CPU tier's stand-in for the device's own rows, which the GPU tier reads with oww_get_mel."""
    import mel_budget as MB
    out = []
    for x in pcm:
        rows = np.concatenate([ref.clamped[0] for ref in MB.stream_reference(x, [1] * N_STEPS)])
        out.append(rows[-ROWS:])
    return np.stack(out).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- the float64 chain
def layers(mel_rows, emb, dtype):
    """The oracle's chain (oracle.oww_oracle: _conv, bn_fold, _activation, _pool over CNN_LAYERS) in `dtype`: mel rows [B, R, 32] ->
    (act, pre): per layer the activation and the pre-activation (the BatchNorm's output; conv19: the convolution), both [B, R_l, F, C]
    BEFORE pooling."""
    h = np.asarray(mel_rows, dtype=dtype)[..., None]
    act, pre = [], []
    for li, (kh, kw, ci, co, relu_first, bn, pool) in enumerate(O.CNN_LAYERS):
        h = O._conv(h, emb["conv"][li].astype(dtype))
        if relu_first:
            h = np.maximum(h, dtype(0))
        if bn:
            scale, shift = O.bn_fold(*emb["bn"][li], dtype=dtype)
            h = h * scale + shift
            pre.append(h)
            h = O._activation(h)
        else:
            pre.append(h)
        act.append(h)
        if pool:
            h = O._pool(h, *pool)
    return act, pre


def layers64(mel_rows, emb):
    return layers(mel_rows, emb, np.float64)


def step_rows(y, l, k, n_steps=3):
    """Rows of layer l's output y [B, R_l, ...] that are new in step k of the n_steps the input ends with (k = n_steps - 1: the last)."""
    r = NEW_ROWS[l]
    end = y.shape[1] - (n_steps - 1 - k) * r
    return y[:, end - r:end]


def ratios(got, y64):
    """[B]: max |got - y64| / max |y64| of every stream, for arrays [B, ...] of ONE layer (or one embedding window) over the rows
    compared.  A stream whose reference is identically zero admits no error; a non-finite value is an infinite error."""
    got, y64 = np.asarray(got, dtype=np.float64), np.asarray(y64, dtype=np.float64)
    assert got.shape == y64.shape, (got.shape, y64.shape)
    B = y64.shape[0]
    err = np.abs(got - y64).reshape(B, -1).max(axis=1)
    M = np.abs(y64).reshape(B, -1).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(M > 0, err / M, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(err), f, np.inf)


def fraction(got, y64):
    """max over streams of |got - y64| / (T * max |y64|): the assertion `fraction(...) <= 1` IS the budget."""
    return float(ratios(got, y64).max()) / T


def assert_within(got, y64, what):
    f = fraction(got, y64)
    assert f <= 1.0, f"{what}: |got - y64| = {f:.2f} x T * max|y64| (T = {T:.2e})"
    return f


# ------------------------------------------------------------------------------------------- emulation of the f16-split kernels
def ladder(absmax, w19):
    """calibrate_hx's scale ladder restated: per-layer maxima (before pooling) -> {'e': output exponents, 'ein': input exponents,
    'xexp': hand-over re-scales}.  Inside a stage the maxima climb 2^5 -> 2^7 -> 2^9 -> 2^11 (stage A: 2^7 .. 2^11), a pooled
    hand-over brings the next stage's input to 2^3, conv19's step puts its largest weight at 2^11 .. 2^12."""
    def ex(l):
        return int(np.frexp(np.float32(absmax[l]))[1]) if absmax[l] > 0 else 0
    cl = lambda e2: min(100, max(-100, e2))       # noqa: E731
    e, ein = [0] * N_LAYERS, [0] * N_LAYERS
    for st, first in enumerate(STAGE_FIRST):
        for i in range(3 if st == 0 else 4):
            l = first + i
            e[l] = cl((7 if st == 0 else 5) + 2 * i - ex(l))
            ein[l] = (0 if st == 0 else cl(3 - ex(l - 1))) if i == 0 else e[l - 1]
    ein[19] = cl(3 - ex(18))
    m = float(np.abs(w19).max())
    e[19] = cl(ein[19] + (cl(12 - int(np.frexp(np.float32(m))[1])) if m > 0 else cl(12)))
    xexp = [ein[last + 1] - e[last] for last in STAGE_LAST]
    return {"e": e, "ein": ein, "xexp": xexp}


def ladder_for(emb, inputs):
    """The ladder of one regime from the float64 oracle's maxima over `inputs` (a list of [B, R, 32] arrays)."""
    mx = np.zeros(N_LAYERS)
    for x in inputs:
        act, _ = layers64(x, emb)
        mx = np.maximum(mx, [float(np.abs(a).max()) for a in act])
    return ladder(mx, emb["conv"][19])


def _split(x, flush=False):
    """fp32 activations / float64 folded weights -> (hi, lo) f16 halves as fp32 arrays: hi = f16(x), lo = f16(x - hi), the difference
    taken in x's own type (exact in both)."""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16).astype(x.dtype)
        lo = (x - hi).astype(np.float16).astype(np.float32)
        hi = hi.astype(np.float32)
    if flush:
        lo = np.where(np.abs(lo) < np.float32(2.0 ** -14), np.float32(0), lo)
    return hi, lo


VARIANTS = ("floor_f16", "floor_no_K", "leak_f16", "drop_xl_wh", "shift_no_K", "lo_flush", "handover_exp", "half_tile_weights")


def variant_sites(variant):
    """(layer where the defect is made, layer where it is first seen): an early, a middle and a late site of every variant.  A hand-over
    defect after layer l is seen in layer l + 1; half channel tiles exist in the 24- and 72-channel layers only (0 .. 2, 7 .. 10)."""
    if variant == "handover_exp":
        return ((2, 3), (10, 11), (18, 19))
    if variant == "half_tile_weights":
        return ((1, 1), (8, 8), (10, 10))
    return ((1, 1), (7, 7), (18, 18))


def emulate_split(mel_rows, emb, exps, variant="", resume=None, upto=N_LAYERS - 1):
    """numpy emulation of the f16-split chain (csrc/owwhip_hx.h) on mel rows [B, R, 32] -> (per-layer activations in true units, fp32,
    before pooling; the carried input of every layer).  Layer l's activations are carried multiplied by K = 2^e[l]; activations and the
    folded weights W' = s w 2^(e - ein) (formed in float64) are split into f16 halves; the product is xh wh + xh wl + xl wh summed in
    fp32 on top of the start value K * shift; the activation is max3(0.2 acc, acc, -0.4 K) (conv0: med3(acc, K shift, +-inf) first);
    pooled hand-overs are multiplied by 2^xexp.  variant = "" is the faithful chain; "<name>@<layer>" makes ONE kernel wrong in ONE
    layer (VARIANTS).  resume = (layer, carried inputs of a faithful run) skips the layers before the defect; upto = the last layer
    evaluated."""
    name, _, at = variant.partition("@")
    at = int(at) if at else -1
    assert name == "" or name in VARIANTS
    e, ein, xexp = exps["e"], exps["ein"], exps["xexp"]
    f32 = np.float32
    out, carried = [None] * N_LAYERS, [None] * N_LAYERS
    if resume is not None:
        l0 = resume[0]
        h = resume[1][l0]
        carried[:l0] = resume[1][:l0]
    else:
        l0 = 0
        h = np.asarray(mel_rows, dtype=f32)[..., None]                  # conv0's input scale is 2^0
    for l in range(l0, upto + 1):
        kh, kw, ci, co, relu_first, bn, pool = O.CNN_LAYERS[l]
        bad = name if l == at else ""
        carried[l] = h
        K = f32(2.0) ** f32(e[l])
        w = emb["conv"][l].astype(np.float64)
        if bn:
            scale, shift = O.bn_fold(*emb["bn"][l], dtype=f32)
            w = w * scale.astype(np.float64)
        else:
            scale = shift = None
        w = w * 2.0 ** (e[l] - ein[l])                                  # (HxFold::split: the halves are cut from the float64 product)
        if bad == "half_tile_weights":
            assert co % 16 == 8
            w = w.copy()
            w[..., co - 8:] = w[..., co - 16:co - 8]
        flush = bad == "lo_flush"
        wh, wl = _split(w, flush)
        xh, xl = _split(h, flush)
        with np.errstate(over="ignore", invalid="ignore"):
            acc = O._conv(xh, wh) + O._conv(xh, wl)
            if bad != "drop_xl_wh":
                acc = acc + O._conv(xl, wh)
            if bn:
                init = shift if bad == "shift_no_K" else shift * K
                acc = acc + init
                if relu_first:
                    acc = np.where(scale >= 0, np.maximum(acc, init), np.minimum(acc, init))
                leak = f32(np.float16(0.2)) if bad == "leak_f16" else f32(0.2)
                floor = f32(np.float16(-0.4)) if bad == "floor_f16" else f32(-0.4)
                floor = floor if bad == "floor_no_K" else floor * K
                acc = np.maximum(np.maximum(leak * acc, acc), floor)
            out[l] = acc * f32(2.0) ** f32(-e[l])
            h = acc
            if pool:
                st = STAGE_LAST.index(l)
                h = O._pool(h, *pool) * f32(2.0) ** f32(xexp[st] + (1 if (name == "handover_exp" and at == l) else 0))
        assert acc.dtype == f32
    return out, carried
