"""The wake-word head kernels against the FLOAT64 oracle over head-weight regimes, and the edges of their stream tiles.

tests/test_weight_regimes.py moves the embedding CNN's weights and tests/test_vad_regimes.py the VAD's; here the heads' own weights
move.  Every regime is weights.synthetic_head rescaled so that the float64 score stays the same (a power of two on one layer, its
inverse on the layer that consumes it: ReLU is positively homogeneous, LayerNorm's output is linear in gamma / beta) or changes in a
way float64 simply follows (a larger bias, a larger output layer), so the name of a failing case says which quantity the kernel
lost.  The fixed heads are compared through StreamEngine.head() on external features -- no CNN runs --, the bank heads through the
float64 bank oracle (tests/bank_oracle.py) the way tests/test_head_bank_gpu.py does.

Contract per (kernel form, regime): every score finite and within TOL_SCORE = 1e-4 of O.head_stage(..., float64) with the range flag
down.  Only `overflow` (ln1 gamma x 1e6) may instead be refused loudly: an OwwRangeError at construction / bank_add that names
use_mfma = 1, or a raised range flag.  A regime is admitted only if the fp32 oracle itself stays within FP32_CAP = 2.5e-5 of float64
on the same inputs (test_regimes_are_admissible, CPU tier): what fp32 cannot carry is not asked of the device.  Measured on the CPU,
fp32 against float64 over every shape and regime below: 8.8e-6 at most (`saturated`, hidden 64), so a miss on the device is the kernel's.
`bias_dominant` is b1 x 32, softened from x 100: at x 100 the float64 scores of the 128-unit draw span 0.005 over the 37 rows (0.054
at x 50, 0.74 at x 32) and the comparison would show nothing.  The bank heads sit behind the CNN, whose synthetic embeddings pin a
random head near 0 or 1 on every stream, so each gets its output bias centred on the eight streams' median logit (_bank_head_cached).

What the file is for: the narrow fp16-split form (heads_hx_kernel HT = 4, the narrow heads_bank_kernel) hands its hidden vector to
the second GEMM through the f16 hi / lo split with no scale of its own.  A numpy emulation of that split on this file's heads and
rows (layer 1 exact, f16 subnormals kept) gives, for the hidden vector in true units, 5.5e-5 at ln1_cold_m10, 2.6e-4 at ln1_cold_m13,
4.2e-4 at noln_cold_m13 and an f16 overflow at noln_hot_p10; with the largest hidden unit at 2^9 .. 2^10 (owwhip.hip: hx_hidden_exp,
folded into the weights at commit / bank_add) 1.5e-7 in all of them.  DESIGN.md 5.17 holds the table.  pytest -m gpu -s prints the
branch and the worst error of every (form, regime)."""
import copy
import functools

import numpy as np
import pytest

from oracle import oww_oracle as O
from openwakeword_amd import weights as W
from openwakeword_amd._lib import OwwError, OwwRangeError
from openwakeword_amd.engine import StreamEngine

from bank_oracle import BankOracle

TOL_SCORE = 1e-4             # the project's score tolerance
FP32_CAP = 2.5e-5            # admission: |fp32 oracle - float64 oracle| on the same inputs
N_ROWS = 37                  # one full 32-stream wave plus a partly filled tile
ZERO_ROW, LOUD_ROW = 5, 20   # an all-zero feature window; one at 30 x the scale
EMB_SEED = 1234
MAX_HEADS, MAX_LABELS = 16, 32           # include/owwhip.h: OWW_MAX_HEADS, OWW_MAX_LABELS

LN64 = dict(kind="binary", T=16, hidden=64, n_out=1, layernorm=True)
# kernel form -> family (use_mfma), how it is reached, the head shape
FORMS = {
    "hx_narrow64_ln": dict(fam=3, shape=LN64),
    "hx_narrow64_noln": dict(fam=3, shape=dict(LN64, layernorm=False)),
    "hx_narrow32pad_ln": dict(fam=3, shape=dict(LN64, hidden=32)),
    "hx_narrow32pad_noln": dict(fam=3, shape=dict(LN64, hidden=32, layernorm=False)),
    "hx_wide128_ln": dict(fam=3, shape=dict(LN64, hidden=128)),
    "hx_wide128_multi7": dict(fam=3, shape=dict(kind="multiclass", T=34, hidden=128, n_out=7, layernorm=False)),
    "hx_gated64_ln": dict(fam=3, shape=dict(LN64, kind="gated")),
    "fp32_heads64_ln": dict(fam=1, shape=LN64),
    "fp32_heads64_noln": dict(fam=1, shape=dict(LN64, layernorm=False)),
    "generic_spw4_h96x2_ln": dict(fam=3, spw=4, shape=dict(LN64, hidden=96, n_blocks=2)),
    "generic_spw16_h96x2_ln": dict(fam=3, spw=16, shape=dict(LN64, hidden=96, n_blocks=2)),
    "bank_ht4_ln": dict(bank=True, shape=LN64),
    "bank_ht4_noln": dict(bank=True, shape=dict(LN64, hidden=32, layernorm=False)),
    "bank_ht8_ln": dict(bank=True, shape=dict(LN64, hidden=128)),
    "bank_ht8_noln": dict(bank=True, shape=dict(LN64, hidden=100, layernorm=False)),
}
SEEDS = ("seed1", "seed2", "seed3", "seed4")
COLD = {"m7": 2.0 ** -7, "m10": 2.0 ** -10, "m13": 2.0 ** -13}          # 2^-13 = 1.2e-4
HOT = {"p6": 2.0 ** 6, "p10": 2.0 ** 10}
_FACTORS = {**COLD, **HOT}


def regimes_of(shape):
    """The regimes that exist for a head shape, `overflow` last."""
    cold_hot = lambda stem: tuple(f"{stem}_cold_{k}" for k in COLD) + tuple(f"{stem}_hot_{k}" for k in HOT)   # noqa: E731
    if shape["layernorm"]:
        out = SEEDS + cold_hot("ln1") + cold_hot("ln2") + ("bias_dominant", "dead_units")
    else:
        out = SEEDS + cold_hot("noln")
    out += ("softmax_large",) if shape["kind"] == "multiclass" else ("saturated",)
    return out + (("overflow",) if shape["layernorm"] else ())


def _shape_key(shape):
    return tuple(sorted(shape.items()))


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _rescale(net, name):
    """One net of a head under regime `name` (in place).  Powers of two: exact in fp32."""
    H = net["w1"].shape[1]
    stem = name.rsplit("_", 1)[0]
    if stem in ("ln1_cold", "ln1_hot"):                 # layer-1 activations x f: ln1 gamma, beta x f, w2 / f
        f = _FACTORS[name.rsplit("_", 1)[1]]
        net["ln1"] = (_f32(net["ln1"][0] * f), _f32(net["ln1"][1] * f))
        net["w2"] = _f32(net["w2"] / f)
    elif stem in ("ln2_cold", "ln2_hot"):               # the first hidden block's activations x f, its consumer / f
        f = _FACTORS[name.rsplit("_", 1)[1]]
        net["ln2"] = (_f32(net["ln2"][0] * f), _f32(net["ln2"][1] * f))
        if net.get("more"):
            net["more"][0]["w"] = _f32(net["more"][0]["w"] / f)
        else:
            net["w3"] = _f32(net["w3"] / f)
    elif stem in ("noln_cold", "noln_hot"):             # no LayerNorm: w1, b1 x f, w2 / f
        f = _FACTORS[name.rsplit("_", 1)[1]]
        net["w1"], net["b1"], net["w2"] = _f32(net["w1"] * f), _f32(net["b1"] * f), _f32(net["w2"] / f)
    elif name == "bias_dominant":                       # LayerNorm sees a vector that its bias dominates (x 32: see the module docstring)
        net["b1"] = _f32(net["b1"] * 32.0)
    elif name == "dead_units":                          # half of the ReLUs never open (|LayerNorm output| < sqrt(H) gamma < 14)
        b = net["ln1"][1].copy()
        b[: H // 2] = -20.0
        net["ln1"] = (net["ln1"][0], _f32(b))
    elif name == "saturated":                           # logits beyond +-40: scores exactly 0 or 1 in fp32
        net["w3"] = _f32(net["w3"] * 16.0)
    elif name == "softmax_large":
        net["w3"] = _f32(net["w3"] * 50.0)
    elif name == "overflow":                            # hidden units of order 1e6: beyond the f16 range in true units
        net["ln1"] = (_f32(net["ln1"][0] * 1e6), net["ln1"][1])
    else:
        raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _head_cached(key, name):
    shape = dict(key)
    seed = int(name[4:]) if name.startswith("seed") else 11
    h = W.synthetic_head(f"regime_{shape['hidden']}", seed, **shape)
    if not name.startswith("seed"):
        for net in ("net", "net2"):
            if net in h:
                _rescale(h[net], name)
    return h


def make_head(shape, name):
    return copy.deepcopy(_head_cached(_shape_key(shape), name))


@functools.lru_cache(maxsize=None)
def features(T, n_rows=N_ROWS):
    """float32 [n_rows, T, 96]: normal(0, 2), one all-zero window, one at 30 x the scale (fixed seed, read-only)."""
    ft = np.random.default_rng(700 + T).normal(0.0, 2.0, (n_rows, T, 96)).astype(np.float32)
    ft[ZERO_ROW] = 0.0
    ft[LOUD_ROW] *= 30.0
    ft.setflags(write=False)
    return ft


@functools.lru_cache(maxsize=None)
def _want_cached(key, name, dtype):
    shape = dict(key)
    out = O.head_stage(features(shape["T"]), _head_cached(key, name), np.dtype(dtype).type).astype(np.float64)
    out.setflags(write=False)
    return out


def want(shape, name, dtype=np.float64):
    return _want_cached(_shape_key(shape), name, np.dtype(dtype).name)


# ------------------------------------------------------------------------------------------------ 0. admission (CPU tier)
_SHAPES = {_shape_key(f["shape"]): f["shape"] for f in FORMS.values()}
_SHAPE_CASES = [(s, r) for s in _SHAPES.values() for r in regimes_of(s)]


def _shape_id(s):
    return f"{s['kind']}{s['hidden']}x{s.get('n_blocks', 1)}_{'ln' if s['layernorm'] else 'noln'}"


@pytest.mark.parametrize("shape,name", _SHAPE_CASES, ids=[f"{_shape_id(s)}-{r}" for s, r in _SHAPE_CASES])
def test_regimes_are_admissible(shape, name):
    """The cap that keeps the device test honest: a regime is asked of the kernels only if the fp32 oracle stays within 2.5e-5 of
    float64 on the same inputs, and only if its float64 scores move with the input (except `saturated`, which must pin them)."""
    w64, w32 = want(shape, name), want(shape, name, np.float32)
    assert np.isfinite(w64).all() and np.isfinite(w32).all()
    err = float(np.abs(w32 - w64).max())
    print(f"\n{_shape_id(shape)} {name}: |fp32 - float64| = {err:.2e}, float64 scores span {np.ptp(w64):.3f}")
    assert err <= FP32_CAP
    if name == "saturated":
        assert (np.minimum(w64, 1.0 - w64) < 1e-12).sum() >= N_ROWS // 2          # (logits beyond +-27)
    else:
        assert np.ptp(w64) > 0.05
    if shape["kind"] == "multiclass":
        np.testing.assert_allclose(w64.sum(axis=1), 1.0, atol=1e-12)
    if name.startswith("seed"):
        return
    # the rescalings that claim to leave float64 alone do
    stem = name.rsplit("_", 1)[0]
    if stem in ("ln1_cold", "ln1_hot", "ln2_cold", "ln2_hot", "noln_cold", "noln_hot"):
        base = O.head_stage(features(shape["T"]), W.synthetic_head(f"regime_{shape['hidden']}", 11, **shape), np.float64)
        assert np.abs(base - w64).max() < 1e-6


_BANK_CASES = [(f, r) for f, spec in FORMS.items() if spec.get("bank") for r in regimes_of(spec["shape"])]


@pytest.mark.parametrize("form,name", _BANK_CASES, ids=[f"{f}-{r}" for f, r in _BANK_CASES])
def test_bank_regimes_are_admissible(form, name):
    """The same cap for the bank comparison, which runs behind the CNN: the all-fp32 bank oracle (CNN included) within 2.5e-5 of the
    float64 one over the eight streams, whose float64 scores differ from stream to stream."""
    shape = FORMS[form]["shape"]
    w64, w32 = bank_want(shape)[name], bank_want(shape, np.float32)[name]
    err = float(np.abs(w32 - w64).max())
    print(f"\n{form} {name}: |fp32 - float64| = {err:.2e}, float64 scores span {np.ptp(w64):.3f}")
    assert np.isfinite(w32).all() and err <= FP32_CAP
    if name != "saturated":
        assert np.ptp(w64) > 0.05


# ------------------------------------------------------------------------------------------------ 1. the device, form by form
@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(EMB_SEED)


def _chunks(shape, names):
    per = max(1, min(MAX_HEADS, MAX_LABELS // shape["n_out"]))
    return [names[i:i + per] for i in range(0, len(names), per)]


def _run_fixed(form, names):
    """Heads `names` of one form in one engine -> {name: (branch, scores or None, text)}.  An engine that refuses several heads at once
    is taken apart into one engine per head, so that a refusal carries the regime's name."""
    shape, ft = form["shape"], features(form["shape"]["T"])
    heads = {n: make_head(shape, n) for n in names}
    try:
        eng = StreamEngine(8, heads, _emb(), use_mfma=form["fam"])
    except OwwError as e:
        if len(names) == 1:
            return {names[0]: ("refused at construction", None, str(e))}
        out = {}
        for n in names:
            out.update(_run_fixed(form, [n]))
        return out
    out = {}
    try:
        for n in names:
            try:
                got = eng.head(n, ft)
            except OwwRangeError as e:
                out[n] = ("range flag", None, str(e))
                eng.range_status(clear=True)
                continue
            out[n] = ("range flag" if eng.range_status(clear=True) else "numeric", got.astype(np.float64), "")
    finally:
        eng.close()
    return out


BANK_STEPS = 6               # the sixth prediction is the first that Model.predict does not zero (model.py:331-333)


@functools.lru_cache(maxsize=None)
def _bank_inputs():
    """Eight streams: int16 PCM [8, 6 * 1280] and the feature rows each starts from, float32 [8, 16, 96] -- normal(0, 2), stream 0 all
    zero, stream 1 at 30 x the scale.  After six steps a 16-row window holds ten of them and six rows of the CNN."""
    r = np.random.default_rng(41)
    init = r.normal(0.0, 2.0, (8, 16, 96)).astype(np.float32)
    init[0] = 0.0
    init[1] *= 30.0
    pcm = W.synthetic_pcm(8, 1280 * BANK_STEPS, seed=42)
    return pcm, init


@functools.lru_cache(maxsize=None)
def _bank_windows():
    """float64 [8, 16, 96]: the feature rows the float64 front end holds for each stream at the sixth step."""
    pcm, init = _bank_inputs()
    proto = O.OracleAudioFeatures(_emb(), dtype=np.float64, init_noise=np.zeros(16000, np.int16))
    out = np.zeros((8, 16, 96))
    for s in range(8):
        p = copy.deepcopy(proto)
        p.features = init[s].astype(np.float64)
        for t in range(BANK_STEPS):
            p(pcm[s, 1280 * t:1280 * (t + 1)])
        out[s] = p.get_features(16)[0]
    return out


@functools.lru_cache(maxsize=None)
def _bank_head_cached(key, name):
    """The regime's head with its output bias moved by minus the median float64 logit of the eight streams: behind the synthetic CNN's
    large, static mean embedding a random head sits far from 0.5 on every stream (weights.py does the same for its seed-1234 heads;
    tests/test_head_bank_gpu.py: _random_bank), and a comparison of scores that are all 1e-9 would show nothing."""
    h = copy.deepcopy(_head_cached(key, name))
    z = O._mlp(_bank_windows(), h["net"], np.float64)[:, 0]
    h["net"]["b3"] = _f32(h["net"]["b3"] - np.median(z))
    return h


@functools.lru_cache(maxsize=None)
def _bank_want_cached(key, dtype):
    """{regime: [8]}: what tests/bank_oracle.py scores at the sixth step for a stream subscribed to every regime's head at once."""
    names = regimes_of(dict(key))
    pcm, init = _bank_inputs()
    dt = np.dtype(dtype).type
    proto = BankOracle({i: _bank_head_cached(key, n) for i, n in enumerate(names)}, _emb(), len(names), dtype=dt, init_noise=np.zeros(16000, np.int16))
    out = np.zeros((8, len(names)))
    for s in range(8):
        o = copy.deepcopy(proto)
        o.preprocessor.features = init[s].astype(dt)
        o.subscribe(range(len(names)))
        for t in range(BANK_STEPS):
            out[s] = o.predict(pcm[s, 1280 * t:1280 * (t + 1)])[1]
    out.setflags(write=False)
    return {n: out[:, i] for i, n in enumerate(names)}


def bank_want(shape, dtype=np.float64):
    return _bank_want_cached(_shape_key(shape), np.dtype(dtype).name)


def _bank_round(eng, ids):
    """Every stream subscribed to the bank heads `ids` from a fresh start, six steps -> device scores [8, len(ids)]."""
    pcm, init = _bank_inputs()
    sub = np.full((8, eng.bank_slots), -1, np.int32)
    sub[:, :len(ids)] = ids
    eng.subscribe(np.arange(8), np.full_like(sub, -1))              # (every slot restarts, whatever it held)
    for s in range(8):
        eng.reset([s], init[s])
    eng.subscribe(np.arange(8), sub)
    for t in range(BANK_STEPS):
        eng.step(pcm[:, 1280 * t:1280 * (t + 1)])
    return eng.bank_scores()[:, :len(ids)].astype(np.float64)


def _run_bank(form):
    shape = form["shape"]
    names = list(regimes_of(shape))
    ref = bank_want(shape)
    out = {}
    eng = StreamEngine(8, {}, _emb(), bank_slots=8, bank_capacity=len(names))
    try:
        ids = {}
        for n in names:
            try:
                ids[n] = eng.bank_add(_bank_head_cached(_shape_key(shape), n))
            except OwwError as e:
                out[n] = ("refused at bank_add", None, None, str(e))
        todo = [n for n in names if n in ids and n != "overflow"]
        rounds = [todo[i:i + 8] for i in range(0, len(todo), 8)] + ([["overflow"]] if "overflow" in ids else [])
        while rounds:
            rnd = rounds.pop(0)
            try:
                got = _bank_round(eng, [ids[n] for n in rnd])
                flag = eng.range_status(clear=True)
            except OwwRangeError as e:
                eng.range_status(clear=True)
                if len(rnd) > 1:                        # which head raised it: one round per head
                    rounds = [[n] for n in rnd] + rounds
                    continue
                out[rnd[0]] = ("range flag", None, None, str(e))
                continue
            if flag and len(rnd) > 1:
                rounds = [[n] for n in rnd] + rounds
                continue
            for k, n in enumerate(rnd):
                out[n] = ("range flag" if flag else "numeric", got[:, k], ref[n], "")
    finally:
        eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _results(form_name):
    form = FORMS[form_name]
    if form.get("bank"):
        return _run_bank(form)
    names = [n for n in regimes_of(form["shape"]) if n != "overflow"]
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        if form.get("spw"):
            mp.setenv("OWW_GENERIC_SPW", str(form["spw"]))          # (read at commit: pins heads_generic_kernel's shape)
        else:
            mp.delenv("OWW_GENERIC_SPW", raising=False)
        for chunk in _chunks(form["shape"], names):
            out.update(_run_fixed(form, chunk))
        if "overflow" in regimes_of(form["shape"]):
            out.update(_run_fixed(form, ["overflow"]))
    return {n: (b, g, None if g is None else want(form["shape"], n), t) for n, (b, g, t) in out.items()}


_DEVICE_CASES = [(f, r) for f, spec in FORMS.items() for r in regimes_of(spec["shape"])]


@pytest.mark.gpu
@pytest.mark.parametrize("form,name", _DEVICE_CASES, ids=[f"{f}-{r}" for f, r in _DEVICE_CASES])
def test_heads_match_float64_or_are_loud(form, name):
    """One of: every score finite and within 1e-4 of float64 with the range flag down; or -- `overflow` only -- a refusal that names
    use_mfma = 1, or a raised range flag.  Prints the branch and the worst |device - float64| of every (form, regime)."""
    shape = FORMS[form]["shape"]
    branch, got, ref, text = _results(form)[name]
    if branch != "numeric":
        print(f"\n{form} {name}: branch = {branch} ({text[:160]})")
        assert name == "overflow", f"{form} {name}: only `overflow` may be refused, this was: {branch}: {text}"
        assert FORMS[form].get("fam", 3) == 3, "the exact-fp32 family has no f16 range to leave"
        if branch.startswith("refused"):
            assert "use_mfma = 1" in text
        return
    assert np.isfinite(got).all(), f"{form} {name}: non-finite score with no error raised: {got}"
    err = np.abs(got - ref)
    worst = float(err.max())
    print(f"\n{form} {name}: branch = numeric, max |device - float64| = {worst:.2e} (row {int(np.argmax(err.max(axis=-1) if err.ndim > 1 else err))})")
    if name != "saturated":
        assert np.ptp(ref) > 0.05
    assert worst <= TOL_SCORE
    if shape["kind"] == "multiclass":
        np.testing.assert_allclose(got.sum(axis=1), 1.0, atol=1e-5)
    if name == "saturated" and not FORMS[form].get("bank"):
        assert (np.minimum(got, 1.0 - got) <= TOL_SCORE).sum() >= N_ROWS // 2


# ------------------------------------------------------------------------------------------------ 2. tile edges, bit for bit
EDGE_FORMS = ("hx_narrow64_ln", "hx_wide128_ln", "hx_wide128_multi7", "generic_spw4_h96x2_ln", "generic_spw16_h96x2_ln")
EDGE_ROWS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129)


@pytest.mark.gpu
@pytest.mark.parametrize("form", EDGE_FORMS)
def test_tile_edges_bit_for_bit(form, monkeypatch):
    """16 streams per MFMA tile, 32 per wave, 128 per workgroup (generic kernel: 4 or 16 per wave): head() on the first n rows must
    return exactly the first n rows of the 129-row call, and a row's bits must not depend on whether its tile neighbours are the
    all-zero window or the 30 x one."""
    spec = FORMS[form]
    shape = spec["shape"]
    if spec.get("spw"):
        monkeypatch.setenv("OWW_GENERIC_SPW", str(spec["spw"]))
    else:
        monkeypatch.delenv("OWW_GENERIC_SPW", raising=False)
    head = make_head(shape, "seed1")
    ft = features(shape["T"], 129)
    eng = StreamEngine(8, {"h": head}, _emb(), use_mfma=spec["fam"])
    try:
        full = eng.head("h", ft)
        ref = O.head_stage(ft, head, np.float64)
        assert np.abs(full - ref).max() <= TOL_SCORE
        for n in EDGE_ROWS:
            got = eng.head("h", ft[:n])
            assert np.array_equal(got, full[:n]), f"{form}: {n} rows differ from the leading rows of 129 at {np.nonzero((got != full[:n]).any(axis=1))[0].tolist()}"
        for parity in (0, 1):
            keep = np.arange(129) % 2 == parity
            for label, fill in (("all-zero", ZERO_ROW), ("30 x", LOUD_ROW)):
                other = np.array(ft)
                other[~keep] = ft[fill]
                got = eng.head("h", other)
                moved = np.nonzero((got[keep] != full[keep]).any(axis=1))[0]
                assert moved.size == 0, f"{form}: rows {np.nonzero(keep)[0][moved].tolist()} change when their neighbours become {label}"
        assert eng.range_status() is False
    finally:
        eng.close()
