"""The voice-activity kernels (openwakeword_amd/csrc/owwhip_vad.h) against the FLOAT64 stand-in over weight regimes, PCM extremes,
a recurrence long enough to wrap every ring, and the edges of the 16-stream LSTM tile.

The VAD runs on the same f16-split MFMAs as the embedding CNN, but with one fixed weight scale (owh::WSCALE = 2^8), activations
in true units, no calibration and no commit-time self-test.  tests/test_weight_regimes.py holds the CNN to "agree with float64
or be refused loudly"; this file holds the VAD to the same rule.  Every comparison is StreamEngine.get_vad() after each step
against one oracle.oww_oracle.OracleVad(StandinVadSession(w, dtype=float64)) per stream, at the project's TOL_VAD = 1e-4.

How far the reference itself is from float64 (fp32 restatement against the float64 one, same regimes, same eight PCM rows):
3.9e-7 at most over all regimes below (`overflow`: 3.0e-7; 150 frames at seed 1234: 3.3e-7) -- 250x inside TOL_VAD, so a miss is
the kernel's.  A regime that is deliberately absent: LSTM weights x 8 (saturating gates) make the recurrence chaotic -- fp32 and
float64 restatements of the same network are 0.96 apart after 40 frames, and no tolerance means anything there."""
import copy
import functools

import numpy as np
import pytest

from oracle import oww_oracle as O
from oracle import parity_sample as PS
from oracle import vad_standin as V
from openwakeword_amd import weights as W
from openwakeword_amd._lib import OwwError, OwwRangeError
from openwakeword_amd.engine import StreamEngine

pytestmark = pytest.mark.gpu
TOL_VAD = 1e-4
TOL_SCORE = 1e-4
N_ROWS = 8
F16_LIMIT = 65520.0          # the first fp32 value that rounds to an f16 infinity (owwhip_hx.h: nan_guard)


@functools.lru_cache(maxsize=None)
def _pcm(n_frames):
    """int16 [8, n_frames * 1280], one row per stream: silence, LSB noise, quiet / normal / clipped noise, full-range uniform, a
    full-scale square wave of period 32 and a constant +32767 (fixed seed, as tests/test_weight_regimes.py::_pcm)."""
    r = np.random.default_rng(99)
    n = n_frames * 1280
    rows = [np.zeros(n), r.integers(-3, 4, n), r.normal(0, 30, n), r.normal(0, 3000, n), r.integers(-32768, 32768, n),
            np.where((np.arange(n) // 16) % 2, 32767, -32768), r.normal(0, 12000, n), np.full(n, 32767)]
    x = np.clip(np.round(np.stack(rows)), -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return x


def _compensated(w, layer, f):
    """Encoder layer `layer`'s weights and bias times f, its consumer's input weights (the next encoder layer, or rows [:64] of
    lstm[0] behind the last one) divided by f.  f is a power of two: every rescale is exact in fp32, ReLU is positively
    homogeneous, so the float64 network is the same up to round-off -- only that layer's activations live a factor f away."""
    w = copy.deepcopy(w)
    cw, cb = w["enc"][layer]
    w["enc"][layer] = ((cw * f).astype(np.float32), (cb * f).astype(np.float32))
    if layer < 3:
        nw, nb = w["enc"][layer + 1]
        w["enc"][layer + 1] = ((nw / f).astype(np.float32), nb)
    else:
        lw, lb = w["lstm"][0]
        lw = lw.copy()
        lw[:64] /= f
        w["lstm"][0] = (lw.astype(np.float32), lb)
    return w


SEEDS = ("seed1", "seed2", "seed3", "seed1234")
HOT_COLD = tuple(f"{k}_{l}" for k in ("hot", "cold") for l in range(4))
REGIMES = SEEDS + HOT_COLD + ("overflow",)


@functools.lru_cache(maxsize=None)
def _regime(name):
    if name.startswith("seed"):
        return W.synthetic_vad(int(name[4:]))
    base = W.synthetic_vad(1234)
    if name.startswith("hot_"):          # layer l's activations x 64 (below about 360), its weights below 48
        return _compensated(base, int(name[4:]), 64.0)
    if name.startswith("cold_"):         # ... / 64: weights near 1e-4 keep few bits in an unscaled f16 low half
        return _compensated(base, int(name[5:]), 1.0 / 64.0)
    if name == "overflow":
        # Every encoder layer's INPUT stays inside the f16 range (so vad_front_kernel's own guards see nothing), but the last
        # layer's OUTPUT -- finite fp32 in the tiles the LSTM kernel reads -- reaches 1.41e5 on the loud rows: layer 2 x 256 (its
        # bias unchanged, nothing compensated in layer 3), layer 3 weights x 128 and bias x 32768, lstm[0]'s input rows / 32768.
        # The float64 network stays tame (largest weight 138.7, loader limit 253.9); the LSTM kernel's f16 split of its input does not.
        w = copy.deepcopy(base)
        cw, cb = w["enc"][2]
        w["enc"][2] = ((cw * 256.0).astype(np.float32), cb)
        cw, cb = w["enc"][3]
        w["enc"][3] = ((cw * 128.0).astype(np.float32), (cb * 32768.0).astype(np.float32))
        lw, lb = w["lstm"][0]
        lw = lw.copy()
        lw[:64] /= 32768.0
        w["lstm"][0] = (lw.astype(np.float32), lb)
        return w
    raise KeyError(name)


def _encoder_max64(w, x):
    """max over everything of the float64 encoder output for int16 PCM x [B, 1280 * k] -> [B]."""
    worst = np.zeros(x.shape[0])
    for i in range(0, x.shape[1], 640):
        a = V.stft_features((x[:, i:i + 640] / 32767).astype(np.float32), np.float64)
        for (cw, cb), (_, _, stride) in zip(w["enc"], V.ENC):
            a = np.maximum(V.conv1d_k3(a, cw.astype(np.float64), cb.astype(np.float64), stride), 0)
        worst = np.maximum(worst, a.reshape(x.shape[0], -1).max(axis=1))
    return worst


@functools.lru_cache(maxsize=None)
def _oracle_scores(name, n_frames):
    """float64 [n_frames, 8]: what OracleVad appends per frame for the eight rows under regime `name` (computed once, read-only)."""
    w, pcm = _regime(name), _pcm(n_frames)
    vads = [O.OracleVad(V.StandinVadSession(w, dtype=np.float64)) for _ in range(N_ROWS)]
    out = np.zeros((n_frames, N_ROWS))
    for t in range(n_frames):
        for s, v in enumerate(vads):
            v(pcm[s, t * 1280:(t + 1) * 1280])
            out[t, s] = v.ring[-1]
    out.setflags(write=False)
    return out


def _fresh_oracle_scores(w, chunks):
    """One fresh float64 OracleVad fed `chunks` ([n, 1280] int16) -> its n ring entries."""
    v = O.OracleVad(V.StandinVadSession(w, dtype=np.float64))
    out = []
    for x in chunks:
        v(x)
        out.append(float(v.ring[-1]))
    return np.array(out)


def _engine(n_streams, w, **kw):
    emb, heads = PS._weights(("alexa",))
    return StreamEngine(n_streams, heads, emb, vad=w, **kw)


# ------------------------------------------------------------------------------------------------ 1. weight regimes
@pytest.mark.parametrize("name", REGIMES)
def test_vad_matches_float64_or_is_loud(name):
    """Exactly one of: creation refuses and names the VAD; a step raises OwwRangeError; every score is finite and within TOL_VAD
    of float64 with the range flag down.  Only `overflow` may take one of the first two.  A non-finite score, or a difference
    in silence, fails.

    `overflow` is the hole this test was written for: vad_lstm_kernel consumes the encoder's fp32 output tiles through
    owh::to_ops, a value >= 65520 there becomes inf / -inf operands, the gates NaN, and NaN h, c and scores went back to the
    stream's state with oww_range_status still false.  With the kernel's nan_guard it takes the OwwRangeError branch, range_where()
    names the 16-stream tile, and after range_status(clear=True) + reset_vad() the streams score finite, correct values again.

    A numpy emulation of the split (x = xh + xl, 256 w = wh + wl in f16; xh wh + xl wh + xh wl) predicts 9e-8 .. 4e-7 for the seeds
    and hot regimes, 6e-7 .. 2.8e-6 for the cold ones, and NaN scores on rows 3-6 of `overflow` at the first frame.  The test
    prints the branch each regime took and its worst |device - float64|."""
    n_frames = 12
    w, pcm = _regime(name), _pcm(n_frames)
    want = _oracle_scores(name, n_frames)
    if name == "overflow":
        enc = _encoder_max64(w, pcm)
        print(f"\noverflow: float64 encoder output per row, max = {np.array2string(enc, precision=4)}")
        assert enc.max() > F16_LIMIT                          # the regime really leaves the f16 range (1.41e5 on the loud rows) ...
        assert enc[0] < 0.5 * F16_LIMIT                       # ... and silence does not: the recovery below is fed silence
    try:
        eng = _engine(N_ROWS, w)
    except OwwError as e:
        assert "VAD" in str(e), f"refused at creation without naming the VAD: {e}"
        assert name == "overflow", f"{name}: nothing here is near the f16 range, creation must not refuse it: {e}"
        print(f"\n{name}: branch = refused at creation ({e})")
        return
    try:
        branch, worst = "numeric", 0.0
        for t in range(n_frames):
            x = pcm[:, t * 1280:(t + 1) * 1280]
            try:
                eng.step(x)
            except OwwRangeError:
                branch = f"OwwRangeError at frame {t}"
                break
            got = eng.get_vad()
            assert np.isfinite(got).all(), f"{name} frame {t}: non-finite VAD score with no error raised: {got}"
            worst = max(worst, float(np.abs(got - want[t]).max()))
        if branch == "numeric":
            assert eng.range_status() is False
            print(f"\n{name}: branch = numeric, max |device - float64| = {worst:.2e} over {n_frames} frames x {N_ROWS} rows")
            assert worst <= TOL_VAD
            return
        print(f"\n{name}: branch = {branch}, max |device - float64| before it = {worst:.2e}")
        assert name == "overflow", f"{name}: activations stay below about 360, OwwRangeError is not an answer here"
        assert worst <= TOL_VAD
        # loud, and it says where: the eight streams share the first 16-stream tile
        assert eng.range_status() is True
        assert eng.range_where() == (0, N_ROWS)
        # the way back: clear the flag, restart the streams named -> finite scores again, equal to a fresh stream's
        assert eng.range_status(clear=True) is True
        first, count = 0, N_ROWS
        eng.reset_vad(list(range(first, first + count)))
        quiet = np.zeros((3, 1280), np.int16)
        fresh = _fresh_oracle_scores(w, quiet)
        for t in range(3):
            eng.step(np.repeat(quiet[t][None], N_ROWS, axis=0))
            got = eng.get_vad()
            assert np.isfinite(got).all(), f"after reset_vad, frame {t}: {got}"
            np.testing.assert_allclose(got, np.full(N_ROWS, fresh[t]), rtol=0, atol=TOL_VAD)
        assert eng.range_status() is False
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. PCM extremes
def test_pcm_extremes_at_the_default_weights():
    """The eight rows on their own at seed 1234, and the proof that the comparison is not vacuous: the float64 scores of the rows
    span more than 0.2 (0.065 .. 0.797 on the CPU), so silence, LSB noise, clipping and a DC rail do score differently."""
    n_frames = 12
    w, pcm = _regime("seed1234"), _pcm(n_frames)
    want = _oracle_scores("seed1234", n_frames)
    assert want.max() - want.min() > 0.2
    eng = _engine(N_ROWS, w)
    try:
        worst = np.zeros(N_ROWS)
        for t in range(n_frames):
            eng.step(pcm[:, t * 1280:(t + 1) * 1280])
            got = eng.get_vad()
            assert np.isfinite(got).all()
            worst = np.maximum(worst, np.abs(got - want[t]))
        print(f"\nPCM extremes: float64 scores {want.min():.3f} .. {want.max():.3f}; max |device - float64| per row = "
              f"{np.array2string(worst, precision=1)}")
        assert worst.max() <= TOL_VAD
        assert eng.range_status() is False
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. long recurrence
LONG_FRAMES = 150


def test_long_recurrence_wraps_every_ring():
    """150 frames = 600 LSTM time steps and 150 ring pushes: the 8-deep device ring wraps 18 times, OracleVad's 125-deep ring once.
    Every frame at TOL_VAD (fp32 against float64 restatement over the same 150 frames: 3.3e-7)."""
    w, pcm = _regime("seed1234"), _pcm(LONG_FRAMES)
    want = _oracle_scores("seed1234", LONG_FRAMES)
    eng = _engine(N_ROWS, w)
    try:
        worst, at = 0.0, 0
        for t in range(LONG_FRAMES):
            eng.step(pcm[:, t * 1280:(t + 1) * 1280])
            got = eng.get_vad()
            assert np.isfinite(got).all(), f"frame {t}"
            d = float(np.abs(got - want[t]).max())
            if d > worst:
                worst, at = d, t
        print(f"\nlong recurrence: max |device - float64| = {worst:.2e} (frame {at} of {LONG_FRAMES})")
        assert worst <= TOL_VAD
        assert eng.range_status() is False
    finally:
        eng.close()


def test_fused_gate_after_the_rings_wrapped():
    """The gate inside the step (vad_threshold = 0.5) over the same 150 frames against OracleModel with the stand-in session behind
    its VAD (model.py:366-381): after frame 125 the oracle's deque has dropped entries and the device ring has wrapped 15 times,
    and ring[-7:-4] must still be the same three frames on both sides.  Skip rule as test_fused_vad_gate_matches_oracle_model: a
    decision within 1e-3 of the threshold is not compared; those stay under 5 % of all pairs, and both branches of the gate are
    seen after frame 130."""
    thr = 0.5
    w, pcm = _regime("seed1234"), _pcm(LONG_FRAMES)
    emb, heads = PS._weights(("alexa",))
    eng = StreamEngine(N_ROWS, heads, emb, vad=w, vad_threshold=thr)
    try:
        proto = O.OracleModel(heads, emb, init_noise=PS.init_noise(), vad_threshold=thr, vad_session=V.StandinVadSession(w))
        eng.reset(None, proto.preprocessor.features[-eng.feature_ring:])
        models = [proto] + [copy.deepcopy(proto) for _ in range(N_ROWS - 1)]
        n_pairs = n_skipped = n_gated = n_open = 0
        for t in range(LONG_FRAMES):
            x = pcm[:, t * 1280:(t + 1) * 1280]
            got = eng.step(x)
            for s, m in enumerate(models):
                pred = m.predict(x[s])
                want = np.array([pred[k] for k in heads])
                n_pairs += 1
                window = list(m.vad.ring)[-7:-4]
                if window and abs(max(window) - thr) < 1e-3:
                    n_skipped += 1
                    continue
                np.testing.assert_allclose(got[s], want, rtol=0, atol=TOL_SCORE, err_msg=f"stream {s} frame {t}")
                if t > 130:
                    n_gated += int((want == 0).all())
                    n_open += int((want != 0).any())
        print(f"\nfused gate, {LONG_FRAMES} frames: {n_skipped} of {n_pairs} pairs within 1e-3 of the threshold; after frame 130: "
              f"{n_gated} gated, {n_open} open")
        assert n_skipped < 0.05 * n_pairs
        assert n_gated > 0 and n_open > 0
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. tile edges, bit for bit
EDGE_FRAMES = 6


def _run_same_input(n_streams, w, chunks):
    """Every stream fed the same chunks -> scores [n_chunks, n_streams]."""
    eng = _engine(n_streams, w)
    try:
        out = []
        for x in chunks:
            eng.step(np.repeat(x[None], n_streams, axis=0))
            out.append(eng.get_vad())
        assert eng.range_status() is False
        return np.stack(out)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _single_stream_scores():
    w = _regime("seed1234")
    chunks = _pcm(EDGE_FRAMES)[4].reshape(EDGE_FRAMES, 1280)
    got = _run_same_input(1, w, chunks)
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("n_streams", [1, 15, 16, 17, 63, 64, 65, 131])
def test_stream_counts_at_the_tile_edges(n_streams):
    """16 streams per wave, four waves per workgroup: one short of, exactly, and one past a wave's and a workgroup's worth, where
    spare waves recompute the last group without storing and the last tile is partly empty.  The same audio in every stream must
    give the same bits in every stream, and the same bits as a one-stream engine."""
    w = _regime("seed1234")
    chunks = _pcm(EDGE_FRAMES)[4].reshape(EDGE_FRAMES, 1280)
    got = _run_same_input(n_streams, w, chunks)
    one = _single_stream_scores()
    assert np.isfinite(got).all()
    differ = np.nonzero((got != got[:, :1]).any(axis=0))[0]
    assert differ.size == 0, f"streams {differ.tolist()} differ from stream 0 on identical input"
    assert np.array_equal(got[:, 0], one[:, 0]), "stream 0 differs from the one-stream engine"
    want = _fresh_oracle_scores(w, chunks)
    worst = float(np.abs(got[:, 0] - want).max())
    print(f"\nS = {n_streams}: all streams bit-identical; max |device - float64| = {worst:.2e}")
    assert worst <= TOL_VAD


def test_reset_vad_leaves_the_tile_neighbours_alone():
    """vad_reset_kernel zeroes one position of a register-dump tile with hand-written index arithmetic.  Two engines of 65 streams
    on identical input; one resets streams 15, 16, 31 and 64 (last of a tile, first of the next, last of the second, the lone
    stream of the fifth) and both run on: every other stream -- the tile neighbours 0-14, 17-30, 32-63 -- stays bit-identical
    between the two, the reset ones equal a fresh stream's scores, and reset_vad() without a list restarts everybody."""
    S, ids = 65, [15, 16, 31, 64]
    w = _regime("seed1234")
    chunks = _pcm(10)[4].reshape(10, 1280)
    a, b = _engine(S, w), _engine(S, w)
    try:
        first = []
        for x in chunks[:6]:
            xs = np.repeat(x[None], S, axis=0)
            a.step(xs); b.step(xs)
            first.append(a.get_vad())
            assert np.array_equal(first[-1], b.get_vad())
        a.reset_vad(ids)
        others = np.setdiff1d(np.arange(S), ids)
        fresh = _fresh_oracle_scores(w, chunks[6:])
        carried = _fresh_oracle_scores(w, chunks)[6:]
        assert np.abs(fresh - carried).max() > 10 * TOL_VAD          # a reset that did nothing would be seen
        worst = 0.0
        for t, x in enumerate(chunks[6:]):
            xs = np.repeat(x[None], S, axis=0)
            a.step(xs); b.step(xs)
            ga, gb = a.get_vad(), b.get_vad()
            touched = others[ga[others] != gb[others]]
            assert touched.size == 0, f"reset_vad({ids}) changed streams {touched.tolist()} (frame {t} after it)"
            assert (ga[ids] == ga[ids[0]]).all()
            worst = max(worst, float(np.abs(ga[ids] - fresh[t]).max()))
            np.testing.assert_allclose(ga[ids], np.full(len(ids), fresh[t]), rtol=0, atol=TOL_VAD)
            np.testing.assert_allclose(gb[ids], np.full(len(ids), carried[t]), rtol=0, atol=TOL_VAD)
        a.reset_vad()
        for t, x in enumerate(chunks[:2]):
            a.step(np.repeat(x[None], S, axis=0))
            assert np.array_equal(a.get_vad(), first[t]), f"reset_vad() did not restart every stream (frame {t})"
        print(f"\nreset_vad({ids}) at S = {S}: neighbours bit-identical; reset streams max |device - float64| = {worst:.2e}")
        assert a.range_status() is False and b.range_status() is False
    finally:
        a.close(); b.close()
