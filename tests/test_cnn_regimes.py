"""The embedding CNN's kernels, layer by layer and stream by stream, against float64 over weight regimes on the relative budget of
tests/cnn_budget.py.

Every comparison is |device - y64| <= T * max|y64| per stream and layer (per embedding window), T = 4 * E32 frozen in tests/cnn_budget.py
and justified on the CPU by tests/test_cnn_budget_cpu.py; nothing here is fitted to a device result.  The float64 reference of the
streaming tests is computed from the DEVICE's own mel rows (oww_get_mel every step), so this file budgets stages A..E and conv19 alone;
the mel front ends have tests/test_mel_regimes.py.  Each test prints its worst fraction of T (DESIGN.md 5.20 records them).  No regime may
be refused at commit and range_status() stays False throughout."""
import functools

import numpy as np
import pytest

import cnn_budget as CB
from oracle import oww_oracle as O
from openwakeword_amd.engine import StreamEngine, LAYER_NEW_SHAPES

pytestmark = pytest.mark.gpu
S9 = CB.N_STREAMS
FAMILY_CASES = ([(3, n) for n in CB.ADMITTED] + [(1, n) for n in CB.REGIMES] + [(0, "seed1234"), (2, "seed1234")])


@functools.lru_cache(maxsize=None)
def _pcm():
    import os
    golden = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_streaming.npz"))
    return CB.pcm_rows(golden["pcm/alexa_test"])


@functools.lru_cache(maxsize=None)
def _weights(name):
    emb, hseed = CB.regime(name)
    return emb, CB.heads_for(name, hseed)


def _engine(name, S, **kw):
    emb, heads = _weights(name)
    return StreamEngine(S, heads, emb, **kw)         # (a refusal at commit raises OwwRangeError: no regime may be refused)


def _stream_layers(eng, S):
    """Reset, 12 one-chunk steps of the PCM rows (stream s takes row s % 9) -> (mel [S, 96, 32]: the device's own rows of all steps,
    dumps {step: [layer][S, rows, F, C]} after steps 10 and 12, features [S, 3, 96] of steps 10 .. 12)."""
    pcm = _pcm()[np.arange(S) % S9]
    eng.reset()
    mel, dumps = [], {}
    for t in range(CB.N_STEPS):
        eng.step(pcm[:, 1280 * t:1280 * (t + 1)])
        mel.append(np.stack([eng.get_mel(s, 8) for s in range(S)]))
        if t + 1 in CB.STEPS_COMPARED:
            dumps[t + 1] = [np.stack([eng.debug_layer(s, l) for s in range(S)]) for l in range(CB.N_LAYERS)]
    feats = np.stack([eng.get_features(s, 3) for s in range(S)])
    return np.concatenate(mel, axis=1), dumps, feats


def _check_layers(name, mel, dumps, feats, what):
    """Every stream, every layer, both steps, and the three embedding windows at T; -> the worst fraction of T."""
    emb, _ = _weights(name)
    assert mel.shape[1:] == (8 * CB.N_STEPS, 32) and np.isfinite(mel).all()
    act64, _ = CB.layers64(mel[:, -CB.ROWS:], emb)                       # rows 4 .. 95: the windows of steps 10, 11, 12
    worst = 0.0
    for step, k in zip(CB.STEPS_COMPARED, (0, 2)):
        for l in range(CB.N_LAYERS):
            got = dumps[step][l]
            assert got.shape[1:] == LAYER_NEW_SHAPES[l]
            worst = max(worst, CB.assert_within(got, CB.step_rows(act64[l], l, k), f"{what}: layer {l} after step {step}"))
    e64 = act64[19].reshape(-1, 3, 96)
    for k in range(3):
        worst = max(worst, CB.assert_within(feats[:, k], e64[:, k], f"{what}: embedding of step {10 + k}"))
    return worst


@pytest.mark.parametrize("family,name", FAMILY_CASES, ids=[f"mfma{f}-{n}" for f, n in FAMILY_CASES])
def test_layers_every_stream(family, name):
    """9 streams (one 8-stream stage-E tile and the start of the next), 12 steps, every layer of every stream after steps 10 and 12."""
    eng = _engine(name, S9, use_mfma=family, debug_layers=True)
    try:
        mel, dumps, feats = _stream_layers(eng, S9)
        worst = _check_layers(name, mel, dumps, feats, f"{name}, use_mfma = {family}")
        assert eng.range_status() is False
    finally:
        eng.close()
    print(f"\n{name}, use_mfma = {family}: worst |layer - float64| = {worst:.3f} T")


def test_the_regime_the_split_cannot_carry_is_not_refused():
    """channel_cold (channels of one layer 2^8 apart) is outside the f16-split table: the faithful emulation leaves T there
    (cnn_budget.NOT_ADMITTED).  The default family must still take the weights, stay finite and raise no range flag; its figure is
    printed, and the exact family is held to T on the same weights above."""
    (name, predicted), = CB.NOT_ADMITTED.items()
    eng = _engine(name, S9, debug_layers=True)
    try:
        mel, dumps, feats = _stream_layers(eng, S9)
        assert eng.range_status() is False
    finally:
        eng.close()
    emb, _ = _weights(name)
    act64, _ = CB.layers64(mel[:, -CB.ROWS:], emb)
    worst = 0.0
    for step, k in zip(CB.STEPS_COMPARED, (0, 2)):
        for l in range(CB.N_LAYERS):
            assert np.isfinite(dumps[step][l]).all()
            worst = max(worst, CB.fraction(dumps[step][l], CB.step_rows(act64[l], l, k)))
    assert np.isfinite(feats).all()
    print(f"\n{name}, use_mfma = 3 (not admitted, emulation {predicted:.1f} T): worst |layer - float64| = {worst:.2f} T")


@pytest.mark.parametrize("S", [1, 33])
@pytest.mark.parametrize("family", [3, 1])
def test_stream_positions(family, S):
    """Seed 1234 at one stream (every tile's tail empty) and at 33 (across the 32-stream padding of the state arrays)."""
    eng = _engine("seed1234", S, use_mfma=family, debug_layers=True)
    try:
        mel, dumps, feats = _stream_layers(eng, S)
        worst = _check_layers("seed1234", mel, dumps, feats, f"S = {S}, use_mfma = {family}")
        assert eng.range_status() is False
    finally:
        eng.close()
    print(f"\nseed1234, S = {S}, use_mfma = {family}: worst |layer - float64| = {worst:.3f} T")


@pytest.mark.parametrize("name", ["seed1234", "cold"])
def test_debug_and_production_kernels_agree_bit_for_bit(name):
    """The layer dumps come from the DBG = true instantiations; the steps of a handle without debug_layers run DBG = false.  Same
    weights, same PCM: the feature rings carry the same bits for every stream."""
    dbg, prod = _engine(name, S9, debug_layers=True), _engine(name, S9)
    try:
        pcm = _pcm()
        dbg.reset(); prod.reset()
        for t in range(CB.N_STEPS):
            x = pcm[:, 1280 * t:1280 * (t + 1)]
            dbg.step(x); prod.step(x)
        for s in range(S9):
            a, b = dbg.get_features(s, 16), prod.get_features(s, 16)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: stream {s} ({CB.PCM_NAMES[s]}) differs between the two builds"
        assert dbg.range_status() is False and prod.range_status() is False
    finally:
        dbg.close(); prod.close()
    print(f"\n{name}: debug_layers and production handles bit-identical over {S9} streams x 16 feature rows")


EMBED_CASES = [(3, n) for n in CB.ADMITTED] + [(1, n) for n in CB.REGIMES]


@pytest.mark.parametrize("family,name", EMBED_CASES, ids=[f"mfma{f}-{n}" for f, n in EMBED_CASES])
def test_embed_windows_on_the_relative_budget(family, name):
    """oww_embed on the mel-row inputs (three windows each) against embedding_stage in float64, per window at T * max|e64|: every stream
    -- the checkerboard between the impulse streams included -- against its own oracle."""
    emb, _ = _weights(name)
    x = CB.mel_inputs()
    want = np.stack([O.embedding_stage(x[:, 8 * k:8 * k + O.MEL_WINDOW], emb, np.float64).reshape(S9, O.EMB_DIM) for k in range(3)], axis=1)
    eng = _engine(name, S9, use_mfma=family)
    try:
        got = eng.embed(x)
        assert eng.range_status() is False
    finally:
        eng.close()
    assert got.shape == (S9, 3, O.EMB_DIM)
    worst, scale = 0.0, float(np.abs(want).max())
    for s in range(S9):
        for k in range(3):
            worst = max(worst, CB.assert_within(got[s:s + 1, k], want[s:s + 1, k], f"{name}, use_mfma = {family}: {CB.MEL_NAMES[s]}, window {k}"))
    print(f"\n{name}, use_mfma = {family}: embed() worst |e - e64| = {worst:.3f} T on |e| <= {scale:.3g}")
