"""Parity of the HIP path with the CPU oracle, through the C ABI.  Needs a real MI355X:  pytest -m gpu

Tolerances (fp32 path, BASELINE north_star asks for per-frame scores within 1e-3 of the reference):
  mel rows      5e-4  in x/10+2 units  (measured ~4e-6)
  embeddings    2e-4  absolute, |e| up to ~10 (measured ~1e-5)
  scores        1e-4  (measured ~7e-6)        -> 10x inside the 1e-3 budget
"""
import numpy as np
import pytest

import cases
from oracle import oww_oracle as O
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine, LAYER_NEW_SHAPES

pytestmark = pytest.mark.gpu

TOL_MEL_DB = 5e-3
TOL_MEL = 5e-4
TOL_EMB = 2e-4
TOL_SCORE = 1e-4
HEADS3 = ["alexa", "hey_mycroft", "hey_jarvis"]


@pytest.fixture(scope="module")
def emb():
    return W.synthetic_embedding(cases.SEED_WEIGHTS)


@pytest.fixture(scope="module")
def heads():
    return {n: W.synthetic_head(n, cases.SEED_WEIGHTS) for n in HEADS3}


@pytest.fixture(scope="module", params=[1, 3, 0, 2], ids=["mfma_rr", "mfma_f16x3", "valu", "mfma_lds"])
def eng(request, emb, heads):
    e = StreamEngine(6, heads, emb, max_chunks=3, use_mfma=request.param, debug_layers=True)
    yield e
    e.close()


def oracle_streams(eng, heads, emb, S, seed0=100):
    models = []
    for s in range(S):
        noise = W.synthetic_pcm(1, 64000, seed=seed0 + s, rms=600.0)[0]
        m = O.OracleModel(heads, emb, init_noise=noise)
        models.append(m)
        eng.reset([s], m.preprocessor.features[-eng.feature_ring:])
    return models


def as_vec(pred, heads):
    return np.array([pred[k] for k in heads], dtype=np.float64)


# ------------------------------------------------------------------------------------------- stage level
@pytest.mark.parametrize("name,pcm", [
    ("noise1760", W.synthetic_pcm(3, 1760, seed=1)),
    ("noise12560", W.synthetic_pcm(2, 12560, seed=2)),
    ("full_scale", np.random.default_rng(0).integers(-32768, 32767, (2, 4000)).astype(np.int16)),
    ("lsb_noise", np.random.default_rng(1).integers(-3, 4, (1, 1760)).astype(np.int16)),
    ("zeros", np.zeros((1, 1760), np.int16)),
    ("unaligned_n", W.synthetic_pcm(2, 1999, seed=3)),
    ("minimum_n", W.synthetic_pcm(1, 512, seed=4)),
])
def test_mel_stage(eng, name, pcm):
    got = eng.mel(pcm)
    want = O.mel_stage(pcm.astype(np.float32), np.float64)[:, 0]
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=TOL_MEL_DB)


def test_mel_stage_golden_clip(eng, golden):
    got = eng.mel(golden["stage/mel_in"][None])[0]
    np.testing.assert_allclose(got, golden["stage/mel_out"], rtol=0, atol=TOL_MEL_DB)


def test_mel_rejects_non_int16(eng):
    with pytest.raises(ValueError):                       # utils.py:195-197
        eng.mel(np.zeros((1, 1760), np.float32))


def test_embedding_stage_full_window(eng, emb, golden):
    """oww_embed evaluates whole 76-row windows with the incremental kernels from scratch state: this is
    the self-check that the streaming CNN state is exact."""
    r = np.random.default_rng(5)
    mel = (golden["stage/mel_out"] / 10 + 2).astype(np.float32)                   # 76 real rows
    rows = 76 + 8 * 2
    batch = np.stack([np.concatenate([mel, mel[:16]]), r.normal(10, 1.5, (rows, 32)).astype(np.float32),
                      np.ones((rows, 32), np.float32)])
    got = eng.embed(batch)
    assert got.shape == (3, 3, 96)
    for b in range(3):
        for j in range(3):
            want = O.embedding_stage(batch[b, 8 * j: 8 * j + 76][None, :, :, None], emb, np.float64).reshape(96)
            np.testing.assert_allclose(got[b, j], want, rtol=0, atol=TOL_EMB)
    np.testing.assert_allclose(got[0, 0], golden["stage/embed_out"], rtol=0, atol=TOL_EMB)
    eng.reset()


def test_head_stage(eng, heads):
    feats = np.random.default_rng(2).normal(0, 2.0, (37, 16, 96)).astype(np.float32)
    for name, h in heads.items():
        got = eng.head(name, feats)
        want = O.head_stage(feats, h, np.float64)
        np.testing.assert_allclose(got, want, rtol=0, atol=TOL_SCORE)
        assert ((got > 0.5).any() and (got < 0.5).any()) or name != "hey_jarvis"


def test_multiclass_and_wide_heads(emb):
    heads = {"timer": W.synthetic_head("timer", 1234), "alexa": W.synthetic_head("alexa", 1234)}
    e = StreamEngine(3, heads, emb)
    try:
        assert e.n_labels == 8 and e.feature_ring == 34
        ft = np.random.default_rng(3).normal(0, 2.0, (4, 34, 96)).astype(np.float32)
        got = e.head("timer", ft)
        np.testing.assert_allclose(got, O.head_stage(ft, heads["timer"], np.float64), rtol=0, atol=TOL_SCORE)
        np.testing.assert_allclose(got.sum(axis=1), 1.0, atol=1e-5)
    finally:
        e.close()


@pytest.mark.parametrize("use_mfma", [3, 1])
def test_generic_heads_of_any_shape(emb, use_mfma):
    """The generic heads kernel (one wave per four streams, hidden units over the lanes): hidden sizes that are not multiples of 64, the
    512 maximum, with and without LayerNorm, a gated pair and a multiclass head outside the fast form, networks of 0, 2, 3 and 8 hidden
    blocks (a 64-unit sigmoid net with other than one block leaves the MFMA path), batches that do not fill the last wave -- against
    the float64 head of the oracle (model.py:299-302, train.py:56-83)."""
    shapes = {"odd48": dict(kind="binary", T=5, hidden=48, n_out=1, layernorm=True),
              "odd100": dict(kind="binary", T=16, hidden=100, n_out=1, layernorm=False),
              "wide512": dict(kind="multiclass", T=3, hidden=512, n_out=8, layernorm=True),
              "gated96": dict(kind="gated", T=16, hidden=96, n_out=1, layernorm=True),
              "tiny1": dict(kind="binary", T=1, hidden=1, n_out=1, layernorm=False),
              # train.py:67-73: any number of hidden blocks behind the first layer (1 in the released models)
              "deep3": dict(kind="binary", T=16, hidden=64, n_out=1, layernorm=True, n_blocks=3),
              "flat0": dict(kind="binary", T=16, hidden=64, n_out=1, layernorm=True, n_blocks=0),
              "deep2gated": dict(kind="gated", T=4, hidden=40, n_out=1, layernorm=True, n_blocks=2),
              "deep8multi": dict(kind="multiclass", T=2, hidden=130, n_out=5, layernorm=False, n_blocks=8)}
    heads = {n: W.synthetic_head(n, 7 + i, **kw) for i, (n, kw) in enumerate(shapes.items())}
    rng = np.random.default_rng(12)
    for S in (1, 5, 18):                                   # the last wave of four streams partly filled
        e = StreamEngine(S, heads, emb, use_mfma=use_mfma)
        try:
            for name, h in heads.items():
                ft = rng.normal(0, 1.5, (S, h["T"], 96)).astype(np.float32)
                got = e.head(name, ft)
                np.testing.assert_allclose(got, O.head_stage(ft, h, np.float64), rtol=0, atol=TOL_SCORE, err_msg=f"{name} S={S}")
            # and through the streaming step (feature ring rows, score columns, post-processing untouched by the head form)
            pcm = W.synthetic_pcm(S, 1280 * 3, seed=S)
            for t in range(3):
                out = e.step(pcm[:, 1280 * t:1280 * (t + 1)])
            assert out.shape == (S, e.n_labels) and np.isfinite(out).all()
        finally:
            e.close()


def test_generic_heads_kernel_gives_the_same_scores_in_both_of_its_shapes(emb, monkeypatch):
    """heads_generic_kernel runs four streams per wave below 2,048 streams and sixteen from there on (heads of up to 128 hidden units):
    the per-stream arithmetic is the same, so the scores must be bit-identical -- pinned shapes on a batch with a partly filled last
    wave, the default choice on a batch above the switch -- and within 1e-4 of the float64 oracle."""
    shapes = {"timer": dict(), "odd100": dict(kind="binary", T=16, hidden=100, n_out=1, layernorm=False),
              "deep2gated": dict(kind="gated", T=4, hidden=40, n_out=1, layernorm=True, n_blocks=2),
              "wide128": dict(kind="binary", T=16, hidden=128, n_out=1, layernorm=True, n_blocks=3),
              "flat0": dict(kind="binary", T=16, hidden=64, n_out=1, layernorm=True, n_blocks=0)}
    heads = {n: W.synthetic_head(n, 31 + i, **kw) for i, (n, kw) in enumerate(shapes.items())}
    rng = np.random.default_rng(13)

    def run(S, spw, feats, pcm):
        if spw:
            monkeypatch.setenv("OWW_GENERIC_SPW", str(spw))
        else:
            monkeypatch.delenv("OWW_GENERIC_SPW", raising=False)
        e = StreamEngine(S, heads, emb, use_mfma=1)
        try:
            out = {n: e.head(n, feats[n]) for n in heads}
            steps = [e.step(pcm[:, 1280 * t:1280 * (t + 1)]).copy() for t in range(3)]
            return out, steps
        finally:
            e.close()

    for S, variants in ((37, (4, 16)), (2100, (4, 0))):
        feats = {n: rng.normal(0, 1.5, (S, h["T"], 96)).astype(np.float32) for n, h in heads.items()}
        pcm = W.synthetic_pcm(S, 1280 * 3, seed=S)
        a, sa = run(S, variants[0], feats, pcm)
        b, sb = run(S, variants[1], feats, pcm)
        for n, h in heads.items():
            np.testing.assert_array_equal(a[n], b[n], err_msg=f"{n} S={S}")
            np.testing.assert_allclose(b[n], O.head_stage(feats[n], h, np.float64), rtol=0, atol=TOL_SCORE, err_msg=f"{n} S={S}")
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y)
    monkeypatch.delenv("OWW_GENERIC_SPW", raising=False)


def test_custom_width_heads_take_the_mfma_path_and_match_the_oracle(emb):
    """The reference's automatic training pipeline writes heads of 32 hidden units (examples/custom_model.yml:89 `layer_size: 32`,
    notebooks/training_models.ipynb: layer_dim = 32; train.py's class default is 128).  In the default family every sigmoid net of up to
    64 hidden units runs on the MFMA head kernel as a zero-padded 64-unit net whose padding stays out of the LayerNorm statistics --
    streaming scores and the post-processing fused into that launch against per-stream oracle models, and masked steps bit for bit."""
    heads = {"custom32": W.synthetic_head("custom32", 21, hidden=32),
             "gated32": W.synthetic_head("gated32", 22, kind="gated", hidden=32),
             "plain20": W.synthetic_head("plain20", 23, hidden=20, layernorm=False)}
    S, n_steps = 37, 9
    eng = StreamEngine(S, heads, emb)
    try:
        info = eng.calibration_info()
        assert np.isfinite(info["selftest_score_err"]) and info["selftest_score_err"] < 1e-4      # f16-split vs the exact family's generic kernel
        pcm = W.synthetic_pcm(S, 1280 * n_steps, seed=5)
        models = oracle_streams(eng, heads, emb, 6)
        worst = 0.0
        for t in range(n_steps):
            x = pcm[:, 1280 * t: 1280 * (t + 1)]
            got = eng.step(x)
            for s in range(6):
                want = as_vec(models[s].predict(x[s]), heads)
                worst = max(worst, float(np.abs(got[s] - want).max()))
        assert worst <= TOL_SCORE, worst
        assert (got[:6] > 0).any()
    finally:
        eng.close()
    # masked steps: a stream that sits steps out equals, bit for bit, a private sequence of its active chunks (cf. test_masked_step.py)
    a, b = StreamEngine(S, heads, emb), StreamEngine(S, heads, emb)
    try:
        rng = np.random.default_rng(9)
        on = rng.random((n_steps, S)) < 0.4
        masked = np.stack([a.step_masked(pcm[:, 1280 * t: 1280 * (t + 1)], on[t]) for t in range(n_steps)])
        counts = on.sum(0)
        packed = np.zeros((int(counts.max()), S, 1280), np.int16)
        for s in range(S):
            packed[:counts[s], s] = pcm[s].reshape(n_steps, 1280)[on[:, s]]
        plain = np.stack([b.step(p) for p in packed])
        for s in range(S):
            ts = np.nonzero(on[:, s])[0]
            np.testing.assert_array_equal(masked[ts, s], plain[:len(ts), s], err_msg=f"stream {s}")
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------- streaming
def test_streaming_every_layer_and_score(eng, emb, heads, golden):
    S, n_steps = 6, 20
    pcm = W.synthetic_pcm(S, 1280 * n_steps, seed=11)
    pcm[1] = np.resize(golden["pcm/alexa_test"], 1280 * n_steps)
    pcm[2] = np.resize(np.concatenate([np.zeros(4000, np.int16), golden["pcm/hey_mycroft_test"]]), 1280 * n_steps)
    pcm[3, 1280 * 6: 1280 * 9] = 0                                   # silence inside a stream
    models = oracle_streams(eng, heads, emb, S)
    for t in range(n_steps):
        x = pcm[:, 1280 * t: 1280 * (t + 1)]
        got = eng.step(x)
        for s in range(S):
            want = as_vec(models[s].predict(x[s]), heads)
            n_new = 5 if t == 0 else 8                               # 5 rows on the first call
            np.testing.assert_allclose(eng.get_mel(s, 8)[-n_new:], models[s].preprocessor.mel_rows[-n_new:], rtol=0, atol=TOL_MEL)
            np.testing.assert_allclose(eng.get_features(s, 16), models[s].preprocessor.features[-16:], rtol=0, atol=TOL_EMB)
            np.testing.assert_allclose(got[s], want, rtol=0, atol=TOL_SCORE)
            if t < 5:
                assert (got[s] == 0).all()                           # model.py:331-333
    # per-layer comparison of the rows that were new in the last step
    for s in (0, 2):
        h = models[s].preprocessor.mel_rows[-76:].astype(np.float64)[None, :, :, None]
        for li, (kh, kw, ci, co, relu_first, bn, pool) in enumerate(O.CNN_LAYERS):
            h = O._conv(h, emb["conv"][li].astype(np.float64))
            if relu_first:
                h = np.maximum(h, 0.0)
            if bn:
                sc, sh = O.bn_fold(*emb["bn"][li], dtype=np.float64)
                h = O._activation(h * sc + sh)
            np.testing.assert_allclose(eng.debug_layer(s, li), h[0, -LAYER_NEW_SHAPES[li][0]:], rtol=0, atol=TOL_EMB,
                                       err_msg=f"CNN layer {li}")
            if pool:
                h = O._pool(h, *pool)


def test_all_catalogue_heads_together(emb):
    """Every pretrained model of the reference's registry at once (openwakeword/__init__.py:26-60): five 64-wide heads
    (six networks: two launches of the grouped head kernel) + the multiclass `timer` (generic kernel, T = 34)."""
    names = ["alexa", "hey_mycroft", "hey_jarvis", "hey_rhasspy", "timer", "weather"]
    heads = {n: W.synthetic_head(n, cases.SEED_WEIGHTS) for n in names}
    S = 5
    e = StreamEngine(S, heads, emb)
    try:
        assert e.n_labels == 5 + 7 and e.feature_ring == 34
        models = oracle_streams(e, heads, emb, S, seed0=700)
        pcm = W.synthetic_pcm(S, 1280 * 9, seed=81)
        for t in range(9):
            x = pcm[:, 1280 * t: 1280 * (t + 1)]
            got = e.step_raw(x)
            for s in range(S):
                col = 0
                for n in names:
                    h = heads[n]
                    feats = models[s].preprocessor
                    models[s].predict(x[s]) if n == names[0] else None
                    want = O.head_stage(feats.get_features(h["T"]), h, np.float64)[0]
                    np.testing.assert_allclose(got[s, col: col + h["n_out"]], want, rtol=0, atol=TOL_SCORE, err_msg=n)
                    col += h["n_out"]
    finally:
        e.close()


def test_multi_chunk_calls(eng, emb, heads):
    """n_chunks>1: one mel pass with a single clamp floor, one embedding per chunk, max over chunks (model.py:287-298)."""
    S = 6
    models = oracle_streams(eng, heads, emb, S, seed0=300)
    for k in (2, 3, 1, 2):
        pcm = W.synthetic_pcm(S, 1280 * k * 4, seed=20 + k)
        for t in range(4):
            x = pcm[:, 1280 * k * t: 1280 * k * (t + 1)]
            got = eng.step(x)
            for s in range(S):
                np.testing.assert_allclose(got[s], as_vec(models[s].predict(x[s]), heads), rtol=0, atol=TOL_SCORE)


def test_reset_subset_and_stream_independence(eng, emb, heads):
    S = 6
    models = oracle_streams(eng, heads, emb, S, seed0=400)
    pcm = W.synthetic_pcm(S, 1280 * 16, seed=31)
    for t in range(8):
        eng.step(pcm[:, 1280 * t: 1280 * (t + 1)])
        for s in range(S):
            models[s].predict(pcm[s, 1280 * t: 1280 * (t + 1)])
    # reset streams 1 and 4 only (AudioFeatures.reset + Model.reset, utils.py:172-178, model.py:226-230)
    for s in (1, 4):
        noise = W.synthetic_pcm(1, 64000, seed=900 + s, rms=600.0)[0]
        models[s] = O.OracleModel(heads, emb, init_noise=noise)
        eng.reset([s], models[s].preprocessor.features[-eng.feature_ring:])
    for t in range(8, 16):
        x = pcm[:, 1280 * t: 1280 * (t + 1)]
        got = eng.step(x)
        for s in range(S):
            np.testing.assert_allclose(got[s], as_vec(models[s].predict(x[s]), heads), rtol=0, atol=TOL_SCORE)
        if t < 13:
            assert (got[[1, 4]] == 0).all() and (got[[0, 2, 3, 5]] != 0).any()


def test_patience_and_debounce_on_device(eng, emb, heads):
    S = 6
    pcm = W.synthetic_pcm(S, 1280 * 30, seed=41)
    for mode in ("patience", "debounce"):
        models = oracle_streams(eng, heads, emb, S, seed0=500)
        if mode == "patience":
            kw = dict(patience={"alexa": 2, "hey_jarvis": 3}, threshold={"alexa": 0.3, "hey_jarvis": 0.35})
            eng.set_postproc([2, 0, 3], [0.3, np.nan, 0.35], 0)
        else:
            kw = dict(debounce_time=0.25, threshold={"alexa": 0.4, "hey_mycroft": 0.5})
            eng.set_postproc([0, 0, 0], [0.4, 0.5, np.nan], int(np.ceil(0.25 / (1280 / 16000))))
        n_zeroed = 0
        for t in range(30):
            x = pcm[:, 1280 * t: 1280 * (t + 1)]
            got = eng.step(x)
            for s in range(S):
                want = as_vec(models[s].predict(x[s], **kw), heads)
                np.testing.assert_allclose(got[s], want, rtol=0, atol=TOL_SCORE)
                n_zeroed += int((want == 0).sum())
        assert n_zeroed > S * 5 * 3                                   # rules fired beyond the first-5 zeroing
    eng.set_postproc(None, None, 0)


def test_graph_replay_matches_eager(emb, heads):
    S = 40
    pcm = W.synthetic_pcm(S, 1280 * 10, seed=51)
    outs = []
    for graph in (False, True):
        e = StreamEngine(S, heads, emb)
        try:
            e.use_graph(graph)
            outs.append(np.stack([e.step(pcm[:, 1280 * t: 1280 * (t + 1)]).copy() for t in range(10)]))
        finally:
            e.close()
    np.testing.assert_array_equal(outs[0], outs[1])
    assert outs[0][6:].max() > 0


def test_mfma_and_valu_paths_agree(emb, heads):
    S = 70                                                            # not a multiple of any per-workgroup stream count
    pcm = W.synthetic_pcm(S, 1280 * 12, seed=61)
    outs = []
    for mfma in (1, 0, 2, 3):
        e = StreamEngine(S, heads, emb, use_mfma=mfma)
        try:
            outs.append(np.stack([e.step(pcm[:, 1280 * t: 1280 * (t + 1)]).copy() for t in range(12)]))
        finally:
            e.close()
    np.testing.assert_allclose(outs[0], outs[1], rtol=0, atol=TOL_SCORE)
    np.testing.assert_allclose(outs[0], outs[2], rtol=0, atol=TOL_SCORE)
    np.testing.assert_allclose(outs[0], outs[3], rtol=0, atol=TOL_SCORE)


def test_large_batch_properties(emb, heads):
    """BASELINE-size batch (65536 streams): properties that need no oracle run.
    (1) streams fed identical audio produce identical scores wherever they sit in the batch;
    (2) a stream's scores do not depend on the other streams (compare with a 64-stream engine);
    (3) scores stay in [0,1] and the first five frames are zero."""
    S = 65536
    base = W.synthetic_pcm(64, 1280 * 8, seed=71)
    pcm = np.tile(base, (S // 64, 1))
    big = StreamEngine(S, heads, emb)
    small = StreamEngine(64, heads, emb)
    try:
        for t in range(8):
            g = big.step(pcm[:, 1280 * t: 1280 * (t + 1)])
            s = small.step(base[:, 1280 * t: 1280 * (t + 1)])
            assert np.isfinite(g).all() and g.min() >= 0 and g.max() <= 1
            if t < 5:
                assert (g == 0).all()
            np.testing.assert_array_equal(g.reshape(S // 64, 64, -1), np.broadcast_to(s, (S // 64, 64, s.shape[1])))
        assert g.max() > 0
    finally:
        big.close()
        small.close()


@pytest.mark.parametrize("S", [40, 2500])
def test_weight_ring_depth_never_changes_a_bit(emb, heads, monkeypatch, S):
    """The stage kernels stream their weights through an LDS ring of 2 slots (large launches) or 3 (at most two workgroups per CU) --
    same arithmetic in the same order, only what is in flight differs.  Scores AND feature rings of a handle pinned to the
    three-slot ring and to the two-slot ring must be bit-identical."""
    pcm = W.synthetic_pcm(S, 1280 * 8, seed=91)

    def run(small):
        monkeypatch.setenv("OWW_SMALL_WGS", str(small))
        e = StreamEngine(S, heads, emb)
        try:
            out = np.stack([e.step(pcm[:, 1280 * t: 1280 * (t + 1)]) for t in range(8)])
            feats = np.stack([e.get_features(s, 16) for s in (0, S // 2, S - 1)])
            assert not e.range_status()
            return out, feats
        finally:
            e.close()

    b = run(1 << 20)                   # three slots
    c = run(0)                         # two slots
    monkeypatch.delenv("OWW_SMALL_WGS")
    np.testing.assert_array_equal(b[0], c[0])
    np.testing.assert_array_equal(b[1], c[1])
    assert b[0][-1].max() > 0


def test_concurrent_block_engines_are_bit_identical(emb, heads):
    """Three engines over the blocks of a 16,480-stream batch, each on its own HIP stream and stepped on device-resident PCM with no
    host sync between them, must give exactly the scores of one 16,480-stream engine, also through a masked step; batch invariance
    makes the rows comparable.  This is the stress test of the small-launch kernels: a block of ~5,500 streams runs the three-slot
    weight ring of the stage kernels and the deep ring of the heads kernel -- counted waits and bare barriers -- while the single
    engine runs the two-slot forms, and three engines' kernels share the CUs.  (The first five scores of a stream are zeroed by
    model.py:331-333: only frames >= 5 can show a difference, so the run is ten frames, three times.)"""
    import torch
    S = 16384 + 96
    borders = [0, 5504, 11008, S]                                   # 5,504 / 5,504 / 5,472 streams
    n_frames = 10
    pcm = W.synthetic_pcm(S, 1280 * n_frames, seed=72)
    on = (np.random.default_rng(3).random(S) < 0.8).astype(np.uint8)
    dev = torch.device("cuda:0")
    # [frame][stream][sample] on the device: a block's chunk of one frame is one contiguous, 16-byte aligned slice
    pcm_dev = torch.from_numpy(np.ascontiguousarray(pcm.reshape(S, n_frames, 1280).transpose(1, 0, 2))).to(dev)
    hip_streams = [torch.cuda.Stream(dev) for _ in range(3)]
    one = StreamEngine(S, heads, emb)
    parts = [StreamEngine(b1 - b0, heads, emb, hip_stream=st.cuda_stream)
             for b0, b1, st in zip(borders[:-1], borders[1:], hip_streams)]
    scores = torch.empty((n_frames, S, one.n_labels), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    try:
        for rep in range(3):
            one.reset()
            for e in parts:
                e.reset()
            want = []
            for t in range(n_frames):
                x = np.ascontiguousarray(pcm[:, 1280 * t: 1280 * (t + 1)])
                want.append(one.step_masked(x, on) if t == 7 else one.step(x))
                for e, b0, b1 in zip(parts, borders[:-1], borders[1:]):
                    x_ptr, sc_ptr = pcm_dev[t, b0:b1].data_ptr(), scores[t, b0:b1].data_ptr()
                    if t == 7:
                        e.step_masked_device(x_ptr, on[b0:b1], sc_ptr)
                    else:
                        e.step_device(x_ptr, 1, sc_ptr)
            for e in parts:
                e.sync()
            got = scores.cpu().numpy()
            for t in range(n_frames):
                np.testing.assert_array_equal(want[t], got[t], err_msg=f"repetition {rep} frame {t}")
            assert want[-1].max() > 0
            for s_ in (0, 5503, 5504, 11007, 11008, S - 1):            # embeddings too, either side of a block border
                k = np.searchsorted(borders, s_, side="right") - 1
                np.testing.assert_array_equal(one.get_features(s_, 4), parts[k].get_features(s_ - borders[k], 4))
    finally:
        one.close()
        for e in parts:
            e.close()


def test_host_fed_pipeline_matches_blocking_steps(emb, heads):
    """oww_submit / oww_collect (upload of step t+1 overlapping the kernels of step t, two steps in flight) deliver
    exactly the scores of the blocking oww_step sequence, post-processing included; order errors are reported."""
    from openwakeword_amd._lib import OwwError
    S, T = 96, 12
    pcm = W.synthetic_pcm(S, 1280 * T, seed=321)
    ref = StreamEngine(S, heads, emb)
    eng = StreamEngine(S, heads, emb)
    try:
        for e in (ref, eng):
            e.set_postproc([0] * e.n_labels, [0.3] * e.n_labels, 4)
        want = [ref.step(np.ascontiguousarray(pcm[:, 1280 * t: 1280 * (t + 1)])) for t in range(T)]
        with pytest.raises(OwwError):
            eng.collect()                                               # nothing in flight
        bufs = [eng.pinned_empty((S, 1280), np.int16) for _ in range(2)]
        got = []
        for t in range(T):
            bufs[t % 2][:] = pcm[:, 1280 * t: 1280 * (t + 1)]
            eng.submit(bufs[t % 2])
            if t >= 1:
                got.append(eng.collect().copy())
            if t == 0:
                continue
        # two in flight is the limit
        bufs[T % 2][:] = 0
        eng.submit(bufs[T % 2])
        with pytest.raises(OwwError):
            eng.submit(bufs[(T + 1) % 2])
        got.append(eng.collect().copy())
        eng.collect()
        for t in range(T):
            np.testing.assert_array_equal(got[t], want[t])
        # pageable memory works too, and the blocking call still interleaves with the pipeline
        x = np.ascontiguousarray(pcm[:, :1280])
        eng.submit(x)
        a = eng.collect()
        b = ref.step(np.zeros((S, 1280), np.int16))
        b = ref.step(x)
        np.testing.assert_array_equal(a, b)
    finally:
        ref.close()
        eng.close()


def test_self_test_and_commit_time_range_handling(emb, heads):
    """StreamEngine.self_test: the deploy-time comparison of the f16-split family with the exact-fp32 family passes on the normal
    weights.  A network whose EMBEDDINGS are of order 1e6 (one late BatchNorm shift of 3e5) used to be refused when the handle was
    created -- round 3's heads took the features in true units and f16 halves cannot hold 1e6.  Since round 4 the heads' GEMM runs
    on calibrated power-of-two scales like every CNN layer (HeadHxParams::fscale), so the same network is ACCEPTED and agrees with
    the exact family; what oww_commit still refuses is in tests/test_weight_regimes.py."""
    import copy
    eng = StreamEngine(4, heads, emb)
    try:
        res = eng.self_test(n_frames=12)
        assert res["max_abs_score_diff"] < 1e-4 and res["max_abs_embedding_diff"] < 2e-4 * max(1.0, res["max_abs_embedding"])
    finally:
        eng.close()
    big = copy.deepcopy(emb)
    gamma, beta, mean, var = big["bn"][10]                              # weights.synthetic_embedding: Keras order
    big["bn"][10] = (gamma, np.full_like(beta, 3.0e5), mean, var)
    eng = StreamEngine(4, heads, big)
    try:
        res = eng.self_test(n_frames=12)
        assert res["max_abs_embedding"] > 1e4
        assert res["max_abs_score_diff"] < 1e-4 and res["max_abs_embedding_diff"] < 2e-4 * res["max_abs_embedding"]
    finally:
        eng.close()
    eng = StreamEngine(4, heads, big, use_mfma=1)                       # the exact family agrees with itself
    try:
        assert eng.self_test(n_frames=12)["max_abs_score_diff"] == 0.0
    finally:
        eng.close()


def test_range_guard_is_sticky_and_loud(emb, heads):
    """An activation beyond the f16 range at run time (here: feature-ring rows of 1e6 handed to the heads) must not score
    silently: the step that sees it and every later call raise OwwRangeError until the flag is cleared; the exact-fp32
    family computes the same input without complaint."""
    from openwakeword_amd._lib import OwwRangeError
    pcm = W.synthetic_pcm(3, 1280 * 3, seed=77)
    huge = np.full((16, 96), 1.0e6, np.float32)
    eng = StreamEngine(3, heads, emb)
    try:
        assert eng.range_status() is False
        eng.step(pcm[:, :1280])
        eng.reset([1], huge)
        with pytest.raises(OwwRangeError):
            eng.step(pcm[:, 1280:2560])
        with pytest.raises(OwwRangeError):                       # sticky
            eng.step(pcm[:, 2560:])
        with pytest.raises(OwwRangeError):
            eng.sync()
        first, n = eng.range_where()                              # the offender (stream 1) is among the streams named
        assert first >= 0 and first <= 1 < first + n <= 3
        assert eng.range_status(clear=True) is True
        assert eng.range_where() == (-1, 0)
        eng.reset()
        assert eng.range_status() is False
        out = eng.step(pcm[:, :1280])
        assert np.isfinite(out).all()
        with pytest.raises(OwwRangeError):                       # the stage-level entry reports it too
            eng.head("alexa", np.full((2, 16, 96), 1.0e6, np.float32))
        eng.range_status(clear=True)
    finally:
        eng.close()
    eng = StreamEngine(3, heads, emb, use_mfma=1)
    try:
        eng.reset([1], huge)
        assert np.isfinite(eng.step(pcm[:, :1280])).all() and eng.range_status() is False
    finally:
        eng.close()


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fuzz_kernel_families_agree(emb, seed):
    """Seeded fuzz over the host-visible degrees of freedom -- stream count (odd, below / above the per-workgroup group
    sizes), head set (binary, gated, multiclass, wide), chunks per call, partial resets in mid-stream -- comparing the
    default f16-split family with the LDS-tiled fp32 family, which shares none of its state layouts or stage kernels."""
    r = np.random.default_rng(seed)
    S = int(r.choice([1, 5, 31, 33, 97, 130]))
    names = list(r.choice(["alexa", "hey_mycroft", "hey_jarvis", "timer", "weather", "hey_rhasspy"], size=int(r.integers(1, 4)), replace=False))
    heads = {n: W.synthetic_head(n, 1234) for n in names}
    kmax = int(r.integers(1, 4))
    engs = [StreamEngine(S, heads, emb, use_mfma=m, max_chunks=kmax) for m in (3, 2)]
    try:
        for step in range(10):
            k = int(r.integers(1, kmax + 1))
            amp = float(r.choice([0.0, 50.0, 3000.0, 20000.0]))
            pcm = np.clip(np.round(r.normal(0.0, 1.0, (S, 1280 * k)) * amp), -32768, 32767).astype(np.int16)
            if step in (3, 7) and S > 1:
                ids = sorted(set(int(i) for i in r.integers(0, S, size=max(1, S // 3))))
                ring = r.normal(0.0, 1.0, (engs[0].feature_ring, 96)).astype(np.float32)
                for e in engs:
                    e.reset(ids, ring)
            a, b = (e.step(pcm).copy() for e in engs)
            assert np.isfinite(a).all()
            np.testing.assert_allclose(a, b, rtol=0, atol=TOL_SCORE, err_msg=f"S={S} heads={names} step={step} k={k}")
        fa = np.stack([engs[0].get_features(s, 16) for s in range(S)])
        fb = np.stack([engs[1].get_features(s, 16) for s in range(S)])
        np.testing.assert_allclose(fa, fb, rtol=0, atol=2e-4)
    finally:
        for e in engs:
            e.close()


def test_device_pcm_pointer_of_any_alignment():
    """A device PCM pointer that is only 2-byte aligned (a slice of a larger int16 tensor) cannot feed the fused front end's 16-byte
    sample loads: such a step takes the separate mel launch (scalar loads) and must give the scores of an aligned copy to fp32
    round-off -- also with the voice-activity front end, which reads the same buffer."""
    import torch
    from openwakeword_amd.engine import StreamEngine
    dev = torch.device("cuda", 0)
    S, T = 300, 6
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    pcm = (torch.randn(T, S * 1280 + 8, device=dev, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16)
    heads = {"alexa": W.synthetic_head("alexa", 1)}
    for vad in (None, W.synthetic_vad(2)):
        kw = dict(vad=vad, vad_threshold=0.5) if vad is not None else {}
        for off in (1, 3, 4):
            out = []
            for aligned in (True, False):
                eng = StreamEngine(S, heads, W.synthetic_embedding(1), **kw)
                sc = torch.empty(S, 1, device=dev)
                rows = []
                try:
                    for t in range(T):
                        x = pcm[t, off:off + S * 1280]
                        x = x.clone() if aligned else x
                        assert (x.data_ptr() % 16 == 0) == aligned
                        torch.cuda.synchronize()
                        eng.step_device(x.data_ptr(), 1, sc.data_ptr())
                        eng.sync()
                        rows.append(sc.cpu().numpy().copy())
                finally:
                    eng.close()
                out.append(np.stack(rows))
            assert np.isfinite(out[1]).all()
            np.testing.assert_allclose(out[1], out[0], rtol=0, atol=1e-5, err_msg=f"offset {off}, vad {vad is not None}")
