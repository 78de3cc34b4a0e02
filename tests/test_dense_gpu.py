"""Dense scoring on the device (include/owwhip.h: oww_score_features / oww_score_clips; csrc/owwhip_dense.h): every window of a feature
sequence through the fixed heads.  The contract: out[b][w][col] is BIT FOR BIT what oww_head returns for that head on the materialised
window, and within TOL_SCORE of the float64 oracle (tests/dense_ref.py; the CPU tier test_dense_cpu.py admits the inputs).  The shapes
are the tile edges of the sliding-window kernel -- 1, 37, 128, 129, 256, 257 and 261 windows per sequence, three sequences -- at window
lengths whose k-step counts leave every residue of the ring depths.  pytest -m gpu -s prints the worst error of every form."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from openwakeword_amd import _lib, utils
from openwakeword_amd import weights as W
from openwakeword_amd.engine import KERNEL_CLASSES, StreamEngine, _ptr

import dense_ref as D
import head_windows as HW

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
S = 4                                    # streams of the handles (dense scoring of features borrows none of them)


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


def _sums_to_one(got):
    if got.shape[-1] > 1:
        np.testing.assert_allclose(got.sum(axis=-1), 1.0, atol=1e-5)


def _head_on_windows(eng, name, f, t_max=None):
    """oww_head on the materialised windows of f [B, n_rows, 96] -> [B, n_win, n_out]."""
    T = int(eng.heads[name]["T"])
    w = np.ascontiguousarray(D.windows_of(f, T, t_max))
    return eng.head(name, w.reshape(-1, T, 96)).reshape(w.shape[0], w.shape[1], -1)


def _launches(eng):
    t = eng.kernel_times()
    return t[KERNEL_CLASSES[6]]["launches"], t[KERNEL_CLASSES[7]]["launches"]


def _check_case(eng, form, T, n_win, slides, worst, label):
    """One (handle, n_win): score_features on the case's rows against float64 and, bit for bit, against oww_head; the path it took."""
    f = D.feats()[:, :D.case_rows(n_win, T)]
    assert eng.score_shape(f.shape[1]) == (n_win, T)
    eng.kernel_times()
    got = eng.score_features(f)
    heads_launches, gathers = _launches(eng)
    flag = eng.range_status(clear=True)
    assert got.shape == (D.B, n_win, eng.n_labels)
    assert (gathers == 0) == slides, f"{label}: {heads_launches} heads launches and {gathers} gathers"
    if slides:                                              # one launch per pass of at most two nets
        assert heads_launches == (HW.FORMS[form]["nn"] + 1) // 2, f"{label}: {heads_launches} sliding launches"
    for n, ref in D.want(form, T).items():
        lo, hi = eng.head_cols[n]
        HW.check_scores(f"{n} {label} n_win={n_win}", got[:, :, lo:hi], ref[:, :n_win], flag, worst)
        _sums_to_one(got[:, :, lo:hi])
        one = _head_on_windows(eng, n, f)
        assert np.array_equal(got[:, :, lo:hi], one), f"{n} {label} n_win={n_win}: differs from oww_head at " \
            f"{np.argwhere(got[:, :, lo:hi] != one)[:6].tolist()}"
    assert eng.range_status(clear=True) is False


# ------------------------------------------------------------------------------------------------ 1. the ring forms at the tile edges
@pytest.mark.parametrize("form", D.SLIDE_FORMS)
def test_every_window_is_oww_head_bit_for_bit_and_float64(form):
    """narrow1-4 (the sliding-window kernel: one to four nets, a gated pair among them) and wide1-2 (the gather fallback) at T 1, 3,
    16, 19, 22 and 1, 37, 128, 129, 256, 257, 261 windows per sequence."""
    worst = [0.0]
    slides = HW.FORMS[form]["ht"] == 4
    for T in D.TS:
        eng = StreamEngine(S, D.form_heads(form, T), _emb())
        try:
            eng.enable_timing(True)
            for n_win in D.N_WINS:
                _check_case(eng, form, T, n_win, slides, worst, f"T={T}")
        finally:
            eng.close()
    print(f"\n{form} ({'sliding kernel' if slides else 'fallback'}): worst |score - float64| over T {D.TS} x n_win {D.N_WINS} = {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ 2. the fallback forms and the routing edge
@pytest.mark.parametrize("form,fam", [("generic130", 3), ("rnn1", 3), ("fp32_2x64", 1)])
def test_fallback_forms_match_oww_head_and_float64(form, fam):
    worst = [0.0]
    for T in D.TS:
        eng = StreamEngine(S, D.form_heads(form, T), _emb(), use_mfma=fam)
        try:
            eng.enable_timing(True)
            for n_win in (37, 129):
                _check_case(eng, form, T, n_win, False, worst, f"use_mfma={fam} T={T}")
        finally:
            eng.close()
    print(f"\n{form} use_mfma={fam} (fallback): worst |score - float64| = {worst[0]:.2e}")


def test_tile_size_edges_and_the_longest_window():
    """The sliding kernel runs tiles of 256 windows while their rows fit the LDS beside a two-slot ring and tiles of 128 beyond: the
    switch lies between T = 72 and 73 for a pass of two nets (narrow4: two passes) and between 113 and 114 for one net; T = 120 is the
    longest window a fixed head may have -- no narrow group takes the fallback.  The same comparison on both sides of each edge."""
    worst = [0.0]
    for form, Ts in D.EDGES:
        for T in Ts:
            eng = StreamEngine(S, D.form_heads(form, T), _emb())
            try:
                eng.enable_timing(True)
                for n_win in D.EDGE_N_WINS:
                    _check_case(eng, form, T, n_win, True, worst, f"T={T}")
            finally:
                eng.close()
    print(f"\nnarrow forms at the tile-size edges: worst |score - float64| = {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ 3. mixed T on one handle
def _mixed_heads():
    shapes = HW.FORMS["narrow4"]["heads"]
    return {f"mix{T}": HW.centre(HW.draw_head(f"mix{T}", shapes[i], T, seed=D.HEAD_SEED),
                                 np.ascontiguousarray(D.windows_of(D.feats(), T, 22)).reshape(-1, T, 96)) for i, T in enumerate((5, 16, 22))}


def test_mixed_window_lengths_end_at_the_same_row():
    heads = _mixed_heads()
    f = D.feats()[:, :129 + 21]
    ref = D.dense_ref(f, heads)
    eng = StreamEngine(S, heads, _emb())
    try:
        assert eng.score_shape(f.shape[1]) == (129, 22)
        got = eng.score_features(f)
        flag = eng.range_status(clear=True)
        for n, h in heads.items():
            lo, hi = eng.head_cols[n]
            HW.check_scores(f"{n} beside T 5, 16, 22", got[:, :, lo:hi], ref[n], flag)
            one = _head_on_windows(eng, n, f, 22)             # rows [w + 22 - T, w + 22)
            assert np.array_equal(got[:, :, lo:hi], one), f"{n}: differs from oww_head at {np.argwhere(got[:, :, lo:hi] != one)[:6].tolist()}"
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. invariances
def test_a_windows_scores_depend_on_its_rows_alone():
    """A sliding group (narrow3, T = 16) and a fallback head (wide1, T = 16) on one handle: shifting the sequence start, scoring one
    sequence alone and scoring in overlapping chunks all return the same bits."""
    heads = {**D.form_heads("narrow3", 16), **D.form_heads("wide1", 16)}
    f = D.feats()
    eng = StreamEngine(S, heads, _emb())
    try:
        out = eng.score_features(f)
        assert out.shape == (D.B, D.ROWS - 15, 3)          # narrow3: a gated pair and a single net; wide1: one
        for k in (1, 31, 128):
            assert np.array_equal(eng.score_features(f[:, k:]), out[:, k:]), f"start shifted by {k} rows"
        for b in range(D.B):
            assert np.array_equal(eng.score_features(f[b:b + 1]), out[b:b + 1]), f"sequence {b} alone"
        bm = types.SimpleNamespace(engine=eng, labels=list(heads), _keep=[eng.head_cols[n][0] for n in heads])
        whole = utils.score_feature_file(f[2], bm)
        parts = utils.score_feature_file(f[2], bm, chunk_rows=100)
        for i, n in enumerate(heads):
            assert np.array_equal(whole[n], out[2, :, i]) and np.array_equal(parts[n], out[2, :, i]), f"{n}: chunks of 100 rows"
        assert eng.range_status() is False
    finally:
        eng.close()


def test_the_gather_route_equals_the_sliding_route(monkeypatch):
    """narrow3 (a gated pair and a single net: two passes) at T = 16 over 261 windows: OWW_DENSE_PATH=ext sends the group down the gather
    fallback -- oww_head's own launch over materialised windows -- and the scores are bit for bit the sliding kernel's."""
    eng = StreamEngine(S, D.form_heads("narrow3", 16), _emb())
    f = D.feats()[:, :D.case_rows(261, 16)]
    try:
        eng.enable_timing(True)
        eng.kernel_times()
        slide = eng.score_features(f)
        assert _launches(eng) == (2, 0)
        monkeypatch.setenv("OWW_DENSE_PATH", "ext")
        ext = eng.score_features(f)
        assert _launches(eng) == (1, 1)                     # one gather, one launch for the whole group
        monkeypatch.delenv("OWW_DENSE_PATH")
        assert np.array_equal(slide, ext), f"differs at {np.argwhere(slide != ext)[:6].tolist()}"
        assert eng.range_status() is False
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. clips
def _smoke_heads():
    return {n: W.synthetic_head(n, 1234) for n in ("alexa", "hey_mycroft", "hey_jarvis")}


@functools.lru_cache(maxsize=None)
def _clips():
    x = W.synthetic_pcm(3, 64000, seed=21, rms=3000.0).astype(np.float64) * np.array([1.0, 0.1, 0.01])[:, None]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def test_score_clips_is_score_features_of_embed_clips():
    eng = StreamEngine(S, _smoke_heads(), _emb())
    try:
        emb = eng.embed_clips(_clips())
        want = eng.score_features(emb)
        got, got_emb = eng.score_clips(_clips(), return_features=True)
        assert got.shape == (3, 41 - 16 + 1, 3) and np.isfinite(got).all()
        assert np.array_equal(got_emb, emb) and np.array_equal(got, want)
        assert np.array_equal(eng.score_clips(_clips()), want)
        assert np.array_equal(eng.score_clips(_clips()[1:2]), want[1:2])
        assert eng.range_status() is False
    finally:
        eng.close()


def test_live_streams_do_not_notice_dense_scoring():
    """Two handles with events and audio rings stepped on the same PCM; one scores features and clips between steps.  Their next three
    steps return the same scores, feature rings, event records, event features and audio."""
    kw = dict(event_capacity=16, event_features=4, audio_chunks=4, event_audio=2)
    pcm = W.synthetic_pcm(S, 1280 * 12, seed=42)
    a, b = StreamEngine(S, _smoke_heads(), _emb(), **kw), StreamEngine(S, _smoke_heads(), _emb(), **kw)
    try:
        for e in (a, b):
            e.set_event_thresholds(np.zeros(3, np.float32))        # every column of every stream reports: records to compare
        for t in range(9):
            if t in (6, 7, 8):
                a.score_features(D.feats()[:, :60])
                a.score_clips(_clips())
            sa, sb = a.step(pcm[:, 1280 * t:1280 * (t + 1)]), b.step(pcm[:, 1280 * t:1280 * (t + 1)])
            assert np.array_equal(sa, sb), f"step {t}"
            (ra, na), (rb, nb) = a.events(), b.events()
            assert na == nb and ra.tobytes() == rb.tobytes(), f"step {t}: events"
            assert np.array_equal(a.event_features(), b.event_features()) and np.array_equal(a.event_audio(), b.event_audio())
            for s in range(S):
                assert np.array_equal(a.get_features(s, 16), b.get_features(s, 16)), f"step {t} stream {s}"
            assert np.array_equal(a.audio(range(S), 4)[0], b.audio(range(S), 4)[0])
        assert na > 0
    finally:
        a.close(); b.close()


def test_batched_model_score_clips_and_mine_windows():
    """BatchedModel.score_clips and utils.mine_windows on the device: the labelled columns are the engine's, and the mined windows are the
    rows of the returned embeddings behind every score at or above the threshold."""
    from openwakeword_amd.model import BatchedModel
    names = ["alexa", "hey_mycroft", "hey_jarvis"]
    bm = BatchedModel(2, names, weights="synthetic")
    try:
        raw, emb = bm.engine.score_clips(_clips(), return_features=True)
        sc, emb2 = bm.score_clips(_clips(), return_features=True)
        assert list(sc) == bm.labels == names and np.array_equal(emb, emb2)
        for i, n in enumerate(names):
            assert np.array_equal(sc[n], raw[:, :, i])
        thr = float(np.median(raw))
        got = utils.mine_windows(_clips(), bm, threshold=thr)
        assert list(got) == names
        for i, n in enumerate(names):
            b, w = np.nonzero(raw[:, :, i] >= thr)
            assert got[n].shape == (b.size, 16, 96)
            for k in range(b.size):
                assert np.array_equal(got[n][k], emb[b[k], w[k]:w[k] + 16])
        assert sum(v.shape[0] for v in got.values()) > 0
    finally:
        bm.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_untouched():
    pcm = W.synthetic_pcm(S, 1280 * 8, seed=43)
    a, b = StreamEngine(S, _smoke_heads(), _emb()), StreamEngine(S, _smoke_heads(), _emb())
    bank = StreamEngine(S, {}, _emb(), bank_slots=2, bank_capacity=4)
    try:
        for t in range(6):
            a.step(pcm[:, 1280 * t:1280 * (t + 1)]); b.step(pcm[:, 1280 * t:1280 * (t + 1)])
        lib, f, out = a._lib, np.ascontiguousarray(D.feats()[:, :40]), np.zeros((3, 40, 3), np.float32)
        nw, tm = C.c_int32(-7), C.c_int32(-7)
        assert lib.oww_score_shape(a._h, 15, C.byref(nw), C.byref(tm)) == EINVAL and (nw.value, tm.value) == (-7, -7)      # n_rows = t_max - 1
        assert lib.oww_score_shape(a._h, 16, None, None) == 0 and lib.oww_score_shape(a._h, 16, C.byref(nw), None) == 0 and nw.value == 1
        assert lib.oww_score_features(a._h, _ptr(f), 0, 3, 15, _ptr(out), 0) == EINVAL
        assert lib.oww_score_features(a._h, _ptr(f), 0, 0, 40, _ptr(out), 0) == EINVAL                                     # B = 0
        assert lib.oww_score_features(a._h, None, 0, 3, 40, _ptr(out), 0) == EINVAL
        assert lib.oww_score_features(a._h, _ptr(f), 0, 3, 40, None, 0) == EINVAL
        clips = _clips()
        assert lib.oww_score_clips(a._h, _ptr(clips), 0, 0, 64000, _ptr(out), 0, None, 0) == EINVAL
        assert lib.oww_score_clips(a._h, _ptr(clips), 0, a.n_streams_padded + 1, 64000, _ptr(out), 0, None, 0) == EINVAL
        assert lib.oww_score_clips(a._h, _ptr(clips), 0, 3, 12512 + 14 * 1280, _ptr(out), 0, None, 0) == EINVAL            # 15 rows
        assert b"oww_score_clips" in lib.oww_last_error()
        with pytest.raises(_lib.OwwError):
            a.score_features(D.feats()[:, :15])
        # a handle with bank heads only
        assert lib.oww_score_shape(bank._h, 40, C.byref(nw), C.byref(tm)) == EINVAL
        assert lib.oww_score_features(bank._h, _ptr(f), 0, 3, 40, _ptr(out), 0) == EINVAL
        assert lib.oww_score_clips(bank._h, _ptr(clips), 0, 3, 64000, _ptr(out), 0, None, 0) == EINVAL
        # before commit
        raw = C.c_void_p()
        cfg = _lib.Config(0, S, 1, 0, 3, 0, None)
        _lib.check(lib.oww_create(C.byref(cfg), C.byref(raw)))
        try:
            assert lib.oww_score_shape(raw, 40, None, None) == ESTATE
            assert lib.oww_score_features(raw, _ptr(f), 0, 3, 40, _ptr(out), 0) == ESTATE
            assert lib.oww_score_clips(raw, _ptr(clips), 0, 3, 64000, _ptr(out), 0, None, 0) == ESTATE
        finally:
            lib.oww_destroy(raw)
        assert lib.oww_score_shape(None, 40, None, None) == ESTATE
        assert not out.any()
        for t in range(6, 8):
            assert np.array_equal(a.step(pcm[:, 1280 * t:1280 * (t + 1)]), b.step(pcm[:, 1280 * t:1280 * (t + 1)])), f"step {t}"
        assert a.range_status() is False
    finally:
        a.close(); b.close(); bank.close()
