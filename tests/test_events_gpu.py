"""Detection events on the GPU (include/owwhip.h: oww_events_*; kernels in csrc/owwhip_events.h).  Every case runs a twin handle without
events on the same audio -- the existing scoring path is the reference -- and holds the events handle's records, counts, order and
feature snapshots to engine.events_from_scores of the twin's scores and to the twin's oww_get_features, bit for bit.

Thresholds are not hand-picked: each label's event threshold is the median of the twin's nonzero post-processed scores of that label
over the scored steps (6 onwards; steps 1-5 read 0 by model.py:331-333), and every case first asserts that at least 20 % of the
participating pairs hit and at least 20 % do not, so that neither an empty nor a full event list can pass it.  Synthetic weights
(embedding seed 3, head seed 1234), Gaussian noise PCM; the PCM seed of each case is recorded at its twin."""
import ctypes as C
import functools

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import CHUNK, EVENT_DTYPE, StreamEngine, events_from_scores

pytestmark = pytest.mark.gpu

FIXED = ["alexa", "hey_mycroft", "weather"]
EMB_SEED = 3
ESTATE, EINVAL = -3, -1


def _heads(names=FIXED):
    return {n: W.synthetic_head(n, 1234) for n in names}


def _engine(S, heads=None, **kw):
    return StreamEngine(S, _heads() if heads is None else heads, W.synthetic_embedding(EMB_SEED), **kw)


def _median_thresholds(scores, on=None):
    """Per column: the median of the nonzero scores of [steps, S, n] (participating rows only)."""
    thr = []
    for c in range(scores.shape[2]):
        v = scores[:, :, c] if on is None else scores[:, :, c][on]
        v = v[v != 0]
        assert v.size, f"column {c} never scored"
        thr.append(np.float32(np.median(v)))
    return np.array(thr, dtype=np.float32)


def _assert_mixed(scores, thr, on=None):
    """The precondition of every comparison: >= 20 % of the participating pairs hit and >= 20 % do not."""
    hit = scores >= thr[None, None, :]
    if on is not None:
        hit = hit[on]
    frac = float(hit.mean())
    print(f"hit fraction over the scored steps: {frac:.3f} ({int(hit.sum())} of {hit.size} pairs)")
    assert 0.2 <= frac <= 0.8, frac


def _check(eng, want, frames, n_total=None, cap=None):
    """events() of the handle against the expected list [(stream, column, bank_id, score)]; returns the records."""
    rec, total = eng.events()
    assert total == (len(want) if n_total is None else n_total)
    stored = want if cap is None else want[:cap]
    assert len(rec) == len(stored)
    assert rec.dtype == EVENT_DTYPE
    assert rec["stream"].tolist() == [w[0] for w in stored]
    assert rec["column"].tolist() == [w[1] for w in stored]
    assert rec["bank_id"].tolist() == [w[2] for w in stored]
    np.testing.assert_array_equal(rec["score"].view(np.uint32), np.array([w[3] for w in stored], dtype=np.float32).view(np.uint32))
    np.testing.assert_array_equal(rec["frame"], np.asarray(frames, dtype=np.uint32)[rec["stream"]] if len(rec) else [])
    want_idx = np.arange(len(rec)) if eng.event_rows > 0 else np.full(len(rec), -1)
    np.testing.assert_array_equal(rec["feature_index"], want_idx)
    assert not rec["reserved"].any()
    return rec


@functools.lru_cache(maxsize=None)
def _twin(S, steps, seed, rows=0):
    """The reference run, made once per shape: a handle without events over `steps` one-chunk steps of noise (PCM seed `seed`); `rows`:
    also every stream's last `rows` feature rows after every step (the 70-stream cases share one run with rows = 16).
    -> (pcm [steps][S, 1280], scores [steps, S, 3], thresholds [3], features [steps, S, rows, 96] or None)."""
    eng = _engine(S)
    pcm = W.synthetic_pcm(S, CHUNK * steps, seed=seed)
    pcm = [np.ascontiguousarray(pcm[:, CHUNK * t: CHUNK * (t + 1)]) for t in range(steps)]
    scores = np.zeros((steps, S, 3), dtype=np.float32)
    feats = np.zeros((steps, S, rows, 96), dtype=np.float32) if rows else None
    for t in range(steps):
        scores[t] = eng.step(pcm[t])
        if rows:
            for s in range(S):
                feats[t, s] = eng.get_features(s, rows)
    with pytest.raises(_lib.OwwError):                       # off by default: no events on this handle
        eng.events()
    assert eng._lib.oww_get_events(eng._h, None, 0, None, None) == ESTATE
    eng.close()
    assert not scores[:5].any() and scores[5:].all()
    thr = _median_thresholds(scores[5:])
    _assert_mixed(scores[5:], thr)
    for a in (scores, thr) + ((feats,) if rows else ()):
        a.setflags(write=False)
    return pcm, scores, thr, feats


def _run_like_case_1(S, steps, seed, capacity, graph=False, rows=0):
    pcm, scores, thr, _ = _twin(S, steps, seed, rows)
    eng = _engine(S, event_capacity=capacity)
    if graph:
        eng.use_graph(True)
    rec, total = eng.events()                                # no call yet: zero events
    assert len(rec) == 0 and total == 0
    eng.set_event_thresholds(thr)
    n_events = 0
    for t in range(steps):
        got = eng.step(pcm[t])
        assert got.tobytes() == scores[t].tobytes()
        want = events_from_scores(scores[t], None, None, thr)
        rec = _check(eng, want, np.full(S, t + 1))
        if t < 5:
            assert len(rec) == 0
        n_events += len(rec)
    assert n_events > 0
    eng.close()


def test_events_equal_the_host_scan_70_streams():
    """Case 1: S = 70, 3 heads, 12 steps (PCM seed 11): exact order, bitwise scores, frame = step number, steps 1-5 empty."""
    _run_like_case_1(70, 12, 11, 256, rows=16)


def test_events_equal_the_host_scan_5500_streams():
    """Case 2: 16,500 pairs = 65 workgroups with a partial last one: the base reduction covers more than one wave's worth of block
    counts (PCM seed 12)."""
    _run_like_case_1(5500, 8, 12, 16500)


def test_events_under_a_captured_graph():
    """Case 8: oww_use_graph(1) replays the step; the events launches follow it outside the graph."""
    _run_like_case_1(70, 12, 11, 256, graph=True, rows=16)


def _hip():
    """hipMemcpy of the HIP runtime libowwhip.so itself is linked against, for the sentinel copies of the overflow case: looked up
    through the library's own handle, so the device pointers it hands out are driven by the runtime that made them."""
    fn = _lib.load()["hipMemcpy"]                            # (dlsym on the library's handle searches its dependencies)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return fn


def test_overflow_is_counted_and_bounded():
    """Case 3: capacity 8: n_total is the true count, the records are the first 8 of the full list, and one-past-capacity sentinels in
    the record and snapshot buffers (the spare entry both buffers carry) are unchanged."""
    S, steps, cap, rows = 70, 12, 8, 3
    pcm, scores, thr, feats = _twin(S, steps, 11, 16)
    eng = _engine(S, event_capacity=cap, event_features=rows)
    eng.set_event_thresholds(thr)
    eng.step(pcm[0])                                         # (the device buffers exist and are idle)
    eng.sync()
    d_rec, d_cnt, d_snap = eng.events_dev_ptrs()
    assert d_rec and d_cnt and d_snap
    hip_memcpy = _hip()
    H2D, D2H = 1, 2
    rec_sent = np.full(32, 0xA5, dtype=np.uint8)
    snap_sent = np.full(rows * 96, -12345.0, dtype=np.float32)
    assert hip_memcpy(d_rec + 32 * cap, rec_sent.ctypes.data, rec_sent.nbytes, H2D) == 0
    assert hip_memcpy(d_snap + snap_sent.nbytes * cap, snap_sent.ctypes.data, snap_sent.nbytes, H2D) == 0
    overflowed = 0
    for t in range(1, steps):
        eng.step(pcm[t])
        want = events_from_scores(scores[t], None, None, thr)
        rec = _check(eng, want, np.full(S, t + 1), cap=cap)
        overflowed += len(want) > cap
        assert len(rec) == min(len(want), cap)
        if len(rec):
            np.testing.assert_array_equal(eng.event_features(), feats[t, rec["stream"], 16 - rows:])
        cnt = np.zeros(2, dtype=np.int32)
        assert hip_memcpy(cnt.ctypes.data, d_cnt, 8, D2H) == 0
        assert cnt.tolist() == [len(rec), len(want)]
    assert overflowed >= 3
    back_rec, back_snap = np.zeros_like(rec_sent), np.zeros_like(snap_sent)
    assert hip_memcpy(back_rec.ctypes.data, d_rec + 32 * cap, back_rec.nbytes, D2H) == 0
    assert hip_memcpy(back_snap.ctypes.data, d_snap + snap_sent.nbytes * cap, back_snap.nbytes, D2H) == 0
    np.testing.assert_array_equal(back_rec, rec_sent)
    np.testing.assert_array_equal(back_snap, snap_sent)
    # asking beyond what was stored is an argument error, not a read
    out = np.zeros((cap + 1, rows, 96), dtype=np.float32)
    assert eng._lib.oww_get_event_features(eng._h, 0, cap + 1, out.ctypes.data_as(C.c_void_p), 0) == EINVAL
    eng.close()


def test_masked_steps_report_participants_only():
    """Case 4: 12 steps at about 50 % random participation through oww_step_masked (PCM seed 13, mask seed 5).  Five steps with every
    stream on (also through oww_step_masked) come first: a stream's first five predictions read 0, and with half the streams sitting
    each step out too few pairs would be past them within 12 steps for the 20 % precondition to be reachable.  No event from a stream
    that sat out although its repeated row is at or above the threshold; frame counts the stream's own steps; nobody on -> (0, 0)."""
    S, warm, steps = 70, 5, 12
    rng = np.random.default_rng(5)
    masks = [np.ones(S, dtype=np.uint8)] * warm + [(rng.random(S) < 0.5).astype(np.uint8) for _ in range(steps)]
    pcm = W.synthetic_pcm(S, CHUNK * (warm + steps), seed=13)
    pcm = [np.ascontiguousarray(pcm[:, CHUNK * t: CHUNK * (t + 1)]) for t in range(warm + steps)]
    twin = _engine(S)
    scores = np.stack([twin.step_masked(pcm[t], masks[t]).copy() for t in range(warm + steps)])
    twin.close()
    on = np.stack(masks[warm:]).astype(bool)
    thr = _median_thresholds(scores[warm:], on)
    _assert_mixed(scores[warm:], thr, on)
    eng = _engine(S, event_capacity=256)
    eng.set_event_thresholds(thr)
    frames = np.zeros(S, dtype=np.int64)
    silent_hits = 0
    for t in range(warm + steps):
        got = eng.step_masked(pcm[t], masks[t])
        assert got.tobytes() == scores[t].tobytes()
        frames += masks[t]
        want = events_from_scores(scores[t], None, None, thr, participating=masks[t])
        rec = _check(eng, want, frames)
        assert masks[t][rec["stream"]].all()
        silent_hits += int(((scores[t] >= thr[None, :]).any(axis=1) & (masks[t] == 0)).sum())
        if t == warm + 6:                                    # a call nobody takes part in, in the middle of the run
            eng.step_masked(pcm[t], np.zeros(S, dtype=np.uint8))
            rec, total = eng.events()
            assert len(rec) == 0 and total == 0
    assert silent_hits > 0, "no sitting-out stream ever repeated a row at or above the threshold"
    eng.close()


def test_multi_chunk_and_long_calls_report_once():
    """Case 5: n_chunks = 2 and a long call (n_chunks = 3 at max_chunks = 2), alternating for 10 calls (PCM seed 14): one event per hit
    with the call's score (the maximum over its chunks, as oww_step returns it), frame = the call number."""
    S, ks = 70, [2, 3] * 5
    pcm = W.synthetic_pcm(S, CHUNK * sum(ks), seed=14)
    calls, o = [], 0
    for k in ks:
        calls.append(np.ascontiguousarray(pcm[:, CHUNK * o: CHUNK * (o + k)]))
        o += k
    twin = _engine(S, max_chunks=2)
    scores = np.stack([twin.step(x).copy() for x in calls])
    twin.close()
    thr = _median_thresholds(scores[5:])
    _assert_mixed(scores[5:], thr)
    eng = _engine(S, max_chunks=2, event_capacity=256)
    eng.set_event_thresholds(thr)
    for t, x in enumerate(calls):
        assert eng.step(x).tobytes() == scores[t].tobytes()
        _check(eng, events_from_scores(scores[t], None, None, thr), np.full(S, t + 1))
    eng.close()


@pytest.mark.parametrize("rows", [16, 3])
def test_snapshots_equal_the_ring_of_the_detecting_step(rows):
    """Case 6: every stored event's block is oww_get_features(stream, rows) read on the twin right after the same step, bit for bit; and
    it is a snapshot: with the next step already submitted the collected step's block still holds the old rows, which the ring (read
    after that next step) no longer does."""
    S, steps = 70, 12
    pcm, scores, thr, feats = _twin(S, steps, 11, 16)
    eng = _engine(S, event_capacity=256, event_features=rows)
    eng.set_event_thresholds(thr)
    n_blocks = 0
    for t in range(steps - 2):
        eng.step(pcm[t])
        rec = _check(eng, events_from_scores(scores[t], None, None, thr), np.full(S, t + 1))
        blocks = eng.event_features()
        assert blocks.shape == (len(rec), rows, 96)
        np.testing.assert_array_equal(blocks.view(np.uint32), feats[t, rec["stream"], 16 - rows:].view(np.uint32))
        if len(rec) > 2:                                     # a sub-range
            np.testing.assert_array_equal(eng.event_features(1, 2), blocks[1:3])
        n_blocks += len(rec)
    assert n_blocks > 0
    t = steps - 2
    eng.submit(pcm[t])
    eng.submit(pcm[t + 1])
    eng.collect()
    rec = _check(eng, events_from_scores(scores[t], None, None, thr), np.full(S, t + 1))
    assert len(rec) > 0
    blocks = eng.event_features()
    np.testing.assert_array_equal(blocks, feats[t, rec["stream"], 16 - rows:])
    ring_now = np.stack([eng.get_features(int(s), rows) for s in rec["stream"]])       # (waits for the step in flight)
    np.testing.assert_array_equal(ring_now, feats[t + 1, rec["stream"], 16 - rows:])
    assert all((blocks[i] != ring_now[i]).any() for i in range(len(rec)))
    eng.collect()
    eng.close()


def test_pipelined_steps_keep_their_own_events():
    """Case 7: submit, submit, collect, collect, then alternating, 10 steps, steps 4 and 8 masked (mask seed 6; PCM seed 11): events and
    snapshots of each collected step equal the synchronous twin's although a later step was already in flight."""
    S, steps, rows = 70, 10, 16
    rng = np.random.default_rng(6)
    masks = {3: (rng.random(S) < 0.5).astype(np.uint8), 7: (rng.random(S) < 0.5).astype(np.uint8)}
    pcm = W.synthetic_pcm(S, CHUNK * steps, seed=11)
    pcm = [np.ascontiguousarray(pcm[:, CHUNK * t: CHUNK * (t + 1)]) for t in range(steps)]
    twin = _engine(S)
    scores, feats = [], []
    for t in range(steps):
        scores.append((twin.step_masked(pcm[t], masks[t]) if t in masks else twin.step(pcm[t])).copy())
        feats.append(np.stack([twin.get_features(s, rows) for s in range(S)]))
    twin.close()
    scores = np.stack(scores)
    on = np.ones((steps, S), dtype=bool)
    for t, m in masks.items():
        on[t] = m != 0
    # streams that sat step 4 out are one prediction behind: their sixth step (the first nonzero one) is step 7 of the run
    thr = _median_thresholds(scores[5:], on[5:])
    _assert_mixed(scores[5:], thr, on[5:])
    eng = _engine(S, event_capacity=256, event_features=rows)
    eng.set_event_thresholds(thr)
    frames = np.zeros(S, dtype=np.int64)
    state = {"sub": 0, "col": 0, "events": 0}

    def submit():
        t = state["sub"]
        eng.submit(pcm[t], masks.get(t))
        state["sub"] += 1
        rec, total = eng.events()                            # between a submit and the next collect: zero events
        assert len(rec) == 0 and total == 0

    def collect():
        t = state["col"]
        assert eng.collect().tobytes() == scores[t].tobytes()
        frames[:] += on[t]
        rec = _check(eng, events_from_scores(scores[t], None, None, thr, participating=on[t]), frames)
        if len(rec):
            np.testing.assert_array_equal(eng.event_features(), feats[t][rec["stream"]])
        state["col"] += 1
        state["events"] += len(rec)

    submit(); submit(); collect(); collect()
    submit()
    while state["sub"] < steps:
        submit(); collect()
    collect()
    assert state["col"] == steps and state["events"] > 0
    eng.close()


def test_bank_events():
    """Case 9: S = 70, two bank slots, three bank heads, differing pairs with some slots empty (PCM seed 15).  The bank threshold is the
    median of the twin's nonzero oww_bank_scores values, with the same 20 % check over the subscribed slots.  Events carry ~slot and the
    subscribed id; an empty slot never reports; after bank_remove the id's events stop on the next step.  The handle has no fixed
    heads: frame is still the stream's prediction counter, the step number."""
    S, K, steps = 70, 2, 12
    bank = [W.synthetic_head(n, 1234) for n in FIXED]
    sub = np.full((S, K), -1, dtype=np.int32)
    for s in range(S):
        sub[s, 0] = (0, 1, 2, -1, 0)[s % 5]
        sub[s, 1] = (1, 2, -1, 0, 0)[s % 5]
    pcm = W.synthetic_pcm(S, CHUNK * steps, seed=15)
    pcm = [np.ascontiguousarray(pcm[:, CHUNK * t: CHUNK * (t + 1)]) for t in range(steps)]

    def make(**kw):
        e = _engine(S, heads={}, bank_slots=K, bank_capacity=8, **kw)
        ids = [e.bank_add(h) for h in bank]
        assert ids == [0, 1, 2]
        e.subscribe(np.arange(S), sub)
        return e

    twin = make()
    bs = []
    for t in range(steps):
        if t == 9:
            twin.bank_remove(1)
        twin.step(pcm[t])
        bs.append(twin.bank_scores().copy())
    twin.close()
    bs = np.stack(bs)
    live = np.broadcast_to(sub >= 0, bs[5:].shape)
    vals = bs[5:][live]
    bank_thr = np.float32(np.median(vals[vals != 0]))
    frac = float((vals >= bank_thr).mean())
    print(f"bank hit fraction over subscribed slots, steps 6-12: {frac:.3f}")
    assert 0.2 <= frac <= 0.8, frac

    eng = make(event_capacity=256, event_features=16)
    assert eng.n_labels == 0
    eng.set_event_thresholds(None, bank=float(bank_thr))
    cur = sub.copy()
    n_removed_before = 0
    for t in range(steps):
        if t == 9:
            eng.bank_remove(1)
            cur[cur == 1] = -1
        eng.step(pcm[t])
        got = eng.bank_scores()
        assert got.tobytes() == bs[t].tobytes()
        want = events_from_scores(None, bs[t], cur, (), bank_thr)
        rec = _check(eng, want, np.full(S, t + 1))
        assert (rec["column"] < 0).all()
        assert (cur[rec["stream"], ~rec["column"]] == rec["bank_id"]).all()
        assert [eng.event_label(r) for r in rec] == rec["bank_id"].tolist()
        if 5 <= t < 9:
            n_removed_before += int((rec["bank_id"] == 1).sum())
        if t >= 9:
            assert not (rec["bank_id"] == 1).any()
    assert n_removed_before > 0
    eng.close()


def test_events_are_off_by_default_and_change_no_score():
    """Case 10: without event_capacity oww_get_events returns OWW_ESTATE (asserted at the twin) and the scores of 12 steps are byte-equal
    to a handle with events on; the launches a handle without events times are the ones it timed before, an events handle adds two
    under the post-processing class."""
    S, steps = 70, 12
    pcm, scores, thr, _ = _twin(S, steps, 11, 16)
    counts = []
    for kw in ({}, dict(event_capacity=64, event_features=16)):
        eng = _engine(S, **kw)
        eng.enable_timing(True)
        for t in range(steps):
            assert eng.step(pcm[t]).tobytes() == scores[t].tobytes()
        counts.append({k: v["launches"] for k, v in eng.kernel_times().items()})
        lib, h = eng._lib, eng._h
        for rc in (lib.oww_get_events(h, None, 0, None, None), lib.oww_events_set_thresholds(h, None, 0.5),
                   lib.oww_get_event_features(h, 0, 0, None, 0)):
            assert rc == (0 if kw else ESTATE)
        assert (lib.oww_event_features_dev(h) is not None) == bool(kw)
        eng.close()
    off, on = counts
    assert on["postproc"] == off["postproc"] + 2 * steps
    assert {k: v for k, v in on.items() if k != "postproc"} == {k: v for k, v in off.items() if k != "postproc"}


def test_configure_limits_and_labels():
    """capacity in [1, 1 << 20] and feature_rows in [0, the feature ring]: OWW_EINVAL (the ring is known at oww_commit); fixed-column
    events name their label."""
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(0, 4, 1, 0, 3, 0, None)
    assert lib.oww_create(C.byref(cfg), C.byref(h)) == 0
    try:
        for cap, rows in ((0, 0), (-1, 0), ((1 << 20) + 1, 0), (16, -1)):
            assert lib.oww_events_configure(h, cap, rows) == EINVAL, (cap, rows)
        assert lib.oww_events_configure(h, 16, 16) == 0
        assert lib.oww_get_events(h, None, 0, None, None) == ESTATE           # not committed
    finally:
        lib.oww_destroy(h)
    with pytest.raises(ValueError, match="feature ring"):
        _engine(4, event_capacity=16, event_features=17)
    # the library's own check, behind the Python one: a ring of 16 rows refuses 17 at commit
    eng = _engine(4, event_capacity=16, event_features=16)
    assert lib.oww_events_configure(eng._h, 16, 16) == ESTATE                 # after commit
    assert [eng.event_label({"column": c, "bank_id": -1}) for c in range(3)] == FIXED
    eng.close()
    import openwakeword_amd.engine as E
    saved = E.check_event_config
    E.check_event_config = lambda cap, rows, ring: (int(cap), int(rows))
    try:
        with pytest.raises(_lib.OwwError, match="feature ring"):
            _engine(4, event_capacity=16, event_features=17)
    finally:
        E.check_event_config = saved
