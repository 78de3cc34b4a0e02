"""Per-stream audio rings on the GPU (include/owwhip.h: oww_audio_configure / oww_get_audio / oww_get_event_audio; kernels in
csrc/owwhip_audio.h).  The definition is engine.audio_ring_model (held to a deque by tests/test_audio_cpu.py): every ring read, every
counter and every event snapshot is compared with it bit for bit, and the scores with a twin handle that keeps no audio.  Engines,
heads, PCM and the median event thresholds are those of tests/test_events_gpu.py (its 70-stream twin run is shared: S = 70 is 17 full
four-wave workgroups of audio_append_kernel plus a partial one)."""
import ctypes as C
import os

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import CHUNK, StreamEngine, audio_ring_model, events_from_scores
from test_events_gpu import _assert_mixed, _engine, _hip, _median_thresholds, _twin

pytestmark = pytest.mark.gpu

S = 70
ALL = np.arange(S)
ODD_LIST = [69, 0, 0, 33]
EINVAL, ESTATE = -1, -3
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _same(eng, model, ns, ids=ALL):
    """audio() of `ids` at every n_chunks of `ns`, the duplicate / unordered list and the counters against the model."""
    for n in ns:
        got, cnt = eng.audio(ids, n)
        assert got.dtype == np.int16 and got.shape == (len(ids), n * CHUNK) and cnt.dtype == np.uint32
        np.testing.assert_array_equal(got, model.last(ids, n))
        np.testing.assert_array_equal(cnt, model.counts[np.asarray(ids)])
    got, cnt = eng.audio(ODD_LIST, ns[-1])
    np.testing.assert_array_equal(got, model.last(ODD_LIST, ns[-1]))
    np.testing.assert_array_equal(cnt, model.counts[ODD_LIST])


def _chunks(seed, k_list):
    pcm = W.synthetic_pcm(S, CHUNK * sum(k_list), seed=seed)
    out, o = [], 0
    for k in k_list:
        out.append(np.ascontiguousarray(pcm[:, CHUNK * o: CHUNK * (o + k)]))
        o += k
    return out


# ---- 1. the ring equals the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_ring_equals_the_model(graph):
    """ring_chunks = 5, 12 one-chunk steps (the ring wraps twice); scores byte-equal to the twin without audio; a handle without audio
    times the launches it timed before, the audio handle one more per step under the post-processing class (not under a graph: timing
    turns the replay off)."""
    steps, ring = 12, 5
    pcm, scores, _, _ = _twin(S, steps, 11, 16)
    eng = _engine(S, audio_chunks=ring)
    off = None
    if graph:
        eng.use_graph(True)
    else:
        eng.enable_timing(True)
        off = _engine(S)
        off.enable_timing(True)
    model = audio_ring_model(S, ring)
    _same(eng, model, (1, 3, 5))                             # before the first step: zeros, counters 0
    assert not eng.audio(ALL, 5)[0].any() and not eng.audio(ALL, 5)[1].any()
    for t in range(steps):
        assert eng.step(pcm[t]).tobytes() == scores[t].tobytes()
        if off is not None:
            assert off.step(pcm[t]).tobytes() == scores[t].tobytes()
        model.append(pcm[t])
        _same(eng, model, (1, 3, 5))
    assert model.counts.tolist() == [steps] * S
    if off is not None:
        a = {k: v["launches"] for k, v in eng.kernel_times().items()}
        b = {k: v["launches"] for k, v in off.kernel_times().items()}
        assert a["postproc"] == b["postproc"] + steps
        assert {k: v for k, v in a.items() if k != "postproc"} == {k: v for k, v in b.items() if k != "postproc"}
        off.close()
    eng.close()


# ---- 2. multi-chunk and long calls -----------------------------------------------------------------------------------------------------------
def test_multi_chunk_and_long_calls():
    """ring_chunks = 5: a 3-chunk call after 4 single steps (the wrap falls inside the call), a 7-chunk call at max_chunks = 8 (the last
    5 chunks stay, the counter advances by 7), and calls of 5 and 3 chunks at max_chunks = 2 (the sliced long path: one append)."""
    ring = 5
    ks = [1, 1, 1, 1, 3, 7, 1]
    eng = _engine(S, max_chunks=8, audio_chunks=ring)
    model = audio_ring_model(S, ring)
    total = 0
    for x, k in zip(_chunks(21, ks), ks):
        eng.step(x)
        model.append(x)
        total += k
        _same(eng, model, (1, 3, 5))
        assert eng.audio([0, S - 1], 1)[1].tolist() == [total, total]
        if k == 7:
            np.testing.assert_array_equal(eng.audio(ALL, 5)[0], x[:, 2 * CHUNK:])
    eng.close()
    ks = [1, 5, 3, 2]
    eng = _engine(S, max_chunks=2, audio_chunks=ring)
    model = audio_ring_model(S, ring)
    for x in _chunks(22, ks):
        eng.step(x)
        model.append(x)
        _same(eng, model, (1, 2, 5))
    assert model.counts[0] == sum(ks)
    eng.close()


# ---- 3. masked steps --------------------------------------------------------------------------------------------------------------------------
def test_masked_steps_move_participants_only():
    """10 steps at 30 % participation by a host mask (the participant-list form), one at 95 % (the mask alone), a device-resident mask,
    and masks nobody takes part in (host and device): after every step every stream's ring and counter, bystanders included."""
    import torch
    ring, steps = 5, 14
    rng = np.random.default_rng(31)
    pcm = _chunks(23, [1] * steps)
    masks = [(rng.random(S) < 0.3).astype(np.uint8) for _ in range(10)] + [(rng.random(S) < 0.95).astype(np.uint8)]
    assert all(0 < m.sum() < S for m in masks)
    eng = _engine(S, audio_chunks=ring)
    twin = _engine(S)
    model = audio_ring_model(S, ring)
    for t, m in enumerate(masks):
        assert eng.step_masked(pcm[t], m).tobytes() == twin.step_masked(pcm[t], m).tobytes()
        model.append(pcm[t], m)
        _same(eng, model, (1, 5))
    t = len(masks)
    eng.step_masked(pcm[t], np.zeros(S, dtype=np.uint8))    # nobody: nothing moves
    _same(eng, model, (1, 5))
    d_scores = torch.zeros((S, eng.n_labels), dtype=torch.float32, device="cuda")
    for m in ((rng.random(S) < 0.3).astype(np.uint8), np.zeros(S, dtype=np.uint8)):
        t += 1
        d_pcm = torch.from_numpy(pcm[t].copy()).cuda()
        d_on = torch.from_numpy(m.copy()).cuda()
        torch.cuda.synchronize()
        _lib.check(eng._lib.oww_step_masked(eng._h, C.c_void_p(d_pcm.data_ptr()), 1, C.c_void_p(d_on.data_ptr()), 1,
                                            C.c_void_p(d_scores.data_ptr()), 1))
        eng.sync()
        model.append(pcm[t], m)
        _same(eng, model, (1, 5))
    assert 0 < model.counts.min() < model.counts.max()
    eng.close(); twin.close()


# ---- 4. unaligned device PCM ------------------------------------------------------------------------------------------------------------------
def test_unaligned_device_pcm():
    """oww_step on a device pointer 2 bytes off a 16-byte boundary (one chunk, then two): the ring and the scores are those of the same
    calls on an aligned pointer."""
    import torch
    ring = 5
    ks = [1, 1, 2, 1, 1, 2, 1]
    calls = _chunks(24, ks)
    a, b = _engine(S, max_chunks=2, audio_chunks=ring), _engine(S, max_chunks=2, audio_chunks=ring)
    model = audio_ring_model(S, ring)
    sa = torch.zeros((S, a.n_labels), dtype=torch.float32, device="cuda")
    sb = torch.zeros_like(sa)
    for x, k in zip(calls, ks):
        d_al = torch.from_numpy(x.copy()).cuda()
        d_odd = torch.zeros(x.size + 16, dtype=torch.int16, device="cuda")
        d_odd[1:1 + x.size] = d_al.reshape(-1)
        assert d_al.data_ptr() % 16 == 0 and (d_odd.data_ptr() + 2) % 16 == 2
        torch.cuda.synchronize()
        a.step_device(d_al.data_ptr(), k, sa.data_ptr())
        b.step_device(d_odd.data_ptr() + 2, k, sb.data_ptr())
        a.sync(); b.sync()
        model.append(x)
        _same(a, model, (1, 5))
        _same(b, model, (1, 5))
        assert sb.cpu().numpy().tobytes() == sa.cpu().numpy().tobytes()
    assert sa.cpu().numpy().any()
    a.close(); b.close()


# ---- 5. ingest ----------------------------------------------------------------------------------------------------------------------------------
def test_ingest_appends_what_the_front_end_consumed():
    """(8000, mu-law): the ring after step_ingest holds the staging buffer's decoded and resampled samples -- the same messages through
    ingest() on a twin handle -- over 6 steps, one of them masked."""
    ring, steps = 5, 6
    rng = np.random.default_rng(51)
    eng, twin = _engine(S, audio_chunks=ring), _engine(S)
    eng.configure_ingest(8000, "ulaw"); twin.configure_ingest(8000, "ulaw")
    model = audio_ring_model(S, ring)
    for t in range(steps):
        msg = rng.integers(0, 256, (S, 640)).astype(np.uint8)
        on = (rng.random(S) < 0.5).astype(np.uint8) if t == 3 else None
        eng.step_ingest(msg, on)
        pcm16 = twin.ingest(msg, on)
        assert pcm16.shape == (S, CHUNK) and pcm16.any()
        model.append(pcm16, on)
        _same(eng, model, (1, 5))
    eng.close(); twin.close()


def test_mixed_ingest_appends_synchronous_and_pipelined():
    """Three classes (8 kHz mu-law, 16 kHz PCM, 48 kHz PCM): the ring after step_ingest_mixed (predict_ingest_mixed's engine call) and
    after submit_ingest_mixed + collect equals ingest_mixed of the same rows on a twin, bit for bit."""
    from openwakeword_amd import resample as R
    ring = 5
    classes = [(8000, "ulaw"), (16000, "pcm16"), (48000, "pcm16")]
    cls = (ALL % 3).astype(np.uint8)
    rng = np.random.default_rng(52)
    eng, twin = _engine(S, audio_chunks=ring), _engine(S)
    for e in (eng, twin):
        e.configure_ingest_classes(classes)
        e.assign_ingest(ALL, cls)
    model = audio_ring_model(S, ring)

    def rows():
        arrs = []
        for s in range(S):
            rate, enc = classes[cls[s]]
            n = R.class_n_in(rate, CHUNK)
            arrs.append(rng.integers(0, 256, n).astype(np.uint8) if enc != "pcm16" else (rng.standard_normal(n) * 3000).astype(np.int16))
        return eng.pack_ingest_rows(arrs, cls)

    for t in range(3):                                       # synchronous
        r = rows()
        eng.step_ingest_mixed(r)
        model.append(twin.ingest_mixed(r))
        _same(eng, model, (1, 5))
    sent = [rows() for _ in range(4)]                        # pipelined: two in flight, one of them masked
    on = (rng.random(S) < 0.5).astype(np.uint8)
    eng.submit_ingest_mixed(sent[0]); eng.submit_ingest_mixed(sent[1], on); eng.collect()
    eng.submit_ingest_mixed(sent[2]); eng.collect(); eng.collect()
    eng.submit_ingest_mixed(sent[3]); eng.collect()
    for i, r in enumerate(sent):
        m = on if i == 1 else None
        model.append(twin.ingest_mixed(r, stream_on=m), m)
    _same(eng, model, (1, 4, 5))
    eng.close(); twin.close()


# ---- 6. event audio --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,ev", [(8, 8), (5, 3)])
def test_event_audio_is_the_ring_of_the_detecting_step(ring, ev):
    """Capacity 256, 12 steps: snapshot i is the model's last `ev` chunks of record i's stream at that step; at step 6, the first with
    events, an 8-chunk snapshot begins with exactly two zero chunks."""
    steps = 12
    pcm, scores, thr, _ = _twin(S, steps, 11, 16)
    _assert_mixed(scores[5:], thr)
    eng = _engine(S, event_capacity=256, audio_chunks=ring, event_audio=ev)
    eng.set_event_thresholds(thr)
    model = audio_ring_model(S, ring)
    assert eng.event_audio().shape == (0, ev * CHUNK)
    n_events = 0
    for t in range(steps):
        assert eng.step(pcm[t]).tobytes() == scores[t].tobytes()
        model.append(pcm[t])
        want = events_from_scores(scores[t], None, None, thr)
        rec, total = eng.events()
        assert total == len(want) and rec["stream"].tolist() == [w[0] for w in want]
        snaps = eng.event_audio()
        assert snaps.dtype == np.int16 and snaps.shape == (len(rec), ev * CHUNK)
        np.testing.assert_array_equal(snaps, model.last(rec["stream"], ev))
        if len(rec):
            np.testing.assert_array_equal(snaps[:, -CHUNK:], pcm[t][rec["stream"]])      # it ends with the detecting chunk
        if len(rec) > 2:
            np.testing.assert_array_equal(eng.event_audio(1, 2), snaps[1:3])
        if t < 5:
            assert len(rec) == 0
        if t == 5:
            assert len(rec) > 0
            if ev == 8:
                assert not snaps[:, :2 * CHUNK].any() and all(snaps[i, 2 * CHUNK:3 * CHUNK].any() for i in range(len(rec)))
        n_events += len(rec)
    assert n_events > 0
    _same(eng, model, (1, ring))
    eng.close()


def test_event_audio_overflow_is_bounded():
    """Capacity 4 on the same run: 4 snapshots, n_total unchanged, and the spare snapshot behind index 3 keeps the bytes planted there
    through oww_event_audio_dev."""
    steps, ring, ev, cap = 12, 8, 8, 4
    pcm, scores, thr, _ = _twin(S, steps, 11, 16)
    eng = _engine(S, event_capacity=cap, audio_chunks=ring, event_audio=ev)
    eng.set_event_thresholds(thr)
    model = audio_ring_model(S, ring)
    eng.step(pcm[0]); model.append(pcm[0])
    eng.sync()
    d_snap = eng.event_audio_dev_ptr()
    assert d_snap and d_snap % 16 == 0
    hip_memcpy = _hip()
    H2D, D2H = 1, 2
    sent = np.full(ev * CHUNK, -12345, dtype=np.int16)
    assert hip_memcpy(d_snap + sent.nbytes * cap, sent.ctypes.data, sent.nbytes, H2D) == 0
    overflowed = 0
    for t in range(1, steps):
        eng.step(pcm[t]); model.append(pcm[t])
        want = events_from_scores(scores[t], None, None, thr)
        rec, total = eng.events()
        assert total == len(want) and len(rec) == min(len(want), cap)
        overflowed += len(want) > cap
        snaps = eng.event_audio()
        assert snaps.shape[0] == len(rec)
        np.testing.assert_array_equal(snaps, model.last(rec["stream"], ev))
        if len(rec):                                         # the device buffer of the synchronous call holds the same snapshots
            dev = np.zeros_like(snaps)
            assert hip_memcpy(dev.ctypes.data, d_snap, dev.nbytes, D2H) == 0
            np.testing.assert_array_equal(dev, snaps)
    assert overflowed >= 3
    back = np.zeros_like(sent)
    assert hip_memcpy(back.ctypes.data, d_snap + sent.nbytes * cap, back.nbytes, D2H) == 0
    np.testing.assert_array_equal(back, sent)
    out = np.zeros((cap + 1, ev * CHUNK), dtype=np.int16)
    assert eng._lib.oww_get_event_audio(eng._h, 0, cap + 1, out.ctypes.data_as(C.c_void_p), 0) == EINVAL
    eng.close()


# ---- 7. pipelined -------------------------------------------------------------------------------------------------------------------------------
def test_pipelined_steps_keep_their_own_event_audio():
    """Six synchronous steps (the first-5 zeroing), then submit, submit, collect, submit, collect, collect: each collected step's
    event_audio is its own step's although a later step is in flight; audio() after the last collect equals the model."""
    steps, ring, ev = 9, 5, 3
    pcm, scores, thr, _ = _twin(S, 12, 11, 16)
    eng = _engine(S, event_capacity=256, audio_chunks=ring, event_audio=ev)
    eng.set_event_thresholds(thr)
    model = audio_ring_model(S, ring)
    want_audio = []
    for t in range(steps):
        model.append(pcm[t])
        want_audio.append(model.last(ALL, ev))
    for t in range(6):
        eng.step(pcm[t])
    state = {"sub": 6, "col": 6, "events": 0}

    def submit():
        eng.submit(pcm[state["sub"]])
        state["sub"] += 1
        with pytest.raises(_lib.OwwError):                   # between a submit and the next collect: zero events, nothing to read
            eng.event_audio(0, 1)

    def collect():
        t = state["col"]
        assert eng.collect().tobytes() == scores[t].tobytes()
        rec, _ = eng.events()
        assert rec["stream"].tolist() == [w[0] for w in events_from_scores(scores[t], None, None, thr)]
        np.testing.assert_array_equal(eng.event_audio(), want_audio[t][rec["stream"]])
        state["col"] += 1
        state["events"] += len(rec)

    submit(); submit(); collect(); submit(); collect(); collect()
    assert state["col"] == steps and state["events"] > 0
    _same(eng, model, (1, 3, 5))
    eng.close()


# ---- 8. reset -------------------------------------------------------------------------------------------------------------------------------------
def test_reset_zeroes_ring_and_counter():
    """After 7 steps oww_reset of streams [3, 64]: their rings and counters read zero, every other stream keeps every bit, and their
    next snapshot zero-fills again (event thresholds 0, so that the freshly reset streams -- scores 0 -- report)."""
    ring, ev = 5, 3
    pcm = _chunks(25, [1] * 9)
    eng = _engine(S, event_capacity=256, audio_chunks=ring, event_audio=ev)
    model = audio_ring_model(S, ring)
    for t in range(7):
        eng.step(pcm[t]); model.append(pcm[t])
    eng.reset([3, 64]); model.reset([3, 64])
    got, cnt = eng.audio(ALL, ring)
    assert not got[[3, 64]].any() and cnt[[3, 64]].tolist() == [0, 0] and (np.delete(cnt, [3, 64]) == 7).all()
    _same(eng, model, (1, 5))
    eng.set_event_thresholds(np.zeros(eng.n_labels, dtype=np.float32))
    for t in (7, 8):
        eng.step(pcm[t]); model.append(pcm[t])
        rec, total = eng.events()
        assert total == S * eng.n_labels == len(rec)
        snaps = eng.event_audio()
        np.testing.assert_array_equal(snaps, model.last(rec["stream"], ev))
        mine = snaps[np.isin(rec["stream"], [3, 64])]
        assert len(mine) == 2 * eng.n_labels and not mine[:, :(ev - (t - 6)) * CHUNK].any() and mine[:, -CHUNK:].any()
    eng.reset(); model.reset()                               # every stream
    _same(eng, model, (1, 5))
    assert not eng.audio(ALL, 5)[1].any()
    eng.close()


# ---- 9. state records ---------------------------------------------------------------------------------------------------------------------------
def test_state_records_carry_ring_and_counter():
    ring, ev, first, more = 5, 3, 7, 4
    pcm, scores, thr, _ = _twin(S, 12, 11, 16)
    plain, plain2 = _engine(S, event_capacity=256), _engine(S, event_capacity=256)
    a = _engine(S, event_capacity=256, audio_chunks=ring, event_audio=ev)
    b = _engine(S, event_capacity=256, audio_chunks=ring, event_audio=ev)
    nb0, fp0 = plain.state_info()
    assert plain2.state_info() == (nb0, fp0)                 # audio off: the record and the fingerprint of a handle without it
    nb, fp = a.state_info()
    assert nb == nb0 + ring * 2560 + 16 and fp != fp0 and b.state_info() == (nb, fp)
    hdr = plain.export_state([0]).view(np.uint32)[0, :8]
    assert hdr[1] == 1 and hdr[2] == nb0                     # kLayoutVersion stays 1
    assert "kLayoutVersion = 1u" in open(os.path.join(ROOT, "openwakeword_amd", "csrc", "owwhip_state_host.h")).read()     # (the record constants' home)
    plain.close(); plain2.close()
    for e in (a, b):
        e.set_event_thresholds(thr)
    model = audio_ring_model(S, ring)
    for t in range(first):
        assert a.step(pcm[t]).tobytes() == b.step(pcm[t]).tobytes() == scores[t].tobytes()
        model.append(pcm[t])
    # a different ring is another configuration: refused, nothing moves
    other = _engine(S, event_capacity=256, audio_chunks=6, event_audio=ev)
    other.step(pcm[0])
    rec = a.export_state([7, 9])
    before = (other.audio(ALL, 6), other.export_state([0, 1]))
    ids = np.array([0], dtype=np.int32)
    assert other._lib.oww_state_import(other._h, ids.ctypes.data_as(C.c_void_p), 1, rec.ctypes.data_as(C.c_void_p), 0) == EINVAL
    assert b"another configuration" in other._lib.oww_last_error()
    after = (other.audio(ALL, 6), other.export_state([0, 1]))
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    other.close()
    # travel: records of a's [7, 9] into b's [0, 1], b's 40 -> 3, and 10 <-> 11
    b.import_state([0, 1], rec)
    b.move_streams([40], [3])
    b.move_streams([10, 11], [11, 10])
    src = ALL.copy()
    src[[0, 1, 3, 10, 11]] = [7, 9, 40, 11, 10]
    got, cnt = b.audio(ALL, ring)
    np.testing.assert_array_equal(got, model.last(src, ring))
    assert cnt.tolist() == [first] * S
    travelled = [0, 1, 3, 10, 11]
    n_snap = 0
    for t in range(first, first + more):
        sa, sb = a.step(pcm[t]), b.step(np.ascontiguousarray(pcm[t][src]))
        assert sa.tobytes() == scores[t].tobytes() and sb.tobytes() == scores[t][src].tobytes()
        model.append(pcm[t])
        ra, _ = a.events()
        rb, _ = b.events()
        snap_a = {(int(r["stream"]), int(r["column"])): x for r, x in zip(ra, a.event_audio())}
        for r, x in zip(rb, b.event_audio()):
            np.testing.assert_array_equal(x, snap_a[(int(src[r["stream"]]), int(r["column"]))])
            n_snap += int(r["stream"]) in travelled
        assert len(ra) > 0 and len(rb) > 0
        ga, ca = a.audio(src, ring)
        gb, cb = b.audio(ALL, ring)
        np.testing.assert_array_equal(gb, ga)
        np.testing.assert_array_equal(gb, model.last(src, ring))
        np.testing.assert_array_equal(cb, ca)
    assert n_snap > 0, "no travelled stream ever reported"
    a.close(); b.close()


# ---- 10. borrowers ------------------------------------------------------------------------------------------------------------------------------
def test_borrowed_stream_entries_touch_no_ring():
    """embed_clips and embed on 8 clips between two steps borrow streams 0 .. 7: every ring and counter keeps every bit."""
    ring = 5
    pcm = _chunks(26, [1] * 4)
    eng = _engine(S, audio_chunks=ring)
    model = audio_ring_model(S, ring)
    for t in range(3):
        eng.step(pcm[t]); model.append(pcm[t])
    before = eng.audio(ALL, ring)
    clips = W.synthetic_pcm(8, 16000, seed=27)
    assert np.isfinite(eng.embed_clips(clips)).all()
    assert np.isfinite(eng.embed(np.random.default_rng(28).standard_normal((8, 76, 32)).astype(np.float32))).all()
    eng.mel(clips)
    after = eng.audio(ALL, ring)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    eng.step(pcm[3]); model.append(pcm[3])
    _same(eng, model, (1, 5))
    eng.close()


# ---- 11. limits -------------------------------------------------------------------------------------------------------------------------------
def test_limits_through_the_c_abi():
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    cfg = _lib.Config(0, 4, 1, 0, 3, 0, None)
    assert lib.oww_create(C.byref(cfg), C.byref(h)) == 0
    try:
        for ring, ev in ((0, 0), (-1, 0), (1025, 0), (5, -1), (5, 6), (1, 2)):
            assert lib.oww_audio_configure(h, ring, ev) == EINVAL, (ring, ev)
        assert lib.oww_audio_configure(h, 1024, 1024) == 0 and lib.oww_audio_configure(h, 5, 0) == 0
        ids = np.zeros(1, dtype=np.int32)
        out = np.zeros(5 * CHUNK, dtype=np.int16)
        assert lib.oww_get_audio(h, vp(ids), 1, 1, vp(out), 0, None) == ESTATE          # not committed
        assert lib.oww_event_audio_dev(h) is None
    finally:
        lib.oww_destroy(h)
    # a handle without audio: the three read entries say so
    plain = _engine(4, event_capacity=16)
    plain.step(W.synthetic_pcm(4, CHUNK, seed=1))
    assert lib.oww_get_audio(plain._h, vp(ids), 1, 1, vp(out), 0, None) == ESTATE
    assert lib.oww_get_event_audio(plain._h, 0, 0, None, 0) == ESTATE
    assert lib.oww_event_audio_dev(plain._h) is None
    with pytest.raises(_lib.OwwError, match="keeps no audio"):
        plain.audio([0], 1)
    plain.close()
    # event_chunks > 0 without events: the Python check first, the library's own behind it at oww_commit
    with pytest.raises(ValueError, match="event_capacity"):
        _engine(4, audio_chunks=5, event_audio=3)
    import openwakeword_amd.engine as E
    saved = E.check_audio_config
    E.check_audio_config = lambda ring, ev, cap: (int(ring), int(ev))
    try:
        with pytest.raises(_lib.OwwError, match="needs events"):
            _engine(4, audio_chunks=5, event_audio=3)
    finally:
        E.check_audio_config = saved
    # audio without snapshots: the event-audio entries refuse, everything else works
    eng = _engine(4, event_capacity=16, audio_chunks=5)
    model = audio_ring_model(4, 5)
    x = W.synthetic_pcm(4, CHUNK, seed=2)
    eng.step(x); model.append(x)
    hh = eng._h
    assert lib.oww_audio_configure(hh, 5, 0) == ESTATE                                # after commit
    assert lib.oww_get_event_audio(hh, 0, 0, None, 0) == EINVAL and b"event_chunks = 0" in lib.oww_last_error()
    assert lib.oww_event_audio_dev(hh) is None
    cnt = np.zeros(2, dtype=np.uint32)
    two = np.array([3, 0], dtype=np.int32)
    big = np.zeros(2 * 5 * CHUNK, dtype=np.int16)
    for n_chunks in (0, -1, 6):
        assert lib.oww_get_audio(hh, vp(two), 2, n_chunks, vp(big), 0, vp(cnt)) == EINVAL, n_chunks
    for bad in (4, -1):
        assert lib.oww_get_audio(hh, vp(np.array([0, bad], dtype=np.int32)), 2, 1, vp(big), 0, vp(cnt)) == EINVAL, bad
    assert lib.oww_get_audio(hh, None, 1, 1, vp(big), 0, None) == EINVAL and lib.oww_get_audio(hh, vp(two), 2, 1, None, 0, None) == EINVAL
    assert lib.oww_get_audio(hh, vp(two), 2, 1, C.c_void_p(0x1002), 1, None) == EINVAL        # a device buffer off 16 bytes: refused unread
    assert lib.oww_get_audio(hh, None, 0, 1, None, 0, None) == 0                              # an empty list is no error
    assert not big.any() and not cnt.any()
    got, c = eng.audio([0, 1, 2, 3], 5)                      # every refusal left the handle as it was
    np.testing.assert_array_equal(got, model.last([0, 1, 2, 3], 5))
    assert c.tolist() == [1] * 4
    eng.close()
    # with snapshots: a record range beyond n_stored
    eng = _engine(4, event_capacity=16, audio_chunks=5, event_audio=2)
    eng.set_event_thresholds(np.zeros(eng.n_labels, dtype=np.float32))
    eng.step(x)
    rec, total = eng.events()
    assert len(rec) == total == 4 * eng.n_labels
    buf = np.zeros((len(rec) + 1, 2 * CHUNK), dtype=np.int16)
    assert lib.oww_get_event_audio(eng._h, 0, len(rec) + 1, vp(buf), 0) == EINVAL
    assert lib.oww_get_event_audio(eng._h, len(rec), 1, vp(buf), 0) == EINVAL
    assert lib.oww_get_event_audio(eng._h, -1, 1, vp(buf), 0) == EINVAL
    assert lib.oww_get_event_audio(eng._h, 1, 2, None, 0) == EINVAL
    assert not buf.any()
    assert lib.oww_get_event_audio(eng._h, len(rec) - 1, 1, vp(buf), 0) == 0
    np.testing.assert_array_equal(buf[0, CHUNK:], x[rec["stream"][-1]])
    assert not buf[0, :CHUNK].any()
    assert eng.event_audio_dev_ptr() != 0
    eng.close()
