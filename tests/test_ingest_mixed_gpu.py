"""Ingest classes on the device (`ingest_mixed_kernel` / oww_ingest_configure_classes / oww_ingest_assign / oww_ingest_mixed /
oww_step_ingest_mixed / oww_submit_ingest_mixed): 37 streams in six classes in one launch.  The contract is bit equality, per stream,
with `ingest_kernel` on a single-format handle fed that stream's data; on top of it the derived budget `0.5 + gamma * A` against the
float64 definition (tests/resample_ref.py), message cuts, masks, state records, the step behind the ingest and the pipelined form.
Two tolerances only: RR.excess <= 0 and bit equality; the end-to-end comparison adds the project's by-path score tolerance 1e-4.

Classes: decode only (16 kHz), the sliding form (8 kHz mu-law and A-law, q = 2), p > H with the largest bank (11.025 kHz, q = 640),
and two general forms with different n_taps (44.1 and 48 kHz) -- so only the 48 kHz streams use the whole history row."""
import ctypes as C
import functools

import numpy as np
import pytest

import resample_ref as RR
from openwakeword_amd import resample as R
from openwakeword_amd import weights as W

pytestmark = pytest.mark.gpu
S = RR.ROWS
CLASSES = [(16000, "pcm16"), (8000, "ulaw"), (8000, "alaw"), (11025, "pcm16"), (44100, "pcm16"), (48000, "pcm16")]
CLS = (np.arange(S) % len(CLASSES)).astype(np.uint8)
N_MSG, N_OUT = 6, 1280
TOTAL = N_MSG * N_OUT
OWW_EINVAL, OWW_ESTATE = -1, -3
HPAD_MAX = max((R.class_params(r, e)[3] - 1 + 7) // 8 * 8 if r != 16000 else 0 for r, e in CLASSES)


def _new_engine(n_streams=S, **kw):
    from openwakeword_amd.engine import StreamEngine
    return StreamEngine(n_streams, {"alexa": W.synthetic_head("alexa", seed=1)}, W.synthetic_embedding(seed=3), **kw)


@pytest.fixture(scope="module")
def eng():
    e = _new_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def single():
    """a second handle of the same construction: the single-format reference runs, and the other side of export / import"""
    e = _new_engine()
    yield e
    e.close()


def _vp(a):
    return None if a is None else (C.c_void_p(int(a)) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p))


def _lib():
    from openwakeword_amd import _lib as L
    return L.load()


def _err():
    return _lib().oww_last_error().decode(errors="replace")


@functools.lru_cache(maxsize=None)
def whole(c):
    """what a single-format handle of class c is fed for the whole recording: [S, n_in] (row s is what stream s gets when it is in
    class c).  G.711: random codes, the first four G.711 streams of the population (1, 2, 7, 8) the constant codes 0x00 / 0xFF / 0x7F /
    0x55."""
    rate, enc = CLASSES[c]
    n = R.class_n_in(rate, TOTAL)
    if enc == "pcm16":
        x = np.ascontiguousarray(RR.signals(rate, n))
    else:
        x = np.random.default_rng([711, n, c]).integers(0, 256, (S, n)).astype(np.uint8)
        for s, v in zip((1, 2, 7, 8), (0x00, 0xFF, 0x7F, 0x55)):
            x[s] = v
    x.setflags(write=False)
    return x


def rows_at(o0, n_out=N_OUT, cls=None, src=None):
    """the rows of one message: outputs [o0, o0 + n_out) of every stream's recording; cls / src override class and source stream"""
    cls = CLS if cls is None else cls
    arrs = []
    for s in range(S):
        rate, _ = CLASSES[int(cls[s])]
        a, n = R.class_n_in(rate, o0) if o0 else 0, R.class_n_in(rate, n_out)
        arrs.append(whole(int(cls[s]))[s if src is None else src[s]][a:a + n])
    return R.pack_ingest_rows(arrs, cls, CLASSES, n_out)


def fresh(e, cls=None):
    """classes configured, every stream in its class, every history zero (and every other bit of stream state reset)"""
    e.reset()
    e.configure_ingest_classes(CLASSES)
    e.assign_ingest(np.arange(S), CLS if cls is None else cls)


_cache = {}


def mixed_six(eng):
    if "six" not in _cache:
        fresh(eng)
        got = np.concatenate([eng.ingest_mixed(rows_at(N_OUT * k)) for k in range(N_MSG)], axis=1)
        got.setflags(write=False)
        _cache["six"] = got
    return _cache["six"]


def single_six(single, c):
    """the parent's kernel: a single-format handle fed whole(c) in six messages -> int16 [S, 7680]"""
    if ("single", c) not in _cache:
        rate, enc = CLASSES[c]
        single.configure_ingest(rate, enc)
        n = R.class_n_in(rate, N_OUT)
        got = np.concatenate([single.ingest(np.ascontiguousarray(whole(c)[:, n * k:n * (k + 1)])) for k in range(N_MSG)], axis=1)
        got.setflags(write=False)
        _cache[("single", c)] = got
    return _cache[("single", c)]


# ---- 1. bit equality with the parent's kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(len(CLASSES)))
def test_every_class_equals_the_single_format_kernel_bit_for_bit(eng, single, c):
    got, want = mixed_six(eng), single_six(single, c)
    assert got.shape == want.shape == (S, TOTAL) and got.dtype == np.int16
    mine = np.flatnonzero(CLS == c)
    bad = np.argwhere(got[mine] != want[mine])
    assert not len(bad), f"class {CLASSES[c]}: {len(bad)} outputs differ from ingest_kernel, first at stream {mine[bad[0][0]]}, output {bad[0][1]}"
    assert (got[mine] != 0).any()


# ---- 2. the budget ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(len(CLASSES)))
def test_six_messages_hold_the_budget_of_the_whole_recording(eng, c):
    rate, enc = CLASSES[c]
    mine = np.flatnonzero(CLS == c)
    got = mixed_six(eng)[mine]
    dec = R.decode(whole(c), enc)[mine]
    if rate == 16000:
        assert (got == dec).all()
        return
    p, q, taps = R.design(rate)
    pre = np.concatenate([np.zeros((len(mine), taps.shape[1] // 2), np.int16), dec], axis=1)
    y, A = RR.ref64(pre, p, q, taps)
    y, A = y[:, :TOTAL], A[:, :TOTAL]
    over = RR.excess(got, y, A, taps.shape[1])
    print(f"{rate} Hz {enc}: worst (err - 0.5)+ / (gamma*A) = {RR.worst_ratio(got, y, A, taps.shape[1]):.3f}, max excess {over.max():.3f}")
    assert (over <= 0).all(), f"{int((over > 0).sum())} outputs outside 0.5 + gamma*A, worst by {over.max():.3f} LSB"


# ---- 3. cuts -----------------------------------------------------------------------------------------------------------------------------
def test_one_message_equals_six_equals_twelve(eng):
    six = mixed_six(eng)
    for rate, _ in CLASSES:
        assert R.class_n_in(rate, 640) * 16000 == 640 * rate                 # 640 outputs are a whole message in every class
    fresh(eng)
    one = eng.ingest_mixed(rows_at(0, TOTAL), n_out=TOTAL)
    assert (one == six).all(), "one message of 7680 outputs differs from six of 1280"
    fresh(eng)
    twelve = np.concatenate([eng.ingest_mixed(rows_at(640 * k, 640), n_out=640) for k in range(12)], axis=1)
    bad = np.argwhere(twelve != six)
    assert not len(bad), f"messages of 640 outputs: {len(bad)} outputs differ, first at {bad[0]}"


# ---- 4. masks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_on", ["host", "device"])
def test_masked_streams_keep_history_output_row_and_record(eng, mask_on):
    import torch
    six = mixed_six(eng)
    fresh(eng)
    served = np.zeros(S, int)
    rb = eng.ingest_row_bytes()
    msgs = [rows_at(N_OUT * k) for k in range(4)]
    for t in range(6):
        on = (np.arange(S) % 3 != t % 3).astype(np.uint8) if t < 5 else np.ones(S, np.uint8)
        rows = np.stack([msgs[min(served[s], 3)][s] for s in range(S)])
        before = eng.export_state(np.arange(S))
        out = np.full((S, N_OUT), 12345, np.int16)
        if mask_on == "host":
            rc = _lib().oww_ingest_mixed(eng._h, _vp(rows), 0, rb, N_OUT, _vp(on), 0, _vp(out), 0)
        else:
            d_on = torch.from_numpy(on).cuda()
            torch.cuda.synchronize()
            rc = _lib().oww_ingest_mixed(eng._h, _vp(rows), 0, rb, N_OUT, _vp(d_on.data_ptr()), 1, _vp(out), 0)
        assert rc == 0, _err()
        after = eng.export_state(np.arange(S))
        for s in range(S):
            if on[s]:
                k = min(served[s], 3)
                if served[s] < 4:
                    assert (out[s] == six[s, N_OUT * k:N_OUT * (k + 1)]).all(), f"step {t}, stream {s}: message {k} differs from the consecutive run"
            else:
                assert (out[s] == 12345).all(), f"step {t}: the output row of stream {s}, which sat out, was written"
                assert (after[s] == before[s]).all(), f"step {t}: the state record of stream {s}, which sat out, changed"
        assert (after[13] != before[13]).any() == bool(on[13])               # (random mu-law codes: its history does move when served)
        served += on
    assert served.min() >= 4


# ---- 5. state ----------------------------------------------------------------------------------------------------------------------------
def test_assign_reset_move_export_import(eng, single):
    six = mixed_six(eng)
    ulaw_first = single_six(single, 1)[:, :N_OUT]
    fresh(eng)
    for k in range(3):
        eng.ingest_mixed(rows_at(N_OUT * k))
    # move and export / import carry history AND class: 4 (44.1 kHz) -> slot 20 (A-law until now), 3 (11.025 kHz) -> the other handle's 9
    fresh(single)
    rec = eng.export_state([3])
    eng.move_streams([4], [20])
    single.import_state([9], rec)
    src = np.arange(S)
    src[20] = 4
    cls = CLS.copy()
    cls[20] = CLS[4]
    src9 = np.arange(S)
    src9[9] = 3
    cls9 = CLS.copy()
    cls9[9] = CLS[3]
    for k in range(3, 6):
        out = eng.ingest_mixed(rows_at(N_OUT * k, cls=cls, src=src))
        home = six[:, N_OUT * k:N_OUT * (k + 1)]
        assert (out[4] == home[4]).all() and (out[20] == home[4]).all(), f"message {k}: the moved stream differs from the stay-at-home run"
        assert (out[6] == home[6]).all()
        out9 = single.ingest_mixed(rows_at(N_OUT * k, cls=cls9, src=src9))
        assert (out9[9] == home[3]).all(), f"message {k}: the imported stream differs from the stay-at-home run"
    # another table: the record is refused
    other = list(CLASSES)
    other[1], other[2] = other[2], other[1]
    single.configure_ingest_classes(other)
    assert single.state_info()[0] == eng.state_info()[0] and single.state_info()[1] != eng.state_info()[1]
    with pytest.raises(Exception, match="fingerprint"):
        single.import_state([9], rec)
    # assign: exactly the listed streams start from silence in their new class (5: 48 kHz -> mu-law; 13: mu-law -> mu-law)
    before = eng.export_state(np.arange(S))
    eng.assign_ingest([5, 13], [1, 1])
    after = eng.export_state(np.arange(S))
    changed = np.flatnonzero((before != after).any(axis=1))
    assert set(changed) == {5, 13}, f"assign touched the records of streams {changed}"
    cls = CLS.copy()
    cls[20], cls[5] = CLS[4], 1
    out = eng.ingest_mixed(rows_at(0, cls=cls))
    assert (out[5] == ulaw_first[5]).all(), "an assigned stream does not start from silence in its new class"
    assert (out[13] == ulaw_first[13]).all() and (out[13] != 0).any(), "re-assigning a stream's own class does not zero its history"
    assert (out[10] != six[10, :N_OUT]).any()                                # a neighbour's history (44.1 kHz noise) was left alone
    # reset: history zero, class kept
    eng.reset([5, 6])
    out = eng.ingest_mixed(rows_at(0, cls=cls))
    assert (out[5] == ulaw_first[5]).all(), "a reset stream lost its class or kept its history"
    assert (out[6] == six[6, :N_OUT]).all()
    assert (out[10] != six[10, :N_OUT]).any()


def test_record_and_fingerprint_of_other_handles_are_what_they_were():
    a, b = _new_engine(4, calibration_pcm=None), _new_engine(4, calibration_pcm=None)
    try:
        base = a.state_info()
        assert b.state_info() == base
        b.configure_ingest_classes(CLASSES)
        nb, fp = b.state_info()
        assert nb == base[0] + HPAD_MAX * 2 + 16 and fp != base[1]           # Hpad_max int16 samples and one 16-byte piece with the class
        b.configure_ingest_classes(CLASSES[:5])
        assert b.state_info()[1] not in (base[1], fp)
        assert a.state_info() == base
        a.configure_ingest(8000, "ulaw")
        b.configure_ingest(8000, "ulaw")                                     # the single form after classes: as if they had never been
        assert a.state_info() == b.state_info() and a.state_info()[0] == base[0] + 32 * 2
        b.configure_ingest_classes([(8000, "ulaw")])                         # one class is not the single form
        assert b.state_info()[0] == a.state_info()[0] + 16 and b.state_info()[1] != a.state_info()[1]
    finally:
        a.close(); b.close()


# ---- 6. the step behind it ---------------------------------------------------------------------------------------------------------------
def _step_rows(codes, k):
    """message k with the mu-law streams fed `codes` instead of their random codes"""
    rows = rows_at(N_OUT * k)
    for s in np.flatnonzero(CLS == 1):
        rows[s, :640] = codes[s, 640 * k:640 * (k + 1)]
    return rows


def test_step_ingest_mixed_end_to_end(eng, single):
    """As tests/test_ingest_gpu.py::test_predict_ingest_end_to_end: 8 kHz mu-law, delay 13 * 2 = 26 whole output samples, 16 samples of
    silence in front so that the 1e-4 measures the paths alone."""
    p, q, taps = R.design(8000)
    delay = taps.shape[1] // 2 * q // p
    assert delay == 26
    rng = np.random.default_rng(8)
    pcm = np.clip(rng.standard_normal((S, 640 * N_MSG)) * 3000, -32000, 32000)
    table = R.decode_ulaw(np.arange(256, dtype=np.uint8)).astype(np.float64)
    codes = np.stack([np.abs(row[:, None] - table[None, :]).argmin(-1) for row in pcm]).astype(np.uint8)
    codes[:, :16] = 0xFF
    fresh(eng)
    fused = [eng.step_ingest_mixed(_step_rows(codes, k)).copy() for k in range(N_MSG)]
    fresh(eng)
    for k in range(N_MSG):
        x = eng.ingest_mixed(_step_rows(codes, k))
        twin = eng.step(x)
        assert (fused[k] == twin).all(), f"step {k}: step_ingest_mixed differs from ingest_mixed + step"
    assert eng.ingest_dev_ptr() != 0 and eng.ingest_dev_ptr() % 16 == 0
    single.reset()
    x16 = single.resample(R.decode_ulaw(codes), 8000)
    delayed = np.concatenate([np.zeros((S, delay), np.int16), x16], axis=1)[:, :TOTAL]
    ulaw = np.flatnonzero(CLS == 1)
    worst = 0.0
    for k in range(N_MSG):
        want = single.step(np.ascontiguousarray(delayed[:, N_OUT * k:N_OUT * (k + 1)]))
        worst = max(worst, float(np.abs(fused[k][ulaw] - want[ulaw]).max()))
    print(f"max |step_ingest_mixed - step(one-piece conversion, delayed {delay})| over the mu-law streams = {worst:.3e}")
    assert worst <= 1e-4
    assert (fused[-1][ulaw] != 0).any()                                      # (the sixth frame is the first the engine does not report as zero)


# ---- 7. pipelined --------------------------------------------------------------------------------------------------------------------------
N_ROUNDS = 10        # six and four more: the engine reports zeros for a stream's first five frames, so six rounds alone would compare few real scores


def _masks():
    m = [(np.arange(S) % 4 != t % 4).astype(np.uint8) for t in range(N_ROUNDS)]
    m[2] = None                                                             # NULL: every stream
    m[4] = (np.arange(S) < 3).astype(np.uint8)                               # few participants: the group lists
    return m


def _pipeline_against_sync(e, with_events=False):
    """The six messages in turn over N_ROUNDS rounds (each stream's audio simply goes on with whatever message comes next).  A stream
    that has not taken part yet in a run repeats the score it had before the run (oww_reset leaves it), so rows are compared from a
    stream's first participation on."""
    rows, masks = [rows_at(N_OUT * (k % N_MSG)) for k in range(N_ROUNDS)], _masks()
    fresh(e)
    sync, sync_ev = [], []
    for k in range(N_ROUNDS):
        sync.append(e.step_ingest_mixed(rows[k], stream_on=masks[k]).copy())
        if with_events:
            sync_ev.append(e.events())
    fresh(e)
    got, got_ev = [], []

    def collect():
        got.append(e.collect().copy())
        if with_events:
            got_ev.append(e.events())

    e.submit_ingest_mixed(rows[0], masks[0])
    for k in range(1, N_ROUNDS):
        e.submit_ingest_mixed(rows[k], masks[k])
        if k == 2:                                                           # two in flight: a third is refused and moves nothing
            rc = _lib().oww_submit_ingest_mixed(e._h, _vp(rows[k]), rows[k].shape[1], None)
            assert rc == OWW_ESTATE and "in flight" in _err(), (rc, _err())
        collect()
    collect()
    seen = np.zeros(S, bool)
    for k in range(N_ROUNDS):
        seen |= np.ones(S, bool) if masks[k] is None else masks[k].astype(bool)
        assert (got[k][seen] == sync[k][seen]).all(), f"round {k}: the pipelined scores differ from step_ingest_mixed"
        if with_events:
            assert got_ev[k][1] == sync_ev[k][1] and len(got_ev[k][0]) == len(sync_ev[k][0]), f"round {k}: event counts differ"
            assert (got_ev[k][0] == sync_ev[k][0]).all(), f"round {k}: event records differ"
    return sync, sync_ev


def test_submit_collect_equals_the_synchronous_run(eng):
    sync, _ = _pipeline_against_sync(eng)
    assert np.isfinite(sync[-1]).all() and (sync[-1] != 0).any(), "no score left the first-frames zeroing: the comparison showed nothing"


def test_submit_collect_with_graph(eng):
    eng.use_graph(True)
    try:
        _pipeline_against_sync(eng)
    finally:
        eng.use_graph(False)


def test_submit_collect_with_events():
    e = _new_engine(event_capacity=64)
    try:
        e.set_event_thresholds([0.0] * e.n_labels)
        _, ev = _pipeline_against_sync(e, with_events=True)
        assert max(n for _, n in ev) > 0, "no event was reported: the comparison showed nothing"
    finally:
        e.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_nothing(eng, single):
    from openwakeword_amd import _lib as L
    lib = _lib()
    six = mixed_six(eng)
    fresh(eng)
    eng.ingest_mixed(rows_at(0))
    before = eng.export_state(np.arange(S))
    rb = eng.ingest_row_bytes()
    rows = rows_at(N_OUT)
    out = np.empty((S, N_OUT), np.int16)
    scores = np.empty((S, eng.n_labels), np.float32)
    ids, on = np.array([3], np.int32), np.ones(S, np.uint8)

    def refused(rc, code, *words):
        msg = _err()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    refused(lib.oww_ingest_assign(eng._h, _vp(ids), 1, _vp(np.array([6], np.uint8))), OWW_EINVAL, "unknown class 6")
    refused(lib.oww_ingest_assign(eng._h, _vp(np.array([3, S], np.int32)), 2, _vp(np.array([1, 1], np.uint8))), OWW_EINVAL, f"stream id {S}")
    p, q, taps = R.design(8000)
    arr = (L.IngestClass * 17)(*[L.IngestClass(1, p, q, taps.shape[1], taps.ctypes.data) for _ in range(17)])
    refused(lib.oww_ingest_configure_classes(eng._h, 17, arr), OWW_EINVAL, "n_classes=17")
    refused(lib.oww_ingest_configure_classes(eng._h, 0, arr), OWW_EINVAL, "n_classes=0")
    arr[1].n_taps = 25
    refused(lib.oww_ingest_configure_classes(eng._h, 2, arr), OWW_EINVAL, "class 1", "n_taps=25")
    for entry in ("ingest", "step"):
        def call(r, pitch, n_out, mask=None):
            if entry == "ingest":
                return lib.oww_ingest_mixed(eng._h, _vp(r), 0, pitch, n_out, _vp(mask), 0, _vp(out), 0)
            return lib.oww_step_ingest_mixed(eng._h, _vp(r), 0, pitch, n_out, _vp(mask), 0, _vp(scores), 0)
        refused(call(rows, rb - 8, N_OUT), OWW_EINVAL, "multiple of 16")
        refused(call(rows, rb - 16, N_OUT), OWW_EINVAL, "row_bytes", str(rb))
        refused(call(rows, rb, 100), OWW_EINVAL, "class 3", "640")             # 100 * 441 is no multiple of 640
        refused(call(None, rb, N_OUT), OWW_EINVAL, "null argument: in")
        refused(call(rows, rb, 0), OWW_EINVAL, "n_out=0")
    big = np.zeros((S, 2 * rb), np.uint8)
    refused(lib.oww_step_ingest_mixed(eng._h, _vp(big), 0, 2 * rb, 2 * N_OUT, _vp(on), 0, _vp(scores), 0), OWW_EINVAL, "one chunk", "2560")
    refused(lib.oww_step_ingest_mixed(eng._h, _vp(rows), 0, rb, 640, None, 0, _vp(scores), 0), OWW_EINVAL, "640", "1280")
    huge = np.zeros((S, 16 * rb), np.uint8)
    refused(lib.oww_ingest_mixed(eng._h, _vp(huge), 0, 16 * rb, 16 * N_OUT, None, 0, None, 0), OWW_EINVAL, "LDS")
    refused(lib.oww_submit_ingest_mixed(eng._h, _vp(rows), rb - 16, None), OWW_EINVAL, "row_bytes")
    # the single-format entries on a handle with classes
    m = np.ascontiguousarray(whole(1)[:, :640])
    refused(lib.oww_ingest(eng._h, _vp(m), 0, 640, None, 0, _vp(out), 0), OWW_ESTATE, "ingest classes")
    refused(lib.oww_step_ingest(eng._h, _vp(m), 0, 640, None, 0, _vp(scores), 0), OWW_ESTATE, "ingest classes")
    assert (eng.export_state(np.arange(S)) == before).all(), "a refused call moved stream state"
    assert (eng.ingest_mixed(rows) == six[:, N_OUT:2 * N_OUT]).all()           # the next message continues the first
    # the mixed entries on a single-configured handle, and on one that configured nothing
    single.configure_ingest(8000, "ulaw")
    single.ingest(m)
    before = single.export_state(np.arange(S))
    refused(lib.oww_ingest_mixed(single._h, _vp(rows), 0, rb, N_OUT, None, 0, _vp(out), 0), OWW_ESTATE, "oww_ingest_configure")
    refused(lib.oww_step_ingest_mixed(single._h, _vp(rows), 0, rb, N_OUT, None, 0, _vp(scores), 0), OWW_ESTATE, "oww_ingest_configure")
    refused(lib.oww_submit_ingest_mixed(single._h, _vp(rows), rb, None), OWW_ESTATE, "oww_ingest_configure")
    refused(lib.oww_ingest_assign(single._h, _vp(ids), 1, _vp(np.array([0], np.uint8))), OWW_ESTATE, "oww_ingest_configure")
    assert (single.export_state(np.arange(S)) == before).all()
    bare = _new_engine(4, calibration_pcm=None)
    try:
        refused(lib.oww_ingest_mixed(bare._h, _vp(rows), 0, rb, N_OUT, None, 0, _vp(out), 0), OWW_ESTATE, "not configured")
        refused(lib.oww_ingest_assign(bare._h, _vp(ids), 1, _vp(np.array([0], np.uint8))), OWW_ESTATE, "not configured")
    finally:
        bare.close()


# ---- 9. a class whose bank stays in global memory ------------------------------------------------------------------------------------------
def test_a_class_with_a_bank_beyond_lds_equals_the_single_format_kernel(eng, single):
    """16001 Hz (q = 16000: a 1.8 MB bank, read from global memory) next to 8 kHz mu-law (its bank in LDS), streams alternating, two
    messages of 16000 outputs: the launch's LDS is the 16001 Hz class's need WITHOUT its bank (owwhip_ingest.h: class_geometry)."""
    classes, n_out, n_msg = [(16001, "pcm16"), (8000, "ulaw")], 16000, 2
    cls = (np.arange(S) % 2).astype(np.uint8)
    n_in = [R.class_n_in(rate, n_out) for rate, _ in classes]
    assert n_in == [16001, 8000] and R.class_row_bytes(classes, n_out) == 32016
    fed = [np.ascontiguousarray(RR.signals(16001, n_in[0] * n_msg)),
           np.random.default_rng([711, 16001]).integers(0, 256, (S, n_in[1] * n_msg)).astype(np.uint8)]
    try:
        eng.reset()
        eng.configure_ingest_classes(classes)
        eng.assign_ingest(np.arange(S), cls)
        got = []
        for k in range(n_msg):
            arrs = [fed[cls[s]][s, n_in[cls[s]] * k:n_in[cls[s]] * (k + 1)] for s in range(S)]
            got.append(eng.ingest_mixed(R.pack_ingest_rows(arrs, cls, classes, n_out), n_out=n_out))
        got = np.concatenate(got, axis=1)
        for c, (rate, enc) in enumerate(classes):
            single.configure_ingest(rate, enc)
            want = np.concatenate([single.ingest(np.ascontiguousarray(fed[c][:, n_in[c] * k:n_in[c] * (k + 1)])) for k in range(n_msg)], axis=1)
            mine = np.flatnonzero(cls == c)
            bad = np.argwhere(got[mine] != want[mine])
            assert not len(bad), f"class {classes[c]}: {len(bad)} outputs differ from ingest_kernel, first at stream {mine[bad[0][0]]}, output {bad[0][1]}"
            assert (got[mine][:, n_out:] != 0).any()
    finally:
        fresh(eng)
