"""The stateful stream ingest on the device (`ingest_kernel` / oww_ingest / oww_step_ingest): G.711 and PCM16 decode and CONTINUOUS rate
conversion, against the float64 definition (tests/resample_ref.py) on the whole recording behind n_taps / 2 zeros, against the
stateless kernel on the same prefixed recording (bit for bit), across message cuts, masks, state records and the step behind it.
Two tolerances only: the derived `0.5 + gamma * A` per output sample (RR.excess <= 0) and bit equality; the end-to-end test adds the
project's by-path score tolerance 1e-4."""
import ctypes as C
import functools

import numpy as np
import pytest

import resample_ref as RR
from openwakeword_amd import resample as R
from openwakeword_amd import weights as W

pytestmark = pytest.mark.gpu
S = RR.ROWS
FRAME = {8000: 640, 44100: 3528, 48000: 3840}                               # one 80 ms message = 1280 samples at 16 kHz
N_MSG = 6
CONFIGS = [(8000, "ulaw"), (8000, "alaw"), (44100, "pcm16"), (48000, "pcm16")]
OWW_EINVAL, OWW_ESTATE = -1, -3


def _new_engine(n_streams=S, **kw):
    from openwakeword_amd.engine import StreamEngine
    return StreamEngine(n_streams, {"alexa": W.synthetic_head("alexa", seed=1)}, W.synthetic_embedding(seed=3), **kw)


@pytest.fixture(scope="module")
def eng():
    e = _new_engine()
    yield e
    e.close()


def _vp(a):
    return None if a is None else (C.c_void_p(int(a)) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p))


def _lib():
    from openwakeword_amd import _lib as L
    return L.load()


def _raw_ingest(h, data, n_in, on=None, out=None, in_dev=0, on_dev=0, out_dev=0):
    """oww_ingest as the header declares it -> (return code, message)."""
    rc = _lib().oww_ingest(h, _vp(data), in_dev, n_in, _vp(on), on_dev, _vp(out), out_dev)
    return rc, _lib().oww_last_error().decode(errors="replace")


def _raw_step_ingest(h, data, n_in, on=None, scores=None):
    rc = _lib().oww_step_ingest(h, _vp(data), 0, n_in, _vp(on), 0, _vp(scores), 0)
    return rc, _lib().oww_last_error().decode(errors="replace")


def _raw_configure(h, enc, p, q, taps, n_taps):
    rc = _lib().oww_ingest_configure(h, enc, p, q, _vp(taps), n_taps)
    return rc, _lib().oww_last_error().decode(errors="replace")


@functools.lru_cache(maxsize=None)
def codes_for(n, seed=0):
    """uint8 [S, n]: rows 0..3 the constant codes 0x00, 0xFF, 0x7F, 0x55, every other row uniform random codes."""
    c = np.random.default_rng([711, n, seed]).integers(0, 256, (S, n)).astype(np.uint8)
    for r, v in enumerate((0x00, 0xFF, 0x7F, 0x55)):
        c[r] = v
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def recording(rate, enc):
    """(what is fed, its decoded int16) for N_MSG messages of one configuration, read-only."""
    n = FRAME[rate] * N_MSG
    fed = RR.signals(rate, n) if enc == "pcm16" else codes_for(n)
    dec = R.decode(fed, enc)
    dec.setflags(write=False)
    return fed, dec


@functools.lru_cache(maxsize=None)
def reference(rate, enc):
    """(prefixed recording, y64, A) of the definition: ref64 on zeros(half) | decoded whole, cut to the outputs the stream has produced."""
    p, q, taps = R.design(rate)
    fed, dec = recording(rate, enc)
    pre = np.concatenate([np.zeros((S, taps.shape[1] // 2), np.int16), dec], axis=1)
    y, A = RR.ref64(pre, p, q, taps)
    n = dec.shape[1] * q // p
    y, A = y[:, :n], A[:, :n]
    for a in (pre, y, A):
        a.setflags(write=False)
    return pre, y, A


def _feed(eng, fed, sizes):
    """the recording message after message (sizes in turn) -> int16 [S, n_out]"""
    outs, at, i = [], 0, 0
    while at < fed.shape[1]:
        n = sizes[i % len(sizes)]
        outs.append(eng.ingest(np.ascontiguousarray(fed[:, at:at + n])))
        at += n
        i += 1
    return np.concatenate(outs, axis=1)


_six = {}


def six_messages(eng, rate, enc):
    """the device's output for the six 80 ms messages, computed once per configuration"""
    if (rate, enc) not in _six:
        eng.configure_ingest(rate, enc)
        got = _feed(eng, recording(rate, enc)[0], [FRAME[rate]])
        got.setflags(write=False)
        _six[(rate, enc)] = got
    return _six[(rate, enc)]


# ---- 1. the budget -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,enc", CONFIGS)
def test_six_messages_hold_the_budget_of_the_whole_recording(eng, rate, enc):
    n_taps = R.design(rate)[2].shape[1]
    got = six_messages(eng, rate, enc)
    _, y, A = reference(rate, enc)
    assert got.dtype == np.int16 and got.shape == y.shape == (S, 1280 * N_MSG)
    over = RR.excess(got, y, A, n_taps)
    print(f"{rate} Hz {enc}: worst (err - 0.5)+ / (gamma*A) = {RR.worst_ratio(got, y, A, n_taps):.3f}, "
          f"{int((got != np.clip(np.rint(y), -32768, 32767)).sum())} of {y.size} outputs differ from rint(y64), max excess {over.max():.3f}")
    assert (over <= 0).all(), f"{int((over > 0).sum())} outputs outside 0.5 + gamma*A, worst by {over.max():.3f} LSB at " \
                              f"{np.unravel_index(np.argmax(over), over.shape)}"
    if enc != "pcm16":
        dc = {"ulaw": (-32124, 0, 0, -716), "alaw": (-5504, 848, -848, -8)}[enc]
        for r, v in enumerate(dc):                                             # constant codes: unit DC gain once the filter is full
            assert np.abs(got[r, 64:].astype(int) - v).max() <= 1, f"row {r} (constant code) is not the DC value {v}"


# ---- 2. the parent's kernel on the prefixed recording --------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,enc", CONFIGS)
def test_six_messages_equal_the_stateless_kernel_on_the_prefixed_recording(eng, rate, enc):
    got = six_messages(eng, rate, enc)
    pre, _, _ = reference(rate, enc)
    want = eng.resample(np.ascontiguousarray(pre), rate)[:, :got.shape[1]]
    bad = np.argwhere(got != want)
    assert not len(bad), f"{rate} Hz {enc}: {len(bad)} outputs differ from oww_resample(zeros(half) | whole), first at {bad[0]}"


# ---- 3. how the recording is cut changes nothing --------------------------------------------------------------------------------------
def test_chunking_invariance_bit_for_bit(eng):
    rate, enc = 8000, "ulaw"
    fed, _ = recording(rate, enc)
    assert fed.shape == (S, 3840)
    six = six_messages(eng, rate, enc)
    eng.configure_ingest(rate, enc)                                          # (zeroes every history)
    one = _feed(eng, fed, [3840])
    assert (one == six).all(), "one message of 3840 differs from six of 640"
    eng.configure_ingest(rate, enc)
    assert (_feed(eng, fed, [160]) == six).all(), "24 messages of 160 differ from six of 640"
    n_taps = R.design(rate)[2].shape[1]
    for n in (2, 8, 24):                                                     # n_in < n_taps - 1: old history samples move down
        assert n < n_taps - 1
        eng.configure_ingest(rate, enc)
        got = _feed(eng, fed[:, :240], [n])
        bad = np.argwhere(got != six[:, :480])
        assert not len(bad), f"messages of {n} samples: {len(bad)} outputs differ, first at {bad[0]}"
    eng.configure_ingest(rate, enc)                                          # and sizes in turn, the last stream (37: no full group) included
    mixed = _feed(eng, fed[:, :3 * (2 + 640 + 8 + 24 + 160)], [2, 640, 8, 24, 160])
    assert (mixed == six[:, :mixed.shape[1]]).all() and (mixed[S - 1] != 0).any()


# ---- 4. decode only --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["ulaw", "alaw"])
def test_decode_only_equals_the_table(eng, enc):
    table = (R.decode_ulaw if enc == "ulaw" else R.decode_alaw)(np.arange(256, dtype=np.uint8))
    eng.configure_ingest(16000, enc)
    for n in (1280, 2560, 37, 256):                                          # 16 codes per lane, and rows that start on odd addresses
        c = np.ascontiguousarray(codes_for(2560, seed=1)[:, :n])
        if n == 256:
            c[4] = np.arange(256, dtype=np.uint8)                            # every code once
        got = eng.ingest(c)
        assert got.shape == (S, n) and (got == table[c]).all(), f"{enc}, {n} codes"
    eng.configure_ingest(16000, "pcm16")
    x = np.ascontiguousarray(RR.signals(16000, 1280))
    assert (eng.ingest(x) == x).all()


# ---- 5. masks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_on", ["host", "device"])
def test_masked_streams_keep_history_and_output_row(eng, mask_on):
    """Even streams are served in steps 0, 2, 3, 5, odd streams in 1, 2, 4, 5; each gets its own k-th message the k-th time it is served."""
    import torch
    rate, enc, n = 8000, "ulaw", 640
    fed, _ = recording(rate, enc)
    msgs = [np.ascontiguousarray(fed[:, n * k:n * (k + 1)]) for k in range(4)]
    eng.configure_ingest(rate, enc)
    want = [eng.ingest(m) for m in msgs]                                     # four consecutive steps
    eng.configure_ingest(rate, enc)
    even = (np.arange(S) % 2 == 0)
    served = np.zeros(S, int)
    for t in range(6):
        on = (even if t in (0, 3) else ~even if t in (1, 4) else np.ones(S, bool)).astype(np.uint8)
        data = np.stack([msgs[min(served[s], 3)][s] for s in range(S)])
        before = eng.export_state(np.arange(S))
        out = np.full((S, 1280), 12345, np.int16)
        if mask_on == "host":
            rc, msg = _raw_ingest(eng._h, data, n, on, out)
        else:
            d_on = torch.from_numpy(on).cuda()
            torch.cuda.synchronize()
            rc, msg = _raw_ingest(eng._h, data, n, d_on.data_ptr(), out, on_dev=1)
        assert rc == 0, msg
        after = eng.export_state(np.arange(S))
        for s in range(S):
            if on[s]:
                assert (out[s] == want[served[s]][s]).all(), f"step {t}, stream {s}: message {served[s]} differs from the consecutive run"
            else:
                assert (out[s] == 12345).all(), f"step {t}: the output row of stream {s}, which sat out, was written"
                assert (after[s] == before[s]).all(), f"step {t}: the state record of stream {s}, which sat out, changed"
        assert (after[5] != before[5]).any() == bool(on[5])                  # (a random-code row: its history does move when served)
        served += on
    assert (served == 4).all()


# ---- 6. state ----------------------------------------------------------------------------------------------------------------------------
def test_history_travels_with_move_export_import_and_reset(eng):
    rate, enc, n = 8000, "ulaw", 640
    fed, _ = recording(rate, enc)
    six = six_messages(eng, rate, enc)
    eng.configure_ingest(rate, enc)
    for k in range(3):
        eng.ingest(np.ascontiguousarray(fed[:, n * k:n * (k + 1)]))
    rec = eng.export_state([5])
    eng.move_streams([5], [20])
    eng.import_state([9], rec)
    for k in range(3, 6):
        m = fed[:, n * k:n * (k + 1)].copy()
        m[20] = m[5]
        m[9] = m[5]
        out = eng.ingest(m)
        home = six[5, 1280 * k:1280 * (k + 1)]
        assert (out[5] == home).all() and (out[20] == home).all(), f"message {k}: the moved stream differs from the stay-at-home run"
        assert (out[9] == home).all(), f"message {k}: the imported stream differs from the stay-at-home run"
        assert (out[6] == six[6, 1280 * k:1280 * (k + 1)]).all()
    eng.reset([5])
    m = np.ascontiguousarray(fed[:, :n])
    out = eng.ingest(m)
    assert (out[5] == six[5, :1280]).all(), "a reset stream does not start from silence"
    assert (out[6] != six[6, :1280]).any()                                   # its neighbour's history was left alone
    eng.reset()
    assert (eng.ingest(m) == six[:, :1280]).all()


def test_record_and_fingerprint_without_ingest_are_what_they_were():
    a, b = _new_engine(4, calibration_pcm=None), _new_engine(4, calibration_pcm=None)
    try:
        base = a.state_info()
        assert b.state_info() == base                                        # taken before any ingest call exists on b
        H = R.design(8000)[2].shape[1] - 1
        b.configure_ingest(8000, "ulaw")
        nb, fp_u = b.state_info()
        assert nb == base[0] + (H + 7) // 8 * 8 * 2 and fp_u != base[1]     # one more section: Hpad int16 samples
        b.configure_ingest(8000, "alaw")
        assert b.state_info()[0] == nb and b.state_info()[1] not in (base[1], fp_u)
        b.configure_ingest(16000, "ulaw")                                    # decode only: no history, but another configuration
        assert b.state_info()[0] == base[0] and b.state_info()[1] != base[1]
        assert a.state_info() == base
        rec = a.export_state([1])
        with pytest.raises(Exception):
            b.import_state([1], rec)
    finally:
        a.close(); b.close()


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------
def test_predict_ingest_end_to_end():
    """8 kHz mu-law: the delay half * q / p = 13 * 2 = 26 output samples is whole.  The recording starts with 16 samples of silence
    (code 0xFF), so the one definitional difference between the two forms -- the continuous filter's first 26 outputs see the first 13
    input samples, the delayed one-piece conversion has zeros there -- vanishes and the 1e-4 measures the paths alone."""
    from openwakeword_amd.model import BatchedModel
    rate, n, steps, B = 8000, 640, 8, 6
    p, q, taps = R.design(rate)
    half = taps.shape[1] // 2
    assert (half * q) % p == 0
    delay = half * q // p
    rng = np.random.default_rng(8)
    pcm = np.clip(rng.standard_normal((B, n * steps)) * 3000, -32000, 32000)
    # mu-law codes of that noise: the nearest code by table search (an encoder is not what is under test)
    table = R.decode_ulaw(np.arange(256, dtype=np.uint8)).astype(np.float64)
    codes = np.stack([np.abs(row[:, None] - table[None, :]).argmin(-1) for row in pcm]).astype(np.uint8)
    codes[:, :16] = 0xFF
    wts = {"heads": {"alexa": W.synthetic_head("alexa", seed=1)}, "embedding": W.synthetic_embedding(seed=3)}
    a, b, c = (BatchedModel(B, ["alexa"], weights=wts) for _ in range(3))
    try:
        a.configure_ingest(rate, "ulaw")
        b.configure_ingest(rate, "ulaw")
        assert a.engine.ingest_dev_ptr() != 0 and a.engine.ingest_dev_ptr() % 16 == 0
        whole = R.decode_ulaw(codes)
        x16 = c.engine.resample(whole, rate)
        delayed = np.concatenate([np.zeros((B, delay), np.int16), x16], axis=1)[:, :1280 * steps]
        worst = 0.0
        for t in range(steps):
            m = np.ascontiguousarray(codes[:, n * t:n * (t + 1)])
            got = a.predict_ingest(m)
            x = b.engine.ingest(m)
            twin = b.engine.step(x)[:, b._keep]
            assert got.shape == (B, 1) and (got == twin).all(), f"step {t}: predict_ingest differs from ingest + step"
            want = c.predict_batch(np.ascontiguousarray(delayed[:, 1280 * t:1280 * (t + 1)]))
            worst = max(worst, float(np.abs(got - want).max()))
        print(f"max |predict_ingest - predict_batch(one-piece conversion, delayed {delay})| over {steps} steps = {worst:.3e}")
        assert worst <= 1e-4
        assert a.engine.ingest_dev_ptr() % 16 == 0
        on = np.arange(B) % 2 == 0                                          # the masked form rides on step_masked
        got = a.predict_ingest(np.ascontiguousarray(codes[:, :n]), on)
        twin = b.engine.step_masked(b.engine.ingest(np.ascontiguousarray(codes[:, :n]), on), on)[:, b._keep]
        assert (got == twin).all()
    finally:
        a.close(); b.close(); c.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_codes_and_leave_the_handle_usable(eng):
    from openwakeword_amd import _lib as L
    lib = _lib()
    fed, _ = recording(8000, "ulaw")
    m = np.ascontiguousarray(fed[:, :640])
    out = np.empty((S, 1280), np.int16)
    scores = np.empty((S, eng.n_labels), np.float32)
    # not configured
    fresh = _new_engine(4, calibration_pcm=None)
    try:
        for rc, msg in (_raw_ingest(fresh._h, m, 640, None, out), _raw_step_ingest(fresh._h, m, 640, None, scores)):
            assert rc == OWW_ESTATE and "not configured" in msg, (rc, msg)
        assert lib.oww_ingest_dev(fresh._h) is None
    finally:
        fresh.close()
    # configure before commit
    h = C.c_void_p()
    cfg = L.Config(0, 4, 1, 0, 3, 0, None)
    assert lib.oww_create(C.byref(cfg), C.byref(h)) == 0
    try:
        p, q, taps = R.design(8000)
        rc, msg = _raw_configure(h, 1, p, q, taps, taps.shape[1])
        assert rc == OWW_ESTATE and "oww_ingest_configure" in msg and "not committed" in msg, (rc, msg)
    finally:
        lib.oww_destroy(h)
    # unknown encoding, bad banks
    p, q, taps = R.design(8000)
    for enc, pp, qq, tp, nt, word in ((7, p, q, taps, 26, "encoding 7"), (-1, p, q, taps, 26, "encoding -1"), (1, p, q, taps, 25, "n_taps=25"),
                                      (1, p, q, None, 26, "null argument: taps"), (1, 2, 1, None, 0, "n_taps = 0"), (1, 0, q, taps, 26, "p=0")):
        eng.configure_ingest(8000, "ulaw")
        before = eng.ingest(m)
        rc, msg = _raw_configure(eng._h, enc, pp, qq, tp, nt)
        assert rc == OWW_EINVAL and "oww_ingest_configure" in msg and word in msg, (rc, msg)
    # messages
    eng.configure_ingest(44100, "pcm16")
    x = np.zeros((S, 3528), np.int16)
    rc, msg = _raw_ingest(eng._h, x, 100, None, out)
    assert rc == OWW_EINVAL and "100" in msg and "441" in msg, (rc, msg)                    # (n_in * q) % p != 0
    rc, msg = _raw_ingest(eng._h, x, 0, None, out)
    assert rc == OWW_EINVAL and "n_in=0" in msg, (rc, msg)
    eng.configure_ingest(8000, "ulaw")
    before = eng.ingest(m)
    rc, msg = _raw_ingest(eng._h, None, 640, None, out)
    assert rc == OWW_EINVAL and "null argument: in" in msg, (rc, msg)
    rc, msg = _raw_step_ingest(eng._h, None, 640, None, scores)
    assert rc == OWW_EINVAL and "null argument: in" in msg, (rc, msg)
    rc, msg = _raw_step_ingest(eng._h, m, 160, None, scores)                                # n_out = 320
    assert rc == OWW_EINVAL and "oww_step_ingest" in msg and "320" in msg and "1280" in msg, (rc, msg)
    rc, msg = _raw_step_ingest(eng._h, m, 1, None, scores)
    assert rc == OWW_EINVAL and "n_out" in msg, (rc, msg)
    rc, msg = _raw_step_ingest(eng._h, np.zeros((S, 1280), np.uint8), 1280, np.ones(S, np.uint8), scores)   # two chunks with a mask
    assert rc == OWW_EINVAL and "2560" in msg, (rc, msg)
    big = np.zeros((S, 30000), np.uint8)
    rc, msg = _raw_ingest(eng._h, big, 30000, None, None)
    assert rc == OWW_EINVAL and "30000" in msg and "LDS" in msg, (rc, msg)
    rc, msg = _raw_ingest(None, m, 640, None, out)
    assert rc < 0 and "oww_ingest" in msg
    # none of the refused calls moved a history: the next message continues the first
    eng2_first, eng2_second = before, eng.ingest(np.ascontiguousarray(fed[:, 640:1280]))
    six = six_messages(eng, 8000, "ulaw")
    assert (eng2_first == six[:, :1280]).all() and (eng2_second == six[:, 1280:2560]).all()
    assert np.isfinite(eng.step_ingest(m)).all()


# ---- 9. a bank that stays in global memory -----------------------------------------------------------------------------------------------
def test_a_bank_beyond_lds_equals_the_stateless_kernel_on_the_prefixed_recording(eng):
    """16001 Hz: p = 16001, q = 16000, a bank of 16000 x 28 floats (1.8 MB) that no workgroup holds, so `ingest_kernel` reads its taps
    from global memory -- the launch branch the host's LDS arithmetic (owwhip_ingest.h: single_check) decides.  Configured through the
    raw ABI; two messages, so that the second one starts from a history.  The contract of section 2: bit equality."""
    rate = n = 16001
    p, q, taps = R.design(rate)
    assert (p, q, taps.shape) == (16001, 16000, (16000, 26)) and q * 28 * 4 > 150 * 1024
    fed = RR.signals(rate, 2 * n)
    try:
        rc, msg = _raw_configure(eng._h, 0, p, q, taps, taps.shape[1])
        assert rc == 0, msg
        got = np.empty((S, 2 * q), np.int16)
        for k in range(2):
            out = np.empty((S, q), np.int16)
            rc, msg = _raw_ingest(eng._h, np.ascontiguousarray(fed[:, n * k:n * (k + 1)]), n, None, out)
            assert rc == 0, msg
            got[:, q * k:q * (k + 1)] = out
        pre = np.concatenate([np.zeros((S, taps.shape[1] // 2), np.int16), fed], axis=1)
        want = eng.resample(np.ascontiguousarray(pre), rate)[:, :got.shape[1]]
        bad = np.argwhere(got != want)
        assert not len(bad), f"{len(bad)} outputs differ from oww_resample(zeros(half) | whole), first at {bad[0]}"
        assert (got[:, q:] != 0).any()
    finally:
        eng.configure_ingest(8000, "ulaw")                                   # (the engine object knows its configuration again)
