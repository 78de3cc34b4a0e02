"""The device resampler (`resample_kernel` / `oww_resample`) at its launch and message edges, against the float64 definition
(tests/resample_ref.py).  Two tolerances only: the derived `0.5 + gamma * A` per output sample, and bit equality.  Every (geometry,
signal) case was admitted on the CPU by tests/test_resample_budget_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as RR
from openwakeword_amd import resample as R
from openwakeword_amd import weights as W

pytestmark = pytest.mark.gpu
S = RR.ROWS


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


def _raw(eng, x, n_in, p, q, taps, n_taps, out, n_out, in_dev=0, out_dev=0, handle="own"):
    """oww_resample as the header declares it -> (return code, message)."""
    from openwakeword_amd import _lib
    lib = _lib.load()
    rc = lib.oww_resample(eng._h if handle == "own" else handle, _vp(x), in_dev, n_in, p, q, _vp(taps), n_taps, _vp(out), out_dev, n_out)
    return rc, lib.oww_last_error().decode(errors="replace")


def _hold(got, y, A, n_taps, what):
    """THE assertion: every output within 0.5 + gamma * A of the clipped float64 value.  Returns the report line's figures."""
    over = RR.excess(got, y, A, n_taps)
    used = RR.worst_ratio(got, y, A, n_taps)
    differ = int((got != np.clip(np.rint(y), -32768, 32767)).sum())
    print(f"{what}: worst (err - 0.5)+ / (gamma*A) = {used:.3f}, {differ} of {y.size} outputs differ from rint(y64), "
          f"max |err| {np.abs(got - np.clip(y, -32768, 32767)).max():.3f}, gamma*A max {RR.gamma(n_taps) * A.max():.3f}")
    assert got.dtype == np.int16 and got.shape == y.shape
    assert (over <= 0).all(), f"{what}: {int((over > 0).sum())} outputs outside 0.5 + gamma*A, worst by {over.max():.3f} LSB at " \
                              f"{np.unravel_index(np.argmax(over), over.shape)}"
    return used, differ


# ---- 1. the budget over the case table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n_in", RR.CASES)
def test_budget_over_the_case_table(eng, rate, n_in):
    p, q, taps, x, y, A = RR.case_reference(rate, n_in)
    n_taps = taps.shape[1]
    g = RR.launch_geometry(n_in, p, q, n_taps)
    got = eng.resample(x, rate)
    _hold(got, y, A, n_taps, f"{rate} Hz n_in {n_in} (n_out {g['n_out']}, {n_taps} taps, opb {g['opb']} x {g['n_wg']} workgroups, "
                             f"taps in {'LDS' if g['taps_in_lds'] else 'global memory'})")
    sat, tie = RR.saturated(y), RR.near_tie(y, A, n_taps)
    assert sat.any() and tie.any()                                           # the clamp and the tie paths are known to be run
    ga = RR.gamma(n_taps) * A
    deep = (y > 32767.5 + ga) | (y < -32768.5 - ga)                          # beyond the range by more than the chain can err: clamped for certain
    assert deep.any() and (got[deep] == np.where(y[deep] > 0, 32767, -32768)).all()
    assert (got[0] == 0).all()                                               # the silence row


# ---- 2. exact indexing with delta banks ------------------------------------------------------------------------------------------
N_OUT_TARGETS = (1, 255, 256, 257, 1279, 1281, 2560, 3841)


@pytest.mark.parametrize("p,q,n_taps", [(7, 5, 10), (5, 7, 8), (1, 1, 2), (1, 1, 4096), (3, 1, 4096), (20011, 20000, 6)])
def test_delta_banks_index_exactly(eng, p, q, n_taps):
    """Phase row ph is a single 1.0 at tap k_ph (random per phase, 0 and n_taps - 1 included): the output is an input sample or 0,
    bit for bit, so an off-by-one in base, span, the phase or the row stride shows as a wrong integer.  n_in is the smallest
    message whose n_out = n_in * q / p is the target; 5/7 cannot produce 255 and runs 256 in its place."""
    rng = np.random.default_rng([p, q, n_taps])
    k_ph = rng.integers(0, n_taps, q)
    k_ph[0] = 0
    k_ph[q - 1] = n_taps - 1 if q > 1 else k_ph[0]
    banks = [k_ph]
    if q == 1:
        banks = [np.array([0]), np.array([n_taps - 1]), np.array([n_taps // 2 - 1])]
    for k_ph in banks:
        taps = np.zeros((q, n_taps), np.float32)
        taps[np.arange(q), k_ph] = 1.0
        for target in N_OUT_TARGETS:
            n_in = -(-target * p // q)
            n_out = n_in * q // p
            assert n_out == (256 if (p, q, target) == (5, 7, 255) else target)   # (7 n / 5 skips 255: the one target not met)
            x = rng.integers(1, 32768, (S, n_in)).astype(np.int16) * rng.choice(np.array([-1, 1], np.int16), (S, n_in))
            out = np.full((S, n_out), 12345, np.int16)
            rc, msg = _raw(eng, x, n_in, p, q, taps, n_taps, out, n_out)
            assert rc == 0, msg
            jp = np.arange(n_out, dtype=np.int64) * p
            src = jp // q + k_ph[jp % q] - n_taps // 2 + 1
            ok = (src >= 0) & (src < n_in)
            want = np.where(ok, x[:, np.where(ok, src, 0)], 0).astype(np.int16)
            bad = np.argwhere(got_ne := (out != want))
            assert not got_ne.any(), f"p/q {p}/{q} n_taps {n_taps} n_out {n_out}: {len(bad)} wrong, first at {bad[0]}: " \
                                     f"got {out[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
            g = RR.launch_geometry(n_in, p, q, n_taps)
            assert g["taps_in_lds"] == (0 if q == 20000 else 1)


# ---- 3. pointer forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n_in", [(11025, 1000), (16001, 1300)])
def test_pointer_forms_are_bit_identical(eng, rate, n_in):
    import torch
    p, q, taps, x, y, A = RR.case_reference(rate, n_in)
    n_taps, n_out = taps.shape[1], y.shape[1]
    x = x.copy()                                                            # (torch wants a writable array)
    host = np.empty((S, n_out), np.int16)
    rc, msg = _raw(eng, x, n_in, p, q, taps, n_taps, host, n_out)
    assert rc == 0, msg
    _hold(host, y, A, n_taps, f"{rate} Hz, host in / host out")
    d_in = torch.from_numpy(x).cuda()
    d_odd = torch.zeros(S * n_in + 3, dtype=torch.int16, device="cuda")        # the message starts one element into the buffer
    d_odd[1:1 + S * n_in] = d_in.reshape(-1)
    assert (d_odd.data_ptr() + 2) % 4 == 2
    torch.cuda.synchronize()
    # host in -> device out
    d_out = torch.full((S, n_out), -7, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rc, msg = _raw(eng, x, n_in, p, q, taps, n_taps, d_out.data_ptr(), n_out, 0, 1)
    assert rc == 0, msg
    eng.sync()
    assert (d_out.cpu().numpy() == host).all(), "host in / device out"
    # device in (aligned, then at an odd element offset) -> host out and device out
    for name, ptr in (("aligned", d_in.data_ptr()), ("odd offset", d_odd.data_ptr() + 2)):
        h2 = np.empty((S, n_out), np.int16)
        rc, msg = _raw(eng, ptr, n_in, p, q, taps, n_taps, h2, n_out, 1, 0)
        assert rc == 0, msg
        assert (h2 == host).all(), f"device in ({name}) / host out"
        d2 = torch.full((S, n_out), -7, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        rc, msg = _raw(eng, ptr, n_in, p, q, taps, n_taps, d2.data_ptr(), n_out, 1, 1)
        assert rc == 0, msg
        eng.sync()
        assert (d2.cpu().numpy() == host).all(), f"device in ({name}) / device out"


# ---- 4. one handle, many rates -------------------------------------------------------------------------------------------------
def test_one_handle_many_rates_between_live_steps():
    """48000, 8000, 16001 (the scratch grows, the bank leaves the LDS), 384000 (it grows again), 48000: every result inside the
    budget, the last equal to the first, and the scores of the steps in between those of a twin that never resamples."""
    a, b = _new_engine(), _new_engine()
    rng = np.random.default_rng(44)
    pcm = (rng.standard_normal((7, S, 1280)) * 4000).astype(np.int16)
    results = []
    try:
        assert (a.step(pcm[0]) == b.step(pcm[0])).all()
        for i, (rate, n_in) in enumerate([(48000, 11520), (8000, 640), (16001, 1300), (384000, 30720), (48000, 11520)]):
            p, q, taps, x, y, A = RR.case_reference(rate, n_in)
            got = a.resample(x, rate)
            _hold(got, y, A, taps.shape[1], f"call {i}: {rate} Hz")
            results.append(got)
            sa, sb = a.step(pcm[i + 1]), b.step(pcm[i + 1])
            assert np.isfinite(sa).all() and (sa == sb).all(), f"scores after the {rate} Hz call differ from the twin's"
        assert (results[4] == results[0]).all()
        assert (a.step(pcm[6]) == b.step(pcm[6])).all()
    finally:
        a.close(); b.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_the_handle_usable(eng):
    rate, n_in = 11025, 1000
    p, q, taps, x, y, A = RR.case_reference(rate, n_in)
    x = np.ascontiguousarray(x)
    n_taps, n_out = taps.shape[1], y.shape[1]
    before = eng.resample(x, rate)
    out = np.empty((S, max(n_out + 1, 1280)), np.int16)
    two = np.full((1, 2), 0.5, np.float32)
    x48 = np.zeros((S, 1), np.int16)
    # (arguments of oww_resample after the handle, word the message must contain)
    bad = [
        ("odd n_taps", (x, n_in, p, q, taps, n_taps - 1, out, n_out), "n_taps=25"),
        ("n_taps 0", (x, n_in, p, q, taps, 0, out, n_out), "n_taps=0"),
        ("n_taps 4098", (x, n_in, p, q, taps, 4098, out, n_out), "n_taps=4098"),
        ("q 65537", (x, n_in, p, 65537, taps, n_taps, out, n_out), "q=65537"),
        ("p 0", (x, n_in, 0, q, taps, n_taps, out, n_out), "p=0"),
        ("n_in 0", (x, 0, p, q, taps, n_taps, out, n_out), "n_in=0"),
        ("n_out + 1", (x, n_in, p, q, taps, n_taps, out, n_out + 1), "n_out"),
        ("n_out - 1", (x, n_in, p, q, taps, n_taps, out, n_out - 1), "n_out"),
        ("n_out 0", (x48, 1, 3, 1, R.design(48000)[2], R.design(48000)[2].shape[1], out, 0), "n_out"),
        ("null in", (None, n_in, p, q, taps, n_taps, out, n_out), "null argument: in"),
        ("null taps", (x, n_in, p, q, None, n_taps, out, n_out), "null argument: taps"),
        ("null out", (x, n_in, p, q, taps, n_taps, None, n_out), "null argument: out"),
        ("staging buffer", (np.zeros((S, 200), np.int16), 200, 200, 1, two, 2, out, 1), "p / q = 200 / 1"),
    ]
    assert n_taps == 26
    for name, args, word in bad:
        rc, msg = _raw(eng, *args)
        assert rc < 0, f"{name}: accepted"
        assert "oww_resample" in msg and word in msg, f"{name}: message {msg!r} does not name it ({word!r})"
        assert (eng.resample(x, rate) == before).all(), f"a valid call after the refusal of {name} gives other bits"
    rc, msg = _raw(eng, x, n_in, p, q, taps, n_taps, out, n_out, handle=None)
    assert rc < 0 and "oww_resample" in msg and "handle" in msg
    assert (eng.resample(x, rate) == before).all()
    _hold(before, y, A, n_taps, "11025 Hz around the refusals")


# ---- 6. stream counts ------------------------------------------------------------------------------------------------------------
def test_one_stream():
    e = _new_engine(1)
    try:
        for rate, n_in in ((11025, 1000), (15999, 2600), (384000, 30720)):
            p, q, taps, x, y, A = RR.case_reference(rate, n_in)
            for r in (3, 4, 7):                                                # alternation, uniform full scale, square wave
                got = e.resample(np.ascontiguousarray(x[r:r + 1]), rate)
                _hold(got, y[r:r + 1], A[r:r + 1], taps.shape[1], f"S = 1, {rate} Hz, row {r}")
    finally:
        e.close()


def test_65600_streams_put_the_stream_index_past_65535():
    """The launch keeps the stream count in the grid's second dimension; 65,600 is the first count used here that exceeds 65,535
    there.  Rows repeat a base of 61: the first 61 are held to the budget, every other row to its twin's bits."""
    n, rate, n_in, nb = 65600, 8000, 640, 61
    p, q, taps, base, y, A = RR.case_reference(rate, n_in, nb)
    x = np.ascontiguousarray(base[np.arange(n) % nb])
    e = _new_engine(n, calibration_pcm=None)
    try:
        got = e.resample(x, rate)
    finally:
        e.close()
    assert got.shape == (n, 1280)
    _hold(got[:nb], y, A, taps.shape[1], "S = 65,600 at 8000 Hz, rows 0..60")
    same = (got.reshape(-1, 1280) == got[np.arange(n) % nb]).all(axis=1)
    assert same.all(), f"{int((~same).sum())} rows differ from their twin, first {int(np.argmin(same))}"
    for s in (65535, 65536, n - 1):
        assert (got[s] == got[s % nb]).all()


# ---- 7. predict_batch(sample_rate=...) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n_in", [(8000, 1280), (44100, 7056)])
def test_predict_batch_converts_two_chunk_messages(rate, n_in):
    from openwakeword_amd.model import BatchedModel
    rng = np.random.default_rng(rate)
    wts = {"heads": {"alexa": W.synthetic_head("alexa", seed=1)}, "embedding": W.synthetic_embedding(seed=3)}
    a, b, c = (BatchedModel(6, ["alexa"], weights=wts, max_chunks=2) for _ in range(3))
    try:
        for t in range(6):
            x = (rng.standard_normal((6, n_in)) * 5000).astype(np.int16)
            got = a.predict_batch(x, sample_rate=rate)
            x16 = b.engine.resample(x, rate)
            assert x16.shape == (6, 2560)
            twin = b.predict_batch(x16)
            assert (got == twin).all(), f"message {t}: predict_batch(sample_rate) differs from resample + predict_batch"
            want = c.predict_batch(R.apply_numpy(x, rate))
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-4)
        with pytest.raises(ValueError):
            a.predict_batch(np.zeros((6, n_in + 16), np.int16), sample_rate=rate)
    finally:
        a.close(); b.close(); c.close()
