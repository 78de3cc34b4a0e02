"""The stateful stream ingest on the device (`ingest_stream<ENC>` behind `ingest_kernel` and `ingest_mixed_kernel`) at every rate the
server serves, in the server's full 13-class table, and under the server itself in device mode.  tests/ingest_rates.py holds the
classes, the message plans and the float64 reference; tests/test_ingest_rates_cpu.py shows that the table reaches every branch and
that the budget is attainable and rejects wrong streams.  The assertions here are `RR.excess <= 0` (the derived `0.5 + gamma * A` of
tests/resample_ref.py), bit equality, return codes and message text; `RR.worst_ratio` is printed (run with -s), never asserted."""
import asyncio
import ctypes as C
import json

import numpy as np
import pytest

pytest.importorskip("aiohttp")                                          # (ingest_rates takes the rates from openwakeword_amd.serve, which needs it)
import ingest_rates as IR  # noqa: E402
import resample_ref as RR
from openwakeword_amd import resample as R
from openwakeword_amd import weights as W

pytestmark = pytest.mark.gpu
S = IR.S
N_OUT, N_MSG, TOTAL = IR.N_OUT, IR.N_MSG, IR.TOTAL
OWW_EINVAL = -1
HEADS = ["alexa", "hey_mycroft", "hey_jarvis"]                               # the three synthetic heads of tests/test_masked_step.py
TELEPHONY = [(8000, "ulaw"), (8000, "alaw"), (8000, "pcm16")]


def _new_engine(n_streams=S, **kw):
    from openwakeword_amd.engine import StreamEngine
    return StreamEngine(n_streams, {"alexa": W.synthetic_head("alexa", seed=1)}, W.synthetic_embedding(seed=3), **kw)


@pytest.fixture(scope="module")
def eng():
    """the single-format handle"""
    e = _new_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def mix():
    """the handle that carries class tables"""
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


def _feed(e, fed, sizes):
    """the recording's messages `sizes` one after the other -> int16 [S, their outputs]"""
    outs, at = [], 0
    for n in sizes:
        outs.append(e.ingest(np.ascontiguousarray(fed[:, at:at + n])))
        at += n
    return np.concatenate(outs, axis=1)


_six = {}


def six_frames(eng, rate, enc):
    """the single-format kernel's output for the six 80 ms frames, computed once per class"""
    if (rate, enc) not in _six:
        eng.configure_ingest(rate, enc)
        got = _feed(eng, IR.recording(rate, enc)[0], IR.MESSAGE_PLANS[(rate, enc)]["six"])
        got.setflags(write=False)
        _six[(rate, enc)] = got
    return _six[(rate, enc)]


def _assert_budget(got, rate, enc, what, rows=None):
    if not IR.params(rate, enc)[3]:                                          # decode only: the decoded samples themselves
        dec = IR.recording(rate, enc)[1]
        assert (got == (dec if rows is None else dec[rows])[:, :got.shape[1]]).all(), f"{what}: decode only differs from the decoded samples"
        return 0.0
    over, worst = IR.holds_budget(got, rate, enc, rows)
    print(f"{what}: worst (err - 0.5)+ / (gamma*A) = {worst:.3f}, max excess {over.max():.3f}")
    assert (over <= 0).all(), f"{what}: {int((over > 0).sum())} outputs outside 0.5 + gamma*A, worst by {over.max():.3f} LSB at " \
                              f"{np.unravel_index(np.argmax(over), over.shape)}"
    return worst


# ---- a. every class, single form, against float64 and the stateless kernel ----------------------------------------------------------------
@pytest.mark.parametrize("rate,enc", IR.CLASSES)
def test_six_frames_hold_the_budget_and_equal_the_stateless_kernel(eng, rate, enc):
    got = six_frames(eng, rate, enc)
    pre, y, _ = IR.reference(rate, enc)
    assert got.dtype == np.int16 and got.shape == y.shape == (S, TOTAL)
    _assert_budget(got, rate, enc, f"{rate} Hz {enc}")
    if IR.params(rate, enc)[3]:
        want = eng.resample(np.ascontiguousarray(pre), rate)[:, :TOTAL]
        bad = np.argwhere(got != want)
        assert not len(bad), f"{rate} Hz {enc}: {len(bad)} outputs differ from oww_resample(zeros(half) | whole), first at {bad[0]}"
    assert (got != 0).any()


# ---- b. message cuts, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,enc", IR.CLASSES)
def test_message_cuts_change_no_bit(eng, rate, enc):
    six = six_frames(eng, rate, enc)
    fed = IR.recording(rate, enc)[0]
    for name, sizes in IR.MESSAGE_PLANS[(rate, enc)].items():
        if name == "six":
            continue
        eng.configure_ingest(rate, enc)                                      # (zeroes every history)
        got = _feed(eng, fed, sizes)
        bad = np.argwhere(got != six[:, :got.shape[1]])
        assert not len(bad), f"{rate} Hz {enc}, plan {name} {sizes[:4]}...: {len(bad)} outputs differ from the six frames, first at {bad[0]}"
        assert got.shape[1] == sum(sizes) * IR.params(rate, enc)[1] // IR.params(rate, enc)[0]


# ---- c. vector and element-wise forms agree -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,enc", [(48000, "pcm16"), (8000, "pcm16"), (8000, "ulaw")])
def test_vector_and_element_wise_forms_agree(eng, rate, enc):
    """The same two frames from a 16-byte aligned device buffer (16-byte loads) and from buffers 2 and (G.711) 1 bytes off (element-wise
    loads), into an aligned output (16-byte stores) and one 2 bytes off (element-wise stores): outputs and next histories, bit for bit."""
    import torch
    lib, n_in = _lib(), IR.frame(rate)
    fed = IR.recording(rate, enc)[0]
    six = six_frames(eng, rate, enc)
    assert IR.geometry_n_in(rate, enc, n_in)["vec_in"] and IR.geometry_n_in(rate, enc, n_in)["vec_out"]
    results = {}
    offsets = [(0, 0), (2, 2), (0, 2), (2, 0)] + ([(1, 2), (1, 0)] if enc != "pcm16" else [])
    for in_off, out_off in offsets:
        eng.configure_ingest(rate, enc)
        outs, states = [], []
        for k in range(2):
            raw = np.ascontiguousarray(fed[:, n_in * k:n_in * (k + 1)]).view(np.uint8).reshape(-1)
            d_in = torch.zeros(raw.size + 32, dtype=torch.uint8, device="cuda")
            d_out = torch.full((S * N_OUT + 16,), 12345, dtype=torch.int16, device="cuda")
            assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
            d_in[in_off:in_off + raw.size] = torch.from_numpy(raw).cuda()
            torch.cuda.synchronize()
            rc = lib.oww_ingest(eng._h, _vp(d_in.data_ptr() + in_off), 1, n_in, None, 0, _vp(d_out.data_ptr() + out_off), 1)
            assert rc == 0, _err()
            states.append(eng.export_state(np.arange(S)).copy())             # (waits for the handle's stream)
            torch.cuda.synchronize()
            host = d_out.cpu().numpy()
            o = out_off // 2
            outs.append(host[o:o + S * N_OUT].reshape(S, N_OUT).copy())
            assert (host[:o] == 12345).all() and (host[o + S * N_OUT:] == 12345).all(), "the kernel wrote outside its output rows"
        results[(in_off, out_off)] = (np.concatenate(outs, axis=1), states)
    base_out, base_states = results[(0, 0)]
    assert (base_out == six[:, :2 * N_OUT]).all(), "device buffers give other bits than host buffers"
    assert (base_states[0] != base_states[1]).any()
    for key, (out, states) in results.items():
        bad = np.argwhere(out != base_out)
        assert not len(bad), f"{rate} Hz {enc}, input {key[0]} and output {key[1]} bytes off 16: {len(bad)} outputs differ, first at {bad[0]}"
        for k in range(2):
            assert (states[k] == base_states[k]).all(), f"{rate} Hz {enc}, offsets {key}: the state record after message {k} differs"


# ---- d. the server's full class table in one launch -------------------------------------------------------------------------------------------
def _rows(classes, cls, k, src_msg=None):
    """message k (src_msg[s] overrides it per stream) of every stream's own recording row, packed for `classes`"""
    arrs = []
    for s in range(S):
        rate, enc = classes[int(cls[s])]
        n, m = IR.frame(rate), k if src_msg is None else int(src_msg[s])
        arrs.append(IR.recording(rate, enc)[0][s, n * m:n * (m + 1)])
    return R.pack_ingest_rows(arrs, cls, classes, N_OUT)


def _mixed_six(mix, classes, cls):
    mix.reset()
    mix.configure_ingest_classes(classes)
    mix.assign_ingest(np.arange(S), cls)
    assert mix.ingest_row_bytes() == R.class_row_bytes(classes)
    return np.concatenate([mix.ingest_mixed(_rows(classes, cls, k)) for k in range(N_MSG)], axis=1)


def _assert_classes_equal_single(eng, got, classes, cls, what):
    for c, (rate, enc) in enumerate(classes):
        mine = np.flatnonzero(cls == c)
        assert len(mine)
        want = six_frames(eng, rate, enc)
        bad = np.argwhere(got[mine] != want[mine])
        assert not len(bad), f"{what}, class {(rate, enc)}: {len(bad)} outputs differ from ingest_kernel, first at stream {mine[bad[0][0]]}, " \
                             f"output {bad[0][1]}"
        _assert_budget(got[mine], rate, enc, f"{what}, {rate} Hz {enc}", rows=mine)


def test_the_servers_full_table_in_one_launch(eng, mix):
    pytest.importorskip("aiohttp")
    classes = IR.server_default_classes()
    assert len(classes) == 13
    cls = (np.arange(S) % 13).astype(np.uint8)
    full = _mixed_six(mix, classes, cls)
    assert full.shape == (S, TOTAL)
    _assert_classes_equal_single(eng, full, classes, cls, "13 classes")
    # the telephony table: rows of 1,280 bytes, the smallest LDS allocation; every 8 kHz stream of the full table keeps its class
    to_tel = {classes.index(c): i for i, c in enumerate(TELEPHONY)}
    cls_tel = np.array([to_tel.get(int(c), s % 3) for s, c in enumerate(cls)], np.uint8)
    assert R.class_row_bytes(TELEPHONY) == 1280
    tel = _mixed_six(mix, TELEPHONY, cls_tel)
    _assert_classes_equal_single(eng, tel, TELEPHONY, cls_tel, "telephony table")
    same = np.flatnonzero(np.isin(cls, list(to_tel)))
    assert len(same) >= 6 and all(classes[cls[s]] == TELEPHONY[cls_tel[s]] for s in same)
    bad = np.argwhere(full[same] != tel[same])
    assert not len(bad), f"the 8 kHz streams carry other bits under the telephony table than under the full one, first at {bad[0]}"


def test_a_masked_message_in_the_full_table(eng, mix):
    pytest.importorskip("aiohttp")
    classes = IR.server_default_classes()
    cls = (np.arange(S) % 13).astype(np.uint8)
    off = (np.arange(S) % 3 == 1) | (np.arange(S) == 11)                     # a third of the streams, and every class among them
    assert set(cls[off]) == set(range(13)) and 12 <= off.sum() <= 13
    mix.reset()
    mix.configure_ingest_classes(classes)
    mix.assign_ingest(np.arange(S), cls)
    for k in range(2):
        mix.ingest_mixed(_rows(classes, cls, k))
    before = mix.export_state(np.arange(S))
    out = np.full((S, N_OUT), 12345, np.int16)
    mix.ingest_mixed(_rows(classes, cls, 2), stream_on=~off, out=out)
    after = mix.export_state(np.arange(S))
    assert (out[off] == 12345).all(), "the output row of a stream that sat out was written"
    assert (after[off] == before[off]).all(), "the state record of a stream that sat out changed"
    # the next message: the streams that sat out get their third frame now, the others their fourth
    nxt = mix.ingest_mixed(_rows(classes, cls, 0, src_msg=np.where(off, 2, 3)))
    for s in range(S):
        rate, enc = classes[cls[s]]
        want = six_frames(eng, rate, enc)
        if not off[s]:
            assert (out[s] == want[s, 2 * N_OUT:3 * N_OUT]).all(), f"stream {s} ({rate} Hz {enc}): the masked launch changed a served stream"
        k = 2 if off[s] else 3
        assert (nxt[s] == want[s, k * N_OUT:(k + 1) * N_OUT]).all(), \
            f"stream {s} ({rate} Hz {enc}, {'sat out' if off[s] else 'served'}): the message after the masked one differs from the consecutive run"


# ---- e. the staging edge at the longest history ---------------------------------------------------------------------------------------------
def test_the_staging_edge_at_96_khz(eng):
    rate, enc = 96000, "pcm16"
    last, first = IR.EDGE96
    fed = IR.recording(rate, enc)[0]
    six = six_frames(eng, rate, enc)
    assert last % 6 == 0 and first == last + 6 and fed.shape[1] >= last + IR.frame(rate)
    eng.configure_ingest(rate, enc)
    got = _feed(eng, fed, [last, IR.frame(rate)])                            # the largest message, and a frame behind it from its history
    assert got.shape == (S, last // 6 + N_OUT)
    bad = np.argwhere(got != six[:, :got.shape[1]])
    assert not len(bad), f"a message of {last} samples: {len(bad)} outputs differ from the same samples fed as frames, first at {bad[0]}"
    _assert_budget(got, rate, enc, f"96 kHz, one message of {last} samples")
    # one step further is refused, and moves nothing
    eng.configure_ingest(rate, enc)
    a = eng.ingest(np.ascontiguousarray(fed[:, :7680]))
    big = np.ascontiguousarray(fed[:, 7680:7680 + first])
    rc = _lib().oww_ingest(eng._h, _vp(big), 0, first, None, 0, None, 0)
    msg = _err()
    assert rc == OWW_EINVAL and "LDS" in msg and str(first) in msg and "153" in msg, (rc, msg)
    b = eng.ingest(np.ascontiguousarray(fed[:, 7680:15360]))
    assert (a == six[:, :N_OUT]).all() and (b == six[:, N_OUT:2 * N_OUT]).all(), "the message after a refusal differs from a handle that never saw it"


# ---- f. the server in device mode on real kernels ---------------------------------------------------------------------------------------------
def _model(n):
    from openwakeword_amd.model import BatchedModel
    heads = {h: W.synthetic_head(h, seed=11 + i) for i, h in enumerate(HEADS)}
    return BatchedModel(n, HEADS, weights={"heads": heads, "embedding": W.synthetic_embedding(seed=3)})


def _private_engine():
    from openwakeword_amd.engine import StreamEngine
    heads = {h: W.synthetic_head(h, seed=11 + i) for i, h in enumerate(HEADS)}
    return StreamEngine(1, heads, W.synthetic_embedding(seed=3), use_mfma=3)


def _announce(rate, enc):
    return str(rate) if enc == "pcm16" else f"{rate} {enc}"


def _client_audio(rng, rate, enc, n_frames):
    n = IR.frame(rate) * n_frames
    if enc == "pcm16":
        return (rng.standard_normal(n) * 5000).astype("<i2")
    return rng.integers(0, 256, n).astype(np.uint8)


def _message_sizes(i, frame_bytes, total, unit):
    """bytes per websocket message of client i: whole frames; several messages per frame, none a multiple of 16 bytes; or a backlog of
    three frames in one message and uneven pieces behind it"""
    if i % 3 == 0:
        return [frame_bytes] * (total // frame_bytes)
    sizes = [] if i % 3 == 1 else [3 * frame_bytes]
    left = total - sum(sizes)
    piece = frame_bytes // 3 // unit * unit                                  # whole samples, about three messages per frame
    while piece % 16 == 0:
        piece += unit
    while left:
        n = min(left, piece)
        sizes.append(n)
        left -= n
    assert sum(sizes) == total and all(n % unit == 0 for n in sizes)
    return sizes


def _private_scores(e, x, rate, enc):
    """a private one-stream handle in the client's format, fed its whole frames through step_ingest"""
    e.reset()
    e.configure_ingest(rate, enc)
    n = IR.frame(rate)
    return np.stack([e.step_ingest(np.ascontiguousarray(x[None, n * k:n * (k + 1)]))[0].copy() for k in range(x.size // n)])


def test_the_server_in_device_mode_on_real_kernels():
    """Thirteen websocket clients, one per class of the default table, against a 16-slot server with ingest="device": every client's
    tapped score rows equal a private handle of its format, and the activation messages are the labels at or above the threshold."""
    pytest.importorskip("aiohttp")
    from aiohttp.test_utils import TestClient, TestServer
    from openwakeword_amd.serve import FanInServer
    n_frames, threshold = 12, 0.02                                           # (the first five frames of a stream score zero)
    rng = np.random.default_rng(13)
    model = _model(16)
    tap = {}
    srv = FanInServer(model, threshold=threshold, window_s=0.002, ingest="device",
                      on_scores=lambda cid, k, row: tap.setdefault(cid, []).append(row.copy()))
    classes = list(srv.classes)
    assert classes == IR.server_default_classes() and srv.row_bytes == 15360
    audio = [_client_audio(rng, rate, enc, n_frames) for rate, enc in classes]
    sizes = [_message_sizes(i, IR.frame(rate) * x.itemsize, x.nbytes, x.itemsize) for i, ((rate, enc), x) in enumerate(zip(classes, audio))]
    frames = [IR.frame(rate) * x.itemsize for (rate, _), x in zip(classes, audio)]
    assert any(n % 16 for sz in sizes for n in sz) and any(sz[0] == 3 * f for sz, f in zip(sizes, frames)) \
        and any(len(sz) > 2 * n_frames for sz in sizes) and any(sz == [f] * n_frames for sz, f in zip(sizes, frames))
    hits = [[] for _ in classes]

    async def client(ws, i):
        await ws.send_str(_announce(*classes[i]))
        raw, o = audio[i].tobytes(), 0
        for j, n in enumerate(sizes[i]):
            await ws.send_bytes(raw[o:o + n])
            o += n
            if j % 3 == i % 3:
                await asyncio.sleep(0.002)
        quiet = 0
        while quiet < 2:                                                     # (the tap fills before the step's messages go out: drain past completion)
            try:
                msg = await ws.receive(timeout=0.1)
                if msg.data:
                    hits[i].append(json.loads(msg.data)["activations"])
                    continue
            except asyncio.TimeoutError:
                pass
            if len(tap.get(i, [])) >= n_frames:
                quiet += 1
        await ws.close()

    async def run():
        async with TestClient(TestServer(srv.app())) as tc:
            wss = []
            for i in range(len(classes)):                                    # one after the other: client i is connection i
                ws = await tc.ws_connect("/ws")
                assert json.loads((await ws.receive()).data)["loaded_models"] == HEADS
                assert srv.conns[i].cid == i
                wss.append(ws)
            await asyncio.gather(*[client(ws, i) for i, ws in enumerate(wss)])

    try:
        asyncio.run(asyncio.wait_for(run(), 120))
    finally:
        model.close()
    assert srv.failed is None and srv.n_stream_steps == n_frames * len(classes)
    e = _private_engine()
    try:
        for i, (rate, enc) in enumerate(classes):
            private = _private_scores(e, audio[i], rate, enc)
            assert len(tap[i]) == n_frames == len(private)
            print(f"client {i} ({rate} Hz {enc}): {len(sizes[i])} messages, largest score {private.max():.4f}")
            np.testing.assert_array_equal(np.stack(tap[i]), private, err_msg=f"client {i} ({rate} Hz {enc})")
            want = [[HEADS[j] for j in np.nonzero(r >= threshold)[0]] for r in private]
            assert hits[i] == [w for w in want if w], f"client {i} ({rate} Hz {enc})"
    finally:
        e.close()
    assert any(hits), "no client had an activation: the message check showed nothing"


@pytest.mark.parametrize("order", [((96000, "pcm16"), (8000, "ulaw")), ((8000, "ulaw"), (96000, "pcm16"))])
def test_a_slot_that_changes_class_starts_from_silence(order):
    """Two slots; a client leaves and a client of another class takes its slot: its scores equal a fresh private handle's, so
    `ingest_assign_kernel` zeroed the whole history row (160 samples for 96 kHz, 32 for 8 kHz), not only the new class's part."""
    pytest.importorskip("aiohttp")
    from aiohttp.test_utils import TestClient, TestServer
    from openwakeword_amd.serve import FanInServer
    n_frames = 7
    rng = np.random.default_rng(29)
    model = _model(2)
    tap = {}
    srv = FanInServer(model, threshold=2.0, window_s=0.0, ingest="device",
                      on_scores=lambda cid, k, row: tap.setdefault(cid, []).append(row.copy()))
    audio = [_client_audio(rng, rate, enc, n_frames) for rate, enc in order]

    async def run():
        async with TestClient(TestServer(srv.app())) as tc:
            for cid, (rate, enc) in enumerate(order):
                ws = await tc.ws_connect("/ws")
                await ws.receive()
                await ws.send_str(_announce(rate, enc))
                await ws.send_bytes(audio[cid].tobytes())                    # one message, seven frames
                while len(tap.get(cid, [])) < n_frames:
                    await asyncio.sleep(0.005)
                assert srv.conns[cid].slot == 0 and sorted(srv.clients) == [0]
                await ws.close()
                while cid in srv.conns:
                    await asyncio.sleep(0.005)

    try:
        asyncio.run(asyncio.wait_for(run(), 60))
    finally:
        model.close()
    assert srv.failed is None
    e = _private_engine()
    try:
        for cid, (rate, enc) in enumerate(order):
            private = _private_scores(e, audio[cid], rate, enc)
            np.testing.assert_array_equal(np.stack(tap[cid]), private, err_msg=f"connection {cid} ({rate} Hz {enc}) in the reused slot")
        assert (np.stack(tap[1])[5:] != 0).any()                             # (past the first-five zeroing: real scores were compared)
    finally:
        e.close()
