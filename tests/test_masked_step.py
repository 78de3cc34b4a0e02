"""oww_step_masked: a stream that sits a step out keeps every bit of its state (the batched form of a client that does not call
predict() while it has no audio, examples/web/streaming_server.py:49-66), and the fan-in server built on it gives every websocket
client the scores of a private model."""
import asyncio
import json

import numpy as np
import pytest

from openwakeword_amd import weights as W

pytestmark = pytest.mark.gpu

HEADS = ["alexa", "hey_mycroft", "hey_jarvis"]


def _engine(S, heads=HEADS, vad=None, vad_threshold=0.0, family=3):
    from openwakeword_amd.engine import StreamEngine
    hs = {n: W.synthetic_head(n, seed=11 + i) for i, n in enumerate(heads)}
    return StreamEngine(S, hs, W.synthetic_embedding(seed=3), vad=vad, vad_threshold=vad_threshold, use_mfma=family)


def _pcm(rng, S, T):
    return (rng.standard_normal((T, S, 1280)) * 4000).astype(np.int16)


@pytest.mark.parametrize("S,with_vad,frac,family,heads", [
    (40, False, 0.6, 3, HEADS), (200, False, 0.6, 3, HEADS), (72, True, 0.6, 3, HEADS),
    (200, False, 0.12, 3, HEADS), (330, True, 0.1, 3, HEADS), (1000, False, 0.03, 3, HEADS),
    # the exact-fp32 family (what a network the fp16 split refuses is served by: VERDICT r04 next 4) and heads outside the fast
    # [T,96] -> 64 -> 64 -> 1 form (the multiclass `timer`, generic head kernel): full launches, participant-only stores
    (40, False, 0.6, 1, HEADS), (200, False, 0.12, 1, HEADS), (72, True, 0.5, 1, HEADS), (330, False, 0.3, 1, ["alexa", "timer"]),
    (200, False, 0.4, 3, ["timer", "hey_jarvis"]), (90, False, 0.1, 3, ["alexa", "timer"])])
def test_masked_step_equals_private_sequences(S, with_vad, frac, family, heads):
    """Random participation masks over 40 steps; every stream's k-th active step must equal, BIT FOR BIT, the k-th step of an
    unmasked engine that is fed the stream's active chunks back to back (S chosen to leave partly filled position tiles).
    frac <= 0.5: the library launches only the groups that hold a participating stream (build_active_lists; owwhip_masked_host.h): same results."""
    rng = np.random.default_rng(5)
    T = 40 if family == 3 else 24
    pcm = _pcm(rng, S, T)
    on = rng.random((T, S)) < frac
    on[:, 0] = True                      # one stream in every step
    on[:, 1] = False                     # one stream in none
    on[::2, 2] = True
    on[1::2, 2] = False
    vad = W.synthetic_vad(seed=9) if with_vad else None
    thr = 0.5 if with_vad else 0.0
    a, b = _engine(S, heads, vad, thr, family), _engine(S, heads, vad, thr, family)
    first = a.step(np.zeros((S, 1280), np.int16)).copy()       # a plain step first, so that "previous scores" exist
    b.step(np.zeros((S, 1280), np.int16))
    masked = np.empty((T, S, a.n_labels), np.float32)
    for t in range(T):
        junk = pcm[t].copy()
        junk[~on[t]] = 12345                                    # samples of a stream sitting out must not be read
        masked[t] = a.step_masked(junk, on[t])
    # reference: stream s gets its active chunks at plain steps 0, 1, 2, ...
    counts = on.sum(0)
    K = int(counts.max())
    packed = np.zeros((K, S, 1280), np.int16)
    for s in range(S):
        packed[:counts[s], s] = pcm[on[:, s], s]
    plain = np.stack([b.step(packed[k]) for k in range(K)])
    for s in range(S):
        ts = np.nonzero(on[:, s])[0]
        np.testing.assert_array_equal(masked[ts, s], plain[:len(ts), s], err_msg=f"stream {s}")
        prev = first[s]
        for t in range(T):                                       # sitting out repeats the previous step's scores
            if not on[t, s]:
                np.testing.assert_array_equal(masked[t, s], prev)
            prev = masked[t, s]
    assert np.abs(masked).max() > 0
    if with_vad:
        assert np.isfinite(a.get_vad()).all()
    a.close(); b.close()


def test_masked_step_with_verifier_and_two_groups():
    """Heads of two window lengths (post-processing in its own launch) and a custom verifier: the masks reach those kernels too."""
    from openwakeword_amd.engine import StreamEngine
    rng = np.random.default_rng(6)
    S, T = 48, 24
    hs = {"a16": W.synthetic_head("a16", seed=1), "b28": W.synthetic_head("b28", seed=2, T=28)}

    def make():
        e = StreamEngine(S, hs, W.synthetic_embedding(seed=3))
        e.set_verifier(0, (rng0.standard_normal(16 * 96) * 0.01).astype(np.float32), 0.1, 0.0)
        return e
    rng0 = np.random.default_rng(1); a = make()
    rng0 = np.random.default_rng(1); b = make()
    pcm = _pcm(rng, S, T)
    on = rng.random((T, S)) < 0.5
    masked = np.stack([a.step_masked(pcm[t], on[t]) for t in range(T)])
    counts = on.sum(0)
    packed = np.zeros((int(counts.max()), S, 1280), np.int16)
    for s in range(S):
        packed[:counts[s], s] = pcm[on[:, s], s]
    plain = np.stack([b.step(p) for p in packed])
    for s in range(S):
        ts = np.nonzero(on[:, s])[0]
        np.testing.assert_array_equal(masked[ts, s], plain[:len(ts), s], err_msg=f"stream {s}")
    a.close(); b.close()


def test_masked_step_argument_errors():
    from openwakeword_amd.engine import StreamEngine
    e = _engine(8)
    with pytest.raises(ValueError):
        e.step_masked(np.zeros((8, 2560), np.int16), np.ones(8))
    with pytest.raises(ValueError):
        e.step_masked(np.zeros((8, 1280), np.int16), np.ones(7))
    e.close()
    hs = {"alexa": W.synthetic_head("alexa", seed=1)}
    f = StreamEngine(8, hs, W.synthetic_embedding(seed=3), use_mfma=2)          # LDS-tiled families: not supported, loudly
    from openwakeword_amd._lib import OwwError
    with pytest.raises(OwwError, match="register-resident"):
        f.step_masked(np.zeros((8, 1280), np.int16), np.ones(8))
    f.close()


def test_fan_in_server_gives_each_client_private_scores():
    """Five websocket clients with different sample rates, message sizes and pacing against one 8-slot server; the per-stream-step
    tap must equal a private single-stream engine run on each client's (resampled) audio, and the activation messages must be the
    labels at or above the threshold."""
    from aiohttp.test_utils import TestClient, TestServer
    from openwakeword_amd.model import BatchedModel
    from openwakeword_amd.serve import FanInServer, to_16k

    rng = np.random.default_rng(8)
    heads = {n: W.synthetic_head(n, seed=11 + i) for i, n in enumerate(HEADS)}
    wts = {"heads": heads, "embedding": W.synthetic_embedding(seed=3)}
    model = BatchedModel(8, HEADS, weights=wts)
    tap = {}
    srv = FanInServer(model, threshold=0.02, window_s=0.002,
                      on_scores=lambda cid, k, row: tap.setdefault(cid, []).append(row.copy()))
    plans = [(16000, 1280, 30), (16000, 700, 41), (8000, 640, 36), (48000, 4096, 25), (16000, 5000, 9)]   # rate, samples/message, messages
    audio = [(rng.standard_normal(n * m) * 5000).astype(np.int16) for _r, n, m in plans]
    got = [dict(loaded=None, hits=[]) for _ in plans]

    async def client(ws, i):
        rate, n, m = plans[i]
        await ws.send_str(str(rate))
        for k in range(m):
            await ws.send_bytes(audio[i][k * n:(k + 1) * n].tobytes())
            if k % 3 == i % 3:
                await asyncio.sleep(0.003 * (i + 1))
        expect_steps = sum(to_16k(audio[i][k * n:(k + 1) * n], rate).size for k in range(m)) // 1280
        # read activation messages until the server has scored everything this client sent
        quiet = 0
        while quiet < 2:                       # (the tap fills before the step's messages go out: drain past completion)
            try:
                msg = await ws.receive(timeout=0.1)
                if msg.data:
                    got[i]["hits"].append(json.loads(msg.data)["activations"])
                    continue
            except asyncio.TimeoutError:
                pass
            if len(tap.get(i, [])) >= expect_steps:
                quiet += 1
        await ws.close()
        return expect_steps

    async def run():
        async with TestClient(TestServer(srv.app())) as tc:
            wss = []
            for i in range(len(plans)):          # one after the other: client i is connection i (its slot comes with its first audio)
                ws = await tc.ws_connect("/ws")
                got[i]["loaded"] = json.loads((await ws.receive()).data)["loaded_models"]
                assert srv.conns[i].cid == i and srv.conns[i].slot is None
                wss.append(ws)
            return await asyncio.gather(*[client(ws, i) for i, ws in enumerate(wss)])

    steps = asyncio.run(asyncio.wait_for(run(), 120))
    model.close()
    assert all(g["loaded"] == HEADS for g in got)
    assert srv.n_stream_steps == sum(steps) and srv.n_steps < sum(steps)          # steps were shared between clients
    for i, (rate, n, m) in enumerate(plans):
        x = np.concatenate([to_16k(audio[i][k * n:(k + 1) * n], rate) for k in range(m)])
        e = _engine(1)
        private = np.stack([e.step(x[None, k * 1280:(k + 1) * 1280])[0] for k in range(x.size // 1280)])
        e.close()
        assert len(private) == steps[i]
        np.testing.assert_array_equal(np.stack(tap[i]), private, err_msg=f"client {i}")
        want = [[HEADS[j] for j in np.nonzero(r >= 0.02)[0]] for r in private]
        assert got[i]["hits"] == [w for w in want if w], f"client {i}"
    assert any(g["hits"] for g in got)


def test_masked_step_properties_at_scale():
    """65,536 x 3 (BASELINE configs[2]): an all-ones mask is oww_step bit for bit, an all-zeros step changes nothing, and a
    half-on mask equals a plain step on exactly the rows it names -- checked on every stream (the oracle is not needed for
    these identities)."""
    import torch
    S, T = 65536, 12
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(17)
    pcm = [(torch.randn(S, 1280, device=dev, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16) for _ in range(T)]
    a, b = _engine(S), _engine(S)
    on_all = np.ones(S, np.uint8)
    half = (np.arange(S) * 2654435761 >> 7) & 1
    half = half.astype(np.uint8)
    zeros = np.zeros(S, np.uint8)
    last = None
    for t in range(T):
        x = pcm[t].cpu().numpy()
        sa = a.step_masked(x, on_all)
        sb = b.step(x)
        np.testing.assert_array_equal(sa, sb)
        if t == 5:                                              # three steps nobody takes part in
            for _ in range(3):
                np.testing.assert_array_equal(a.step_masked(pcm[0].cpu().numpy(), zeros), sa)
        last = sb
    # half the streams advance in a, all of them in b: the advanced rows agree, the others repeat a's previous scores
    x = pcm[3].cpu().numpy()
    sa = a.step_masked(x, half)
    sb = b.step(x)
    np.testing.assert_array_equal(sa[half == 1], sb[half == 1])
    np.testing.assert_array_equal(sa[half == 0], last[half == 0])
    assert (sb != last).any()
    a.close(); b.close()


def test_fan_in_server_slot_reuse_and_refusal():
    """Two slots: a third simultaneous client is refused (close code 1013); when a client leaves, the next one gets its slot in
    the state of a fresh model (first-5 zeroing, empty sample tail, initial feature ring) -- its scores equal a private engine's."""
    from aiohttp import WSMsgType
    from aiohttp.test_utils import TestClient, TestServer
    from openwakeword_amd.model import BatchedModel
    from openwakeword_amd.serve import FanInServer

    rng = np.random.default_rng(21)
    heads = {n: W.synthetic_head(n, seed=11 + i) for i, n in enumerate(HEADS)}
    model = BatchedModel(2, HEADS, weights={"heads": heads, "embedding": W.synthetic_embedding(seed=3)})
    tap = {}
    srv = FanInServer(model, threshold=2.0, window_s=0.0, on_scores=lambda cid, k, row: tap.setdefault(cid, []).append(row.copy()))
    first = (rng.standard_normal(1280 * 12) * 6000).astype(np.int16)
    second = (rng.standard_normal(1280 * 9) * 2000).astype(np.int16)

    async def run():
        async with TestClient(TestServer(srv.app())) as tc:
            a = await tc.ws_connect("/ws"); await a.receive()
            b = await tc.ws_connect("/ws"); await b.receive()
            c = await tc.ws_connect("/ws")
            msg = await c.receive()
            assert msg.type in (WSMsgType.CLOSE, WSMsgType.CLOSING, WSMsgType.CLOSED) and c.close_code == 1013
            await a.send_str("16000")
            await a.send_bytes(first.tobytes())                       # one message, twelve chunks
            while len(tap.get(0, [])) < 12:
                await asyncio.sleep(0.01)
            assert srv.conns[0].slot == 0 and srv.conns[1].slot is None   # (b has not sent audio: no device state, no slot yet)
            await a.close()
            while 0 in srv.conns:
                await asyncio.sleep(0.01)
            n_before = len(tap[0])
            d = await tc.ws_connect("/ws"); await d.receive()        # connection 2 ...
            await d.send_bytes(second.tobytes())
            while len(tap.get(2, [])) < 9:
                await asyncio.sleep(0.01)
            assert srv.conns[2].slot == 0 and sorted(srv.clients) == [0]      # ... takes over slot 0
            await d.close(); await b.close()
            return n_before

    n_before = asyncio.run(asyncio.wait_for(run(), 60))
    model.close()
    assert n_before == 12
    for audio, got in ((first, tap[0]), (second, tap[2])):
        e = _engine(1)
        want = np.stack([e.step(audio[None, k * 1280:(k + 1) * 1280])[0] for k in range(audio.size // 1280)])
        e.close()
        np.testing.assert_array_equal(np.stack(got), want)
    assert (np.stack(tap[2][:5]) == 0).all()                           # model.py:331-333 for the new owner of the slot


@pytest.mark.parametrize("family", [3, 1])
def test_masked_submit_pipeline_equals_masked_steps(family):
    """oww_submit_masked with two steps in flight gives what blocking oww_step_masked calls give."""
    rng = np.random.default_rng(31)
    S, T = 96, 14
    pcm = _pcm(rng, S, T)
    on = rng.random((T, S)) < 0.7
    a, b = _engine(S, family=family), _engine(S, family=family)
    want = np.stack([a.step_masked(pcm[t], on[t]) for t in range(T)])
    bufs = [b.pinned_empty((S, 1280)) for _ in range(2)]
    got = []
    for t in range(T):
        bufs[t % 2][:] = pcm[t]
        b.submit(bufs[t % 2], on[t])
        if t >= 1:
            got.append(b.collect().copy())
    got.append(b.collect().copy())
    np.testing.assert_array_equal(np.stack(got), want)
    a.close(); b.close()


def test_serve_cli_with_two_worker_processes_on_one_port():
    """`python -m openwakeword_amd.serve --workers 2`: two server processes share the port (SO_REUSEPORT), each with its own handle on the
    GPU; every client gets the model list and one answer per 1280-sample chunk it sent (threshold 0), whichever worker took it."""
    import os
    import socket
    import subprocess
    import sys
    import time
    import aiohttp
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "openwakeword_amd.serve", "--workers", "2", "--streams", "8", "--models", "alexa", "hey_jarvis",
           "--weights", "synthetic", "--threshold", "0.0", "--host", "127.0.0.1", "--port", str(port)]
    p = subprocess.Popen(cmd, cwd=root, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        rng = np.random.default_rng(77)
        audio = [(rng.standard_normal(1280 * 6) * 4000).astype(np.int16) for _ in range(6)]

        async def client(session, x):
            for _ in range(600):                               # both workers import torch and create their handles first
                try:
                    ws = await session.ws_connect(f"http://127.0.0.1:{port}/ws")
                    break
                except aiohttp.ClientError:
                    assert p.poll() is None, p.stderr.read()[-2000:]
                    await asyncio.sleep(0.2)
            else:
                raise AssertionError("the server never came up")
            assert json.loads((await ws.receive()).data)["loaded_models"] == ["alexa", "hey_jarvis"]
            await ws.send_str("16000")
            await ws.send_bytes(x.tobytes())
            got = []
            while len(got) < x.size // 1280:
                msg = await ws.receive(timeout=60)
                got.append(json.loads(msg.data)["activations"])
            await ws.close()
            return got

        async def run():
            async with aiohttp.ClientSession() as session:
                first = await client(session, audio[0])        # (wait for the workers once, then the rest in parallel)
                rest = await asyncio.gather(*[client(session, x) for x in audio[1:]])
                return [first] + list(rest)
        answers = asyncio.run(asyncio.wait_for(run(), 300))
        assert all(len(a) == 6 and all(hits == ["alexa", "hey_jarvis"] for hits in a) for a in answers)
    finally:
        import signal
        os.killpg(p.pid, signal.SIGTERM)                        # the parent and its two workers: the process group this test started
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [2, 4, 6])
def test_random_many_stream_runs_match_one_oracle_model_per_stream(seed):
    """tools/fuzz_batched_vs_oracle.py: BatchedModel -- device post-processing (first-five zeroing, patience / debounce on the score
    rings), masked steps, resets of stream subsets in mid-run, multi-chunk calls, the device voice-activity stand-in and its gate --
    against one OracleModel per stream; 48 seeds x 140-150 steps of it ran clean on the GPU in round 6 (136 k scores, max 8.3e-6:
    profiles/r06_fuzz_batched_vs_oracle.txt)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz_batched_vs_oracle", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_batched_vs_oracle.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rec = fz.one_seed(seed, 45)
    assert rec["worst"] <= fz.TOL and rec["scores"] > 0
