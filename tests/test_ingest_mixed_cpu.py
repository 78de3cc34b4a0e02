"""Ingest classes without a GPU: the header and the ctypes binding, the host definition `resample.ingest_mixed_numpy` (per stream
`ingest_numpy`, bit for bit, and inside the derived budget `0.5 + gamma * A` of tests/resample_ref.py), the row packer, the frame
table of the server's rates, the HIP-free class table and argument checks (openwakeword_amd/csrc/owwhip_ingest.h) as a stand-alone
program under AddressSanitizer + UBSan, and the fan-in server's `ingest="device"` path through real (loopback) websockets with
stand-ins in the manner of tests/test_serve_pump_cpu.py: here the stand-in engine serves `submit_ingest_mixed` with
`ingest_mixed_numpy`.  Reference behaviour being replaced: per-message conversion in the handler
(examples/web/streaming_server.py:50-59)."""
import asyncio
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_ref as RR
from openwakeword_amd import _lib as L
from openwakeword_amd import resample as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLASSES = [(16000, "pcm16"), (8000, "ulaw"), (8000, "alaw"), (11025, "pcm16"), (44100, "pcm16"), (48000, "pcm16")]
FRAMES = {8000: 640, 11025: 882, 12000: 960, 16000: 1280, 22050: 1764, 24000: 1920, 32000: 2560, 44100: 3528, 48000: 3840, 88200: 7056,
          96000: 7680}
NEW = ("oww_ingest_configure_classes", "oww_ingest_assign", "oww_ingest_mixed", "oww_step_ingest_mixed", "oww_submit_ingest_mixed")


# ---- header and binding ------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "owwhip.h")) as f:
        return f.read()


def test_header_declares_the_entries_and_the_binding_matches():
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+OWW_INGEST_MAX_CLASSES\s+16\b", code) and L.INGEST_MAX_CLASSES == 16
    assert re.search(r"#define\s+OWW_ABI_VERSION\s+6\b", code)
    st = re.search(r"typedef struct oww_ingest_class \{(.*?)\} oww_ingest_class;", code, re.S)
    assert st, "struct oww_ingest_class is not declared"
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"const float\*", "", st.group(1)))
    assert fields == [n for n, _ in L.IngestClass._fields_] == ["encoding", "p", "q", "n_taps", "taps"]
    assert C.sizeof(L.IngestClass) == 24 and L.IngestClass.taps.offset == 16
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, re.S)
        assert m, f"{name} is not declared"
        want = []
        for arg in (a.strip() for a in m.group(1).split(",")):
            if "*" in arg:
                want.append(C.POINTER(L.IngestClass) if "oww_ingest_class" in arg else C.c_void_p)
            else:
                want.append(ctype[arg.split()[0]])
        res, args = L.SYMBOLS[name]
        assert res is C.c_int and args == want, f"{name}: ctypes prototype {args} against the header's {want}"
        assert "streaming_server.py:5" in src[src.index("ingest classes"):], "the header comment cites the seam it replaces"


# ---- the host definition -----------------------------------------------------------------------------------------------------------------
def _population(S=12, n_msg=6, seed=3):
    cls = np.arange(S) % len(CLASSES)
    rng = np.random.default_rng(seed)
    rec = []
    for s in range(S):
        rate, enc = CLASSES[cls[s]]
        n = R.class_n_in(rate, 1280 * n_msg)
        rec.append(RR.signals(rate, n)[s + 3].copy() if enc == "pcm16" else rng.integers(0, 256, n).astype(np.uint8))
    return cls, rec


def _whole(x, rate, enc):
    """one-piece conversion of a stream's recording: what ingest_numpy gives for the whole of it, rounded as the device rounds"""
    dec = R.decode(x, enc)
    if rate == 16000:
        return dec
    y, _ = R.ingest_numpy(dec, rate)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def test_ingest_mixed_numpy_is_ingest_numpy_per_stream_and_holds_the_budget():
    cls, rec = _population()
    S, hist, hist1 = len(rec), [None] * len(rec), [None] * len(rec)
    outs = []
    for k in range(6):
        arrs = []
        for s in range(S):
            n = R.class_n_in(CLASSES[cls[s]][0], 1280)
            arrs.append(rec[s][n * k:n * (k + 1)])
        rows = R.pack_ingest_rows(arrs, cls, CLASSES)
        assert rows.shape == (S, R.class_row_bytes(CLASSES)) == (S, 7680) and rows.dtype == np.uint8
        out = R.ingest_mixed_numpy(rows, cls, CLASSES, hist)
        for s in range(S):                                                   # per stream: ingest_numpy on that stream alone, bit for bit
            rate, enc = CLASSES[cls[s]]
            dec = R.decode(arrs[s], enc)
            if rate == 16000:
                want = dec
            else:
                y, hist1[s] = R.ingest_numpy(dec, rate, hist1[s])
                want = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
                assert (np.asarray(hist[s]) == np.asarray(hist1[s])).all()
            assert (out[s] == want).all(), f"message {k}, stream {s}"
        outs.append(out)
        rows0 = rows if k == 0 else rows0
    got = np.concatenate(outs, axis=1)
    for s in range(S):
        rate, enc = CLASSES[cls[s]]
        assert (got[s] == _whole(rec[s], rate, enc)).all(), f"stream {s}: six messages differ from the one-piece conversion"
        if rate == 16000:
            continue
        p, q, taps = R.design(rate)
        pre = np.concatenate([np.zeros(taps.shape[1] // 2, np.int16), R.decode(rec[s], enc)])[None, :]
        y, A = RR.ref64(pre, p, q, taps)
        over = RR.excess(got[s:s + 1], y[:, :got.shape[1]], A[:, :got.shape[1]], taps.shape[1])
        assert (over <= 0).all(), f"stream {s} ({rate} Hz {enc}): outside 0.5 + gamma*A by {over.max():.3f}"
    # a stream that sits out is not read, keeps its history and has a zero row
    before = [None if h is None else np.array(h, copy=True) for h in hist]
    on = np.ones(S, np.uint8)
    on[[1, 4]] = 0
    out = R.ingest_mixed_numpy(rows0, cls, CLASSES, hist, stream_on=on)
    assert not out[1].any() and not out[4].any() and (hist[1] == before[1]).all() and (hist[4] == before[4]).all()
    assert (hist[7] != before[7]).any()                                      # (random mu-law codes: served, its history moved on)


def test_pack_ingest_rows_refuses_wrong_lengths_and_dtypes():
    cls = [1, 5]
    ok = [np.zeros(640, np.uint8), np.zeros(3840, np.int16)]
    rows = R.pack_ingest_rows(ok, cls, CLASSES)
    assert rows.shape == (2, 7680)
    with pytest.raises(ValueError, match="640"):
        R.pack_ingest_rows([np.zeros(639, np.uint8), ok[1]], cls, CLASSES)
    with pytest.raises(ValueError, match="3840"):
        R.pack_ingest_rows([ok[0], np.zeros(3841, np.int16)], cls, CLASSES)
    with pytest.raises(ValueError, match="uint8"):
        R.pack_ingest_rows([np.zeros(640, np.int16), ok[1]], cls, CLASSES)
    with pytest.raises(ValueError, match="int16"):
        R.pack_ingest_rows([ok[0], np.zeros(3840, np.float32)], cls, CLASSES)
    with pytest.raises(ValueError, match="unknown class"):
        R.pack_ingest_rows(ok, [1, 6], CLASSES)
    with pytest.raises(ValueError, match="class ids"):
        R.pack_ingest_rows(ok, [1], CLASSES)
    with pytest.raises(ValueError, match="shape"):
        R.pack_ingest_rows([np.zeros((1, 640), np.uint8), ok[1]], cls, CLASSES)
    with pytest.raises(ValueError):
        R.pack_ingest_rows(ok, cls, CLASSES, out=np.zeros((2, 7680), np.int16))
    kept = np.full((2, 7680), 9, np.uint8)                                   # None: the row is left alone
    R.pack_ingest_rows([None, ok[1]], cls, CLASSES, out=kept)
    assert (kept[0] == 9).all() and not kept[1].any()
    with pytest.raises(ValueError, match="whole"):
        R.class_n_in(11025, 100)


def test_every_served_rate_has_a_whole_80_ms_frame():
    from openwakeword_amd import serve
    assert tuple(sorted(FRAMES)) == tuple(serve.RATES)
    for rate, n in FRAMES.items():
        assert R.class_n_in(rate) == n and n * 16000 == 1280 * rate
        if rate != 16000:
            p, q, _ = R.design(rate)
            assert (n * q) % p == 0 and n * q // p == 1280
    full = [(r, "pcm16") for r in serve.RATES] + [(8000, "ulaw"), (8000, "alaw")]
    assert len(full) == 13 <= L.INGEST_MAX_CLASSES and R.class_row_bytes(full) == 15360


# ---- the class table and the argument checks as a host program under the sanitizers -----------------------------------------------------
def test_class_table_and_checks_under_the_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    exe = str(tmp_path / "ingest_classes_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *sanitize, os.path.join(ROOT, "tests", "ingest_classes_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    got = dict(ln.split(" ", 1) for ln in run.stdout.splitlines())
    from openwakeword_amd import serve
    full = [(r, "pcm16") for r in serve.RATES] + [(8000, "ulaw"), (8000, "alaw")]
    params = [R.class_params(r, e) for r, e in full]
    floats = sum(q * ((nt + 3) // 4 * 4) for _, q, _, nt in params)
    hpad = max((nt - 1 + 7) // 8 * 8 if nt else 0 for _, _, _, nt in params)
    assert got["full"].startswith(f"rc=0 classes=13 bank_floats={floats} Hpad_max={hpad} last_off={floats - 2 * 28} last_slide=1 ")
    assert got["pad"] == "ntp=28 tail=0,0 first=2"
    # the launch's LDS: the 11.025 kHz class with its 640 x 28 bank behind history + message + the output tile
    lds = ((28 + 882 + 8 + 3) // 4 * 4) * 4 + 2048 * 2 + 640 * 28 * 4
    assert got["frame"] == f"rc=0 lds={lds} min_row=15360 -"
    for name, words in {"row_small": ("15344", "15360"), "row_odd": ("multiple of 16",), "not_whole": ("class 1", "441", "640"),
                        "lds": ("class 9", "LDS", "98304"), "null_in": ("null argument: in",), "n_out0": ("n_out=0",), "n_out_big": ("2^24",),
                        "seventeen": ("kept=1", "n_classes=17"), "zero": ("n_classes=0",), "null": ("null argument: classes",),
                        "bad0": ("kept=1", "class 3", "encoding 7"), "bad1": ("kept=1", "n_taps=25"), "bad2": ("kept=1", "decode only"),
                        "bad3": ("kept=1", "p=0"), "bad4": ("kept=1", "q=65537"), "bad5": ("kept=1", "n_taps=4098"),
                        "null_taps": ("null argument: taps",), "assign_class": ("unknown class 13",), "assign_stream": ("stream id 36",),
                        "assign_null": ("null list",)}.items():
        assert got[name].startswith("rc=-1 ") and all(w in got[name] for w in words), (name, got[name])
    assert got["decode_only"] == "rc=0 Hpad_max=0 bank_floats=1" and got["assign_ok"] == "rc=0" and got["assign_none"] == "rc=0"
    # the single form: one row, no `class` in its messages, and single_check with the launch's LDS as oww_ingest always sized it
    assert got["one_row"] == "rc=0 classes=1 bank_floats=56 Hpad_max=32 ntp=28 slide=1"
    for name, words in {"one_bad0": ("encoding 7",), "one_bad1": ("n_taps=25",), "one_bad2": ("n_taps = 0",), "one_bad3": ("p=0",),
                        "one_bad4": ("null argument: taps",), "s_zero": ("n_out=1280", "n_in=0"), "s_lds": ("n_out=1280", "30000", "LDS", "98304"),
                        "s_null": ("null argument: in",), "s_n_out_big": ("2^24",), "s_not_whole": ("100", "441")}.items():
        assert got[name].startswith("rc=-1 ") and all(w in got[name] for w in words), (name, got[name])
        assert "class" not in got[name] and (not name.startswith("one_bad") or ("kept=1" in got[name] and " c: " in got[name])), (name, got[name])
    lds = ((28 + 640 + 8 + 3) // 4 * 4) * 4 + 2048 * 2 + 2 * 28 * 4
    assert got["s_ulaw"] == f"rc=0 n_out=1280 lds={lds} xs_len=676 taps_in_lds=1 row=640 -"
    lds = ((28 + 16001 + 8 + 3) // 4 * 4) * 4 + 2048 * 2                     # the bank (16000 x 28 floats = 1.8 MB) stays in global memory
    assert got["s_big_bank"] == f"rc=0 n_out=16000 lds={lds} xs_len=16040 taps_in_lds=0 bank_floats={16000 * 28} -"
    # the fingerprint hashes the bytes the handle's two formulas hashed
    for name in ("fp_ulaw8k", "fp_pcm44k", "fp_full", "fp_decode_table", "fp_none"):
        assert got[name] == "equal=1", (name, got[name])
    assert got["fp_alaw_decode"] == "equal=1 placeholder=1"
    assert got["fp_single_vs_one_class"] == "differ=1 same_rows=1"


# ---- the server, device mode -------------------------------------------------------------------------------------------------------------
serve = pytest.importorskip("openwakeword_amd.serve")
pytest.importorskip("aiohttp")


class _Engine:
    """serves submit_ingest_mixed with the host definition; keeps every converted chunk per slot since the slot's last reset"""
    has_vad = False

    def __init__(self, S):
        self.S, self.q, self.classes = S, [], None
        self.cls, self.hist, self.by_slot = np.zeros(S, int), [None] * S, [[] for _ in range(S)]
        self.assigned = []

    def pinned_empty(self, shape, dtype=np.int16):
        return np.zeros(shape, dtype)

    def submit(self, pcm, on):                                               # ingest="host": 16 kHz chunks
        assert pcm.shape == (self.S, 1280) and pcm.dtype == np.int16 and len(self.q) < 2
        for s in np.nonzero(on)[0]:
            self.by_slot[s].append(pcm[s].copy())
        self.q.append(np.zeros((self.S, 2), np.float32))

    def submit_ingest_mixed(self, rows, on):
        assert rows.dtype == np.uint8 and rows.shape == (self.S, R.class_row_bytes(self.classes)) and len(self.q) < 2
        out = R.ingest_mixed_numpy(rows, self.cls, self.classes, self.hist, stream_on=on)
        for s in np.nonzero(on)[0]:
            self.by_slot[s].append(out[s].copy())
        self.q.append(np.zeros((self.S, 2), np.float32))

    def collect(self):
        return self.q.pop(0)


class _Model:
    labels, _keep = ["a", "b"], [0, 1]

    def __init__(self, S):
        self.n_streams, self.engine = S, _Engine(S)

    def configure_ingest_classes(self, formats):
        self.engine.classes = list(formats)

    def assign_ingest(self, ids, cls):
        for s, c in zip(ids, cls):
            self.engine.cls[s], self.engine.hist[s] = c, None
            self.engine.assigned.append((s, c, len(self.engine.by_slot[s])))

    def reset(self, ids=None, reset_vad=False):
        for s in ids:
            self.engine.hist[s], self.engine.by_slot[s] = None, []


def _serve(clients, S, ingest, rates=None):
    """clients: (rate message, bytes, message sizes in bytes); one after the other when S == 1.  -> per connection the scored chunks"""
    from aiohttp.test_utils import TestClient, TestServer
    model = _Model(S)
    got = {}

    def tap(cid, k, row):
        got.setdefault(cid, []).append(model.engine.by_slot[srv.conns[cid].slot][k].copy())
    srv = serve.FanInServer(model, threshold=2.0, window_s=0.001, on_scores=tap, ingest=ingest, rates=rates)

    async def client(tc, i, want, door):
        text, data, sizes = clients[i]
        async with door:                                                     # one connect at a time: the connection id is the last one given out
            ws = await tc.ws_connect("/ws")
            await ws.receive()
            cid = srv._next_cid - 1
        await ws.send_str(text)
        o = 0
        for j, n in enumerate(sizes):
            await ws.send_bytes(data[o:o + n])
            o += n
            if j % 3 == 2:
                await asyncio.sleep(0.002)
        assert o == len(data)
        for _ in range(2000):
            if len(got.get(cid, [])) >= want[i]:
                break
            await asyncio.sleep(0.002)
        await ws.close()
        return cid

    async def run(want):
        async with TestClient(TestServer(srv.app())) as tc:
            door = asyncio.Lock()
            if S == 1:
                cids = []
                for i in range(len(clients)):
                    cids.append(await client(tc, i, want, door))
                    await _gone(srv)
            else:
                cids = await asyncio.gather(*[client(tc, i, want, door) for i in range(len(clients))])
            await _gone(srv)
            return cids

    async def _gone(srv):
        for _ in range(1000):
            if not srv.conns:
                return False
            await asyncio.sleep(0.002)
        raise AssertionError("connections were not reaped")

    def go(want):
        return asyncio.run(asyncio.wait_for(run(want), 60))
    return go, got, srv, model


def _uneven(total, unit, seed):
    """message sizes in bytes: whole samples, uneven, summing to total"""
    rng, sizes, left = np.random.default_rng(seed), [], total
    while left:
        n = min(left, int(rng.integers(1, 700)) * unit)
        sizes.append(n)
        left -= n
    return sizes


def _recordings(n_frames=6):
    rng = np.random.default_rng(12)
    out = []
    for text, rate, enc in (("8000 ulaw", 8000, "ulaw"), ("16000", 16000, "pcm16"), ("44100", 44100, "pcm16"), ("48000", 48000, "pcm16"),
                            ("8000", 8000, "pcm16")):
        n = FRAMES[rate] * n_frames
        if enc == "pcm16":
            t = np.arange(n)
            x = (8000 * np.sin(2 * np.pi * 440.0 * t / rate) + rng.standard_normal(n) * 2000).astype("<i2")
        else:
            x = rng.integers(0, 256, n).astype(np.uint8)
        out.append((text, rate, enc, x))
    return out


def test_server_device_mode_scores_the_one_piece_conversion(monkeypatch):
    def no_host_resampler(*a, **k):
        raise AssertionError("to_16k was called with ingest=\"device\"")
    monkeypatch.setattr(serve, "to_16k", no_host_resampler)
    recs = _recordings()
    clients = [(text, x.tobytes(), _uneven(x.nbytes, x.itemsize, 40 + i)) for i, (text, rate, enc, x) in enumerate(recs)]
    go, got, srv, model = _serve(clients, S=8, ingest="device")
    assert len(srv.classes) == 13 and srv.row_bytes == 15360 and model.engine.classes == srv.classes
    cids = go([6] * len(clients))
    for i, (text, rate, enc, x) in enumerate(recs):
        want = _whole(x, rate, enc)
        chunks = got[cids[i]]
        assert len(chunks) == 6, f"{text}: {len(chunks)} chunks scored"
        assert (np.concatenate(chunks) == want).all(), f"{text}: the scored 16 kHz audio is not the one-piece conversion of the recording"
    assert srv.failed is None and srv.slots.n_used == 0 and int(srv._inflight.sum()) == 0


def test_host_mode_differs_at_message_edges_at_8_khz():
    """What the device mode is for: per-message conversion (the default mode, like the example) is not the conversion of the recording."""
    text, rate, enc, x = _recordings()[4]
    assert (text, rate, enc) == ("8000", 8000, "pcm16")
    sizes = [1280] * (x.nbytes // 1280)                                      # 80 ms messages
    go, got, srv, _ = _serve([(text, x.tobytes(), sizes)], S=2, ingest="host")
    cid = go([6])[0]
    host = np.concatenate(got[cid])
    go, got, srv, _ = _serve([(text, x.tobytes(), sizes)], S=2, ingest="device")
    dev = np.concatenate(got[go([6])[0]])
    assert (dev == _whole(x, rate, enc)).all()
    assert host.shape == dev.shape and (host != dev).any()


def test_a_slot_that_changes_hands_starts_from_silence_in_its_new_class():
    recs = _recordings(3)
    (t48, r48, e48, x48), (tu, ru, eu, xu) = recs[3], recs[0]
    clients = [(t48, x48.tobytes(), _uneven(x48.nbytes, 2, 1)), (tu, xu.tobytes(), _uneven(xu.nbytes, 1, 2)),
               (t48, x48.tobytes(), _uneven(x48.nbytes, 2, 3))]
    go, got, srv, model = _serve(clients, S=1, ingest="device")
    cids = go([3, 3, 3])
    assert (np.concatenate(got[cids[0]]) == _whole(x48, r48, e48)).all()
    assert (np.concatenate(got[cids[1]]) == _whole(xu, ru, eu)).all(), "the mu-law caller inherited the 48 kHz caller's history or class"
    assert (np.concatenate(got[cids[2]]) == _whole(x48, r48, e48)).all()
    c48, cu = srv._class_of[(48000, "pcm16")], srv._class_of[(8000, "ulaw")]
    assert model.engine.assigned == [(0, c48, 0), (0, cu, 0), (0, c48, 0)]    # assigned behind the reset, before the slot's first chunk


def test_rate_messages():
    from aiohttp.test_utils import TestClient, TestServer

    async def ask(srv, text, accepted_as):
        async with TestClient(TestServer(srv.app())) as tc:
            ws = await tc.ws_connect("/ws")
            await ws.receive()
            c = srv.conns[srv._next_cid - 1]
            await ws.send_str(text)
            if accepted_as is None:                                          # refused: the error message, then the close
                msg = await ws.receive()
                await ws.close()
                return json.loads(msg.data).get("error") if isinstance(msg.data, str) else "closed"
            for _ in range(2000):                                            # accepted: the connection carries the format
                if (c.rate, c.enc) == accepted_as:
                    break
                await asyncio.sleep(0.001)
            await ws.close()
            return "accepted" if (c.rate, c.enc) == accepted_as else f"not accepted: {(c.rate, c.enc)}"

    def answer(srv, text):
        w = text.split()
        ok = {"8000 ulaw": (8000, "ulaw"), "8000 alaw": (8000, "alaw"), "44100": (44100, "pcm16"), "8000": (8000, "pcm16")}
        refused = (srv.ingest == "host" and len(w) != 1) or text not in ok or (ok[text][0], ok[text][1]) not in \
            getattr(srv, "_class_of", {(r, "pcm16"): 0 for r in serve.RATES})
        return asyncio.run(asyncio.wait_for(ask(srv, text, None if refused else ok[text]), 30))
    dev = serve.FanInServer(_Model(2), ingest="device")
    assert answer(dev, "8000 ulaw") == "accepted" and answer(dev, "8000 alaw") == "accepted" and answer(dev, "44100") == "accepted"
    for text in ("16000 ulaw", "22051", "8000 mp3", "ulaw", "8000 ulaw x"):
        assert answer(dev, text) == "unsupported sample rate", text
    tel = serve.FanInServer(_Model(2), ingest="device", rates=[(8000, "ulaw"), (8000, "alaw"), 8000])
    assert tel.row_bytes == 1280 and len(tel.classes) == 3
    assert answer(tel, "8000 alaw") == "accepted" and answer(tel, "48000") == "unsupported sample rate"
    host = serve.FanInServer(_Model(2))
    assert host.ingest == "host" and answer(host, "8000 ulaw") == "unsupported sample rate" and answer(host, "8000") == "accepted"
    with pytest.raises(ValueError):
        serve.FanInServer(_Model(2), ingest="gpu")
    with pytest.raises(ValueError):
        serve.FanInServer(_Model(2), ingest="device", rates=[22051])
