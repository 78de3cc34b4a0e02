"""The three launch sites of Model.predict's post-processing (csrc/owwhip_postproc.h) -- owk::postproc_kernel, the epilogue of
owh::heads_hx_kernel and owh::bank_post_kernel -- held to tests/postproc_ref.py's reference_rules BIT FOR BIT (np.array_equal on uint32 views).

Method.  A twin handle runs the identical call sequence (audio, resets, masks, subscriptions, chunk counts) with no rules and no gate.
Heads, verifier and post-processing never feed back into raw scores, so the twin's raw table is the subject's (read from the subject
with oww_get_raw after every call, and compared).  Thresholds are then picked from that table as actual elements of it, the same value
moved one float32 step up and down on other labels, so that score == threshold really occurs; the expected output is reference_rules on
the device's own raw table.  After each run every applicable fault of the catalogue is applied to the measured table on the CPU and
must move at least one final score of that run: a run in which a `>` for a `>=` could not have shown proves nothing.  The counts are
printed (DESIGN.md 5.25 records them); only "at least one" is asserted.

Audio: fixture clips, noise at several levels with loud and quiet segments, silence, and streams whose audio repeats with the period
of a call -- their raw scores settle to a constant, so a threshold picked on it meets equality call after call.  Every head's output
bias is re-centred on the median logit of a first pass (synthetic heads otherwise pin near 0 or 1)."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

import postproc_ref as P
from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine, default_calibration_pcm

pytestmark = pytest.mark.gpu

F32 = np.float32
S_BIG = 37                       # one full 32-stream wave and a partly filled one
EMB_SEED = 3
BINARY = ["alexa", "hey_mycroft", "hey_jarvis", "hey_rhasspy", "weather"]
THREE = BINARY[:3]
N_CHUNKS = 100                   # (the longest schedule: 70 calls, eighteen of them of two chunks, behind the timed prefix)
LOGIT_DOWN = 64.0


def _audio(S, n_chunks=N_CHUNKS, seed=17):
    """int16 [S, n_chunks * 1280], distinct per stream and moving in time: the fixture clips at several phases under a loud / quiet
    envelope, noise at several levels in segments, clip + noise, noise bursts between silence, digital silence, and (every fifth
    stream) sums of harmonics of 12.5 Hz -- one period per call -- in long blocks or in an order that repeats every seven calls."""
    rng = np.random.default_rng(seed)
    clips = default_calibration_pcm()
    n = n_chunks * 1280
    t = np.arange(n)
    seg = (t // (1280 * 6)) % 4                                        # six-call segments
    out = np.zeros((S, n), np.int16)

    def periodic(k):
        r = np.random.default_rng(1000 + k)
        x = np.zeros(1280)
        for m in r.choice(np.arange(8, 300), 6, replace=False):
            x += r.uniform(300.0, 2500.0) * np.sin(2 * np.pi * m * np.arange(1280) / 1280 + r.uniform(0, 6.28))
        return np.tile(x, n_chunks)

    block = t // 1280
    for s in range(S):
        kind = s % 5
        x = np.zeros(n)
        if s % 15 == 9:
            pass                                                       # digital silence
        elif kind == 4 and s % 10 == 4:
            # three one-call waveforms (one of them faint) in a fixed order that repeats every seven calls: the scores move, and repeat
            waves = np.stack([periodic(3 * s)[:1280], 0.02 * periodic(3 * s + 1)[:1280], periodic(3 * s + 2)[:1280]])
            order = np.array([0, 2, 0, 1, 1, 2, 0])[(np.arange(n_chunks) + s) % 7]
            x = waves[order].ravel()
        elif kind == 4:
            x = np.where((block < 34) | (block >= 56), periodic(3 * s), periodic(3 * s + 1))
        else:
            if kind in (0, 2) and clips is not None:
                x += np.roll(np.resize(clips[s % len(clips)].astype(np.float64), n), 97 * s + 13) * np.array([1.0, 0.15, 0.6, 0.03])[seg]
            if kind in (1, 2) or clips is None:
                x += rng.standard_normal(n) * (30.0, 300.0, 3000.0, 9000.0)[s % 4] * np.array([1.0, 0.1, 3.0, 0.5])[(seg + s) % 4]
            if kind == 3:
                x += rng.standard_normal(n) * 4000.0 * (((t // (1280 * 3)) + s) % 3 == 0)
        out[s] = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return out


def _raw(e):
    out = np.empty((e.n_streams, e.n_labels), F32)
    _lib.check(e._lib.oww_get_raw(e._h, out.ctypes.data_as(C.c_void_p)))
    return out


def _emb():
    return W.synthetic_embedding(seed=EMB_SEED)


def _bank_heads():
    return {"narrow": W.synthetic_head("bank_narrow", 21, hidden=64, layernorm=True),
            "wide": W.synthetic_head("bank_wide", 22, hidden=128, layernorm=False)}


@pytest.fixture(scope="module")
def centred():
    """{"heads": {name: head}, "features": [S, 16, 96]}: the binary heads of the default family and the two bank heads with every
    net's output bias moved by minus its median logit over one pass of the S = 37 audio.  The logits are read from copies of the nets
    whose output layer is scaled down by 64 (their sigmoid does not saturate): z = 64 logit(p)."""
    heads = {n: W.synthetic_head(n, seed=11 + i) for i, n in enumerate(BINARY)}
    heads.update(_bank_heads())
    nets = {}
    for name, h in heads.items():
        nets[name] = h["net"]
        if h["kind"] == "gated":
            nets[name + "#2"] = h["net2"]
    probes = {}
    for key, net in nets.items():
        m = copy.deepcopy(net)
        m["w3"] = (m["w3"] / F32(LOGIT_DOWN)).astype(F32)
        m["b3"] = np.zeros_like(m["b3"])
        probes[key] = {"kind": "binary", "T": 16, "hidden": int(net["w1"].shape[1]), "n_out": 1, "net": m}
    pcm = _audio(S_BIG)
    eng = StreamEngine(S_BIG, probes, _emb(), max_chunks=2)
    try:
        p = np.stack([eng.step_raw(pcm[:, 1280 * c:1280 * (c + 1)]) for c in range(60)]).astype(np.float64)
        feats = np.stack([eng.get_features(s, 16) for s in range(S_BIG)])
    finally:
        eng.close()
    p = np.clip(p[8:], 1e-6, 1 - 1e-6)
    z = LOGIT_DOWN * np.log(p / (1 - p))
    for i, key in enumerate(nets):
        nets[key]["b3"] = (nets[key]["b3"] - F32(np.median(z[:, :, i]))).astype(F32)
    return {"heads": heads, "features": feats}


def _verifier(centred):
    """(w [16 * 96], bias): a folded verifier whose logit has a spread of 2 and median 0 over the fixture's feature windows."""
    w = np.random.default_rng(8).standard_normal(16 * 96)
    z = centred["features"].reshape(S_BIG, -1).astype(np.float64) @ w
    w *= 2.0 / max(z.std(), 1e-9)
    return w.astype(F32), float(-np.median(z) * 2.0 / max(z.std(), 1e-9))


# ---------------------------------------------------------------------------------------------------------------------------
def _drive(eng, sched, pcm, rules, bank_ids=(), first_chunk=0):
    """The schedule on one handle -> {"scores", "raw" [C, S, NL], "bank" [C, S, K]}.  rules = False: the twin (no set_postproc, no
    bank_set_postproc, no gate)."""
    Cn, S = sched.n_calls, sched.S
    out = {"scores": np.zeros((Cn, S, eng.n_labels), F32), "raw": np.zeros((Cn, S, eng.n_labels), F32), "bank": np.zeros((Cn, S, sched.K), F32)}
    cur, c = np.full(S, first_chunk), 0               # a stream that sits a call out keeps its audio for its next call
    for op in sched.ops:
        if op[0] == "post":
            if rules:
                eng.set_postproc(op[1], op[2], op[3])
        elif op[0] == "bank_post":
            if rules:
                eng.bank_set_postproc(bank_ids[op[1]], op[2], float(op[3]))
        elif op[0] == "gate":
            if rules:
                eng.set_vad_threshold(float(op[1]))
        elif op[0] == "vad":
            eng.push_vad(op[1])
        elif op[0] == "reset":
            eng.reset(op[1])
        elif op[0] == "reset_vad":
            eng.reset_vad(op[1])
        elif op[0] == "sub":
            eng.subscribe(op[1], np.where(op[2] < 0, -1, np.asarray(bank_ids)[np.maximum(op[2], 0)]))
        else:
            k, on = op[1], op[2]
            x = np.stack([pcm[i, 1280 * cur[i]:1280 * (cur[i] + k)] for i in range(S)])
            cur += k * (np.ones(S, int) if on is None else np.asarray(on, int))
            out["scores"][c] = eng.step(x) if on is None else eng.step_masked(x, on)
            out["raw"][c] = _raw(eng)
            if sched.K:
                out["bank"][c] = eng.bank_scores()
            c += 1
    return out


PREFIX_CHUNKS = 7


def _prefix(eng, pcm, shapes, want):
    """A short timed prefix: one call of each shape the schedule uses -> asserts the post-processing launches each took (0 = the rules
    ran inside the heads launch), then puts every stream back to its start-up state."""
    S = eng.n_streams
    eng.enable_timing(True)
    cur = 0
    for shape in shapes:
        k = shape if isinstance(shape, int) else 1
        before = eng.kernel_times()["postproc"]["launches"]
        x = np.ascontiguousarray(pcm[:, 1280 * cur:1280 * (cur + k)])
        cur += k
        if shape == "masked":
            eng.step_masked(x, np.arange(S) % 3 != 1)
        else:
            eng.step(x)
        assert eng.kernel_times()["postproc"]["launches"] - before == want[shape], (shape, want)
    assert cur <= PREFIX_CHUNKS
    eng.enable_timing(False)
    eng.reset()
    eng.reset_vad()


def _shapes(sched):
    out = []
    for op in sched.calls:
        shape = "masked" if op[2] is not None else op[1]
        if shape not in out:
            out.append(shape)
    return out


def _same(a, b, what):
    a, b = P.bits(a), P.bits(b)
    assert a.shape == b.shape, what
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} differ, first at (call, stream, column) {bad[0].tolist()}")


def _report(path, S, counts):
    print("POSTPROC_COUNTS " + json.dumps({"path": path, "S": S, "moved": counts}))
    silent = [f for f, n in counts.items() if n == 0]
    assert not silent, f"{path}, S = {S}: the run could not have shown {silent}"


SINGLE_ROWS = (4, 0, 14, 2, 19, 1, 34, 3, 29, 5, 7, 6)     # rows of the S = 37 audio an S = 1 handle is run on, one pass each


def _single_stream(path, one_pass):
    """S = 1: one stream's 70 calls cannot show every fault at once, so the handle is run on one row of the audio after the other
    (one_pass(pcm [1, n]) -> {fault: scores moved}; every pass is compared exactly) until the passes together have shown them all."""
    pcm, total = _audio(S_BIG), {}
    for row in SINGLE_ROWS:
        for f, n in one_pass(pcm[row:row + 1]).items():
            total[f] = total.get(f, 0) + n
        if all(n > 0 for n in total.values()):
            break
    _report(path, 1, total)


def _check_fixed(path, S, make, launches, pcm=None, before=None, report=True):
    """Twin pass -> thresholds -> subject pass -> exact comparison and the no-vacuity condition, for a handle with fixed heads only.
    make() -> a fresh handle; before(eng): what both handles get before the first call (a verifier); launches: post-processing launches
    per call shape."""
    pcm = _audio(S) if pcm is None else pcm
    kw = P.PATHS[path]
    plain = P.make_schedule(S, **kw)
    twin = make()
    try:
        if before:
            before(twin)
        table = _drive(twin, plain, pcm, rules=False, first_chunk=PREFIX_CHUNKS)["raw"]
        feats_twin = [twin.get_features(s, 16) for s in (0, S - 1)]
    finally:
        twin.close()
    sched, want, counts = P.choose_schedule(lambda pick, seed: P.make_schedule(S, pick=pick, vad_seed=seed, **kw), table,
                                            tries=4 if S > 1 else 2)
    eng = make()
    try:
        if before:
            before(eng)
        _prefix(eng, pcm, _shapes(sched), launches)
        got = _drive(eng, sched, pcm, rules=True, first_chunk=PREFIX_CHUNKS)
        feats = [eng.get_features(s, 16) for s in (0, S - 1)]
    finally:
        eng.close()
    on = np.stack([np.ones(S, bool) if op[2] is None else np.asarray(op[2], bool) for op in sched.calls])
    _same(got["raw"][on], table[on], f"{path}: raw scores of the subject and of its rule-free twin")
    _same(got["scores"], want["scores"], f"{path}: final scores against reference_rules")
    assert (got["scores"] != 0).any() or S == 1
    if report:
        _report(path, S, counts)
    return got, want, sched, (feats, feats_twin), counts


def _fixed_engine(names, centred, S, family=3, **kw):
    heads = {n: centred["heads"][n] for n in names}
    return lambda: StreamEngine(S, heads, _emb(), max_chunks=2, use_mfma=family, **kw)


KERNEL = {1: 1, 2: 1, 3: 1, "masked": 1}
EPILOGUE = {1: 0, "masked": 0}


# ---- 1. the epilogue of heads_hx_kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [S_BIG, 1])
def test_epilogue_of_the_heads_launch(centred, S):
    """Default family, alexa + hey_mycroft + the gated hey_jarvis, one-chunk calls (masked ones among them)."""
    make = _fixed_engine(THREE, centred, S)
    if S == 1:
        _single_stream("epilogue", lambda pcm: _check_fixed("epilogue", 1, make, EPILOGUE, pcm, report=False)[4])
    else:
        _check_fixed("epilogue", S, make, EPILOGUE)


# ---- 2. owk::postproc_kernel, four ways -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [1, 0])
def test_postproc_kernel_of_the_other_families(centred, family):
    _check_fixed(f"family{family}", S_BIG, _fixed_engine(THREE, centred, S_BIG, family=family), KERNEL)


def test_postproc_kernel_with_the_six_default_models(centred):
    """12 labels in several head groups: the five binary models and `timer` (seven outputs, T = 34)."""
    heads = {n: centred["heads"][n] for n in BINARY}
    heads["timer"] = W.synthetic_head("timer", seed=19)
    _check_fixed("default6", S_BIG, lambda: StreamEngine(S_BIG, heads, _emb(), max_chunks=2), KERNEL)


@pytest.mark.parametrize("S", [S_BIG, 1])
def test_postproc_kernel_on_multi_chunk_and_long_calls(centred, S):
    """The flagship handle leaves the epilogue for every call of two chunks and of three (longer than max_chunks: the sliced form)."""
    make, launches = _fixed_engine(THREE, centred, S), {1: 0, 2: 1, 3: 1, "masked": 0}
    if S == 1:
        _single_stream("long", lambda pcm: _check_fixed("long", 1, make, launches, pcm, report=False)[4])
    else:
        _check_fixed("long", S, make, launches)


def test_postproc_kernel_behind_a_verifier(centred):
    """A handle-wide verifier on hey_mycroft: oww_get_raw returns the re-scored value, and the ring keeps it."""
    w, b = _verifier(centred)
    got, _, sched, _, _ = _check_fixed("verifier", S_BIG, _fixed_engine(THREE, centred, S_BIG), KERNEL,
                                    before=lambda e: e.set_verifier(1, w, b, 0.5))
    plain = _fixed_engine(THREE, centred, S_BIG)()
    try:
        base = _drive(plain, sched, _audio(S_BIG), rules=False, first_chunk=PREFIX_CHUNKS)["raw"]
    finally:
        plain.close()
    on = np.stack([np.ones(S_BIG, bool) if op[2] is None else np.asarray(op[2], bool) for op in sched.calls])
    hit = base[..., 1] >= F32(0.5)
    assert hit[on].any() and (~hit)[on].any()
    assert (got["raw"][..., 1] != base[..., 1])[on & hit].mean() > 0.9            # re-scored where the head reached the threshold ...
    _same(got["raw"][..., 1][on & ~hit], base[..., 1][on & ~hit], "below the verifier threshold the head's score stays")
    _same(got["raw"][..., 0][on], base[..., 0][on], "labels without a verifier")


# ---- 3. one handle between the two copies ---------------------------------------------------------------------------------------
def test_handover_between_epilogue_and_kernel(centred):
    """One-chunk, two-chunk and masked calls interleaved by a fixed pattern: ring, count and nfeat pass between the epilogue and
    postproc_kernel + advance_kernel with no seam; the feature ring ends where the twin's does."""
    _, _, _, (feats, feats_twin), _ = _check_fixed("handover", S_BIG, _fixed_engine(THREE, centred, S_BIG), {1: 0, 2: 1, "masked": 0})
    for a, b in zip(feats, feats_twin):
        _same(a, b, "get_features of subject and twin")


# ---- 4. owh::bank_post_kernel ---------------------------------------------------------------------------------------------------
def _bank_pass(centred, S, pcm):
    """One twin + subject pass of the bank path -> {fault: scores moved}."""
    kw = P.PATHS["bank"]
    bank = [centred["heads"]["narrow"], centred["heads"]["wide"]]
    fixed = {"alexa": centred["heads"]["alexa"]}
    plain = P.make_schedule(S, **kw)
    twin = StreamEngine(S, {**fixed, "narrow": bank[0], "wide": bank[1]}, _emb(), max_chunks=2, bank_slots=3, bank_capacity=4)
    try:
        ids = [twin.bank_add(h) for h in bank]
        t = _drive(twin, plain, pcm, rules=False, bank_ids=ids, first_chunk=PREFIX_CHUNKS)
    finally:
        twin.close()
    raw, head_raw = t["raw"][..., :1], t["raw"][..., 1:]
    free = P.reference_rules(plain.without_rules(), raw, head_raw)    # (no rules, no gate: first-five zeroing only)
    seen = free["bank_count"] >= 5
    assert seen.any()
    _same(t["bank"][seen], free["bank"][seen], "the twin's bank_scores against the same nets as fixed heads")
    sched, want, counts = P.choose_schedule(lambda pick, seed: P.make_schedule(S, pick=pick, vad_seed=seed, **kw), raw, head_raw,
                                            tries=4 if S > 1 else 2)
    eng = StreamEngine(S, fixed, _emb(), max_chunks=2, bank_slots=3, bank_capacity=4)
    try:
        ids = [eng.bank_add(h) for h in bank]
        _prefix(eng, pcm, _shapes(sched), {1: 0, 2: 1, "masked": 0})           # (nothing subscribed yet: the fixed head's launches only)
        eng.subscribe(np.arange(S), np.tile(np.array([ids[0], -1, -1], np.int32), (S, 1)))
        eng.enable_timing(True)
        before = eng.kernel_times()["postproc"]["launches"]
        eng.step(pcm[:, :1280])
        assert eng.kernel_times()["postproc"]["launches"] - before == 1         # bank_post_kernel; the fixed head stays on the epilogue
        eng.enable_timing(False)
        eng.subscribe(np.arange(S), np.full((S, 3), -1, np.int32))
        eng.reset()
        eng.reset_vad()
        got = _drive(eng, sched, pcm, rules=True, bank_ids=ids, first_chunk=PREFIX_CHUNKS)
    finally:
        eng.close()
    on = np.stack([np.ones(S, bool) if op[2] is None else np.asarray(op[2], bool) for op in sched.calls])
    _same(got["raw"][on], raw[on], "bank: fixed raw scores of the subject and of its twin")
    _same(got["scores"], want["scores"], "bank: the fixed label's final scores against reference_rules")
    _same(got["bank"], want["bank"], "bank: slot scores against reference_rules")
    assert (got["bank"] != 0).any() or S == 1
    return counts


@pytest.mark.parametrize("S", [S_BIG, 1])
def test_bank_post_kernel(centred, S):
    """K = 3 slots over a narrow (64-unit) and a wide (128-unit) bank head, empty slots, per-head rules changed twice, subscriptions
    changed at two points (one slot of each touched stream keeps its head and its ring), masked and two-chunk calls, the stream's gate.
    The twin carries the two bank heads as fixed heads too: their raw scores are the slots' raw scores at every call, the five hidden
    ones after a (re)start included, and its own bank_scores confirm them wherever a slot's count is at least 5."""
    if S == 1:
        _single_stream("bank", lambda pcm: _bank_pass(centred, 1, pcm))
    else:
        _report("bank", S, _bank_pass(centred, S, _audio(S)))


# ---- 5. graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replay_of_the_epilogue(centred):
    """oww_use_graph on the flagship path with set_postproc and set_vad_threshold changed between replays (both are baked into the
    captured launch): identical to the eager run of the same sequence and to reference_rules."""
    make = _fixed_engine(THREE, centred, S_BIG)
    got, want, sched, _, _ = _check_fixed("graph", S_BIG, make, EPILOGUE)
    eng = make()
    try:
        eng.use_graph(True)
        replay = _drive(eng, sched, _audio(S_BIG), rules=True, first_chunk=PREFIX_CHUNKS)
    finally:
        eng.close()
    _same(replay["raw"], got["raw"], "graph replay: raw scores")
    _same(replay["scores"], got["scores"], "graph replay against the eager run")
    _same(replay["scores"], want["scores"], "graph replay against reference_rules")
