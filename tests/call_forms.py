"""Call forms: the same audio in the same call sizes through every public way of running a step (include/owwhip.h: oww_step,
oww_step_masked, oww_submit / oww_submit_masked / oww_collect, oww_step_ingest_mixed, oww_submit_ingest_mixed) on a handle with
every feature switched on.  HIP-free: this module states the scenarios (handle configuration, audio, schedule of calls, mutations
between calls), the table of forms (which call kinds a form expresses itself), the order of submits and collects of the pipelined
forms, what a driver records and when, and the comparison of two traces.  tests/test_call_forms_cpu.py holds the schedule and the
table to their conditions without a GPU; tests/test_call_forms_gpu.py drives every form and holds its trace to the base form's, bit
for bit.

Four scenarios, 70 streams each (two full 32-stream blocks plus six: every stage's and the heads' tiles are ragged; 70 x (9 labels
+ 2 slots) = 770 pairs, 280 in IIe: the event kernels run four, or two, workgroups):

  I    "VAD network"            max_chunks = 1, the on-device VAD network with gate 0.5, one-chunk calls only
  II   "pushed VAD, long calls" max_chunks = 2, a VAD score pushed per stream and call, 2-chunk calls and long calls of 3 and 5 chunks
  III  "mixed ingest"           II with three ingest classes (16 kHz PCM16, 8 kHz mu-law, 48 kHz PCM16) assigned round robin; the input
                                is one message per stream in the stream's own format
  IIe  "in-heads epilogue"      II without the multiclass head: the fixed heads are one narrow group, so post-processing and the ring
                                counters ride in the heads launch of every one-chunk call -- until mutation B assigns verifiers, and
                                again after F has removed them.  (With the multiclass head the fixed heads run as two groups and the
                                epilogue is never taken: scenarios I - III cannot see a bank launch behind it.)

I - III: fixed heads alexa (binary, 64 units), hey_jarvis (a gated pair) and timer (multiclass, 7 columns, 128 units, T = 34: the
wide heads launch; the feature ring has 34 rows).  All of them: a head bank of K = 2 slots and capacity 8
with three heads of 32 / 64 / 128 units and subscriptions that leave slots empty; a verifier pool of 4; events with capacity 32,
4 feature rows and 2 chunks of audio per event; audio rings of 5 chunks."""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Dict, List, Optional

import numpy as np

from openwakeword_amd import resample as R
from openwakeword_amd import weights as W
from openwakeword_amd.engine import CHUNK, EMB_DIM, default_calibration_pcm

S, K = 70, 2
ALL = np.arange(S)
EMB_SEED, HEAD_SEED, VAD_SEED = 3, 1234, 9
FIXED = ["alexa", "hey_jarvis", "timer"]                      # columns 0 | 1 | 2..8
EVENT_CAPACITY, EVENT_FEATURES, AUDIO_CHUNKS, EVENT_AUDIO = 32, 4, 5, 2
BANK_CAPACITY, VERIFIER_CAPACITY = 8, 4
INGEST_CLASSES = [(16000, "pcm16"), (8000, "ulaw"), (48000, "pcm16")]
CLS = (ALL % 3).astype(np.uint8)
WARMUP = 8                                                    # (the first five predictions of a stream are reported as 0)

SCENARIOS = {
    "I": dict(title="VAD network", vad_net=True, max_chunks=1, ingest=False, vad_threshold=0.5),
    "II": dict(title="pushed VAD, long calls", vad_net=False, max_chunks=2, ingest=False, vad_threshold=0.4),
    "III": dict(title="mixed ingest", vad_net=False, max_chunks=2, ingest=True, vad_threshold=0.4),
    "IIe": dict(title="in-heads epilogue", vad_net=False, max_chunks=2, ingest=False, vad_threshold=0.4, heads=FIXED[:2]),
}


def head_names(scenario: str) -> List[str]:
    return SCENARIOS[scenario].get("heads", FIXED)


def n_labels(scenario: str) -> int:
    return sum({"alexa": 1, "hey_jarvis": 1, "timer": 7}[n] for n in head_names(scenario))


def t_ring(scenario: str) -> int:
    """Rows of the feature ring: the longest window of the fixed heads, 16 at least."""
    return max([16] + [{"timer": 34}.get(n, 16) for n in head_names(scenario)])


# ---- the schedule -------------------------------------------------------------------------------------------------------------------------
# Call kinds: u1 = unmasked, one chunk; u2 = unmasked, two chunks (= max_chunks); long = unmasked, more chunks than max_chunks (sliced);
# dense / sparse = a mask of about 70 % / 15 %; wide = all but two to six streams; empty / full = a mask with nobody / everybody on.
# Which launches a HOST mask takes is owl::participants' rule (csrc/owwhip_masked_host.h): more than 7/8 of the streams on
# (8 n > 7 S: 62 of 70) = the full launches, whose stores skip the streams that sit out; fewer = the group lists; nobody = nothing is
# launched.  So sparse AND dense masks take the lists, wide and full masks the full launches, and only a wide mask runs a full launch
# with somebody sitting out.  A mask on the device (form device_mask) always takes the full launches.
KINDS = ("u1", "u2", "long", "dense", "sparse", "wide", "empty", "full")
MASKED = ("dense", "sparse", "wide", "empty", "full")
LIST_MASKS, FULL_LAUNCH_MASKS = ("dense", "sparse"), ("wide", "full")


def takes_full_launches(mask: np.ndarray) -> bool:
    """owl::participants' rule for a host mask, restated."""
    return 8 * int(np.count_nonzero(mask)) > 7 * mask.size


_TEMPLATE = (["u1"] * WARMUP +
             ["dense", "sparse", "sparse", "u2", "long3"] +               # 8 .. 12
             ["u1", "u1", "dense", "empty", "wide", "sparse"] +           # 13 .. 18   (A before 13)
             ["u1", "u1", "sparse", "wide"] +                             # 19 .. 22   (B before 19)
             ["u1", "u1", "dense", "u2", "long5"] +                       # 23 .. 27   (B2 before 23)
             ["u1", "u1", "dense"] +                                      # 28 .. 30   (C before 28)
             ["u1", "u1", "sparse"] +                                     # 31 .. 33   (C2 before 31)
             ["u1", "u1", "sparse", "dense", "u2"] +                      # 34 .. 38   (D before 34)
             ["u1", "u1", "dense", "sparse", "sparse", "long3"] +         # 39 .. 44   (E before 39)
             ["u1", "u1", "wide"] +                                       # 45 .. 47   (F before 45)
             ["u1", "u1", "full", "sparse"])                              # 48 .. 51   (F2 before 48)
_ONE_CHUNK_ONLY = {"u2": "u1", "long3": "dense", "long5": "sparse"}       # scenario I: the VAD network refuses longer calls
# Applied BEFORE the call of that index, pipeline drained.  B, C and F are applied in two parts with two unmasked one-chunk calls in
# between, so that each part invalidates a captured graph on its own: B the per-stream assignments (the verifier list), B2 the
# handle-wide verifier; C set_postproc and the event thresholds, C2 set_vad_threshold; F the handle-wide verifier's removal, F2 the
# removal of every per-stream assignment.
MUTATIONS = {13: "A", 19: "B", 23: "B2", 28: "C", 31: "C2", 34: "D", 39: "E", 45: "F", 48: "F2"}
# state, audio rings and features of every stream are recorded AFTER these calls.  14 and 16 bracket a dense mask (group lists) and the
# empty mask (nothing launched), 16 and 17 a wide mask (full launches whose stores skip): what sat out must have kept every bit
CHECKPOINTS = (14, 16, 17, 33, 44, 51)
SAT_OUT_BRACKETS = ((14, 16), (16, 17))
NO_VAD_PUSH = (15, 16, 17)                                    # (oww_push_vad moves the VAD ring of every stream, masked or not)
N_CALLS = len(_TEMPLATE)

Call = namedtuple("Call", "index kind n_chunks mask first_chunk push_vad")

# mutation D: lists over streams; moves stay inside an ingest class (s % 3) so that scenario III's messages keep their format
RESET_IDS = [21, 34, 47, 60, 69]
MOVE_SRC = [2, 5, 10, 13, 16]                                 # a swap and a 3-cycle
MOVE_DST = [5, 2, 13, 16, 10]
EXPORT_IDS = [6, 7, 8, 9]
IMPORT_IDS = [42, 43, 44, 45]


def _mask(kind: str, index: int) -> Optional[np.ndarray]:
    if kind in ("u1", "u2", "long"):
        return None
    if kind == "empty":
        return np.zeros(S, np.uint8)
    if kind == "full":
        return np.ones(S, np.uint8)
    rng = np.random.default_rng([2024, index])
    if kind == "wide":                                        # stream 1 and one to five others off: 64 .. 68 of 70 on
        on = np.ones(S, np.uint8)
        on[rng.choice(np.arange(2, S), 1 + index % 5, replace=False)] = 0
        on[1] = 0
        return on
    on = (rng.random(S) < (0.7 if kind == "dense" else 0.15)).astype(np.uint8)
    on[0], on[1] = 1, 0                                       # stream 0 in every mask, stream 1 in none
    return on


@functools.lru_cache(maxsize=None)
def schedule(scenario: str) -> List[Call]:
    calls, chunk = [], 0
    for i, k in enumerate(_TEMPLATE):
        if SCENARIOS[scenario]["max_chunks"] == 1:
            k = _ONE_CHUNK_ONLY.get(k, k)
        n = {"u2": 2, "long3": 3, "long5": 5}.get(k, 1)
        kind = "long" if k.startswith("long") else k
        m = _mask(kind, i)
        if m is not None:
            m.setflags(write=False)
        calls.append(Call(i, kind, n, m, chunk, not SCENARIOS[scenario]["vad_net"] and i not in NO_VAD_PUSH))
        chunk += n
    return calls


def n_chunks_total(scenario: str) -> int:
    c = schedule(scenario)[-1]
    return c.first_chunk + c.n_chunks


# ---- the forms --------------------------------------------------------------------------------------------------------------------------
# native: the call kinds the form expresses itself; every other call is made in the base form (step / step_masked on host arrays; in
# scenario III behind ingest_mixed to the host) ON THE FORM'S OWN HANDLE -- the only fallback -- for the reason given.  depth: steps in
# flight of a pipelined form.  exempt: observables not compared, with the sentence of include/owwhip.h that documents the behaviour
# (none today).
Form = namedtuple("Form", "drives native fallback depth scenarios exempt")
_ALL, _GENERAL, _ONLY_III = frozenset(KINDS), ("I", "II", "III", "IIe"), ("III",)
_SUBMIT = frozenset(("u1", "u2") + MASKED)
FORMS: Dict[str, Form] = {
    "host": Form("step / step_masked on host arrays, eager (the base form of scenarios I, II and IIe)", _ALL, "", 0, ("I", "II", "IIe"), {}),
    "graph": Form("use_graph(True): unmasked one-chunk calls replay a captured graph", _ALL, "", 0, _GENERAL, {}),
    "timing": Form("enable_timing(True): every launch between two timing events", _ALL, "", 0, _GENERAL, {}),
    "device": Form("step_device / step_masked_device: PCM and scores on the device, masks on the host", _ALL, "", 0, _GENERAL, {}),
    "device_mask": Form("oww_step_masked with the mask on the device (full launches, no group lists); an unmasked one-chunk call is "
                        "the all-ones mask", frozenset(("u1",) + MASKED), "oww_step_masked takes one chunk", 0, _GENERAL, {}),
    "unaligned": Form("step_device / step_masked_device with the PCM pointer 2 bytes off a 16-byte boundary: the separate mel kernel "
                      "in place of the fused front end, the element-wise audio append", _ALL, "", 0, _GENERAL, {}),
    "pipe1": Form("submit / submit(stream_on=) + collect, one step in flight", _SUBMIT, "oww_submit takes at most max_chunks chunks",
                  1, _GENERAL, {}),
    "pipe2": Form("submit / submit(stream_on=) + collect, two steps in flight wherever two consecutive calls allow it", _SUBMIT,
                  "oww_submit takes at most max_chunks chunks", 2, _GENERAL, {}),
    "own_stream": Form("step / step_masked on a handle created on the caller's HIP stream", _ALL, "", 0, _GENERAL, {}),
    "ingest_host": Form("ingest_mixed to the host, then step / step_masked (the base form of scenario III)", _ALL, "", 0, _ONLY_III, {}),
    "step_ingest": Form("step_ingest_mixed on host rows", _ALL, "", 0, _ONLY_III, {}),
    "submit_ingest1": Form("submit_ingest_mixed + collect, one step in flight", frozenset(("u1",) + MASKED),
                           "oww_submit_ingest_mixed takes one chunk", 1, _ONLY_III, {}),
    "submit_ingest2": Form("submit_ingest_mixed + collect, two steps in flight wherever two consecutive calls allow it",
                           frozenset(("u1",) + MASKED), "oww_submit_ingest_mixed takes one chunk", 2, _ONLY_III, {}),
    "ingest_dev": Form("oww_step_ingest_mixed with the rows already on the device", _ALL, "", 0, _ONLY_III, {}),
}


def base_form(scenario: str) -> str:
    return "ingest_host" if SCENARIOS[scenario]["ingest"] else "host"


def forms_of(scenario: str) -> List[str]:
    """Every form of the scenario but its base form."""
    return [f for f, spec in FORMS.items() if scenario in spec.scenarios and f != base_form(scenario)]


CASES = [(s, f) for s in SCENARIOS for f in forms_of(s)]

# ---- the order of submits and collects ---------------------------------------------------------------------------------------------------
# One Op per call: `native` = the form makes it itself; in_flight = steps in flight when it is submitted (0 for unpipelined forms);
# collects = the calls collected right after it, oldest first (their per-call observables are recorded then); drained = nothing is in
# flight afterwards, so the "last step" getters are read.  A pipeline is drained before a call it cannot express, before a mutation,
# behind a checkpoint call and at the end.
Op = namedtuple("Op", "index native in_flight collects drained")


def plan(scenario: str, form: str) -> List[Op]:
    calls, spec = schedule(scenario), FORMS[form]
    ops, queue = [], []
    for c in calls:
        i = c.index
        native = c.kind in spec.native
        if not native or spec.depth == 0:
            assert not queue
            ops.append(Op(i, native, 0, [i] if native and spec.depth else [], True))
            continue
        in_flight = len(queue)
        queue.append(i)
        collects = []
        if len(queue) == 2:
            collects.append(queue.pop(0))
        more = spec.depth == 2 and i + 1 < len(calls) and calls[i + 1].kind in spec.native and (i + 1) not in MUTATIONS \
            and i not in CHECKPOINTS
        if not more:
            collects += queue
            queue = []
        ops.append(Op(i, True, in_flight, collects, not queue))
    assert not queue
    return ops


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _audio(n_streams: int, T: int, seed: int) -> np.ndarray:
    """int16 [S, T * 1280], distinct per stream, built as tests/test_stream_state_gpu.py::_audio builds it: the shipped speech clips at
    several phases and gains, noise at several levels, clip + noise, and silence.  (A copy, so that this module stays importable
    without the GPU suite; tests/test_call_forms_cpu.py::test_audio_is_the_state_suites holds it to its source.)"""
    rng = np.random.default_rng(seed)
    clips = default_calibration_pcm()
    n = T * CHUNK
    out = np.zeros((n_streams, n), np.int16)
    for s in range(n_streams):
        kind = s % 5
        if kind == 4 and s % 3 == 0:
            continue
        x = np.zeros(n)
        if kind in (0, 2) and clips is not None:
            x += np.roll(np.resize(clips[s % len(clips)].astype(np.float64), n), 97 * s + 13)
        if kind in (1, 2, 3, 4) or clips is None:
            x += rng.standard_normal(n) * (30.0, 300.0, 3000.0, 9000.0)[s % 4]
        out[s] = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return out


def encode_ulaw(x: np.ndarray) -> np.ndarray:
    """int16 -> the G.711 mu-law code whose expansion (resample.decode_ulaw) is nearest."""
    table = R.decode_ulaw(np.arange(256, dtype=np.uint8)).astype(np.int32)
    order = np.argsort(table, kind="stable")
    vals = table[order]
    x = np.asarray(x).astype(np.int32)
    hi = np.clip(np.searchsorted(vals, x), 1, 255)
    pick = np.where(x - vals[hi - 1] <= vals[hi] - x, hi - 1, hi)
    return order[pick].astype(np.uint8)


JUNK16 = np.int16(0x5A5B)                                     # rows of streams that sit out: never read


@functools.lru_cache(maxsize=None)
def scenario_data(scenario: str) -> dict:
    """Everything a driver feeds: per call `pcm` int16 [S, n * 1280] (scenarios I, II) or `rows` uint8 [S, row_bytes] (III) with junk in
    the rows of streams that sit out, `vad` float32 [n_calls, S] (pushed scores either side of the gate), the parameters of the
    mutations.  Read-only and shared by every driver."""
    cfg, calls = SCENARIOS[scenario], schedule(scenario)
    T = n_chunks_total(scenario)
    x16 = _audio(S, T, seed=100 + len(scenario))
    d = {"pcm": [], "rows": [], "vad": np.random.default_rng(77).random((N_CALLS, S)).astype(np.float32)}
    if cfg["ingest"]:
        own = []
        for s in range(S):
            if CLS[s] == 0:
                own.append(x16[s])
            elif CLS[s] == 1:
                own.append(encode_ulaw(x16[s][::2]))
            else:
                own.append(np.repeat(x16[s], 3))
    for c in calls:
        on = np.ones(S, bool) if c.mask is None else c.mask != 0
        a, b = c.first_chunk * CHUNK, (c.first_chunk + c.n_chunks) * CHUNK
        if cfg["ingest"]:
            n_out = c.n_chunks * CHUNK
            arrs = []
            for s in range(S):
                per = R.class_n_in(INGEST_CLASSES[CLS[s]][0], CHUNK)
                arrs.append(own[s][c.first_chunk * per:(c.first_chunk + c.n_chunks) * per] if on[s] else None)
            out = np.full((S, R.class_row_bytes(INGEST_CLASSES, n_out)), 0xA5, np.uint8)
            rows = R.pack_ingest_rows(arrs, CLS, INGEST_CLASSES, n_out, out)
            rows.setflags(write=False)
            d["rows"].append(rows)
        else:
            pcm = np.ascontiguousarray(x16[:, a:b])
            pcm[~on] = JUNK16
            pcm.setflags(write=False)
            d["pcm"].append(pcm)
    rng = np.random.default_rng(5)
    d["verifier_w"] = [rng.normal(0.0, 0.05, 16 * EMB_DIM).astype(np.float32) for _ in range(3)]
    d["verifier_b"] = [0.1, -0.2, 0.05]
    d["init_features"] = rng.normal(0.0, 1.0, (t_ring(scenario), EMB_DIM)).astype(np.float32)
    clips = _audio(8, 13, seed=78)[:, :512 + 75 * 160 + 8 * 160 * 3]       # 8 clips of four embedding windows
    d["clips"] = np.ascontiguousarray(clips)
    d["dense_feats"] = rng.normal(0.0, 1.0, (2, 40, EMB_DIM)).astype(np.float32)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- heads, bank and subscriptions -----------------------------------------------------------------------------------------------------------
def fixed_heads(scenario: str) -> dict:
    """alexa (binary), hey_jarvis (gated pair), timer (multiclass): the catalogue shapes at the seed whose output biases are centred
    (weights._LOGIT_CENTRE_SEED1234), as tests/test_events_gpu.py uses them."""
    return {n: W.synthetic_head(n, HEAD_SEED) for n in head_names(scenario)}


def bank_head(i: int, seed: int = 100) -> dict:
    """tests/test_head_bank_gpu.py::_random_bank's recipe: 32 / 64 / 128 units, LayerNorm on and off, the output bias shifted so that
    scores fall either side of 0.5."""
    h = W.synthetic_head(f"bank{i}", seed + i, hidden=(32, 64, 128)[i % 3], layernorm=bool(i % 2), T=16)
    h["net"]["b3"] = (h["net"]["b3"] - np.float32(4.0)).astype(np.float32)
    return h


def subscriptions() -> np.ndarray:
    """int32 [S, K]: heads 0..2, about a third of the slots empty, streams 3 and 68 with both slots empty, stream 0 with both taken."""
    sub = np.random.default_rng(3).integers(-1, 3, size=(S, K)).astype(np.int32)
    sub[0], sub[3], sub[68] = [0, 2], [-1, -1], [-1, -1]
    return sub


RESUBSCRIBED = ALL[2::4]                                      # mutation A: a quarter of the streams
NEW_HEAD_IDS = ALL[3::8]                                      # ... and who takes the new head into slot 1


def resubscriptions() -> np.ndarray:
    new = np.random.default_rng(4).integers(-1, 3, size=(RESUBSCRIBED.size, K)).astype(np.int32)
    new[new == 1] = 0                                         # (head 1 is removed right after)
    return new


VAD_BIAS_SHIFT = -3.0


def vad_weights() -> dict:
    """The VAD stand-in's random weights with the decoder bias shifted by VAD_BIAS_SHIFT: on this audio the float64 oracle
    (oracle/vad_standin.py) puts the unshifted network's scores between 0.56 and 0.99 with a median logit of 3.0, which no gate at 0.5
    ever closes; shifted, the median score is 0.51 and about a quarter of the (stream, call) pairs fall below the gate for three calls
    running.  The same conditioning weights.synthetic_head applies to the heads' output biases."""
    vad = dict(W.synthetic_vad(seed=VAD_SEED))
    wd, bd = vad["dec"]
    vad["dec"] = (wd, float(bd) + VAD_BIAS_SHIFT)
    return vad


def engine_kwargs(scenario: str) -> dict:
    cfg = SCENARIOS[scenario]
    kw = dict(max_chunks=cfg["max_chunks"], vad_threshold=cfg["vad_threshold"], bank_slots=K, bank_capacity=BANK_CAPACITY,
              verifier_capacity=VERIFIER_CAPACITY, event_capacity=EVENT_CAPACITY, event_features=EVENT_FEATURES,
              audio_chunks=AUDIO_CHUNKS, event_audio=EVENT_AUDIO)
    if cfg["vad_net"]:
        kw["vad"] = vad_weights()
    return kw


def configure(e, scenario: str, cal: Optional[dict]) -> None:
    """What every driver does to its fresh handle.  cal: the thresholds of calibrate() (None: the calibration run itself)."""
    for i in range(3):
        assert e.bank_add(bank_head(i)) == i
    e.bank_set_postproc(0, 2, 0.3)
    e.subscribe(ALL, subscriptions())
    if SCENARIOS[scenario]["ingest"]:
        e.configure_ingest_classes(INGEST_CLASSES)
        e.assign_ingest(ALL, CLS)
    if cal is not None:
        e.set_event_thresholds(fixed=cal["event_fixed"][0], bank=cal["event_bank"][0])


def mutate(e, scenario: str, tag: str, cal: dict) -> Dict[str, np.ndarray]:
    """Mutation `tag` on a drained handle; returns what it read (compared like every other observable)."""
    d, out = scenario_data(scenario), {}
    if tag == "A":
        e.subscribe(RESUBSCRIBED, resubscriptions())
        e.bank_remove(1)
        assert e.bank_add(bank_head(7)) == 1, "the new head does not take the freed id"
        e.subscribe(NEW_HEAD_IDS, current_subscriptions()[NEW_HEAD_IDS])
    elif tag == "B":
        v = [e.verifier_add(d["verifier_w"][i], d["verifier_b"][i]) for i in range(2)]
        ids = ALL[0::3]
        e.assign_verifiers(0, ids, [v[i % 2] for i in range(ids.size)], np.zeros(ids.size, np.float32))
        ids = np.array([s for s in ALL[1::2] if current_subscriptions()[s, 0] >= 0], np.int32)   # (a pool verifier needs a taken slot)
        e.assign_verifiers(0, ids, [v[(i + 1) % 2] for i in range(ids.size)], np.zeros(ids.size, np.float32), bank=True)
    elif tag == "B2":
        e.set_verifier(1, d["verifier_w"][2], d["verifier_b"][2], threshold=0.05)
    elif tag == "C":
        e.set_postproc([2] + [0] * (n_labels(scenario) - 1), cal["postproc"], 2)
        e.set_event_thresholds(fixed=cal["event_fixed"][1], bank=cal["event_bank"][1])
    elif tag == "C2":
        if not SCENARIOS[scenario]["vad_net"]:               # (scenario I: the gate of the VAD network stays at 0.5)
            e.set_vad_threshold(0.6)
    elif tag == "D":
        e.reset(RESET_IDS, d["init_features"])
        e.move_streams(MOVE_SRC, MOVE_DST)
        e.import_state(IMPORT_IDS, e.export_state(EXPORT_IDS))
    elif tag == "E":
        out["embed_clips"] = e.embed_clips(d["clips"])
        out["score_features"] = e.score_features(d["dense_feats"])
        st = e.bank_score_stats(d["dense_feats"], [0, 2, 1])
        out.update({f"bank_score_stats.{k}": v for k, v in st.items()})
    elif tag == "F":
        e.set_verifier(1, None)
    elif tag == "F2":
        for bank in (False, True):
            for col in range(K if bank else n_labels(scenario)):
                e.assign_verifiers(col, ALL, np.full(S, -1, np.int32), np.zeros(S, np.float32), bank=bank)
    else:
        raise ValueError(tag)
    return out


def current_subscriptions() -> np.ndarray:
    """The subscription table after mutation A and before D (which moves streams), restated on the host."""
    # (mutation A leaves this table; B assigns bank verifiers by it)
    sub = subscriptions()
    sub[RESUBSCRIBED] = resubscriptions()
    sub[sub == 1] = -1                                        # bank_remove(1) empties its slots
    sub[NEW_HEAD_IDS, 1] = 1
    return sub


def calibrate(scores: np.ndarray, bank_scores: np.ndarray) -> dict:
    """Thresholds from the base form's own scores over the calls before the first mutation (warm-up excluded), the way
    tests/test_events_gpu.py takes its thresholds from its twin: per column quantiles of the nonzero scores, high enough that a call
    reports a few dozen of its 770 pairs, so that capacity 32 overflows in some calls and not in others."""
    def q(v, p, default):
        v = v[v != 0]
        return np.float32(np.quantile(v, p)) if v.size else np.float32(default)
    fixed = [np.array([q(scores[..., c], p, 0.5) for c in range(scores.shape[-1])], np.float32) for p in (0.95, 0.92)]
    bank = [float(q(bank_scores, p, 0.5)) for p in (0.85, 0.8)]
    post = np.array([q(scores[..., c], 0.5, 0.5) for c in range(scores.shape[-1])], np.float32)
    return {"event_fixed": fixed, "event_bank": bank, "postproc": post}


# ---- the trace -----------------------------------------------------------------------------------------------------------------------------
# trace["call"][i]:       scores, events (record bytes [n, 32]), n_total, event_streams (int32 [n]), event_features, event_audio
# trace["drained"][i]:    bank_scores, raw, vad (scenario I), verifier_stats           -- only where plan()[i].drained
# trace["checkpoint"][i]: state, audio, audio_counts, features                         -- i in CHECKPOINTS
# trace["mutation"][i]:   what mutate() returned                                       -- i in MUTATIONS
PER_CALL = ("scores", "events", "n_total", "event_features", "event_audio")
DRAINED = ("bank_scores", "raw", "vad", "verifier_stats")
CHECKPOINT = ("state", "audio", "audio_counts", "features")


def new_trace() -> dict:
    return {"call": {}, "drained": {}, "checkpoint": {}, "mutation": {}}


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _differing_streams(name: str, a: np.ndarray, b: np.ndarray, rec_a: dict) -> str:
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    if a.ndim == 0 or a.shape[0] == 0:
        return f"{a.tolist()} and {b.tolist()}"
    rows = np.flatnonzero((_bits(a) != _bits(b)).reshape(a.shape[0], -1).any(axis=1))
    if a.shape[0] == S:
        return f"{rows.size} streams differ, first {rows[:6].tolist()}"
    if name.startswith("event") and "event_streams" in rec_a and len(rec_a["event_streams"]) == a.shape[0]:
        return f"{rows.size} records differ, first {rows[:6].tolist()} (streams {rec_a['event_streams'][rows[:6]].tolist()})"
    return f"{rows.size} rows differ, first {rows[:6].tolist()}"


def compare(base: dict, got: dict, form: str) -> List[str]:
    """Every observable `got` holds against the base trace, on bits.  Returns one line per difference: where (call index), what, and the
    first differing streams.  Nothing `got` recorded is skipped but the observables the form table exempts."""
    exempt = FORMS[form].exempt
    diffs, n = [], 0
    for section in ("call", "drained", "checkpoint", "mutation"):
        for i in sorted(got[section]):
            assert i in base[section], f"the base trace has no {section} record of call {i}"
            assert set(got[section][i]) == set(base[section][i]), \
                f"call {i}, {section}: recorded {sorted(got[section][i])}, the base form {sorted(base[section][i])}"
            for name, g in got[section][i].items():
                if name == "event_streams" or name in exempt:
                    continue
                w = base[section][i][name]
                g, w = np.asarray(g), np.asarray(w)
                n += 1
                if g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
                    where = f"before call {i} (mutation {MUTATIONS[i]})" if section == "mutation" else f"call {i}"
                    diffs.append(f"{where}, {name}: {_differing_streams(name, w, g, base[section][i])}")
    got["n_compared"] = n
    return diffs
