"""A scratch buffer that grew, or did not grow, on an earlier call must not change a later result.

The host layer keeps grow-on-demand scratch behind `reset`, `reset_vad`, a host-fed `step` longer than `max_chunks`, `embed_clips`,
`resample`, masked steps, `subscribe`, `export_state` / `import_state` and `ingest`.  Every case below calls one of them three times
with small -> larger -> small arguments on handle A and, after each call, compares what came back BIT FOR BIT with a handle of the same
configuration that meets that size first: Rs only ever sees the small arguments (calls 1 and 3), Rl only the larger ones (call 2).
Before a call the reference takes over A's whole stream state (`export_state` -> `import_state` of every stream, which the state
suite holds to bit-exact continuation), so both have the same stream history; after it both take one ordinary one-chunk step with a
VAD score per stream, and scores, bank scores, events, event features and the state records of every stream must be equal as well.
The kernels are deterministic and batch invariant (asserted bit-exactly elsewhere), so equality is the condition: no tolerance.

Configuration: 33 streams (the smallest count with a padded tail and a second 32-stream group), max_chunks = 2, three fixed heads,
a per-stream verifier pool of 2 with one verifier assigned, events with snapshots, the VAD gate, 8 kHz mu-law ingest and, in the
f16-split family (use_mfma = 3), a head bank of K = 2 slots and capacity 4; the exact-fp32 family (1) has no bank and skips nothing
else."""
import numpy as np
import pytest

from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine
from test_stream_state_gpu import _audio, _eq, _heads

pytestmark = pytest.mark.gpu

S, K, WARM = 33, 2, 6                            # (six warm-up steps: the first five predictions of a stream are reported as 0)
ALL = np.arange(S)
FAMILIES = [3, 1]


def _handle(family, subscribed=True):
    bank = family == 3
    e = StreamEngine(S, _heads(), W.synthetic_embedding(seed=3), use_mfma=family, max_chunks=2, vad_threshold=0.4,
                     bank_slots=K if bank else 0, bank_capacity=4 if bank else 0, verifier_capacity=2, event_capacity=64, event_features=2)
    e.configure_ingest(8000, "ulaw")
    e.set_event_thresholds(fixed=[0.0] * e.n_labels, bank=0.0 if bank else None)
    r = np.random.default_rng(5)
    v = e.verifier_add(r.normal(0.0, 0.05, 16 * 96).astype(np.float32), 0.1)
    e.assign_verifiers(0, [0, 32], [v, v], [0.0, 0.0])
    if bank:
        for i in range(4):
            e.bank_add(W.synthetic_head(f"bank{i}", seed=40 + i, hidden=(32, 64, 128, 48)[i]))
        if subscribed:
            e.subscribe([0, 7, 32], [[0, 2], [1, -1], [3, 0]])
    return e


class Trio:
    """A and its two references after the same warm-up; `step` is the follow-up comparison."""

    def __init__(self, family, subscribed=True):
        self.family = family
        self.a, self.rs, self.rl = (_handle(family, subscribed) for _ in range(3))
        self.pcm = _audio(S, WARM + 3, seed=30 + family)
        self.vad = np.random.default_rng(9).random((WARM + 3, S)).astype(np.float32)
        for t in range(WARM):
            for e in (self.a, self.rs, self.rl):
                e.push_vad(self.vad[t])
                e.step(self.pcm[t])

    def ref(self, i):
        return self.rl if i == 1 else self.rs

    def sync(self, i):
        self.ref(i).import_state(ALL, self.a.export_state(ALL))

    def step(self, i, what, rows=ALL, records=True):
        if not records:                                  # (a case without state sync: the third handle keeps in step)
            third = self.rs if i == 1 else self.rl
            third.push_vad(self.vad[WARM + i])
            third.step(self.pcm[WARM + i])
        for e in (self.a, self.ref(i)):
            e.push_vad(self.vad[WARM + i])
        got, want = [], []
        for e, out in ((self.a, got), (self.ref(i), want)):
            out.append(e.step(self.pcm[WARM + i])[rows])
            if self.family == 3:
                out.append(e.bank_scores()[rows])
            rec, total = e.events()
            keep = np.isin(rec["stream"], rows)
            out += [rec[keep].view(np.uint8), e.event_features()[keep]]
            if records:
                out += [np.array([total]), e.export_state(ALL)]
        for k, (g, w) in enumerate(zip(got, want)):
            _eq(g, w, f"family {self.family}, {what}, call {i + 1}: follow-up step, output {k}")
        if records:
            assert np.abs(got[0]).max() > 0 and got[-2][0] > 0, f"family {self.family}, {what}: the follow-up step scores nothing"

    def close(self):
        for e in (self.a, self.rs, self.rl):
            e.close()


def _drive(family, what, args, call):
    """call(engine, arg) -> array or tuple of arrays, on A and on the reference that meets arg first, from the same stream state."""
    t = Trio(family)
    for i, arg in enumerate(args):
        t.sync(i)
        got, want = call(t.a, arg), call(t.ref(i), arg)
        for k, (g, w) in enumerate(zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,))):
            _eq(g, w, f"family {family}, {what}, call {i + 1}, output {k}")
        t.step(i, what)
    t.close()


# ---- the state records first: they are what the other cases synchronise with, here their own scratch is met at 1, 4 and 1 streams ----
@pytest.mark.parametrize("family", FAMILIES)
def test_state_export_and_import_of_1_4_1_streams(family):
    t = Trio(family)
    src = [[3], [1, 8, 31, 32], [5]]
    dst = [[20], [2, 9, 30, 21], [22]]           # (disjoint, so that Rs, which misses call 2, still equals A on the streams of call 3)
    for i in range(3):
        rec = t.a.export_state(src[i])
        _eq(rec, t.ref(i).export_state(src[i]), f"family {family}, export, call {i + 1}")
        for e in (t.a, t.ref(i)):
            e.import_state(dst[i], rec)
        _eq(t.a.export_state(dst[i]), t.ref(i).export_state(dst[i]), f"family {family}, import, call {i + 1}")
        t.step(i, "state records", rows=np.array(src[i] + dst[i]), records=False)
    t.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_reset_of_1_5_2_streams(family):
    def call(e, ids):
        e.reset(ids)
        return e.export_state(ALL)
    _drive(family, "reset", [[4], [0, 8, 9, 31, 32], [32, 2]], call)


@pytest.mark.parametrize("family", FAMILIES)
def test_reset_vad_of_1_5_2_streams(family):
    def call(e, ids):
        e.reset_vad(ids)
        return e.export_state(ALL)
    _drive(family, "reset_vad", [[4], [0, 8, 9, 31, 32], [32, 2]], call)


@pytest.mark.parametrize("family", FAMILIES)
def test_host_fed_step_of_3_5_3_chunks(family):
    long_pcm = _audio(S, 11, seed=77).transpose(1, 0, 2).reshape(S, 11 * 1280)
    cut = {0: long_pcm[:, :3 * 1280], 1: long_pcm[:, 3 * 1280:8 * 1280], 2: long_pcm[:, 8 * 1280:]}
    _drive(family, "long step", [0, 1, 2], lambda e, i: e.step(np.ascontiguousarray(cut[i])))


@pytest.mark.parametrize("family", FAMILIES)
def test_embed_clips_of_1_3_1_clips(family):
    n = 512 + 75 * 160                           # 76 mel frames: one embedding window
    clips = _audio(4, 10, seed=78).transpose(1, 0, 2).reshape(4, 12800)[:, :n]
    _drive(family, "embed_clips", [clips[:1], clips[1:4], clips[3:4]], lambda e, c: e.embed_clips(np.ascontiguousarray(c)))


@pytest.mark.parametrize("family", FAMILIES)
def test_resample_of_160_1600_160_samples(family):
    x = _audio(S, 2, seed=79).transpose(1, 0, 2).reshape(S, 2560)
    _drive(family, "resample", [x[:, :160], x[:, 160:1760], x[:, 1760:1920]], lambda e, c: e.resample(np.ascontiguousarray(c), 8000))


@pytest.mark.parametrize("family", FAMILIES)
def test_masked_steps_of_1_9_1_participants(family):
    pcm = _audio(S, 3, seed=80)
    masks = np.zeros((3, S), np.uint8)
    masks[0, 32] = 1
    masks[1, [0, 1, 2, 8, 15, 16, 30, 31, 32]] = 1
    masks[2, 7] = 1
    _drive(family, "masked step", [0, 1, 2], lambda e, i: (e.step_masked(pcm[i], masks[i]), e.export_state(ALL)))


def test_subscriptions_that_need_1_then_4_then_1_bank_tiles():
    family = 3                                   # (the bank runs on the f16-split family only)
    one = np.full((S, K), -1)
    one[0, 0] = 0                                                                    # one entry: one tile
    many = np.stack([np.arange(S) % 2, 2 + np.arange(S) % 2], 1)                     # four heads, 16 or 17 entries each: four tiles
    t = Trio(family, subscribed=False)           # (no subscription at creation: the tile table is first met here)
    for i, table in enumerate([one, many, one]):
        for e in (t.a, t.ref(i)):
            e.subscribe(ALL, table)
        t.sync(i)
        assert t.a.bank_routing() == t.ref(i).bank_routing() and sum(t.a.bank_routing()["tiles"]) == (4 if i == 1 else 1)
        t.step(i, "subscribe")
    t.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_ingest_of_80_800_80_samples(family):
    msg = np.random.default_rng(81).integers(0, 256, (S, 960), dtype=np.uint8)
    _drive(family, "ingest", [msg[:, :80], msg[:, 80:880], msg[:, 880:]],
           lambda e, m: (e.ingest(np.ascontiguousarray(m)), e.export_state(ALL)))
