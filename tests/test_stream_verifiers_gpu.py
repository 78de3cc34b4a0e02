"""Per-stream custom verifiers on the GPU (include/owwhip.h: oww_verifier_* / oww_assign_verifiers / oww_bank_assign_verifiers).

Yardstick of the bit-identity tests: for every verifier V, a second handle with V as the label's handle-wide verifier
(oww_set_verifier) on the same inputs.  Inputs: the synthetic weights of seed cases.SEED_WEIGHTS, Gaussian PCM of RMS 3000 and the
reference's feature seeding from noise of RMS 600, with thresholds 0.3 / 0.5, so that between 10 % and 90 % of the verified pairs past
the first five frames are re-scored -- every test that claims verification asserts that share from verifier_stats()."""
import copy
import functools

import numpy as np
import pytest

from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine
from openwakeword_amd.model import BatchedModel, fold_verifier
from oracle import oww_oracle as O

from golden import cases
from verifier_fixture import trained_verifier

pytestmark = pytest.mark.gpu

NAMES = ["alexa", "hey_mycroft", "hey_jarvis"]
S = 8
DEFAULT, NONE = -1, -2


def _heads(names=NAMES):
    return {n: W.synthetic_head(n, cases.SEED_WEIGHTS) for n in names}


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(cases.SEED_WEIGHTS)


@functools.lru_cache(maxsize=None)
def _oracle0():
    """An OracleModel whose feature buffer holds the reference's start-up embeddings of noise (utils.py:169)."""
    noise = W.synthetic_pcm(1, 64000, seed=3, rms=600.0)[0]
    return O.OracleModel(_heads(), _emb(), init_noise=noise)


@functools.lru_cache(maxsize=None)
def _verifier(seed):
    return fold_verifier(trained_verifier(seed))


def _engine(n=S, heads=None, capacity=0, **kw):
    e = StreamEngine(n, _heads() if heads is None else heads, _emb(), verifier_capacity=capacity, **kw)
    e.reset(None, _oracle0().preprocessor.features[-e.feature_ring:].astype(np.float32))
    return e


def _pcm(n_frames, n=S):
    return W.synthetic_pcm(n, n_frames * 1280, seed=0xA11CE, rms=3000.0)


# the call schedule of test 1: 44 calls over 48 frames -- one-chunk steps, two 3-chunk calls, two masked steps, graph mode from call 31
def _schedule():
    ops = []
    for t in range(44):
        if t in (10, 25):
            ops.append(("chunks", 3))
        elif t == 15:
            ops.append(("mask", np.arange(S) % 2 == 0))
        elif t == 30:
            ops.append(("mask", np.arange(S) % 3 != 0))
        else:
            ops.append(("graph" if t >= 31 else "chunks", 1))
    return ops


def _run(engines, ops, pcm, each=None):
    """Apply the schedule to every engine; each(t, op, scores_per_engine) after every call."""
    f = 0
    for t, (kind, arg) in enumerate(ops):
        if kind == "graph" and arg == 1 and (t == 0 or ops[t - 1][0] != "graph"):
            for e in engines:
                e.use_graph(True)
        if kind == "mask":
            x = pcm[:, f * 1280:(f + 1) * 1280]
            out = [e.step_masked(x, arg) for e in engines]
            f += 1
        else:
            k = arg
            x = pcm[:, f * 1280:(f + k) * 1280]
            out = [e.step(x) for e in engines]
            f += k
        if each is not None:
            each(t, kind, arg, out)
    return f


def _share(n_eval, n_pairs):
    share = n_eval / n_pairs
    print(f"re-scored {n_eval} of {n_pairs} verified pairs past the first five frames: {share:.3f}")
    assert 0.10 <= share <= 0.90, share
    return share


def test_per_stream_verifiers_bit_identical_to_handle_wide():
    """Three verifiers on disjoint stream subsets of two columns (alexa at 0.3, hey_mycroft at 0.5) of one handle equal, bit for
    bit, handles with each verifier handle-wide; 44 calls (1- and 3-chunk, masked, graph mode), so the 30-deep ring wraps."""
    vs = [_verifier(seed) for seed in (0, 1, 2)]
    thr = {0: 0.3, 1: 0.5}                                   # column -> threshold
    assign = {0: np.array([0, 0, 0, 1, 1, 1, 2, 2]), 1: np.array([1, 1, 1, 1, 2, 2, 2, 0])}
    a = _engine(capacity=4)
    ids = [a.verifier_add(w, b) for w, b in vs]
    assert ids == [0, 1, 2]
    for col, v in assign.items():
        a.assign_verifiers(col, np.arange(S), np.array(ids)[v], np.full(S, thr[col]))
    assert a.verifier_stats()[0] == 2 * S
    yard = []
    for w, b in vs:
        e = _engine()
        for col in thr:
            e.set_verifier(col, w, b, thr[col])
        yard.append(e)
    counts = {"eval": 0, "pairs": 0}

    def check(t, kind, arg, out):
        got = out[0]
        for col, v in assign.items():
            for s in range(S):
                np.testing.assert_array_equal(got[s, col], out[1 + v[s]][s, col], err_msg=f"call {t} stream {s} column {col}")
        for s in range(S):
            np.testing.assert_array_equal(got[s, 2], out[1][s, 2])
        if t >= 5:
            n_on = int(np.sum(arg)) if kind == "mask" else S
            counts["eval"] += a.verifier_stats()[1]
            counts["pairs"] += 2 * n_on

    frames = _run([a] + yard, _schedule(), _pcm(48), check)
    assert frames == 48
    _share(counts["eval"], counts["pairs"])
    assert not a.range_status()
    for e in [a] + yard:
        e.close()


def test_configured_pool_without_assignments_changes_nothing():
    """A handle with a verifier pool and no assignment scores bit for bit what a handle without a pool scores, with and without a
    handle-wide verifier, over the calls of the bit-identity test."""
    w, b = _verifier(0)
    for handle_wide in (False, True):
        plain, pooled = _engine(), _engine(capacity=8)
        pooled.verifier_add(w, b)
        if handle_wide:
            for e in (plain, pooled):
                e.set_verifier(0, w, b, 0.3)

        def check(t, kind, arg, out):
            np.testing.assert_array_equal(out[0], out[1], err_msg=f"call {t}")

        _run([plain, pooled], _schedule(), _pcm(48), check)
        assert pooled.verifier_stats() == (0, 0)
        plain.close()
        pooled.close()


def test_overrides_none_stream_and_default():
    """NONE on a label with a handle-wide verifier W equals no verifier; a per-stream V overrides W; DEFAULT is W.  Assignments change
    between graph-mode steps; each stream is judged against the handle its assignment of the moment corresponds to."""
    (wv, bv), (ww, bw) = _verifier(3), _verifier(4)
    a = _engine(capacity=2)
    vid = a.verifier_add(wv, bv)
    a.set_verifier(0, ww, bw, 0.3)
    plain, with_v, with_w = _engine(), _engine(), _engine()
    with_v.set_verifier(0, wv, bv, 0.3)
    with_w.set_verifier(0, ww, bw, 0.3)
    ref = np.array([0, 0, 0, 1, 1, 1, 2, 2])                 # 0: plain (NONE), 1: V, 2: W (DEFAULT)
    a.assign_verifiers(0, np.arange(8), np.array([NONE] * 3 + [vid] * 3 + [DEFAULT] * 2), np.full(8, 0.3))
    counts = {"eval": 0, "pairs": 0}
    ops = [("chunks", 1)] * 12 + [("graph", 1)] * 20

    def check(t, kind, arg, out):
        for s in range(S):
            np.testing.assert_array_equal(out[0][s], out[1 + ref[s]][s], err_msg=f"call {t} stream {s} judged against {ref[s]}")
        if 5 <= t <= 25:                                     # (after call 25 the handle-wide kernel serves every pair)
            counts["eval"] += a.verifier_stats()[1]
            counts["pairs"] += int(np.sum(ref != 0))
        if t == 18:                                          # NONE -> DEFAULT, V -> NONE, DEFAULT -> V (graph mode)
            a.assign_verifiers(0, np.arange(8), np.array([DEFAULT] * 3 + [NONE] * 3 + [vid] * 2), np.full(8, 0.3))
            ref[:] = [2, 2, 2, 0, 0, 0, 1, 1]
        if t == 25:                                          # every pair back to the default: the handle-wide kernel again
            a.assign_verifiers(0, np.arange(8), np.full(8, DEFAULT), np.full(8, 0.3))
            ref[:] = 2
            assert a.verifier_stats()[0] == 0

    _run([a, plain, with_v, with_w], ops, _pcm(32), check)
    _share(counts["eval"], counts["pairs"])
    for e in (a, plain, with_v, with_w):
        e.close()


def test_bank_slot_verifiers():
    """A stream subscribed to bank head X with V on that slot scores what a fixed head X with V handle-wide scores.  Resubscribing
    drops the assignment, oww_reset keeps it, oww_bank_remove and oww_verifier_remove revert it."""
    heads = _heads(["alexa", "hey_mycroft"])
    x = heads["alexa"]
    w, b = _verifier(5)

    def make(capacity):
        e = _engine(heads=heads, capacity=capacity, bank_slots=1, bank_capacity=4)
        ids = [e.bank_add(x), e.bank_add(x)]
        e.subscribe(np.arange(S), np.full((S, 1), ids[0]))
        return e, ids

    a, (x1, x2) = make(2)
    vid = a.verifier_add(w, b)
    a.assign_verifiers(0, np.arange(S), np.full(S, vid), np.full(S, 0.3), bank=True)
    y, (y1, y2) = make(0)
    y.set_verifier(0, w, b, 0.3)                             # yardstick: the fixed head X of the same handle, V handle-wide
    verified = np.ones(S, bool)
    counts = {"eval": 0, "pairs": 0}
    pcm = _pcm(40)
    for t in range(40):
        xs = pcm[:, t * 1280:(t + 1) * 1280]
        a.step(xs)
        fy = y.step(xs)
        ga, gy = a.bank_scores()[:, 0], y.bank_scores()[:, 0]
        for s in range(S):
            want = fy[s, 0] if verified[s] else gy[s]
            np.testing.assert_array_equal(ga[s], want, err_msg=f"step {t} stream {s} verified={verified[s]}")
        if 5 <= t < 30:
            counts["eval"] += a.verifier_stats()[1]
            counts["pairs"] += int(verified.sum())
        if t == 12:                                          # streams 0-3 move to X2 and back: a new head in the slot, no verifier
            for e, h2, h1 in ((a, x2, x1), (y, y2, y1)):
                e.subscribe(np.arange(4), np.full((4, 1), h2))
                e.subscribe(np.arange(4), np.full((4, 1), h1))
            verified[:4] = False
            assert a.verifier_stats()[0] == 4
        if t == 20:                                          # Model.reset keeps custom_verifier_models
            a.reset(None, _oracle0().preprocessor.features[-a.feature_ring:].astype(np.float32))
            y.reset(None, _oracle0().preprocessor.features[-y.feature_ring:].astype(np.float32))
            assert a.verifier_stats()[0] == 4
        if t == 30:
            a.subscribe(np.arange(2), np.full((2, 1), x2))   # streams 0-1 on X2 with V, then X2 leaves the bank: empty slots
            y.subscribe(np.arange(2), np.full((2, 1), y2))
            a.assign_verifiers(0, np.arange(2), np.full(2, vid), np.full(2, 0.3), bank=True)
            assert a.verifier_stats()[0] == 6
            a.bank_remove(x2)
            y.bank_remove(y2)
            assert a.verifier_stats()[0] == 4
            a.verifier_remove(vid)                           # streams 4-7: back to the default (none)
            verified[:] = False
            assert a.verifier_stats()[0] == 0
    _share(counts["eval"], counts["pairs"])
    assert not a.range_status()
    a.close()
    y.close()


def _verified_head_fn(head, w, b, thr):
    def fn(x):
        sc = O.head_stage(x, head, np.float32)
        if sc[0, 0] >= thr:
            z = float(x.reshape(-1).astype(np.float64) @ w.astype(np.float64) + b)
            sc = np.array([[1.0 / (1.0 + np.exp(-z))]], np.float32)
        return [sc]
    return fn


def test_oracle_parity_public_api():
    """BatchedModel.add_verifier / assign_verifiers against N independent OracleModels, each with its own scikit-learn pipeline around
    its head function (as tests/test_model_api.py does for the handle-wide verifier); 1e-4."""
    pipes = [trained_verifier(seed) for seed in range(4)]
    heads = _heads()
    bm = BatchedModel(S, NAMES, weights={"embedding": _emb(), "heads": heads}, verifier_capacity=4)
    try:
        ids = [bm.add_verifier(p) for p in pipes]
        own = np.arange(S) % 4
        bm.assign_verifiers(np.arange(S), "alexa", np.array(ids)[own], threshold=0.3)
        bm.assign_verifiers(np.arange(S), "hey_mycroft", np.array(ids)[(own + 1) % 4], threshold=0.5)
        with pytest.raises(ValueError, match="not matched"):
            bm.assign_verifiers([0], "no_such_model", 0)

        def pipe_fn(head, pipe, thr):
            def fn(x):
                sc = O.head_stage(x, head, np.float32)
                if sc[0, 0] >= thr:
                    sc = np.array([[pipe.predict_proba(x)[0][-1]]], np.float32)
                return [sc]
            return fn

        models = []
        for s in range(S):
            m = copy.deepcopy(_oracle0())
            m.head_fns = {"alexa": pipe_fn(heads["alexa"], pipes[own[s]], 0.3),
                          "hey_mycroft": pipe_fn(heads["hey_mycroft"], pipes[(own[s] + 1) % 4], 0.5),
                          "hey_jarvis": (lambda x, _h=heads["hey_jarvis"]: [O.head_stage(x, _h, np.float32)])}
            models.append(m)
        bm.reset(None, _oracle0().preprocessor.features[-bm.engine.feature_ring:].astype(np.float32))
        pcm = _pcm(40)
        worst, n_eval, n_pairs = 0.0, 0, 0
        for t in range(40):
            x = pcm[:, t * 1280:(t + 1) * 1280]
            got = bm.predict_batch(x)
            for s, m in enumerate(models):
                pred = m.predict(x[s])
                want = np.array([pred[k] for k in NAMES], np.float32)
                worst = max(worst, float(np.max(np.abs(got[s] - want))))
            if t >= 5:
                n_eval += bm.verifier_stats()[1]
                n_pairs += 2 * S
        print(f"worst |device - oracle| = {worst:.3g}")
        assert worst <= 1e-4, worst
        _share(n_eval, n_pairs)
    finally:
        bm.close()


def test_scale_131072_streams_1024_verifiers():
    """131,072 streams x 3 heads, every stream assigned one of 1,024 distinct verifiers on alexa (threshold 0.3): no range flag, the
    evaluation counter equals the host count of hits over the raw scores of a handle without verifiers, 64 sampled streams match
    the oracle at 1e-4."""
    n, n_ver, steps, thr = 131072, 1024, 40, 0.3
    base_pcm = _pcm(steps)                                   # stream s carries the audio of stream s % 8 of the other tests
    base = [_verifier(seed) for seed in range(8)]
    pool = [((base[i % 8][0] * np.float32(1.0 + i / 4096.0)).astype(np.float32), base[i % 8][1]) for i in range(n_ver)]
    a = _engine(n, capacity=n_ver)
    ids = np.array([a.verifier_add(w, b) for w, b in pool], np.int32)
    own = np.arange(n) % n_ver
    a.assign_verifiers(0, np.arange(n), ids[own], np.full(n, thr, np.float32))
    p = _engine(n)
    rng = np.random.default_rng(7)
    sample = np.sort(rng.choice(n, 64, replace=False))
    heads = _heads()
    models = {}
    for s in sample:
        m = copy.deepcopy(_oracle0())
        w, b = pool[own[s]]
        m.head_fns = {"alexa": _verified_head_fn(heads["alexa"], w, b, thr),
                      "hey_mycroft": (lambda x, _h=heads["hey_mycroft"]: [O.head_stage(x, _h, np.float32)]),
                      "hey_jarvis": (lambda x, _h=heads["hey_jarvis"]: [O.head_stage(x, _h, np.float32)])}
        models[s] = m
    worst, n_eval, n_pairs = 0.0, 0, 0
    for t in range(steps):
        x = np.ascontiguousarray(np.tile(base_pcm[:, t * 1280:(t + 1) * 1280], (n // S, 1)))
        got = a.step(x)
        raw = p.step_raw(x)
        ev = a.verifier_stats()[1]
        assert ev == int(np.sum(raw[:, 0] >= np.float32(thr))), t
        if t >= 5:
            n_eval += ev
            n_pairs += n
        for s in sample:
            pred = models[s].predict(x[s])
            worst = max(worst, float(np.max(np.abs(got[s] - np.array([pred[k] for k in NAMES], np.float32)))))
    print(f"worst |device - oracle| over {sample.size} streams = {worst:.3g}")
    assert worst <= 1e-4, worst
    _share(n_eval, n_pairs)
    assert not a.range_status()
    a.close()
    p.close()
