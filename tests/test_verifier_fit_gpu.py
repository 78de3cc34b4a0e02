"""The device-side custom-verifier fit on the GPU (include/owwhip.h: oww_verifier_fit / oww_verifier_get; owwhip_fit.h).

Yardstick: the float64 definition of tests/verifier_fit_ref.py (fit64: the optimum of scikit-learn's objective, which
tests/test_verifier_fit_cpu.py holds to scikit-learn at tol = 1e-12), scored in float64 on each case's training windows plus 128
held-out windows.  Bounds: 1e-4 to the definition (the project's score parity class); to the fp32 restatement (fit32) 4 x the
restatement's own distance to the definition, taken as the largest such distance over the table (one figure per run, printed): the
device and the restatement stop their iterations at different residuals below eps_stop, so a per-case figure as small as fp32
round-off of w itself (N = 2: 2e-8) would measure the stop point, not the arithmetic."""
import copy
import functools

import numpy as np
import pytest

from openwakeword_amd import weights as W
from openwakeword_amd._lib import OwwError
from openwakeword_amd.engine import StreamEngine
from openwakeword_amd.model import BatchedModel
from oracle import oww_oracle as O

from golden import cases
import verifier_fit_ref as R

pytestmark = pytest.mark.gpu

NAMES = ["alexa", "hey_mycroft", "hey_jarvis"]
SCORE_CLASS = 1e-4


def _heads(names):
    return {n: W.synthetic_head(n, cases.SEED_WEIGHTS) for n in names}


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(cases.SEED_WEIGHTS)


def _engine(capacity, names=("alexa", "timer"), n=4):
    return StreamEngine(n, _heads(names), _emb(), verifier_capacity=capacity)


def _fit(e, cs, on_device=False):
    """one oww_verifier_fit over the cases cs (same T, same C) -> result dicts"""
    T, C = cs[0]["T"], cs[0]["C"]
    assert all(c["T"] == T and c["C"] == C for c in cs)
    X = np.concatenate([c["X"] for c in cs]).reshape(-1, T, 96)
    y = np.concatenate([c["y"] for c in cs])
    off = np.concatenate([[0], np.cumsum([c["X"].shape[0] for c in cs])])
    if on_device:
        import torch
        xd = torch.from_numpy(X).cuda()
        torch.cuda.synchronize()
        return e.verifier_fit(xd, off, y, T, C, on_device=True)
    return e.verifier_fit(X, off, y, T, C)


def test_accuracy_every_case_of_the_table():
    """every case of the table in a few batched calls (one per (T, C)); the verifier read back with oww_verifier_get and scored in
    float64: within 1e-4 of the float64 definition and within 4 x the restatement's distance of the restatement; residual <= eps_stop,
    iterations below the cap."""
    table = R.table()
    d32 = max(R.reference(c["name"])["d32"] for c in table)
    print(f"restatement to definition, largest over the table: {d32:.3g}")
    e = _engine(len(table))
    try:
        groups = {}
        for c in table:
            groups.setdefault((c["T"], c["C"]), []).append(c)
        worst64 = worst32 = 0.0
        for (T, C), cs in sorted(groups.items()):
            for c, r in zip(cs, _fit(e, cs)):
                ref = R.reference(c["name"])
                assert r["status"] == R.ST_OK and r["id"] >= 0, (c["name"], r)
                assert r["n_pos"] == int(c["y"].sum()) and r["n_neg"] == int((1 - c["y"]).sum())
                w, b = e.verifier_get(r["id"], T)
                s = R.scores(w, b, ref["A"])
                e64, e32 = float(np.abs(s - ref["s64"]).max()), float(np.abs(s - ref["s32"]).max())
                print(f"{c['name']:7s} N={c['X'].shape[0]:4d} T={T:2d} C={C:g} {c['regime']:5s} it={r['iterations']} (ref {ref['fit32']['iterations']}) "
                      f"res={r['residual']:.2e} |dev-f64|={e64:.2e} |dev-f32|={e32:.2e} |f32-f64|={ref['d32']:.2e}")
                worst64, worst32 = max(worst64, e64), max(worst32, e32)
                assert e64 <= SCORE_CLASS, (c["name"], e64)
                assert e32 <= 4 * d32, (c["name"], e32, d32)
                assert r["residual"] <= R.EPS_STOP and r["iterations"] < R.NEWTON_CAP, (c["name"], r)
        print(f"worst |device - float64| = {worst64:.3g}, worst |device - restatement| = {worst32:.3g} (bound {4 * d32:.3g})")
    finally:
        e.close()


def _bits(e, r, T):
    w, b = e.verifier_get(r["id"], T)
    return w.tobytes() + np.float32(b).tobytes()


def test_batch_invariance_bit_for_bit(monkeypatch):
    """a problem's (w, bias) is the same bits fitted alone, first, last or in the middle of a shuffled batch of different N (2, 17, 65,
    200), from host and from device windows, and when the call is forced into several slabs"""
    rows = [("b2", 2, "gauss"), ("b17", 17, "dup"), ("b65", 65, "gauss"), ("b200", 200, "imbal")]
    cs = [R.make_case(nm, N, 16, 1e-3, reg, 900 + i, 3 if reg == "imbal" else None) for i, (nm, N, reg) in enumerate(rows)]
    e = _engine(64)
    try:
        alone = {}
        for c in cs:
            (r,) = _fit(e, [c])
            assert r["status"] == R.ST_OK
            alone[c["name"]] = _bits(e, r, 16)
        orders = [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 3, 1]]
        for k, order in enumerate(orders):
            for mode in ("host", "device", "slabs"):
                if mode == "slabs":                 # 200 windows of 1536 floats need ~2.6 MB: every problem becomes a slab of its own
                    monkeypatch.setenv("OWW_FIT_SCRATCH_BYTES", "1000000")
                elif mode == "device" and k != 2:
                    continue
                batch = [cs[i] for i in order]
                res = _fit(e, batch, on_device=mode == "device")
                monkeypatch.delenv("OWW_FIT_SCRATCH_BYTES", raising=False)
                for c, r in zip(batch, res):
                    assert r["status"] == R.ST_OK, (c["name"], r)
                    assert _bits(e, r, 16) == alone[c["name"]], (c["name"], order, mode)
    finally:
        e.close()


def test_statuses_and_pool_accounting():
    """one call with a one-class problem, a NaN window, N = 1 and three good problems; then a refusal for lack of free slots leaves
    the pool as it was, bit for bit"""
    good = [R.make_case(f"g{i}", N, 16, 1e-3, "gauss", 950 + i) for i, N in enumerate((17, 33, 65))]
    one = R.make_case("one", 20, 16, 1e-3, "gauss", 960)
    one["y"][:] = 1
    nan = R.make_case("nan", 20, 16, 1e-3, "gauss", 961)
    nan["X"][7, 100] = np.nan
    n1 = R.make_case("n1", 2, 16, 1e-3, "gauss", 962)
    n1 = dict(n1, X=n1["X"][:1], y=n1["y"][:1])
    e = _engine(5)
    try:
        batch = [good[0], one, nan, good[1], n1, good[2]]
        res = _fit(e, batch)
        want = [R.ST_OK, R.ST_ONE_CLASS, R.ST_NONFINITE, R.ST_OK, R.ST_BAD_N, R.ST_OK]
        assert [r["status"] for r in res] == want, res
        assert all((r["id"] >= 0) == (r["status"] == R.ST_OK) and (r["id"] >= 0 or r["id"] == -1) for r in res)
        ids = [r["id"] for r in res if r["status"] == R.ST_OK]
        assert len(set(ids)) == 3
        free = [i for i in range(5) if i not in ids]
        for i in free:                              # not live: the NaN problem's slot among them
            with pytest.raises(OwwError):
                e.verifier_get(i, 16)
        # the pool's free count dropped by exactly three: two more verifiers fit, a third does not
        before = {i: _bits(e, dict(id=i), 16) for i in ids}
        with pytest.raises(OwwError, match="free pool slots"):
            _fit(e, good)
        assert {i: _bits(e, dict(id=i), 16) for i in ids} == before
        for i in free:
            with pytest.raises(OwwError):
                e.verifier_get(i, 16)
        res2 = _fit(e, good[:2])
        assert sorted(r["id"] for r in res2) == sorted(free)
        assert {i: _bits(e, dict(id=i), 16) for i in ids} == before
        # whole-call refusals change nothing either
        for kw in (dict(T=0), dict(T=35), dict(C=0.0), dict(C=float("nan"))):
            with pytest.raises(OwwError):
                e.verifier_fit(np.zeros((17, 35 * 96), np.float32), [0, 17], good[0]["y"], kw.get("T", 16), kw.get("C", 1e-3))
        with pytest.raises(OwwError):
            e.verifier_fit(good[0]["X"], [0, 10, 5], good[0]["y"], 16)
        with pytest.raises(OwwError):
            e.verifier_fit(good[0]["X"], [0, 17], np.full(17, 2, np.uint8), 16)
        assert {i: _bits(e, dict(id=i), 16) for i in ids} == before
    finally:
        e.close()


def test_fit_then_add_on_a_second_handle_gives_the_same_scores():
    """fit_verifiers -> get_verifier -> add_verifier((w, bias)) on a second handle: bit-equal verified scores on both"""
    c = R.make_case("eq", 65, 16, 1e-3, "gauss", 970)
    kw = dict(weights={"embedding": _emb(), "heads": _heads(NAMES)}, verifier_capacity=2)
    a, b = BatchedModel(8, NAMES, **kw), BatchedModel(8, NAMES, **kw)
    try:
        (vid,) = a.fit_verifiers(c["X"].reshape(-1, 16, 96), c["y"])
        w, bias = a.get_verifier(vid)
        vid_b = b.add_verifier((w, bias))
        for m, v in ((a, vid), (b, vid_b)):
            m.assign_verifiers(np.arange(8), "alexa", v, threshold=0.0)
        pcm = W.synthetic_pcm(8, 10 * 1280, seed=0xA11CE, rms=3000.0)
        n_eval = 0
        for t in range(10):
            x = pcm[:, t * 1280:(t + 1) * 1280]
            np.testing.assert_array_equal(a.predict_batch(x), b.predict_batch(x))
            n_eval += a.verifier_stats()[1]
        assert n_eval > 0
    finally:
        a.close()
        b.close()


def _pipeline(X, y):
    """the reference's pipeline at tol = 1e-12 around [N, T, 96] windows (tests/verifier_fixture.py's form)"""
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import FunctionTransformer, StandardScaler
    from verifier_fixture import flatten_features
    pipe = make_pipeline(FunctionTransformer(flatten_features), StandardScaler(), LogisticRegression(random_state=0, max_iter=20000, C=0.001, tol=1e-12))
    pipe.fit(X, y)
    return pipe


def test_end_to_end_capture_fit_assign_step():
    """70 streams with a pool: windows of two users captured with score_clip_hits, fitted with fit_verifiers, assigned, 12 steps:
    within 1e-4 of OracleModels carrying the tol = 1e-12 scikit-learn pipelines fitted on the same windows; streams without an
    assignment keep the bits of a twin that never fitted anything; a fit between submit and collect does not change the collected scores"""
    S, THR = 70, 0.3
    heads = _heads(NAMES)
    kw = dict(weights={"embedding": _emb(), "heads": heads}, verifier_capacity=4)
    bm, twin = BatchedModel(S, NAMES, **kw), BatchedModel(S, NAMES, **kw)
    try:
        users = []
        for u in range(2):
            clips = W.synthetic_pcm(4, 96000, seed=40 + u, rms=3000.0)        # 6 s each: some 60 windows of 16 rows per clip
            hits = bm.score_clip_hits(clips, threshold=0.0)["alexa"]           # threshold 0: every window, as the reference's negatives
            X = hits["windows"][:120].astype(np.float32)
            y = (hits["score"][:120] >= np.median(hits["score"][:120])).astype(np.uint8)
            assert X.shape == (120, 16, 96) and 0 < y.sum() < 120, (X.shape, int(y.sum()))
            users.append((X, y))
        ids = bm.fit_verifiers([X for X, _ in users], [y for _, y in users])
        assert len(set(ids)) == 2
        pipes = [_pipeline(X, y) for X, y in users]
        own = np.where(np.arange(S) < 30, 0, np.where(np.arange(S) < 60, 1, -1))
        for u in range(2):
            bm.assign_verifiers(np.flatnonzero(own == u), "alexa", ids[u], threshold=THR)
        noise = W.synthetic_pcm(1, 64000, seed=3, rms=600.0)[0]
        oracle0 = O.OracleModel(heads, _emb(), init_noise=noise)
        init = oracle0.preprocessor.features[-bm.engine.feature_ring:].astype(np.float32)
        bm.reset(None, init)
        twin.reset(None, init)

        def pipe_fn(head, pipe):
            def fn(x):
                sc = O.head_stage(x, head, np.float32)
                if pipe is not None and sc[0, 0] >= THR:
                    sc = np.array([[pipe.predict_proba(x)[0][-1]]], np.float32)
                return [sc]
            return fn

        models = []
        for s in range(S):
            m = copy.deepcopy(oracle0)
            m.head_fns = {"alexa": pipe_fn(heads["alexa"], pipes[own[s]] if own[s] >= 0 else None),
                          "hey_mycroft": pipe_fn(heads["hey_mycroft"], None), "hey_jarvis": pipe_fn(heads["hey_jarvis"], None)}
            models.append(m)
        pcm = W.synthetic_pcm(S, 12 * 1280, seed=0xA11CE, rms=3000.0)
        extra = R.make_case("mid", 33, 16, 1e-3, "gauss", 980)
        worst, n_eval = 0.0, 0
        for t in range(12):
            x = np.ascontiguousarray(pcm[:, t * 1280:(t + 1) * 1280])          # (submit takes a contiguous array)
            if t == 8:                              # a fit between submit and collect
                bm.submit_batch(x)
                (r,) = bm.engine.verifier_fit(extra["X"], [0, 33], extra["y"], 16)
                assert r["status"] == R.ST_OK
                got = bm.collect_batch()
            else:
                got = bm.predict_batch(x)
            ref = twin.predict_batch(x)
            np.testing.assert_array_equal(got[own < 0], ref[own < 0])
            np.testing.assert_array_equal(got[:, 1:], ref[:, 1:])
            for s, m in enumerate(models):
                pred = m.predict(x[s])
                worst = max(worst, float(np.max(np.abs(got[s] - np.array([pred[k] for k in NAMES], np.float32)))))
            if t >= 5:
                n_eval += bm.verifier_stats()[1]
        print(f"worst |device - oracle| = {worst:.3g}; {n_eval} verifier evaluations")
        assert n_eval > 0
        assert worst <= SCORE_CLASS, worst
    finally:
        bm.close()
        twin.close()
