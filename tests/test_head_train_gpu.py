"""Training bank heads on the device (include/owwhip.h: oww_train_*; owwhip_train.h) on the GPU.

Yardsticks: the float64 definition of tests/head_train_ref.py (ref64, which tests/test_head_train_cpu.py holds to the reference's
own train.Model at 1e-10), the fp32 restatement's decisions (kept counts, step / skip, where a loss is recorded), and the
reference's own fp32 run stored in tests/golden/head_train.npz (T <= 2).  Budgets: test_head_train_cpu.py's budget_param
(per shape class) and BUDGET_SCORE, 8 x the largest distance of any fp32 run (torch's, the restatement's four summation orders) from ref64."""
import functools

import numpy as np
import pytest

from openwakeword_amd import train as T_
from openwakeword_amd import weights as W
from openwakeword_amd._lib import OwwError
from openwakeword_amd.engine import StreamEngine
from openwakeword_amd.model import BatchedModel
from oracle import oww_oracle as O

import head_train_ref as R
from bank_oracle import BankOracle
from test_head_train_cpu import BUDGET_SCORE, budget_param, admitted_cases, case_of, golden, ref32_of, ref64_of

pytestmark = pytest.mark.gpu
EMB_SEED = 3


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(EMB_SEED)


def _engine(S=4, ring=16, **kw):
    return StreamEngine(S, {"alexa": W.synthetic_head("alexa", 1234)}, _emb(), feature_ring=ring, **kw)


def _run(e, case, problems=None, splits=None, pool_on_device=False, tables_on_device=False, shared=False):
    """the case's problems (default all) in one session -> (records [U', n], loss [U', K], kept [U', K])"""
    us = list(range(case["U"])) if problems is None else list(problems)
    heads = [T_.record_to_head(case["init"][u], case["T"], case["D"]) for u in us]
    tr = T_.HeadTrainer(e, case["T"], case["D"], len(us), init=heads)
    try:
        if pool_on_device:
            import torch
            pd = torch.from_numpy(case["pool"]).cuda()
            torch.cuda.synchronize()
            tr.set_pool(pd, n_windows=case["pool"].shape[0], on_device=True)
        else:
            tr.set_pool(case["pool"])
        idx, y = case["idx"][us], case["y"][us]
        if shared:
            idx, y = idx[0], y[0]
        K = case["K"]
        cuts = [0, K] if splits is None else splits
        for a, b in zip(cuts[:-1], cuts[1:]):
            i, yy = np.ascontiguousarray(idx[..., a:b, :]), np.ascontiguousarray(y[..., a:b, :])
            if tables_on_device:
                import torch
                idv, yd = torch.from_numpy(i).cuda(), torch.from_numpy(yy).cuda()
                torch.cuda.synchronize()
                tr.steps(idv, yd, case["lr"][a:b], case["nw"][a:b], on_device=True, shape=i.shape)
            else:
                tr.steps(i, yy, case["lr"][a:b], case["nw"][a:b])
        return tr.records(), tr.history["loss"], tr.history["kept"]
    finally:
        tr.close()


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _check_decisions(name, loss, kept, ref):
    np.testing.assert_array_equal(kept, ref["kept"], err_msg=name)
    np.testing.assert_array_equal(~np.isnan(loss), ref["steps"], err_msg=name)


@pytest.mark.parametrize("name", [n for n in admitted_cases() if n != R.SATURATION])
def test_case_within_budget(eng, name):
    """parameters within the budget of ref64 (and of the reference's own fp32 run where a golden exists), scores of 64 probe windows
    within the score budget; kept counts and step / skip decisions exactly the restatement's; recorded losses to fp32 round-off"""
    case, r64, r32 = case_of(name), ref64_of(name), ref32_of(name, 0)
    rec, loss, kept = _run(eng, case)
    _check_decisions(name, loss, kept, r32)
    g = golden().get(name)
    for u in range(case["U"]):
        e64 = R.rel_param_error(rec[u], r64["params"][u], case)
        sc = float(np.abs(R.score(rec[u], case) - R.score(r64["params"][u], case)).max())
        eg = R.rel_param_error(rec[u], g["params"][u], case) if g is not None else float("nan")
        print(f"{name} u={u}: |dev - ref64| param {e64:.2e} score {sc:.2e}; |dev - reference fp32| param {eg:.2e}")
        assert e64 <= budget_param(case) and sc <= BUDGET_SCORE, (name, u, e64, sc)
        if g is not None:
            assert eg <= budget_param(case), (name, u, eg)
    st = r64["steps"]
    if st.any():
        assert np.abs(loss[st] / r64["loss"][st] - 1).max() <= 1e-4, name
    if g is not None:
        np.testing.assert_array_equal(kept, g["kept"], err_msg=name)


def test_saturation_case_is_held_to_its_golden(eng):
    """one kept negative at p = 1.0f exactly: binary_cross_entropy's fp32 gradient is zero there, so it contributes nothing (float64
    does not saturate at that logit and is no yardstick for it)"""
    case = case_of(R.SATURATION)
    g = golden()[R.SATURATION]
    rec, loss, kept = _run(eng, case)
    np.testing.assert_array_equal(kept, g["kept"])
    np.testing.assert_array_equal(~np.isnan(loss), ~np.isnan(g["loss"]))
    e = R.rel_param_error(rec[0], g["params"][0], case)
    sc = float(np.abs(R.score(rec[0], case) - R.score(g["params"][0], case)).max())
    print(f"saturated: |dev - reference fp32| param {e:.2e} score {sc:.2e}")
    assert e <= budget_param(case) and sc <= BUDGET_SCORE, (e, sc)


def test_batch_invariance_bit_for_bit(eng):
    """a problem's parameters: alone, as u = 0, 1, 2 of three, among 70, from a host or a device pool and tables, with one table shared
    by all problems"""
    case = case_of("fresh_u3")
    alone = [_run(eng, case, [u])[0][0] for u in range(3)]
    three = _run(eng, case)[0]
    for u in range(3):
        np.testing.assert_array_equal(three[u], alone[u])
    rot = _run(eng, case, [2, 0, 1])[0]
    for i, u in enumerate([2, 0, 1]):
        np.testing.assert_array_equal(rot[i], alone[u])
    # among 70: the three problems repeated; every copy has its original's bits
    big = dict(case)
    reps = [u % 3 for u in range(70)]
    big["U"], big["init"], big["idx"], big["y"] = 70, case["init"][reps], case["idx"][reps], case["y"][reps]
    many = _run(eng, big)[0]
    for i, u in enumerate(reps):
        np.testing.assert_array_equal(many[i], alone[u])
    dev = _run(eng, case, pool_on_device=True, tables_on_device=True)[0]
    np.testing.assert_array_equal(dev, three)
    # one shared table: every problem trains on problem 0's batches
    sh = _run(eng, case, shared=True)[0]
    own = dict(case)
    own["idx"], own["y"] = case["idx"][[0, 0, 0]], case["y"][[0, 0, 0]]
    np.testing.assert_array_equal(sh, _run(eng, own)[0])


def test_one_call_or_two_bit_for_bit(eng):
    case = case_of("ramp_k40")
    one = _run(eng, case)
    two = _run(eng, case, splits=[0, 20, 40])
    for a, b in zip(one, two):
        np.testing.assert_array_equal(a, b)


def test_refusals_leave_the_state_untouched(eng):
    case = case_of("fresh_n33")
    T, D = case["T"], case["D"]
    head = T_.record_to_head(case["init"][0], T, D)
    with pytest.raises(OwwError):
        eng.train_set_pool(case["pool"])                          # no session
    with pytest.raises(OwwError):
        eng.train_end()
    with pytest.raises(ValueError):
        eng.train_steps(1, case["idx"][0, :1], case["y"][0, :1], case["lr"][:1], case["nw"][:1])      # no session
    for bad_T, bad_D in ((0, 32), (17, 32), (1, 24), (1, 144), (1, 0)):
        with pytest.raises((OwwError, ValueError)):
            eng.train_begin(np.zeros((1, max(T_.param_count(max(bad_T, 1), max(bad_D, 16)), 1)), np.float32), bad_T, bad_D)
    with pytest.raises((OwwError, ValueError)):
        eng.train_begin(np.zeros((0, T_.param_count(T, D)), np.float32), T, D)      # U = 0
    tr = T_.HeadTrainer(eng, T, D, 1, init=[head])
    try:
        np.testing.assert_array_equal(tr.records()[0], case["init"][0])            # get before any step: the initial record, bit for bit
        with pytest.raises(OwwError):
            T_.HeadTrainer(eng, T, D, 1, init=[head])                               # a second begin
        idx, y, lr, nw = case["idx"][:, :4], case["y"][:, :4], case["lr"][:4], case["nw"][:4]
        with pytest.raises(OwwError):
            tr.steps(idx, y, lr, nw)                                                # no pool yet
        tr.set_pool(case["pool"])
        P = case["pool"].shape[0]
        bad = []
        i2 = idx.copy(); i2[0, 1, 3] = P; bad.append((i2, y, lr, nw))
        i3 = idx.copy(); i3[0, 0, 0] = -2; bad.append((i3, y, lr, nw))
        y2 = y.copy(); y2[0, 2, 1] = 2; bad.append((idx, y2, lr, nw))
        for v in (np.nan, np.inf, -1e-3):
            l2 = lr.copy(); l2[1] = v; bad.append((idx, y, l2, nw))
            w2 = nw.copy(); w2[2] = v; bad.append((idx, y, lr, w2))
        bad.append((np.zeros((1, 1, 4097), np.int32), np.zeros((1, 1, 4097), np.uint8), lr[:1], nw[:1]))
        bad.append((np.zeros((1, 4097, 1), np.int32), np.zeros((1, 4097, 1), np.uint8), np.zeros(4097), np.ones(4097, np.float32)))
        for args in bad:
            with pytest.raises(OwwError):
                tr.steps(*args)
        for wrong_U in (0, 2):                                                      # the engine sizes tables and records by the session's U
            with pytest.raises(ValueError):
                eng.train_steps(wrong_U, idx[0], y[0], lr, nw)
        np.testing.assert_array_equal(tr.records()[0], case["init"][0])
        assert tr.history["loss"].shape[1] == 0
        tr.steps(case["idx"], case["y"], case["lr"], case["nw"])                   # and the session still trains: the same bits as a fresh one
        got = tr.records()
    finally:
        tr.close()
    np.testing.assert_array_equal(got, _run(eng, case)[0])
    np.testing.assert_array_equal(got, _run(eng, case)[0])                          # begin / end twice over


def test_end_to_end_train_bank_serve():
    """init_head -> 300 steps on a separable pool (U = 3, D = 32, T = 16) -> heads() -> bank_add -> dense scores against the oracle on the
    returned parameters -> 12 live steps of 70 streams subscribed to the trained heads against oracles carrying them"""
    S, U, D, T, steps, n = 70, 3, 32, 16, 300, 128
    r = np.random.default_rng(11)
    pool, lab = R._pool(r, 600, T)
    pos, neg = np.flatnonzero(lab == 1), np.flatnonzero(lab == 0)
    problems = [(pos[u::U], neg[u::U]) for u in range(U)]
    heads_fixed = {"alexa": W.synthetic_head("alexa", 1234)}
    bm = BatchedModel(S, ["alexa"], weights={"heads": heads_fixed, "embedding": _emb()}, bank_slots=1, bank_capacity=8)
    try:
        heads, hist = T_.train_heads(bm, pool, problems, steps, hidden=D, n_batch=n, lr=1e-3, max_negative_weight=10, seed=5)
        assert hist["loss"].shape == (U, steps) and np.isfinite(hist["loss"][:, 1:]).any()
        # the restatement on the same batches (the same trajectory class)
        idx, y = T_.draw_tables(problems, steps, n, 5)
        k = np.arange(steps)
        case = dict(T=T, D=D, K=steps, U=U, pool=pool, idx=idx, y=y, nw=np.asarray(T_.negative_weight_schedule(steps, 10), np.float32),
                    lr=np.asarray(T_.lr_warmup_cosine_decay(k, steps // 5, steps // 3, steps, target_lr=1e-3), np.float64),
                    init=np.stack([T_.head_to_record(T_.init_head(T, D, 5 + u)) for u in range(U)]))
        r32 = R.ref_train(case, np.float32, order=2)
        X = pool.reshape(600, -1)
        for u in range(U):
            rows = np.concatenate(problems[u])
            acc_dev = np.mean((R.forward(R.unpack(T_.head_to_record(heads[u]), T, D, np.float64), X[rows], np.float64)["p"] >= 0.5) == lab[rows])
            acc_ref = np.mean((R.forward(R.unpack(r32["params"][u], T, D, np.float64), X[rows], np.float64)["p"] >= 0.5) == lab[rows])
            print(f"problem {u}: training accuracy device {acc_dev:.4f} restatement {acc_ref:.4f}")
            assert acc_dev >= acc_ref and acc_dev > 0.9
        ids = [bm.bank_add(h) for h in heads]
        got = bm.bank_score_features(pool[:64], ids)                               # [64, 1, U]
        for u in range(U):
            want = O.head_stage(pool[:64], heads[u], dtype=np.float64)[:, 0]
            assert np.abs(got[:, 0, u] - want).max() <= 1e-4
        sub = np.array(ids, np.int32)[np.arange(S) % U][:, None]
        bm.subscribe(np.arange(S), sub)
        bank = {ids[u]: heads[u] for u in range(U)}
        noise = W.synthetic_pcm(1, 64000, seed=3, rms=600.0)[0]
        first = BankOracle(bank, _emb(), 1, init_noise=noise)
        bm.engine.reset(None, first.preprocessor.features[-bm.engine.feature_ring:].astype(np.float32))
        sample = [0, 1, 2, 35, 69]
        oracles = {s: BankOracle(bank, _emb(), 1, features=first.preprocessor.features) for s in sample}
        for s in sample:
            oracles[s].subscribe(sub[s])
        worst = 0.0
        for t in range(12):
            x = (r.standard_normal((S, 1280)) * 3000).astype(np.int16)
            bm.predict_batch(x)
            b = bm.bank_scores()
            for s in sample:
                _, want = oracles[s].predict(x[s])
                if len(oracles[s].rings[0]) > 5:
                    worst = max(worst, abs(float(b[s, 0]) - want[0]))
        print(f"live bank scores of trained heads against the oracle: {worst:.2e}")
        assert worst <= 1e-4
    finally:
        bm.close()
