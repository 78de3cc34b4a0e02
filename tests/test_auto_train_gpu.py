"""auto_train on the device (include/owwhip.h: oww_train_new_sequence .. oww_train_get_slot; owwhip_autotrain.h) on the GPU.

Yardsticks: tests/auto_train_ref.py -- eval_ref in float64 for the scores (within BUDGET_SCORE = 4e-6, the score budget of
test_head_train_cpu.py: the forward pass is the same arithmetic) and for the five counts (exact on every admitted case),
average_ref bit for bit, auto_train_ref in float64 and the reference's own run in tests/golden/auto_train.npz for every decision of
the end-to-end cases, the final record of a case within 8 x the floor the reference's fp32 run shows against its double run on that case
(test_auto_train_cpu.py: MEASURED_FLOOR, budget_param); the fallback (nothing selected) the live record bit for bit."""
import functools

import numpy as np
import pytest

from openwakeword_amd import train as T_
from openwakeword_amd import weights as W
from openwakeword_amd._lib import OwwError
from openwakeword_amd.engine import StreamEngine
from openwakeword_amd.model import BatchedModel
from oracle import oww_oracle as O

import auto_train_ref as A
import head_train_ref as R
from test_auto_train_cpu import budget_param, E2E, EVAL, e2e_case, golden, golden_entries, ref64_of
from test_head_train_cpu import BUDGET_SCORE

pytestmark = pytest.mark.gpu
EMB_SEED = 3


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(EMB_SEED)


@pytest.fixture(scope="module")
def eng():
    e = StreamEngine(4, {"alexa": W.synthetic_head("alexa", 1234)}, _emb(), feature_ring=16)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def eval_case(name):
    return A.make_eval_case(name)


def _session(e, case, problems=None):
    us = list(range(case["U"])) if problems is None else list(problems)
    tr = T_.HeadTrainer(e, case["T"], case["D"], len(us), init=[T_.record_to_head(case["init"][u], case["T"], case["D"]) for u in us])
    tr.set_eval_pool(case["pool"])
    return tr


def _tables(case, us):
    return (case["idx"], case["y"]) if case["shared"] else (case["idx"][us], case["y"][us])


def _counts(out, u):
    return {c: int(out[c][u]) for c in A.COUNTS}


# ---------------------------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("name", EVAL)
def test_eval_against_float64(eng, name):
    """scores within the score budget of eval_ref in float64, NaN in empty slots; all five counts exact; live parameters and a slot"""
    case = eval_case(name)
    want_c, want_s = A.eval_case_ref(case, np.float64)
    tr = _session(eng, case)
    try:
        idx, y = _tables(case, list(range(case["U"])))
        live = tr.evaluate(idx, y, scores=True)
        tr.reserve_checkpoints(3)
        tr.snapshot(np.full(case["U"], 2, np.int32))
        slot = tr.evaluate(idx, y, source=2, scores=True)
        bare = tr.evaluate(idx, y)
    finally:
        tr.close()
    empty = np.isnan(want_s)
    for out in (live, slot):
        assert np.array_equal(np.isnan(out["scores"]), empty)
        err = float(np.abs(out["scores"][~empty] - want_s[~empty]).max())
        print(f"{name}: |dev - float64| score {err:.2e}")
        assert err <= BUDGET_SCORE
        for u in range(case["U"]):
            assert _counts(out, u) == want_c[u], (name, u)
    assert np.array_equal(live["scores"], slot["scores"], equal_nan=True)
    assert "scores" not in bare and all(_counts(bare, u) == want_c[u] for u in range(case["U"]))
    if name == A.HALF:
        assert np.all(live["scores"][~empty] == np.float32(0.5))
        assert live["neg_ge"][0] == live["n_neg"][0] > 0 and live["neg_gt"][0] == 0 and live["pos_gt"][0] == 0
    m = T_.metrics_from_counts(np.stack([[want_c[u][c] for c in A.COUNTS] for u in range(case["U"])]))
    for f in ("recall", "accuracy", "n_fp"):
        assert np.array_equal(live[f], m[f])


def test_eval_pool_can_be_replaced(eng):
    """a smaller pool, then a larger one (a new allocation), then a smaller one again (the same buffer): each call evaluates its own"""
    case = eval_case("fresh_n63")
    idx, y = case["idx"], case["y"]
    tr = _session(eng, case)
    try:
        base = tr.evaluate(idx, y, scores=True)
        half = case["pool"][:100]
        tr.set_eval_pool(half)
        with pytest.raises(OwwError):
            tr.evaluate(idx, y)                                                    # rows past the smaller pool are refused
        small = tr.evaluate(np.where(idx < 100, idx, -1), y, scores=True)
        keep = (idx < 100) & (idx >= 0)
        assert np.array_equal(small["scores"][keep], base["scores"][keep]) and np.isnan(small["scores"][~keep]).all()
        tr.set_eval_pool(np.concatenate([case["pool"], case["pool"]]))
        again = tr.evaluate(idx, y, scores=True)
        assert np.array_equal(again["scores"], base["scores"], equal_nan=True) and all(np.array_equal(again[c], base[c]) for c in A.COUNTS)
    finally:
        tr.close()


def test_bits_do_not_depend_on_company(eng):
    """a problem's scores and counts alone, as u = 0, 1, 2 of three, among 70, from host or device tables, in one call of 300 rows or in
    150 + 150 with the counts added"""
    import torch
    case = eval_case("spread_n300")

    def run(us, rows=slice(None), on_device=False, keep=None):
        sub = dict(case, U=len(us), init=case["init"][us])
        tr = _session(eng, sub)
        try:
            idx, y = np.ascontiguousarray(case["idx"][us][:, rows]), np.ascontiguousarray(case["y"][us][:, rows])
            if on_device:
                di, dy = torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda()
                torch.cuda.synchronize()
                out = tr.evaluate(di.data_ptr(), dy.data_ptr(), scores=True, on_device=True, shape=idx.shape)
            else:
                out = tr.evaluate(idx, y, scores=True)
        finally:
            tr.close()
        k = us.index(keep)
        return out["scores"][k], np.array([out[c][k] for c in A.COUNTS])

    for u in range(3):
        s0, c0 = run([u], keep=u)
        for us in ([0, 1, 2], [2, 1, 0], [(u + i) % 3 for i in range(70)]):
            s, c = run(us, keep=u)
            assert np.array_equal(s, s0, equal_nan=True) and np.array_equal(c, c0), (u, us[:3])
    s0, c0 = run([1], keep=1)
    s, c = run([0, 1, 2], on_device=True, keep=1)
    assert np.array_equal(s, s0, equal_nan=True) and np.array_equal(c, c0)
    sa, ca = run([1], rows=slice(0, 150), keep=1)
    sb, cb = run([1], rows=slice(150, 300), keep=1)
    assert np.array_equal(np.concatenate([sa, sb]), s0, equal_nan=True) and np.array_equal(ca + cb, c0)


# ---------------------------------------------------------------------------------------------------------------- snapshot and average
def _train_case():
    return R.make_case("fresh_u3")


def test_snapshot_keeps_the_record(eng):
    case = _train_case()
    U = case["U"]
    tr = T_.HeadTrainer(eng, case["T"], case["D"], U, init=[T_.record_to_head(r, case["T"], case["D"]) for r in case["init"]])
    try:
        tr.set_pool(case["pool"])
        tr.reserve_checkpoints(3)
        assert not tr.checkpoint_records(1).any()                                  # slots start at zero
        tr.steps(case["idx"][:, :4], case["y"][:, :4], case["lr"][:4], case["nw"][:4])
        at4 = tr.records()
        tr.snapshot([1, -1, 2])
        np.testing.assert_array_equal(tr.checkpoint_records(1)[0], at4[0])
        np.testing.assert_array_equal(tr.checkpoint_records(2)[2], at4[2])
        assert not tr.checkpoint_records(1)[1].any() and not tr.checkpoint_records(2)[1].any() and not tr.checkpoint_records(0).any()
        tr.steps(case["idx"][:, 4:], case["y"][:, 4:], case["lr"][4:], case["nw"][4:])
        assert not np.array_equal(tr.records()[0], at4[0])
        np.testing.assert_array_equal(tr.checkpoint_records(1)[0], at4[0])        # unchanged by later steps
        tr.snapshot([-1, -1, -1])
        np.testing.assert_array_equal(tr.checkpoint_records(1)[0], at4[0])
        np.testing.assert_array_equal(tr.checkpoint_records(2)[2], at4[2])
        heads = tr.checkpoint_heads(1)
        np.testing.assert_array_equal(T_.head_to_record(heads[0]), at4[0])
        final = tr.records()
    finally:
        tr.close()
    # the steps saw nothing of the snapshots: the same bits as a session without them
    tr = T_.HeadTrainer(eng, case["T"], case["D"], U, init=[T_.record_to_head(r, case["T"], case["D"]) for r in case["init"]])
    try:
        tr.set_pool(case["pool"])
        tr.steps(case["idx"], case["y"], case["lr"], case["nw"])
        np.testing.assert_array_equal(tr.records(), final)
    finally:
        tr.close()


@pytest.mark.parametrize("C", [1, 3])
def test_average_is_average_models(eng, C):
    """bit for bit average_ref: none, one, all, dst among the selected, a different selection per problem; evaluate(source = dst) is
    evaluate on a session opened with the averaged record"""
    case = _train_case()
    ev = eval_case("spread_n64")                                                  # T = 2, D = 16, as the training case
    assert (ev["T"], ev["D"]) == (case["T"], case["D"])
    U = case["U"]
    tr = T_.HeadTrainer(eng, case["T"], case["D"], U, init=[T_.record_to_head(r, case["T"], case["D"]) for r in case["init"]])
    try:
        tr.set_pool(case["pool"])
        tr.set_eval_pool(ev["pool"])
        tr.reserve_checkpoints(C)
        slots = []
        for c in range(C):
            tr.steps(case["idx"][:, 3 * c:3 * c + 3], case["y"][:, 3 * c:3 * c + 3], case["lr"][3 * c:3 * c + 3], case["nw"][3 * c:3 * c + 3])
            tr.snapshot(np.full(U, c, np.int32))
            slots.append(tr.records())
        tr.steps(case["idx"][:, 3 * C:], case["y"][:, 3 * C:], case["lr"][3 * C:], case["nw"][3 * C:])
        live = tr.records()
        slots = np.stack(slots)                                                    # [C, U, n]
        assert not np.array_equal(live, slots[-1])
        sels = [np.zeros((U, C), np.uint8), np.ones((U, C), np.uint8)]
        one = np.zeros((U, C), np.uint8); one[:, C - 1] = 1; sels.append(one)
        if C == 3:
            mixed = np.array([[0, 0, 0], [1, 0, 1], [0, 1, 1]], np.uint8); sels.append(mixed)
        for sel in sels:
            for dst in range(C):                                                   # dst among the selected, and not
                tr.average(sel, dst)
                got = tr.checkpoint_records(dst)
                for u in range(U):
                    pick = np.flatnonzero(sel[u])
                    want = A.average_ref([slots[c, u] for c in pick]) if pick.size else live[u]
                    assert np.array_equal(got[u].view(np.uint32), want.view(np.uint32)), (sel.tolist(), dst, u)
                keep = (got.copy(), tr.evaluate(ev["idx"], ev["y"], source=dst, scores=True))
                slots[dst] = got                                                   # the host's picture of the slots follows the device's
        last_records, last_out = keep
    finally:
        tr.close()
    t2 = T_.HeadTrainer(eng, case["T"], case["D"], U, init=[T_.record_to_head(r, case["T"], case["D"]) for r in last_records])
    try:
        t2.set_eval_pool(ev["pool"])
        fresh = t2.evaluate(ev["idx"], ev["y"], scores=True)
    finally:
        t2.close()
    assert np.array_equal(fresh["scores"], last_out["scores"], equal_nan=True)
    assert all(np.array_equal(fresh[c], last_out[c]) for c in A.COUNTS)


# ---------------------------------------------------------------------------------------------------------------- new_sequence
def test_new_sequence_resets_counters_and_keeps_moments(eng):
    """batches of 100 fire every second step; after 5 steps 100 samples are held.  With new_sequence the next step starts over (skip,
    fire, ...) and Adam carries on; kept counts, step / skip decisions and losses are the restatement's, and differ from a run
    without the call"""
    case = A.make_midacc_case()
    idx, y = T_.draw_tables(case["problems"], 12, 100, 4)
    lr, nw = np.full(12, 1e-3), np.linspace(1, 50, 12).astype(np.float32)

    def device(call):
        tr = T_.HeadTrainer(eng, 1, 16, 1, init=case["init_heads"])
        try:
            tr.set_pool(case["pool"])
            tr.steps(idx[:, :5], y[:, :5], lr[:5], nw[:5])
            if call:
                tr.new_sequence()
            tr.steps(idx[:, 5:], y[:, 5:], lr[5:], nw[5:])
            return tr.records()[0], tr.history["loss"][0], tr.history["kept"][0]
        finally:
            tr.close()

    def restated(call, dt, **kw):
        st = A.Stepper(case["init"][0], 1, 16, case["pool"], dt, **kw)
        got = []
        for k in range(12):
            if k == 5 and call:
                st.new_sequence()
            got.append(st.step(idx[0, k], y[0, k], lr[k], nw[k]))
        return st.record(), np.array([g[2] for g in got]), np.array([g[0] for g in got]), np.array([g[1] for g in got])

    rec, loss, kept = device(True)
    r_rec, r_loss, r_kept, r_step = restated(True, np.float64)
    assert r_step.tolist() == [False, True, False, True, False] + [False, True, False, True, False, True, False]
    np.testing.assert_array_equal(kept, r_kept)
    np.testing.assert_array_equal(~np.isnan(loss), r_step)
    assert np.abs(loss[r_step] / r_loss[r_step] - 1).max() <= 1e-4
    sub = dict(T=1, D=16)
    from test_head_train_cpu import budget_param
    assert R.rel_param_error(rec, r_rec, sub) <= budget_param(sub)
    # moments kept: a restatement that drops them at the call lands elsewhere
    st = A.Stepper(case["init"][0], 1, 16, case["pool"], np.float64)
    for k in range(12):
        if k == 5:
            st.new_sequence(("moments_reset_seq",))
        st.step(idx[0, k], y[0, k], lr[k], nw[k])
    assert R.rel_param_error(rec, st.record(), sub) > 100 * budget_param(sub)
    rec0, loss0, kept0 = device(False)
    assert (~np.isnan(loss0)).tolist() == [False, True] * 6
    assert not np.array_equal(np.isnan(loss0), np.isnan(loss)) and not np.array_equal(rec0, rec)


# ---------------------------------------------------------------------------------------------------------------- auto_train
@functools.lru_cache(maxsize=None)
def _bm():
    return BatchedModel(4, ["alexa"], weights={"heads": {"alexa": W.synthetic_head("alexa", 1234)}, "embedding": _emb()}, bank_slots=1,
                        bank_capacity=8)


@pytest.fixture(scope="module")
def bm():
    b = _bm()
    yield b
    b.close()


@functools.lru_cache(maxsize=None)
def _device_run(name):
    """auto_train on the case, once per module"""
    case, bm = e2e_case(name), _bm()
    heads, report = T_.auto_train(bm, case["pool"], case["problems"], case["val_pool"], (case["val_idx"], case["val_y"]), case["fp_idx"],
                                  steps=case["steps"], max_negative_weight=case["max_negative_weight"],
                                  target_fp_per_hour=case["target_fp_per_hour"], hidden=case["D"], n_batch=case["n_batch"], seed=case["seed"],
                                  init=case["init_heads"])
    return heads, report


@pytest.mark.parametrize("name", E2E)
def test_auto_train_decides_as_the_reference(bm, name):
    """every validation's histories, every checkpoint step, the selected set, both weight doublings and the fallback against the
    golden file (the reference's own fp32 run) and auto_train_ref in float64; the final record within the budget of float64"""
    case, r64, g = e2e_case(name), ref64_of(name), golden()
    heads, report = _device_run(name)
    assert [s["max_negative_weight"] for s in report["plan"]] == r64["weights"] == [1000, 2000, 4000]
    want = golden_entries(name, r64)
    for u in range(case["U"]):
        rp, k = report["problems"][u], f"{name}/{u}/"
        for f in ("val_recall", "val_accuracy", "val_n_fp", "val_fp_per_hr"):
            assert np.array_equal(rp[f], g[k + f]) and np.array_equal(rp[f], want[k + f]) and rp[f].dtype == g[k + f].dtype, (u, f)
        assert np.array_equal(np.asarray(rp["checkpoint_steps"], np.int32).reshape(-1, 2), g[k + "ckpt_at"]), u
        assert np.array_equal(np.asarray(rp["checkpoint_steps"], np.int32).reshape(-1, 2), want[k + "ckpt_at"]), u
        assert np.array_equal(np.asarray(rp["selected"], np.int32), g[k + "selected"]) and list(rp["selected"]) == list(r64["selected"][u]), u
        assert np.array_equal(rp["kept"], g[k + "kept"]) and np.array_equal(~np.isnan(rp["loss"]), g[k + "stepped"]), u
        assert np.array_equal(rp["counts"], g[k + "counts"]) and np.array_equal(rp["fp_counts"], g[k + "fp_counts"]), u
        rec = T_.head_to_record(heads[u])
        e64, eg = R.rel_param_error(rec, r64["params"][u], case), R.rel_param_error(rec, g[k + "params"], case)
        print(f"{name} u={u}: final record |dev - float64| {e64:.2e}, |dev - reference fp32| {eg:.2e} (budget {budget_param(name):.2e}); "
              f"{len(rp['checkpoint_steps'])} checkpoints, {len(rp['selected'])} selected")
        assert e64 <= budget_param(name), (name, u, e64)
        assert rp["combined"] == r64["combined"][u], u
        assert R.rel_param_error(rp["live_record"], r64["live"][u], case) <= budget_param(name), (name, u)
        if not rp["selected"]:                     # the fallback, exact: the live model as training left it, bit for bit
            assert np.array_equal(rec.view(np.uint32), rp["live_record"].view(np.uint32)), (name, u)
        else:
            assert not np.array_equal(rec, rp["live_record"]), (name, u)


def test_results_go_into_the_bank(bm):
    case = e2e_case("mixed_u3")
    heads, _ = _device_run("mixed_u3")
    ids = [bm.bank_add(h) for h in heads]
    got = bm.bank_score_features(case["val_pool"][:64], ids)                      # [64, 1, U]
    for u, h in enumerate(heads):
        want = O.head_stage(case["val_pool"][:64], h, dtype=np.float64)[:, 0]
        assert np.abs(got[:, 0, u] - want).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_session_untouched(eng):
    case = eval_case("spread_n300")
    U, P = case["U"], case["pool"].shape[0]
    for call in (eng.train_new_sequence, lambda: eng.train_set_eval_pool(case["pool"]), lambda: eng.train_checkpoints(2)):
        with pytest.raises(OwwError):
            call()                                                                 # no session
    with pytest.raises(ValueError):
        eng.train_eval(case["idx"], case["y"])
    tr = T_.HeadTrainer(eng, case["T"], case["D"], U, init=case["init_heads"])
    try:
        idx, y = case["idx"], case["y"]
        with pytest.raises(OwwError):
            tr.evaluate(idx, y)                                                    # no eval pool
        tr.set_eval_pool(case["pool"])
        base = tr.evaluate(idx, y, scores=True)
        for call in (lambda: tr.evaluate(idx, y, source=0), lambda: tr.snapshot(np.zeros(U, np.int32)),
                     lambda: tr.average(np.ones((U, 1), np.uint8), 0), lambda: tr.engine.train_get_slot(0, 0, tr.n_params)):
            with pytest.raises(OwwError):
                call()                                                             # no slots
        for bad_C in (0, -1, 65536):
            with pytest.raises(OwwError):
                tr.reserve_checkpoints(bad_C)
        tr.reserve_checkpoints(2)
        tr.snapshot(np.array([0, 1, 0], np.int32))
        before = [tr.checkpoint_records(c) for c in range(2)]
        bad = []
        i2 = idx.copy(); i2[1, 299] = P; bad.append(lambda: tr.evaluate(i2, y))
        i3 = idx.copy(); i3[0, 0] = -2; bad.append(lambda: tr.evaluate(i3, y))
        y2 = y.copy(); y2[2, 17] = 2; bad.append(lambda: tr.evaluate(idx, y2))
        bad += [lambda: tr.evaluate(idx, y, source=2), lambda: tr.evaluate(idx, y, source=-2),
                lambda: tr.snapshot(np.array([0, 2, 0], np.int32)), lambda: tr.snapshot(np.array([-2, 0, 0], np.int32)),
                lambda: tr.average(np.ones((U, 2), np.uint8), 2), lambda: tr.average(np.ones((U, 2), np.uint8), -1),
                lambda: tr.engine.train_get_slot(U, 0, tr.n_params), lambda: tr.engine.train_get_slot(0, 2, tr.n_params),
                lambda: tr.engine.train_get_slot(0, 0, tr.n_params - 1)]
        for call in bad:
            with pytest.raises(OwwError):
                call()
        with pytest.raises(ValueError):
            tr.snapshot(np.zeros(U + 1, np.int32))
        with pytest.raises(ValueError):
            tr.average(np.ones((U, 3), np.uint8), 0)
        for c in range(2):
            np.testing.assert_array_equal(tr.checkpoint_records(c), before[c])
        np.testing.assert_array_equal(tr.records(), case["init"])
        again = tr.evaluate(idx, y, scores=True)                                   # and a valid call gives the bits it gave
        assert np.array_equal(again["scores"], base["scores"], equal_nan=True) and all(np.array_equal(again[c], base[c]) for c in A.COUNTS)
        at0 = tr.evaluate(idx, y, source=0, scores=True)
        assert np.array_equal(at0["scores"][[0, 2]], base["scores"][[0, 2]], equal_nan=True)
    finally:
        tr.close()
    with pytest.raises(OwwError):
        eng.train_new_sequence()                                                   # the session is closed, its slots released
