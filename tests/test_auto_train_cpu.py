"""auto_train on the device, the tier that needs no GPU: admission of the case tables (tests/auto_train_ref.py), the float64 restatement
against the reference's own Model.auto_train cast to double, average_ref against average_models bit for bit, the switchable defects,
the fp32 floor the device's final record is held to, the committed golden file, the host layer (tests/auto_train_check.cpp:
owwhip_autotrain_host.h alone under AddressSanitizer / UBSan) and the policy functions of openwakeword_amd/train.py.

Admission: a case enters a table only if the reference in fp32 and in double, auto_train_ref in float64 and in fp32
under the four summation orders all give the same kept counts, step / skip decisions, five counts at every validation, checkpoint
steps and selected sets, and no float64 validation score lies within 16 x the largest |p_fp32 - p_float64| measured on that case of
0.5 (the exact-0.5 head is exempt: its p is 0.5f by construction in every arithmetic)."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from openwakeword_amd import train as T_

from test_pack_host_cpu import _host_clangxx
import auto_train_ref as A
import head_train_ref as R
from test_head_train_cpu import BUDGET_SCORE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = R.reference_train_module() is not None
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="the reference checkout is not on this machine")
E2E = [t[0] for t in A.E2E_TABLE]
EVAL = [t[0] for t in A.EVAL_TABLE]

# the reference's fp32 run against its double run on each end-to-end case, final record, relative max-abs per tensor
# (head_train_ref.rel_param_error), as measured (three digits, rounded up); test_fp32_floor holds each entry to a fresh measurement.
# The device's final record of a case is held to 8 x that case's own floor.
MEASURED_FLOOR = {"none_sel": 1.48e-6, "all_t16": 1.39e-6, "subset_t1": 9.57e-7, "mixed_u3": 2.70e-6, "varied_d32": 1.18e-6}


def budget_param(name):
    return 8 * MEASURED_FLOOR[name]


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    return A.make_e2e_case(name)


@functools.lru_cache(maxsize=None)
def ref64_of(name):
    return A.auto_train_ref(e2e_case(name), np.float64)


@functools.lru_cache(maxsize=None)
def ref32_of(name, order):
    return A.auto_train_ref(e2e_case(name), np.float32, order)


@functools.lru_cache(maxsize=None)
def torch_of(name, double):
    return A.run_reference_auto_train(e2e_case(name), double) if HAVE_REF else None


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(A.GOLDEN)
    return {k: z[k] for k in z.files}


def dp_of(name):
    """the largest |p_fp32 - p_float64| over the case's validation scores: the reference's two runs where it is here, else the restatement's"""
    a, b = (torch_of(name, False), torch_of(name, True)) if HAVE_REF else (ref32_of(name, 0), ref64_of(name))
    return max(float(np.abs(x - y).max()) for u in range(len(a["val_p"])) for x, y in zip(a["val_p"][u], b["val_p"][u]))


@functools.lru_cache(maxsize=None)
def _admit(name):
    """-> None when admitted, else the reason"""
    r64 = ref64_of(name)
    runs = {f"ref32/{o}": ref32_of(name, o) for o in range(4)}
    if HAVE_REF:
        runs.update({"reference fp32": torch_of(name, False), "reference double": torch_of(name, True)})
    bad = {k: A.same_run(r64, r) for k, r in runs.items()}
    bad = {k: v for k, v in bad.items() if v}
    if bad:
        return f"decisions differ from ref64: {bad}"
    if any(len(v) != 55 for v in r64["val_at"]):
        return "a validation is missing"
    dp, hm = dp_of(name), A.half_margin(r64)
    return None if hm >= 16 * dp else f"a float64 validation score lies {hm:.2e} from 0.5 (margin {16 * dp:.2e})"


# ---------------------------------------------------------------------------------------------------------------- the tables
def test_tables_cover_the_issue():
    t = A.EVAL_TABLE
    assert {c[1] for c in t} >= {16, 48, 128} and {c[2] for c in t} >= {1, 2, 16} and {c[3] for c in t} == {1, 3}
    assert {c[4] for c in t} >= {1, 63, 64, 65, 300} and {c[5] for c in t} >= {"fresh", "spread", "half", "saturate"}
    assert {c[6] for c in t} == {True, False}
    assert any((A.make_eval_case(n)["idx"] < 0).any() for n in EVAL)
    for n in E2E:
        c = e2e_case(n)
        assert c["steps"] == 200 and c["n_batch"] == 160 and c["val_idx"].shape[1] == 300 and c["fp_idx"].size == 2000


@pytest.mark.parametrize("name", E2E)
def test_e2e_case_is_admitted(name):
    assert _admit(name) is None, _admit(name)


def test_e2e_table_holds_the_roles():
    """some validations not checkpointed; nothing selected (the live model returned); a strict subset averaged; U = 3 deciding differently"""
    runs = {n: ref64_of(n) for n in E2E}
    per = [(n, u) for n in E2E for u in range(e2e_case(n)["U"])]
    assert any(len(runs[n]["ckpt_at"][u]) < 55 for n, u in per)
    none = [(n, u) for n, u in per if not runs[n]["selected"][u]]
    assert none and all(np.array_equal(runs[n]["params"][u], runs[n]["live"][u]) for n, u in none)
    assert any(0 < len(runs[n]["selected"][u]) < len(runs[n]["ckpt_at"][u]) for n, u in per)
    # and one whose recall, accuracy and false-positive histories all vary while its rules drop validations and pick a strict subset
    assert any(len(set(runs[n][f][u].tolist())) >= 3 for n, u in per for f in ("val_recall",)
               if len(runs[n]["ckpt_at"][u]) < 55 and 0 < len(runs[n]["selected"][u]) < len(runs[n]["ckpt_at"][u])
               and len(set(runs[n]["val_accuracy"][u].tolist())) >= 3 and len(set(runs[n]["val_fp_per_hr"][u].tolist())) >= 2)
    three = [n for n in E2E if e2e_case(n)["U"] == 3]
    assert three and all(len({(tuple(runs[n]["ckpt_at"][u]), tuple(runs[n]["selected"][u])) for u in range(3)}) == 3 for n in three)
    assert all(runs[n]["weights"] == [1000, 2000, 4000] for n in E2E)          # both doublings


@pytest.mark.parametrize("name", EVAL)
def test_eval_case_is_admitted(name):
    case = A.make_eval_case(name)
    c64, s64 = A.eval_case_ref(case, np.float64)
    c32, s32 = A.eval_case_ref(case, np.float32)
    assert c64 == c32
    if name == A.HALF:
        assert np.all(s32[~np.isnan(s32)] == 0.5) and all(c["neg_ge"] == c["n_neg"] and c["neg_gt"] == 0 and c["pos_gt"] == 0 for c in c32)
        return
    ok = ~np.isnan(s64)
    dp = float(np.abs(s32[ok] - s64[ok]).max())
    assert dp <= BUDGET_SCORE / 2                  # (a case on which fp32 arithmetic itself spends over half the score budget tests no kernel)
    assert float(np.abs(s64[ok] - 0.5).min()) >= 16 * dp
    if case["regime"] == "saturate":
        assert (s32[ok] == 0).any() and (s32[ok] == 1).any()
    if case["regime"] == "spread":
        assert (s64[ok] < 0.2).any() and (s64[ok] > 0.8).any()


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["fresh_n33", "accum_n127", "empty_dup", "fresh_u3"])
def test_stepper_is_ref_train(name):
    """the stateful step of auto_train_ref is head_train_ref.ref_train's, bit for bit, in float64 and in fp32 under every order"""
    case = R.make_case(name)
    for dt, orders in ((np.float64, (0,)), (np.float32, (0, 1, 2, 3))):
        for o in orders:
            want = R.ref_train(case, dt, order=o)
            for u in range(1 if o == 3 else case["U"]):          # (ref_train's shuffle generator runs on from problem to problem)
                st = A.Stepper(case["init"][u], case["T"], case["D"], case["pool"], dt, o)
                got = [st.step(case["idx"][u, k], case["y"][u, k], case["lr"][k], case["nw"][k]) for k in range(case["K"])]
                assert np.array_equal(st.record(), want["params"][u])
                assert [g[0] for g in got] == list(want["kept"][u]) and [g[1] for g in got] == list(want["steps"][u])
                assert np.array_equal(np.array([g[2] for g in got]), want["loss"][u], equal_nan=True)


@needs_ref
@pytest.mark.parametrize("name", E2E)
def test_ref64_is_the_reference_in_double(name):
    r64, t64 = ref64_of(name), torch_of(name, True)
    assert A.same_run(r64, t64) is None
    for u in range(e2e_case(name)["U"]):
        for f in ("val_recall", "val_accuracy", "val_n_fp", "val_fp_per_hr"):
            assert np.array_equal(r64[f][u], t64[f][u]) and r64[f][u].dtype == t64[f][u].dtype, f
        assert r64["combined"][u] == t64["combined"][u]
        stepped = r64["stepped"][u]
        np.testing.assert_allclose(r64["loss"][u][stepped], t64["loss"][u], rtol=1e-10)
        assert R.rel_param_error(r64["params"][u], t64["params"][u], e2e_case(name)) <= 1e-10
        assert R.rel_param_error(r64["live"][u], t64["live"][u], e2e_case(name)) <= 1e-10


@needs_ref
def test_fp32_floor():
    """the figure the device's final record is held to (8 x): measured here, written into DESIGN.md 5.39"""
    assert set(MEASURED_FLOOR) == set(E2E)
    for name in E2E:
        c = e2e_case(name)
        floor = max(R.rel_param_error(torch_of(name, False)["params"][u], torch_of(name, True)["params"][u], c) for u in range(c["U"]))
        print(f"{name}: reference fp32 against double, final record: {floor:.3e} (recorded {MEASURED_FLOOR[name]:.3e})")
        assert abs(floor / MEASURED_FLOOR[name] - 1) <= 0.02, name      # (2 %: another BLAS may sum in another order)
        for o in range(4):                         # the restatement's fp32 runs sit inside the budget the device gets
            assert max(R.rel_param_error(ref32_of(name, o)["params"][u], ref64_of(name)["params"][u], c) for u in range(c["U"])) <= budget_param(name)


@needs_ref
def test_average_ref_is_average_models():
    import torch
    tr = R.reference_train_module()
    T, D = 2, 32
    r = np.random.default_rng(11)
    recs = [T_.head_to_record(T_.init_head(T, D, 40 + i)) * np.float32(r.uniform(0.5, 30)) for i in range(5)]
    recs[1][7] = np.float32(-0.0)
    model = tr.Model(n_classes=1, input_shape=(T, 96), model_type="dnn", layer_dim=D, n_blocks=1)

    def net_of(rec):
        import copy
        n = copy.deepcopy(model.model)
        P_ = R.unpack(rec, T, D, np.float32)
        with torch.no_grad():
            for lin, w, b in ((n.layer1, "w1", "b1"), (n.blocks[0].fcn_layer, "w2", "b2"), (n.last_layer, "w3", "b3")):
                lin.weight.copy_(torch.from_numpy(P_[w].reshape(-1, lin.weight.shape[0]).T.copy()))
                lin.bias.copy_(torch.from_numpy(P_[b]))
            for ln, g, b in ((n.layernorm1, "g1", "be1"), (n.blocks[0].layer_norm, "g2", "be2")):
                ln.weight.copy_(torch.from_numpy(P_[g]))
                ln.bias.copy_(torch.from_numpy(P_[b]))
        return n

    def rec_of(n):
        out = {}
        for lin, w, b in ((n.layer1, "w1", "b1"), (n.blocks[0].fcn_layer, "w2", "b2"), (n.last_layer, "w3", "b3")):
            out[w], out[b] = lin.weight.detach().numpy().T.copy(), lin.bias.detach().numpy().copy()
        for ln, g, b in ((n.layernorm1, "g1", "be1"), (n.blocks[0].layer_norm, "g2", "be2")):
            out[g], out[b] = ln.weight.detach().numpy().copy(), ln.bias.detach().numpy().copy()
        return np.concatenate([out[f].ravel() for f in T_.FIELDS])

    for pick in ([0], [2, 4], [0, 1, 3], [0, 1, 2, 3, 4]):
        want = rec_of(model.average_models(models=[net_of(recs[i]) for i in pick]))
        got = A.average_ref([recs[i] for i in pick])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), pick


# ---------------------------------------------------------------------------------------------------------------- the defects
def _find(pred):
    for n in E2E:
        for u in range(e2e_case(n)["U"]):
            if pred(ref64_of(n), u):
                return n
    raise AssertionError("no case of the table shows this")


def test_defect_fp_gt_moves_the_exact_half_head():
    case = A.make_eval_case(A.HALF)
    good, _ = A.eval_case_ref(case, np.float32)
    bad, _ = A.eval_case_ref(case, np.float32, defects=("fp_gt",))
    assert good[0]["neg_ge"] == good[0]["n_neg"] > 0 and bad[0]["neg_ge"] == 0


def test_defect_counters_not_reset_moves_the_mid_accumulation_case():
    case = A.make_midacc_case()
    good = A.auto_train_ref(case, np.float64)
    assert good["stepped"][0][:50].tolist() == [False, True] * 25 and not good["stepped"][0][54]      # sequence 2 ends with samples held
    assert good["stepped"][0][55:].tolist() == [False, True] * 2 + [False]                             # sequence 3 starts from reset counters
    bad = A.auto_train_ref(case, np.float64, defects=("acc_not_reset_seq",))
    assert bad["stepped"][0][55] and not np.array_equal(good["stepped"][0], bad["stepped"][0])
    assert not np.array_equal(good["live"], bad["live"])


@pytest.mark.parametrize("defect,field", [("moments_reset_seq", "live"), ("val_before_step", "val_p"), ("step_gt1_dropped", "val_at"),
                                          ("no_weight_doubling", "weights")])
@pytest.mark.parametrize("name", E2E)
def test_defect_moves_every_case(name, defect, field):
    good, bad = ref64_of(name), A.auto_train_ref(e2e_case(name), np.float64, defects=(defect,))
    if field == "val_p":
        assert any(not np.array_equal(a, b) for a, b in zip(good[field][0], bad[field][0]))
    elif field == "live":
        assert not np.array_equal(good[field], bad[field])
    else:
        assert good[field] != bad[field] if field == "weights" else list(good[field][0]) != list(bad[field][0])
    if defect == "step_gt1_dropped":
        assert len(bad["val_at"][0]) == 57 and (1, 1) in bad["val_at"][0] and (2, 1) in bad["val_at"][0]
    if defect == "no_weight_doubling":
        assert bad["weights"] == [1000, 1000, 1000] and not np.array_equal(good["live"], bad["live"])


def test_defect_percentile_without_current_value():
    name = _find(lambda r, u: len(r["ckpt_at"][u]) < 55)
    moved = False
    for n in [name] + E2E:
        bad = A.auto_train_ref(e2e_case(n), np.float64, defects=("pct_without_current",))
        moved = moved or any(bad["ckpt_at"][u] != ref64_of(n)["ckpt_at"][u] for u in range(e2e_case(n)["U"]))
    assert moved


def test_defect_average_divided_first():
    name = _find(lambda r, u: 1 < len(r["selected"][u]))
    good, bad = ref32_of(name, 0), A.auto_train_ref(e2e_case(name), np.float32, 0, defects=("avg_divide_first",))
    assert A.same_run(good, bad) is None and not np.array_equal(good["params"], bad["params"])


def test_defect_fallback_returns_a_checkpoint():
    name = _find(lambda r, u: not r["selected"][u] and r["ckpt_at"][u])
    good, bad = ref64_of(name), A.auto_train_ref(e2e_case(name), np.float64, defects=("fallback_checkpoint",))
    u = next(u for u in range(e2e_case(name)["U"]) if not good["selected"][u])
    assert np.array_equal(good["params"][u], good["live"][u]) and not np.array_equal(bad["params"][u], good["params"][u])


# ---------------------------------------------------------------------------------------------------------------- the golden file
def golden_entries(name, run):
    """what tests/golden/auto_train.npz holds of one reference run (fp32): results only"""
    out = {}
    for u in range(len(run["kept"])):
        k = f"{name}/{u}/"
        for f in ("val_recall", "val_accuracy", "val_n_fp", "val_fp_per_hr", "kept", "stepped"):
            out[k + f] = np.asarray(run[f][u])
        out[k + "val_at"] = np.asarray(run["val_at"][u], np.int32).reshape(-1, 2)
        out[k + "ckpt_at"] = np.asarray(run["ckpt_at"][u], np.int32).reshape(-1, 2)
        out[k + "selected"] = np.asarray(run["selected"][u], np.int32)
        out[k + "counts"] = np.asarray([[c[f] for f in A.COUNTS] for c in run["counts"][u]], np.int32)
        out[k + "fp_counts"] = np.asarray(run["fp_counts"][u], np.int32)
        out[k + "params"] = np.asarray(run["params"][u], np.float32)
    return out


def test_golden_covers_the_table():
    g = golden()
    for name in A.GOLDEN_CASES:
        for u in range(e2e_case(name)["U"]):
            assert f"{name}/{u}/params" in g
    assert os.path.getsize(A.GOLDEN) < 1 << 20


@needs_ref
@pytest.mark.parametrize("name", A.GOLDEN_CASES)
def test_golden_is_reproducible(name):
    g = golden()
    for k, v in golden_entries(name, torch_of(name, False)).items():
        if k.endswith("params"):
            assert R.rel_param_error(v, g[k], e2e_case(name)) <= budget_param(name), k      # (another BLAS may sum in another order)
        else:
            assert np.array_equal(v, g[k]) and v.dtype == g[k].dtype, k


@pytest.mark.parametrize("name", A.GOLDEN_CASES)
def test_golden_agrees_with_ref64(name):
    g, r64 = golden(), ref64_of(name)
    for k, v in golden_entries(name, r64).items():
        if k.endswith("params"):
            assert R.rel_param_error(g[k], v, e2e_case(name)) <= budget_param(name), k
        elif k.endswith("val_recall") or k.endswith("val_accuracy") or k.endswith("val_fp_per_hr") or k.endswith("val_n_fp"):
            assert np.array_equal(v, g[k]), k
        else:
            assert np.array_equal(v, g[k]), k


# ---------------------------------------------------------------------------------------------------------------- the policy in train.py
def test_plan_is_the_reference_schedule():
    plan = T_.auto_train_plan(200)
    assert [s["n_steps"] for s in plan] == [20 * 10, 20, 20] and [s["max_negative_weight"] for s in plan] == [1000, 2000, 4000]
    assert [len(s["val_steps"]) for s in plan] == [19, 18, 18] and plan[0]["val_steps"][0] == 150 and plan[1]["val_steps"] == list(range(2, 20))
    for s, (n, max_steps, lr, weights, val_steps, w) in zip(plan, A.sequences(dict(steps=200, max_negative_weight=1000, target_fp_per_hour=0.2))):
        want = [float(T_.lr_warmup_cosine_decay(k, warmup_steps=max_steps // 5, hold=max_steps // 3, total_steps=max_steps, target_lr=lr)) for k in range(n)]
        assert s["lr"].tolist() == want and s["neg_weight"].tolist() == np.asarray(weights, np.float32).tolist()
    assert [s["max_negative_weight"] for s in T_.auto_train_plan(200, target_fp_per_hour=1000)] == [1000, 1000, 1000]
    big = T_.auto_train_plan(400000)               # int16 wraps above 32,767: the late validation steps of sequence 2 go negative and never match
    assert len(big[1]["val_steps"]) < 18
    for bad in (205, 40, 0):
        with pytest.raises(ValueError):
            T_.auto_train_plan(bad)


def test_metrics_from_counts():
    m = T_.metrics_from_counts(np.array([[3, 7, 2, 1, 2], [0, 4, 0, 0, 0]], np.int32))
    assert m["recall"].dtype == np.float32 and m["recall"].tolist() == [np.float32(2) / np.float32(3), 0.0]
    assert m["accuracy"].tolist() == [np.float32(8) / np.float32(10), 1.0] and m["n_fp"].tolist() == [2, 0]
    for e in (dict(n_pos=3, n_neg=7, pos_gt=2, neg_gt=1, neg_ge=2),):
        rec, acc, nfp = A.metrics(e)
        assert (rec, acc, nfp) == (m["recall"][0], m["accuracy"][0], m["n_fp"][0])


def test_keep_and_select_rules():
    assert T_.keep_checkpoint([np.int64(3)], [np.float32(0.5)])                                   # the first validation always passes
    assert not T_.keep_checkpoint([np.int64(1), np.int64(1), np.int64(3)], [np.float32(0.5)] * 3)
    assert not T_.keep_checkpoint([np.int64(1)] * 30, [np.float32(0.9)] * 29 + [np.float32(0.1)])
    hist = dict(val_accuracy=[np.float32(v) for v in (0.5, 0.9, 0.9)], val_recall=[np.float32(v) for v in (0.5, 0.9, 0.9)],
                val_fp_per_hr=[np.float32(v) for v in (2, 0, 0)])
    scores = [dict(val_accuracy=h, val_recall=r, val_fp_per_hr=f) for h, r, f in zip(hist["val_accuracy"], hist["val_recall"], hist["val_fp_per_hr"])]
    assert T_.select_checkpoints(hist, scores) == [1, 2]


# ---------------------------------------------------------------------------------------------------------------- the host layer
def _check_exe():
    cxx = _host_clangxx()
    if cxx is None or not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    d = tempfile.mkdtemp(prefix="auto_train_check")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "auto_train_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "auto_train_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    return exe, d


EINVAL, ESTATE = -1, -3
MAXROWS = 1 << 20
#              name        open P        EP   C      U      T   D    src n        sh tables sc Cnew   slots dst gu gslot gn
HOST_CASES = [("plain",     1,  300,     300, 55,    3,     2,  32,  -1, 300,     0, "ok",  1, 55,    "ok", 0,  2, 54,  0),
              ("shared",    1,  2300,    2300, 3,    70,    16, 128, 2,  65,      1, "ok",  0, 1,     "ok", 2,  69, 0,  0),
              ("edges",     1,  1,       1,   65535, 3,     1,  16,  65534, 1,    1, "ok",  1, 65535, "ok", 65534, 2, 65534, 0),
              ("many",      1,  7,       7,   1,     65535, 1,  16,  0,  1,       1, "ok",  0, 1,     "ok", 0,  65534, 0, 0),
              ("maxrows",   1,  5,       5,   1,     1,     34, 48,  -1, MAXROWS, 0, "ok",  1, 1,     "ok", 0,  0, 0,   0),
              ("nosession", 0,  300,     300, 55,    3,     2,  32,  -1, 300,     0, "ok",  1, 55,    "ok", 0,  0, 0,   0),
              ("nopool",    1,  0,       0,   55,    3,     2,  32,  -1, 300,     0, "ok",  1, 55,    "ok", 0,  0, 0,   0),
              ("noslots",   1,  300,     300, 0,     3,     2,  32,  0,  300,     0, "ok",  1, 0,     "ok", 0,  0, 0,   0),
              ("src_hi",    1,  300,     300, 5,     3,     2,  32,  5,  300,     0, "ok",  1, 65536, "hi", 5,  3, 5,   0),
              ("src_lo",    1,  300,     300, 5,     3,     2,  32,  -2, 300,     0, "ok",  1, -1,    "lo", -1, -1, -1, 0),
              ("n_hi",      1,  1 << 31, 300, 5,     3,     2,  32,  -1, MAXROWS + 1, 0, "ok", 1, 5,  "ok", 0,  0, 0,   7),
              ("n_lo",      1,  -1,      300, 5,     3,     2,  32,  -1, 0,       0, "ok",  1, 5,     "ok", 0,  0, 0,   0),
              ("idx_hi",    1,  300,     300, 5,     3,     2,  32,  -1, 300,     0, "hi",  1, 5,     "ok", 0,  0, 0,   0),
              ("idx_lo",    1,  300,     300, 5,     3,     2,  32,  -1, 300,     1, "lo",  1, 5,     "ok", 0,  0, 0,   0),
              ("label",     1,  300,     300, 5,     3,     2,  32,  4,  65,      0, "lab", 0, 5,     "ok", 0,  0, 0,   0),
              ("largest",   1,  1 << 62, 300, 5,     65535, 34, 128, -1, 64,      1, "ok",  0, 65535, "ok", 0,  0, 0,   0)]


def _expected(c):
    name, open_, P, EP, C, U, T, D, src, n, sh, tables, sc, Cnew, slots, dst, gu, gslot, gn = c
    F = 96 * T
    n_par = T_.param_count(T, D)
    stride = (n_par + 3) // 4 * 4
    no = None if open_ else ESTATE
    seq = no or 0
    pool = no or (EINVAL if P < 1 or P > 2 ** 31 - 1 or P > (2 ** 63 - 1) // 4 // F else 0)
    if not open_ or EP < 1:
        ev = ESTATE
    elif src < -1:
        ev = EINVAL
    elif src >= 0 and C < 1:
        ev = ESTATE
    elif src >= C and src >= 0:
        ev = EINVAL
    elif n < 1 or n > MAXROWS:
        ev = EINVAL
    else:
        ev = EINVAL if tables != "ok" else 0
    if not open_:
        ck = ESTATE
    elif Cnew < 1 or Cnew > 65535 or U * stride > (2 ** 63 - 1) // 4 // Cnew:
        ck = EINVAL
    else:
        ck = 0
    snap = no or (ESTATE if C < 1 else EINVAL if slots != "ok" else 0)
    avg = no or (ESTATE if C < 1 else EINVAL if not 0 <= dst < C else 0)
    get = no or (ESTATE if C < 1 else EINVAL if not 0 <= gu < U or not 0 <= gslot < C or gn else 0)
    lines = [f"case {name} seq {seq} epool {pool} eval {ev} ckpt {ck} snap {snap} avg {avg} get {get}"]
    if ev == 0:
        lines.append(f"plan {(n + 63) // 64} {(1 if sh else U) * n} {U * n if sc else 0}")
    if ck == 0:
        lines.append(f"slots {Cnew * U * stride}")
    return lines


def test_host_layer_under_sanitizers():
    exe, d = _check_exe()
    path = os.path.join(d, "cases.txt")
    with open(path, "w") as f:
        for c in HOST_CASES:
            f.write(" ".join(str(v) for v in c) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    blocks = re.split(r"(?m)^(?=case )", run.stdout)[1:]
    assert len(blocks) == len(HOST_CASES)
    for c, blk in zip(HOST_CASES, blocks):
        assert blk.strip().splitlines() == _expected(c), c[0]


def test_every_new_symbol_has_a_prototype():
    from openwakeword_amd import _lib
    text = open(os.path.join(ROOT, "include", "owwhip.h")).read()
    names = set(re.findall(r"\b(oww_train_\w+)\s*\(", text))
    assert names >= {"oww_train_new_sequence", "oww_train_set_eval_pool", "oww_train_eval", "oww_train_checkpoints", "oww_train_snapshot",
                     "oww_train_average", "oww_train_get_slot"}
    assert names <= set(_lib.SYMBOLS)
