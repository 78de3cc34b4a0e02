"""Training bank heads on the device, the tier that needs no GPU: the float64 definition (tests/head_train_ref.py: ref64) against the
reference's own train.Model cast to double, admission of the case table, the budget the device is held to, the switchable defects
of the fp32 restatement, the committed golden file, the host layer (tests/train_check.cpp: owwhip_train_host.h alone under
AddressSanitizer / UBSan) and the Python layer around the session.

Bounds.  ref64 against the reference in double: 1e-10 relative in every parameter tensor (largest seen 5.6e-13).  The budget of the
device: 8 x the largest distance of an fp32 run (torch's own, and the restatement under its four summation orders) from ref64 over
the admitted table, the margin this project gives fp32 floors elsewhere, taken per shape class -- the measured values stand beside the constants.  The
selection margin: 16 x the largest |p_fp32 - p_ref64| seen over the admitted table."""
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
from openwakeword_amd import weights as W
from openwakeword_amd.model import check_bank_head

from test_pack_host_cpu import _host_clangxx
import head_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [t[0] for t in R.TABLE]

# fp32 against ref64 over the admitted table (saturation case apart), measured per shape class, so that the 8 x margin means the same
# for every case.  Parameters: the wide class (T = 16 with D = 128: 196,608 W1 elements, where Adam's g / (|g| + eps) amplifies
# rounding on the many gradient elements near eps) 2.60e-4; every other shape 2.05e-5 (fresh_d112; the issue's own shapes <= 1.7e-5).
# Scores of the 64 probe windows, all shapes: 4.5e-7.
MEASURED_PARAM = {"wide": 2.7e-4, "rest": 2.1e-5}
MEASURED_SCORE = 5.0e-7
BUDGET_SCORE = 8 * MEASURED_SCORE


def shape_class(case):
    return "wide" if (case["T"], case["D"]) == (16, 128) else "rest"


def budget_param(case):
    return 8 * MEASURED_PARAM[shape_class(case)]


# |p_fp32 - p_ref64| over the admitted table, measured: 2.6e-7 (fresh cases), 1.59e-6 at the x 8 output layer
MEASURED_DP = 1.6e-6
P_MARGIN = 16 * MEASURED_DP
HAVE_REF = R.reference_train_module() is not None


@functools.lru_cache(maxsize=None)
def case_of(name):
    return R.make_case(name)


@functools.lru_cache(maxsize=None)
def ref64_of(name):
    return R.ref_train(case_of(name), np.float64)


@functools.lru_cache(maxsize=None)
def ref32_of(name, order):
    return R.ref_train(case_of(name), np.float32, order=order)


@functools.lru_cache(maxsize=None)
def torch32_of(name):
    return R.run_reference(case_of(name)) if HAVE_REF else None


@functools.lru_cache(maxsize=None)
def golden():
    """the committed reference runs: name -> dict(params, loss, kept)"""
    z = np.load(R.GOLDEN)
    return {n: dict(params=z[n + "/params"], loss=z[n + "/loss"], kept=z[n + "/kept"]) for n in R.GOLDEN_CASES}


def _p_margin(name):
    return min(float(np.minimum(np.abs(p - 0.001), np.abs(p - 0.999)).min()) for p in ref64_of(name)["p"].values() if p.size)


@functools.lru_cache(maxsize=None)
def _admit(name):
    """-> None when admitted, else the reason"""
    r64 = ref64_of(name)
    runs = {f"ref32/{o}": ref32_of(name, o) for o in range(4)}
    if name == R.SATURATION:                       # judged against the fp32 golden alone: float64 does not saturate there
        g = golden()[name]
        bad = [k for k, r in runs.items() if not (np.array_equal(r["kept"], g["kept"]) and np.array_equal(r["steps"], ~np.isnan(g["loss"])))]
        return f"decisions differ from the golden in {bad}" if bad else None
    bad = [k for k, r in runs.items() if not R.same_decisions(r64, r)]
    t32 = torch32_of(name)
    if t32 is not None and not R.same_decisions(r64, t32):
        bad.append("reference fp32")
    if name in golden():
        g = golden()[name]
        if not (np.array_equal(r64["kept"], g["kept"]) and np.array_equal(r64["steps"], ~np.isnan(g["loss"]))):
            bad.append("golden")
    if bad:
        return f"decisions differ from ref64 in {bad}"
    pm = _p_margin(name)
    return None if pm >= P_MARGIN else f"a ref64 p lies {pm:.2e} from a selection threshold (margin {P_MARGIN:.2e})"


def admitted_cases():
    return [n for n in NAMES if _admit(n) is None]


def test_case_table_covers_the_issue():
    t = R.TABLE
    assert {c[1] for c in t} >= {16, 32, 48, 112, 128} and {c[2] for c in t} >= {1, 2, 16}
    assert {c[3] for c in t} >= {1, 33, 127, 128, 129, 300} and {c[4] for c in t} >= {1, 2, 12, 40} and {c[5] for c in t} == {1, 3}
    assert all(case_of(n)["pool"].shape[0] <= 600 for n in NAMES)
    assert {c[6] for c in t} >= {"fresh", "trained", "alldrop", "saturated", "dead", "empty_dup", "faint"}
    assert all(case_of(n)["lr"][0] == 0 for n in NAMES)
    c = case_of("ramp_k40")
    assert c["nw"][0] == 1 and c["nw"][-1] == 1500
    c = case_of("empty_dup")
    assert (c["idx"] == -1).any() and any(np.unique(row[row >= 0]).size < (row >= 0).sum() for row in c["idx"][0])
    r = ref64_of("alldrop")
    assert (r["kept"][0, :5] == 0).all() and r["steps"].any()
    r = ref64_of("accum_n127")
    assert not r["steps"][0, 0] and r["steps"][0, 1]
    r = ref64_of("trained_k12")
    assert (r["kept"] < 129).any()
    c = case_of("dead_relu")
    X = c["pool"].reshape(c["pool"].shape[0], -1)
    assert (R.forward(R.unpack(ref64_of("dead_relu")["params"][0], c["T"], c["D"], np.float64), X, np.float64)["h1"][:, 3] == 0).all()


def test_admission():
    """a case stays only if the reference's fp32 run, ref64 and ref32 under all four orders make the same decisions at every step, and no
    ref64 p lies inside the selection margin; at most one case in ten is dropped"""
    reasons = {n: _admit(n) for n in NAMES}
    dropped = {n: r for n, r in reasons.items() if r is not None}
    print("dropped by admission:", dropped or "none")
    assert len(dropped) * 10 <= len(NAMES), dropped
    assert R.SATURATION in admitted_cases()
    dp = 0.0
    for n in admitted_cases():
        if n == R.SATURATION:
            continue
        r64 = ref64_of(n)
        for r in [ref32_of(n, o) for o in range(4)] + ([torch32_of(n)] if HAVE_REF else []):
            dp = max(dp, max(float(np.abs(np.asarray(r["p"][k], np.float64) - r64["p"][k]).max()) for k in r64["p"] if r64["p"][k].size))
    print(f"largest |p_fp32 - p_ref64| over the admitted table: {dp:.3g} (MEASURED_DP {MEASURED_DP:g})")
    assert dp <= MEASURED_DP


def test_saturation_case_saturates():
    c = case_of(R.SATURATION)
    r32, r64 = ref32_of(R.SATURATION, 0), ref64_of(R.SATURATION)
    assert r32["p"][0, 0][0] == 1.0 and r32["sets"][0, 0][0] and r64["p"][0, 0][0] < 1.0       # kept, at exactly 1.0f
    assert all((p[1:] < 1.0).all() for p in r32["p"].values())
    g = golden()[R.SATURATION]
    assert R.rel_param_error(r32["params"][0], g["params"][0], c) <= budget_param(c)
    assert R.rel_param_error(r64["params"][0], g["params"][0], c) > budget_param(c)               # float64 is no yardstick here


@pytest.mark.skipif(not HAVE_REF, reason="the reference checkout is not on this machine")
@pytest.mark.parametrize("name", NAMES)
def test_ref64_is_the_reference_in_double(name):
    c = case_of(name)
    t64 = R.run_reference(c, double=True)
    r64 = ref64_of(name)
    assert R.same_decisions(r64, t64)
    err = max(R.rel_param_error(r64["params"][u], t64["params"][u], c) for u in range(c["U"]))
    print(f"{name}: ref64 against train.Model in double: {err:.2e}")
    assert err <= 1e-10
    st = r64["steps"]
    np.testing.assert_allclose(r64["loss"][st], t64["loss"][st], rtol=1e-10)


def test_budget_measured():
    """the distance of every fp32 run from ref64 after each admitted case's K steps: what the budget is 8 x of"""
    worst_p, worst_s = {"wide": 0.0, "rest": 0.0}, 0.0
    for n in admitted_cases():
        if n == R.SATURATION:
            continue
        c, r64 = case_of(n), ref64_of(n)
        recs = [ref32_of(n, o)["params"] for o in range(4)]
        if HAVE_REF:
            recs.append(torch32_of(n)["params"])
        elif n in golden():
            recs.append(golden()[n]["params"])
        for rec in recs:
            for u in range(c["U"]):
                worst_p[shape_class(c)] = max(worst_p[shape_class(c)], R.rel_param_error(rec[u], r64["params"][u], c))
                worst_s = max(worst_s, float(np.abs(R.score(rec[u], c) - R.score(r64["params"][u], c)).max()))
    print(f"fp32 against ref64, largest over the admitted table: parameters {worst_p} (MEASURED_PARAM {MEASURED_PARAM}), "
          f"scores {worst_s:.3g} (MEASURED_SCORE {MEASURED_SCORE:g})")
    assert all(worst_p[k] <= MEASURED_PARAM[k] for k in worst_p) and worst_s <= MEASURED_SCORE


def test_golden_is_within_budget_of_ref64():
    for n in R.GOLDEN_CASES:
        if n == R.SATURATION or _admit(n) is not None:
            continue
        c, g, r64 = case_of(n), golden()[n], ref64_of(n)
        np.testing.assert_array_equal(g["kept"], r64["kept"])
        for u in range(c["U"]):
            assert R.rel_param_error(g["params"][u], r64["params"][u], c) <= MEASURED_PARAM[shape_class(c)], n


@pytest.mark.skipif(not HAVE_REF, reason="the reference checkout is not on this machine")
def test_golden_is_reproducible(tmp_path):
    out = str(tmp_path / "again.npz")
    run = subprocess.run([os.sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_train.py"), out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    a, b = np.load(out), np.load(R.GOLDEN)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


DEFECT_CASE = {"bias_k": "fresh_n33", "eps_in_sqrt": "faint_pos", "mean_n": "trained_k12", "negw_on_pos": "fresh_u3", "acc_not_divided": "fresh_n33",
               "acc_not_reset": "accum_n127", "p_minus_y": R.SATURATION, "ln_no_means": "fresh_u3", "relu_prenorm": "dead_relu",
               "pad_not_zeroed": "fresh_n33", "empty_slot_read": "empty_dup", "negw_by_opt": "accum_n127", "idx_problem0": "fresh_u3", "moments_frozen_lr0": "ramp_k40"}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_moves_its_case_beyond_the_budget(defect):
    n = DEFECT_CASE[defect]
    c = case_of(n)
    bad = R.ref_train(c, np.float32, order=0, defects=(defect,))
    want = golden()[n]["params"] if n == R.SATURATION else ref64_of(n)["params"]
    ep = max(R.rel_param_error(bad["params"][u], want[u], c) for u in range(c["U"]))
    es = max(float(np.abs(R.score(bad["params"][u], c) - R.score(want[u], c)).max()) for u in range(c["U"]))
    print(f"{defect} on {n}: parameters {ep:.2e} (budget {budget_param(c):.1e}), scores {es:.2e} (budget {BUDGET_SCORE:.1e})")
    if defect == "acc_not_divided":
        # Adam's update is invariant to the gradient's scale but for eps (measured here: parameters 6.2e-6, scores 3.9e-8, inside the
        # budget), so no parameter bound can see this defect; the loss record does: it is acc_steps (here 4) times too large, against
        # the 1e-4 the GPU tier holds the recorded losses to
        st = ref64_of(n)["steps"]
        assert np.abs(bad["loss"][st] / ref64_of(n)["loss"][st] - 1).max() > 1e-4
        return
    assert ep > budget_param(c) and es > BUDGET_SCORE


# ---- the host layer ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_check_exe():
    cxx = _host_clangxx()
    if cxx is None or not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    d = tempfile.mkdtemp(prefix="train_check")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "train_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "train_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    return exe, d


EINVAL, ESTATE = -1, -3
#              name         com open U      T   D    TR  P        K     n     sh tables lr      nw       -> begin, pool, steps
HOST_CASES = [("plain",      1,  0,  3,     2,  32,  16, 600,     12,   129,  0, "ok",  "1e-3", "1",     0, 0, 0),
              ("shared",     1,  0,  70,    16, 128, 16, 600,     40,   300,  1, "ok",  "0",    "1500",  0, 0, 0),
              ("edges",      1,  0,  65535, 1,  16,  34, 1,       4096, 4096, 1, "ok",  "1e-3", "0",     0, 0, 0),
              ("n1",         1,  0,  1,     34, 48,  34, 5,       1,    1,    0, "ok",  "1e-3", "1",     0, 0, 0),
              ("uncommitted", 0, 0,  1,     1,  32,  16, 10,      1,    1,    0, "ok",  "1e-3", "1",     ESTATE, -99, -99),
              ("second",     1,  1,  1,     1,  32,  16, 10,      1,    1,    0, "ok",  "1e-3", "1",     ESTATE, -99, -99),
              ("u0",         1,  0,  0,     1,  32,  16, 10,      1,    1,    0, "ok",  "1e-3", "1",     EINVAL, -99, -99),
              ("u_big",      1,  0,  65536, 1,  32,  16, 10,      1,    1,    0, "ok",  "1e-3", "1",     EINVAL, -99, -99),
              ("d24",        1,  0,  1,     1,  24,  16, 10,      1,    1,    0, "ok",  "1e-3", "1",     EINVAL, -99, -99),
              ("d144",       1,  0,  1,     1,  144, 16, 10,      1,    1,    0, "ok",  "1e-3", "1",     EINVAL, -99, -99),
              ("d0",         1,  0,  1,     1,  0,   16, 10,      1,    1,    0, "ok",  "1e-3", "1",     EINVAL, -99, -99),
              ("t0",         1,  0,  1,     0,  32,  16, 10,      1,    1,    0, "ok",  "1e-3", "1",     EINVAL, -99, -99),
              ("t17",        1,  0,  1,     17, 32,  16, 10,      1,    1,    0, "ok",  "1e-3", "1",     EINVAL, -99, -99),
              ("p0",         1,  0,  1,     1,  32,  16, 0,       1,    1,    0, "ok",  "1e-3", "1",     0, EINVAL, -99),
              ("p_big",      1,  0,  1,     1,  32,  16, 1 << 31, 1,    1,    0, "ok",  "1e-3", "1",     0, EINVAL, -99),
              ("k0",         1,  0,  2,     1,  32,  16, 10,      0,    8,    0, "ok",  "1e-3", "1",     0, 0, EINVAL),
              ("k4097",      1,  0,  2,     1,  32,  16, 10,      4097, 8,    0, "ok",  "1e-3", "1",     0, 0, EINVAL),
              ("n0",         1,  0,  2,     1,  32,  16, 10,      4,    0,    0, "ok",  "1e-3", "1",     0, 0, EINVAL),
              ("n4097",      1,  0,  2,     1,  32,  16, 10,      4,    4097, 0, "ok",  "1e-3", "1",     0, 0, EINVAL),
              ("idx_hi",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "hi",  "1e-3", "1",     0, 0, EINVAL),
              ("idx_lo",     1,  0,  2,     1,  32,  16, 10,      4,    8,    1, "lo",  "1e-3", "1",     0, 0, EINVAL),
              ("label2",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "lab", "1e-3", "1",     0, 0, EINVAL),
              ("lr_nan",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "ok",  "nan",  "1",     0, 0, EINVAL),
              ("lr_inf",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "ok",  "inf",  "1",     0, 0, EINVAL),
              ("lr_neg",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "ok",  "-1e-9", "1",    0, 0, EINVAL),
              ("nw_nan",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "ok",  "1e-3", "nan",   0, 0, EINVAL),
              ("nw_inf",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "ok",  "1e-3", "inf",   0, 0, EINVAL),
              ("nw_neg",     1,  0,  2,     1,  32,  16, 10,      4,    8,    0, "ok",  "1e-3", "-1",    0, 0, EINVAL)]


def _expected(case):
    name, com, opn, U, T, D, TR, P, K, n, sh, tables, lr, nw, rb, rp, rs = case
    lines = [f"case {name} begin {rb} pool {rp} steps {rs}"]
    if rb:
        return lines
    F = 96 * T
    off, o = [], 0
    for _, shape in T_.record_shapes(T, D):
        off.append(o)
        o += int(np.prod(shape))
    assert o == T_.param_count(T, D)
    lines.append("layout " + " ".join(str(v) for v in [F, D] + off + [o, (o + 3) // 4 * 4, o - F * D]))
    if rs:
        return lines
    nt = (n + 63) // 64
    lines.append(f"plan {nt} {nt * 64} {U * nt * 64 * D} {U * nt * (o - F * D)} {U * nt} {(F + 63) // 64}")
    return lines


def test_host_layer_under_sanitizers():
    exe, d = _train_check_exe()
    path = os.path.join(d, "cases.txt")
    with open(path, "w") as f:
        for c in HOST_CASES:
            f.write(" ".join(str(v) for v in c[:14]) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    blocks = re.split(r"(?m)^(?=case )", run.stdout)[1:]
    assert len(blocks) == len(HOST_CASES)
    for c, blk in zip(HOST_CASES, blocks):
        assert blk.strip().splitlines() == _expected(c), c[0]


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
def test_symbols_and_record_layout():
    from openwakeword_amd import _lib
    for s in ("oww_train_param_count", "oww_train_begin", "oww_train_set_pool", "oww_train_steps", "oww_train_get", "oww_train_end"):
        assert s in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.oww_abi_version() == 6
    for T, D in ((1, 16), (2, 32), (16, 128), (34, 48)):
        assert lib.oww_train_param_count(T, D) == T_.param_count(T, D)
    assert lib.oww_train_param_count(1, 24) == 0 and lib.oww_train_param_count(0, 32) == 0


def test_heads_and_records_round_trip():
    for T, D in ((1, 16), (16, 32), (2, 128)):
        h = T_.init_head(T, D, 3)
        check_bank_head(h, 16)
        rec = T_.head_to_record(h)
        assert rec.size == T_.param_count(T, D)
        back = T_.record_to_head(rec, T, D)
        check_bank_head(back, 16)
        np.testing.assert_array_equal(T_.head_to_record(back), rec)
        b1 = 1 / np.sqrt(96 * T)
        assert np.abs(h["net"]["w1"]).max() <= b1 and np.abs(h["net"]["w1"]).max() > 0.9 * b1 and np.abs(h["net"]["b2"]).max() <= 1 / np.sqrt(D)
        assert (h["net"]["ln1"][0] == 1).all() and (h["net"]["ln2"][1] == 0).all()
    s = W.synthetic_head("x", 1, hidden=32, layernorm=True, T=16)
    np.testing.assert_array_equal(T_.record_to_head(T_.head_to_record(s), 16, 32)["net"]["w2"], s["net"]["w2"])
    with pytest.raises(ValueError):
        T_.head_to_record(W.synthetic_head("x", 1, hidden=32, layernorm=False, T=16))


@pytest.mark.skipif(not HAVE_REF, reason="the reference checkout is not on this machine")
def test_schedules_restate_the_reference():
    tr = R.reference_train_module()
    m = tr.Model(n_classes=1, input_shape=(16, 96), model_type="dnn", layer_dim=32, n_blocks=1)
    for K, warm, hold in ((50, 10, 16), (12, 2, 4), (7, 1, 0)):
        for k in range(K):
            assert float(T_.lr_warmup_cosine_decay(k, warm, hold, K, target_lr=1e-3)) == float(m.lr_warmup_cosine_decay(k, warm, hold, K, target_lr=1e-3))
    assert T_.negative_weight_schedule(50, 1500) == np.linspace(1, 1500, 50).tolist()


def test_draw_tables_is_seeded():
    probs = [(np.arange(0, 50), np.arange(50, 200)), (np.arange(10, 20), np.arange(300, 400))]
    a, b = T_.draw_tables(probs, 5, 33, seed=4), T_.draw_tables(probs, 5, 33, seed=4)
    np.testing.assert_array_equal(a[0], b[0])
    idx, y = a
    assert idx.shape == (2, 5, 33) and y.sum() == 2 * 5 * 16
    assert np.isin(idx[0][y[0] == 1], probs[0][0]).all() and np.isin(idx[1][y[1] == 0], probs[1][1]).all()
    assert not np.array_equal(idx, T_.draw_tables(probs, 5, 33, seed=5)[0])


def test_tables_come_in_chunks_that_make_up_draw_tables(monkeypatch):
    """train_heads draws a chunk at a time (one chunk of host memory, not the whole table); the chunks are draw_tables' tables"""
    monkeypatch.setattr(T_, "TABLE_CHUNK", 4)
    probs = [(np.arange(0, 50), np.arange(50, 200)), (np.arange(10, 20), np.arange(300, 400))]
    chunks = list(T_.iter_tables(probs, 10, 9, seed=2))
    assert [(a, i.shape, y.shape) for a, i, y in chunks] == [(0, (2, 4, 9), (2, 4, 9)), (4, (2, 4, 9), (2, 4, 9)), (8, (2, 2, 9), (2, 2, 9))]
    idx, y = T_.draw_tables(probs, 10, 9, seed=2)
    np.testing.assert_array_equal(np.concatenate([c[1] for c in chunks], axis=1), idx)
    np.testing.assert_array_equal(np.concatenate([c[2] for c in chunks], axis=1), y)
    # a longer run starts with the same chunks: the generators carry on, they are not re-seeded per chunk
    np.testing.assert_array_equal(T_.draw_tables(probs, 8, 9, seed=2)[0], idx[:, :8])
    assert not np.array_equal(idx[:, :4], idx[:, 4:8])
