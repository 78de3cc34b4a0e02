"""Dense scoring over the head bank without a GPU (include/owwhip.h: oww_bank_score_shape / oww_bank_score_features /
oww_bank_score_stats): the host arithmetic of csrc/owwhip_dense_bank_host.h as a plain host program (tests/dense_bank_check.cpp) under
AddressSanitizer / UBSan, the three symbols through header, binding and engine, utils.validate_bank's chunk combination on a
stand-in model, and the admission of the device tier's heads."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from openwakeword_amd import _build, _lib, engine, model, utils

import dense_bank_ref as DB
import dense_ref as D
import head_windows as HW
from test_abi_cpu import ROOT, declared_symbols
from test_pack_host_cpu import _host_clangxx

ENTRIES = ("oww_bank_score_shape", "oww_bank_score_features", "oww_bank_score_stats")


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_engine_declare_the_three_entries():
    declared = declared_symbols()
    eng_src = inspect.getsource(engine.StreamEngine)
    for name in ENTRIES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert f"self._lib.{name}(" in eng_src, name
    with open(os.path.join(ROOT, "include", "owwhip.h")) as f:
        header = f.read()
    assert "#define OWW_ABI_VERSION 6" in header and "#define OWW_N_KERNEL_CLASSES 10" in header
    for cite in ("train.py:225-258", "874-879", "train.py:100"):
        assert cite in header, cite
    # argument counts of the binding against the header's prototypes
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1)
        assert len(_lib.SYMBOLS[name][1]) == len(args.split(",")), name
    for meth in ("bank_score_shape", "bank_score_features", "bank_score_stats"):
        assert callable(getattr(engine.StreamEngine, meth)) and callable(getattr(model.BatchedModel, meth)), meth
    assert "owwhip_dense_bank_host.h" in [os.path.basename(d) for d in _build.DEPS]
    doc = utils.validate_bank.__doc__
    assert "train.py:875" in doc and "last window" in doc


def test_host_arithmetic_and_refusals_under_the_sanitizers(tmp_path):
    cxx = _host_clangxx()
    if cxx is None or not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    exe = str(tmp_path / "dense_bank_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "dense_bank_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k != "OWW_DENSE_BANK_HPW"}
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    got = dict(ln.split(" ", 1) for ln in run.stdout.splitlines())
    assert got["done"] == "1" and got["refusals"] == "ok" and got["keys"] == "ok"
    assert int(got["plans"]) == 15 * 3 * 9 * 6 and int(got["staged_rows"]) > 10 ** 7
    # eight hours x 256 heads: 1,408 tiles, eight heads per workgroup; ten minutes: 30 tiles, the heads spread until the grid passes
    # 1,024 workgroups; one head alone: one workgroup per tile
    assert got["plan_big"] == "8 1408 45056" and got["plan_one"] == "1 30 30"
    hpw, tiles, grid = (int(x) for x in got["plan_small"].split())
    assert tiles == 30 and grid == tiles * -(-256 // hpw) and grid >= 1024 and 1 <= hpw <= 8
    hpw, grid = (int(x) for x in got["plan_huge"].split())
    assert hpw > 8 and grid <= 2 ** 31 - 1
    assert int(got["matrix_bytes"]) == 8 * 45000 * 1024 * 4


# ---- utils.validate_bank on a stand-in -------------------------------------------------------------------------------------------------
def _scan_inputs():
    heads = DB.heads()
    X = np.ascontiguousarray(D.feats()[2, :211])
    return heads, X, DB.StubBankModel(heads)


def test_validate_bank_in_chunks_is_one_unchunked_numpy_evaluation(tmp_path):
    heads, X, bm = _scan_inputs()
    ids = [6, 0, 3, 0, 4]                                        # w16, n1, n19, n1 again, n22: t_max = 22
    matrix = bm.bank_score_features(X, ids)[0]                   # [190, 5]: one evaluation, no chunks
    assert matrix.shape == (211 - 22 + 1, 5)
    # thresholds: the default, and per head a value that occurs in its column (the >= edge)
    for thr in (None, [float(np.sort(matrix[:, k])[matrix.shape[0] // 2]) for k in range(len(ids))]):
        t = np.full(len(ids), 0.5, np.float32) if thr is None else np.asarray(thr, np.float32)
        bm.calls.clear()
        whole = utils.validate_bank(X, bm, ids, thr)
        assert bm.calls == [(1, 211, 96)]
        path = str(tmp_path / "neg.npy")
        np.save(path, X)
        for chunk_rows in (100, 22, 57):
            bm.calls.clear()
            parts = utils.validate_bank(path, bm, ids, thr, chunk_rows=chunk_rows)
            assert len(bm.calls) == len(utils.dense_chunks(211, 22, chunk_rows)) > 1
            assert parts == whole, f"chunk_rows = {chunk_rows}"
        assert list(whole) == [6, 0, 3, 4]
        for k, i in enumerate(ids):
            n_fp = int((matrix[:, k] >= t[k]).sum())
            assert whole[i]["n_false_positives"] == n_fp and n_fp > 0
            assert whole[i]["false_positives_per_hour"] == n_fp / (190 * 0.08 / 3600.0)
            assert whole[i]["max_score"] == float(matrix[:, k].max()) and whole[i]["argmax_window"] == int(matrix[:, k].argmax())
    assert utils.validate_bank(X, bm, ids, hours=2.0)[6]["false_positives_per_hour"] == utils.validate_bank(X, bm, ids)[6]["n_false_positives"] / 2.0
    with pytest.raises(ValueError):
        utils.validate_bank(X[:, :95], bm, ids)
    with pytest.raises(ValueError):
        utils.validate_bank(X, bm, ids, chunk_rows=21)


def test_validate_bank_keeps_the_first_of_equal_maxima_across_chunks():
    """A column whose maximum occurs in two chunks: the earlier window wins, with the chunk's window offset added."""

    class Flat:
        def bank_score_shape(self, ids, n_rows):
            return n_rows - 3, 4

        def bank_score_stats(self, feats, ids, thresholds=None):
            col = np.asarray(feats)[0, 3:, 0:1]                  # the "score" of window w is feature 0 of its last row
            return DB.np_stats(col[None], thresholds)

    X = np.zeros((40, 96), np.float32)
    X[3 + 7, 0] = X[3 + 29, 0] = 0.75
    X[3 + 30, 0] = 0.6
    for chunk_rows in (40, 13, 4):
        got = utils.validate_bank(X, Flat(), [5], chunk_rows=chunk_rows)[5]
        assert got == {"n_false_positives": 3, "false_positives_per_hour": 3 / (37 * 0.08 / 3600.0), "max_score": 0.75, "argmax_window": 7}, chunk_rows


# ---- admission of the device tier's inputs ---------------------------------------------------------------------------------------------
def test_device_heads_are_admitted():
    """Every bank head of the device tier: the fp32 oracle within FP32_CAP of float64 (else TOL_SCORE would judge the number format),
    and at least MID_SHARE of its float64 scores in (0.05, 0.95) on the windows it meets (else a sigmoid comparison shows nothing)."""
    w64, w32 = DB.want(), DB.want(np.float32)
    assert list(w64) == list(DB.NARROW + DB.WIDE) and sorted(DB.ADD_ORDER) == sorted(w64)
    for n, h in DB.heads().items():
        gap = float(np.abs(w64[n] - w32[n]).max())
        share = HW.mid_fraction(w64[n])
        print(f"\n{n}: T = {h['T']}, hidden = {h['hidden']}, fp32 - float64 = {gap:.2e}, mid share = {share:.2f}")
        assert w64[n].shape == (D.B, max(DB.N_WINS), 1) and HW.is_binary(h)
        assert (h["hidden"] <= 64) == (n in DB.NARROW)
        assert gap <= HW.FP32_CAP and share >= HW.MID_SHARE, n
    assert max(int(h["T"]) for h in DB.heads().values()) == DB.T_MAX
    assert D.case_rows(max(DB.N_WINS), DB.T_MAX) <= D.ROWS


def test_edge_heads_are_admitted():
    for T in DB.EDGE_TS:
        h = DB.edge_head(T)
        f = D.feats()[:, :D.case_rows(max(DB.EDGE_N_WINS), T)]
        w64, w32 = D.dense_ref(f, {"e": h})["e"], D.dense_ref(f, {"e": h}, np.float32)["e"]
        gap, share = float(np.abs(w64 - w32).max()), HW.mid_fraction(w64)
        print(f"\nedge T = {T}: fp32 - float64 = {gap:.2e}, mid share = {share:.2f}")
        assert gap <= HW.FP32_CAP and share >= HW.MID_SHARE and f.shape[1] <= D.ROWS
