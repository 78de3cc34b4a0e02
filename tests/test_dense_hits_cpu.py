"""Ordered hit lists of dense scoring without a GPU (include/owwhip.h: oww_score_hits_layout / oww_score_hits / oww_score_clip_hits /
oww_bank_score_hits): numpy's statement of the contract (tests/dense_hits_ref.py) against plain loops, the host side
(csrc/owwhip_dense_hits_host.h) as a plain host program (tests/dense_hits_check.cpp) under AddressSanitizer / UBSan, the agreement of
header and binding, and the Python layer's host logic -- BatchedModel.score_clip_hits' batches, utils.mine_clip_hits against
utils.mine_windows, utils.mine_feature_file's chunk offsets, totals and cap -- on stand-in engines."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from openwakeword_amd import _build, _lib, engine, model, utils

import dense_bank_ref as DB
import dense_hits_ref as H
import dense_ref as D
import head_windows as HW
from test_abi_cpu import ROOT, declared_symbols
from test_pack_host_cpu import _host_clangxx

ENTRIES = ("oww_score_hits_layout", "oww_score_hits", "oww_score_clip_hits", "oww_bank_score_hits")


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def test_dense_hits_ref_is_the_contract_in_plain_loops():
    rng = np.random.default_rng(3)
    B, n_rows, Ts, t_max = 3, 40, (2, 5, 7), 7
    n_win = n_rows - t_max + 1
    f = rng.normal(0.0, 1.0, (B, n_rows, 96)).astype(np.float32)
    m = rng.random((B, n_win, 3)).astype(np.float32)
    m[1, 4, 0] = m[2, 33, 0] = np.float32(0.75)                 # equality with the threshold counts
    thr = np.array([0.75, 0.2, np.nan], np.float32)
    for cap in (1, 5, 1000):
        got = H.hits(m, thr, cap, f, Ts, t_max)
        for c in range(3):
            want = [(b, w) for b in range(B) for w in range(n_win) if m[b, w, c] >= thr[c]]
            assert got[c]["n_total"] == len(want)
            assert list(zip(got[c]["seq"], got[c]["window"])) == want[:cap]
            for k, (b, w) in enumerate(want[:cap]):
                assert got[c]["score"][k] == m[b, w, c]
                np.testing.assert_array_equal(got[c]["windows"][k], f[b, w + t_max - Ts[c]:w + t_max])
    got = H.hits(m, thr, 1000)
    assert (1, 4) in list(zip(got[0]["seq"], got[0]["window"])) and got[2]["n_total"] == 0 and got[1]["n_total"] > 0
    assert [c["n_total"] for c in H.hits(m, None, 1)] == [int((m[:, :, c] >= 0.5).sum()) for c in range(3)]
    t = H.thresholds_from(m)
    assert all((m[:, :, c] == t["median"][c]).any() for c in range(3)) and np.isnan(t["nan0"][0])
    assert [c["n_total"] for c in H.hits(m, t["above"], 4)] == [0, 0, 0] and [c["n_total"] for c in H.hits(m, t["zero"], 4)] == [B * n_win] * 3
    assert all(c["n_total"] >= 1 for c in H.hits(m, t["max"], 4))


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_layers_declare_the_four_entries():
    declared = declared_symbols()
    eng_src = inspect.getsource(engine.StreamEngine)
    with open(os.path.join(ROOT, "include", "owwhip.h")) as f:
        header = f.read()
    assert "#define OWW_ABI_VERSION 6" in header and "#define OWW_N_KERNEL_CLASSES 10" in header
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert f"self._lib.{name}(" in eng_src, name
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1)
        assert len(_lib.SYMBOLS[name][1]) == len(args.split(",")), name
    assert re.search(r"typedef struct oww_dense_hit \{ int32_t seq; int32_t window; float score; int32_t reserved;", flat)
    assert engine.DENSE_HIT.itemsize == 16 and engine.DENSE_HIT.names == ("seq", "window", "score", "reserved")
    assert [engine.DENSE_HIT.fields[n][1] for n in engine.DENSE_HIT.names] == [0, 4, 8, 12]
    for cite in ("model.py:428-479", "mine_false_positives.py", "train.py:100"):
        assert cite in header, cite
    for meth in ("score_hits", "score_clip_hits", "bank_score_hits"):
        assert callable(getattr(engine.StreamEngine, meth)) and callable(getattr(model.BatchedModel, meth)), meth
    assert callable(utils.mine_clip_hits) and callable(utils.mine_feature_file)
    base = [os.path.basename(d) for d in _build.DEPS]
    assert "owwhip_dense_hits_host.h" in base and "owwhip_dense.h" in base


def test_host_side_under_the_sanitizers(tmp_path):
    cxx = _host_clangxx()
    if cxx is None or not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    exe = str(tmp_path / "dense_hits_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "dense_hits_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    got = dict(ln.split(" ", 1) for ln in run.stdout.splitlines())
    assert got["done"] == "1" and got["refusals"] == "ok"
    assert [got[f"wps_{n}"] for n in (1, 31, 32, 33, 257)] == ["1", "1", "1", "2", "9"]
    assert int(got["mask_bytes_1024"]) == 32 << 20                  # 1,024 heads over a 2^18-row chunk
    assert got["win_offset_mixed"] == "0 4800 20160 41280 42240" and int(got["win_total_big"]) > 1 << 31
    # set bits of the masks the program builds: 32 + 1 + 2 + 2, none, every bit of 3 x 3 words, one
    assert (got["compact_edges"], got["compact_none"], got["compact_full"], got["compact_single"]) == ("37", "0", "288", "1")
    assert int(got["compact_random"]) > 7 and int(got["slab_pieces_2e20_120"]) > 1


# ---- the Python layer on stand-in engines ----------------------------------------------------------------------------------------------
def _mixed_heads():
    shapes = HW.FORMS["narrow4"]["heads"]
    return {f"mix{T}": HW.centre(HW.draw_head(f"mix{T}", shapes[i], T, seed=D.HEAD_SEED),
                                 np.ascontiguousarray(D.windows_of(D.feats(), T, 22)).reshape(-1, T, 96)) for i, T in enumerate((5, 16, 22))}


class _StubHitsEngine(D.StubDenseEngine):
    """+ score_hits / score_clip_hits, from dense_hits_ref on the stand-in's own matrix."""

    def _Ts(self):
        return [int(h["T"]) for h in self.heads.values() for _ in range(int(h["n_out"]))]

    def score_hits(self, f, thresholds=None, cap=4096, return_windows=True):
        f = np.asarray(f, np.float32)
        f = f[None] if f.ndim == 2 else f
        return H.hits(self.score_features(f), thresholds, cap, f if return_windows else None, self._Ts(), self.t_max)

    def score_clip_hits(self, pcm, thresholds=None, cap=4096, return_windows=True):
        return self.score_hits(self.embed(pcm), thresholds, cap, return_windows)


class _StubHitsModel(D.StubDenseModel):
    def __init__(self, heads, n_streams=4):
        super().__init__(heads, n_streams)
        self.engine = _StubHitsEngine(heads, n_streams)
        for meth in ("score_hits", "score_clip_hits", "_label_thresholds"):
            setattr(self, meth, getattr(model.BatchedModel, meth).__get__(self))


def test_mine_clip_hits_is_mine_windows_and_honours_the_cap():
    heads = _mixed_heads()
    bm = _StubHitsModel(heads, n_streams=2)                     # five clips: three calls of at most two
    pcm = (np.random.default_rng(8).normal(0.0, 6000.0, (5, 12512 + 1280 * 40))).astype(np.int16)
    thr = float(np.median(D.dense_raw(bm.engine.embed(pcm), heads, np.float64)))
    want = utils.mine_windows(pcm, bm, threshold=thr)
    got = utils.mine_clip_hits(pcm, bm, threshold=thr)
    assert list(got) == list(want) == list(heads) and sum(v.shape[0] for v in want.values()) > 10
    for n in heads:
        assert got[n].dtype == np.float32 and got[n].shape == want[n].shape and got[n].tobytes() == want[n].tobytes(), n
    lists = bm.score_clip_hits(pcm, thr, cap=4096)
    for n in heads:
        assert lists[n]["n_total"] == want[n].shape[0] and np.all(np.diff(lists[n]["seq"].astype(np.int64) * 1000 + lists[n]["window"]) > 0)
        assert lists[n]["seq"].max() >= 2                      # clips of a later batch keep their own index
    few = bm.score_clip_hits(pcm, thr, cap=7)                   # the cap bounds the merged list; the total does not notice
    for n in heads:
        k = min(7, want[n].shape[0])
        assert few[n]["n_total"] == want[n].shape[0] and few[n]["windows"].tobytes() == want[n][:k].tobytes(), n
        assert np.array_equal(few[n]["seq"], lists[n]["seq"][:k]) and np.array_equal(few[n]["score"], lists[n]["score"][:k])
    by_label = bm.score_clip_hits(pcm, {"mix16": 2.0}, cap=4096)        # a threshold per label; the others keep 0.5
    assert by_label["mix16"]["n_total"] == 0 and by_label["mix5"]["n_total"] == bm.score_clip_hits(pcm, 0.5)["mix5"]["n_total"]


def test_mine_feature_file_in_chunks_is_one_call(tmp_path):
    heads = _mixed_heads()
    X = np.ascontiguousarray(D.feats()[2, :211])
    bm = _StubHitsModel(heads)
    m = D.dense_raw(X[None], heads, np.float64)
    thr = float(np.median(m))
    want = H.hits(m, thr, 10 ** 6, X[None], [5, 16, 22], 22)
    whole = utils.mine_feature_file(X, bm, thr)
    path = str(tmp_path / "feats.npy")
    np.save(path, X)
    bm.engine.calls.clear()
    parts = utils.mine_feature_file(path, bm, thr, chunk_rows=100)
    assert bm.engine.calls == [(1, 100, 96), (1, 100, 96), (1, 53, 96)]          # 79 + 79 + 32 windows
    capped = utils.mine_feature_file(X, bm, thr, cap=9, chunk_rows=100)
    assert list(whole) == list(parts) == list(heads)
    for c, n in enumerate(heads):
        assert want[c]["n_total"] > 9
        for got in (whole[n], parts[n]):
            assert got["n_total"] == want[c]["n_total"] and np.array_equal(got["window"], want[c]["window"]) and got["window"].dtype == np.int64
            assert got["score"].tobytes() == want[c]["score"].tobytes() and got["windows"].tobytes() == want[c]["windows"].tobytes()
        assert capped[n]["n_total"] == want[c]["n_total"] and np.array_equal(capped[n]["window"], want[c]["window"][:9])
        assert capped[n]["windows"].tobytes() == want[c]["windows"][:9].tobytes()
    with pytest.raises(ValueError):
        utils.mine_feature_file(X[:, :95], bm)


class _StubBankHits(DB.StubBankModel):
    def bank_score_hits(self, feats, ids, thresholds=None, cap=4096, return_windows=True):
        f = np.asarray(feats, np.float32)
        f = f[None] if f.ndim == 2 else f
        Ts = [int(self.heads[self.names[i]]["T"]) for i in ids]
        return H.hits(self.bank_score_features(f, ids), thresholds, cap, f if return_windows else None, Ts, max(Ts))


def test_mine_feature_file_over_bank_ids_agrees_with_validate_bank():
    heads = DB.heads()
    X = np.ascontiguousarray(D.feats()[2, :211])
    bm = _StubBankHits(heads)
    ids = [6, 0, 3, 4]                                          # w16, n1, n19, n22 by position in the name list
    thr = [0.5, 0.4, 0.6, 0.5]
    counts = utils.validate_bank(X, bm, ids, thr, chunk_rows=100)
    whole = utils.mine_feature_file(X, bm, thr, ids=ids)
    parts = utils.mine_feature_file(X, bm, thr, ids=ids, chunk_rows=64)
    m = bm.bank_score_features(X, ids)
    assert list(whole) == ids
    for k, i in enumerate(ids):
        w = np.nonzero(m[0, :, k] >= np.float32(thr[k]))[0]
        assert whole[i]["n_total"] == parts[i]["n_total"] == counts[i]["n_false_positives"] == w.size
        assert np.array_equal(whole[i]["window"], w) and np.array_equal(parts[i]["window"], w)
        assert parts[i]["score"].tobytes() == m[0, w, k].tobytes() and parts[i]["windows"].tobytes() == whole[i]["windows"].tobytes()
    assert sum(v["n_total"] for v in whole.values()) > 0
