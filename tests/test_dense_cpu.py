"""Dense scoring without a GPU (include/owwhip.h: oww_score_shape / oww_score_features / oww_score_clips): the float64 expectation
tests/dense_ref.py against train.py:875's own slicing expression, the admission of every (form, T) the device tier uses, the host
arithmetic of csrc/owwhip_dense_host.h as a plain host program (tests/dense_check.cpp) under AddressSanitizer / UBSan, and the Python
layer's host logic -- utils.score_feature_file's chunk overlap, utils.mine_windows' window cut -- on a stand-in engine."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oww_oracle as O
from openwakeword_amd import _build, _lib, utils

import dense_ref as D
import head_windows as HW
from test_abi_cpu import ROOT, declared_symbols
from test_pack_host_cpu import _host_clangxx

ALL_FORMS = D.SLIDE_FORMS + D.FALLBACK_FORMS


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def test_dense_ref_is_the_reference_scan_plus_its_dropped_last_window():
    """train.py:875 builds np.array([X[i:i+T] for i in range(0, N - T, 1)]) and runs the model over it: N - T windows, the last one
    dropped.  dense_ref's windows are those plus the last, and its scores the oracle's on each."""
    T, N = 5, 23
    X = np.random.default_rng(1).normal(0.0, 1.0, (N, 96)).astype(np.float32)
    theirs = np.array([X[i:i + T] for i in range(0, X.shape[0] - T, 1)])
    ours = D.windows_of(X[None], T)[0]
    assert theirs.shape == (N - T, T, 96) and ours.shape == (N - T + 1, T, 96)
    np.testing.assert_array_equal(ours[:-1], theirs)
    np.testing.assert_array_equal(ours[-1], X[N - T:])
    head = HW.draw_head("pin", HW.FORMS["narrow1"]["heads"][0], T, seed=D.HEAD_SEED)
    ref = D.dense_ref(X[None], {"pin": head})["pin"]
    np.testing.assert_array_equal(ref[0, :-1], O.head_stage(theirs, head, np.float64))
    # (a batch of one window takes another BLAS path than a batch of nineteen: float64 rounding, not bits)
    np.testing.assert_allclose(ref[0, -1:], O.head_stage(X[None, N - T:], head, np.float64), rtol=1e-12, atol=0)


def test_dense_ref_aligns_mixed_window_lengths_at_the_end():
    """Heads of T = 5, 16, 22 on one handle: window w of the T-row head is rows [w + 22 - T, w + 22) -- the last T rows of the longest
    head's window, what the heads of a live handle see at one instant."""
    f = D.feats()[:, :60]
    heads = {f"m{T}": HW.draw_head(f"m{T}", HW.FORMS["narrow1"]["heads"][0], T, seed=D.HEAD_SEED) for T in (5, 16, 22)}
    ref = D.dense_ref(f, heads)
    for T in (5, 16, 22):
        assert ref[f"m{T}"].shape == (D.B, 60 - 22 + 1, 1)
        for w in (0, 7, 38):
            np.testing.assert_allclose(ref[f"m{T}"][:, w], O.head_stage(f[:, w + 22 - T:w + 22], heads[f"m{T}"], np.float64), rtol=1e-12, atol=0)
    raw = D.dense_raw(f, heads, np.float64)
    assert raw.shape == (D.B, 39, 3)


# ---- admission of the device tier's inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL_FORMS)
def test_device_cases_are_admitted(form):
    """For every (form, T) of the device tier: the fp32 oracle stays within FP32_CAP of float64 (else TOL_SCORE would judge the number
    format, not the kernel), and every binary head has at least MID_SHARE of its float64 scores in (0.05, 0.95) on the windows it
    meets (else a sigmoid comparison shows nothing)."""
    for T in D.TS:
        w64, w32 = D.want(form, T), D.want(form, T, np.float32)
        for n, h in D.form_heads(form, T).items():
            gap = float(np.abs(w64[n] - w32[n]).max())
            share = HW.mid_fraction(w64[n]) if HW.is_binary(h) else None
            print(f"\n{n}: fp32 - float64 = {gap:.2e}, mid share = {share}")
            assert w64[n].shape == (D.B, max(D.N_WINS), int(h["n_out"]))
            assert gap <= HW.FP32_CAP, f"{n}: the fp32 oracle is {gap:.2e} from float64"
            if share is not None:
                assert share >= HW.MID_SHARE, f"{n}: only {share:.2f} of the float64 scores lie in (0.05, 0.95)"


def test_routing_edge_cases_are_admitted():
    for form, Ts in D.EDGES:
        for T in Ts:
            w64, w32 = D.want(form, T), D.want(form, T, np.float32)
            for n, h in D.form_heads(form, T).items():
                n_win = max(D.EDGE_N_WINS)
                gap = float(np.abs(w64[n] - w32[n])[:, :n_win].max())
                share = HW.mid_fraction(w64[n][:, :n_win])
                print(f"\n{n}: fp32 - float64 = {gap:.2e}, mid share = {share:.2f}")
                assert w64[n].shape[1] >= n_win and gap <= HW.FP32_CAP and share >= HW.MID_SHARE


def test_device_cases_reach_the_tile_edges():
    assert [(n + 127) // 128 for n in D.N_WINS] == [1, 1, 1, 2, 2, 3, 3] and [n % 128 for n in D.N_WINS] == [1, 37, 0, 1, 0, 1, 5]
    assert [(n + 255) // 256 for n in D.N_WINS] == [1, 1, 1, 1, 1, 2, 2] and [n % 256 for n in D.N_WINS] == [1, 37, 128, 129, 0, 1, 5]
    assert set((1, 37, 128, 129, 261)) <= set(D.N_WINS)
    # the edge lengths straddle the limits dense_check.cpp prints (t_limit: 72 for two nets, 113 for one, tiles of 256)
    assert D.EDGES == (("narrow4", (72, 73)), ("narrow1", (113, 114, 120)))
    assert max(D.case_rows(n, T) for n in D.N_WINS for T in D.TS) <= D.ROWS


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_build_hashes_the_kernel():
    declared = declared_symbols()
    for name in ("oww_score_shape", "oww_score_features", "oww_score_clips"):
        assert name in declared and name in _lib.SYMBOLS
    base = [os.path.basename(d) for d in _build.DEPS]
    assert "owwhip_dense.h" in base and "owwhip_dense_host.h" in base
    with open(os.path.join(ROOT, "include", "owwhip.h")) as f:
        assert "#define OWW_ABI_VERSION 6" in f.read()


def test_host_arithmetic_and_refusals_under_the_sanitizers(tmp_path):
    cxx = _host_clangxx()
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    exe = str(tmp_path / "dense_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "dense_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    got = dict(ln.split(" ", 1) for ln in run.stdout.splitlines())
    assert got["done"] == "1" and got["refusals"] == "ok"
    assert got["passes"] == "ok"
    assert [got[f"tiles_{n}"] for n in (1, 127, 128, 129, 255, 256, 257, 261)] == ["1 1", "1 1", "1 1", "2 1", "2 1", "2 1", "3 2", "3 2"]
    # (32 waves + T - 1) x 400 bytes of rows + 2 slots x nets x 8 KB <= 160 KB: tiles of 256 windows up to T = 113 / 72, of 128 beyond
    assert (got["t_limit_1"], got["t_limit_2"]) == ("113 241", "72 200")
    assert (got["fits_to_120_1"], got["fits_to_120_2"]) == ("120 113", "120 72")
    assert (got["geo_1_16"], got["geo_2_16"], got["geo_2_73"]) == ("8 4", "8 3", "4 4")
    assert int(got["slab_windows_16"]) == (256 << 20) // (16 * 384) and int(got["slab_big_bytes"]) > 1 << 31


# ---- the Python layer on a stand-in engine -------------------------------------------------------------------------------------------
def _mixed_heads():
    shapes = HW.FORMS["narrow4"]["heads"]
    return {f"mix{T}": HW.centre(HW.draw_head(f"mix{T}", shapes[i], T, seed=D.HEAD_SEED),
                                 np.ascontiguousarray(D.windows_of(D.feats(), T, 22)).reshape(-1, T, 96)) for i, T in enumerate((5, 16, 22))}


def test_dense_chunks_cover_every_window_once():
    for n_rows, t_max, chunk in ((300, 22, 100), (300, 22, 22), (300, 1, 7), (22, 22, 50), (150, 16, 149), (150, 16, 150)):
        chunks = utils.dense_chunks(n_rows, t_max, chunk)
        n_win = n_rows - t_max + 1
        assert chunks[0][0] == 0 and chunks[-1][1] == n_win
        for (a0, a1, r0, r1), nxt in zip(chunks, chunks[1:] + [None]):
            assert 0 < a1 - a0 and r1 - r0 <= chunk and r0 == a0 and r1 == a1 + t_max - 1 and r1 <= n_rows
            if nxt is not None:
                assert nxt[0] == a1 and r1 - nxt[2] == t_max - 1          # the overlap
    with pytest.raises(ValueError):
        utils.dense_chunks(300, 22, 21)


def test_score_feature_file_in_chunks_is_one_call(tmp_path):
    heads = _mixed_heads()
    X = np.ascontiguousarray(D.feats()[2, :211])
    want = D.dense_raw(X[None], heads, np.float64)[0]
    bm = D.StubDenseModel(heads)
    whole = utils.score_feature_file(X, bm)
    assert bm.engine.calls == [(1, 211, 96)]
    path = str(tmp_path / "feats.npy")
    np.save(path, X)
    bm.engine.calls.clear()
    parts = utils.score_feature_file(path, bm, chunk_rows=100)
    assert bm.engine.calls == [(1, 100, 96), (1, 100, 96), (1, 53, 96)]          # 79 + 79 + 32 windows
    assert list(whole) == list(parts) == list(heads)
    for i, n in enumerate(heads):
        assert whole[n].shape == (190,)
        np.testing.assert_array_equal(whole[n], want[:, i])
        np.testing.assert_array_equal(parts[n], want[:, i])
    with pytest.raises(ValueError):
        utils.score_feature_file(X[:, :95], bm)


def test_mine_windows_cuts_each_models_own_rows():
    heads = _mixed_heads()
    bm = D.StubDenseModel(heads, n_streams=2)                   # five clips: three calls of at most two
    pcm = (np.random.default_rng(8).normal(0.0, 6000.0, (5, 12512 + 1280 * 40))).astype(np.int16)
    emb = bm.engine.embed(pcm)
    assert emb.shape == (5, 41, 96)
    scores = D.dense_raw(emb, heads, np.float64)
    thr = float(np.median(scores))                              # about half of the windows of some model
    got = utils.mine_windows(pcm, bm, threshold=thr)
    assert [c[0] for c in bm.engine.calls] == [2, 2, 1]
    assert list(got) == list(heads)
    for i, (n, h) in enumerate(heads.items()):
        T = int(h["T"])
        b, w = np.nonzero(scores[:, :, i] >= thr)
        assert got[n].shape == (b.size, T, 96) and got[n].dtype == np.float32
        for k in range(b.size):
            np.testing.assert_array_equal(got[n][k], emb[b[k], w[k] + 22 - T:w[k] + 22])
        # each kept window scores what put it there (float32 in another batch: rounding apart)
        if b.size:
            again = O.head_stage(got[n], h, np.float32)[:, 0]
            np.testing.assert_allclose(again, scores[b, w, i], rtol=0, atol=1e-5)
    assert sum(v.shape[0] for v in got.values()) > 0
    none = utils.mine_windows(pcm, bm, threshold=2.0)
    assert all(v.shape == (0, int(heads[n]["T"]), 96) for n, v in none.items())
