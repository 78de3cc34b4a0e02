"""The per-stream audio rings without a GPU (include/owwhip.h: oww_audio_configure / oww_get_audio / oww_get_event_audio): the numpy
definition engine.audio_ring_model against a collections.deque, the Python-side argument checks, the header's new entries against
their ctypes prototypes, and the host arithmetic of csrc/owwhip_audio_host.h as a plain host program (tests/audio_check.cpp) under
AddressSanitizer / UBSan."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd.engine import AUDIO_RING_MAX, CHUNK, StreamEngine, audio_ring_model, check_audio_config
from openwakeword_amd.model import BatchedModel
from test_abi_cpu import ROOT, declared_symbols
from test_pack_host_cpu import _host_clangxx

EINVAL, ESTATE = -1, -3


# ---- the numpy model is a deque(maxlen = ring * 1280) per stream, padded with leading zeros ---------------------------------------------
@pytest.mark.parametrize("ring", [1, 5, 8])
def test_ring_model_is_a_deque(ring):
    S = 6
    rng = np.random.default_rng(100 + ring)
    model = audio_ring_model(S, ring)
    dq = [collections.deque(maxlen=ring * CHUNK) for _ in range(S)]
    counts = np.zeros(S, dtype=np.int64)

    def check():
        for n in range(1, ring + 1):
            got = model.last(np.arange(S), n)
            assert got.dtype == np.int16 and got.shape == (S, n * CHUNK)
            for s in range(S):
                have = np.array(dq[s], dtype=np.int16)
                want = np.concatenate([np.zeros(ring * CHUNK - have.size, dtype=np.int16), have])[-n * CHUNK:]
                np.testing.assert_array_equal(got[s], want)
        np.testing.assert_array_equal(model.counts, counts.astype(np.uint32))
        np.testing.assert_array_equal(model.last([S - 1, 0, 0], 1), model.last(np.arange(S), 1)[[S - 1, 0, 0]])

    check()                                                  # nothing received: zeros, counters 0
    assert not model.last(np.arange(S), ring).any() and not model.counts.any()
    for call, k in enumerate([1, 3, 7, 1, 1, 3, 7, 7, 1, 3, 1, 1]):
        pcm = rng.integers(-32768, 32768, size=(S, k * CHUNK), dtype=np.int64).astype(np.int16)
        on = None if call % 3 else (rng.random(S) < 0.5)
        model.append(pcm, on)
        for s in range(S):
            if on is None or on[s]:
                dq[s].extend(pcm[s].tolist())
                counts[s] += k
        check()
        if call in (4, 8):                                   # resets in between: one stream, then a list
            ids = [2] if call == 4 else [0, S - 1]
            model.reset(ids)
            for s in ids:
                dq[s].clear()
                counts[s] = 0
            check()
    model.reset()
    assert not model.buf.any() and not model.counts.any()
    with pytest.raises(ValueError):
        model.last([0], ring + 1)
    with pytest.raises(ValueError):
        model.last([0], 0)
    with pytest.raises(ValueError):
        model.append(np.zeros((S, CHUNK + 1), dtype=np.int16))
    assert model.counts.dtype == np.uint32


# ---- the limits of oww_audio_configure, before any device is touched ------------------------------------------------------------------------
def test_check_audio_config_accepts_and_refuses():
    assert check_audio_config(0, 0, 0) == (0, 0)
    assert check_audio_config(125, 0, 0) == (125, 0)
    assert check_audio_config(1, 1, 16) == (1, 1)
    assert check_audio_config(np.int32(AUDIO_RING_MAX), np.int64(AUDIO_RING_MAX), 1) == (1024, 1024)
    assert AUDIO_RING_MAX == 1024
    for ring, ev, cap, word in ((-1, 0, 0, "audio_chunks"), (1025, 0, 0, "audio_chunks"), (5, -1, 16, "event_audio"), (5, 6, 16, "event_audio"),
                                (0, 1, 16, "event_audio"), (5, 3, 0, "event_capacity"), (5.0, 0, 0, "integer"), (5, True, 16, "integer"),
                                ("5", 0, 0, "integer")):
        with pytest.raises(ValueError, match=word):
            check_audio_config(ring, ev, cap)
    assert StreamEngine.check_audio_config(5, 3, 16) == BatchedModel.check_audio_config(5, 3, 16) == (5, 3)
    # the constructors refuse before the library is loaded or a device is touched: no GPU, no OwwError, a ValueError
    with pytest.raises(ValueError, match="audio_chunks"):
        StreamEngine(4, {}, audio_chunks=2000)
    with pytest.raises(ValueError, match="event_capacity"):
        StreamEngine(4, {}, audio_chunks=5, event_audio=3)
    with pytest.raises(ValueError, match="event_audio"):
        BatchedModel(4, ["alexa"], weights="synthetic", audio_chunks=5, event_audio=6, event_capacity=16)


# ---- header <-> ctypes ----------------------------------------------------------------------------------------------------------------------
_CTYPES = {"int": C.c_int, "int32_t": C.c_int32}
_NEW = ("oww_audio_configure", "oww_get_audio", "oww_get_event_audio", "oww_event_audio_dev")


def _prototype(name):
    """(return type, [parameter types]) of `name` as include/owwhip.h declares it, comments stripped as test_abi_cpu does."""
    src = open(os.path.join(ROOT, "include", "owwhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"([A-Za-z_0-9 \*]+?)\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/owwhip.h"
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def test_new_entries_are_declared_and_bound_with_matching_signatures():
    names = declared_symbols()
    for n in _NEW:
        assert n in names and n in _lib.SYMBOLS, n
        ret, params = _prototype(n)
        res, args = _lib.SYMBOLS[n]
        assert res is (C.c_void_p if "*" in ret else C.c_int), (n, ret)
        assert len(params) == len(args), (n, params)
        for decl, ct in zip(params, args):
            want = C.c_void_p if "*" in decl else _CTYPES[decl.split()[0]]
            assert ct is want, (n, decl, ct)
    assert _prototype("oww_get_audio")[1][-1].startswith("uint32_t*") and _prototype("oww_event_audio_dev")[0] == "const int16_t*"
    lib = _lib.load()
    for n in _NEW:
        assert hasattr(lib, n), f"{n} is not exported"
    src = open(os.path.join(ROOT, "include", "owwhip.h")).read()
    assert "#define OWW_ABI_VERSION 6" in src and _lib.ABI_VERSION == 6          # additive entries: the version does not move
    # without a handle the entries refuse instead of crashing
    assert lib.oww_audio_configure(None, 5, 0) == EINVAL
    assert lib.oww_get_audio(None, None, 0, 1, None, 0, None) == EINVAL
    assert lib.oww_get_event_audio(None, 0, 0, None, 0) == EINVAL
    assert lib.oww_event_audio_dev(None) is None


def test_the_source_hash_covers_the_new_headers():
    from openwakeword_amd import _build
    base = [os.path.basename(d) for d in _build.DEPS]
    assert "owwhip_audio.h" in base and "owwhip_audio_host.h" in base


# ---- the HIP-free header as a host program under the sanitizers -------------------------------------------------------------------------------
def test_index_map_sizes_and_refusals_under_the_sanitizers(tmp_path):
    cxx = _host_clangxx()
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    exe = str(tmp_path / "audio_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "audio_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    got = dict(ln.split(" ", 1) for ln in run.stdout.splitlines())
    # 12 calls x 6 rounds, `ring` ages read after each
    assert [int(got[f"walk_{r}"]) for r in (1, 5, 125)] == [72 * 1, 72 * 5, 72 * 125]
    assert int(got["ring_42gb"]) == 131072 * 125 * 2560 == 41_943_040_000
    assert int(got["ring_max"]) == 1048576 * 1024 * 2560 == 2_748_779_069_440 > 1 << 41
    assert int(got["counter_max"]) == 4 << 20
    assert int(got["snap_max"]) == ((1 << 20) + 1) * 1024 * 2560
    assert int(got["gather_max"]) == int(got["ring_max"])
    assert got["record_125"] == f"{125 * 2560 + 16} record_0 0 words_1024 {1024 * 640} quads 160"
    ok = ("cfg_ok", "cfg_ok_edges", "commit_ok", "ready_ok", "get_ok", "get_unaligned_host", "ev_ok")
    for name in ok:
        assert got[name] == "rc=0 -", (name, got[name])
    refusals = {"cfg_null": (EINVAL, "null handle"), "cfg_committed": (ESTATE, "before oww_commit"), "cfg_ring0": (EINVAL, "ring_chunks = 0 outside [1, 1024]"),
                "cfg_ring_neg": (EINVAL, "ring_chunks = -3"), "cfg_ring_big": (EINVAL, "ring_chunks = 1025"), "cfg_ev_neg": (EINVAL, "event_chunks = -1"),
                "cfg_ev_big": (EINVAL, "event_chunks = 6 outside [0, ring_chunks = 5]"), "commit_no_events": (EINVAL, "needs events"),
                "ready_null": (EINVAL, "oww_get_audio: null handle"), "ready_uncommitted": (ESTATE, "keeps no audio"),
                "ready_no_audio": (ESTATE, "oww_get_event_audio: the handle keeps no audio"), "get_chunks0": (EINVAL, "n_chunks = 0 outside [1, ring_chunks = 5]"),
                "get_chunks_big": (EINVAL, "n_chunks = 6"), "get_id_hi": (EINVAL, "stream id 70 out of range (0..69)"), "get_id_lo": (EINVAL, "stream id -1"),
                "get_null_list": (EINVAL, "null list or buffer"), "get_null_out": (EINVAL, "null list or buffer"), "get_n_neg": (EINVAL, "n = -1"),
                "get_unaligned": (EINVAL, "16-byte aligned"), "ev_none": (EINVAL, "event_chunks = 0"), "ev_beyond": (EINVAL, "[2, 2 + 3) of 4 stored"),
                "ev_huge": (EINVAL, "of 4 stored"), "ev_first_neg": (EINVAL, "[-1, -1 + 1)"), "ev_null_out": (EINVAL, "out is null"),
                "ev_unaligned": (EINVAL, "16-byte aligned")}
    for name, (rc, words) in refusals.items():
        assert got[name].startswith(f"rc={rc} ") and words in got[name], (name, got[name])
    assert set(got) == set(ok) | set(refusals) | {"walk_1", "walk_5", "walk_125", "ring_42gb", "ring_max", "counter_max", "snap_max", "gather_max",
                                                  "record_125"}
