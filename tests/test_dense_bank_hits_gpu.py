"""Ordered hit lists over the head bank on the device (include/owwhip.h: oww_bank_score_hits; csrc/owwhip_dense.h:
heads_dense_bank_kernel's MASK mode, dense_hits_*_kernel).  The yardstick is oww_bank_score_features' matrix on the same handle, which
tests/test_dense_bank_gpu.py holds to float64 and to the fixed-head twins' bits: positions, totals, scores and windows equal numpy's
statement of the contract (tests/dense_hits_ref.py) on that matrix and the rows, bit for bit.  The seven heads of dense_bank_ref (five
narrow: one sliding launch; two wide: the fallback) in one call, on a handle whose ids have a hole."""
import ctypes as C
import functools

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import KERNEL_CLASSES, StreamEngine, _ptr

import dense_bank_ref as DB
import dense_hits_ref as H
import dense_ref as D
import head_windows as HW

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ESTATE = -1, -4, -3
S = 4
NAMES = list(DB.NARROW + DB.WIDE)


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


def _rows(n_win, t_max=DB.T_MAX):
    return D.feats()[:, :D.case_rows(n_win, t_max)]


def _launches(eng):
    t = eng.kernel_times()
    return t[KERNEL_CLASSES[6]]["launches"], t[KERNEL_CLASSES[7]]["launches"]


def _Ts(names):
    return [int(DB.heads()[n]["T"]) for n in names]


@pytest.fixture(scope="module")
def bank():
    """(engine, {name: bank id}): as tests/test_dense_bank_gpu.py's -- the seven heads added in a shuffled order with one head more added
    in between and removed again, so the ids have a hole."""
    heads = DB.heads()
    eng = StreamEngine(S, {}, _emb(), bank_slots=1, bank_capacity=16, feature_ring=HW.BANK_RING)
    ids = {}
    for k, n in enumerate(DB.ADD_ORDER):
        if k == 3:
            gone = eng.bank_add(heads["n3"])
        ids[n] = eng.bank_add(heads[n])
    eng.bank_remove(gone)
    assert sorted(ids.values()) != list(range(7)) and gone not in ids.values()
    eng.gone = gone
    eng.enable_timing(True)
    yield eng, ids
    eng.close()


def _check(eng, f, aid, names, thr, cap, label, matrix=None):
    matrix = eng.bank_score_features(f, aid) if matrix is None else matrix
    got = eng.bank_score_hits(f, aid, thr, cap)
    H.assert_columns_equal(got, H.hits(matrix, thr, cap, f, _Ts(names), max(_Ts(names))), label)
    return got


# ------------------------------------------------------------------------------------------------ 3. the bank
def test_seven_heads_in_one_call_at_every_edge(bank):
    eng, ids = bank
    aid = [ids[n] for n in NAMES]
    for n_win in DB.N_WINS:
        f = _rows(n_win)
        matrix = eng.bank_score_features(f, aid)
        thr = H.thresholds_from(matrix)
        for kind in ("median", "max", "above", "zero"):
            got = _check(eng, f, aid, NAMES, thr[kind], D.B * n_win, f"n_win={n_win} thresholds={kind}", matrix)
            st = eng.bank_score_stats(f, aid, thr[kind])
            assert [c["n_total"] for c in got] == st["count"].sum(axis=0).tolist(), f"n_win={n_win} {kind}: totals against the statistics"
            if kind == "max":                                   # the first hit of the column's maximum is a sequence's max / argmax
                for c, col in enumerate(got):
                    b, w = int(col["seq"][0]), int(col["window"][0])
                    assert col["score"][0] == st["max"][b, c] == st["max"][:, c].max() and w == st["argmax"][b, c]
        _check(eng, f, aid, NAMES, None, D.B * n_win, f"n_win={n_win} default thresholds", matrix)
    assert eng.range_status() is False


def test_launch_counts(bank):
    """Without hits: the sliding launch for the five narrow heads, per wide head one gather, one heads launch and one slab pass into the
    mask, and the compaction -- nothing more.  With hits: per column with hits one gather, one re-score launch and one score pass."""
    eng, ids = bank
    aid = [ids[n] for n in NAMES]
    f = _rows(261)
    thr = H.thresholds_from(eng.bank_score_features(f, aid))
    eng.kernel_times()
    none = eng.bank_score_hits(f, aid, thr["above"], 16)
    assert _launches(eng) == (1 + 2, 2 + 2 + 1) and not any(c["n_total"] for c in none)
    eng.bank_score_hits(f, aid, thr["max"], 16)
    assert _launches(eng) == (1 + 2 + 7, 2 + 2 + 1 + 7 * 2)
    assert eng.range_status() is False


@pytest.mark.parametrize("n_win", (129, 261))
def test_heads_per_workgroup_duplicates_and_the_gather_route(bank, monkeypatch, n_win):
    eng, ids = bank
    f = _rows(n_win)
    nid = [ids[n] for n in DB.NARROW]
    monkeypatch.delenv("OWW_DENSE_BANK_HPW", raising=False)
    matrix = eng.bank_score_features(f, nid)
    thr = H.thresholds_from(matrix)["median"]
    cap = D.B * n_win
    base = _check(eng, f, nid, DB.NARROW, thr, cap, "the plan's own hpw", matrix)
    order = [2, 0, 2, 4, 2]
    for hpw in DB.HPWS:
        monkeypatch.setenv("OWW_DENSE_BANK_HPW", str(hpw))
        H.assert_columns_equal(eng.bank_score_hits(f, nid, thr, cap), base, f"hpw={hpw}")
        dup = eng.bank_score_hits(f, [nid[k] for k in order], thr[order], cap)
        H.assert_columns_equal(dup, [base[k] for k in order], f"hpw={hpw}, a duplicated id")
    monkeypatch.delenv("OWW_DENSE_BANK_HPW")
    monkeypatch.setenv("OWW_DENSE_PATH", "ext")
    H.assert_columns_equal(eng.bank_score_hits(f, nid, thr, cap), base, "OWW_DENSE_PATH=ext")
    monkeypatch.setenv("OWW_DENSE_SLAB_MB", "1")                # slabs that start and end inside mask words
    H.assert_columns_equal(eng.bank_score_hits(f, nid, thr, cap), base, "OWW_DENSE_PATH=ext, 1 MB slabs")
    monkeypatch.delenv("OWW_DENSE_SLAB_MB")
    monkeypatch.delenv("OWW_DENSE_PATH")
    # capacity: one hot head does not starve the others -- every column has its own slots
    few = eng.bank_score_hits(f, nid, thr, 3)
    H.assert_columns_equal(few, H.hits(matrix, thr, 3, f, _Ts(DB.NARROW), 22), "cap=3")
    assert all(c["seq"].size == 3 and c["n_total"] > 3 for c in few)
    assert eng.range_status() is False


def test_tile_size_edge_and_the_longest_window():
    eng = StreamEngine(S, {}, _emb(), bank_slots=1, bank_capacity=4, feature_ring=HW.T_MAX)
    try:
        for T in DB.EDGE_TS:
            bid = eng.bank_add(DB.edge_head(T))
            for n_win in DB.EDGE_N_WINS:
                f = _rows(n_win, T)
                matrix = eng.bank_score_features(f, [bid])
                got = eng.bank_score_hits(f, [bid], H.thresholds_from(matrix)["median"], D.B * n_win)
                H.assert_columns_equal(got, H.hits(matrix, H.thresholds_from(matrix)["median"], D.B * n_win, f, [T], T), f"T={T} n_win={n_win}")
                assert got[0]["n_total"] >= 1
            eng.bank_remove(bid)
        assert eng.range_status() is False
    finally:
        eng.close()


def test_device_resident_features_and_windows_give_the_host_routes_bytes(bank):
    """feats_on_device = windows_on_device = 1 with torch's buffers: records and window bytes are the host route's (seven heads, both paths)."""
    import torch
    from openwakeword_amd.engine import DENSE_HIT
    eng, ids = bank
    aid = np.array([ids[n] for n in NAMES], np.int32)
    f = np.ascontiguousarray(_rows(129))
    cap = 48
    thr = H.thresholds_from(eng.bank_score_features(f, aid))["median"]
    off = eng.score_hits_layout(cap, aid)
    d_f = torch.from_numpy(f).cuda()
    win_h = np.full(int(off[-1]), np.float32(-77.0), np.float32)
    d_win = torch.full((int(off[-1]),), -77.0, device="cuda")
    out = []
    for fp, fd, wp, wd in ((_ptr(f), 0, _ptr(win_h), 0), (C.c_void_p(d_f.data_ptr()), 1, C.c_void_p(d_win.data_ptr()), 1)):
        hits, ns, nt = np.zeros((7, cap), DENSE_HIT), np.zeros(7, np.int32), np.zeros(7, np.int64)
        _lib.check(eng._lib.oww_bank_score_hits(eng._h, fp, fd, D.B, f.shape[1], _ptr(aid), 7, _ptr(thr), cap, hits.ctypes.data_as(C.c_void_p), _ptr(ns),
                                                _ptr(nt), wp, wd))
        out.append((hits, ns, nt))
    torch.cuda.synchronize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*out)) and (out[0][1] == cap).all()
    assert d_win.cpu().numpy().tobytes() == win_h.tobytes() and not (win_h == -77.0).any()
    assert eng.range_status() is False


# ------------------------------------------------------------------------------------------------ 6. live streams untouched
def test_live_streams_do_not_notice():
    fixed = {n: W.synthetic_head(n, 1234) for n in ("alexa", "hey_mycroft")}
    heads = DB.heads()
    pcm = W.synthetic_pcm(S, 1280 * 5, seed=44)

    def make():
        e = StreamEngine(S, fixed, _emb(), bank_slots=1, bank_capacity=8, feature_ring=HW.BANK_RING)
        b = [e.bank_add(heads[n]) for n in ("n16", "w5", "n22")]
        e.subscribe(range(S), np.array([[b[0]], [b[1]], [b[2]], [-1]], np.int32))
        return e, b

    (a, ba), (b, _) = make(), make()
    try:
        for t in range(5):
            if t == 3:
                got = a.bank_score_hits(_rows(129), ba, 0.0, 64)
                assert [c["n_total"] for c in got] == [3 * 129] * 3 and all(c["windows"].shape[0] == 64 for c in got)
                a.score_hits(_rows(129), 0.0, 64)
            sa, sb = a.step(pcm[:, 1280 * t:1280 * (t + 1)]), b.step(pcm[:, 1280 * t:1280 * (t + 1)])
            assert np.array_equal(sa, sb), f"step {t}: fixed scores"
            assert np.array_equal(a.bank_scores(), b.bank_scores()), f"step {t}: bank scores"
        assert a.export_state(range(S)).tobytes() == b.export_state(range(S)).tobytes()
        assert a.bank_routing() == b.bank_routing()
        assert a.range_status() is False
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_move_nothing_and_a_valid_call_follows(bank):
    eng, ids = bank
    lib, h = eng._lib, eng._h
    f = np.ascontiguousarray(_rows(37))
    n_rows = f.shape[1]
    ok = np.array([ids["n16"], ids["n22"]], np.int32)
    hits, ns, nt = np.full((2, 8, 4), -5, np.int32), np.full(2, -5, np.int32), np.full(2, -5, np.int64)
    off = np.full(3, -5, np.int64)

    def rc(**kw):
        a = dict(feats=_ptr(f), dev=0, B=D.B, n_rows=n_rows, ids=_ptr(ok), n=2, thr=None, cap=8, hits=_ptr(hits), ns=_ptr(ns), nt=_ptr(nt), win=None, wdev=0)
        a.update(kw)
        return lib.oww_bank_score_hits(h, a["feats"], a["dev"], a["B"], a["n_rows"], a["ids"], a["n"], a["thr"], a["cap"], a["hits"], a["ns"], a["nt"],
                                       a["win"], a["wdev"])

    assert rc(cap=0) == EINVAL and b"cap = 0" in lib.oww_last_error() and rc(cap=(1 << 20) + 1) == EINVAL
    assert rc(n=0) == EINVAL and rc(ids=None) == EINVAL and rc(n_rows=21) == EINVAL and rc(B=0) == EINVAL and rc(feats=None) == EINVAL
    for bad in (eng.gone, 15, 16, -1):                          # a dead id, named in the message
        lst = np.array([ids["n16"], bad], np.int32)
        assert rc(ids=_ptr(lst)) == EINVAL and f"{bad} is not a bank head".encode() in lib.oww_last_error()
        assert lib.oww_score_hits_layout(h, _ptr(lst), 2, 8, _ptr(off)) == EINVAL
    thr = np.array([0.5, np.nan], np.float32)
    assert rc(thr=_ptr(thr)) == EINVAL and b"threshold 1" in lib.oww_last_error()
    assert rc(hits=None) == EINVAL and rc(ns=None) == EINVAL and rc(nt=None) == EINVAL
    assert rc(feats=C.c_void_p(f.ctypes.data + 4), dev=1) == EINVAL
    assert rc(win=C.c_void_p(4096 + 4), wdev=1) == EINVAL and b"16-byte aligned" in lib.oww_last_error()
    big = 2 ** 31 - 1
    assert rc(B=big, n_rows=big) == ENOMEM and b"bytes" in lib.oww_last_error()
    assert lib.oww_score_hits_layout(h, _ptr(ok), 2, 0, _ptr(off)) == EINVAL
    raw = C.c_void_p()
    cfg = _lib.Config(0, S, 1, 0, 3, 0, None)
    _lib.check(lib.oww_create(C.byref(cfg), C.byref(raw)))
    try:
        _lib.check(lib.oww_bank_configure(raw, 1, 4))
        assert lib.oww_bank_score_hits(raw, _ptr(f), 0, D.B, n_rows, _ptr(ok), 2, None, 8, _ptr(hits), _ptr(ns), _ptr(nt), None, 0) == ESTATE
    finally:
        lib.oww_destroy(raw)
    assert (hits == -5).all() and (ns == -5).all() and (nt == -5).all() and (off == -5).all()
    with pytest.raises(ValueError):
        eng.bank_score_hits(f, ok, [0.5, 0.5, 0.5])
    # ... and a valid call follows
    assert lib.oww_score_hits_layout(h, _ptr(ok), 2, 8, _ptr(off)) == 0 and list(off) == [0, 8 * 16 * 96, 8 * 16 * 96 + 8 * 22 * 96]
    matrix = eng.bank_score_features(f, ok)
    _check(eng, f, ok, ("n16", "n22"), None, 8, "the valid call after the refusals", matrix)
    assert eng.range_status() is False
