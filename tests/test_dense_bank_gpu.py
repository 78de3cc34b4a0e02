"""Dense scoring over the head bank on the device (include/owwhip.h: oww_bank_score_features / oww_bank_score_stats;
csrc/owwhip_dense.h: heads_dense_bank_kernel).  The contract: column i of the matrix is BIT FOR BIT what the same net scores as a fixed
head through oww_score_features (a twin handle carrying that one head), within TOL_SCORE of the float64 oracle, and the statistics are
exactly numpy's on that matrix.  Shapes: three sequences of dense_ref.feats(), 1 .. 261 windows (the tile edges), seven bank heads of
T = 1 .. 22 in one call -- five narrow (one launch of the sliding kernel) and two wide (the fallback) -- on a handle whose ids have a
hole.  The CPU tier (test_dense_bank_cpu.py) admits the heads.  pytest -m gpu -s prints the worst error."""
import ctypes as C
import functools

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import KERNEL_CLASSES, StreamEngine, _ptr

import dense_bank_ref as DB
import dense_ref as D
import head_windows as HW

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ESTATE = -1, -4, -3
S = 4


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


def _rows(n_win, t_max=DB.T_MAX):
    return D.feats()[:, :D.case_rows(n_win, t_max)]


def _launches(eng):
    t = eng.kernel_times()
    return t[KERNEL_CLASSES[6]]["launches"], t[KERNEL_CLASSES[7]]["launches"]


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    assert a.tobytes() == b.tobytes(), f"{what}: differs at {np.argwhere(a != b)[:6].tolist()}"


@pytest.fixture(scope="module")
def bank():
    """(engine, {name: bank id}): S = 4 streams, no fixed heads, one bank slot; the seven heads added in a shuffled order with one head
    more added in between and removed again, so the ids have a hole."""
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


@pytest.fixture(scope="module")
def twins():
    """{name: [3, windows, 1]}: each head alone as the FIXED head of a handle of its own, through oww_score_features over the rows of
    the largest case (computed once, read-only).  Window w of the bank call at t_max = 22 is the twin's window w + 22 - T."""
    f = _rows(max(DB.N_WINS))
    out = {}
    for n, h in DB.heads().items():
        eng = StreamEngine(S, {n: h}, _emb())
        try:
            out[n] = eng.score_features(f)
            assert eng.range_status() is False
        finally:
            eng.close()
        out[n].setflags(write=False)
    return out


def _twin_cols(twins, names, n_win, t_max=DB.T_MAX):
    cols = []
    for n in names:
        off = t_max - int(DB.heads()[n]["T"])
        cols.append(twins[n][:, off:off + n_win, 0])
    return np.stack(cols, axis=2)


# ------------------------------------------------------------------------------------------------ 1. mixed T in one call, both paths
def test_seven_heads_of_mixed_length_in_one_call(bank, twins):
    eng, ids = bank
    names = list(DB.NARROW + DB.WIDE)
    worst = [0.0]
    for n_win in DB.N_WINS:
        f = _rows(n_win)
        assert eng.bank_score_shape([ids[n] for n in names], f.shape[1]) == (n_win, DB.T_MAX)
        eng.kernel_times()
        got = eng.bank_score_features(f, [ids[n] for n in names])
        launches = _launches(eng)
        flag = eng.range_status(clear=True)
        assert got.shape == (D.B, n_win, 7)
        # one sliding launch for the five narrow heads; per wide head one gather, one heads launch, one scatter
        assert launches == (1 + 2, 2 + 2), f"n_win={n_win}: {launches}"
        for i, n in enumerate(names):
            HW.check_scores(f"{n} n_win={n_win}", got[:, :, i:i + 1], DB.want()[n][:, :n_win], flag, worst)
        _same(got, _twin_cols(twins, names, n_win), f"n_win={n_win} against the fixed-head twins")
        eng.kernel_times()
        narrow = eng.bank_score_features(f, [ids[n] for n in DB.NARROW])
        assert _launches(eng) == (1, 0), f"n_win={n_win}: the narrow heads alone"
        _same(narrow, got[:, :, :5], f"n_win={n_win}: the narrow heads alone")
    print(f"\nseven bank heads, T 1 .. 22, n_win {DB.N_WINS}: worst |score - float64| = {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ 2. slice edges
@pytest.mark.parametrize("n_win", (129, 261))
def test_heads_per_workgroup_do_not_change_a_bit(bank, twins, monkeypatch, n_win):
    eng, ids = bank
    f = _rows(n_win)
    nid = [ids[n] for n in DB.NARROW]
    monkeypatch.delenv("OWW_DENSE_BANK_HPW", raising=False)
    base = eng.bank_score_features(f, nid)
    _same(base, _twin_cols(twins, DB.NARROW, n_win), "the plan's own hpw against the twins")
    for hpw in DB.HPWS:
        monkeypatch.setenv("OWW_DENSE_BANK_HPW", str(hpw))
        eng.kernel_times()
        _same(eng.bank_score_features(f, nid), base, f"hpw={hpw}")
        assert _launches(eng) == (1, 0)
        _same(eng.bank_score_features(f, nid[::-1]), base[:, :, ::-1], f"hpw={hpw}, ids reversed")
        dup = [nid[2], nid[0], nid[2], nid[4], nid[2]]
        _same(eng.bank_score_features(f, dup), base[:, :, [2, 0, 2, 4, 2]], f"hpw={hpw}, a duplicated id")
        st = eng.bank_score_stats(f, nid)
        for k, v in DB.np_stats(base).items():
            _same(st[k], v, f"hpw={hpw}: {k}")
    monkeypatch.delenv("OWW_DENSE_BANK_HPW")
    # one head per call: t_max is then the head's own T, and its windows start t_max - T rows earlier
    for i, n in enumerate(DB.NARROW):
        T = int(DB.heads()[n]["T"])
        assert eng.bank_score_shape([nid[i]], f.shape[1]) == (f.shape[1] - T + 1, T)
        one = eng.bank_score_features(f, [nid[i]])
        _same(one[:, DB.T_MAX - T:DB.T_MAX - T + n_win], base[:, :, i:i + 1], f"{n} alone")
    assert eng.range_status() is False


# ------------------------------------------------------------------------------------------------ 3. tile-size edge
def test_tile_size_edge_and_the_longest_window():
    """Tiles of 256 windows while the rows of t_s fit beside a two-slot ring (113), tiles of 128 beyond (114, 120)."""
    eng = StreamEngine(S, {}, _emb(), bank_slots=1, bank_capacity=4, feature_ring=HW.T_MAX)
    worst = [0.0]
    try:
        eng.enable_timing(True)
        for T in DB.EDGE_TS:
            h = DB.edge_head(T)
            bid = eng.bank_add(h)
            f = _rows(max(DB.EDGE_N_WINS), T)
            twin = StreamEngine(S, {"e": h}, _emb())
            try:
                want_bits = twin.score_features(f)
            finally:
                twin.close()
            ref = D.dense_ref(f, {"e": h})["e"]
            for n_win in DB.EDGE_N_WINS:
                eng.kernel_times()
                got = eng.bank_score_features(f[:, :D.case_rows(n_win, T)], [bid])
                assert _launches(eng) == (1, 0)
                HW.check_scores(f"T={T} n_win={n_win}", got, ref[:, :n_win], eng.range_status(clear=True), worst)
                _same(got, want_bits[:, :n_win], f"T={T} n_win={n_win} against the twin")
                st = eng.bank_score_stats(f[:, :D.case_rows(n_win, T)], [bid])
                for k, v in DB.np_stats(got).items():
                    _same(st[k], v, f"T={T} n_win={n_win}: {k}")
            eng.bank_remove(bid)
    finally:
        eng.close()
    print(f"\nnarrow bank heads at T {DB.EDGE_TS}: worst |score - float64| = {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ 4. statistics
@pytest.mark.parametrize("path", ("default", "ext"))
def test_statistics_are_numpys_on_the_matrix(bank, twins, monkeypatch, path):
    eng, ids = bank
    names = list(DB.NARROW + DB.WIDE)
    aid = [ids[n] for n in names]
    if path == "ext":
        monkeypatch.setenv("OWW_DENSE_PATH", "ext")
    for n_win in (1, 37, 261):
        f = _rows(n_win)
        matrix = _twin_cols(twins, names, n_win)                 # (test 1 holds the entry's matrix to these bits)
        occurring = [float(np.sort(matrix[:, :, k].ravel())[matrix[:, :, k].size // 2]) for k in range(7)]
        for thr in (None, occurring, [0.0] * 7, [1.0] * 7):
            want = DB.np_stats(matrix, thr)
            eng.kernel_times()
            got = eng.bank_score_stats(f, aid, thr)
            launches = _launches(eng)
            again = eng.bank_score_stats(f, aid, thr)
            for k in ("count", "max", "argmax"):
                _same(got[k], want[k], f"{path} n_win={n_win} thresholds={'0.5' if thr is None else thr[0]}: {k}")
                _same(again[k], got[k], f"{path} n_win={n_win}: {k} of the repeated call")
            assert launches == ((1 + 2, 2 + 2) if path == "default" else (7, 14)), launches
        assert (DB.np_stats(matrix, occurring)["count"].sum(axis=0) > 0).all() and (DB.np_stats(matrix, [0.0] * 7)["count"] == n_win).all()
    assert eng.range_status() is False


# ------------------------------------------------------------------------------------------------ 5. OWW_DENSE_PATH=ext
def test_the_gather_route_equals_the_sliding_route(bank, monkeypatch):
    eng, ids = bank
    nid = [ids[n] for n in DB.NARROW]
    f = _rows(261)
    eng.kernel_times()
    slide = eng.bank_score_features(f, nid)
    assert _launches(eng) == (1, 0)
    monkeypatch.setenv("OWW_DENSE_PATH", "ext")
    ext = eng.bank_score_features(f, nid)
    assert _launches(eng) == (5, 10)                             # per head: a gather, heads_bank_kernel, a scatter
    monkeypatch.delenv("OWW_DENSE_PATH")
    _same(slide, ext, "sliding against gathered")
    assert eng.range_status() is False


# ------------------------------------------------------------------------------------------------ 6. live streams untouched
def test_live_streams_do_not_notice(twins):
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
            if t == 3:                                           # between steps 2 and 3
                got = a.bank_score_features(_rows(129), ba)
                _same(got, _twin_cols(twins, ("n16", "w5", "n22"), 129), "the call in between")
                a.bank_score_stats(_rows(129), ba)
            sa, sb = a.step(pcm[:, 1280 * t:1280 * (t + 1)]), b.step(pcm[:, 1280 * t:1280 * (t + 1)])
            _same(sa, sb, f"step {t}: fixed scores")
            _same(a.bank_scores(), b.bank_scores(), f"step {t}: bank scores")
        _same(a.export_state(range(S)), b.export_state(range(S)), "stream state records")
        assert a.bank_routing() == b.bank_routing()
        assert a.range_status() is False
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_move_nothing_and_a_valid_call_follows(bank, twins):
    eng, ids = bank
    lib, h = eng._lib, eng._h
    f = np.ascontiguousarray(_rows(37))
    n_rows = f.shape[1]
    ok = np.array([ids["n16"], ids["n22"]], np.int32)
    out = np.zeros((D.B, 37, 2), np.float32)
    cnt, mx, am = np.zeros((D.B, 2), np.int32), np.zeros((D.B, 2), np.float32), np.zeros((D.B, 2), np.int32)
    nw, tm = C.c_int32(-7), C.c_int32(-7)

    def feats_rc(**kw):
        a = dict(feats=_ptr(f), dev=0, B=D.B, n_rows=n_rows, ids=_ptr(ok), n=2, out=_ptr(out), odev=0)
        a.update(kw)
        return lib.oww_bank_score_features(h, a["feats"], a["dev"], a["B"], a["n_rows"], a["ids"], a["n"], a["out"], a["odev"])

    def stats_rc(**kw):
        a = dict(feats=_ptr(f), dev=0, B=D.B, n_rows=n_rows, ids=_ptr(ok), n=2, thr=None, cnt=_ptr(cnt), mx=_ptr(mx), am=_ptr(am))
        a.update(kw)
        return lib.oww_bank_score_stats(h, a["feats"], a["dev"], a["B"], a["n_rows"], a["ids"], a["n"], a["thr"], a["cnt"], a["mx"], a["am"])

    # n_ids < 1, a null list
    assert lib.oww_bank_score_shape(h, _ptr(ok), 0, n_rows, C.byref(nw), C.byref(tm)) == EINVAL and (nw.value, tm.value) == (-7, -7)
    assert feats_rc(n=0) == EINVAL and stats_rc(n=0) == EINVAL and feats_rc(ids=None) == EINVAL and stats_rc(n=-1) == EINVAL
    # an id that is not live: the removed head, an id never used, one outside the bank -- named in the message
    for bad in (eng.gone, 15, 16, -1):
        lst = np.array([ids["n16"], bad], np.int32)
        assert lib.oww_bank_score_shape(h, _ptr(lst), 2, n_rows, None, None) == EINVAL
        assert f"{bad} is not a bank head".encode() in lib.oww_last_error()
        assert feats_rc(ids=_ptr(lst)) == EINVAL and stats_rc(ids=_ptr(lst)) == EINVAL
    # n_rows < t_max (22 for this list)
    assert lib.oww_bank_score_shape(h, _ptr(ok), 2, 21, C.byref(nw), C.byref(tm)) == EINVAL and (nw.value, tm.value) == (-7, -7)
    assert feats_rc(n_rows=21) == EINVAL and stats_rc(n_rows=21) == EINVAL
    assert lib.oww_bank_score_shape(h, _ptr(ok), 2, 22, C.byref(nw), None) == 0 and nw.value == 1
    # a NaN threshold
    thr = np.array([0.5, np.nan], np.float32)
    assert stats_rc(thr=_ptr(thr)) == EINVAL and b"threshold 1" in lib.oww_last_error()
    # null pointers, B = 0, misaligned device pointers (refused before anything reads them)
    assert feats_rc(feats=None) == EINVAL and feats_rc(out=None) == EINVAL and feats_rc(B=0) == EINVAL
    assert stats_rc(feats=None) == EINVAL and stats_rc(cnt=None) == EINVAL and stats_rc(mx=None) == EINVAL and stats_rc(am=None) == EINVAL
    assert feats_rc(feats=C.c_void_p(f.ctypes.data + 4), dev=1) == EINVAL and stats_rc(feats=C.c_void_p(f.ctypes.data + 4), dev=1) == EINVAL
    assert feats_rc(out=C.c_void_p(out.ctypes.data + 4), odev=1) == EINVAL
    # sizes: 64-bit, the bytes in the message
    big = 2 ** 31 - 1
    assert feats_rc(B=big, n_rows=big) == ENOMEM and b"bytes" in lib.oww_last_error()
    assert stats_rc(B=big, n_rows=big) == ENOMEM and b"bytes" in lib.oww_last_error()
    # a handle without a bank, a handle before commit, no handle
    plain = StreamEngine(S, {"alexa": W.synthetic_head("alexa", 1234)}, _emb())
    try:
        assert lib.oww_bank_score_shape(plain._h, _ptr(ok), 2, n_rows, None, None) == ESTATE
        assert lib.oww_bank_score_features(plain._h, _ptr(f), 0, D.B, n_rows, _ptr(ok), 2, _ptr(out), 0) == ESTATE
        assert lib.oww_bank_score_stats(plain._h, _ptr(f), 0, D.B, n_rows, _ptr(ok), 2, None, _ptr(cnt), _ptr(mx), _ptr(am)) == ESTATE
    finally:
        plain.close()
    raw = C.c_void_p()
    cfg = _lib.Config(0, S, 1, 0, 3, 0, None)
    _lib.check(lib.oww_create(C.byref(cfg), C.byref(raw)))
    try:
        _lib.check(lib.oww_bank_configure(raw, 1, 4))
        assert lib.oww_bank_score_shape(raw, _ptr(ok), 2, n_rows, None, None) == ESTATE
        assert lib.oww_bank_score_features(raw, _ptr(f), 0, D.B, n_rows, _ptr(ok), 2, _ptr(out), 0) == ESTATE
        assert lib.oww_bank_score_stats(raw, _ptr(f), 0, D.B, n_rows, _ptr(ok), 2, None, _ptr(cnt), _ptr(mx), _ptr(am)) == ESTATE
    finally:
        lib.oww_destroy(raw)
    assert lib.oww_bank_score_shape(None, _ptr(ok), 2, n_rows, None, None) == ESTATE
    with pytest.raises(_lib.OwwError):
        eng.bank_score_features(f[:, :21], ok)
    with pytest.raises(ValueError):
        eng.bank_score_stats(f, ok, [0.5])
    assert not out.any() and not cnt.any() and not mx.any() and not am.any()
    # ... and a valid call follows
    assert feats_rc() == 0 and stats_rc() == 0
    want = _twin_cols(twins, ("n16", "n22"), 37)
    _same(out, want, "the valid call after the refusals")
    for k, v in zip(("count", "max", "argmax"), (cnt, mx, am)):
        _same(v, DB.np_stats(want)[k], k)
    assert eng.range_status() is False
