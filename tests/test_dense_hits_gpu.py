"""Ordered hit lists of dense scoring on the device, fixed heads and clips (include/owwhip.h: oww_score_hits / oww_score_clip_hits;
csrc/owwhip_dense.h: the sliding kernel's MASK mode, dense_hits_*_kernel).  The yardstick is the matrix of oww_score_features /
oww_score_clips on the same handle, which tests/test_dense_gpu.py holds to float64 and to oww_head's bits: positions, totals, scores
and windows must equal numpy's statement of the contract (tests/dense_hits_ref.py) on that matrix and the rows, bit for bit -- no
tolerance appears.  Shapes: dense_ref's three sequences at 1 .. 261 windows (the tile and word edges) and T = 1 .. 22, and one array
of 2 x 40,000 windows, the smallest that takes a column's workgroup through more than one compaction turn."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from openwakeword_amd import _lib, utils
from openwakeword_amd import weights as W
from openwakeword_amd.engine import DENSE_HIT, KERNEL_CLASSES, StreamEngine, _ptr

import dense_hits_ref as H
import dense_ref as D
import head_windows as HW

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
S = 4
KINDS = ("median", "max", "above", "zero", "nan0")


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


def _launches(eng):
    t = eng.kernel_times()
    return t[KERNEL_CLASSES[6]]["launches"], t[KERNEL_CLASSES[7]]["launches"]


def _col_T(eng):
    Ts = [0] * eng.n_labels
    for n, (lo, hi) in eng.head_cols.items():
        for c in range(lo, hi):
            Ts[c] = int(eng.heads[n]["T"])
    return Ts


def _check_case(eng, f, label, kinds=KINDS):
    """Every threshold set taken from the handle's own matrix on f: the lists are dense_hits_ref's on that matrix and those rows."""
    matrix = eng.score_features(f)
    Ts, t_max = _col_T(eng), eng.score_shape(f.shape[1])[1]
    cap = matrix.shape[0] * matrix.shape[1]
    thr = H.thresholds_from(matrix)
    for kind in kinds:
        got = eng.score_hits(f, thr[kind], cap)
        want = H.hits(matrix, thr[kind], cap, f, Ts, t_max)
        H.assert_columns_equal(got, want, f"{label} thresholds={kind}")
        totals = [c["n_total"] for c in want]
        if kind == "above":
            assert not any(totals)
        if kind == "zero":
            assert totals == [cap] * len(totals)
        if kind in ("median", "max"):
            assert all(t >= 1 for t in totals)
        if kind == "nan0":
            assert totals[0] == 0 and all(t >= 1 for t in totals[1:])
    assert eng.range_status(clear=True) is False


# ------------------------------------------------------------------------------------------------ 1. every form at the tile and word edges
@pytest.mark.parametrize("form", D.SLIDE_FORMS)
def test_hit_lists_are_numpys_on_the_matrix(form):
    """narrow1-4 (the sliding kernel's MASK mode: one to four nets, gated pairs among them) and wide1-2 (the gather fallback; wide2
    carries a multiclass head) at T 1, 3, 16, 19, 22 and 1, 37, 128, 129, 256, 257, 261 windows per sequence."""
    for T in D.TS:
        eng = StreamEngine(S, D.form_heads(form, T), _emb())
        try:
            for n_win in D.N_WINS:
                _check_case(eng, D.feats()[:, :D.case_rows(n_win, T)], f"{form} T={T} n_win={n_win}")
        finally:
            eng.close()


def _family(form):
    fam = HW.FORMS[form]["fam"]
    return fam[0] if isinstance(fam, tuple) else fam


@pytest.mark.parametrize("form", D.FALLBACK_FORMS)
def test_fallback_forms_at_every_edge(form):
    """Generic, recurrent and fp32 heads (the gather fallback: slab scores ORed into partial mask words, the [windows][NL] score
    scratch) at every T, every n_win and every threshold set, as the sliding forms above."""
    for T in D.TS:
        eng = StreamEngine(S, D.form_heads(form, T), _emb(), use_mfma=_family(form))
        try:
            for n_win in D.N_WINS:
                _check_case(eng, D.feats()[:, :D.case_rows(n_win, T)], f"{form} T={T} n_win={n_win}")
        finally:
            eng.close()


@pytest.mark.parametrize("form,fam", [("fp32_2x64", 0), ("narrow3", 2)])
def test_the_other_kernel_families(form, fam):
    for T in D.TS:
        eng = StreamEngine(S, D.form_heads(form, T), _emb(), use_mfma=fam)
        try:
            for n_win in (37, 129):
                _check_case(eng, D.feats()[:, :D.case_rows(n_win, T)], f"{form} use_mfma={fam} T={T} n_win={n_win}", ("median", "zero", "nan0"))
        finally:
            eng.close()


def test_the_gather_route_gives_the_same_lists(monkeypatch):
    """narrow3 at T = 16 over 261 windows: OWW_DENSE_PATH=ext sends the group down the fallback (slab scores ORed into the mask)."""
    eng = StreamEngine(S, D.form_heads("narrow3", 16), _emb())
    f = D.feats()[:, :D.case_rows(261, 16)]
    try:
        thr = H.thresholds_from(eng.score_features(f))["median"]
        slide = eng.score_hits(f, thr, 783)
        monkeypatch.setenv("OWW_DENSE_PATH", "ext")
        ext = eng.score_hits(f, thr, 783)
        monkeypatch.setenv("OWW_DENSE_SLAB_MB", "1")            # slabs of 170 windows: they start and end inside mask words
        small = eng.score_hits(f, thr, 783)
        monkeypatch.delenv("OWW_DENSE_SLAB_MB")
        monkeypatch.delenv("OWW_DENSE_PATH")
        H.assert_columns_equal(ext, slide, "ext")
        H.assert_columns_equal(small, slide, "ext, 1 MB slabs")
        assert sum(c["n_total"] for c in slide) > 100 and eng.range_status() is False
    finally:
        eng.close()


def test_tile_size_edges():
    for form, Ts in D.EDGES:
        for T in Ts:
            eng = StreamEngine(S, D.form_heads(form, T), _emb())
            try:
                for n_win in D.EDGE_N_WINS:
                    _check_case(eng, D.feats()[:, :D.case_rows(n_win, T)], f"{form} T={T} n_win={n_win}", ("median",))
            finally:
                eng.close()


def _mixed_heads():
    shapes = HW.FORMS["narrow4"]["heads"]
    return {f"mix{T}": HW.centre(HW.draw_head(f"mix{T}", shapes[i], T, seed=D.HEAD_SEED),
                                 np.ascontiguousarray(D.windows_of(D.feats(), T, 22)).reshape(-1, T, 96)) for i, T in enumerate((5, 16, 22))}


# ------------------------------------------------------------------------------------------------ 2. capacity
def test_capacity_keeps_the_first_hits_and_writes_nothing_behind_them():
    """Heads of T = 5, 16, 22 on one handle, 261 windows: cap = 1, a column's total and its total - 1.  The stored prefix is the first
    cap hits in order, n_total does not notice, and a guard pattern in the caller's buffers -- behind every column's stored records
    and windows, and behind the buffers' ends -- survives."""
    eng = StreamEngine(S, _mixed_heads(), _emb())
    f = D.feats()[:, :D.case_rows(261, 22)]
    try:
        matrix = eng.score_features(f)
        thr = H.thresholds_from(matrix)["median"]               # column 0: half of its windows; column 1: a quarter; column 2: its maximum
        thr[1] = np.sort(matrix[:, :, 1].ravel())[matrix[:, :, 1].size * 3 // 4]
        thr[2] = matrix[:, :, 2].max()
        Ts = _col_T(eng)
        full = H.hits(matrix, thr, 10 ** 6, f, Ts, 22)
        total = full[0]["n_total"]
        assert total > 2 and len({c["n_total"] for c in full}) > 1
        fc = np.ascontiguousarray(f)
        fp = _ptr(fc)
        for cap in (1, total, total - 1):
            want = H.hits(matrix, thr, cap, f, Ts, 22)
            H.assert_columns_equal(eng.score_hits(f, thr, cap), want, f"cap={cap}")
            off = eng.score_hits_layout(cap)
            assert list(off) == list(np.cumsum([0] + [cap * T * 96 for T in Ts]))
            flat = np.full((3 * cap + 8) * 4, 0x5A5A5A5A, np.int32)
            win = np.full(int(off[-1]) + 64, np.float32(-77.0), np.float32)
            ns, nt = np.zeros(3, np.int32), np.zeros(3, np.int64)
            _lib.check(eng._lib.oww_score_hits(eng._h, fp, 0, D.B, f.shape[1], _ptr(thr), cap, _ptr(flat), _ptr(ns), _ptr(nt), _ptr(win), 0))
            rec = flat.view(DENSE_HIT)
            assert list(nt) == [c["n_total"] for c in full] and list(ns) == [min(c["n_total"], cap) for c in full]
            for c in range(3):
                n = int(ns[c])
                got = rec[c * cap:c * cap + n]
                assert np.array_equal(got["seq"], want[c]["seq"]) and np.array_equal(got["window"], want[c]["window"]) and not got["reserved"].any()
                assert got["score"].tobytes() == want[c]["score"].tobytes()
                assert (flat[(c * cap + n) * 4:(c + 1) * cap * 4] == 0x5A5A5A5A).all(), f"cap={cap} column {c}: records behind the list"
                assert win[off[c]:off[c] + n * Ts[c] * 96].tobytes() == want[c]["windows"].tobytes()
                assert (win[off[c] + n * Ts[c] * 96:off[c + 1]] == -77.0).all(), f"cap={cap} column {c}: windows behind the list"
            assert (flat[3 * cap * 4:] == 0x5A5A5A5A).all() and (win[off[-1]:] == -77.0).all(), f"cap={cap}: behind the buffers"
        # windows NULL: the lists alone
        bare = eng.score_hits(f, thr, total, return_windows=False)
        assert all(c["windows"] is None for c in bare)
        H.assert_columns_equal(bare, H.hits(matrix, thr, total), "no windows")
    finally:
        eng.close()


def test_a_long_array_takes_several_compaction_turns_and_slabs(monkeypatch):
    """Two sequences of 40,000 windows (T = 3): a column has 2,500 mask words, so its workgroup walks three turns of 1,024 words and
    carries the running offset across them; with a 4 MB slab budget the 40,000 stored hits are re-scored in 11 pieces, whose records
    and windows land behind one another.  cap 30,000 cuts the list inside the second sequence."""
    T, nw = 3, 40000
    f = np.random.default_rng(77).normal(0.0, 1.0, (2, nw + T - 1, 96)).astype(np.float32)
    eng = StreamEngine(S, D.form_heads("narrow1", T), _emb())
    try:
        matrix = eng.score_features(f)
        thr = H.thresholds_from(matrix)["median"]
        monkeypatch.setenv("OWW_DENSE_SLAB_MB", "4")
        for cap in (2 * nw, 30000):
            want = H.hits(matrix, thr, cap, f, [T], T)
            assert want[0]["n_total"] >= nw and want[0]["seq"][-1] == 1
            H.assert_columns_equal(eng.score_hits(f, thr, cap), want, f"cap={cap}")
        assert eng.range_status() is False
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. independence
def test_lists_depend_on_a_windows_rows_alone():
    """A sliding group (narrow3, T = 16) and a fallback head (wide1, T = 16) on one handle, 261 windows: chunks overlapping by
    t_max - 1 rows merge to the whole array's lists; another batch size and order of sequences only permutes seq."""
    heads = {**D.form_heads("narrow3", 16), **D.form_heads("wide1", 16)}
    f = D.feats()[:, :D.case_rows(261, 16)]
    eng = StreamEngine(S, heads, _emb())
    try:
        matrix = eng.score_features(f)
        thr = H.thresholds_from(matrix)["median"]
        whole = eng.score_hits(f, thr, 783)
        H.assert_columns_equal(whole, H.hits(matrix, thr, 783, f, [16] * 3, 16), "whole")
        labels = ["c0", "c1", "c2"]
        bm = types.SimpleNamespace(engine=eng, labels=labels,
                                   score_hits=lambda x, t, cap: dict(zip(labels, eng.score_hits(x, t, cap))))
        for chunk_rows in (1 << 18, 100, 47):
            for b in range(D.B):
                got = utils.mine_feature_file(f[b], bm, thr, chunk_rows=chunk_rows)
                for c, lab in enumerate(labels):
                    sel = whole[c]["seq"] == b
                    assert got[lab]["n_total"] == int(sel.sum()) and np.array_equal(got[lab]["window"], whole[c]["window"][sel]), f"chunks of {chunk_rows}"
                    assert got[lab]["score"].tobytes() == whole[c]["score"][sel].tobytes()
                    assert got[lab]["windows"].tobytes() == whole[c]["windows"][sel].tobytes()
        perm = [2, 0, 1]
        moved = eng.score_hits(np.ascontiguousarray(f[perm]), thr, 783)
        pair = eng.score_hits(np.ascontiguousarray(f[1:]), thr, 783)
        for c in range(3):
            for new, old in enumerate(perm):
                a, b = moved[c]["seq"] == new, whole[c]["seq"] == old
                assert np.array_equal(moved[c]["window"][a], whole[c]["window"][b]) and moved[c]["score"][a].tobytes() == whole[c]["score"][b].tobytes()
                assert moved[c]["windows"][a].tobytes() == whole[c]["windows"][b].tobytes()
            rest = whole[c]["seq"] >= 1
            assert np.array_equal(pair[c]["seq"] + 1, whole[c]["seq"][rest]) and np.array_equal(pair[c]["window"], whole[c]["window"][rest])
            assert pair[c]["score"].tobytes() == whole[c]["score"][rest].tobytes()
        assert eng.range_status() is False
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. clips
def _smoke_heads():
    return {n: W.synthetic_head(n, 1234) for n in ("alexa", "hey_mycroft", "hey_jarvis")}


@functools.lru_cache(maxsize=None)
def _clips():
    x = W.synthetic_pcm(3, 64000, seed=21, rms=3000.0).astype(np.float64) * np.array([1.0, 0.1, 0.01])[:, None]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def test_clip_hits_are_numpys_on_score_clips():
    eng = StreamEngine(S, _smoke_heads(), _emb())
    try:
        matrix, emb = eng.score_clips(_clips(), return_features=True)
        thr = H.thresholds_from(matrix)
        for kind in ("median", "zero", "above"):
            got = eng.score_clip_hits(_clips(), thr[kind], 128)
            H.assert_columns_equal(got, H.hits(matrix, thr[kind], 128, emb, [16] * 3, 16), f"clips thresholds={kind}")
        one = eng.score_clip_hits(_clips()[1:2], thr["median"], 128)
        H.assert_columns_equal(one, H.hits(matrix[1:2], thr["median"], 128, emb[1:2], [16] * 3, 16), "one clip")
        assert eng.range_status() is False
    finally:
        eng.close()


def test_mine_clip_hits_is_mine_windows_bit_for_bit():
    from openwakeword_amd.model import BatchedModel
    names = ["alexa", "hey_mycroft", "hey_jarvis"]
    bm = BatchedModel(2, names, weights="synthetic")            # three clips: two calls
    try:
        raw = bm.engine.score_clips(_clips()[:2])
        thr = float(np.sort(raw.ravel())[raw.size // 2])
        want = utils.mine_windows(_clips(), bm, threshold=thr)
        got = utils.mine_clip_hits(_clips(), bm, threshold=thr)
        assert list(got) == list(want) == names and sum(v.shape[0] for v in want.values()) > 0
        for n in names:
            assert got[n].shape == want[n].shape and got[n].dtype == np.float32 and got[n].tobytes() == want[n].tobytes(), n
        lists = bm.score_clip_hits(_clips(), {names[0]: thr}, cap=5)
        sc = bm.score_clips(_clips())
        b, w = np.nonzero(sc[names[0]] >= np.float32(thr))
        assert lists[names[0]]["n_total"] == b.size and np.array_equal(lists[names[0]]["seq"], b[:5]) and np.array_equal(lists[names[0]]["window"], w[:5])
        assert lists[names[1]]["n_total"] == int((sc[names[1]] >= np.float32(0.5)).sum())
    finally:
        bm.close()


def test_device_resident_features_clips_and_windows_give_the_host_routes_bytes():
    """feats_on_device, pcm_on_device and windows_on_device = 1 with torch's buffers: the records and the window bytes (copied device to
    device, read back here) are the host route's.  Heads of T = 5, 16, 22 (a sliding group) beside a wide head (the fallback)."""
    import torch
    heads = {**_mixed_heads(), **D.form_heads("wide1", 16)}
    f = np.ascontiguousarray(D.feats()[:, :D.case_rows(129, 22)])
    eng = StreamEngine(S, heads, _emb())
    try:
        nc, cap = eng.n_labels, 64
        thr = H.thresholds_from(eng.score_features(f))["median"]
        off = eng.score_hits_layout(cap)

        def run(call, windows_ptr, on_device):
            hits, ns, nt = np.zeros((nc, cap), DENSE_HIT), np.zeros(nc, np.int32), np.zeros(nc, np.int64)
            _lib.check(call(hits.ctypes.data_as(C.c_void_p), _ptr(ns), _ptr(nt), windows_ptr, on_device))
            return hits, ns, nt

        lib, h = eng._lib, eng._h
        d_f = torch.from_numpy(f).cuda()
        win_h = np.full(int(off[-1]), np.float32(-77.0), np.float32)
        d_win = torch.full((int(off[-1]),), -77.0, device="cuda")
        host = run(lambda hp, ns, nt, wp, wd: lib.oww_score_hits(h, _ptr(f), 0, D.B, f.shape[1], _ptr(thr), cap, hp, ns, nt, wp, wd), _ptr(win_h), 0)
        dev = run(lambda hp, ns, nt, wp, wd: lib.oww_score_hits(h, C.c_void_p(d_f.data_ptr()), 1, D.B, f.shape[1], _ptr(thr), cap, hp, ns, nt, wp, wd),
                  C.c_void_p(d_win.data_ptr()), 1)
        torch.cuda.synchronize()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host, dev)) and host[1].min() >= 1
        assert d_win.cpu().numpy().tobytes() == win_h.tobytes() and (win_h != -77.0).any()
        # clips: device PCM in, device windows out
        pcm = np.ascontiguousarray(_clips())
        n_rows = (((pcm.shape[1] - 512) // 160 + 1) - 76) // 8 + 1
        cthr = H.thresholds_from(eng.score_clips(pcm))["median"]
        d_pcm = torch.from_numpy(pcm).cuda()
        win_h[:] = -77.0
        d_win.fill_(-77.0)
        host = run(lambda hp, ns, nt, wp, wd: lib.oww_score_clip_hits(h, _ptr(pcm), 0, 3, pcm.shape[1], _ptr(cthr), cap, hp, ns, nt, wp, wd), _ptr(win_h), 0)
        dev = run(lambda hp, ns, nt, wp, wd: lib.oww_score_clip_hits(h, C.c_void_p(d_pcm.data_ptr()), 1, 3, pcm.shape[1], _ptr(cthr), cap, hp, ns, nt, wp, wd),
                  C.c_void_p(d_win.data_ptr()), 1)
        torch.cuda.synchronize()
        assert n_rows == 41 and all(a.tobytes() == b.tobytes() for a, b in zip(host, dev)) and host[1].min() >= 1
        assert d_win.cpu().numpy().tobytes() == win_h.tobytes() and (win_h != -77.0).any()
        assert eng.range_status() is False
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. no matrix, no side effects
def test_launch_counts_of_a_call_without_and_with_hits():
    """narrow3 at T = 16 (two sliding passes): a call without hits is the matrix entry's heads launches plus ONE class-7 launch, the
    compaction -- no gather, no re-score.  With hits in both columns: per column one gather, one re-score launch, one score pass."""
    eng = StreamEngine(S, D.form_heads("narrow3", 16), _emb())
    f = D.feats()[:, :D.case_rows(261, 16)]
    try:
        eng.enable_timing(True)
        eng.kernel_times()
        matrix = eng.score_features(f)
        assert _launches(eng) == (2, 0)
        thr = H.thresholds_from(matrix)
        none = eng.score_hits(f, thr["above"], 64)
        assert _launches(eng) == (2, 1) and not any(c["n_total"] for c in none)
        some = eng.score_hits(f, thr["max"], 64)
        assert _launches(eng) == (2 + 2, 1 + 2 * 2) and all(c["n_total"] >= 1 for c in some)
        assert eng.range_status() is False
    finally:
        eng.close()


def test_live_streams_do_not_notice_hit_lists():
    """Two handles with events and audio rings stepped on the same PCM; one mines features and clips between steps.  Their next steps
    return the same scores, feature rings, event records, event features and audio."""
    kw = dict(event_capacity=16, event_features=4, audio_chunks=4, event_audio=2)
    pcm = W.synthetic_pcm(S, 1280 * 12, seed=42)
    a, b = StreamEngine(S, _smoke_heads(), _emb(), **kw), StreamEngine(S, _smoke_heads(), _emb(), **kw)
    try:
        for e in (a, b):
            e.set_event_thresholds(np.zeros(3, np.float32))
        mined = 0
        for t in range(9):
            if t in (6, 7, 8):
                mined += sum(c["n_total"] for c in a.score_hits(D.feats()[:, :60], 0.0, 32))
                mined += sum(c["n_total"] for c in a.score_clip_hits(_clips(), 0.0, 32))
            sa, sb = a.step(pcm[:, 1280 * t:1280 * (t + 1)]), b.step(pcm[:, 1280 * t:1280 * (t + 1)])
            assert np.array_equal(sa, sb), f"step {t}"
            (ra, na), (rb, nb) = a.events(), b.events()
            assert na == nb and ra.tobytes() == rb.tobytes(), f"step {t}: events"
            assert np.array_equal(a.event_features(), b.event_features()) and np.array_equal(a.event_audio(), b.event_audio())
            for s in range(S):
                assert np.array_equal(a.get_features(s, 16), b.get_features(s, 16)), f"step {t} stream {s}"
            assert np.array_equal(a.audio(range(S), 4)[0], b.audio(range(S), 4)[0])
        assert na > 0 and mined == 3 * (3 * 45 * 3 + 3 * 26 * 3) and a.range_status() is False
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_untouched():
    pcm = W.synthetic_pcm(S, 1280 * 8, seed=43)
    a, b = StreamEngine(S, _smoke_heads(), _emb()), StreamEngine(S, _smoke_heads(), _emb())
    bank = StreamEngine(S, {}, _emb(), bank_slots=2, bank_capacity=4)
    try:
        for t in range(6):
            a.step(pcm[:, 1280 * t:1280 * (t + 1)]); b.step(pcm[:, 1280 * t:1280 * (t + 1)])
        lib, f, clips = a._lib, np.ascontiguousarray(D.feats()[:, :40]), _clips()
        hits = np.full((3, 8, 4), -5, np.int32)
        ns, nt, off = np.full(3, -5, np.int32), np.full(3, -5, np.int64), np.full(4, -5, np.int64)

        def feat_call(h=a._h, fp=_ptr(f), B=3, n_rows=40, cap=8, hp=_ptr(hits), nsp=_ptr(ns), ntp=_ptr(nt), wp=None, wd=0):
            return lib.oww_score_hits(h, fp, 0, B, n_rows, None, cap, hp, nsp, ntp, wp, wd)

        def clip_call(h=a._h, B=3, n=64000, cap=8, hp=_ptr(hits)):
            return lib.oww_score_clip_hits(h, _ptr(clips), 0, B, n, None, cap, hp, _ptr(ns), _ptr(nt), None, 0)

        assert feat_call(cap=0) == EINVAL and b"cap = 0" in lib.oww_last_error()
        assert feat_call(cap=(1 << 20) + 1) == EINVAL
        assert feat_call(n_rows=15) == EINVAL and feat_call(B=0) == EINVAL and feat_call(fp=None) == EINVAL
        assert feat_call(hp=None) == EINVAL and feat_call(nsp=None) == EINVAL and feat_call(ntp=None) == EINVAL
        assert feat_call(wp=C.c_void_p(4096 + 4), wd=1) == EINVAL and b"16-byte aligned" in lib.oww_last_error()      # (refused before it is touched)
        assert clip_call(cap=0) == EINVAL and clip_call(B=0) == EINVAL and clip_call(B=a.n_streams_padded + 1) == EINVAL
        assert clip_call(n=12512 + 14 * 1280) == EINVAL and clip_call(hp=None) == EINVAL
        assert lib.oww_score_hits_layout(a._h, None, 0, 0, _ptr(off)) == EINVAL and lib.oww_score_hits_layout(a._h, None, 0, 8, None) == EINVAL
        assert lib.oww_score_hits_layout(a._h, None, 0, 8, _ptr(off)) == 0 and list(off) == [0, 8 * 16 * 96, 16 * 16 * 96, 24 * 16 * 96]
        off[:] = -5
        # a handle with bank heads only; the bank entry on a handle without a bank
        assert feat_call(h=bank._h) == EINVAL and clip_call(h=bank._h) == EINVAL and lib.oww_score_hits_layout(bank._h, None, 0, 8, _ptr(off)) == EINVAL
        one = np.zeros(1, np.int32)
        assert lib.oww_bank_score_hits(a._h, _ptr(f), 0, 3, 40, _ptr(one), 1, None, 8, _ptr(hits), _ptr(ns), _ptr(nt), None, 0) == ESTATE
        assert lib.oww_score_hits_layout(a._h, _ptr(one), 1, 8, _ptr(off)) == ESTATE
        # before commit
        raw = C.c_void_p()
        cfg = _lib.Config(0, S, 1, 0, 3, 0, None)
        _lib.check(lib.oww_create(C.byref(cfg), C.byref(raw)))
        try:
            assert feat_call(h=raw) == ESTATE and clip_call(h=raw) == ESTATE and lib.oww_score_hits_layout(raw, None, 0, 8, _ptr(off)) == ESTATE
        finally:
            lib.oww_destroy(raw)
        assert feat_call(h=None) == ESTATE
        assert (hits == -5).all() and (ns == -5).all() and (nt == -5).all() and (off == -5).all()
        with pytest.raises(_lib.OwwError):
            a.score_hits(D.feats()[:, :15])
        for t in range(6, 8):
            assert np.array_equal(a.step(pcm[:, 1280 * t:1280 * (t + 1)]), b.step(pcm[:, 1280 * t:1280 * (t + 1)])), f"step {t}"
        assert a.range_status() is False
    finally:
        a.close(); b.close(); bank.close()
