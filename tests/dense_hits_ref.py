"""Shared by the hit-list tests (include/owwhip.h: oww_score_hits / oww_score_clip_hits / oww_bank_score_hits): numpy's statement of the
contract on a score matrix and the rows it was computed from, and the comparison of a call's columns with it.  HIP-free."""
import numpy as np


def hits(matrix, thresholds, cap, feats=None, Ts=None, t_max=None):
    """Per column c of matrix [B, n_win, n_cols]: np.argwhere(matrix[..., c] >= thresholds[c]) in its own (row-major) order is the
    column's hit list -- ascending (seq, window).  Returns a list of {"seq", "window", "score", "n_total", "windows"} holding the first
    `cap` hits, their entries of the matrix, the count without the cap and, given feats [B, n_rows, 96] and the columns' window lengths
    Ts under the call's t_max, each hit's own rows [window + t_max - T, window + t_max) of its sequence.  thresholds None = 0.5
    everywhere; a NaN threshold compares false with every score."""
    matrix = np.asarray(matrix)
    n_cols = matrix.shape[2]
    thr = np.full(n_cols, 0.5, np.float32) if thresholds is None else np.broadcast_to(np.asarray(thresholds, np.float32), (n_cols,))
    out = []
    for c in range(n_cols):
        with np.errstate(invalid="ignore"):
            at = np.argwhere(matrix[:, :, c] >= thr[c])
        keep = at[:cap]
        col = {"seq": keep[:, 0].astype(np.int32), "window": keep[:, 1].astype(np.int32), "score": matrix[keep[:, 0], keep[:, 1], c].astype(np.float32),
               "n_total": int(at.shape[0]), "windows": None}
        if feats is not None:
            T = int(Ts[c])
            idx = (keep[:, 1] + (t_max - T))[:, None] + np.arange(T)[None, :]
            col["windows"] = np.asarray(feats)[keep[:, 0][:, None], idx].astype(np.float32).reshape(keep.shape[0], T, 96)
        out.append(col)
    return out


def assert_columns_equal(got, want, label=""):
    """Bit for bit: positions, scores, totals and (where the expectation has them) windows of every column."""
    assert len(got) == len(want), f"{label}: {len(got)} columns, expected {len(want)}"
    for c, (g, w) in enumerate(zip(got, want)):
        where = f"{label} column {c}"
        assert g["n_total"] == w["n_total"], f"{where}: n_total {g['n_total']}, expected {w['n_total']}"
        assert np.array_equal(g["seq"], w["seq"]) and np.array_equal(g["window"], w["window"]), \
            f"{where}: positions {list(zip(g['seq'][:6], g['window'][:6]))}, expected {list(zip(w['seq'][:6], w['window'][:6]))}"
        assert g["score"].dtype == np.float32 and g["score"].tobytes() == w["score"].tobytes(), f"{where}: scores differ from the matrix"
        if w["windows"] is not None:
            assert g["windows"] is not None and g["windows"].shape == w["windows"].shape, f"{where}: windows shape"
            assert g["windows"].tobytes() == w["windows"].tobytes(), f"{where}: windows differ from the rows"


def thresholds_from(matrix):
    """The threshold sets of the device tier, taken FROM the matrix [B, n_win, n_cols]: per column the median score (a score that
    occurs, so `>=` is tested at equality; np.partition picks an element, no mean of two), the column's maximum (one hit at least),
    a value above the maximum (none), 0.0 (every window), and the median with column 0 set to NaN (never reports)."""
    flat = matrix.reshape(-1, matrix.shape[2])
    med = np.partition(flat, flat.shape[0] // 2, axis=0)[flat.shape[0] // 2].astype(np.float32)
    mx = flat.max(axis=0).astype(np.float32)
    nan0 = med.copy()
    nan0[0] = np.nan
    return {"median": med, "max": mx, "above": np.nextafter(mx, np.float32(np.inf)).astype(np.float32) + np.float32(1.0),
            "zero": np.zeros(matrix.shape[2], np.float32), "nan0": nan0}
