"""Shared by tests/test_dense_bank_cpu.py and tests/test_dense_bank_gpu.py: dense scoring over the head bank (include/owwhip.h:
oww_bank_score_shape / oww_bank_score_features / oww_bank_score_stats).

The bank heads of the device tier -- five narrow ones (64 hidden units: the sliding kernel) and two wide ones (128: the fallback) of
mixed window lengths, each centred on the windows it meets when all seven are listed (t_max = 22) -- their float64 expectation through
tests/dense_ref.py, numpy's statistics of a score matrix, and a host stand-in for a model with a bank so that utils.validate_bank's
chunk combination runs without a GPU.  HIP-free."""
import copy
import functools

import numpy as np

import dense_ref as D
import head_windows as HW

NARROW_TS = (1, 3, 16, 19, 22)           # bank_ht4: KST = 3, 9, 48, 57, 66 (dense_ref.TS)
WIDE_TS = (5, 16)                        # bank_ht8
T_MAX = 22
N_WINS = D.N_WINS                        # 1, 37, 128, 129, 256, 257, 261: the tile edges of both tile sizes
EDGE_TS = (113, 114, 120)                # tiles of 256 windows up to t_s = 113, of 128 beyond; 120 = the longest window
EDGE_N_WINS = D.EDGE_N_WINS              # 37, 129
HPWS = (1, 2, 3, 5)                      # OWW_DENSE_BANK_HPW: slices of 1, 2, 3 and all five narrow heads (and the plan's own)


def name_of(form, T):
    return f"{'n' if form == 'bank_ht4' else 'w'}{T}"


@functools.lru_cache(maxsize=None)
def _heads():
    out = {}
    for form, Ts in (("bank_ht4", NARROW_TS), ("bank_ht8", WIDE_TS)):
        for T in Ts:
            ft = np.ascontiguousarray(D.windows_of(D.feats(), T, T_MAX)).reshape(-1, T, 96)
            out[name_of(form, T)] = HW.bank_head(form, T, ft)
    return out


def heads():
    """{name: head}: n1, n3, n16, n19, n22 (narrow) and w5, w16 (wide), centred on their windows of dense_ref.feats() at t_max = 22."""
    return copy.deepcopy(_heads())


NARROW = tuple(name_of("bank_ht4", T) for T in NARROW_TS)
WIDE = tuple(name_of("bank_ht8", T) for T in WIDE_TS)
ADD_ORDER = ("n19", "w16", "n1", "n22", "w5", "n3", "n16")       # a shuffled order; one head is added and removed after the third


@functools.lru_cache(maxsize=None)
def edge_head(T):
    """A narrow bank head of window length T (113, 114, 120), alone in its call: centred on its own windows of dense_ref.feats()."""
    ft = np.ascontiguousarray(D.windows_of(D.feats(), T)).reshape(-1, T, 96)
    return HW.bank_head("bank_ht4", T, ft)


@functools.lru_cache(maxsize=None)
def _want(dtype):
    f = D.feats()[:, :D.case_rows(max(N_WINS), T_MAX)]
    out = D.dense_ref(f, _heads(), dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


def want(dtype=np.float64):
    """{name: [3, 261, 1]} from the oracle in `dtype` over the largest case (computed once, read-only); a case reads [:, :n_win]."""
    return _want(np.dtype(dtype).name)


def np_stats(matrix, thresholds=None):
    """numpy's count / max / first argmax over the windows of a score matrix [B, n_win, n]: what oww_bank_score_stats must equal."""
    m = np.asarray(matrix, np.float32)
    thr = np.full(m.shape[2], 0.5, np.float32) if thresholds is None else np.asarray(thresholds, np.float32)
    return {"count": (m >= thr[None, None, :]).sum(axis=1).astype(np.int32), "max": m.max(axis=1), "argmax": m.argmax(axis=1).astype(np.int32)}


class StubBankModel:
    """bank_score_shape / bank_score_features / bank_score_stats of a BatchedModel on the host: float64 oracle scores rounded to float32
    (so that a window's bits do not depend on the chunk it is scored in, as on the device), statistics by numpy.  ids index `names`."""

    def __init__(self, heads_by_name):
        self.names = list(heads_by_name)
        self.heads = heads_by_name
        self.calls = []

    def _sel(self, ids):
        return {f"{k}:{self.names[i]}": self.heads[self.names[i]] for k, i in enumerate(ids)}

    def bank_score_shape(self, ids, n_rows):
        t_max = max(int(self.heads[self.names[i]]["T"]) for i in ids)
        if n_rows < t_max:
            raise ValueError("fewer rows than one window")
        return n_rows - t_max + 1, t_max

    def bank_score_features(self, feats, ids):
        f = np.asarray(feats, np.float32)
        return D.dense_raw(f[None] if f.ndim == 2 else f, self._sel(ids), np.float64)

    def bank_score_stats(self, feats, ids, thresholds=None):
        self.calls.append(np.asarray(feats).shape)
        return np_stats(self.bank_score_features(feats, ids), thresholds)
