"""Shared by tests/test_dense_cpu.py and tests/test_dense_gpu.py: dense scoring (include/owwhip.h: oww_score_features / oww_score_clips).

The float64 expectation dense_ref -- O.head_stage over numpy's sliding_window_view windows with the entries' end alignment -- the
inputs and heads of the device tier, and a host stand-in for the engine so that the Python layer (utils.score_feature_file's chunk
overlap, utils.mine_windows' window cut) runs without a GPU.  HIP-free."""
import copy
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import oww_oracle as O

import head_windows as HW

B = 3
ROWS = 300                               # rows of the input array; a case reads its first n_win + T - 1
TS = (1, 3, 16, 19, 22)                  # KST = 3, 9, 48, 57, 66: odd and even, multiples of the ring depths and not
# windows per sequence.  Tiles of 128 (four waves): a partial tile, one wave and a bit, a full tile, a full tile + 1, three tiles with a
# partial last; tiles of 256 (eight waves, what every T of TS runs): partial tiles, a full tile, a full tile + 1 and + 5
N_WINS = (1, 37, 128, 129, 256, 257, 261)
SLIDE_FORMS = ("narrow1", "narrow2", "narrow3", "narrow4", "wide1", "wide2")
FALLBACK_FORMS = ("generic130", "rnn1", "fp32_2x64")
# the routing edges of the sliding kernel (owwhip_dense_host.h: t_limit): a pass of two nets runs tiles of 256 windows up to T = 72 and
# of 128 beyond, a pass of one net up to 113; 120 is the longest window a fixed head may have, so no narrow group takes the fallback
EDGES = (("narrow4", (72, 73)), ("narrow1", (113, 114, 120)))
EDGE_N_WINS = (37, 129)
HEAD_SEED = 11


@functools.lru_cache(maxsize=None)
def feats():
    """float32 [3, 300, 96]: N(0, 1); rows 40-59 of sequence 1 zero, rows 100-102 of sequence 2 at 30 x the scale (read-only)."""
    f = np.random.default_rng(9100).normal(0.0, 1.0, (B, ROWS, 96)).astype(np.float32)
    f[1, 40:60] = 0.0
    f[2, 100:103] *= 30.0
    f.setflags(write=False)
    return f


def windows_of(f, T, t_max=None):
    """[B, n_win, T, 96] (a view): window w of a head of length T on a handle whose longest window is t_max = rows
    [w + t_max - T, w + t_max) of each sequence of f [B, n_rows, 96]; n_win = n_rows - t_max + 1."""
    f = np.asarray(f)
    t_max = T if t_max is None else t_max
    assert f.ndim == 3 and 1 <= T <= t_max <= f.shape[1]
    return sliding_window_view(f[:, t_max - T:], T, axis=1).transpose(0, 1, 3, 2)


def dense_ref(f, heads, dtype=np.float64):
    """{name: [B, n_win, n_out]}: what oww_score_features returns for f [B, n_rows, 96] on a handle with `heads`, from the oracle in
    `dtype` on the materialised windows."""
    t_max = max(int(h["T"]) for h in heads.values())
    out = {}
    for n, h in heads.items():
        w = np.ascontiguousarray(windows_of(f, int(h["T"]), t_max))
        with np.errstate(over="ignore"):
            s = O.head_stage(w.reshape(-1, int(h["T"]), 96), h, np.dtype(dtype).type)
        out[n] = np.asarray(s, np.float64).reshape(w.shape[0], w.shape[1], -1)
    return out


def dense_raw(f, heads, dtype=np.float32):
    """[B, n_win, n_labels]: dense_ref's columns side by side in head order, as the entries lay them out."""
    r = dense_ref(f, heads, dtype)
    return np.concatenate([r[n] for n in heads], axis=2).astype(np.float32)


def case_rows(n_win, T):
    return n_win + T - 1


@functools.lru_cache(maxsize=None)
def _form_heads(form, T):
    w = np.ascontiguousarray(windows_of(feats(), T)).reshape(-1, T, 96)
    out = {}
    for i, shape in enumerate(HW.FORMS[form]["heads"]):
        name = f"dense_{form}_t{T}_{i}"
        out[name] = HW.centre(HW.draw_head(name, shape, T, seed=HEAD_SEED), w)
    return out


def form_heads(form, T):
    """{name: head} of one (form, T) (tests/head_windows.py: FORMS), drawn with seed 11 and centred on all windows of feats()."""
    return copy.deepcopy(_form_heads(form, T))


@functools.lru_cache(maxsize=None)
def _want(form, T, dtype):
    f = feats()[:, :min(ROWS, case_rows(max(N_WINS), T))]
    out = dense_ref(f, _form_heads(form, T), dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


def want(form, T, dtype=np.float64):
    """{name: [3, 261, n_out]} of one (form, T) over the largest case (the longer edge lengths: the windows the 300 rows hold), computed
    once; a case of n_win windows reads [:, :n_win]."""
    return _want(form, T, np.dtype(dtype).name)


# ------------------------------------------------------------------------------------------------ a host stand-in for the engine
class StubDenseEngine:
    """score_shape / score_features / score_clips of StreamEngine on the host: float64 oracle scores as float32, and as a clip's "embeddings" a
    fixed random projection of its 80 ms chunks (any deterministic map from samples to rows serves the host logic under test)."""

    def __init__(self, heads, n_streams=4):
        self.heads = heads
        self.head_names = list(heads)
        self.n_labels = sum(int(h["n_out"]) for h in heads.values())
        self.n_streams_padded = n_streams
        self.t_max = max(int(h["T"]) for h in heads.values())
        self.calls = []
        self._proj = np.random.default_rng(5).normal(0.0, 1.0, (1280, 96)).astype(np.float32) / 36.0

    def score_shape(self, n_rows):
        if n_rows < self.t_max:
            raise ValueError("fewer rows than one window")
        return n_rows - self.t_max + 1, self.t_max

    def score_features(self, f):
        f = np.asarray(f, np.float32)
        self.calls.append(f.shape)
        # float64 rounded to float32: a window's bits then do not depend on the batch it is scored in, as on the device (a float32
        # oracle takes another BLAS path per batch size and moves the last bit)
        return dense_raw(f, self.heads, np.float64)

    def embed(self, pcm):
        n_out = ((pcm.shape[1] - 512) // 160 + 1 - 76) // 8 + 1
        x = pcm[:, :n_out * 1280].reshape(pcm.shape[0], n_out, 1280).astype(np.float32) / 32768.0
        return (x @ self._proj).astype(np.float32)

    def score_clips(self, pcm, return_features=False):
        emb = self.embed(pcm)
        out = self.score_features(emb)
        return (out, emb) if return_features else out


class StubDenseModel:
    """What utils.score_feature_file / utils.mine_windows read of a BatchedModel, over a StubDenseEngine; score_clips is BatchedModel's."""

    def __init__(self, heads, n_streams=4):
        from openwakeword_amd.model import BatchedModel
        self.engine = StubDenseEngine(heads, n_streams)
        self.labels, self._keep, self._parent, col = [], [], {}, 0
        for n, h in heads.items():
            for j in range(int(h["n_out"])):
                self.labels.append(n if int(h["n_out"]) == 1 else f"{n}:{j}")
                self._keep.append(col + j)
                self._parent[col + j] = n
            col += int(h["n_out"])
        self._model_T = {n: int(h["T"]) for n, h in heads.items()}
        self.score_clips = BatchedModel.score_clips.__get__(self)
