"""Per-stream custom verifiers, host side: BatchedModel's refusals happen before the library is touched, the header declares the new
entries, and fold_verifier reproduces the reference pipeline's predict_proba for several fitted verifiers."""
import os
import re

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd.model import BatchedModel, fold_verifier

from verifier_fixture import trained_verifier

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class _Engine:
    feature_ring = 16

    def __init__(self):
        self.calls = []
        self._next = 0

    def verifier_add(self, w, b):
        self.calls.append(("add", w.size))
        self._next += 1
        return self._next - 1

    def verifier_remove(self, vid):
        self.calls.append(("remove", vid))

    def assign_verifiers(self, label, ids, v, t, bank=False):
        self.calls.append(("assign", label, bank, ids.tolist(), v.tolist(), t.tolist()))


def _bare_model(S=8, K=2, capacity=4):
    m = BatchedModel.__new__(BatchedModel)          # (no library, no GPU: the checks run before the engine is reached)
    m.n_streams, m.bank_slots, m.verifier_capacity, m.engine, m._debounce_frames = S, K, capacity, _Engine(), 0
    m._parent = {0: "alexa", 1: "timer", 2: "timer", 3: "short"}
    m._model_T = {"alexa": 16, "timer": 16, "short": 12}
    m._verifier_T = {}
    return m


def _wb(T=16, seed=0):
    return np.random.default_rng(seed).normal(0, 0.01, T * 96).astype(np.float32), 0.5


def test_assignments_reach_the_engine():
    m = _bare_model()
    v0 = m.add_verifier(_wb())
    v1 = m.add_verifier(_wb(12))
    assert (v0, v1) == (0, 1)
    m.assign_verifiers([0, 3], "alexa", [v0, -2], threshold=0.3)
    m.assign_verifiers(np.array([5]), "timer", v0)                      # multiclass: every column of the model
    m.assign_verifiers([1, 2], "short", v1, threshold=[0.2, 0.4])
    m.assign_bank_verifiers([7], 1, [v0], threshold=0.5)
    assigns = [c for c in m.engine.calls if c[0] == "assign"]
    assert [(c[1], c[2]) for c in assigns] == [(0, False), (1, False), (2, False), (3, False), (1, True)]
    assert assigns[0][3:5] == ([0, 3], [0, -2])
    assert assigns[3][5] == pytest.approx([0.2, 0.4])
    m.remove_verifier(v0)
    assert ("remove", 0) in m.engine.calls


@pytest.mark.parametrize("call,msg", [
    (lambda m, v: m.assign_verifiers([0], "no_such_model", v), "not matched"),
    (lambda m, v: m.assign_verifiers([0], "short", v), "T = 12"),
    (lambda m, v: m.assign_verifiers([0], "alexa", -3), "-1"),
    (lambda m, v: m.assign_verifiers([0], "alexa", 9), "not a verifier"),
    (lambda m, v: m.assign_verifiers([8], "alexa", v), "stream ids"),
    (lambda m, v: m.assign_verifiers([-1], "alexa", v), "stream ids"),
    (lambda m, v: m.assign_verifiers([[0]], "alexa", v), "1-D"),
    (lambda m, v: m.assign_verifiers([0.5], "alexa", v), "1-D integer"),
    (lambda m, v: m.assign_verifiers([0, 1], "alexa", [v, v, v]), "verifier_ids"),
    (lambda m, v: m.assign_verifiers([0, 1], "alexa", [0.5, 1.0]), "verifier_ids"),
    (lambda m, v: m.assign_verifiers([0, 1], "alexa", v, threshold=[0.1, 0.2, 0.3]), "threshold"),
    (lambda m, v: m.assign_verifiers([0], "alexa", v, threshold="high"), "threshold"),
    (lambda m, v: m.assign_bank_verifiers([0], 2, v), "slot"),
    (lambda m, v: m.assign_bank_verifiers([0], 0, -5), "-1"),
    (lambda m, v: m.remove_verifier(7), "not a verifier"),
    (lambda m, v: m.add_verifier((np.zeros(100, np.float32), 0.0)), "T x 96"),
    (lambda m, v: m.add_verifier((np.zeros(17 * 96, np.float32), 0.0)), "feature ring"),
    (lambda m, v: m.add_verifier(object()), "pipeline"),
])
def test_refusals_before_the_library(call, msg):
    m = _bare_model()
    v = m.add_verifier(_wb())
    m.engine.calls.clear()
    with pytest.raises(ValueError, match=msg):
        call(m, v)
    assert m.engine.calls == []


def test_no_pool_or_no_bank():
    m = _bare_model(capacity=0)
    for call in (lambda: m.add_verifier(_wb()), lambda: m.assign_verifiers([0], "alexa", 0)):
        with pytest.raises(ValueError, match="verifier_capacity"):
            call()
    m = _bare_model(K=0)
    with pytest.raises(ValueError, match="bank_slots"):
        m.assign_bank_verifiers([0], 0, -1)
    assert m.engine.calls == []


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_fold_verifier_round_trip(seed):
    """The folded (w, bias) of a fitted pipeline gives its predict_proba to 1e-6 (float64 evaluation of the float32 weights)."""
    pipe = trained_verifier(seed)
    w, b = fold_verifier(pipe)
    assert w.dtype == np.float32 and w.shape == (16 * 96,)
    X = np.random.default_rng(100 + seed).normal(0, 4.0, (9, 16, 96)).astype(np.float32)
    want = pipe.predict_proba(X)[:, -1]
    got = 1.0 / (1.0 + np.exp(-(X.reshape(9, -1).astype(np.float64) @ w.astype(np.float64) + b)))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def test_header_declares_the_verifier_entries():
    src = open(os.path.join(ROOT, "include", "owwhip.h")).read()
    assert re.search(r"#define OWW_VERIFIER_DEFAULT\s+-1\b", src)
    assert re.search(r"#define OWW_VERIFIER_NONE\s+-2\b", src)
    assert re.search(r"#define OWW_ABI_VERSION 6\b", src)
    for name in ("oww_verifier_configure", "oww_verifier_add", "oww_verifier_remove", "oww_assign_verifiers",
                 "oww_bank_assign_verifiers", "oww_verifier_stats"):
        assert re.search(r"\bint\s+" + name + r"\(", src), name
        assert name in _lib.SYMBOLS, name
