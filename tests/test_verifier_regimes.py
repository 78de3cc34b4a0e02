"""verifier_kernel and stream_verifier_kernel against float64 across window lengths, ring positions and weight regimes
(tests/verifier_budget.py has the restatement, the budget and the regimes; tests/test_verifier_budget_cpu.py derives every number spent
here on the CPU; DESIGN.md 5.24 has the figures).

Yardstick: the same handle, reset, with no verifier gives raw0[t] (oww_get_raw) and the ring rows of every stream after every call --
runs are bit-reproducible.  With verifiers, wherever raw0 >= threshold the score must lie within the relative budget of
ref64(window, w, b), the window being the last T rows get_features() returns after the call (the rows the verifier saw); everywhere else
the raw output must equal raw0 bit for bit; the per-stream kernel's evaluation counter must equal the host's count of raw0 >= threshold
on every call.  Regimes are calibrated on the twin run's windows.  pytest -m gpu -s prints each test's worst fraction of its budget."""
import functools

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine, _ptr

import verifier_budget as VB

pytestmark = pytest.mark.gpu

S = 5                            # S % 4 != 0: idle waves in verifier_kernel's last workgroup
DEFAULT, NONE = VB.DEFAULT, VB.NONE
NREG = len(VB.REGIMES)


# ------------------------------------------------------------------------------------------------ handles
def _heads(key):
    if key in ("H34", "H34f1"):      # T = TR for the multiclass head, T < TR for the others; labels 0, 1, 2 and 3..5
        return {"t1": W.synthetic_head("t1", 1234, T=1), "t5": W.synthetic_head("t5", 1234, T=5), "t16": W.synthetic_head("t16", 1234),
                "m34": W.synthetic_head("timer", 1234, T=34, n_out=3)}
    if key == "H120":
        return {"t16": W.synthetic_head("t16", 1234), "t120": W.synthetic_head("t120", 1234, T=120)}
    if key == "HL":                  # column 2 is the bank head as a fixed head: the slot's raw0 (bit-identical, tests/test_head_bank_gpu.py)
        return {"a16": W.synthetic_head("a16", 1234), "b5": W.synthetic_head("b5", 1234, T=5), "x34": W.synthetic_head("x34", 1234, T=34)}
    raise KeyError(key)


def _get_raw(eng):
    raw = np.empty((eng.n_streams, eng.n_labels), np.float32)
    _lib.check(eng._lib.oww_get_raw(eng._h, _ptr(raw)))
    return raw


class Handle:
    def __init__(self, key):
        self.key = key
        self.heads = _heads(key)
        self.S = VB.HL_S if key == "HL" else S
        self.TR = 120 if key == "H120" else 34
        kw = dict(bank_slots=1, bank_capacity=2) if key == "HL" else {}
        self.eng = StreamEngine(self.S, self.heads, W.synthetic_embedding(1234), max_chunks=3, feature_ring=self.TR,
                                use_mfma=1 if key == "H34f1" else 3, verifier_capacity=32, **kw)
        assert self.eng.feature_ring == self.TR
        self.label_T = [int(h["T"]) for h in self.heads.values() for _ in range(int(h["n_out"]))]
        self.NL = len(self.label_T)
        self.K = 1 if key == "HL" else 0
        if self.K:
            self.eng.subscribe(np.arange(self.S), np.full((self.S, 1), self.eng.bank_add(self.heads["x34"])))
        self.init = np.random.default_rng(78).normal(1.5, 0.5, (self.TR, 96)).astype(np.float32)
        self.ops = _schedule(self.S, 12 if key == "HL" else self.TR + 6)
        self.pcm = VB.case_pcm(self.S, sum(op[1] if op[0] == "chunks" else 1 for op in self.ops))
        self.pool = {}                                   # (regime, T) -> pool id
        self.twin = None
        self.twin = self._record()

    # ---- configuration
    def clear(self):
        ids = np.arange(self.S)
        for l in range(self.NL):
            self.eng.set_verifier(l, None)
            self.eng.assign_verifiers(l, ids, np.full(self.S, DEFAULT), np.zeros(self.S))
        for k in range(self.K):
            self.eng.assign_verifiers(k, ids, np.full(self.S, DEFAULT), np.zeros(self.S), bank=True)
        assert self.eng.verifier_stats()[0] == 0
        self.eng.reset(None, self.init)

    def pool_id(self, regime, T):
        if (regime, T) not in self.pool:
            self.pool[regime, T] = self.eng.verifier_add(*self.verifier(regime, T))
        return self.pool[regime, T]

    @functools.lru_cache(maxsize=None)
    def verifier(self, regime, T):
        """(w, b) of a regime at T, calibrated on the twin run's windows of the streams that took part in each call."""
        rings = np.concatenate([r[on] for (_, r, _, on) in self.twin])
        w, b = VB.folded(VB.triple(regime, T, VB.windows(rings, T)))
        return w, float(np.float32(b))

    # ---- running
    def calls(self, n=None):
        """(t, raw [S, NL], rings [S, TR, 96], bank scores or None, stream_on [S]) after every call of the schedule."""
        f = 0
        for t, (kind, arg) in enumerate(self.ops[:n]):
            if kind == "mask":
                on = np.asarray(arg, bool)
                self.eng.step_masked(self.pcm[:, f * 1280:(f + 1) * 1280], on)
                raw = _get_raw(self.eng)
                f += 1
            else:
                on = np.ones(self.S, bool)
                raw = self.eng.step_raw(self.pcm[:, f * 1280:(f + arg) * 1280])
                f += arg
            rings = np.stack([self.eng.get_features(s, self.TR) for s in range(self.S)])
            yield t, raw, rings, (self.eng.bank_scores() if self.K else None), on

    def _record(self):
        self.clear()
        return [(raw, rings, bank, on) for _, raw, rings, bank, on in self.calls()]

    def close(self):
        self.eng.close()


def _schedule(n_streams, n_calls):
    """One-chunk calls with one 3-chunk call and two masked steps with different streams off (so that streams hold different nfeat);
    n_calls = TR + 6 lets nfeat % TR take every residue."""
    ops = [("chunks", 1)] * n_calls
    ops[7] = ("chunks", 3)
    ops[9] = ("mask", np.arange(n_streams) % 2 == 0)
    ops[10] = ("mask", ~np.isin(np.arange(n_streams), VB.MASK_OFF) if n_streams == VB.HL_S else np.arange(n_streams) % 3 != 0)
    return ops


_HANDLES = {}


def _handle(key):
    if key not in _HANDLES:
        _HANDLES[key] = Handle(key)
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


# ------------------------------------------------------------------------------------------------ the check of one run
class Plan:
    """Who verifies what: fix[(s, l)] / bank[(s, k)] = (regime, T, w, b, thr)."""

    def __init__(self):
        self.fix, self.bank = {}, {}


def _run(h, plan, stream_kernel, n=None, before=None, worst=None):
    """Run the schedule on the configured handle; returns (scores {(t, s, l): float32}, hits {(t, s, l)}, evaluations per call).  before(t)
    may reconfigure the handle and edit the plan in front of call t."""
    worst = {} if worst is None else worst
    scores, hits, evals = {}, set(), []
    gen = h.calls(n)
    t = 0
    while True:
        if before is not None:
            before(t)
        try:
            t_, raw, rings, bank, on = next(gen)
        except StopIteration:
            break
        raw0, rings0, bank0, on0 = h.twin[t]
        assert np.array_equal(on, on0)
        assert np.array_equal(rings[on], rings0[on]), f"call {t}: the verified run's feature rows left the twin's"
        n_hit = 0
        expect = raw0.copy()
        for (s, l), (regime, T, w, b, thr) in plan.fix.items():
            if not on[s] or not raw0[s, l] >= np.float32(thr):
                continue
            n_hit += 1
            hits.add((t, s, l))
            expect[s, l] = np.nan
            _, want, kappa = VB.ref64(rings[s, h.TR - T:].reshape(-1), w, b)
            frac = abs(float(raw[s, l]) - float(want)) / float(VB.budget(T, kappa))
            worst[regime, T] = max(worst.get((regime, T), 0.0), frac)
            assert frac <= 1.0, f"call {t} stream {s} label {l} {regime} T={T}: |score - float64| = {abs(float(raw[s, l]) - float(want)):.3e}, " \
                                f"{frac:.2f} budgets (kappa {float(kappa):.1f})"
            scores[t, s, l] = raw[s, l]
        same = on[:, None] & ~np.isnan(expect)
        assert np.array_equal(raw[same], raw0[same]), f"call {t}: an output no verifier re-scored left raw0 at {np.argwhere(same & (raw != raw0)).tolist()}"
        for (s, k), (regime, T, w, b, thr) in plan.bank.items():
            hit = bool(on[s]) and bool(raw0[s, 2] >= np.float32(thr))      # the slot's head is fixed column 2 of the twin
            n_hit += hit
            if not on[s] or t < 6:                       # bank_scores() are post-processed: zero during the first five frames
                continue
            if hit:
                _, want, kappa = VB.ref64(rings[s, h.TR - T:].reshape(-1), w, b)
                frac = abs(float(bank[s, k]) - float(want)) / float(VB.budget(T, kappa))
                worst[regime, T] = max(worst.get((regime, T), 0.0), frac)
                assert frac <= 1.0, f"call {t} stream {s} slot {k} {regime} T={T}: {frac:.2f} budgets"
            else:
                assert bank[s, k] == bank0[s, k], f"call {t} stream {s} slot {k}"
        if stream_kernel:
            assert h.eng.verifier_stats()[1] == n_hit, f"call {t}: {h.eng.verifier_stats()[1]} evaluations, the host counts {n_hit}"
        evals.append(n_hit)
        t += 1
    assert not h.eng.range_status()
    return scores, hits, evals


def _report(tag, worst):
    if not worst:
        print(f"\n{tag}: nothing re-scored")
        return
    by_regime = {}
    for (regime, T), v in worst.items():
        by_regime[regime] = max(by_regime.get(regime, 0.0), v)
    print(f"\n{tag}: worst fraction of the budget {max(worst.values()):.3f}; by regime " +
          ", ".join(f"{r} {by_regime[r]:.3f}" for r in VB.REGIMES if r in by_regime) + "; by T " +
          ", ".join(f"{T}: {max(v for (_, t), v in worst.items() if t == T):.3f}" for T in sorted({t for _, t in worst})))


# ------------------------------------------------------------------------------------------------ 1. regimes x T on verifier_kernel
@functools.lru_cache(maxsize=None)
def _wide_pass(key, p):
    """Pass p of a handle: label l carries regime (l + p) % 6 handle-wide at threshold 0 -> (scores, worst)."""
    h = _handle(key)
    h.clear()
    plan = Plan()
    for l, T in enumerate(h.label_T):
        regime = VB.REGIMES[(l + p) % NREG]
        w, b = h.verifier(regime, T)
        h.eng.set_verifier(l, w, b, 0.0)
        for s in range(h.S):
            plan.fix[s, l] = (regime, T, w, b, 0.0)
    worst = {}
    scores, hits, evals = _run(h, plan, False, worst=worst)
    assert evals == [int(on.sum()) * h.NL for (_, _, _, on) in h.twin]          # threshold 0: every pair, the first five frames included
    return scores, worst


@pytest.mark.parametrize("p", range(NREG))
@pytest.mark.parametrize("key", ["H34", "H120"])
def test_regimes_on_the_handle_wide_kernel(key, p):
    """Every regime on every label (T = 1, 5, 16, 34 x 3 on the 34-row ring; 16 and 120 on the 120-row ring) over TR + 6 calls: the window
    wraps at every ring position; a 3-chunk call and two masked steps leave the streams at different positions."""
    _, worst = _wide_pass(key, p)
    _report(f"verifier_kernel {key} pass {p}", worst)


def test_regimes_on_the_exact_fp32_family():
    """Pass 0 of H34 behind the heads of family 1: the verifier does not care which family wrote raw."""
    _, worst = _wide_pass("H34f1", 0)
    _report("verifier_kernel H34 family 1 pass 0", worst)


# ------------------------------------------------------------------------------------------------ 2. the same on stream_verifier_kernel
@pytest.mark.parametrize("p", [0, 3])
@pytest.mark.parametrize("key", ["H34", "H120"])
def test_regimes_on_the_per_stream_kernel(key, p):
    """Stream s carries the pool verifier of regime (s + l + p) % 6 on label l: the same budget, and bit for bit the handle-wide
    kernel's score of the same (regime, label, stream, call)."""
    h = _handle(key)
    h.clear()
    plan = Plan()
    ids = np.arange(h.S)
    for l, T in enumerate(h.label_T):
        regs = [VB.REGIMES[(s + l + p) % NREG] for s in range(h.S)]
        h.eng.assign_verifiers(l, ids, [h.pool_id(r, T) for r in regs], np.zeros(h.S))
        for s, r in enumerate(regs):
            plan.fix[s, l] = (r, T) + h.verifier(r, T) + (0.0,)
    assert h.eng.verifier_stats()[0] == h.S * h.NL
    worst = {}
    scores, _, _ = _run(h, plan, True, worst=worst)
    _report(f"stream_verifier_kernel {key} pass {p}", worst)
    n_same = 0
    for (t, s, l), v in scores.items():
        q = (VB.REGIMES.index(plan.fix[s, l][0]) - l) % NREG                    # the handle-wide pass that had this regime on label l
        assert v == _wide_pass(key, q)[0][t, s, l], f"call {t} stream {s} label {l}: the two kernels differ"
        n_same += 1
    assert n_same == len(scores) > 0


# ------------------------------------------------------------------------------------------------ 3. mixed T in one launch
def _mid(h, l, lo=8):
    """A threshold that occurred: the median of label l's raw0 over the calls from `lo` on."""
    v = np.sort(np.concatenate([raw0[on, l] for (raw0, _, _, on) in h.twin[lo:]]))
    return float(v[v.size // 2])


def test_mixed_labels_removed_and_replaced_verifiers():
    """The multiclass head's three labels carry different verifiers and thresholds, one of them none, next to labels of T = 1, 5 and
    16; a label whose verifier is removed scores raw0 again, and set again with another regime reads the new weights only."""
    h = _handle("H34")
    h.clear()
    plan = Plan()

    def put(l, regime, thr):
        w, b = h.verifier(regime, h.label_T[l])
        h.eng.set_verifier(l, w, b, thr)
        for s in range(h.S):
            plan.fix[s, l] = (regime, h.label_T[l], w, b, thr)

    def drop(l):
        h.eng.set_verifier(l, None)
        for s in range(h.S):
            del plan.fix[s, l]

    put(0, "offset", 0.0)
    put(1, "lowvar", _mid(h, 1))
    put(2, "unit", 0.0)
    put(3, "unit", 0.0)
    put(4, "alternating", _mid(h, 4))                  # label 5: no verifier
    thr4 = plan.fix[0, 4][4]

    def before(t):
        if t == 14:
            drop(3)
        if t == 20:
            put(3, "sparse_rows", 0.0)
            put(1, "alternating", 0.0)                   # replaced without a removal in between
    worst = {}
    scores, hits, evals = _run(h, plan, False, worst=worst, before=before)
    _report("verifier_kernel H34 mixed labels", worst)
    assert not any(l == 5 for (_, _, l) in hits)
    assert not any(l == 3 and 14 <= t < 20 for (t, _, l) in hits) and any(l == 3 and t >= 20 for (t, _, l) in hits)
    n4 = sum(l == 4 for (_, _, l) in hits)
    want4 = sum(int(np.sum(raw0[on, 4] >= np.float32(thr4))) for (raw0, _, _, on) in h.twin)
    assert n4 == want4 and 0 < n4 < sum(int(on.sum()) for (_, _, _, on) in h.twin)


def test_pool_slot_refilled_with_a_shorter_verifier():
    """A pool slot freed by oww_verifier_remove and refilled with a verifier of smaller T serves the new verifier only; the pairs of the
    removed one fall back to the default (none)."""
    h = _handle("H34")
    h.clear()
    plan = Plan()
    ids = np.arange(h.S)
    w34 = (h.verifier("unit", 34)[0] * np.float32(1.5)).astype(np.float32)       # (not one of the cached pool entries)
    b34 = h.verifier("unit", 34)[1]
    vid = h.eng.verifier_add(w34, b34)
    h.eng.assign_verifiers(3, ids, np.full(h.S, vid), np.zeros(h.S))
    keep = h.pool_id("offset", 16)
    h.eng.assign_verifiers(2, ids[:2], np.full(2, keep), np.zeros(2))           # keeps the per-stream kernel on after the removal
    for s in range(h.S):
        plan.fix[s, 3] = ("unit", 34, w34, b34, 0.0)
    for s in range(2):
        plan.fix[s, 2] = ("offset", 16) + h.verifier("offset", 16) + (0.0,)
    state = {}

    def before(t):
        if t == 12:
            h.eng.verifier_remove(vid)
            for s in range(h.S):
                del plan.fix[s, 3]
        if t == 16:
            w5, b5 = h.verifier("alternating", 5)
            state["vid"] = h.eng.verifier_add(w5, b5)
            h.eng.assign_verifiers(1, ids, np.full(h.S, state["vid"]), np.zeros(h.S))
            for s in range(h.S):
                plan.fix[s, 1] = ("alternating", 5, w5, b5, 0.0)
    worst = {}
    try:
        _, hits, _ = _run(h, plan, True, n=24, worst=worst, before=before)
        assert state["vid"] == vid, "the freed slot was not the one refilled"
        assert any(l == 1 and t >= 16 for (t, _, l) in hits) and not any(l == 3 and t >= 12 for (t, _, l) in hits)
    finally:
        h.clear()
        if "vid" in state:
            h.eng.verifier_remove(state["vid"])
    _report("stream_verifier_kernel H34 refilled slot", worst)


# ------------------------------------------------------------------------------------------------ 4. threshold edges
@pytest.mark.parametrize("stream_kernel", [False, True])
def test_threshold_edges(stream_kernel):
    """thr equal to a raw0 that occurred at a known (call, stream): that pair is re-scored at that call; at the next float above it is
    not and stays bit-equal to raw0; thr = 0 re-scores every pair from the first frame on; thr = 1.5 none."""
    h = _handle("H34")
    t0, s0, n = 15, 2, 20
    at = h.twin[t0][0][s0]                                # raw0 of every label at (t0, s0)
    for name, thrs in (("equal", at), ("next", np.nextafter(at, np.float32(2.0))), ("zero", np.zeros(h.NL, np.float32)),
                       ("never", np.full(h.NL, 1.5, np.float32))):
        h.clear()
        plan = Plan()
        for l, T in enumerate(h.label_T):
            regime = VB.REGIMES[1 + l % (NREG - 1)]
            w, b = h.verifier(regime, T)
            if stream_kernel:
                h.eng.assign_verifiers(l, np.arange(h.S), np.full(h.S, h.pool_id(regime, T)), np.full(h.S, thrs[l]))
            else:
                h.eng.set_verifier(l, w, b, float(thrs[l]))
            for s in range(h.S):
                plan.fix[s, l] = (regime, T, w, b, float(thrs[l]))
        worst = {}
        _, hits, evals = _run(h, plan, stream_kernel, n=n, worst=worst)
        pairs = [int(on.sum()) * h.NL for (_, _, _, on) in h.twin[:n]]
        host = [int(np.sum(raw0[on] >= thrs[None, :])) for (raw0, _, _, on) in h.twin[:n]]
        assert evals == host                              # (and, per-stream kernel, equal to verifier_stats() on every call: _run)
        if name == "equal":
            assert all((t0, s0, l) in hits for l in range(h.NL))
        elif name == "next":
            assert not any((t0, s0, l) in hits for l in range(h.NL))
            assert sum(evals) > 0
        elif name == "zero":
            assert evals == pairs and evals[0] > 0
        else:
            assert sum(evals) == 0 and not hits
        print(f"{'stream_verifier_kernel' if stream_kernel else 'verifier_kernel'} thr {name}: {sum(evals)} of {sum(pairs)} pairs re-scored" +
              (f", worst fraction of the budget {max(worst.values()):.3f}" if worst else ""))


# ------------------------------------------------------------------------------------------------ 5. list shapes
HL_REGIMES = {0: "unit", 1: "offset", 2: "alternating"}         # pool verifier of column 0 (T = 16), column 1 (T = 5), the slot (T = 34)


def _apply(h, lay):
    """Put a VB.Layout on handle HL -> the plan of its entries."""
    ids = np.arange(h.S)
    pool = {v: h.pool_id(HL_REGIMES[v], T) for v, T in VB.HL_POOL.items()}
    plan = Plan()
    hw = {}
    for c in range(3):
        if lay.ver_T[c]:
            hw[c] = h.verifier("sparse_rows", lay.ver_T[c])
            h.eng.set_verifier(c, hw[c][0], hw[c][1], float(lay.ver_thr[c]))
    for c in range(3):
        h.eng.assign_verifiers(c, ids, [pool[v] if v >= 0 else v for v in lay.fix[:, c]], lay.fix_thr[:, c])
    h.eng.assign_verifiers(0, ids, [pool[v] if v >= 0 else v for v in lay.bank[:, 0]], lay.bank_thr[:, 0], bank=True)
    for e in lay.entries():
        if e.v >= 0:
            item = (HL_REGIMES[e.v], e.T) + h.verifier(HL_REGIMES[e.v], e.T) + (e.thr,)
        else:
            item = ("sparse_rows", e.T) + hw[~e.v] + (e.thr,)
        if e.col >= 0:
            plan.fix[e.s, e.col] = item
        else:
            plan.bank[e.s, ~e.col] = item
    return plan


def _hl_mid(h):
    return tuple(_mid(h, c, lo=6) for c in (0, 1, 2))


@pytest.mark.parametrize("n", VB.ENTRY_COUNTS)
def test_list_of_n_entries(n):
    """1, 15, 16, 17, 63, 64 and 65 entries: a lone lane, a wave one short, full, one over; a workgroup one short, full, one over."""
    h = _handle("HL")
    h.clear()
    lay = VB.count_layout(n, _hl_mid(h))
    assert len(lay.entries()) == n
    plan = _apply(h, lay)
    assert len(plan.fix) + len(plan.bank) == n == h.eng.verifier_stats()[0]
    worst = {}
    _, hits, evals = _run(h, plan, True, worst=worst)
    assert sum(evals) > 0 and (n < 3 or sum(evals) < n * len(evals))
    _report(f"stream_verifier_kernel HL {n} entries ({sum(evals)} evaluations)", worst)


def test_mixed_wave_all_hit_wave_and_no_hit_wave():
    """One workgroup: a wave whose 16 entries all hit (the ballot loop runs 16 times), a wave where none hits, a wave that mixes pool
    entries on a fixed column, handle-wide defaults, slot entries and three window lengths, a wave of 15 defaults; one masked step
    switches off some entries of the mixed wave."""
    h = _handle("HL")
    h.clear()
    lay = VB.mixed_layout(_hl_mid(h)[1])
    ents = lay.entries()
    wave = lambda k: [e for i, e in enumerate(ents) if VB.wave_of(i) == k]
    assert len(ents) == 63 and all(e.thr == 0.0 for e in wave(VB.ALL_HIT_WAVE)) and all(e.thr == 1.5 for e in wave(VB.NO_HIT_WAVE))
    mixed = wave(VB.MIXED_WAVE)
    assert {e.T for e in mixed} == {16, 5, 34} and any(e.col < 0 for e in mixed) and any(e.v < 0 for e in mixed) and \
        any(e.col >= 0 and e.v >= 0 for e in mixed) and 0 < sum(e.s in VB.MASK_OFF for e in mixed) < 16
    plan = _apply(h, lay)
    worst = {}
    _, hits, evals = _run(h, plan, True, worst=worst)
    all_hit = {(e.s, e.col) for e in wave(VB.ALL_HIT_WAVE) if e.col >= 0}
    no_hit = {(e.s, e.col) for e in wave(VB.NO_HIT_WAVE) if e.col >= 0}
    for t, (_, _, _, on) in enumerate(h.twin):
        assert all((t, s, c) in hits for (s, c) in all_hit if on[s])
        assert not any((t, s, c) in hits for (s, c) in no_hit)
    _report(f"stream_verifier_kernel HL mixed list ({sum(evals)} evaluations)", worst)


# ------------------------------------------------------------------------------------------------ refusals
def test_set_verifier_refuses_non_finite_arguments():
    """oww_set_verifier refuses what oww_verifier_add refuses, in its words, and leaves the label as it was."""
    h = _handle("H34")
    h.clear()
    w, b = h.verifier("unit", 16)
    for bad, value, msg in ((3, np.nan, "weight 3 is not finite"), (1535, np.inf, "weight 1535 is not finite"), (0, -np.inf, "weight 0 is not finite")):
        x = w.copy()
        x[bad] = value
        with pytest.raises(_lib.OwwError, match=f"oww_set_verifier: {msg}"):
            h.eng.set_verifier(2, x, b, 0.0)
    for value in (np.nan, np.inf):
        with pytest.raises(_lib.OwwError, match="oww_set_verifier: the bias is not finite"):
            h.eng.set_verifier(2, w, value, 0.0)
    with pytest.raises(_lib.OwwError, match="oww_verifier_add: weight 3 is not finite"):
        x = w.copy()
        x[3] = np.nan
        h.eng.verifier_add(x, b)
    _run(h, Plan(), False, n=3)                          # nothing was set: raw0 bit for bit
