"""The post-processing rules without a device (tests/postproc_ref.py): the literal restatement equals the oracle's Model.predict (which
tests/test_oracle_golden.py pins to vectors the reference produced), the device-form mirror equals the literal restatement bit for bit on
the schedule the GPU tests run, and every fault of the catalogue moves at least one final score there -- on scripted score tables that
hold exact 0.0 and 1.0, values equal to the thresholds and values one float32 step either side of them."""
import numpy as np
import pytest

import postproc_ref as P
from oracle import oww_oracle as O
from openwakeword_amd import weights as W

F32 = np.float32
NAMES = ["alexa", "hey_mycroft", "hey_rhasspy"]


class _Vad:
    """A `session` for OracleVad whose score is the scripted one of the current frame (both 640-sample sub-frames)."""

    def __init__(self):
        self.value = F32(0.0)

    def run(self, _, feed):
        return [np.array([[self.value]], F32), feed["h"], feed["c"]]


def _oracle(table, call, gate):
    """OracleModel with every stage scripted: heads read table[call[0]], the front end is zeros."""
    heads = {n: W.synthetic_head(n) for n in NAMES}
    fns = {n: (lambda x, _i=i: [np.array([[table[call[0], 0, _i]]], F32)]) for i, n in enumerate(NAMES)}
    vad = _Vad()
    mdl = O.OracleModel(heads, None, head_fns=fns, vad_threshold=float(gate), vad_session=vad,
                        mel_fn=lambda x: np.zeros((1, 1, O.n_mel_frames(x.shape[1]), 32), F32),
                        embed_fn=lambda x: np.zeros((x.shape[0], 96), F32), init_noise=np.zeros(16000, np.int16))
    return mdl, vad


@pytest.mark.parametrize("mode", ["patience", "debounce", "neither"])
def test_reference_rules_equal_the_oracle_predict(mode):
    C, gate = 48, P.VAD_THR if mode != "neither" else F32(0.0)
    raw, _ = P.scripted_tables(1, 3, 0, C, seed=11)
    thr = np.array([P.ulp(0.5, 0), P.ulp(0.35, 1), P.ulp(0.65, -1)], F32)
    sched = P.Schedule(1, 3, 0, 0)
    vad = P.vad_script(1, P.N_CALLS)[:C]
    sched.ops.append(("gate", gate))
    if mode == "patience":
        sched.ops.append(("post", [2, 0, 3], thr, 0))
        kw = dict(patience={"alexa": 2, "hey_rhasspy": 3}, threshold={n: float(t) for n, t in zip(NAMES, thr)})
    elif mode == "debounce":
        thr[1] = np.nan
        sched.ops.append(("post", [0, 0, 0], thr, 4))
        kw = dict(debounce_time=3.5 * 0.08, threshold={"alexa": float(thr[0]), "hey_rhasspy": float(thr[2])})     # ceil(3.5) = 4 frames
    else:
        kw = {}
    two = (7, 30) if mode != "debounce" else ()          # (the reference derives the debounce frames from the call's length)
    for c in range(C):
        if c == 20:
            sched.ops.append(("reset", np.array([0])))
        sched.ops += [("vad", vad[c]), ("call", 2 if c in two else 1, None)]
    want = P.reference_rules(sched, raw)["scores"]
    call = [0]
    mdl, v = _oracle(raw, call, gate)
    got = np.zeros_like(want)
    for c in range(C):
        if c == 20:
            mdl.reset()
        call[0], v.value = c, vad[c, 0]
        out = mdl.predict(np.zeros(1280 * (2 if c in two else 1), np.int16), **kw)
        got[c, 0] = [out[n] for n in NAMES]
    assert np.array_equal(P.bits(got), P.bits(want))
    assert (want != 0).sum() > 10 and ((want == 0) & (raw != 0))[6:].sum() > 5          # the rules let through, and refused


def _full(S, pick):
    return P.make_schedule(S, 12, pick, K=3, H=2)


def _tables(S, NL, H):
    return P.scripted_tables(S, NL, H, seed=3 + S)


@pytest.fixture(scope="module")
def full():
    raw, head_raw = _tables(37, 12, 2)
    sched = _full(37, P.picker(raw, head_raw))
    return sched, raw, head_raw, P.reference_rules(sched, raw, head_raw)


def test_schedule_covers_what_it_claims(full):
    sched = full[0]
    assert sched.n_calls >= 65 and set(sched.applicable()) == set(P.FAULTS)
    pats = {p for op in sched.ops if op[0] == "post" for p in op[1]}
    assert pats >= set(P.PATS)
    assert {op[3] for op in sched.ops if op[0] == "post"} >= {1, 4, 29, 30, 31, 40}
    thr = np.concatenate([op[2] for op in sched.ops if op[0] == "post"])
    assert np.isnan(thr).any() and (thr == 0).any() and (thr < 0).any()
    assert sum(op[0] == "reset" for op in sched.ops) == 2 and sum(op[0] == "reset_vad" for op in sched.ops) == 2
    assert [op[1] > 0 for op in sched.ops if op[0] == "gate"] == [True, False, True]
    # the VAD script: every position of the three-entry window decides the gate alone at least once, at values thr and thr + ulp
    v = P.vad_script(37)
    alone = np.zeros(3, int)
    for s in range(37):
        for c in range(6, P.N_CALLS):
            hot = v[c - 6:c - 3, s] >= P.VAD_THR              # entries L-7 .. L-5 of the L = c + 1 pushed before call c
            if hot.sum() == 1:
                alone[np.argmax(hot)] += 1
    assert (alone > 0).all()
    assert set(np.unique(v)) == {F32(0.0), P.ulp(0.5, -1), F32(0.5), P.ulp(0.5, 1), F32(1.0)}


def test_tables_hold_the_edges(full):
    sched, raw, head_raw, _ = full
    assert (raw == 0).any() and (raw == 1).any()
    cells = set(np.unique(raw))
    picked = {F32(t) for op in sched.ops if op[0] == "post" for t in op[2] if t > 0}
    for t in picked:                                         # a picked threshold is a cell of the table or one step from one
        assert {P.ulp(t, -1), t, P.ulp(t, 1)} & cells
    assert any(t in cells and P.ulp(t, 1) in cells and P.ulp(t, -1) in cells for t in picked)
    for op in sched.ops:
        if op[0] == "post":                                  # equality with a label's own threshold really occurs
            assert any(t > 0 and (raw[:, :, l] == t).any() for l, t in enumerate(op[2]))


@pytest.mark.parametrize("S", [37, 1])
@pytest.mark.parametrize("path", ["full"] + list(P.PATHS))
def test_device_form_equals_reference_rules(path, S):
    kw = dict(NL=12, K=3, H=2) if path == "full" else P.PATHS[path]
    raw, head_raw = _tables(S, kw["NL"], kw.get("H", 0))
    sched = P.make_schedule(S, pick=P.picker(raw, head_raw), **kw)
    want = P.reference_rules(sched, raw, head_raw)
    got = P.device_rules(sched, raw, head_raw)
    assert np.array_equal(P.bits(got["scores"]), P.bits(want["scores"]))
    assert np.array_equal(P.bits(got["bank"]), P.bits(want["bank"]))
    assert (want["scores"] != 0).any() and (not sched.K or (want["bank"] != 0).any())


@pytest.mark.parametrize("fault", P.FAULTS)
def test_every_fault_moves_a_final_score(full, fault):
    sched, raw, head_raw, want = full
    assert P.moved(want, P.device_rules(sched, raw, head_raw, fault=fault)) > 0, P.FAULT_NOTES[fault]


@pytest.mark.parametrize("path,S", [(p, 37) for p in P.PATHS] + [(p, 1) for p in ("epilogue", "long", "bank")])     # (as the GPU tier)
def test_each_gpu_path_schedule_lets_every_applicable_fault_show(path, S):
    """The schedule alone -- call shapes, rule phases, resets, masks, the VAD script -- satisfies the GPU tests' no-vacuity condition on
    scripted tables; on the device the measured tables take their place.  One stream's 70 calls cannot show every fault at once: as in
    the GPU tests, an S = 1 handle is run on one table after the other until the passes together have shown them all."""
    kw = P.PATHS[path]
    total = {}
    for seed in range(1 if S > 1 else 8):
        raw, head_raw = P.scripted_tables(S, kw["NL"], kw.get("H", 0), seed=3 + S + seed)
        sched, want, counts = P.choose_schedule(lambda pick, vad: P.make_schedule(S, pick=pick, vad_seed=vad, **kw), raw, head_raw,
                                                tries=4 if S > 1 else 2)
        assert set(counts) == set(sched.applicable())
        for f, n in counts.items():
            total[f] = total.get(f, 0) + n
        if all(n > 0 for n in total.values()):
            break
    silent = [f for f, n in total.items() if n == 0]
    assert not silent, silent
