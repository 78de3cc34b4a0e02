"""The head kernels against the FLOAT64 oracle at every shape of their first layer's k loop (tests/head_windows.py; the CPU tier that
admits the cases and guards their coverage is test_head_windows_cpu.py).  The window length T alone decides how the weight ring's
conditional tail groups run, and the other head files fix T = 16 / 34; here T moves through the lengths whose KST = 3 T leaves every
residue of the ring depths 2, 4 and 6, through KST <= D and an empty main loop, on external features, on the feature ring (row slots
that wrap inside a window), under a participant list, in the bank kernel at both wave counts, and -- side cases -- in the exact-fp32,
generic and recurrent kernels up to the longest window each accepts.  Contract everywhere: every score finite, within TOL_SCORE of
O.head_stage(..., float64), the range flag down (head_windows.check_scores).  pytest -m gpu -s prints the worst error of every case;
DESIGN.md 5.22 records them."""
import functools

import numpy as np
import pytest

from oracle import oww_oracle as O
from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine, _ptr

import head_windows as HW

pytestmark = pytest.mark.gpu

MAX_HEADS, MAX_LABELS = 16, 32           # include/owwhip.h: OWW_MAX_HEADS, OWW_MAX_LABELS
PIN = "OWW_SMALL_WGS_HEADS"              # read at commit; 0 = never the deep weight rings


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


def _t_chunks(form):
    """The window lengths of a form, as many per engine as the handle's head and label limits allow."""
    shapes = HW.FORMS[form]["heads"]
    per = min(MAX_HEADS // len(shapes), MAX_LABELS // sum(s["n_out"] for s in shapes))
    Ts = HW.FORMS[form]["Ts"]
    return [Ts[i:i + per] for i in range(0, len(Ts), per)]


def _sums_to_one(got):
    if got.shape[1] > 1:
        np.testing.assert_allclose(got.sum(axis=1), 1.0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 1. external features, both rings
@pytest.mark.parametrize("form", HW.RING_FORMS)
def test_external_windows_match_float64_on_both_rings(form, monkeypatch):
    """eng.head() of every (form, T) against float64 with the ring the launch picks itself (deep at 37 rows: 6 slots for one or two
    narrow nets and one wide net, 4 otherwise) and pinned to two slots; the two runs bit for bit the same -- the kernel's "same
    arithmetic in the same order"."""
    worst = [0.0]
    for Ts in _t_chunks(form):
        heads = {}
        for T in Ts:
            heads.update(HW.form_heads(form, T))
        runs = {}
        for pin in ("default", "two-slot"):
            if pin == "two-slot":
                monkeypatch.setenv(PIN, "0")
            else:
                monkeypatch.delenv(PIN, raising=False)
            eng = StreamEngine(HW.N_ROWS, heads, _emb())
            try:
                for T in Ts:
                    for n, ref in HW.want(form, T).items():
                        got = eng.head(n, HW.windows(T))
                        HW.check_scores(f"{n} {pin}", got, ref, eng.range_status(clear=True), worst)
                        _sums_to_one(got)
                        runs[pin, n] = got
            finally:
                eng.close()
                monkeypatch.delenv(PIN, raising=False)
        for n in heads:
            assert np.array_equal(runs["default", n], runs["two-slot", n]), f"{n}: the deep and the two-slot ring differ in " \
                f"rows {np.nonzero((runs['default', n] != runs['two-slot', n]).any(axis=1))[0].tolist()}"
    print(f"\n{form}: worst |score - float64| over T {HW.FORMS[form]['Ts']} x both rings = {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ 2. ring mode
RING_MODE_FORMS = ("narrow4", "narrow2", "wide2")      # committed in this order: launches of 4 narrow nets, a gated pair, 2 wide nets
RING_STEPS_MAX = HW.BANK_RING + 2
S_RING, S_MASKED = 37, 133


def _ring_rows(T):
    return max(16, T + 3)               # (a handle's feature ring has sixteen rows at least)


@functools.lru_cache(maxsize=None)
def _pcm(S):
    """int16 [S, 27 * 1280]: noise whose level differs from stream to stream (60 dB in all; stream 0 silent), so that the embeddings and
    with them the heads' logits differ between the streams."""
    amp = np.geomspace(1e-3, 1.0, S)
    amp[0] = 0.0
    x = W.synthetic_pcm(S, 1280 * RING_STEPS_MAX, seed=77, rms=8000.0).astype(np.float64) * amp[:, None]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _chunk(S, t):
    return _pcm(S)[:, 1280 * t:1280 * (t + 1)]


@functools.lru_cache(maxsize=None)
def _init_rows(S):
    return np.random.default_rng(78).normal(0.0, 1.0, (S, RING_STEPS_MAX + 1, 96)).astype(np.float32)


def _seed(eng, S):
    for s in range(S):
        eng.reset([s], _init_rows(S)[s, :eng.feature_ring])


@functools.lru_cache(maxsize=None)
def _embedding_rows(S):
    """float32 [27, S, 96]: the row the CNN appends to each stream's feature ring at each step of _pcm(S), from a handle of its own.
    Used only to centre the heads of the ring-mode and bank tests on the windows they will meet; every comparison reads the rows of
    the handle under test."""
    eng = StreamEngine(S, {"probe": W.synthetic_head("alexa", 1234)}, _emb())
    try:
        _seed(eng, S)
        out = np.zeros((RING_STEPS_MAX, S, 96), np.float32)
        for t in range(RING_STEPS_MAX):
            eng.step(_chunk(S, t))
            out[t] = np.stack([eng.get_features(s, 1)[0] for s in range(S)])
    finally:
        eng.close()
    out.setflags(write=False)
    return out


def _probe_windows(S, T, n_steps, ring):
    """[S, T, 96]: each stream's last T rows after n_steps on a ring of `ring` rows (seeded rows where the window reaches back before
    the first step)."""
    rows = np.concatenate([_init_rows(S).transpose(1, 0, 2)[:ring], _embedding_rows(S)[:n_steps]])[-T:]
    return np.ascontiguousarray(rows.transpose(1, 0, 2))


def _ring_heads(S, T):
    """The ring-mode handle's heads at window length T, centred on the windows of the step before the last."""
    ft = _probe_windows(S, T, _ring_rows(T) + 1, _ring_rows(T))
    heads = {}
    for form in RING_MODE_FORMS:
        for i, shape in enumerate(HW.FORMS[form]["heads"]):
            name = f"{form}_ring_t{T}_{i}"
            heads[name] = HW.centre(HW.draw_head(name, shape, T, seed=3), ft)
    groups, other = HW.head_groups(heads)
    assert [(g["ht"], g["n_nets"]) for g in groups] == [(4, 4), (4, 2), (8, 2)] and not other
    return heads


def _raw(eng):
    out = np.empty((eng.n_streams, eng.n_labels), dtype=np.float32)
    _lib.check(eng._lib.oww_get_raw(eng._h, _ptr(out)))
    return out


def _own_windows(eng, T, streams=None):
    return np.stack([eng.get_features(s, T) for s in (range(eng.n_streams) if streams is None else streams)])


def _check_ring_step(eng, heads, T, raw, label, worst, streams=None):
    ft = _own_windows(eng, T, streams)
    rows = slice(None) if streams is None else streams
    shares = []
    for n, h in heads.items():
        lo, hi = eng.head_cols[n]
        ref = O.head_stage(ft, h, np.float64)
        HW.check_scores(f"{n} {label}", raw[rows, lo:hi], ref, False, worst)
        _sums_to_one(raw[rows, lo:hi])
        if HW.is_binary(h):
            shares.append(HW.mid_fraction(ref))
    return shares


@pytest.mark.parametrize("T", HW.T_EDGE)
def test_ring_windows_match_float64(T):
    """A handle whose feature ring is three rows longer than T (sixteen at least), every stream seeded with rows of its own, stepped
    ring + 2 times one chunk at a time: the windows' row slots wrap at positions T does not divide.  After each of the last three steps
    every stream's raw scores against float64 on that stream's own get_features(s, T) -- the heads alone are judged, the CNN has
    tests/test_cnn_regimes.py."""
    S, ring = S_RING, _ring_rows(T)
    heads = _ring_heads(S, T)
    worst = [0.0]
    eng = StreamEngine(S, heads, _emb(), feature_ring=ring)
    try:
        assert eng.feature_ring == ring
        _seed(eng, S)
        for t in range(ring + 2):
            raw = eng.step_raw(_chunk(S, t))
            if t >= ring - 1:
                shares = _check_ring_step(eng, heads, T, raw, f"step {t + 1}", worst)
                if t == ring:                               # the step the heads were centred on: the comparison is not vacuous
                    print(f"\nT={T}: share of float64 scores in (0.05, 0.95) per binary head: {[round(x, 2) for x in shares]}")
                    assert min(shares) >= HW.MID_SHARE
        assert eng.range_status() is False
    finally:
        eng.close()
    print(f"\nring mode T={T} (ring {ring}): worst |score - float64| = {worst[0]:.2e}")


def test_ring_windows_under_a_participant_list():
    """T = 19 on a ring of 22 rows, 133 streams (two workgroups): a masked step at one quarter participation runs the heads from the
    participant list.  The participants score what float64 scores on their own rows and, bit for bit, what an unmasked twin handle fed
    the same chunk scores for them; the others keep their raw scores."""
    S, T = S_MASKED, 19
    ring = _ring_rows(T)
    heads = _ring_heads(S, T)
    on = np.random.default_rng(5).random(S) < 0.25
    assert 8 <= on.sum() <= S // 2 and on[:128].any() and on[128:].any()
    part = np.nonzero(on)[0]
    worst = [0.0]
    a, b = StreamEngine(S, heads, _emb(), feature_ring=ring), StreamEngine(S, heads, _emb(), feature_ring=ring)
    try:
        for e in (a, b):
            _seed(e, S)
            for t in range(ring + 1):
                e.step_raw(_chunk(S, t))
        before = _raw(a)
        a.step_masked(_chunk(S, ring + 1), on)
        raw_a = _raw(a)
        raw_b = b.step_raw(_chunk(S, ring + 1))
        _check_ring_step(a, heads, T, raw_a, "masked step", worst, part)
        assert np.array_equal(raw_a[on], raw_b[on]), f"participants {part[(raw_a[on] != raw_b[on]).any(axis=1)].tolist()} differ from the unmasked twin"
        assert np.array_equal(raw_a[~on], before[~on]), "a stream that sat the step out changed its raw scores"
        assert (raw_b[~on] != before[~on]).any()            # (the step does move scores)
        assert a.range_status() is False and b.range_status() is False
    finally:
        a.close(); b.close()
    print(f"\nparticipant list T={T}: {on.sum()} of {S} streams, worst |score - float64| = {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ 3. bank
BANK_STEPS = 7               # the sixth prediction is the first that is not zeroed (model.py:331-333): steps 6 and 7 are compared


@pytest.mark.parametrize("waves", sorted(HW.BANK_SUBSCRIBERS))
@pytest.mark.parametrize("form", sorted(HW.BANK_FORMS))
def test_bank_windows_match_float64_and_the_fixed_kernel(form, waves):
    """One bank head per T of T_EDGE on a handle with fixed heads at T = 16 and a feature ring of 25 rows, every stream subscribed to
    all seven: 37 streams make one-wave tiles, 133 four-wave tiles.  bank_scores() of steps 6 and 7 against float64 on the streams' own
    ring rows, and bit for bit what the same nets score as fixed heads of a twin handle on the same PCM (heads_gemm1's promise; the
    twin's launches run the six-slot ring, the bank kernel two slots)."""
    S = HW.BANK_SUBSCRIBERS[waves]
    cls = 0 if form == "bank_ht4" else 1
    fixed = HW.form_heads("narrow4", HW.T_FULL)
    bank = {T: HW.bank_head(form, T, _probe_windows(S, T, BANK_STEPS, HW.BANK_RING)) for T in HW.T_EDGE}
    twin_heads = {f"{form}_t{T}": bank[T] for T in HW.T_EDGE}
    worst = [0.0]
    eng = StreamEngine(S, fixed, _emb(), feature_ring=HW.BANK_RING, bank_slots=len(bank), bank_capacity=8)
    twin = StreamEngine(S, twin_heads, _emb(), feature_ring=HW.BANK_RING)
    try:
        assert eng.feature_ring == twin.feature_ring == HW.BANK_RING
        ids = [eng.bank_add(bank[T]) for T in HW.T_EDGE]
        for e in (eng, twin):
            _seed(e, S)
        eng.subscribe(np.arange(S), np.tile(np.array(ids, np.int32), (S, 1)))
        r = eng.bank_routing()
        assert r["waves_per_tile"][cls] == waves and r["entries"][cls] == S * len(ids) and r["entries"][1 - cls] == 0
        for t in range(BANK_STEPS):
            eng.step(_chunk(S, t))
            fx = twin.step(_chunk(S, t))
            if t < BANK_STEPS - 2:
                continue
            got = eng.bank_scores()
            rows = _own_windows(eng, HW.BANK_RING)
            assert np.array_equal(rows, _own_windows(twin, HW.BANK_RING))
            shares = []
            for k, T in enumerate(HW.T_EDGE):
                ref = O.head_stage(rows[:, -T:], bank[T], np.float64)
                HW.check_scores(f"{form} T={T} waves={waves} step {t + 1}", got[:, k:k + 1], ref, False, worst)
                lo, hi = twin.head_cols[f"{form}_t{T}"]
                assert np.array_equal(got[:, k], fx[:, lo]), f"{form} T={T}: bank and fixed kernel differ for streams {np.nonzero(got[:, k] != fx[:, lo])[0].tolist()}"
                shares.append(HW.mid_fraction(ref))
            if t == BANK_STEPS - 1:
                print(f"\n{form} waves={waves}: share of float64 scores in (0.05, 0.95) per T: {[round(x, 2) for x in shares]}")
                assert min(shares) >= HW.MID_SHARE
        raw = _raw(eng)                                     # the fixed heads of the bank handle, on its own rows too
        for n, h in fixed.items():
            lo, hi = eng.head_cols[n]
            HW.check_scores(f"{n} beside the bank", raw[:, lo:hi], O.head_stage(rows[:, -HW.T_FULL:], h, np.float64), False)
        assert eng.range_status() is False and twin.range_status() is False
    finally:
        eng.close(); twin.close()
    print(f"\n{form} waves={waves}: worst |bank score - float64| over T {HW.T_EDGE} = {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ 4. side cases
SIDE_ROWS = (1, 5, 37)       # streams of the handle = rows of the call; the recurrent kernel's last wave of two then holds one stream
_SIDE = [(f, fam) for f, spec in HW.FORMS.items() if "nn" not in spec for fam in (spec["fam"] if isinstance(spec["fam"], tuple) else (spec["fam"],))]


@pytest.mark.parametrize("form,fam", _SIDE, ids=[f"{f}-mfma{fam}" for f, fam in _SIDE])
def test_side_kernels_match_float64(form, fam):
    """heads64_kernel (use_mfma = 1) at T 1, 19, 120; the generic kernel (130 hidden units) at T = 120; heads_rnn_kernel at T 1, 2, 63
    and 64 (its largest LDS footprint) with one and eight outputs, in the default and the plain family."""
    Ts = HW.FORMS[form]["Ts"]
    heads = {}
    for T in Ts:
        heads.update(HW.form_heads(form, T))
    if form.startswith("rnn"):
        assert not HW.head_groups(heads)[0]
    worst = [0.0]
    for S in SIDE_ROWS:
        eng = StreamEngine(S, heads, _emb(), use_mfma=fam)
        try:
            for T in Ts:
                for n, ref in HW.want(form, T).items():
                    got = eng.head(n, HW.windows(T)[:S])
                    HW.check_scores(f"{n} use_mfma={fam} S={S}", got, ref[:S], eng.range_status(clear=True), worst)
                    _sums_to_one(got)
        finally:
            eng.close()
    print(f"\n{form} use_mfma={fam}: worst |score - float64| over T {Ts} x S {SIDE_ROWS} = {worst[0]:.2e}")
