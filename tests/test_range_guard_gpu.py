"""The f16 range guard at every layer that keeps a history and at every head form (use_mfma = 3).

A. A conv history of ONE stream is driven out of the f16 range through its state record (tests/range_guard.py: export, poison,
   import).  The next step must raise OwwRangeError, oww_range_where must name the block of streams the guard of that layer reports
   -- (first, min(n, S - first)), n from range_guard.REPORTED_STREAMS, first a multiple of n, the offender inside -- and every stream
   outside the block must carry the bits of a twin handle that heard the same audio and was never poisoned (oww_get_raw and the
   device's score matrix, read after the flag was cleared).  Whole sections at streams 0, 31, 32, 63, 68 of 69; one seeded word at
   stream 32; the whole-section form again under the resident stage B, the unfused front end, two-chunk steps, a captured graph,
   submit / collect and masked steps; the VAD's (h, c) section on a handle with a VAD.
   Masked steps over a participant list (a third of the streams): the header promises (-1, 0) for the position there.  That is the
   heads kernel's case (it walks the list, a wave is no block of streams): asserted for hist19.  The stage kernels walk a list of
   GROUPS and still know theirs (hstage_kernel: s_first = glist[g] * SPT; the front end walks the streams themselves), so for their
   sections the exact block is asserted under the list too.
B. Recovery as serve._recover_range does it, with two offenders in one step.
C. eng.embed(mel * 2^k): flag down -> every window inside cnn_budget.T of float64; flag up -> nothing asked of the values.
D. Every head form under features * 2^k: flag down -> within TOL_SCORE of float64; and one loud row in a dense call.
E. conv19 on a bank-only handle whose offender is subscribed to nothing."""
import ctypes as C

import numpy as np
import pytest

from oracle import oww_oracle as O
from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd._lib import OwwRangeError
from openwakeword_amd.engine import StreamEngine

import cnn_budget as CB
import range_guard as RG
import test_head_regimes as HR

pytestmark = pytest.mark.gpu

S = 69                                   # two full waves of 32 + a wave whose last group of eight holds five
OFFENDERS = (0, 31, 32, 63, 68)
WARM = 3
N_CHUNKS = 32


def _emb():
    return W.synthetic_embedding(1234)


def _fixed_heads():
    return {n: RG.make_head(n) for n in RG.FIXED_SHAPES}


_PCM = W.synthetic_pcm(S, 1280 * N_CHUNKS, seed=515)                  # noise audio, rms 3000
_PCM.setflags(write=False)


def _chunk(t, n=1):
    return np.ascontiguousarray(_PCM[:, 1280 * t:1280 * (t + n)])


def _pair(**kw):
    kw.setdefault("feature_ring", 16)
    return (StreamEngine(S, _fixed_heads(), _emb(), **kw), StreamEngine(S, _fixed_heads(), _emb(), **kw))


def _raw(e):
    out = np.empty((e.n_streams, e.n_labels), np.float32)
    _lib.check(e._lib.oww_get_raw(e._h, out.ctypes.data_as(C.c_void_p)))
    return out


def _scores_dev(e):
    """The device's score matrix (oww_scores_dev), copied with the HIP runtime the library itself is linked against."""
    fn = _lib.load()["hipMemcpy"]
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty((e.n_streams, e.n_labels), np.float32)
    assert e.scores_dev_ptr and fn(out.ctypes.data, e.scores_dev_ptr, out.nbytes, 2) == 0
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_outside_equal(eng, twin, first, n, what):
    keep = np.ones(S, bool)
    keep[first:first + n] = False
    for name, fn in (("oww_get_raw", _raw), ("oww_scores_dev", _scores_dev)):
        a, b = _bits(fn(eng)), _bits(fn(twin))
        bad = np.flatnonzero((a != b).any(axis=1) & keep)
        assert bad.size == 0, f"{what}: {name} of streams {bad.tolist()} outside [{first}, {first + n}) differs from the twin"
    assert np.isfinite(_raw(twin)).all()


def _step_plain(e):
    return e.step(_chunk(WARM))


def _warm(eng, twin):
    for e in (eng, twin):
        e.reset()
        for t in range(WARM):
            e.step(_chunk(t))


def _poisoned_step(eng, twin, section, s, seed=None, step=_step_plain, has_vad=False):
    """Warm both handles, poison `section` of stream s of `eng`, step both once -> range_where of eng (flag cleared on return)."""
    _warm(eng, twin)
    rec = eng.export_state([s])[0]
    words = None if seed is None else RG.seeded_words(rec, section, seed, has_vad)
    eng.import_state([s], RG.poison(rec, section, words, has_vad)[None])
    step(twin)
    assert twin.range_status() is False
    with pytest.raises(OwwRangeError):
        step(eng)
    where = eng.range_where()
    assert eng.range_status(clear=True) is True
    assert eng.range_where() == (-1, 0) and eng.range_status() is False
    return where


def _check_case(eng, twin, section, s, what, **kw):
    where = _poisoned_step(eng, twin, section, s, **kw)
    n_tab = RG.REPORTED_STREAMS[section]
    first, n = where
    assert where == RG.expected_where(section, s, S), f"{what}: range_where = {where}"
    assert first % n_tab == 0 and first <= s < first + n and n == min(n_tab, S - first)
    _assert_outside_equal(eng, twin, first, n, what)


# ------------------------------------------------------------------------------------------------ A. every history-bearing layer
@pytest.fixture(scope="module")
def pair():
    eng, twin = _pair()
    yield eng, twin
    eng.close(); twin.close()


def test_record_is_where_the_mirror_says(pair):
    eng, twin = pair
    _warm(eng, twin)
    nb = eng.state_info()[0]
    off = RG.offsets(nb)
    rec = eng.export_state([32])[0]
    for name in RG.NAMES:
        assert RG.candidate_words(rec, name).size > off[name][1] // 4, f"{name}: a warmed-up history is mostly non-zero"
    # hist2's dwords 6, 7 are never written; hist_mel holds f16 pairs of mel values in [0, 12]
    h2 = rec.view(np.uint32)[off["hist2"][0]:][:2048].reshape(4, 8, 64)
    assert not h2[:, 6:].any() and h2[:, :3].any()
    hm = rec.view(np.uint32)[off["hist_mel"][0]:][:64]
    hi = (hm & 0xffff).astype(np.uint16).view(np.float16).astype(np.float32)
    assert (hi > -1.0).all() and (hi < 16.0).all() and np.ptp(hi) > 0


@pytest.mark.parametrize("section", RG.NAMES)
def test_whole_section(pair, section):
    eng, twin = pair
    for s in OFFENDERS:
        _check_case(eng, twin, section, s, f"{section} of stream {s}")


@pytest.mark.parametrize("section", RG.NAMES)
def test_one_word(pair, section):
    eng, twin = pair
    for seed in range(8):
        _check_case(eng, twin, section, 32, f"{section}, one word (seed {seed}) of stream 32", seed=seed)


@pytest.mark.parametrize("env,sections", [("OWW_RESIDENT_B", ("B:b", "B:d")), ("OWW_NO_FUSE", ("hist_mel", "hist2"))])
def test_whole_section_other_kernel_forms(monkeypatch, env, sections):
    monkeypatch.setenv(env, "1")
    eng, twin = _pair()
    try:
        for section in sections:
            for s in OFFENDERS:
                _check_case(eng, twin, section, s, f"{env}=1: {section} of stream {s}")
    finally:
        eng.close(); twin.close()


def _step_two_chunks(e):
    return e.step(_chunk(WARM, 2))


def _step_pipelined(e):
    pcm = _chunk(WARM)
    e.submit(pcm)                         # (the flag is still down: submit itself succeeds)
    return e.collect()


def _mask(s, every):
    return (np.arange(S) % every == s % every).astype(np.uint8)


@pytest.mark.parametrize("variant", ["two_chunks", "graph", "submit_collect", "masked_all"])
def test_whole_section_step_variants(variant):
    eng, twin = _pair(max_chunks=2 if variant == "two_chunks" else 1)
    try:
        if variant == "graph":
            for e in (eng, twin):
                e.use_graph(True)
                e.step(_chunk(0))         # the captured clean step
        step = {"two_chunks": _step_two_chunks, "graph": _step_plain, "submit_collect": _step_pipelined,
                "masked_all": lambda e: e.step_masked(_chunk(WARM), np.ones(S, np.uint8))}[variant]
        for section in RG.NAMES:
            for s in OFFENDERS:
                _check_case(eng, twin, section, s, f"{variant}: {section} of stream {s}", step=step)
    finally:
        eng.close(); twin.close()


def test_whole_section_masked_participant_list():
    """A third of the streams take part, the offender among them (23 of 69: at most half, so the launches walk lists)."""
    eng, twin = _pair()
    try:
        for section in RG.NAMES:
            for s in OFFENDERS:
                on = _mask(s, 3)
                assert on[s] and 2 * int(on.sum()) <= S
                where = _poisoned_step(eng, twin, section, s, step=lambda e: e.step_masked(_chunk(WARM), on))
                block = RG.expected_where(section, s, S)
                if section == "hist19":
                    assert where == (-1, 0), f"{section} of stream {s}: the heads walk a participant list, range_where = {where}"
                else:
                    assert where == block, f"{section} of stream {s}: range_where = {where}"
                _assert_outside_equal(eng, twin, block[0], block[1], f"participant list: {section} of stream {s}")
    finally:
        eng.close(); twin.close()


def test_vad_state():
    vad = W.synthetic_vad()
    eng, twin = _pair(vad=vad)
    try:
        assert eng.state_info()[0] == RG.DEFAULT_RECORD_BYTES + 4 * (4 + RG.VAD_HC_WORDS)
        where = _poisoned_step(eng, twin, RG.VAD_HC, 40, has_vad=True)
        assert where == (32, 16) == RG.expected_where(RG.VAD_HC, 40, S)
        _assert_outside_equal(eng, twin, 32, 16, "VAD (h, c) of stream 40")
        keep = np.ones(S, bool)
        keep[32:48] = False
        assert np.array_equal(_bits(eng.get_vad())[keep], _bits(twin.get_vad())[keep])
    finally:
        eng.close(); twin.close()


# ------------------------------------------------------------------------------------------------ B. recovery
def test_recovery_resets_only_the_named_streams(pair):
    """Two offenders in one step.  Each round: range_where -> clear -> reset the named streams -> step.  The flag must be down after
    at most two rounds and stay down for 20 steps; a stream that was never named carries the twin's bits at every step; a stream
    that was reset carries the bits of the twin's stream reset at the same step."""
    eng, twin = pair
    _warm(eng, twin)
    rec = eng.export_state([5, 50])
    eng.import_state([5, 50], np.stack([RG.poison(rec[0], "C:b"), RG.poison(rec[1], "E:d")]))
    named = np.zeros(S, bool)
    t, rounds, quiet = WARM, 0, 0
    while quiet < 21:
        assert t < N_CHUNKS
        twin.step(_chunk(t))
        try:
            eng.step(_chunk(t))
            quiet += 1
        except OwwRangeError:
            assert quiet == 0, f"the flag came back {quiet} steps after the recovery"
            rounds += 1
            assert rounds <= 2, "the recovery loop needed a third round"
            first, n = eng.range_where()
            assert n > 0 and (first <= 5 < first + n or first <= 50 < first + n), (first, n)
            assert eng.range_status(clear=True) is True
            ids = np.arange(first, first + n)
            named[ids] = True
            eng.reset(ids)
            twin.reset(ids)
        t += 1
        if quiet:                                       # the handle scores again: everybody carries the twin's bits
            for name, fn in (("raw", _raw), ("scores", _scores_dev)):
                bad = np.flatnonzero((_bits(fn(eng)) != _bits(fn(twin))).any(axis=1))
                assert bad.size == 0, f"step {t - 1} ({quiet} after the recovery): {name} of streams {bad.tolist()} differs (named: {np.flatnonzero(named).tolist()})"
        else:
            keep = ~named
            keep[[5, 50]] = False                       # (an offender not yet named is wrong until its round)
            bad = np.flatnonzero((_bits(_raw(eng)) != _bits(_raw(twin))).any(axis=1) & keep)
            assert bad.size == 0, f"step {t - 1}: streams {bad.tolist()} were never named and differ from the twin"
    assert 1 <= rounds <= 2 and eng.range_status() is False
    assert named[5] and named[50], f"an offender was never named (named: {np.flatnonzero(named).tolist()}) and still agrees with nobody"


# ------------------------------------------------------------------------------------------------ C. the CNN across the boundary
@pytest.mark.parametrize("name", RG.CNN_REGIMES)
def test_cnn_gain_sweep(name):
    emb, hseed = CB.regime(name)
    x = RG.cnn_inputs()
    eng = StreamEngine(8, CB.heads_for(name, hseed), emb)
    first_up, state = None, []
    try:
        for g in RG.MEL_GAINS:
            xg = x * np.float32(g)
            try:
                got = eng.embed(xg)
                up = eng.range_status(clear=True)
            except OwwRangeError:
                got, up = None, True
                assert eng.range_status(clear=True) is True
            state.append(up)
            if up:
                first_up = first_up or g
                continue
            e64 = O.embedding_stage(xg, emb, np.float64)[:, :, 0, :]
            r = RG.window_ratios(got, e64)
            print(f"\n{name} gain 2^{int(np.log2(g))}: flag down, worst window {r.max() / CB.T:.3f} x T")
            assert r.max() <= CB.T, (f"{name}, gain 2^{int(np.log2(g))}: flag DOWN and window {int(np.argmax(r))} is {r.max() / CB.T:.2f} x T "
                                     f"off float64 -- a finite wrong answer the guard did not see")
        print(f"\n{name}: first flag at mel gain 2^{int(np.log2(first_up)) if first_up else None}; flags {['up' if u else 'down' for u in state]}")
        assert state[0] is False, "gain 2^0 must score"
        assert state[-1] is True, "gain 2^24 must be loud"
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ D. every head form
def _flagged(call):
    """call() -> (result or None, flag was up); the flag is cleared by the caller's engine afterwards."""
    try:
        return call(), False
    except OwwRangeError:
        return None, True


@pytest.fixture(scope="module")
def fixed_eng():
    heads = {n: RG.make_head(n) for n in (*RG.FIXED_SHAPES, "gated")}
    eng = StreamEngine(8, heads, _emb())
    yield eng, heads
    eng.close()


@pytest.fixture(scope="module")
def bank_eng():
    eng = StreamEngine(8, {}, _emb(), bank_slots=2, bank_capacity=4)
    heads = {n: RG.make_head(n) for n in RG.BANK_SHAPES}
    ids = {n: eng.bank_add(h) for n, h in heads.items()}
    yield eng, heads, ids
    eng.close()


def _sweep(form, run, want):
    """run(gain) -> (scores or None, up); want(gain, scores) -> float64 reference.  The rule of part D."""
    states = []
    for g in RG.FEATURE_GAINS:
        got, up = run(g)
        states.append(up)
        if up:
            continue
        with np.errstate(over="ignore"):                # (exp of a saturated logit in the float64 sigmoid)
            ref = want(g, got)
        assert np.isfinite(got).all(), f"{form}, gain {g:g}: non-finite score with the flag down"
        err = float(np.abs(got.astype(np.float64) - ref).max())
        assert err <= HR.TOL_SCORE, f"{form}, gain 2^{int(np.log2(g))}: flag DOWN and |device - float64| = {err:.2e}"
    ups = [int(np.log2(g)) for g, u in zip(RG.FEATURE_GAINS, states) if u]
    print(f"\n{form}: first flag at feature gain 2^{ups[0] if ups else None}")
    assert states[0] is False, f"{form}: gain 2^0 must score"
    assert states[-1] is True, f"{form}: gain 2^20 must be loud"


@pytest.mark.parametrize("form", [*RG.FIXED_SHAPES, "gated"])
def test_head_entry_gain_sweep(fixed_eng, form):
    eng, heads = fixed_eng
    ft = HR.features(16)

    def run(g):
        got, up = _flagged(lambda: eng.head(form, ft * np.float32(g)))
        return got, eng.range_status(clear=True) or up

    _sweep(f"head({form})", run, lambda g, got: O.head_stage(ft * np.float32(g), heads[form], np.float64))


@pytest.mark.parametrize("form", list(RG.BANK_SHAPES))
def test_live_bank_gain_sweep(bank_eng, form):
    """The features go in through reset(init_features); six steps follow, because the first five predictions of a slot read zero
    (model.py:331-333): the sixth score is the head on ten of those rows and six rows of the CNN, taken as the device holds them."""
    eng, heads, ids = bank_eng
    ft = HR.features(16)[:8]
    pcm = W.synthetic_pcm(8, 1280 * 6, seed=42)
    sub = np.full((8, 2), -1, np.int32)
    sub[:, 0] = ids[form]

    def run(g):
        eng.subscribe(np.arange(8), np.full_like(sub, -1))
        for s in range(8):
            eng.reset([s], ft[s] * np.float32(g))
        eng.subscribe(np.arange(8), sub)
        up = False
        for t in range(6):
            _, u = _flagged(lambda: eng.step(pcm[:, 1280 * t:1280 * (t + 1)]))
            up = eng.range_status(clear=True) or u or up
        got, u = _flagged(lambda: eng.bank_scores()[:, 0])
        return got, eng.range_status(clear=True) or u or up

    def want(g, got):
        win = np.stack([eng.get_features(s, 16) for s in range(8)])
        return O.head_stage(win, heads[form], np.float64)[:, 0]

    _sweep(f"live {form}", run, want)
    eng.subscribe(np.arange(8), np.full_like(sub, -1))
    eng.reset()


def _dense_call(eng, feats, ids=None):
    """oww_score_features / oww_bank_score_features through the bound C entry, so that the scores survive an OWW_ERANGE return ->
    (return code, scores)."""
    f = np.ascontiguousarray(feats, dtype=np.float32)
    B, n_rows, _ = f.shape
    if ids is None:
        n_win, _ = eng.score_shape(n_rows)
        out = np.full((B, n_win, eng.n_labels), np.nan, np.float32)
        rc = eng._lib.oww_score_features(eng._h, f.ctypes.data_as(C.c_void_p), 0, B, n_rows, out.ctypes.data_as(C.c_void_p), 0)
    else:
        a = np.ascontiguousarray(ids, dtype=np.int32)
        n_win, _ = eng.bank_score_shape(a, n_rows)
        out = np.full((B, n_win, a.size), np.nan, np.float32)
        rc = eng._lib.oww_bank_score_features(eng._h, f.ctypes.data_as(C.c_void_p), 0, B, n_rows, a.ctypes.data_as(C.c_void_p), a.size,
                                              out.ctypes.data_as(C.c_void_p), 0)
    return rc, out


def _dense_sequences(n_rows, B=3, seed=9):
    f = np.random.default_rng(seed).normal(0.0, 2.0, (B, n_rows, 96)).astype(np.float32)
    f.setflags(write=False)
    return f


def _windows(f, T=16):
    B, n_rows, _ = f.shape
    return np.stack([f[:, w:w + T] for w in range(n_rows - T + 1)], axis=1).reshape(-1, T, 96)


def test_dense_fixed_gain_sweep(fixed_eng):
    eng, heads = fixed_eng
    f = _dense_sequences(40, B=2)
    cols = [eng.head_cols[n][0] for n in heads]

    def run(g):
        rc, out = _dense_call(eng, f * np.float32(g))
        up = eng.range_status(clear=True)
        assert rc in (0, _lib.ERANGE) and (rc == _lib.ERANGE) == up
        return (None if up else out[:, :, cols].reshape(-1, len(cols))), up

    def want(g, got):
        w = _windows(f * np.float32(g))
        return np.concatenate([O.head_stage(w, h, np.float64) for h in heads.values()], axis=1)

    _sweep("score_features", run, want)


def test_dense_bank_gain_sweep(bank_eng):
    eng, heads, ids = bank_eng
    f = _dense_sequences(40, B=2)
    lst = [ids[n] for n in heads]

    def run(g):
        rc, out = _dense_call(eng, f * np.float32(g), lst)
        up = eng.range_status(clear=True)
        assert rc in (0, _lib.ERANGE) and (rc == _lib.ERANGE) == up
        return (None if up else out.reshape(-1, len(lst))), up

    def want(g, got):
        w = _windows(f * np.float32(g))
        return np.concatenate([O.head_stage(w, h, np.float64) for h in heads.values()], axis=1)

    _sweep("bank_score_features", run, want)


LOUD_SEQ, LOUD_ROW, N_WIN = 1, 137, 261


def _loud():
    clean = _dense_sequences(N_WIN + 15, B=3, seed=10)
    loud = np.array(clean)
    loud[LOUD_SEQ, LOUD_ROW, 40] = 1.0e6
    touched = np.zeros((3, N_WIN), bool)
    touched[LOUD_SEQ, LOUD_ROW - 15:LOUD_ROW + 1] = True              # the windows w .. w + 15 that hold the row
    return clean, loud, touched


def test_dense_fixed_one_loud_row(fixed_eng):
    eng, heads = fixed_eng
    clean, loud, touched = _loud()
    rc, ref = _dense_call(eng, clean)
    assert rc == 0 and ref.shape[:2] == (3, N_WIN) and np.isfinite(ref).all() and eng.range_status() is False
    rc, got = _dense_call(eng, loud)
    assert rc == _lib.ERANGE and eng.range_status(clear=True) is True
    moved = (_bits(got) != _bits(ref)).any(axis=2)
    assert not (moved & ~touched).any(), f"windows {np.argwhere(moved & ~touched)[:8].tolist()} do not hold the loud row and changed"


def test_dense_bank_one_loud_row(bank_eng):
    eng, heads, ids = bank_eng
    clean, loud, touched = _loud()
    lst = [ids["bank64"], ids["bank128"], ids["bank64"]]              # (two heads of one slice, and a duplicate)
    rc, ref = _dense_call(eng, clean, lst)
    assert rc == 0 and ref.shape == (3, N_WIN, 3) and np.isfinite(ref).all() and eng.range_status() is False
    rc, got = _dense_call(eng, loud, lst)
    assert rc == _lib.ERANGE and eng.range_status(clear=True) is True
    moved = (_bits(got) != _bits(ref)).any(axis=2)
    assert not (moved & ~touched).any(), f"windows {np.argwhere(moved & ~touched)[:8].tolist()} do not hold the loud row and changed"
    with pytest.raises(OwwRangeError):
        eng.bank_score_stats(loud, lst)
    assert eng.range_status(clear=True) is True
    st = eng.bank_score_stats(clean, lst)
    assert np.array_equal(st["max"], ref.max(axis=1)) and eng.range_status() is False


# ------------------------------------------------------------------------------------------------ E. conv19 without fixed heads
def test_conv19_on_a_bank_only_handle(bank_eng):
    """Nobody reads the offender's embedding (no fixed head, no subscription): either the flag is up or the row itself says so."""
    eng, heads, ids = bank_eng
    off = 3
    sub = np.full((8, 2), -1, np.int32)
    sub[:, 0] = ids["bank64"]
    sub[off] = -1
    pcm = W.synthetic_pcm(8, 1280 * (WARM + 1), seed=43)
    eng.reset()
    eng.subscribe(np.arange(8), sub)
    for t in range(WARM):
        eng.step(pcm[:, 1280 * t:1280 * (t + 1)])
    rec = eng.export_state([off])[0]
    eng.import_state([off], RG.poison(rec, "hist19")[None])
    _, up = _flagged(lambda: eng.step(pcm[:, 1280 * WARM:]))
    up = eng.range_status(clear=True) or up
    newest = eng.get_features(off, 1)[0]
    print(f"\nconv19, bank-only handle, offender unsubscribed: flag {'up' if up else 'down'}, newest feature row "
          f"{'non-finite' if not np.isfinite(newest).all() else 'finite'}")
    assert up or not np.isfinite(newest).all(), "conv19 swallowed an out-of-range history: finite embedding, flag down"
    eng.subscribe(np.arange(8), np.full_like(sub, -1))
    eng.reset()
