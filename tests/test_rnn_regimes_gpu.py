"""The recurrent head kernel (owk::heads_rnn_kernel) against the FLOAT64 oracle across gate regimes and call routes (tests/rnn_regimes.py;
the CPU tier that admits the cases, holds the oracle to torch.nn.LSTM and shows what each case catches is test_rnn_regimes_cpu.py).
1. every admitted (regime, T, n_out) through StreamEngine.head() at 37 streams, three regimes in all three kernel families;
2. a stream's bits do not depend on its slot in the wave of two, nor on its neighbour;
3. calls of several chunks, the sliced long call included, against the oracle model: the kernel's max-combining store;
4. the same between masked one-chunk steps.
Contract of 1: every score finite, within TOL_SCORE of O.head_stage(..., float64), the range flag down, softmax rows summing to one,
the dead-ReLU head exactly 1/8.  pytest -m gpu -s prints the worst error of every regime; DESIGN.md 5.36 records them."""
import ctypes as C
import functools

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine

import rnn_regimes as R
from rnn_regimes import TOL_SCORE
from head_windows import check_scores

pytestmark = pytest.mark.gpu
SUM_TO_ONE = 1e-5                    # a softmax row's sum (tests/test_rnn_heads.py, tests/test_head_windows_gpu.py)
WORST = {}                           # (family, regime) -> worst |score - float64| seen by test 1, for the table printed at the end


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


def _raw(e):
    out = np.empty((e.n_streams, e.n_labels), np.float32)
    _lib.check(e._lib.oww_get_raw(e._h, out.ctypes.data_as(C.c_void_p)))
    return out


# ------------------------------------------------------------------------------------------------ 1. regimes through head()
_HANDLES = [(fam, i) for fam in (3, 1, 0) for i in range(len(R.handles(fam)))]


@pytest.mark.parametrize("fam,i", _HANDLES, ids=[f"mfma{fam}-T{R.handles(fam)[i][0]}-{i}" for fam, i in _HANDLES])
def test_regimes_match_float64(fam, i):
    """One handle of the case table: its heads committed side by side (the commit self-test must take every admitted regime: a
    refusal raises here, with the library's message), each scored on windows(T) at 37 streams -- 19 waves, the last with one stream."""
    T, hnd = R.handles(fam)[i]
    eng = StreamEngine(R.N_ROWS, R.handle_heads(hnd), _emb(), use_mfma=fam)
    try:
        for c in hnd:
            got = eng.head(R.name_of(c), R.windows(T))
            worst = [0.0]
            check_scores(f"{R.name_of(c)} use_mfma={fam}", got, R.want(c), eng.range_status(clear=True), worst)
            WORST[fam, c[0]] = max(WORST.get((fam, c[0]), 0.0), worst[0])
            if c[2] > 1:
                np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=SUM_TO_ONE, err_msg=R.name_of(c))
            if c[0] == "relu_dead":
                exact = np.float32(0.125) if c[2] == 8 else np.float32(0.0)
                assert got.dtype == np.float32 and np.array_equal(got, np.full_like(got, exact)), f"{R.name_of(c)}: not {exact} bit for bit"
    finally:
        eng.close()


def test_regimes_worst_error_table():
    """Prints what test_regimes_match_float64 measured, per regime (run after it in file order; on its own it has nothing to print)."""
    print("\nregime        use_mfma   worst |score - float64|   fraction of TOL_SCORE")
    for (fam, r), v in sorted(WORST.items(), key=lambda kv: (list(R.REGIMES).index(kv[0][1]), -kv[0][0])):
        print(f"{r:12s}  {fam:8d}   {v:.2e}                  {v / TOL_SCORE:.3f}")
        assert v <= TOL_SCORE
    if len({r for _f, r in WORST}) == len({c[0] for c in R.ADMITTED}):
        assert {r for f, r in WORST if f != 3} == set(R.FAMILY_REGIMES)


# ------------------------------------------------------------------------------------------------ 2. slot and neighbour invariance
@pytest.mark.parametrize("T", R.SLOT_T)
def test_a_streams_bits_do_not_depend_on_slot_or_neighbour(T):
    """Six rows of windows(T) -- the zero and the loud row among them -- each scored alone in a handle of one stream, as stream 0 of
    two, as stream 1 of two beside the loud row, and as stream 36 of 37 (the last wave's only stream, its second slot clamped to the
    same stream): the same bits in all four places, for seed1, remember and gates_x4 with one and eight outputs."""
    cases = [(r, T, n) for r in R.FAMILY_REGIMES for n in R.N_OUTS]
    assert sum(c[2] for c in cases) <= R.MAX_LABELS
    heads = {R.name_of(c): R.head(c) for c in cases}
    ft = R.windows(T)
    fill = np.random.default_rng(7).normal(0.0, 1.0, (R.N_ROWS, T, 96)).astype(np.float32)
    got = {}
    for S in (1, 2, R.N_ROWS):
        eng = StreamEngine(S, heads, _emb())
        try:
            for c in cases:
                n = R.name_of(c)
                for row in R.SLOT_ROWS:
                    if S == 1:
                        got[n, row, "alone"] = eng.head(n, ft[row:row + 1])[0]
                    elif S == 2:
                        got[n, row, "slot 0 of 2"] = eng.head(n, np.stack([ft[row], fill[0]]))[0]
                        got[n, row, "slot 1 beside the loud row"] = eng.head(n, np.stack([ft[R.LOUD_ROW], ft[row]]))[1]
                    else:
                        batch = fill.copy()
                        batch[R.N_ROWS - 1] = ft[row]
                        got[n, row, "stream 36 of 37"] = eng.head(n, batch)[R.N_ROWS - 1]
            assert eng.range_status() is False
        finally:
            eng.close()
    for c in cases:
        n = R.name_of(c)
        for row in R.SLOT_ROWS:
            ref = got[n, row, "alone"]
            assert np.isfinite(ref).all() and np.abs(ref - R.want(c)[row]).max() <= TOL_SCORE, (n, row)
            for place in ("slot 0 of 2", "slot 1 beside the loud row", "stream 36 of 37"):
                assert np.array_equal(ref.view(np.uint32), got[n, row, place].view(np.uint32)), \
                    f"{n} row {row}: {place} gives {got[n, row, place]} against {ref} alone"
        rows = np.stack([got[R.name_of(c), row, "alone"] for row in R.SLOT_ROWS])
        assert np.ptp(rows, axis=0).max() > 0.0, f"{n}: the six rows score the same"


# ------------------------------------------------------------------------------------------------ 3. and 4. call routes
def _run_calls(e, schedule):
    """The schedule on a handle whose first CALL_ORACLE streams start from the oracle models' feature rings -> per call (scores, raw)."""
    inits, calls = R.oracle_calls(schedule)
    assert e.feature_ring == inits[0].shape[0]
    for s in range(R.CALL_ORACLE):
        e.reset([s], inits[s])
    pcm = R.call_pcm(sum(k for k, _ in schedule))
    out = []
    for c in calls:
        x = np.ascontiguousarray(pcm[:, 1280 * c["at"]:1280 * (c["at"] + c["k"])])
        if c["off"]:
            on = np.ones(R.CALL_S, np.uint8)
            on[list(c["off"])] = 0
            scores = e.step_masked(x, on)
        else:
            scores = e.step(x)
        out.append((scores.copy(), _raw(e)))
    return calls, out


def _check_against_oracle(calls, out, label):
    worst = worst_raw = 0.0
    for i, (c, (scores, raw)) in enumerate(zip(calls, out)):
        took_part = [s for s in range(R.CALL_ORACLE) if s not in c["off"]]
        assert np.isfinite(scores).all() and np.isfinite(raw).all()
        err = np.abs(scores[took_part].astype(np.float64) - c["scores"][took_part])
        worst = max(worst, float(err.max()))
        assert err.max() <= TOL_SCORE, f"{label} call {i} ({c['k']} chunks): {err.max():.3e} from the oracle model at {np.unravel_index(int(err.argmax()), err.shape)}"
        # the raw scores are the maximum over the call's chunks of what the oracle's heads returned chunk by chunk
        err = np.abs(raw[took_part].astype(np.float64) - c["chunk_raw"][took_part].max(axis=1))
        worst_raw = max(worst_raw, float(err.max()))
        assert err.max() <= TOL_SCORE, f"{label} call {i} ({c['k']} chunks): raw scores {err.max():.3e} from the maximum over the chunks"
    print(f"\n{label}: worst |score - oracle model| = {worst:.2e}, raw {worst_raw:.2e}")


def _assert_early_maxima(calls):
    share, n = R.early_max_share(calls)
    print(f"\nthe maximum sits before the last chunk, by more than {R.EARLY_MARGIN}, in {share:.3f} of {n} (call, stream, column) triples")
    assert share >= R.EARLY_SHARE and n > 0


@pytest.mark.parametrize("use_mfma", [3, 1])
def test_multi_chunk_and_sliced_calls_match_the_oracle_model(use_mfma):
    """max_chunks = 3; calls of 1, 2, 3, 5 (sliced: more than max_chunks), 1 and 3 chunks after a five-call warm-up (the reference
    returns zeros for its first five predictions).  Every chunk after a call's first reaches the kernel's max-combining store
    (store_raw with accumulate_max; step_chunk(..., !first)); the oracle model takes the maximum over the call's chunks too
    (model.py:287-298).  Non-vacuity, on the oracle alone: often enough the maximum is NOT the last chunk's value."""
    assert max(R.CALL_SIZES) > R.CALL_MAX_CHUNKS
    e = StreamEngine(R.CALL_S, R.call_heads(), R.call_emb(), max_chunks=R.CALL_MAX_CHUNKS, use_mfma=use_mfma)
    try:
        assert e.n_labels == len(R.CALL_LABELS)
        calls, out = _run_calls(e, R.PLAIN_CALLS)
        assert e.range_status() is False
    finally:
        e.close()
    _assert_early_maxima(calls)
    _check_against_oracle(calls, out, f"use_mfma={use_mfma}")
    assert (out[-1][0][:R.CALL_ORACLE, :R.CALL_RNN_COLS] > 0).all()


def test_multi_chunk_calls_between_masked_steps():
    """A masked one-chunk step between calls of several chunks.  A stream that sits the masked step out keeps its raw and its
    post-processed recurrent columns bit for bit (the kernel's store skips it), and its next multi-chunk call matches the oracle model,
    which simply was not called for that chunk.  With a recurrent head the host mask always takes the full launches -- every stream's
    wave runs, the stores of those that sit out are dropped -- because build_active_lists returns -1 when rnn_nets is not empty
    (owwhip.hip).  No counter tells a list launch from a full one: kernel_times() counts one "heads" entry per step either way, so
    that route is stated here, not asserted; what is asserted is what it must deliver."""
    e = StreamEngine(R.CALL_S, R.call_heads(), R.call_emb(), max_chunks=R.CALL_MAX_CHUNKS)
    try:
        calls, out = _run_calls(e, R.MASKED_CALLS)
        assert e.range_status() is False
    finally:
        e.close()
    _assert_early_maxima(calls)
    _check_against_oracle(calls, out, "masked schedule")
    masked = [i for i, c in enumerate(calls) if c["off"]]
    assert len(masked) == 2 and all(calls[i - 1]["k"] > 1 and calls[i + 1]["k"] > 1 for i in masked)
    for i in masked:
        off = sorted(calls[i]["off"])
        on = [s for s in range(R.CALL_S) if s not in off]
        for what, k in (("post-processed", 0), ("raw", 1)):
            before, after = out[i - 1][k][:, :R.CALL_RNN_COLS], out[i][k][:, :R.CALL_RNN_COLS]
            assert np.array_equal(before[off].view(np.uint32), after[off].view(np.uint32)), f"call {i}: a stream that sat out changed its {what} scores"
            assert (before[on] != after[on]).any(axis=1).all(), f"call {i}: a stream that took part kept its {what} scores"
