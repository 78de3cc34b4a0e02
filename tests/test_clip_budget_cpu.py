"""CPU tier of the bulk clip-embedding comparison (tests/clip_ref.py): the two budgets the device tier uses admit these clips at clip
length, the faults the device tier has to see move the float64 chain far beyond the CNN budget, and the step arithmetic of
oww_embed_clips never reads past a clip's last row."""
import functools

import numpy as np
import pytest

import clip_ref as CR
import cnn_budget as CB
import mel_budget as MB
from oracle import oww_oracle as O
from openwakeword_amd import weights as W

SEEN = 100 * CB.T                # a fault has to move a window by 1e-3 of its largest float64 value


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


@functools.lru_cache(maxsize=None)
def _spec(name, n):
    s = CR.spec64(CR.clip(name, n))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _e64(name, n):
    return CR.cnn64(CR.windows(_spec(name, n)), _emb())


# ------------------------------------------------------------------------------------------------------------ clips and lengths
def test_clips_are_fixed_int16_and_ordered():
    x = CR.clips()
    assert x.shape == (7, CR.N) and x.dtype == np.int16 and not x.flags.writeable
    i = {name: k for k, name in enumerate(CR.ORDER)}
    assert i["zeros"] == i["square_fs"] + 1 and i["lsb"] == i["square_fs"] - 1      # square_fs precedes zeros; reversed, it precedes lsb
    assert set(np.unique(CR.clip("lsb"))) == {-1, 0, 1} and not CR.clip("zeros").any()
    sq = CR.clip("square_fs")
    assert set(np.unique(sq)) == {-32768, 32767} and np.array_equal(sq[:-16], sq[16:]) and sq[0] != sq[8]
    for n in CR.LENGTHS:
        tail, head = CR.clip("loud_tail", n).astype(np.int64), CR.clip("loud_head", n).astype(np.int64)
        assert np.abs(tail[:n - CR.LOUD]).max() <= 40 < 12000 < np.abs(tail[n - CR.LOUD:]).max()
        assert np.abs(head[CR.LOUD:]).max() <= 40 < 12000 < np.abs(head[:CR.LOUD]).max()
        for name in ("noise3000", "speechlike", "lsb", "square_fs"):
            assert np.array_equal(CR.clip(name, n), CR.clip(name)[:n])
    assert np.abs(CR.clip("speechlike").astype(np.int64)).max() < 20000


def test_length_table():
    for n, (F, nw) in CR.LENGTHS.items():
        assert CR.n_frames(n) == O.n_mel_frames(n) == F and CR.n_windows(F) == nw
        assert CR.windows(np.zeros((F, 32))).shape == (nw, 76, 32)
    assert CR.n_frames(12511) == 75 and CR.n_windows(CR.n_frames(13791)) == 1
    assert CR.LENGTHS[CR.N_LONG][1] > 16                                              # more windows than the default feature ring


def test_loud_ends_set_the_floor_of_the_far_window():
    """loud_tail: window 0 holds no loud frame, and most of it lies under a floor the clip's end sets; loud_head: the same for the last
    window."""
    for name, w in (("loud_tail", 0), ("loud_head", -1)):
        ref = CR.mel_ref(CR.clip(name, CR.N_TWO))
        rows = slice(0, 76) if w == 0 else slice(8, 84)
        assert ref.u[0, rows].max() < ref.u.max() - 30.0
        assert (ref.u[0, rows] < ref.floor[0]).mean() > 0.5


def test_same_floor_clips():
    """The clips whose first windows must be bit-identical at 13,792 and 35,072 samples are chosen from float64 alone."""
    names = CR.same_floor_at(CR.N_TWO, CR.N_LONG)
    print(f"\nsame per-clip maximum at {CR.N_TWO} and {CR.N_LONG} samples: {names}")
    assert "noise3000" in names and "square_fs" in names and "loud_tail" not in names and "speechlike" not in names


def test_references_agree_with_the_oracle_front_end():
    """clip_embeddings64 is OracleAudioFeatures.clip_embeddings without the casts: the two agree to fp32 round-off on a single clip;
    mel_units32 is / 10 + 2 to one fp32 ulp; mel_ref's clamped rows are mel_stage(float64) per clip."""
    emb = _emb()
    x = CR.clips(CR.N_TWO, ("noise3000", "loud_tail"))
    want = np.stack([np.asarray(O.OracleAudioFeatures(emb, init_noise=np.zeros(64000, np.int16)).clip_embeddings(c)).reshape(-1, 96) for c in x])
    got = CR.clip_embeddings64(x, emb)
    assert got.shape == want.shape == (2, 2, 96) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5 * np.abs(got).max())
    ref = CR.mel_ref(x)
    for b in range(2):
        np.testing.assert_allclose(ref.clamped[b], O.mel_stage(x[b], np.float64)[0, 0], rtol=0, atol=1e-9)
    db = ref.clamped.astype(np.float32)
    np.testing.assert_allclose(CR.mel_units32(db), db.astype(np.float64) / 10 + 2, rtol=0, atol=6e-7)
    assert np.array_equal(CR.mel_units32(db, ref.floor[0] + 20), CR.mel_units32(np.maximum(db, np.float32(ref.floor[0] + 20))))


# --------------------------------------------------------------------------------------------------------------------- admission
@pytest.mark.parametrize("n", list(CR.LENGTHS))
def test_both_budgets_admit_the_clips(n):
    """The fp32 oracle against float64 at clip length: its mel rows inside T0 + (T1 / 4) 10^((D - 80) / 20) -- E32 of the mel budget
    was taken at 6,400 samples or fewer -- and its CNN, on its own mel rows, inside cnn_budget.E32 of every window's max |e64|."""
    emb, worst_mel, worst_cnn = _emb(), {}, {}
    for name in CR.ORDER:
        x = CR.clip(name, n)
        ref = MB.reference(x)
        u, Rf = MB._unclamped(x[None], ref.u.shape[1])
        D = np.maximum(Rf[:, :u.shape[1], None] - u, 0.0)               # to the value's own frame: the oracle transforms frames alone
        got = O.mel_stage(x.astype(np.float32), np.float32)[:, 0]
        err = np.abs(got.astype(np.float64) - ref.clamped)
        worst_mel[name] = float((err / (MB.T0 + (MB.T1 / 4) * 10.0 ** ((D - 80.0) / 20.0))).max())
        rows = CR.windows(O.mel_transform(got[0]))
        assert rows.dtype == np.float32 and rows.shape[0] == CR.LENGTHS[n][1]
        e32 = O.embedding_stage(rows[..., None], emb, np.float32).reshape(-1, 96)
        worst_cnn[name] = float(CB.ratios(e32, CR.cnn64(rows, emb)).max())
    print(f"\nn = {n}: fp32 oracle, mel error / (T0 + E32 ...) and CNN error / max |e64| per clip")
    for name in CR.ORDER:
        print(f"    {name:12s} {worst_mel[name]:.3f}   {worst_cnn[name]:.2e}")
    assert max(worst_mel.values()) <= 1.0
    assert max(worst_cnn.values()) <= CB.E32


# ------------------------------------------------------------------------------------------- fault sensitivity, float64 chain
@pytest.mark.parametrize("name", CR.SHIFT_CLIPS)
def test_a_walk_off_by_one_row_is_seen(name):
    """Every window of the 35,072-sample clip, cut one mel row late ((it * 8 - 3) * 32) and one row early: at least 100 T of the
    window's maximum.  (zeros and square_fs are stationary and move by 0; loud_tail and loud_head move by 3.7e-5 in their quiet middle:
    those four are not in this condition.)"""
    s, e = _spec(name, CR.N_LONG), _e64(name, CR.N_LONG)
    late = CR.window_movement(CR.cnn64(CR.windows(s[1:]), _emb()), e)
    early = CR.window_movement(CR.cnn64(CR.windows(s[7:]), _emb())[:17], e[1:])
    assert late.shape == (18,) and early.shape == (17,)
    print(f"\n{name}: least movement of a window, walk one row late {late.min():.2e}, one row early {early.min():.2e}")
    assert min(late.min(), early.min()) >= SEEN


def test_clips_outside_the_shift_condition():
    for name in ("zeros", "square_fs"):
        s = _spec(name, CR.N_LONG)
        assert float(np.ptp(s, axis=0).max()) < 1e-9, f"{name} is stationary"
    for name in ("loud_tail", "loud_head"):
        s, e = _spec(name, CR.N_LONG), _e64(name, CR.N_LONG)
        m = CR.window_movement(CR.cnn64(CR.windows(s[1:]), _emb()), e).min()
        print(f"\n{name}: least movement of a window, walk one row late {m:.2e}")
        assert m < SEEN


def test_a_call_wide_floor_is_seen():
    """[square_fs, lsb, zeros, loud_tail] at 13,792 samples with one floor for the call (clamp_transform_rows_kernel reading smax[0]:
    square_fs is clip 0 and the loudest): every window of the three quiet clips moves by at least 100 T."""
    emb = _emb()
    db = [O.mel_stage(CR.clip(name, CR.N_TWO), np.float64)[0, 0] for name in CR.FLOOR_BATCH]
    assert max(d.max() for d in db) == db[0].max()
    floor = db[0].max() - O.TOP_DB
    moved = {}
    for name, d in zip(CR.FLOOR_BATCH[1:], db[1:]):
        wrong = CR.cnn64(CR.windows(O.mel_transform(np.maximum(d, floor))), emb)
        moved[name] = CR.window_movement(wrong, _e64(name, CR.N_TWO))
        assert moved[name].shape == (2,)
    print("\ncall-wide floor, movement per window: " + ", ".join(f"{k} {v.min():.2f} .. {v.max():.2f}" for k, v in moved.items()))
    assert min(v.min() for v in moved.values()) >= SEEN


@pytest.mark.parametrize("n", [CR.N_MIN, CR.N_LONG])
@pytest.mark.parametrize("name", ["zeros", "lsb"])
def test_a_leaking_lead_in_is_seen(name, n):
    """Window 0 computed from rows [-4, 72): square_fs's last four rows (in its own mel units) in front of the quiet clip."""
    s = np.concatenate([_spec("square_fs", n)[-4:], _spec(name, n)])
    m = float(CR.window_movement(CR.cnn64(s[None, :76], _emb()), _e64(name, n)[:1])[0])
    print(f"\n{name}, n = {n}: window 0 with square_fs's tail as its first four rows moves by {m:.2e}")
    assert m >= SEEN


def test_a_stale_first_window_is_seen():
    """Window 0 of noise3000 with its first two mel rows replaced by the all-ones reset history (a warm-up one step short of flushing
    the borrowed stream)."""
    s = _spec("noise3000", CR.N_MIN).copy()
    s[:2] = 1.0
    m = float(CR.window_movement(CR.cnn64(s[None, :76], _emb()), _e64("noise3000", CR.N_MIN))[0])
    print(f"\nnoise3000: window 0 with two rows of reset history moves by {m:.2e}")
    assert m >= SEEN


# ------------------------------------------------------------------------------------------------------------- step arithmetic
def test_step_arithmetic_of_embed_clips():
    """oww_embed_clips restated: n_out = (F - 76) / 8 + 1 windows, n_steps = 9 + n_out, step `it` reads rows [8 it - 4, 8 it + 4) and
    window j leaves after step 9 + j.  The last step never reads past row F, only step 0 reads in front of row 0 (four rows), and the
    rows consumed up to window j's step end exactly where the reference's window j ends."""
    for F in range(76, 401):
        n_out = (F - 76) // 8 + 1
        n_steps = 9 + n_out
        assert n_out == CR.n_windows(F) == CR.windows(np.zeros((F, 1))).shape[0]
        first = [8 * it - 4 for it in range(n_steps)]
        assert first[0] == -4 and first[1] == 4 and 8 * (n_steps - 1) + 4 <= F
        for j in range(n_out):
            assert 8 * (9 + j) + 4 == 8 * j + 76
        assert F - (8 * (n_steps - 1) + 4) == (F - 76) % 8                           # rows left unused
