"""Bulk clip embedding -- oww_embed_clips and oww_embed (openwakeword_amd/csrc/owwhip.hip) -- against float64 and against itself.

The path has code no streaming step runs: owk::mel_kernel in clip mode at 76 frames and more, clamp_transform_rows_kernel with one
floor per clip, a window walk that hands run_cnn a caller's mel pointer, a row stride and a NEGATIVE offset on step 0 (every clip but
the first reads its neighbour's last four rows as lead-in), nine warm-up steps that flush the borrowed streams, park_state around it
all and a 2-D gather of the output.  Two stages, each with the budget the project already has (tests/clip_ref.py; admitted for these
clips by tests/test_clip_budget_cpu.py):

  (a) oww_mel_clips against mel_budget's level-aware budget, at the six clip lengths;
  (b) oww_embed_clips against the float64 CNN of the windows of the DEVICE'S OWN mel rows, every window within cnn_budget.T of its
      max |e64|, every kernel family; and end to end against float64 within the existing 2e-4 max(1, |e|);
  (c) bit-exact invariances: clip order, batch size, clip length, B around S / 8 / Spad / the mel grid, what the borrowed streams
      held, host or device buffers, the feature ring's length;
  (d) oww_embed on 76 + 8 j rows, and its refusal of anything else.

Each test prints its worst figure (DESIGN.md section 5.26 records them)."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import clip_ref as CR
import cnn_budget as CB
import mel_budget as MB
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine

pytestmark = pytest.mark.gpu
FAMILIES = (3, 1, 2, 0)
RR = (3, 1)                       # the register-resident families: every invariance; 2 and 0 (LDS-tiled): clip order and length
S = 13
LENGTHS = tuple(CR.LENGTHS)
E2E = 2e-4                        # the existing end-to-end bound, x max(1, |e|)


@functools.lru_cache(maxsize=None)
def _emb():
    return W.synthetic_embedding(1234)


def _engine(n_streams=S, family=3, heads=None, **kw):
    return StreamEngine(n_streams, heads or {"alexa": W.synthetic_head("alexa", 1234)}, _emb(), use_mfma=family, **kw)


@pytest.fixture(scope="module")
def engines():
    """One 13-stream handle per kernel family, made on first use."""
    made = {}

    def get(family):
        if family not in made:
            made[family] = _engine(S, family)
        return made[family]
    yield get
    for e in made.values():
        assert e.range_status() is False
        e.close()


# ------------------------------------------------------------------------------------------------ float64, computed once
@functools.lru_cache(maxsize=None)
def _mel_ref(n):
    return CR.mel_ref(CR.clips(n))


@functools.lru_cache(maxsize=None)
def _e2e64(n):
    e = CR.clip_embeddings64(CR.clips(n), _emb())
    e.setflags(write=False)
    return e


_CNN64 = {}


def _cnn64_of(rows32):
    """float64 embeddings [W, 96] of the windows of ONE clip's fp32 mel rows [F, 32]; one evaluation per distinct set of rows (the mel
    kernel is the same in every family, so the families share them)."""
    rows32 = np.ascontiguousarray(rows32, dtype=np.float32)
    key = (rows32.shape, hashlib.sha1(rows32.tobytes()).hexdigest())
    if key not in _CNN64:
        e = CR.cnn64(CR.windows(rows32), _emb())
        e.setflags(write=False)
        _CNN64[key] = e
    return _CNN64[key]


def _walk_fraction(got, db32):
    """got [B, W, 96] against the float64 CNN of the device's own rows (dB, clamped: oww_mel_clips) -> worst fraction of T per clip."""
    rows = CR.mel_units32(db32)
    return np.array([float(CB.ratios(got[b], _cnn64_of(rows[b])).max()) / CB.T for b in range(got.shape[0])])


def _eq(a, b, msg):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, f"{msg}: shapes {a.shape} and {b.shape}"
    if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
        raise AssertionError(f"{msg}: {len(bad)} of {a.size} values differ, first at {bad[:4].tolist()}, largest |a - b| = {np.abs(a - b).max():.3e}")


def _cycled(B, n):
    """int16 [B, n]: the mixed batch repeated (clip b is ORDER[b % 7])."""
    return np.ascontiguousarray(CR.clips(n)[np.arange(B) % len(CR.ORDER)])


# ------------------------------------------------------------------------------------------------ (a) clip-mode mel
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("family", [3, 0])
def test_clip_mode_mel_at_clip_lengths(engines, family, n):
    x, ref = CR.clips(n), _mel_ref(n)
    got = engines(family).mel_clips(x)
    assert got.shape == ref.clamped.shape == (7, CR.LENGTHS[n][0], 32) and np.isfinite(got).all()
    r = {name: MB.worst_ratio(got[b:b + 1], MB.Ref(*(a[b:b + 1] for a in ref))) for b, name in enumerate(CR.ORDER)}
    print(f"\nmel_clips, family {family}, n = {n}: worst |device - float64| / budget " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ (b) the walk and the CNN
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("family", FAMILIES)
def test_walk_and_cnn_meet_the_budget_on_the_devices_own_rows(engines, family, n):
    eng, x = engines(family), CR.clips(n)
    got = eng.embed_clips(x)
    assert got.shape == (7, CR.LENGTHS[n][1], 96) and np.isfinite(got).all()
    f = _walk_fraction(got, eng.mel_clips(x))
    e64 = _e2e64(n)
    e2e = np.abs(got - e64) / np.maximum(1.0, np.abs(e64))
    print(f"\nembed_clips, family {family}, n = {n}: worst window error / (T max |e64|) " + ", ".join(f"{k} {v:.3f}" for k, v in zip(CR.ORDER, f))
          + f"; end to end {e2e.max():.2e} (bound {E2E:.0e})")
    assert f.max() <= 1.0, f"over the CNN budget: {dict(zip(CR.ORDER, f.round(2)))}"
    assert e2e.max() <= E2E


# ------------------------------------------------------------------------------------------------ (c) bit-exact invariances
@pytest.mark.parametrize("family", FAMILIES)
def test_clip_order_batch_size_and_length_leave_the_bits_alone(engines, family):
    """Every clip of the mixed batch: alone, in the reversed batch (where lsb follows square_fs as zeros does in the forward one), and,
    for the clips whose maximum is the same at both lengths, its first windows cut from the 35,072-sample clip."""
    eng = engines(family)
    full = {n: eng.embed_clips(CR.clips(n)) for n in (CR.N_TWO, CR.N_LONG)}
    for n, got in full.items():
        x = CR.clips(n)
        rev = eng.embed_clips(np.ascontiguousarray(x[::-1]))
        for b, name in enumerate(CR.ORDER):
            _eq(eng.embed_clips(x[b:b + 1])[0], got[b], f"family {family}, n = {n}: {name} alone and in the batch")
            _eq(rev[len(CR.ORDER) - 1 - b], got[b], f"family {family}, n = {n}: {name} in the reversed batch")
    same = CR.same_floor_at(CR.N_TWO, CR.N_LONG)
    assert "noise3000" in same and "square_fs" in same
    for name in same:
        b = CR.ORDER.index(name)
        _eq(full[CR.N_LONG][b, :2], full[CR.N_TWO][b], f"family {family}: {name}, the first two windows of the long clip")


@pytest.mark.parametrize("family", RR)
def test_batch_sizes_around_8_S_and_Spad(family):
    """S = 3 (Spad 32): B = 1, 7, 8, 9 and 32, so B > S and B = Spad; S = 13: B = 13.  Every clip carries its single-clip bits."""
    for n_streams, sizes in ((3, (7, 8, 9, 32)), (13, (13,))):
        eng = _engine(n_streams, family)
        try:
            assert eng.n_streams_padded == 32
            x = CR.clips(CR.N_TWO)
            alone = [eng.embed_clips(x[b:b + 1])[0] for b in range(len(CR.ORDER))]            # B = 1
            for B in sizes:
                got = eng.embed_clips(_cycled(B, CR.N_TWO))
                assert got.shape == (B, 2, 96)
                for b in range(B):
                    _eq(got[b], alone[b % 7], f"family {family}, S = {n_streams}, B = {B}: clip {b} ({CR.ORDER[b % 7]})")
            assert eng.range_status() is False
        finally:
            eng.close()


@pytest.mark.parametrize("family", RR)
def test_more_clips_than_the_mel_grid(family):
    """B = 1,544 on S = 1,544 at 12,512 samples: the mel kernel's persistent grid has 1,536 workgroups and loops.  Clips 0, 1,535,
    1,536 and 1,543 carry their single-clip bits and meet the CNN budget on their own rows; every clip carries the bits of the first
    clip with its samples."""
    B, n, probe = 1544, CR.N_MIN, (0, 1535, 1536, 1543)
    eng = _engine(B, family)
    try:
        x = _cycled(B, n)
        got = eng.embed_clips(x)
        assert got.shape == (B, 1, 96) and np.isfinite(got).all()
        for b in probe:
            _eq(eng.embed_clips(x[b:b + 1])[0], got[b], f"family {family}: clip {b} of {B} and alone")
        _eq(got, got[np.arange(B) % 7], f"family {family}: clips b and b % 7 hold the same samples")
        f = _walk_fraction(got[list(probe)], eng.mel_clips(x[list(probe)]))
        print(f"\nB = {B}, family {family}: worst window error / (T max |e64|) of clips {probe}: " + ", ".join(f"{v:.3f}" for v in f))
        assert f.max() <= 1.0
        assert eng.range_status() is False
    finally:
        eng.close()


def _dirty(eng, how):
    """The four states a borrowed stream can be in: fresh, seven steps of full-scale uniform noise, seven steps of square_fs, and
    streams [0, 8) noisy with the rest fresh."""
    eng.reset()
    if how == "reset":
        return
    if how == "square":
        pcm = np.repeat(CR.clip("square_fs", 7 * 1280)[None], S, axis=0)
    else:
        pcm = np.random.default_rng(41).integers(-32768, 32768, (S, 7 * 1280)).astype(np.int16)
    for t in range(7):
        eng.step(np.ascontiguousarray(pcm[:, 1280 * t:1280 * (t + 1)]))
    if how == "first8":
        eng.reset(list(range(8, S)))


@pytest.mark.parametrize("family", RR)
def test_what_the_borrowed_streams_held_changes_nothing(family):
    """Four handles in four states return the same embeddings, and each then continues its own streaming bit for bit like a twin with
    the same history that never embedded."""
    x = CR.clips(CR.N_LONG)
    after = W.synthetic_pcm(S, 2 * 1280, seed=43)
    first = None
    for how in ("reset", "noise", "square", "first8"):
        a, twin = _engine(S, family), _engine(S, family)
        try:
            _dirty(a, how); _dirty(twin, how)
            got = a.embed_clips(x)
            if first is None:
                first = got
                assert _walk_fraction(got, a.mel_clips(x)).max() <= 1.0
            _eq(got, first, f"family {family}: embeddings from a handle in state '{how}' and from one just reset")
            assert np.array_equal(a.export_state(range(S)), twin.export_state(range(S))), f"family {family}, state '{how}': the state records after the call"
            for t in range(2):
                chunk = np.ascontiguousarray(after[:, 1280 * t:1280 * (t + 1)])
                _eq(a.step(chunk), twin.step(chunk), f"family {family}, state '{how}': scores of step {t} after the call")
            for s in range(S):
                _eq(a.get_features(s, 16), twin.get_features(s, 16), f"family {family}, state '{how}': feature ring of stream {s}")
            assert a.range_status() is False
        finally:
            a.close(); twin.close()


@pytest.mark.parametrize("n", [CR.N_MIN, CR.N_LONG])
@pytest.mark.parametrize("family", RR)
def test_device_buffers_give_the_host_buffers_bits(engines, family, n):
    """embed_clips_device on torch device tensors: one window, and 18 (the 2-D gather's destination pitch is 18 rows)."""
    eng, x = engines(family), CR.clips(n)
    want = eng.embed_clips(x)
    d_x = torch.from_numpy(np.array(x)).to("cuda:0")                    # (a writable copy: the clips are read-only)
    d_out = torch.full((x.shape[0], CR.LENGTHS[n][1], 96), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    eng.embed_clips_device(d_x.data_ptr(), x.shape[0], n, d_out.data_ptr())
    torch.cuda.synchronize()
    _eq(d_out.cpu().numpy(), want, f"family {family}, n = {n}: device and host buffers")


@pytest.mark.parametrize("family", RR)
def test_a_longer_feature_ring_changes_nothing(engines, family):
    """18 windows through a 16-row ring (it wraps) and through a 34-row ring (an rnn head with T = 34): the same embeddings."""
    heads = {"alexa": W.synthetic_head("alexa", 1234), "rnn5": W.synthetic_head("rnn5", 62, kind="rnn", n_out=5, T=34)}
    x = CR.clips(CR.N_LONG)
    assert engines(family).feature_ring == 16
    long_ring = _engine(S, family, heads=heads)
    try:
        assert long_ring.feature_ring == 34
        _eq(long_ring.embed_clips(x), engines(family).embed_clips(x), f"family {family}: 34-row and 16-row feature ring")
    finally:
        long_ring.close()


# ------------------------------------------------------------------------------------------------ (d) oww_embed
@pytest.mark.parametrize("family", FAMILIES)
def test_embed_on_whole_windows(engines, family):
    """76, 84 and 212 of the device's own rows of the 35,072-sample clips: within the CNN budget per window, and the windows
    oww_embed_clips returns for them within the existing 2e-5."""
    eng, x = engines(family), CR.clips(CR.N_LONG)
    rows = CR.mel_units32(eng.mel_clips(x))
    clips = eng.embed_clips(x)
    for r in (76, 84, 212):
        got = eng.embed(np.ascontiguousarray(rows[:, :r]))
        nw = (r - 76) // 8 + 1
        assert got.shape == (7, nw, 96)
        f = np.array([float(CB.ratios(got[b], _cnn64_of(rows[b])[:nw]).max()) / CB.T for b in range(7)])
        d = float(np.abs(got - clips[:, :nw]).max())
        print(f"\nembed, family {family}, {r} rows: worst window error / (T max |e64|) {f.max():.3f}; largest |embed - embed_clips| {d:.2e}")
        assert f.max() <= 1.0
        np.testing.assert_allclose(got, clips[:, :nw], rtol=0, atol=2e-5)


@pytest.mark.parametrize("rows", [75, 77, 83])
def test_embed_refuses_partial_windows(engines, rows):
    with pytest.raises(ValueError):
        engines(3).embed(np.full((2, rows, 32), 2.0, np.float32))
