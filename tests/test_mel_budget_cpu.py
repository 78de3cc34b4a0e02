"""CPU tier of the mel front end's float64 comparison (tests/mel_budget.py): the budget's constants against the fp32 reference's own
error, the conditions that keep the budget tight where it matters, and the product's mel tables against the oracle's."""
import functools

import numpy as np
import pytest

import mel_budget as MB
from oracle import oww_oracle as O
from openwakeword_amd import weights as W

LENGTHS = (1999, MB.N_CLIP, MB.N)


def test_regimes_are_fixed_int16_and_long_enough():
    regs = MB.regimes()
    assert len(regs) == 27 and tuple(regs) == MB.REGIMES
    for name, x in regs.items():
        assert x.dtype == np.int16 and x.shape == (MB.N,) and MB.N >= 1280 * 3 + 480, name
        assert not x.flags.writeable
    assert int(regs["dc_neg"].min()) == -32768 and int(regs["dc_pos"].max()) == 32767
    assert set(np.unique(regs["lsb"])) == {-1, 0, 1}
    assert int(np.abs(regs["last_one"].astype(np.int64)).sum()) == 1 and regs["last_one"][MB.N_CLIP - 1] == 1
    # the largest power any int16 input can reach stays far inside fp32: no regime may be refused
    assert (32768.0 * 200.0) ** 2 < 1e-20 * float(np.finfo(np.float32).max)


@functools.lru_cache(maxsize=None)
def _oracle_envelope(name):
    """(E, worst ratio): E = max (err - T0)+ * 10^((80 - D) / 20) of the fp32 oracle against float64 over LENGTHS, D taken to each
    value's OWN frame (the oracle transforms every frame alone; the pair coupling is the kernels'); ratio = err / (T0 + E32 * ...)."""
    E = ratio = 0.0
    for n in LENGTHS:
        pcm = MB.regimes()[name][:n]
        ref = MB.reference(pcm)
        u, Rf = MB._unclamped(pcm[None], ref.u.shape[1])
        assert (u <= Rf[:, :u.shape[1], None] + 1e-9).all(), "R_f bounds every mel value of its frame"
        D = np.maximum(Rf[:, :u.shape[1], None] - u, 0.0)
        got = O.mel_stage(pcm.astype(np.float32), np.float32)[:, 0].astype(np.float64)
        err = np.abs(got - ref.clamped)
        E = max(E, float((np.maximum(err - MB.T0, 0.0) * 10.0 ** ((80.0 - D) / 20.0)).max()))
        ratio = max(ratio, float((err / (MB.T0 + (MB.T1 / 4) * 10.0 ** ((D - 80.0) / 20.0))).max()))
    return E, ratio


def test_constants():
    assert MB.T0 == 2e-4 and MB.T1 == 4 * MB.E32
    assert set(MB.LEAKAGE) <= set(MB.REGIMES)


@pytest.mark.parametrize("name", MB.REGIMES)
def test_fp32_oracle_stays_inside_a_quarter_of_the_margin(name):
    """The reference's own fp32 arithmetic meets T0 + (T1 / 4) * 10^((D - 80) / 20) on every regime, the leakage ones included."""
    E, ratio = _oracle_envelope(name)
    print(f"\n{name}: fp32 oracle envelope {E:.3e} dB, worst error / (T0 + E32 ...) = {ratio:.3f}")
    assert ratio <= 1.0


def test_frozen_E32_is_the_measured_envelope():
    """E32 is neither stale nor loose: the envelope measured now lies in (0.6 E32, E32] (measured 1.27e-3 dB, frozen 1.5e-3)."""
    E = {name: _oracle_envelope(name)[0] for name in MB.REGIMES}
    worst = max(E, key=E.get)
    print(f"\nE32 measured {E[worst]:.3e} dB on {worst}; frozen {MB.E32:.3e}, T1 = {MB.T1:.3e}")
    assert 0.6 * MB.E32 < E[worst] <= MB.E32


def test_budget_is_tight_where_the_energy_is():
    """From float64 alone, over the 4,320-sample call of every regime: at least 40 % of all compared values have a budget <= 2 T0
    (measured 50 %), and every regime but the two leakage ones has at least 1 % such values (the least: tone3800, 3 %)."""
    tight = total = 0
    for name in MB.REGIMES:
        ref = MB.reference(MB.regimes()[name][:MB.N_CLIP])
        t = ref.budget <= 2 * MB.T0
        tight, total = tight + int(t.sum()), total + t.size
        if name not in MB.LEAKAGE:
            assert t.mean() >= 0.01, f"{name}: {t.mean():.3%} of the values have a budget <= 2 T0"
    print(f"\n{tight / total:.1%} of {total} compared values have a budget <= 2 T0")
    assert tight >= 0.40 * total


@pytest.mark.parametrize("name", MB.LEAKAGE)
def test_leakage_regimes_lie_far_below_their_frame_energy(name):
    """Float64 puts the call maximum 102 dB (5 kHz tone) and 127 dB (Nyquist alternation) below R: rows of pure leakage, D > 100."""
    ref = MB.reference(MB.regimes()[name][:MB.N_CLIP])
    assert ref.R.max() - ref.u.max() > 100.0
    assert (ref.R[:, :, None] - ref.u).min() > 100.0


def test_pairs_follow_the_kernel_frame_numbering():
    """R_pair is the larger R_f of frames (2j, 2j + 1); a last odd frame's partner is cut from the zero-extended input; a streaming
    call numbers its frames from the 480-sample tail, so its pairs lie three clip frames later."""
    x = MB.regimes()["onset_even"]
    ref = MB.reference(x[:MB.N_CLIP])
    _, Rf = MB._unclamped(x[None, :MB.N_CLIP], 24)
    assert np.array_equal(ref.R[0, 0::2], ref.R[0, 1::2])
    assert np.array_equal(ref.R[0, 0::2], np.maximum(Rf[0, 0::2], Rf[0, 1::2]))
    assert (ref.R[0] - Rf[0]).max() > 20.0                         # a quiet frame beside a loud one: its budget is the partner's
    odd = MB.reference(x[:512 + 2 * 160])                           # three frames
    _, Rf3 = MB._unclamped(x[None, :512 + 2 * 160], 3)
    assert odd.R.shape == (1, 3) and Rf3.shape == (1, 4) and odd.R[0, 2] == max(Rf3[0, 2], Rf3[0, 3])
    calls = MB.stream_reference(x, (1, 1))
    _, Rs = MB._unclamped(x[None, 1280 - 480:2560], 8)
    assert np.array_equal(calls[1].R[0, 0::2], np.maximum(Rs[0, 0::2], Rs[0, 1::2]))


@pytest.mark.parametrize("name", ["noise3000", "noise_silence", "tone60"])
def test_stream_reference_is_the_oracles_streaming_front_end(name):
    """The rows of stream_reference are what the oracle's float64 mel_stage gives for the buffer the reference hands its mel graph:
    the first 1280 samples alone (five rows), afterwards the last 480 samples of the stream so far and the new chunks."""
    x = MB.regimes()[name]
    calls = MB.stream_reference(x, (1, 1, 2))
    first = O.mel_transform(O.mel_stage(x[:1280].astype(np.float32), np.float64)[0, 0])
    assert first.shape == (5, 32)
    np.testing.assert_allclose(calls[0].clamped[0, 3:], first, rtol=0, atol=1e-12)
    assert (calls[0].clamped[0, :3] == 1.0).all() and (calls[0].budget[0, :3] == 0).all()
    for ref, (a, b) in zip(calls[1:], ((1280, 2560), (2560, 5120))):
        want = O.mel_transform(O.mel_stage(x[a - 480:b].astype(np.float32), np.float64)[0, 0])
        np.testing.assert_allclose(ref.clamped[0], want, rtol=0, atol=1e-12)
        assert (ref.budget >= MB.T0 / 10).all()


# ------------------------------------------------------------------------------------------------ the product's tables
def test_filterbank_equals_the_oracles_bit_for_bit():
    assert np.array_equal(W.mel_filterbank().view(np.uint32), O.mel_filterbank(np.float32).view(np.uint32))


def test_sparse_taps_rebuild_the_dense_bank():
    fb = W.mel_filterbank()
    start, taps, lo, hi = W.mel_sparse_taps()
    assert (lo, hi) == (2, 121) and taps.shape == (32, 16) and W.MEL_TAPS == 16
    dense = np.zeros_like(fb)
    for m in range(32):
        assert 2 <= start[m] and start[m] + 16 <= fb.shape[0]
        dense[start[m]:start[m] + 16, m] = taps[m]
        assert np.count_nonzero(fb[:, m]) <= 16
    assert np.array_equal(dense.view(np.uint32), fb.view(np.uint32))
    assert np.count_nonzero(fb[:2]) == 0 and np.count_nonzero(fb[122:]) == 0


def test_every_fft_bin_feeds_at_most_two_filters():
    per_bin = np.count_nonzero(W.mel_filterbank(), axis=1)
    assert per_bin.max() == 2 and per_bin[2:122].min() >= 1


def test_hann_window_equals_the_oracles_padded_window():
    padded = O.hann_window_padded(np.float32)
    assert np.array_equal(W.hann_window().view(np.uint32), padded[56:456].view(np.uint32))
    assert np.count_nonzero(padded[:56]) == 0 and np.count_nonzero(padded[456:]) == 0
