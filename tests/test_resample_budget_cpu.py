"""CPU tier of the device resampler's float64 comparison (tests/resample_ref.py): the filter design against a second implementation,
the float64 reference against the host restatement, every (geometry, signal) case of the GPU tier admitted through an fp32-chain
emulation, the case table held to the branches it is there for, and five plausibly wrong kernels shown to be rejected."""
import functools

import numpy as np
import pytest

import resample_ref as RR
from openwakeword_amd import resample as R
from openwakeword_amd import serve

PIN_RATES = tuple(serve.RATES) + (24000, 15999, 16001, 192000, 384000)       # (12000 is on the whitelist already)
# what the GPU tier runs beside the table: the 61 base rows of the large-S test
ADMITTED = tuple((rate, n_in, RR.ROWS) for rate, n_in in RR.CASES) + ((8000, 640, 61),)


@pytest.mark.parametrize("rate", sorted(set(PIN_RATES)))
def test_design_equals_an_independent_implementation(rate):
    """Own Bessel series, own sinc, own normalisation: equal to design()'s float32 taps to float32 rounding.  Two float64
    evaluations of the same formula differ by a few 2^-53 of the largest term, which moves a float32 rounding by at most one step;
    2^-40 absolute covers the taps at the sinc's zero crossings, where sin(pi * n) is 1e-16 in one implementation and 0 in the other."""
    p, q, taps = R.design(rate)
    p2, q2, ind = RR.independent_taps(rate)
    assert (p, q) == (p2, q2) == RR.ratio(rate) and taps.shape == ind.shape and taps.dtype == np.float32
    step = np.spacing(np.abs(ind).astype(np.float32)).astype(np.float64)
    assert (np.abs(taps.astype(np.float64) - ind) <= step + 2.0 ** -40).all()
    assert (taps == ind.astype(np.float32)).mean() > 0.9                     # and nearly all of them bit for bit


@pytest.mark.parametrize("rate,n_in", [(r, 997) for r in sorted(set(PIN_RATES) - {16000})])
def test_ref64_rounds_to_the_host_restatement(rate, n_in):
    """ref64 (header text, one pass per tap) and apply_numpy (gathered windows, one sum) are two float64 evaluations; away from
    rounding ties -- farther than 1e-6, a thousand times their own error -- they must give the same int16."""
    p, q, taps = R.design(rate)
    n_in = max(n_in, 3 * p // q + 1)
    x = RR.signals(rate, n_in, 12)
    y, A = RR.ref64(x, p, q, taps)
    want = R.apply_numpy(x, rate)
    assert want.shape == y.shape == (12, n_in * q // p)
    clear = np.abs(y - np.floor(y) - 0.5) > 1e-6
    assert clear.mean() > 0.9                                                # (the mask is not vacuous; the alternation row does tie)
    assert (np.clip(np.rint(y), -32768, 32767)[clear] == want[clear]).all()
    assert (A >= np.abs(y) - 1e-9).all()


@functools.lru_cache(maxsize=None)
def _admit(rate, n_in, rows):
    p, q, taps, x, y, A = RR.case_reference(rate, n_in, rows)
    got = RR.emulate32(x, p, q, taps)
    return got, float(RR.excess(got, y, A, taps.shape[1]).max()), RR.worst_ratio(got, y, A, taps.shape[1])


@pytest.mark.parametrize("rate,n_in,rows", ADMITTED)
def test_case_is_admitted_by_the_fp32_chain_emulation(rate, n_in, rows):
    """A case enters the GPU table only through here: the emulated chain is inside the budget on every output of every row, and the
    case's float64 values contain what the GPU tier relies on -- a clamped output and an output within gamma * A of a tie."""
    p, q, taps, x, y, A = RR.case_reference(rate, n_in, rows)
    got, worst_excess, used = _admit(rate, n_in, rows)
    n_taps = taps.shape[1]
    print(f"admit {rate} Hz n_in {n_in}: n_taps {n_taps} gamma*A max {RR.gamma(n_taps) * A.max():.3f} LSB, emulation uses "
          f"{used:.3f} of gamma*A, {int((got != np.clip(np.rint(y), -32768, 32767)).sum())} of {y.size} differ from rint(y64)")
    assert worst_excess <= 0.0
    assert RR.saturated(y).any(), "no output of this case is clamped"
    assert RR.near_tie(y, A, n_taps).any(), "no output of this case sits within gamma * A of a tie"
    assert used < 1.0


def test_full_scale_budget_is_what_the_docstring_says():
    for rate, lim in ((8000, 0.55), (48000, 0.55), (96000, 0.55), (192000, 1.2), (384000, 2.3)):
        p, q, taps = R.design(rate)
        ga = RR.gamma(taps.shape[1]) * 32768.0 * np.abs(taps.astype(np.float64)).sum(1).max()
        assert ga < lim, (rate, ga)
    assert R.design(192000)[2].shape[1] == 306 and R.design(384000)[2].shape[1] == 610


def test_case_table_covers_every_branch():
    geo = {}
    for rate, n_in in RR.CASES:
        p, q, taps = R.design(rate)
        g = RR.launch_geometry(n_in, p, q, taps.shape[1])
        g.update(p=p, q=q, n_taps=taps.shape[1])
        assert not g["refused"] and g["n_out"] >= 1
        geo[(rate, n_in)] = g
    have = lambda f: [k for k, g in geo.items() if f(g)]                      # noqa: E731
    assert have(lambda g: g["n_wg"] > 1 and g["fractional_start"])
    assert have(lambda g: g["n_wg"] > 1 and g["n_out"] % g["opb"] == 0)
    assert have(lambda g: g["n_out"] < 256)
    assert have(lambda g: g["n_out"] % 256 != 0 and g["n_out"] > 256)
    assert have(lambda g: g["opb"] == 768 and g["n_wg"] > 1) and have(lambda g: g["opb"] == 256 and g["n_wg"] > 1)
    assert have(lambda g: g["taps_in_lds"] == 0 and g["n_wg"] > 1)
    assert have(lambda g: g["q"] == 1 and g["n_wg"] > 1)
    assert have(lambda g: g["ntp"] == g["n_taps"]) and have(lambda g: g["ntp"] == g["n_taps"] + 2)
    assert have(lambda g: g["p"] < g["q"]) and have(lambda g: g["p"] > g["q"])
    # the stated reason of single cases
    assert geo[(8000, 3)]["n_out"] == 6
    assert geo[(12000, 2880)]["n_wg"] == 3 and (geo[(12000, 2880)]["p"], geo[(12000, 2880)]["q"]) == (3, 4)
    assert geo[(22050, 1764)]["n_taps"] == geo[(22050, 1764)]["ntp"] == 36
    assert geo[(24000, 3847)]["n_out"] == 2564
    assert geo[(44100, 7056)]["n_wg"] == 2 and geo[(44100, 7056)]["n_out"] == 2560
    assert (geo[(192000, 30720)]["opb"], geo[(192000, 30720)]["n_wg"]) == (768, 4)
    assert (geo[(384000, 30720)]["opb"], geo[(384000, 30720)]["n_wg"]) == (256, 5)
    assert (geo[(16001, 1300)]["taps_in_lds"], geo[(16001, 1300)]["n_wg"]) == (0, 2)
    assert (geo[(15999, 2600)]["taps_in_lds"], geo[(15999, 2600)]["n_wg"]) == (0, 3)
    # the refusal the GPU tier asks for, and the geometries of the existing device test, which all stay in one workgroup with LDS taps
    assert RR.launch_geometry(200, 200, 1, 2)["refused"]
    for rate, n_in in ((8000, 640), (48000, 3840), (44100, 3528), (22050, 1764), (32000, 2560)):
        p, q, taps = R.design(rate)
        g = RR.launch_geometry(n_in, p, q, taps.shape[1])
        assert (g["opb"], g["n_wg"], g["taps_in_lds"]) == (1280, 1, 1)


@pytest.mark.parametrize("variant", RR.VARIANTS)
def test_the_budget_rejects_a_wrong_kernel(variant):
    """Each defect, emulated with the same fp32 chain, must break the assertion -- and not only on the six-output case, which is
    all edges: on a case with several workgroups per stream, and on one whose bank is read from global memory, where most outputs
    lie in the interior of the message (interior: more than two filter lengths from either end; the edge clamp, an edge defect by
    nature, is looked for anywhere in those cases).  Truncation moves an output by less than 1, so only cases with gamma * A < 0.5 can show
    it: it is looked for at those rates alone."""
    caught = {}
    for rate, n_in in RR.CASES:
        p, q, taps, x, y, A = RR.case_reference(rate, n_in)
        if variant == "truncate" and RR.gamma(taps.shape[1]) * A.max() >= 0.5:
            continue
        bad = RR.emulate32(x, p, q, taps, variant)
        over = RR.excess(bad, y, A, taps.shape[1]) > 0
        g = RR.launch_geometry(n_in, p, q, taps.shape[1])
        caught[(rate, n_in)] = (int(over.sum()), int(over[:, 2 * taps.shape[1]:-2 * taps.shape[1]].sum()), g["n_wg"], g["taps_in_lds"])
    print(f"{variant}: outputs rejected (all, interior) per case: " + ", ".join(f"{k[0]}/{k[1]}: {v[0]}, {v[1]}" for k, v in caught.items()))
    assert any(v[0] for v in caught.values()), f"the budget accepts a kernel with defect {variant!r} on every case"
    where = 0 if variant == "edge_clamp" else 1                              # (an edge defect leaves the interior alone by nature)
    assert any(v[where] and v[2] > 1 for v in caught.values()), f"{variant!r} is not caught on a multi-workgroup case"
    assert any(v[where] and v[3] == 0 for v in caught.values()), f"{variant!r} is not caught on a global-taps case"
