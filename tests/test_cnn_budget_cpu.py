"""CPU tier of the embedding CNN's float64 comparison (tests/cnn_budget.py): the frozen E32 against the fp32 oracle's own error over the
whole case table, which (regime, input) pairs a faithful f16-split kernel can carry at T = 4 * E32, which branches of the activation
the table reaches, and that a kernel with one wrong constant, term or exponent in one layer leaves the budget at that layer."""
import functools
import os

import numpy as np
import pytest

import cnn_budget as CB
from oracle import oww_oracle as O

SETS = ("mel", "pcm")                    # the embed() inputs; the float64 oracle's mel rows of the streaming PCM (12 steps, last 92 rows)
INPUTS = tuple(("mel", n) for n in CB.MEL_NAMES) + tuple(("pcm", n) for n in CB.PCM_NAMES)


@functools.lru_cache(maxsize=None)
def _sets():
    golden = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_streaming.npz"))
    return {"mel": CB.mel_inputs(), "pcm": CB.oracle_mel_of_pcm(CB.pcm_rows(golden["pcm/alexa_test"]))}


def _worst_over_steps(got, y64, l):
    """[B]: the largest err / M of layer l over the three steps the inputs end with."""
    return np.max([CB.ratios(CB.step_rows(got, l, k), CB.step_rows(y64, l, k)) for k in range(3)], axis=0)


@functools.lru_cache(maxsize=None)
def _analysis(name):
    """Per regime: the ladder, and per input set the float64 chain, the faithful emulation's carried inputs, and [20, 9] arrays of
    err / M for the fp32 oracle and the faithful emulation."""
    emb, _ = CB.regime(name)
    exps = CB.ladder_for(emb, [_sets()[sn] for sn in SETS])
    out = {"emb": emb, "exps": exps}
    for sn in SETS:
        x = _sets()[sn]
        a64, p64 = CB.layers64(x, emb)
        a32, _ = CB.layers(x, emb, np.float32)
        emu, carried = CB.emulate_split(x, emb, exps)
        out[sn] = {"a64": a64, "p64": p64, "carried": carried, "emu19": emu[19],
                   "e32": np.stack([_worst_over_steps(a32[l], a64[l], l) for l in range(CB.N_LAYERS)]),
                   "emu": np.stack([_worst_over_steps(emu[l], a64[l], l) for l in range(CB.N_LAYERS)])}
    return out


def _names(sn):
    return CB.MEL_NAMES if sn == "mel" else CB.PCM_NAMES


def test_constants_and_table():
    assert CB.T == 4 * CB.E32
    assert CB.NEW_ROWS == (8, 8, 8, 4, 4, 4, 4, 4, 4, 4, 4, 2, 2, 2, 2, 2, 2, 2, 2, 1)
    assert len(CB.REGIMES) == 10 and set(CB.SEEDS) == {"seed1234", "seed1", "seed2"}
    mel = CB.mel_inputs()
    assert mel.shape == (9, 76 + 16, 32) and mel.dtype == np.float32 and not mel.flags.writeable
    assert (mel[1] == 1).all() and (mel[2] == -6).all() and (mel[3] == 12).all() and set(np.unique(mel[5])) == {-6.0, 12.0}
    for s, b in ((4, 0), (6, 15), (7, 16), (8, 31)):
        d = mel[s] - 2.0
        assert np.count_nonzero(d) == 1 and d[CB.IMPULSE_ROW, b] == 8.0
    pcm = _sets()["pcm"]
    assert pcm.shape == (9, 92, 32)
    x = CB.pcm_rows(np.zeros(5, np.int16))
    assert x.dtype == np.int16 and x.shape == (9, 12 * 1280) and not x[0].any() and not x[8, :6 * 1280].any()
    assert set(np.unique(x[6])) == {-32767, 32767} and (x[6, :16] == -32767).all() and (x[6, 16:32] == 32767).all()
    assert abs(float(x[1].std()) - 1.0) < 0.2 and int(np.abs(x[5]).max()) > 32000 and int(np.abs(x[8]).max()) > 32000


def test_regimes_restate_the_weight_regime_module():
    """cnn_budget.regime() is tests/test_weight_regimes.py::_regime plus channel_cold."""
    import test_weight_regimes as TW
    for name in CB.REGIMES:
        if name == "channel_cold":
            continue
        a, sa = CB.regime(name)
        b, sb = TW._regime(name)
        assert sa == sb
        for u, v in zip(a["conv"], b["conv"]):
            np.testing.assert_array_equal(u, v)
        for u, v in zip(a["bn"], b["bn"]):
            for p, q in zip(u, v):
                np.testing.assert_array_equal(p, q)


def test_channel_cold_is_the_same_function_in_exact_arithmetic():
    """2^-8 on a channel's BatchNorm and 2^8 on the next convolution's weights of that input channel: the float64 chains agree wherever
    the cold channels stay above the activation's floor; the regime moves the scale inside a layer, not the network."""
    base, _ = CB.regime("seed1234")
    cold, _ = CB.regime("channel_cold")
    for l in (4, 8, 12, 16):
        idx = np.arange(base["bn"][l][0].size) % 4 == 0
        np.testing.assert_array_equal(cold["bn"][l][0][idx], base["bn"][l][0][idx] * np.float32(2.0 ** -8))
        np.testing.assert_array_equal(cold["bn"][l][1][~idx], base["bn"][l][1][~idx])
        np.testing.assert_array_equal(cold["conv"][l + 1][:, :, idx], base["conv"][l + 1][:, :, idx] * np.float32(2.0 ** 8))
        np.testing.assert_array_equal(cold["conv"][l + 1][:, :, ~idx], base["conv"][l + 1][:, :, ~idx])


@pytest.mark.parametrize("name", CB.REGIMES)
def test_fp32_oracle_stays_inside_E32(name):
    """The reference's own fp32 chain is within E32 * max|y64| of float64 on every (regime, input, layer, step)."""
    a = _analysis(name)
    worst = max(((float(a[sn]["e32"][l, s]), sn, _names(sn)[s], l) for sn in SETS for l in range(CB.N_LAYERS) for s in range(9)))
    print(f"\n{name}: fp32 oracle envelope {worst[0]:.3e} = {worst[0] / CB.E32:.2f} E32 at input {worst[1]}/{worst[2]}, layer {worst[3]}")
    assert worst[0] <= CB.E32


def test_frozen_E32_is_the_measured_envelope():
    """E32 is neither stale nor loose: the envelope measured now lies in (E32 / 1.5, E32] (measured 1.94e-6, frozen 2.5e-6)."""
    worst = max(((float(_analysis(n)[sn]["e32"][l, s]), n, sn, _names(sn)[s], l)
                 for n in CB.REGIMES for sn in SETS for l in range(CB.N_LAYERS) for s in range(9)))
    print(f"\nE32 measured {worst[0]:.3e} at (regime {worst[1]}, input {worst[2]}/{worst[3]}, layer {worst[4]}); frozen {CB.E32:.2e}, "
          f"T = {CB.T:.2e}")
    assert CB.E32 / 1.5 < worst[0] <= CB.E32


def test_admission():
    """A (regime, input) pair enters the f16-split table only if the FAITHFUL emulation stays within T at every layer.  What is left out is
    listed with its figure; at most one regime, no seed."""
    left_out = {}
    print()
    for name in CB.REGIMES:
        a = _analysis(name)
        frac = {(sn, _names(sn)[s]): float(a[sn]["emu"][:, s].max()) / CB.T for sn in SETS for s in range(9)}
        worst = max(frac, key=frac.get)
        out = {k: v for k, v in frac.items() if not v <= 1.0}
        print(f"{name}: faithful f16-split emulation at most {frac[worst]:.2f} T (input {worst[0]}/{worst[1]}); "
              f"{len(frac) - len(out)} of {len(frac)} inputs admitted; ladder e = {a['exps']['e']}")
        for k, v in sorted(out.items()):
            print(f"    not admitted: ({name}, {k[0]}/{k[1]}) at {v:.2f} T")
        if out:
            left_out[name] = max(out.values())
    assert set(left_out) == set(CB.NOT_ADMITTED), "cnn_budget.NOT_ADMITTED is what the emulation leaves out: a whole regime each"
    assert len(left_out) <= 1 and not set(left_out) & set(CB.SEEDS)
    for name, v in left_out.items():
        assert v == pytest.approx(CB.NOT_ADMITTED[name], rel=0.25), "the recorded figure is the measured one"
    assert CB.ADMITTED == tuple(n for n in CB.REGIMES if n not in left_out)


# (regime, branch) -> layers of 1 .. 18 that CANNOT reach 1 % by the regime's own arithmetic
_L5 = (1, 5, 9, 13, 17)
COVERAGE_EXEMPT = {
    ("hot", "leaky"): _L5,               # BatchNorm output x 3e3: the leaky band (-2, 0] holds 1e-4 of the values
    ("cold", "floor"): _L5,              # BatchNorm output x 1e-4: |pre-activation| < 2, the floor is out of reach
    ("conv_1e-3", "floor"): tuple(range(1, 19)),   # every pre-activation is its BatchNorm shift +- 1e-3: none below -2
}


def _coverage(name):
    """[20, 3]: the share of float64 pre-activations in the positive, leaky and floor (< -2) branch over the regime's inputs together,
    the all-ones input left out."""
    a = _analysis(name)
    cnt, n = np.zeros((CB.N_LAYERS, 3)), np.zeros(CB.N_LAYERS)
    for sn in SETS:
        keep = [s for s in range(9) if not (sn == "mel" and CB.MEL_NAMES[s] == "ones")]
        for l in range(CB.N_LAYERS):
            p = a[sn]["p64"][l][keep]
            cnt[l] += [(p > 0).sum(), ((p <= 0) & (p >= -2)).sum(), (p < -2).sum()]
            n[l] += p.size
    return cnt / n[:, None]


@pytest.mark.parametrize("name", CB.REGIMES)
def test_every_branch_of_the_activation_is_reached(name):
    """Every BatchNorm layer 1 .. 18 has at least 1 % of its float64 pre-activations in each of the three branches, over the regime's
    inputs together.  Three regimes move the pre-activations themselves (hot x 3e3, cold x 1e-4, conv_1e-3) and cannot reach one branch
    in the layers they rescale, whatever the input: those (regime, layer, branch) are listed, and held to be UNREACHED (below 1 %), so
    the list cannot outlive its reason.  Layer 0 (conv, ReLU, BatchNorm) reaches its floor only under a negative BatchNorm scale."""
    cov = _coverage(name)
    print(f"\n{name}: smallest share over layers 1..18: positive {cov[1:19, 0].min():.3f}, leaky {cov[1:19, 1].min():.3f}, "
          f"floor {cov[1:19, 2].min():.3f}; layer 0 floor {cov[0, 2]:.4f}")
    for b, branch in enumerate(("positive", "leaky", "floor")):
        exempt = COVERAGE_EXEMPT.get((name, branch), ())
        for l in range(1, 19):
            if l in exempt:
                assert cov[l, b] < 0.01, (name, l, branch, cov[l, b])
            else:
                assert cov[l, b] >= 0.01, (name, l, branch, cov[l, b])
    if name == "negative_bn":
        assert cov[0, 2] >= 0.01


# ------------------------------------------------------------------------------------------------------------------------ teeth
def _break(variant, site, seen, regimes):
    """The first admitted case on which `variant` made in layer `site` leaves T at layer `seen`: (fraction of T, regime, input)."""
    best = (0.0, None, None)
    for name in regimes:
        a = _analysis(name)
        for sn in SETS:
            emu, _ = CB.emulate_split(_sets()[sn], a["emb"], a["exps"], f"{variant}@{site}", resume=(site, a[sn]["carried"]), upto=seen)
            r = _worst_over_steps(emu[seen], a[sn]["a64"][seen], seen) / CB.T
            s = int(r.argmax())
            if r[s] > best[0]:
                best = (float(r[s]), name, f"{sn}/{_names(sn)[s]}")
            if best[0] > 1.0:
                return best
    return best


@pytest.mark.parametrize("variant", CB.VARIANTS)
def test_a_wrong_kernel_leaves_the_budget_where_it_is_wrong(variant):
    """Each wrong kernel, made in an early, a middle and a late layer, breaks |got - y64| <= T * M at that layer on an admitted case."""
    print()
    for site, seen in CB.variant_sites(variant):
        f, name, inp = _break(variant, site, seen, CB.ADMITTED)
        print(f"{variant} in layer {site}: {f:.2f} T at layer {seen} on ({name}, {inp})")
        assert f > 1.0, (variant, site)


@pytest.mark.parametrize("variant", ["floor_f16", "leak_f16"])
def test_the_flat_tolerance_let_the_f16_constants_through(variant):
    """What the relative budget is for: a floor or a leak slope rounded to f16 in ONE layer, rejected above, passes the older comparisons.
    tests/test_gpu_parity.py holds embeddings to a flat 2e-4 on 3000-rms noise and the fixture clips: on those two inputs of this table
    the defect stays below 2e-4 absolute at every site.  tests/test_weight_regimes.py allows 2e-4 * max(1, |e|): every input of the
    table stays below that (the largest figure, 2.4e-4, is the N(10, 1.5) mel input, which no older test runs)."""
    a = _analysis("seed1234")
    old = [CB.PCM_NAMES.index("noise3000"), CB.PCM_NAMES.index("alexa")]
    print()
    for site, _ in CB.variant_sites(variant):
        err, scale = {}, {}
        for sn in SETS:
            emu, _ = CB.emulate_split(_sets()[sn], a["emb"], a["exps"], f"{variant}@{site}", resume=(site, a[sn]["carried"]))
            e64 = a[sn]["a64"][19]
            err[sn] = np.abs(emu[19].astype(np.float64) - e64).reshape(9, -1).max(axis=1)
            scale[sn] = np.abs(e64).reshape(9, -1).max(axis=1)
        print(f"{variant} in layer {site}: max |embedding - float64| = {err['pcm'][old].max():.2e} on noise3000 / alexa (flat tolerance 2e-4), "
              f"{max(err['mel'].max(), err['pcm'].max()):.2e} over the table on |e| <= {max(scale['mel'].max(), scale['pcm'].max()):.3g}")
        assert err["pcm"][old].max() < 2e-4
        for sn in SETS:
            assert (err[sn] < 2e-4 * np.maximum(1.0, scale[sn])).all()


def test_emulated_embedding_is_the_oracles_embedding_stage():
    """layers64's last layer is oracle.oww_oracle.embedding_stage in float64, window by window (what the GPU tier compares embed() with)."""
    emb, _ = CB.regime("seed1")
    x = _sets()["mel"]
    act, _ = CB.layers64(x, emb)
    want = np.stack([O.embedding_stage(x[:, 8 * k:8 * k + 76], emb, np.float64).reshape(9, 96) for k in range(3)], axis=1)
    np.testing.assert_allclose(act[19].reshape(9, 3, 96), want, rtol=0, atol=1e-12)
