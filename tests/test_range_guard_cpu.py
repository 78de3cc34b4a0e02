"""The range-guard bench (tests/range_guard.py) against the sources, and the admission of its two gain sweeps (no GPU).

The mirror of the conv histories is held to csrc/owwhip_layout.h and to DESIGN.md 5.16's record table.  A gain is admitted to a
sweep only if the fp32 oracle itself stays inside the project's fp32 envelope at that gain, so that a finite device result outside
the budget with the range flag down is the kernel's fault and not the number format's: the CNN sweep against cnn_budget.E32 in
cnn_budget's normalisation, the head sweep against test_head_regimes.FP32_CAP.  Both hold at every gain, so no gain is dropped and
the device budgets are cnn_budget.T and TOL_SCORE, unchanged.

Heads without LayerNorm saturate under the feature gain (their logits grow with it): their float64 scores end up at exactly 0 or 1
and the device comparison at large gains is one of saturated sigmoids.  They stay in the sweep -- what is asked of them at those
gains is to be loud or still right -- and only the LayerNorm forms, whose scores keep moving, are held to np.ptp(want) > 0.05."""
import os
import re

import numpy as np
import pytest

from oracle import oww_oracle as O

import cnn_budget as CB
import range_guard as RG
import test_head_regimes as HR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _layout_array(name):
    with open(os.path.join(ROOT, "openwakeword_amd", "csrc", "owwhip_layout.h")) as f:
        src = f.read()
    m = re.search(r"inline constexpr int %s\[N_STATE\]\s*=\s*\{([^}]*)\}" % name, src)
    assert m, name
    return tuple(int(v) for v in m.group(1).split(","))


def test_mirror_matches_the_layout_header():
    with open(os.path.join(ROOT, "openwakeword_amd", "csrc", "owwhip_layout.h")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int N_STATE\s*=\s*(\d+)", src).group(1)) == len(RG.NAMES) == 11
    assert _layout_array("kStateLenRr") == RG.WORDS
    assert _layout_array("kStateSpgRr") == RG.STREAMS_PER_GROUP
    # the comment above the arrays names the sections in the mirror's order
    assert re.search(r"hist_mel, hist2, B:b,d\s+C:b,d\s+D:b,d\s+E:b,d\s+hist19", src)
    # a stage's guard reports the streams of its group: the table is kStateSpgRr except where another kernel reports
    for name, spg in zip(RG.NAMES, RG.STREAMS_PER_GROUP):
        assert RG.REPORTED_STREAMS[name] == (32 if name == "hist19" else spg)


def test_default_record_is_49344_bytes():
    words = RG.HEADER_WORDS + sum(RG.WORDS) + sum(RG.OTHER_WORDS_DEFAULT.values())
    assert words * 4 == RG.DEFAULT_RECORD_BYTES == 49344
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "(49,344 bytes; offsets in 4-byte words)" in f.read()


@pytest.mark.parametrize("has_vad", [False, True])
def test_offsets_tile_both_ends(has_vad):
    nb = RG.DEFAULT_RECORD_BYTES + (4 * (4 + RG.VAD_HC_WORDS) if has_vad else 0)
    off = RG.offsets(nb, has_vad)
    flat = [n for n, g in zip(RG.NAMES, RG.STREAMS_PER_GROUP) if g == 1]
    grouped = [n for n, g in zip(RG.NAMES, RG.STREAMS_PER_GROUP) if g > 1] + ([RG.VAD_HC] if has_vad else [])
    at = RG.HEADER_WORDS
    for n in flat:
        assert off[n] == (at, RG.WORDS[RG.NAMES.index(n)])
        at += off[n][1]
    assert off[grouped[-1]][0] + off[grouped[-1]][1] == nb // 4
    for a, b in zip(grouped, grouped[1:]):
        assert off[a][0] + off[a][1] == off[b][0]
    middle = off[grouped[0]][0] - at
    assert middle == sum(RG.OTHER_WORDS_DEFAULT.values()) + (4 if has_vad else 0)


def test_poison_writes_what_the_docstring_says():
    r = np.random.default_rng(5)
    rec = r.integers(1, 255, RG.DEFAULT_RECORD_BYTES, dtype=np.uint8)
    off = RG.offsets(rec.size)
    for name in RG.NAMES:
        first, n = off[name]
        for words in (None, RG.seeded_words(rec, name, 3)):
            got = RG.poison(rec, name, words).view(np.uint32)
            changed = np.flatnonzero(got != rec.view(np.uint32))
            assert changed.size and changed.min() >= first and changed.max() < first + n, name     # nothing outside the section
            sec = got[first:first + n]
            if name == "hist_mel":
                assert (sec[changed - first] == 0xFC007C00).all()
                assert changed.size == (n if words is None else 1)
            elif name == "hist2":
                d = ((changed - first) // 64) % 8
                assert set(d.tolist()) <= {0, 1, 2, 3, 4, 5}                                       # dwords 6, 7 stay as they were
                assert (sec[(changed - first)[d < 3]] == 0x7C007C00).all() and (sec[(changed - first)[d >= 3]] == 0xFC00FC00).all()
                assert changed.size == (n // 8 * 6 if words is None else 2)
            else:
                assert (sec.view(np.float32)[changed - first] == np.float32(1.0e5)).all()
                assert changed.size == (n if words is None else 1)
    # the halves are the f16 split of 1.0e5
    with np.errstate(over="ignore"):
        hi = np.float32(1.0e5).astype(np.float16)
        lo = (np.float32(1.0e5) - hi.astype(np.float32)).astype(np.float16)
    assert hi.view(np.uint16) == RG.HI_INF and lo.view(np.uint16) == RG.LO_NINF
    # a word that is zero in the warmed-up record is never drawn
    rec0 = rec.copy()
    first, n = off["C:b"]
    rec0.view(np.uint32)[first:first + n] = 0
    rec0.view(np.uint32)[first + 17] = 1
    assert all(RG.seeded_words(rec0, "C:b", seed)[0] == 17 for seed in range(8))


def test_expected_where():
    assert RG.expected_where("C:b", 31, 69) == (30, 2)
    assert RG.expected_where("E:d", 68, 69) == (64, 5)             # the last group of eight holds five
    assert RG.expected_where("hist19", 63, 69) == (32, 32)
    assert RG.expected_where("hist19", 68, 69) == (64, 5)
    assert RG.expected_where(RG.VAD_HC, 40, 69) == (32, 16)
    assert RG.MEL_GAINS[0] == 1.0 and RG.MEL_GAINS[-1] == 2.0 ** 24 and len(RG.MEL_GAINS) == 13
    assert RG.FEATURE_GAINS[0] == 1.0 and RG.FEATURE_GAINS[-1] == 2.0 ** 20 and len(RG.FEATURE_GAINS) == 21


@pytest.mark.parametrize("name", RG.CNN_REGIMES)
def test_mel_gain_sweep_is_admitted(name):
    """fp32 oracle against float64 on mel * 2^k, per window, in cnn_budget's normalisation: inside E32 at every gain (measured: 9.4e-7
    at worst against E32 = 2.5e-6), so the device is held to T = 4 * E32 over the whole sweep."""
    emb, _ = CB.regime(name)
    x = RG.cnn_inputs()
    worst = 0.0
    for g in RG.MEL_GAINS:
        xg = x * np.float32(g)
        e64 = O.embedding_stage(xg, emb, np.float64)[:, :, 0, :]
        e32 = O.embedding_stage(xg, emb, np.float32)[:, :, 0, :]
        assert e64.shape == (3, 3, 96) and np.isfinite(e32).all()
        r = float(RG.window_ratios(e32, e64).max())
        worst = max(worst, r)
        assert r <= CB.E32, f"{name}, gain {g:g}: the fp32 oracle is {r:.2e} of the window's largest value off float64"
    print(f"\n{name}: fp32 oracle's worst window over the mel gains {worst:.2e} (E32 = {CB.E32:.1e})")


@pytest.mark.parametrize("form", list(RG.HEAD_SHAPES))
def test_feature_gain_sweep_is_admitted(form):
    head = RG.make_head(form)
    ft = HR.features(16)
    worst, span = 0.0, np.inf
    for g in RG.FEATURE_GAINS:
        with np.errstate(over="ignore"):
            w64 = O.head_stage(ft * np.float32(g), head, np.float64)
            w32 = O.head_stage(ft * np.float32(g), head, np.float32)
        assert np.isfinite(w32).all() and np.isfinite(w64).all()
        err = float(np.abs(w32.astype(np.float64) - w64).max())
        worst, span = max(worst, err), min(span, float(np.ptp(w64)))
        assert err <= HR.FP32_CAP, f"{form}, gain {g:g}: |fp32 - float64| = {err:.2e}"
        if RG.HEAD_SHAPES[form]["layernorm"]:
            assert np.ptp(w64) > 0.05, f"{form}, gain {g:g}: the float64 scores no longer move"
    print(f"\n{form}: |fp32 - float64| <= {worst:.2e}, smallest span of the float64 scores {span:.3f}")


@pytest.mark.parametrize("has_vad", [False, True])
def test_mirror_against_the_layout_planner(has_vad):
    """range_guard.offsets against ows::layout (csrc/owwhip_state_host.h) on the default register-resident configuration, sections in
    the order owwhip.hip::state_layout lists them (tests/planners_check.cpp): the eleven conv histories at both ends of the record,
    and the VAD's (h, c) section behind them when the handle has a VAD."""
    from test_planners_cpu import record_offsets, self_checks
    got = record_offsets(has_vad)
    nb = int(self_checks()["record_bytes%d" % int(has_vad)])
    assert nb == RG.DEFAULT_RECORD_BYTES + (4 * (4 + RG.VAD_HC_WORDS) if has_vad else 0)
    want = RG.offsets(nb, has_vad)
    assert len(want) == 11 + int(has_vad) and (RG.VAD_HC in got) == has_vad
    for name, at in want.items():
        assert got[name] == at, name
    # what lies between the two ends is what the default record's table says
    for name, words in RG.OTHER_WORDS_DEFAULT.items():
        assert -(-got[name][1] // 4) * 4 == words, name
