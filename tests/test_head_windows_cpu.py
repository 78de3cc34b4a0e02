"""CPU tier of the head kernels over feature-window lengths (tests/head_windows.py; the device tier is test_head_windows_gpu.py):
the cases are admissible (fp32 itself carries them), centred (the sigmoid comparison is not vacuous), the comparison would see a weight
ring that drops a chunk or reuses a stale one, and the case table reaches every shape of the k loop the ABI's window lengths can
produce.  pytest -s prints the figures DESIGN.md 5.22 records."""
import numpy as np
import pytest

from oracle import oww_oracle as O

import head_windows as HW

_CASES = [(f, T) for f, spec in HW.FORMS.items() for T in spec["Ts"]]
_DENSE = [(f, T) for f, T in _CASES if not f.startswith("rnn")]
_ids = lambda cases: [f"{f}-T{T}" for f, T in cases]       # noqa: E731


@pytest.mark.parametrize("form,T", _CASES, ids=_ids(_CASES))
def test_cases_are_admissible(form, T):
    """What fp32 cannot carry is not asked of the device: the fp32 oracle within FP32_CAP of float64 on the case's own inputs."""
    w64, w32 = HW.want(form, T), HW.want(form, T, np.float32)
    for n in w64:
        assert np.isfinite(w64[n]).all() and np.isfinite(w32[n]).all()
        err = float(np.abs(w32[n] - w64[n]).max())
        print(f"\n{n}: |fp32 - float64| = {err:.2e}")
        assert err <= HW.FP32_CAP
        if w64[n].shape[1] > 1:
            np.testing.assert_allclose(w64[n].sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("form", sorted(HW.BANK_FORMS))
def test_bank_shapes_are_admissible(form):
    for T in HW.T_EDGE:
        ft = HW.windows(T)
        h = HW.bank_head(form, T, ft)
        err = float(np.abs(O.head_stage(ft, h, np.float32).astype(np.float64) - O.head_stage(ft, h, np.float64)).max())
        print(f"\n{form} T={T}: |fp32 - float64| = {err:.2e}, share in (0.05, 0.95) = {HW.mid_fraction(O.head_stage(ft, h, np.float64)):.2f}")
        assert err <= HW.FP32_CAP
        assert HW.mid_fraction(O.head_stage(ft, h, np.float64)) >= HW.MID_SHARE


@pytest.mark.parametrize("form,T", _CASES, ids=_ids(_CASES))
def test_binary_cases_are_centred(form, T):
    """At least a quarter of a binary case's float64 scores lie in (0.05, 0.95), and the centring did what it says: the median float64
    logit of every net is zero to the rounding of the fp32 bias (a gated head's first net: the gate lies in a gap of the logits)."""
    heads, w64 = HW.form_heads(form, T), HW.want(form, T)
    for n, h in heads.items():
        if not HW.is_binary(h):
            assert np.ptp(w64[n]) > 0.05                   # (softmax rows: they move with the input)
            continue
        share = HW.mid_fraction(w64[n])
        print(f"\n{n}: share of float64 scores in (0.05, 0.95) = {share:.2f}")
        assert share >= HW.MID_SHARE
        for i, z in enumerate(HW.logits64(h, HW.windows(T))):
            if h["kind"] == "gated" and i == 0:            # the gating net: no row on the gate, and rows on both sides of it
                assert np.abs(z).min() >= HW.GATE_MARGIN and min((z > 0).sum(), (z < 0).sum()) >= HW.N_ROWS // 3
            else:
                assert abs(np.median(z)) < 1e-5


@pytest.mark.parametrize("form,T", _DENSE, ids=_ids(_DENSE))
def test_a_lost_kstep_moves_a_score(form, T):
    """The comparison would see a pipeline fault: on the float64 oracle, a first layer that lost one k-step -- the chunk dropped, or the
    slot still holding the k-step before -- moves at least one compared score of every head by more than 10 x TOL_SCORE, at the first
    k-step, the middle one and the last two (where the conditional groups run)."""
    ft, w64 = HW.windows(T), HW.want(form, T)
    least = np.inf
    for n, h in HW.form_heads(form, T).items():
        for ks in HW.fault_ksteps(T):
            for variant in ("dropped", "stale"):
                if variant == "stale" and ks == 0:
                    continue                               # (no k-step before the first)
                moved = float(np.abs(O.head_stage(ft, HW.kstep_fault(h, ks, variant), np.float64) - w64[n]).max())
                least = min(least, moved)
                assert moved > 10 * HW.TOL_SCORE, f"{n}: k-step {ks} {variant} moves the scores by {moved:.2e} only"
    print(f"\n{form} T={T}: least movement over k-steps {HW.fault_ksteps(T)} x (dropped, stale) = {least:.2e}")


def test_kstep_fault_is_what_it_says():
    h = HW.form_heads("narrow2", 3)["narrow2_t3_0"]
    d, s = HW.kstep_fault(h, 4, "dropped"), HW.kstep_fault(h, 4, "stale")
    for k in ("net", "net2"):
        assert not d[k]["w1"][128:160].any() and np.array_equal(d[k]["w1"][:128], h[k]["w1"][:128]) and np.array_equal(d[k]["w1"][160:], h[k]["w1"][160:])
        assert np.array_equal(s[k]["w1"][128:160], h[k]["w1"][96:128]) and np.array_equal(s[k]["w1"][:128], h[k]["w1"][:128])
    assert HW.fault_ksteps(1) == [0, 1, 2] and HW.fault_ksteps(120) == [0, 180, 358, 359]


def test_case_table_reaches_every_shape_of_the_k_loop():
    """Through the mirror of the launch rule: every (NBUF, KST mod NBUF) that 3 T can produce for NBUF 2, 4 and 6; KST <= D; an empty
    main loop; a main-loop group followed by a partial tail group -- each on the fixed kernel, the two-slot shapes on the bank kernel
    too, at both of its wave counts."""
    cases = HW.ring_cases()
    for label, sh in cases:
        print(f"\n{label}: KST {sh['KST']} NBUF {sh['NBUF']} prologue {sh['prologue']} main groups {sh['main_groups']} tail groups {sh['tail_groups']} "
              f"partial {sh['partial']}")
    fixed = [sh for label, sh in cases if not label.startswith("bank")]
    bank = [sh for label, sh in cases if label.startswith("bank")]
    assert [HW.reachable_residues(n) for n in (2, 4, 6)] == [[0, 1], [0, 1, 2, 3], [0, 3]]
    for nbuf in (2, 4, 6):
        assert sorted({sh["mod"] for sh in fixed if sh["NBUF"] == nbuf}) == HW.reachable_residues(nbuf), nbuf
        assert any(sh["main_then_partial"] for sh in fixed if sh["NBUF"] == nbuf), nbuf
    for nbuf in (4, 6):                                    # (two slots: the main loop runs from KST = 3 on, and D = 1 < 3)
        assert any(sh["empty_main"] for sh in fixed if sh["NBUF"] == nbuf), nbuf
        assert any(sh["kst_le_d"] for sh in fixed if sh["NBUF"] == nbuf), nbuf
        assert any(sh["KST"] == nbuf and sh["empty_main"] for sh in fixed if sh["NBUF"] == nbuf) or nbuf == 4      # (3 T = 4 does not exist)
    assert {sh["NBUF"] for sh in bank} == {HW.BANK_NBUF}
    for waves in (1, 4):
        assert sorted({sh["mod"] for sh in bank if sh["waves"] == waves}) == [0, 1]
        assert any(sh["main_then_partial"] for sh in bank if sh["waves"] == waves)
    # both forms of the fixed kernel and every NN meet a partial tail group at every ring depth they run
    for form in HW.RING_FORMS:
        mine = [sh for label, sh in cases if label.startswith(form + " ")]
        assert {sh["NBUF"] for sh in mine} == {2, HW.heads_nbuf(HW.FORMS[form]["ht"], HW.FORMS[form]["nn"], HW.N_ROWS)}
        for nbuf in {sh["NBUF"] for sh in mine}:
            assert any(sh["partial"] for sh in mine if sh["NBUF"] == nbuf), (form, nbuf)


def test_mirror_of_the_launch_rule():
    """The mirror restates owwhip_pack.h::pack_head_groups / owwhip.hip::run_heads / owwhip_bank_host.h::route; the cases the issue names."""
    assert HW.tail_shape(16, 4) == dict(KST=48, NBUF=4, mod=0, main_groups=11, tail_groups=1, partial=0, prologue=3, kst_le_d=False,
                                        empty_main=True is False, main_then_partial=False)
    assert HW.tail_shape(1, 6)["kst_le_d"] and HW.tail_shape(1, 6)["prologue"] == 3 and HW.tail_shape(1, 4)["kst_le_d"]
    assert HW.tail_shape(2, 6)["empty_main"] and HW.tail_shape(2, 6)["KST"] == 6 and HW.tail_shape(2, 6)["partial"] == 0
    sh = HW.tail_shape(5, 6)
    assert (sh["main_groups"], sh["tail_groups"], sh["partial"]) == (1, 2, 3)
    assert [HW.heads_nbuf(4, n, 37) for n in (1, 2, 3, 4)] == [6, 6, 4, 4] and [HW.heads_nbuf(8, n, 37) for n in (1, 2)] == [6, 4]
    assert HW.heads_nbuf(4, 4, 37, 0) == 2 and HW.heads_nbuf(8, 1, 65537 * 128) == 2
    assert HW.bank_waves(37 * 7, 7) == 1 and HW.bank_waves(133 * 7, 7) == 4 and HW.bank_waves(95, 1) == 1 and HW.bank_waves(96, 1) == 4
    groups, other = HW.head_groups({**HW.form_heads("narrow3", 19), **HW.form_heads("wide2", 19), **HW.form_heads("narrow1", 7),
                                    **HW.form_heads("generic130", 120), **HW.form_heads("rnn1", 2)})
    assert [(g["T"], g["ht"], g["n_nets"]) for g in groups] == [(19, 4, 3), (19, 8, 2), (7, 4, 1)]
    assert other == ["generic130_t120_0", "rnn1_t2_0"]


def test_bank_waves_mirror_against_the_routing_planner():
    """head_windows.bank_waves restates one line of owb::route (csrc/owwhip_bank_host.h); tests/planners_check.cpp prints what the
    planner itself chooses at both sides of the 96-entries-per-group edge, for one group and for two."""
    from test_planners_cpu import self_checks
    got = self_checks()
    for n, g in ((95, 1), (96, 1), (191, 2), (192, 2)):
        assert HW.bank_waves(n, g) == int(got[f"bank_wg_{n}_{g}"]), (n, g)
