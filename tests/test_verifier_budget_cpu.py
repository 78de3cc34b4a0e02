"""CPU tier of the custom-verifier suite: every number tests/test_verifier_regimes.py spends on the device is derived and guarded here,
on oracle.oww_oracle feature rows and never on a device result (tests/verifier_budget.py has the definitions; DESIGN.md 5.24 the
figures; pytest -s prints them)."""
import functools
import warnings

import numpy as np
import pytest

from openwakeword_amd.model import VerifierFoldWarning, fold_verifier, verifier_fold_deviation

import verifier_budget as VB
from verifier_fixture import trained_verifier

TEETH = 100.0            # a fault moves the score by this many budgets ...
TEETH_SHARE = 0.90       # ... in this share of the windows with |z64| <= Z_SEEN
Z_SEEN = 4.0
SEEN_SHARE = 0.80
MIN_WINDOWS = 200


@functools.lru_cache(maxsize=None)
def _case(regime, T, data="oracle"):
    """(rings or None, windows X, triple, w, b) of a regime at T: on the oracle rings, or -- `lowvar` only -- on their near-constant
    form."""
    rings = VB.oracle_rings(VB.ring_rows(T))
    X = VB.windows(rings, T)
    if data == "near_constant":
        X, rings = VB.near_constant(X), None
    assert X.shape[0] >= MIN_WINDOWS, X.shape
    t = VB.triple(regime, T, X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", VerifierFoldWarning)
        w, b = VB.folded(t)
    return rings, X, t, w, b


CASES = [(r, T, "oracle") for r in VB.REGIMES for T in VB.T_VALUES] + [("lowvar", T, "near_constant") for T in VB.T_VALUES]


def test_e32_and_a_are_the_measured_envelope():
    """E32[T] = max |z_restate32 - z_ref64| / kappa and A = max |score_restate32 - sigmoid64(z_restate32)| over every case; each
    frozen constant is at least its measurement and at most twice it."""
    e32 = {T: 0.0 for T in VB.T_VALUES}
    a = 0.0
    for regime, T, data in CASES:
        _, X, _, w, b = _case(regime, T, data)
        z32, s32 = VB.restate32(X, w, b)
        z64, _, kappa = VB.ref64(X, w, b)
        e = float(np.max(np.abs(z32.astype(np.float64) - z64) / kappa))
        e32[T] = max(e32[T], e)
        a = max(a, float(np.max(np.abs(s32.astype(np.float64) - VB.sigmoid64(z32)))))
        print(f"{regime:12s} {data:13s} T={T:3d} E32 = {e / VB.U24:.3f} x 2^-24   max |score32 - score64| = "
              f"{float(np.max(np.abs(s32 - VB.ref64(X, w, b)[1]))):.2e}  median kappa = {float(np.median(kappa)):.1f}")
    print("E32 / 2^-24:", {T: round(v / VB.U24, 4) for T, v in e32.items()}, " A:", a)
    for T in VB.T_VALUES:
        assert e32[T] <= VB.E32[T] <= 2 * e32[T], (T, e32[T], VB.E32[T])
    assert a <= VB.A <= 2 * a, (a, VB.A)


@pytest.mark.parametrize("regime", [r for r in VB.REGIMES if r != "reference"])
def test_no_blind_comparisons(regime):
    for T in VB.T_VALUES:
        _, X, _, w, b = _case(regime, T)
        z64 = VB.ref64(X, w, b)[0]
        share = float(np.mean(np.abs(z64) <= Z_SEEN))
        print(f"{regime} T={T}: {share:.3f} of {X.shape[0]} windows have |z64| <= {Z_SEEN}")
        assert share >= SEEN_SHARE, (regime, T, share)


def _fault_moves(regime, T):
    """fault -> (share of the seen windows the fault moves by >= TEETH budgets -- float64 alone, and on the restatement --, median move
    in budgets)."""
    rings, X, _, w, b = _case(regime, T)
    z64, s64, kappa = VB.ref64(X, w, b)
    seen = np.abs(z64) <= Z_SEEN
    bud = VB.budget(T, kappa)
    out = {}
    for fault in VB.FAULTS:
        xf, wf, bf = VB.faulty(fault, rings, T, w, b)
        ref_move = np.abs(VB.ref64(xf, wf, bf)[1] - s64) / bud
        got_move = np.abs(VB.restate32(xf, wf, bf)[1].astype(np.float64) - s64) / bud
        out[fault] = (float(np.mean(ref_move[seen] >= TEETH)), float(np.mean(got_move[seen] >= TEETH)), float(np.median(got_move[seen])))
    return out


@pytest.mark.parametrize("T", [T for T in VB.T_VALUES if T > 1])
@pytest.mark.parametrize("regime", [r for r in VB.REGIMES if r != "reference"])
def test_every_fault_moves_the_score_by_a_hundred_budgets(regime, T):
    """Each fault of VB.FAULTS, applied to the restatement, leaves the float64 reference by >= 100 budgets in >= 90 % of the windows
    with |z64| <= 4.  That the inputs can show it is asserted on the float64 reference alone first."""
    for fault, (ref_share, got_share, med) in _fault_moves(regime, T).items():
        print(f"{regime:12s} T={T:3d} {fault:9s}: float64 {ref_share:.3f}, restatement {got_share:.3f} of the seen windows move >= "
              f"{TEETH:.0f} budgets (median {med:.0f})")
        assert ref_share >= TEETH_SHARE, ("the inputs cannot show this fault", regime, T, fault, ref_share)
        assert got_share >= TEETH_SHARE, (regime, T, fault, got_share)


def test_reference_regime_sees_little():
    """Not an assertion on the fixture's verifier, a record: how many budgets the same faults move it -- the reason the
    other regimes exist."""
    for T in VB.T_VALUES[1:]:
        for fault, (ref_share, got_share, med) in _fault_moves("reference", T).items():
            print(f"reference    T={T:3d} {fault:9s}: {got_share:.3f} of the windows move >= {TEETH:.0f} budgets (median {med:.1f})")
            assert 0.0 <= got_share <= 1.0
        rings, X, _, w, b = _case("reference", T)
        s64 = VB.ref64(X, w, b)[1]
        for fault in VB.FAULTS:
            move = np.abs(VB.ref64(*VB.faulty(fault, rings, T, w, b))[1] - s64)
            print(f"reference    T={T:3d} {fault:9s}: |score move| median {np.median(move):.2e}, {np.mean(move <= 1e-4):.3f} of the windows "
                  f"stay inside the flat 1e-4")


@pytest.mark.parametrize("regime,T,data", CASES)
def test_fold_stays_within_its_rounding(regime, T, data):
    """The folded fp32 map evaluated in float64 against the unfolded pipeline in float64: within 4 * 2^-24 * kappa_hat in the logit."""
    _, X, t, w, b = _case(regime, T, data)
    z_fold = VB.ref64(X, w, b)[0]
    z_pipe = VB.pipeline_logit(t, X)
    kh = VB.kappa_hat(t, w, b)
    dz = float(np.max(np.abs(z_fold - z_pipe)))
    ds = float(np.max(np.abs(VB.sigmoid64(z_fold) - VB.sigmoid64(z_pipe))))
    print(f"{regime:12s} {data:13s} T={T:3d} kappa_hat = {kh:9.1f}  |dz| = {dz:.2e} ({dz / (VB.U24 * kh):.2f} x 2^-24 kappa_hat)  "
          f"|dscore| = {ds:.2e}  predicted device deviation = {verifier_fold_deviation(w, b, t.mean, t.scale)[0]:.2e}")
    assert dz <= 4 * VB.U24 * kh, (regime, T, dz, kh)


def test_fold_warning():
    """fold_verifier warns where the predicted deviation of the device score from the pipeline leaves the 1e-4 score class.  `lowvar`
    on data that holds its near-constant columns warns at every T and names those columns; at T <= 34 no other regime does, nor does
    `lowvar` on the oracle rows, which hold no such column; the fixture and a ready pair never warn.  At T = 120 the dense regimes
    `offset` and `alternating` warn as well: 11,520 features whose mean is four to five times their spread carry a mass near 2,000
    at a logit spread of 2, and their device budget is above 1e-4 too.  Where the scaler was fitted to the data
    (`offset`, `lowvar`), silence means that the case's largest device budget plus the fold's rounding bound is inside the class;
    kappa_hat says nothing about data far from the scaler's mean_ (`unit` at T = 120: silent at 9.2e-5, budget 1.3e-4)."""
    for regime, T, data in CASES:
        _, X, t, _, _ = _case(regime, T, data)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            w, b = fold_verifier(VB.Pipeline(t))
            w2, b2 = fold_verifier((w, b))
        rec = [r for r in rec if issubclass(r.category, VerifierFoldWarning)]
        pred, kh, worst = verifier_fold_deviation(w, b, t.mean, t.scale)
        assert len(rec) == int(pred > 1e-4), (regime, T, data, pred)
        assert kh == pytest.approx(VB.kappa_hat(t, w, b))
        if (regime, data) == ("lowvar", "near_constant"):
            assert len(rec) == 1, (regime, T, data)
            msg = str(rec[0].message)
            assert all(str(int(i)) in msg for i in worst), (msg, worst)
            assert all(VB.lowvar_columns(T * VB.EMB)[worst])
        elif T <= 34:
            assert not rec, (regime, T, [str(r.message) for r in rec])
        else:
            print(f"{regime:12s} T={T}: predicted {pred:.2e}, {'warns' if rec else 'silent'}")
        if not rec and regime in ("offset", "lowvar"):       # (kappa_hat speaks of data the scaler was fitted to: these two regimes)
            spent = float(np.max(VB.budget(T, VB.ref64(X, w, b)[2]))) + 0.25 * 4 * VB.U24 * kh
            assert spent <= 1e-4, (regime, T, data, spent)
        with warnings.catch_warnings():          # the fold's result does not depend on the warning
            warnings.simplefilter("ignore")
            w3, b3 = fold_verifier(VB.Pipeline(t))
        assert np.array_equal(w, w3) and b == b3 and np.array_equal(w, w2) and b == b2
    with warnings.catch_warnings():
        warnings.simplefilter("error", VerifierFoldWarning)
        for seed in range(3):
            fold_verifier(trained_verifier(seed))
        fold_verifier((np.full(16 * 96, 1e6, np.float32), -1e9))


def test_model_constant_is_the_budget_s():
    from openwakeword_amd import model
    assert model.VERIFIER_E32 * VB.U24 == max(VB.E32.values())


# ------------------------------------------------------------------------------------------------ the pair list
def _layout(S, NL, K):
    return (np.full((S, NL), VB.DEFAULT), np.zeros((S, NL), np.float32), np.full((S, K), VB.DEFAULT), np.zeros((S, K), np.float32))


def test_pair_list_mirror():
    """sv_list reproduces the order of owwhip_verifier_host.h::sv_list, and the list shapes of the GPU tier put the entries where its cases say."""
    L = VB
    for n in L.ENTRY_COUNTS:
        lay = L.count_layout(n)
        ents = lay.entries()
        assert len(ents) == n
        assert VB.n_waves(n) == -(-n // 16) and VB.n_workgroups(n) == -(-n // 64)
        assert [(e.s, e.col < 0, e.col if e.col >= 0 else ~e.col) for e in ents] == \
            sorted((e.s, e.col < 0, e.col if e.col >= 0 else ~e.col) for e in ents)       # stream-major, columns before slots
    # every pair at the default: no list at all, whatever handle-wide verifiers exist
    fix, fthr, bank, bthr = _layout(4, 2, 1)
    assert VB.sv_list(fix, fthr, bank, bthr, {}, [16, 0], [0.5, 0.0]) == []
    # one NONE switches the list on; the handle-wide verifier then appears as a default entry of every other stream
    fix[1, 0] = VB.NONE
    ents = VB.sv_list(fix, fthr, bank, bthr, {}, [16, 0], [0.5, 0.0])
    assert [(e.s, e.col, e.v, e.T, e.thr) for e in ents] == [(0, 0, ~0, 16, 0.5), (2, 0, ~0, 16, 0.5), (3, 0, ~0, 16, 0.5)]
    # the mixed layout: one wave holds all four kinds of entry and three window lengths; one wave hits on every entry, one on none
    lay = L.mixed_layout()
    ents = lay.entries()
    kinds = lambda es: {("bank" if e.col < 0 else "default" if e.v < 0 else "pool") for e in es}
    wave = [e for i, e in enumerate(ents) if VB.wave_of(i) == L.MIXED_WAVE]
    assert len(wave) == 16 and kinds(wave) == {"bank", "default", "pool"} and len({e.T for e in wave}) == 3
    assert {e.col for e in wave if e.col >= 0 and e.v >= 0} and {e.col for e in wave if e.col >= 0 and e.v < 0}
    hit_all = [e for i, e in enumerate(ents) if VB.wave_of(i) == L.ALL_HIT_WAVE]
    hit_none = [e for i, e in enumerate(ents) if VB.wave_of(i) == L.NO_HIT_WAVE]
    assert len(hit_all) == 16 and all(e.thr == 0.0 for e in hit_all)
    assert len(hit_none) == 16 and all(e.thr == 1.5 for e in hit_none)
    off = L.MASK_OFF
    assert 0 < sum(e.s in off for e in wave) < 16          # the masked step switches off some entries of the mixed wave, not all


def _case_text(name, fix, fix_thr, bank, bank_thr, pool_T, ver_T, ver_thr):
    """One case in the format tests/planners_check.cpp reads: thresholds as bit patterns."""
    fix, bank = np.asarray(fix), np.asarray(bank)
    pool = [pool_T.get(i, 0) for i in range(max(pool_T, default=-1) + 1)]
    hexes = lambda a: " ".join("%08x" % int(b) for b in np.asarray(a, np.float32).reshape(-1).view(np.uint32))      # noqa: E731
    ints = lambda a: " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))                                        # noqa: E731
    return "\n".join([f"case {name} {fix.shape[0]} {fix.shape[1]} {bank.shape[1]} {len(pool)} {len(ver_T)}", ints(fix), hexes(fix_thr), ints(bank),
                      hexes(bank_thr), ints(pool), ints(ver_T), hexes(ver_thr)]) + "\n"


def test_pair_list_mirror_against_the_library_header(tmp_path):
    """verifier_budget.sv_list against owsv::sv_list (csrc/owwhip_verifier_host.h), which the library uploads: the tables of the cases
    above and of the GPU tier's handle HL through tests/planners_check.cpp, entries compared field by field, thresholds by bit
    pattern.  So the GPU tier's argument about which entries share a wave rests on the list the device really walks."""
    from test_planners_cpu import run_planners
    cases = {}
    fix, fthr, bank, bthr = _layout(4, 2, 1)
    cases["all_default"] = (fix.copy(), fthr, bank, bthr, {}, [16, 0], [0.5, 0.0])
    fix[1, 0] = VB.NONE                          # NONE on a column that has a handle-wide verifier; column 1's has T = 0 under DEFAULT
    cases["one_none"] = (fix.copy(), fthr, bank, bthr, {}, [16, 0], [0.5, 0.0])
    cases["no_handle_wide"] = (fix.copy(), fthr, bank, bthr, {}, [], [])
    f0, t0, b0, bt0 = _layout(5, 2, 0)           # K = 0
    f0[2, 1], t0[2, 1], f0[4, 0] = 1, np.float32(0.3), VB.NONE
    cases["no_bank"] = (f0, t0, b0, bt0, {0: 16, 1: 5}, [16, 5], [0.25, np.float32(0.1)])
    for n in VB.ENTRY_COUNTS:
        lay = VB.count_layout(n, (0.5, 0.25, 0.75))
        cases[f"count_{n}"] = (lay.fix, lay.fix_thr, lay.bank, lay.bank_thr, VB.HL_POOL, lay.ver_T, lay.ver_thr)
    lay = VB.mixed_layout(0.4)
    cases["mixed"] = (lay.fix, lay.fix_thr, lay.bank, lay.bank_thr, VB.HL_POOL, lay.ver_T, lay.ver_thr)
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case_text(name, *c) for name, c in cases.items()))
    got, cur = {}, None
    for ln in run_planners("verifier", str(path)):
        tok = ln.split()
        if tok[0] == "case":
            cur = got.setdefault(tok[1], [])
            assert int(tok[2]) >= 0
        else:
            cur.append((int(tok[1]), int(tok[2]), int(tok[3]), int(tok[4]), int(tok[5], 16)))
    assert list(got) == list(cases)
    for name, c in cases.items():
        want = [(e.s, e.col, e.T, e.v, int(np.float32(e.thr).view(np.uint32))) for e in VB.sv_list(*c)]
        assert got[name] == want, name
    assert got["all_default"] == [] and len(got["one_none"]) == 3 and got["no_handle_wide"] == [] and len(got["mixed"]) == 63
    assert [len(got[f"count_{n}"]) for n in VB.ENTRY_COUNTS] == list(VB.ENTRY_COUNTS)
    assert got["no_bank"][4:6] == [(2, 0, 16, ~0, int(np.float32(0.25).view(np.uint32))), (2, 1, 5, 1, int(np.float32(0.3).view(np.uint32)))]
