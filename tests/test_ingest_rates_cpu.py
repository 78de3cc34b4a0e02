"""The stream ingest at every served rate and class table, without a GPU (tests/ingest_rates.py holds the table): the table reaches
every branch of `ingest_stream` and every class of the server's own default table; a numpy float32 restatement of the kernel's chain,
fed every message plan with the history carried as int16, holds the derived budget `0.5 + gamma * A` of tests/resample_ref.py at the
new rates and tap counts; six deliberately wrong streams do not, each at a named class; and the Python mirror of the launch arithmetic
equals what openwakeword_amd/csrc/owwhip_ingest.h itself derives, printed by a stand-alone program under AddressSanitizer + UBSan
(tests/ingest_rates_check.cpp), which also prints the staging edge at 96 kHz the device tier uses."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytest.importorskip("aiohttp")                                          # (ingest_rates takes the rates from openwakeword_amd.serve, which needs it)
import ingest_rates as IR  # noqa: E402
from openwakeword_amd import resample as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EDGE96 = IR.EDGE96


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def _reached():
    """every (class, plan, message) of the table with its geometry"""
    for c in IR.CLASSES:
        for name, sizes in IR.MESSAGE_PLANS[c].items():
            for n_in in sorted(set(sizes)):
                yield c, name, IR.geometry_n_in(*c, n_in)


def test_the_table_covers_the_servers_default_classes():
    pytest.importorskip("aiohttp")
    served = IR.server_default_classes()
    assert len(served) == 13 and len(set(served)) == 13
    missing = [c for c in served if c not in IR.CLASSES or "six" not in IR.MESSAGE_PLANS[c]]
    assert not missing, f"classes of FanInServer's default table without a case: {missing}"
    assert R.class_row_bytes(served) == 15360


def test_the_table_reaches_every_branch():
    seen = list(_reached())

    def some(pred, what):
        hits = [(c, name, g["n_in"]) for c, name, g in seen if pred(c, g)]
        assert hits, f"no case reaches: {what}"
        return hits

    for q in (2, 4, 8):
        some(lambda c, g: g["slide"] and g["q"] == q and c[1] == "pcm16", f"the sliding form at q = {q} with PCM16")
        some(lambda c, g: g["slide"] and g["q"] == q and c[1] == "pcm16" and g["n_tiles"] > 1, f"the sliding form at q = {q} across a tile edge")
    for q in (2, 4):
        some(lambda c, g: g["slide"] and g["q"] == q and c[1] != "pcm16", f"the sliding form at q = {q} with G.711")
    for c in IR.CLASSES:                                                      # (a tile edge inside a group of four: x0 != 0)
        if IR.geometry(*c)["slide"] and IR.geometry(*c)["q"] in (4, 8):
            assert IR.geometry(*c)["x0"] % 4 != 0 and "tile_edge" in IR.MESSAGE_PLANS[c]
    some(lambda c, g: g["p"] == 3 and g["q"] == 4 and not g["slide"], "q = 4 outside the sliding form (12 kHz)")
    some(lambda c, g: g["q"] == 1 and g["n_taps"] and not g["slide"], "q = 1 outside the sliding form")
    some(lambda c, g: g["ntp_is_n_taps"], "ntp == n_taps: a row without zero padding")
    some(lambda c, g: g["n_taps"] and g["ntp"] == g["n_taps"] + 2, "ntp == n_taps + 2")
    some(lambda c, g: not g["n_taps"], "decode only")
    for enc in ("pcm16", "ulaw", "alaw"):
        some(lambda c, g: c[1] == enc and g["vec_in"], f"16-byte loads of {enc}")
        some(lambda c, g: c[1] == enc and not g["vec_in"], f"element-wise loads of {enc}")
    some(lambda c, g: c == (22050, "pcm16") and not g["vec_in"] and g["n_in"] == 1764, "the 3,528-byte frame at 22.05 kHz: element-wise loads")
    some(lambda c, g: g["vec_out"], "16-byte stores")
    some(lambda c, g: not g["vec_out"], "element-wise stores")
    some(lambda c, g: g["n_tiles"] == 1, "one tile")
    some(lambda c, g: g["n_tiles"] > 1 and not g["slide"], "more than one tile in the general form")
    some(lambda c, g: g["short"] and g["H"] >= 77 and c[0] == 48000, "n_in < H at 48 kHz")
    some(lambda c, g: g["short"] and g["H"] == 153 and c[0] == 96000, "n_in < H at 96 kHz, the longest history")
    some(lambda c, g: g["short"] and g["slide"], "n_in < H in the sliding form")
    some(lambda c, g: g["n_taps"] == 154 and g["n_in"] == 15360 and g["n_tiles"] == 2, "two frames at 96 kHz: 15,360 in, 2,560 out, two tiles")
    assert not [x for x in seen if x[2]["refused"]], "a plan holds a message that does not stage"
    assert all(g["taps_in_lds"] for _, _, g in seen if g["n_taps"])
    for rate in (88200, 96000):                                               # six frames in one message do not stage there
        assert IR.geometry_n_in(rate, "pcm16", 6 * IR.frame(rate))["refused"] and len(IR.MESSAGE_PLANS[(rate, "pcm16")]["whole"]) == 2
    assert not IR.geometry_n_in(96000, "pcm16", EDGE96[0])["refused"] and IR.geometry_n_in(96000, "pcm16", EDGE96[1])["refused"]


# ---- the host's own arithmetic -----------------------------------------------------------------------------------------------------------
def test_the_mirror_equals_owwhip_ingest_h_under_the_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    exe = str(tmp_path / "ingest_rates_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *sanitize, os.path.join(ROOT, "tests", "ingest_rates_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    cases = {}
    for c, _, g in _reached():
        cases[f"{R.ENCODINGS[c[1]]}:{g['p']}:{g['q']}:{g['n_taps']}:{g['n_in']}"] = (c, g)
    for n_in in EDGE96 + (6 * IR.frame(96000),):                              # the edge itself, and the six frames that do not stage
        cases[f"0:6:1:154:{n_in}"] = ((96000, "pcm16"), IR.geometry_n_in(96000, "pcm16", n_in))
    run = subprocess.run([exe, *cases], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    got = dict(ln.split(" ", 1) for ln in run.stdout.splitlines())
    assert got["edge96"].startswith(f"last={EDGE96[0]} first={EDGE96[1]} ") and "LDS" in got["edge96"]
    for key, (c, g) in cases.items():
        bps = 2 if c[1] == "pcm16" else 1
        if g["refused"]:
            assert got[key].startswith(f"rc=-1 slide={g['slide']} ntp={g['ntp']} Hpad={g['Hpad']} ") and " single_rc=-1 " in got[key], (key, got[key])
            continue
        lds = g["lds_with_taps"] if g["taps_in_lds"] else g["lds_bare"]
        want = (f"rc=0 slide={g['slide']} ntp={g['ntp']} Hpad={g['Hpad']} xs_len={g['xs_len']} stage={g['stage']} lds_bare={g['lds_bare']} "
                f"lds_with_taps={g['lds_with_taps']} taps_in_lds={g['taps_in_lds']} single_rc=0 n_out={g['n_out']} lds={lds} row={g['n_in'] * bps}")
        assert got[key] == want, f"{c}, n_in = {g['n_in']}:\n  library {got[key]}\n  mirror  {want}"


# ---- admission: a correct fp32 chain holds the budget ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,enc", IR.CLASSES)
def test_the_fp32_chain_holds_the_budget_in_every_plan(rate, enc):
    six = IR.emulate(rate, enc, IR.MESSAGE_PLANS[(rate, enc)]["six"])
    assert six.shape == (IR.S, IR.TOTAL) and six.dtype == np.int16
    for name, sizes in IR.MESSAGE_PLANS[(rate, enc)].items():
        got = six if name == "six" else IR.emulate(rate, enc, sizes)
        assert (got == six[:, :got.shape[1]]).all(), f"plan {name}: the cut changes the emulation's bits"
        over, worst = IR.holds_budget(got, rate, enc)
        assert (over <= 0).all(), f"plan {name}: {int((over > 0).sum())} outputs outside 0.5 + gamma*A, worst by {over.max():.3f} LSB " \
                                  f"(worst share of the allowance {worst:.3f})"
    if IR.params(rate, enc)[3]:
        assert (six != 0).any(axis=1).sum() >= IR.S - 2                       # (every row but silence and, where its tap rounds to 0, the last impulse)


# ---- the budget rejects wrong streams: the class and plan that catch each -------------------------------------------------------------------
CAUGHT_BY = {
    "history_dropped": [((96000, "pcm16"), "six"), ((22050, "pcm16"), "half")],
    "history_shifted": [((88200, "pcm16"), "whole"), ((4000, "ulaw"), "half")],
    "phase_plus_one": [((12000, "pcm16"), "six"), ((24000, "pcm16"), "tiny")],
    "last_tap_skipped": [((22050, "pcm16"), "six")],
    "tile_edge_group": [((4000, "pcm16"), "tile_edge"), ((2000, "pcm16"), "tile_edge")],
    "history_not_moved_down": [((96000, "pcm16"), "short_history"), ((48000, "pcm16"), "short_history")],
}


@pytest.mark.parametrize("mutation", IR.MUTATIONS)
def test_the_budget_rejects_a_wrong_stream(mutation):
    assert set(CAUGHT_BY) == set(IR.MUTATIONS)
    for c, plan in CAUGHT_BY[mutation]:
        sizes = IR.MESSAGE_PLANS[c][plan]
        good, _ = IR.holds_budget(IR.emulate(*c, sizes), *c)
        bad, _ = IR.holds_budget(IR.emulate(*c, sizes, mutation), *c)
        assert (good <= 0).all()
        assert (bad > 0).any(), f"{mutation}: class {c}, plan {plan} stays inside 0.5 + gamma*A"
