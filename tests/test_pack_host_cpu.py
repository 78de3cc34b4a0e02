"""The host-side weight packer (openwakeword_amd/csrc/owwhip_pack.h) as a stand-alone host program under AddressSanitizer + UBSan.

tests/pack_check.cpp includes only that header: blob parsing, the operand-order packers, the f16-split scales, the scale ladder and
the image phases of oww_commit, none of which makes a HIP call.  This test writes the blobs of every case below with the package's
own builders, builds the program with ROCm's host clang++ (-fsanitize=address,undefined -fno-sanitize-recover=undefined; without
the sanitizers where a GPU is present, so that no sanitizer runs on a shared GPU machine), runs it as a process of its own -- it is
never loaded into Python -- and compares every printed field of every case with
tests/golden/pack_fingerprints.json.  No tolerance: return codes, error messages, FNV-1a-64 of the image bytes, every offset, every
scale exponent and the group tables must be equal.

The fingerprints were recorded from the commit named under "recorded_from", i.e. from BEFORE the packer moved into the header, when
it was reachable only through a committed handle.  Procedure: a scratch translation unit that #includes that commit's owwhip.hip
(packing makes no HIP call, so it runs without a GPU), defines the header's names as thin adapters over that commit's functions -- a
host-constructed oww_ctx filled from the input struct for the phases that took a handle, oww_load_* / oww_add_head on such a handle
for the parsers, the ladder lines of calibrate_hx verbatim -- and then #includes tests/pack_check.cpp unchanged (an empty
owwhip_pack.h in front of the include path); built with hipcc --offload-arch=gfx950 and run on the directory this test writes.  The
scratch unit is not part of the repository.  To record again after a deliberate layout change: run this file as a script with a
directory argument (PYTHONPATH: the repository root and tests/golden) to write the cases, run pack_check on it, and store the
lines (name -> rest of the line).
"""
import copy
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cases
from openwakeword_amd import weights as W
from openwakeword_amd.engine import pack_embedding_blob, pack_head_blob, pack_mel_blob, pack_vad_blob
from test_weight_regimes import _regime

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pack_fingerprints.json")
with open(GOLDEN) as _f:
    EXPECTED = json.load(_f)


def _const(name):
    with open(os.path.join(ROOT, "include", "owwhip.h")) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


def _hdr_patch(blob, field, value):
    b = np.array(blob, copy=True)
    b.view(np.int32)[field] = value
    return b


def _nan_at(blob, header_bytes, last):
    b = np.array(blob, copy=True).view(np.uint8).copy()
    f = b[header_bytes:].view(np.float32)
    f[-1 if last else 0] = np.nan
    return b


def write_cases(d):
    """Writes every blob and cases.txt into directory d."""
    lines = []

    def put(name, arr):
        np.ascontiguousarray(arr).view(np.uint8).tofile(os.path.join(d, name))
        return name

    seed = W.synthetic_embedding(cases.SEED_WEIGHTS)
    mel, emb = pack_mel_blob(), pack_embedding_blob(seed)
    put("mel.bin", mel), put("emb.bin", emb)
    r = np.random.default_rng(11)
    put("probe.bin", r.normal(0.0, 8.0, (16, 32, 96)).astype(np.float32))

    # ---- embedding: the four kernel families; f16-split on a fixed non-trivial ladder
    for fam in ("valu", "mfma", "rr", "hx"):
        lines.append(f"image emb_{fam} family={fam} ladder={int(fam == 'hx')}")
    put("emb_negbn.bin", pack_embedding_blob(_regime("negative_bn")[0]))              # the +-inf bound path of conv0's folded ReLU
    lines.append("image emb_hx_negative_bn family=hx ladder=1 emb=emb_negbn.bin")
    big = copy.deepcopy(seed)
    big["conv"][5] = (big["conv"][5] * 1e7).astype(np.float32)                        # folded weight beyond the f16 range: OWW_ERANGE, layer 5
    put("emb_big.bin", pack_embedding_blob(big))
    lines.append("image emb_hx_out_of_range family=hx ladder=1 emb=emb_big.bin")

    # ---- heads, one handle each
    wide = W.synthetic_head("timer", 3, T=16)
    head_sets = {
        "five_narrow": [W.synthetic_head(f"n{i}", 20 + i) for i in range(5)],       # f16-split group cap of four: two groups
        "h32_noln": [W.synthetic_head("h32", 5, hidden=32, layernorm=False)],         # eh folded into b1 / u1
        "gated": [W.synthetic_head("hey_jarvis", 6)],
        "t16_t28": [W.synthetic_head("a", 7), W.synthetic_head("b", 8, T=28)],        # separate groups
        "wide": [wide],                                                               # 128 x 7 softmax: ht 8
        "wide_off": [wide],                                                           # ... with the wide switch off: generic
        "h96_two_blocks": [W.synthetic_head("deep", 9, hidden=96, n_blocks=2)],       # generic
        "rnn": [W.synthetic_head("rnn", 10, kind="rnn", n_out=1)],
    }
    for name, heads in head_sets.items():
        files = ",".join(put(f"head_{name}_{i}.bin", pack_head_blob(h)) for i, h in enumerate(heads))
        nowide = int(name == "wide_off")
        lines.append(f"image heads_{name}_rr family=rr heads={files} nowide={nowide}")
        lines.append(f"image heads_{name}_hx_probe family=hx ladder=1 heads={files} nowide={nowide} probe=probe.bin")
        lines.append(f"image heads_{name}_hx_noprobe family=hx ladder=1 heads={files} nowide={nowide}")

    # ---- bank heads: the sequence of oww_bank_add (b3 in the pad block)
    put("bank_narrow.bin", pack_head_blob(W.synthetic_head("alexa", 12)))
    put("bank_wide.bin", pack_head_blob(W.synthetic_head("bw", 13, hidden=128)))
    for n in ("narrow", "wide"):
        lines.append(f"bank bank_{n}_probe bank_{n}.bin probe.bin")
        lines.append(f"bank bank_{n}_noprobe bank_{n}.bin -")

    # ---- VAD
    vad = W.synthetic_vad(cases.SEED_WEIGHTS)
    vad_blob = pack_vad_blob(vad)
    put("vad.bin", vad_blob)
    lines.append("image vad_hx family=hx ladder=1 vad=vad.bin")
    bad = copy.deepcopy(vad)
    bad["enc"][2][0][1, 3, 5] = 300.0                                                 # 2^8 * 300 leaves the f16 range: OWW_EINVAL
    put("vad_big.bin", pack_vad_blob(bad))
    lines.append("image vad_weight_300 family=hx ladder=1 vad=vad_big.bin")

    # ---- mel tables: the product blob rides in every image case; a bank where FFT bin 12 feeds three filters
    m3 = np.array(mel, copy=True)
    m3.view(np.int32)[400 + 5:400 + 8] = 12
    m3.view(np.float32)[432 + 5 * 16:432 + 8 * 16:16] = 0.5
    put("mel_three.bin", m3)
    lines.append("image mel_three_filters family=hx ladder=1 mel=mel_three.bin")

    # ---- scale ladder
    tiny = copy.deepcopy(seed)
    tiny["conv"][19] = (tiny["conv"][19] * 1e-4).astype(np.float32)
    put("emb_tiny.bin", pack_embedding_blob(tiny))
    typical = (0.37 * 1.9 ** (np.arange(20) % 7) * (1 + np.arange(20))).astype(np.float32)
    zero = typical.copy(); zero[9] = 0.0
    clamp = typical.copy(); clamp[4], clamp[5], clamp[6] = 1e-30, 1e30, 3e38          # +100 at layer 4, -100 at layer 6
    put("absmax_typical.bin", typical), put("absmax_zero.bin", zero), put("absmax_clamp.bin", clamp)
    for n in ("typical", "zero", "clamp"):
        lines.append(f"ladder ladder_{n} absmax_{n}.bin emb.bin")
    lines.append("ladder ladder_tiny_last_layer absmax_typical.bin emb_tiny.bin")

    # ---- malformed blobs, every kind
    head = pack_head_blob(W.synthetic_head("m", 14, hidden=32))
    rnn = pack_head_blob(W.synthetic_head("rnn", 10, kind="rnn", n_out=1))
    kinds = {"mel": (mel, 0), "emb": (emb, 0), "head": (head, 32), "rnn": (rnn, 32), "vad": (vad_blob, 32)}
    for k, (blob, hdr) in kinds.items():
        raw = np.ascontiguousarray(blob).view(np.uint8)
        pk = "head" if k == "rnn" else k
        lines.append(f"parse parse_{k}_ok {pk} " + put(f"p_{k}_ok.bin", raw))
        lines.append(f"parse parse_{k}_minus4 {pk} " + put(f"p_{k}_m4.bin", raw[:-4]))
        lines.append(f"parse parse_{k}_plus4 {pk} " + put(f"p_{k}_p4.bin", np.concatenate([raw, np.zeros(4, np.uint8)])))
        lines.append(f"parse parse_{k}_nan_first {pk} " + put(f"p_{k}_nan0.bin", _nan_at(raw, hdr, False)))
        lines.append(f"parse parse_{k}_nan_last {pk} " + put(f"p_{k}_nan1.bin", _nan_at(raw, hdr, True)))
    max_blocks = _const("OWW_MAX_HEAD_BLOCKS")
    for tag, field, value in [("kind4", 0, 4), ("T0", 1, 0), ("T121", 1, 121), ("hidden0", 2, 0), ("hidden513", 2, 513),
                              ("nout0", 3, 0), ("nout9", 3, 9), ("blocks", 5, max_blocks)]:
        lines.append(f"parse parse_head_{tag} head " + put(f"p_head_{tag}.bin", _hdr_patch(head, field, value)))
    for tag, field, value in [("T65", 1, 65), ("hidden65", 2, 65), ("ln", 4, 1)]:      # RNN_TMAX = RNN_H = 64
        lines.append(f"parse parse_rnn_{tag} head " + put(f"p_rnn_{tag}.bin", _hdr_patch(rnn, field, value)))

    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return [ln.split()[1] for ln in lines]


def _host_clangxx():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    return cxx if os.path.exists(cxx) else None


@pytest.fixture(scope="module")
def produced(tmp_path_factory):
    cxx = _host_clangxx()
    if cxx is None:
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    d = tmp_path_factory.mktemp("pack_check")
    names = write_cases(str(d))
    exe = str(d / "pack_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *sanitize, os.path.join(ROOT, "tests", "pack_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    run = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"pack_check exit {run.returncode}:\n{run.stderr[-4000:]}"
    got = dict(ln.split(" ", 1) for ln in run.stdout.splitlines())
    return names, got


def test_every_case_ran_and_none_is_missing_from_the_golden_file(produced):
    names, got = produced
    assert sorted(got) == sorted(names) == sorted(EXPECTED["cases"])
    assert re.fullmatch(r"[0-9a-f]{40}", EXPECTED["recorded_from"])


@pytest.mark.parametrize("name", sorted(EXPECTED["cases"]))
def test_fingerprint_equals_the_parent_commits(produced, name):
    _names, got = produced
    want = EXPECTED["cases"][name]
    if got[name] != want:                                    # field by field, so that the report names what moved
        g, w = got[name].split(" "), want.split(" ")
        diff = [(a, b) for a, b in zip(g, w) if a != b] or [(len(g), len(w))]
        pytest.fail(f"{name}: {len(diff)} field(s) differ, first (got, recorded): {diff[:4]}")


def test_expected_outcomes_of_the_refusal_cases():
    """What the recorded lines must say whatever commit they came from: the refusals carry the documented code and name their cause."""
    c = EXPECTED["cases"]
    assert c["emb_hx_out_of_range"].startswith("rc=-5 ") and "conv_layer_5:" in c["emb_hx_out_of_range"]
    assert c["vad_weight_300"].startswith("rc=-1 ") and "VAD_encoder" in c["vad_weight_300"]
    assert c["mel_three_filters"].startswith("rc=-1 ") and "FFT_bin_12_feeds_more_than_two" in c["mel_three_filters"]
    refused = [n for n in c if n.startswith("parse_") and not n.endswith("_ok") and "_nan_" not in n]
    assert len(refused) == 5 * 2 + 8 + 3
    for name in refused:                                     # nbytes +- 4 of every kind, every header field one step outside its range
        assert c[name].startswith("rc=-1 untouched=1 "), (name, c[name])
    for k in ("emb", "head", "rnn"):
        for at in ("first", "last"):
            assert c[f"parse_{k}_nan_{at}"].startswith("rc=-1 untouched=1 ") and "not_finite" in c[f"parse_{k}_nan_{at}"]
    assert "groups={T=16 NH=256 n=4 ht=4" in c["heads_five_narrow_hx_probe"] and c["heads_five_narrow_hx_probe"].count("{T=16") == 2
    assert c["heads_t16_t28_hx_probe"].count("{T=") == 2 and "ht=8" in c["heads_wide_hx_probe"]
    assert "groups= generic=0," in c["heads_wide_off_hx_probe"] and "groups= generic=0," in c["heads_h96_two_blocks_hx_probe"]
    assert "rnn=0," in c["heads_rnn_hx_probe"] and "eh=0 " not in c["heads_h32_noln_hx_probe"].split("groups=")[1]


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    print("\n".join(write_cases(sys.argv[1])))
