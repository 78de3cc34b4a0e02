"""Detection events without a GPU (include/owwhip.h: oww_events_*): the record layout a C caller and the numpy dtype agree on, the
definition of an event restated on host arrays (engine.events_from_scores), argument errors as codes, keyword validation."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from openwakeword_amd import _lib, engine
from openwakeword_amd.engine import EVENT_DTYPE, events_from_scores
from openwakeword_amd.model import BatchedModel

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIELDS = ["stream", "column", "bank_id", "score", "frame", "feature_index", "reserved"]


def test_event_record_layout_matches_the_numpy_dtype(tmp_path):
    """oww_event compiled as C99 from the header: 32 bytes, and every field where EVENT_DTYPE puts it."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "event_layout.c"
    src.write_text('#include <stdio.h>\n#include "owwhip.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(oww_event));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(oww_event, {f}));\n' for f in FIELDS)
                   + '  printf("abi %d classes %d\\n", OWW_ABI_VERSION, OWW_N_KERNEL_CLASSES);\n  return 0;\n}\n')
    exe = tmp_path / "event_layout"
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == 32 == EVENT_DTYPE.itemsize
    assert list(EVENT_DTYPE.names) == FIELDS
    for f in FIELDS:
        assert int(out[f]) == EVENT_DTYPE.fields[f][1], f
    assert EVENT_DTYPE["score"] == np.float32 and EVENT_DTYPE["frame"] == np.uint32 and EVENT_DTYPE["reserved"].shape == (2,)
    assert out["abi"].split() == ["6", "classes", "10"]                     # additive: neither constant moved


def test_events_from_scores_order_and_equality():
    """Ascending stream; fixed columns first, ascending; then slots, ascending; `>=` holds at equality."""
    half = np.float32(0.5)
    scores = np.array([[0.9, 0.1, 0.5],
                       [0.0, 0.0, 0.0],
                       [0.2, 0.7, np.nextafter(half, np.float32(0))]], dtype=np.float32)
    bank = np.array([[0.6, 0.8], [0.9, 0.2], [0.5, 0.5]], dtype=np.float32)
    sub = np.array([[7, 3], [4, 4], [9, 2]])
    got = events_from_scores(scores, bank, sub, 0.5, 0.5)
    assert [(s, c, b) for s, c, b, _ in got] == [(0, 0, -1), (0, 2, -1), (0, ~0, 7), (0, ~1, 3), (1, ~0, 4), (2, 1, -1), (2, ~0, 9), (2, ~1, 2)]
    assert [v for *_, v in got] == [scores[0, 0], scores[0, 2], bank[0, 0], bank[0, 1], bank[1, 0], scores[2, 1], bank[2, 0], bank[2, 1]]
    assert all(isinstance(v, np.float32) for *_, v in got)
    # per-column thresholds; one ulp below the threshold is no hit
    got = events_from_scores(scores, None, None, [0.95, 0.7, half], 0.5)
    assert [(s, c) for s, c, _, _ in got] == [(0, 2), (2, 1)]


def test_events_from_scores_nan_masked_and_empty_slots():
    scores = np.array([[0.9, 0.9], [0.9, 0.9], [0.9, 0.9]], dtype=np.float32)
    bank = np.full((3, 2), 0.99, dtype=np.float32)
    sub = np.array([[-1, 5], [5, -1], [-1, -1]])
    # a NaN threshold silences the column; a stream that sat out reports nothing although its row is above the threshold; an
    # unsubscribed slot never reports although its score cell is
    got = events_from_scores(scores, bank, sub, [np.nan, 0.5], 0.5, participating=[1, 0, 1])
    assert [(s, c, b) for s, c, b, _ in got] == [(0, 1, -1), (0, ~1, 5), (2, 1, -1)]
    assert events_from_scores(scores, bank, sub, 0.5, 0.5, participating=[0, 0, 0]) == []
    assert events_from_scores(scores, bank, sub, np.nan, np.nan) == []
    # bank only (no fixed heads), and fixed only
    got = events_from_scores(None, bank, sub, (), 0.5)
    assert [(s, c, b) for s, c, b, _ in got] == [(0, ~1, 5), (1, ~0, 5)]
    assert len(events_from_scores(scores)) == 6
    with pytest.raises(ValueError):
        events_from_scores(scores, bank, None)
    with pytest.raises(ValueError):
        events_from_scores(scores, bank, sub, participating=[1, 1])


def test_argument_errors_surface_as_codes_on_a_null_handle():
    lib = _lib.load()
    n = C.c_int32(7)
    rec = np.zeros(4, dtype=EVENT_DTYPE)
    out = np.zeros(96, dtype=np.float32)
    assert lib.oww_events_configure(None, 16, 0) == -1 and b"oww_events_configure" in lib.oww_last_error()
    assert lib.oww_events_set_thresholds(None, None, 0.5) == -1
    assert lib.oww_get_events(None, rec.ctypes.data_as(C.c_void_p), 4, C.byref(n), C.byref(n)) == -1
    assert lib.oww_get_event_features(None, 0, 1, out.ctypes.data_as(C.c_void_p), 0) == -1
    cnt = C.c_void_p(1)
    assert lib.oww_events_dev(None, C.byref(cnt)) is None and cnt.value is None
    assert lib.oww_event_features_dev(None) is None
    assert n.value == 7 and not rec.view(np.uint8).any()


@pytest.mark.parametrize("kw", [dict(event_capacity=-1), dict(event_capacity=(1 << 20) + 1), dict(event_capacity=8, event_features=-1),
                                dict(event_features=4), dict(event_capacity=2.5), dict(event_capacity=True),
                                dict(event_capacity=8, event_features="16")])
def test_batched_model_keyword_validation(kw):
    with pytest.raises(ValueError, match="event_"):
        BatchedModel(4, ["alexa"], weights="synthetic", **kw)


def test_engine_keyword_validation_knows_the_ring():
    assert engine.check_event_config(8, 16, 16) == (8, 16)
    assert engine.check_event_config(0, 0, 16) == (0, 0)
    with pytest.raises(ValueError, match="feature ring"):
        engine.check_event_config(8, 17, 16)
