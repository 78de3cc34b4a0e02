"""Stream state records, host side: the four C entries exist (header, library, ctypes) and refuse a null handle; the slot
allocator's compaction plan; the Python wrappers' argument checks, which run before the library is reached."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from openwakeword_amd import _build, _lib
from openwakeword_amd.model import BatchedModel
from openwakeword_amd.serve import SlotAllocator

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("oww_state_info", "oww_state_export", "oww_state_import", "oww_move_streams")


def test_entries_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "owwhip.h")) as f:
        header = f.read()
    assert "#define OWW_ABI_VERSION 6" in header and "#define OWW_N_KERNEL_CLASSES 10" in header
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(oww_ctx\* h,", header, re.M), name
        assert name in _lib.SYMBOLS
    lib = C.CDLL(_build.lib_path())
    for name in ENTRIES:
        assert hasattr(lib, name), f"libowwhip.so does not export {name}"


def test_null_handle_is_an_error_code():
    lib = _lib.load()
    ids = np.zeros(1, dtype=np.int32)
    buf = np.zeros(64, dtype=np.uint8)
    nb, fp = C.c_size_t(0), C.c_uint64(0)
    assert lib.oww_state_info(None, C.byref(nb), C.byref(fp)) < 0
    assert lib.oww_state_export(None, ids.ctypes.data, 1, buf.ctypes.data, 0) < 0
    assert lib.oww_state_import(None, ids.ctypes.data, 1, buf.ctypes.data, 0) < 0
    assert lib.oww_move_streams(None, ids.ctypes.data, ids.ctypes.data, 1) < 0
    assert lib.oww_last_error()


# ---- SlotAllocator.plan_compaction ------------------------------------------------------------------------------------------------
def _churned(seed, n_slots=1024, group=32, keys=("a", "b", "c", None)):
    """An allocator after seeded arrivals and departures over several keys, then a wave of departures that leaves sparse blocks.
    Never more than half full, so no key borrows another key's block.  Returns it with {slot: the key it was allocated with}."""
    rng = np.random.default_rng(seed)
    al = SlotAllocator(n_slots, group)
    owner = {}

    def leave():
        slot = list(owner)[int(rng.integers(len(owner)))]
        al.release(slot)
        del owner[slot]

    for _ in range(3000):
        if owner and (rng.random() < 0.45 or al.n_used >= n_slots // 2):
            leave()
        else:
            key = keys[int(rng.integers(len(keys)))]
            owner[al.alloc(key)] = key
    for _ in range(len(owner) * 2 // 5):
        leave()
    return al, owner


def _blocks_per_key(al, owner):
    out = {}
    for slot in owner:
        out.setdefault(al.key_of(slot), set()).add(slot // al.group)
    return {k: len(v) for k, v in out.items()}


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("max_moves", [None, 0, 7, 100])
def test_plan_compaction(seed, max_moves):
    al, owner = _churned(seed)
    for slot, key in owner.items():
        assert al.key_of(slot) == key                    # (the fixture's premise: every key owns its blocks alone)
    before = _blocks_per_key(al, owner)
    n_used = al.n_used
    src, dst = al.plan_compaction(max_moves)
    assert src.dtype == np.int32 and dst.dtype == np.int32 and src.shape == dst.shape and src.ndim == 1
    if max_moves is not None:
        assert src.size <= max_moves
    assert len(set(src.tolist())) == src.size and len(set(dst.tolist())) == dst.size
    assert not set(src.tolist()) & set(dst.tolist())
    moved = dict(owner)
    for s, d in zip(src.tolist(), dst.tolist()):
        assert s in owner, "a source slot was not in use"
        assert d not in owner, "a destination slot was not free"
        moved[d] = moved.pop(s)
    # keys never mix: every stream still sits in a block of its own key, by the allocator's tables after the plan
    for slot, key in moved.items():
        assert al.key_of(slot) == key
    assert al.n_used == n_used == len(moved)
    after = _blocks_per_key(al, moved)
    per_key = {}
    for key in moved.values():
        per_key[key] = per_key.get(key, 0) + 1
    for key, n in per_key.items():
        assert after[key] <= before[key]
        if max_moves is None:
            assert after[key] == math.ceil(n / al.group), (key, n, after[key])
    if max_moves is None:
        assert sum(before.values()) > sum(after.values()) and src.size > 0       # (the fixture does leave something to repair)
    # the tables agree with replaying the moves by hand: new arrivals never land on a stream, every stream can leave, and the
    # emptied allocator hands out every slot again
    for _ in range(40):
        slot = al.alloc("b")
        assert slot not in moved
        moved[slot] = "b"
    for slot in list(moved):
        al.release(slot)
    assert al.n_used == 0 and not al._tag and len(al._fresh) == al.n_blocks
    assert {al.alloc("z") for _ in range(al.n_slots)} == set(range(al.n_slots))
    with pytest.raises(IndexError):
        al.alloc("z")


def test_plan_compaction_on_an_empty_and_on_a_packed_allocator():
    al = SlotAllocator(256, 32)
    src, dst = al.plan_compaction()
    assert src.size == 0 and dst.size == 0
    slots = [al.alloc("a") for _ in range(64)]
    src, dst = al.plan_compaction()
    assert src.size == 0                                 # two full blocks: nothing to gain
    for s in slots[1:32:2] + slots[32:64:2]:
        al.release(s)
    src, dst = al.plan_compaction()
    assert src.size == 16 and {al.key_of(int(d)) for d in dst} == {"a"}
    assert len({int(d) // 32 for d in dst}) == 1 and len({int(s) // 32 for s in src}) == 1


# ---- wrappers: argument checks before the library ---------------------------------------------------------------------------------
class _StateEngine:
    RECORD = 208

    def __init__(self):
        self.calls = []

    def state_info(self):
        return self.RECORD, 0x1234

    def export_state(self, ids):
        self.calls.append(("export", ids))
        return np.zeros((len(ids), self.RECORD), dtype=np.uint8)

    def import_state(self, ids, rec):
        self.calls.append(("import", ids, rec))

    def move_streams(self, s, d):
        self.calls.append(("move", s, d))


def _bare_model(S=8):
    m = BatchedModel.__new__(BatchedModel)               # (no library, no GPU: the checks run before the engine is reached)
    m.n_streams, m.bank_slots, m.engine, m._debounce_frames = S, 0, _StateEngine(), 0
    return m


@pytest.mark.parametrize("ids,rec,msg", [
    ([0, 1], np.zeros((1, 208), np.uint8), "shape"),                 # length mismatch
    ([0, 1], np.zeros((2, 200), np.uint8), "shape"),                 # wrong record width
    ([0, 1], np.zeros((2, 208), np.float32), "uint8"),               # wrong dtype
    ([0, 1], np.zeros((2, 52), np.int32), "uint8"),
    ([0, 1], np.zeros(416, np.uint8), "shape"),
    ([0, 8], np.zeros((2, 208), np.uint8), "stream ids"),
    ([-1], np.zeros((1, 208), np.uint8), "stream ids"),
    ([[0]], np.zeros((1, 208), np.uint8), "1-D"),
    ([0.5], np.zeros((1, 208), np.uint8), "integer"),
    ([3, 3], np.zeros((2, 208), np.uint8), "twice"),
])
def test_bad_import_arguments(ids, rec, msg):
    m = _bare_model()
    with pytest.raises(ValueError, match=msg):
        m.import_streams(np.array(ids), rec)
    assert m.engine.calls == []


@pytest.mark.parametrize("src,dst,msg", [
    ([0, 1], [2], "same length"),
    ([0, 1], [2, 2], "twice"),
    ([0, 9], [1, 2], "stream ids"),
    ([0, 1], [1, 8], "stream ids"),
    ([0.0], [1], "integer"),
    ([[0]], [[1]], "1-D"),
])
def test_bad_move_arguments(src, dst, msg):
    m = _bare_model()
    with pytest.raises(ValueError, match=msg):
        m.move_streams(np.array(src), np.array(dst))
    assert m.engine.calls == []


def test_bad_export_arguments_and_pass_through():
    m = _bare_model()
    with pytest.raises(ValueError, match="stream ids"):
        m.export_streams([8])
    with pytest.raises(ValueError, match="1-D"):
        m.export_streams([[1]])
    assert m.engine.calls == []
    rec = m.export_streams([1, 2])
    assert rec.shape == (2, 208) and rec.dtype == np.uint8
    m.import_streams([4, 5], rec)
    m.move_streams([0, 1], [1, 0])                       # a swap is legal
    assert [c[0] for c in m.engine.calls] == ["export", "import", "move"]
