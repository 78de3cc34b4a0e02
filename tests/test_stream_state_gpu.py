"""Stream state records on the GPU (include/owwhip.h: oww_state_*, oww_move_streams): a stream that is exported and imported, or
moved, continues BIT FOR BIT as if it had stayed where it was -- across handles, inside a handle, under masked steps, with the VAD
network, with bank subscriptions and per-stream verifiers, from device buffers, behind queued steps and at 131,072 streams -- and
every refusal leaves the handle untouched.  Every comparison is np.array_equal on float bits."""
import ctypes as C

import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine, default_calibration_pcm

pytestmark = pytest.mark.gpu

HEADS = ["alexa", "hey_mycroft", "hey_jarvis"]


def _heads(seed=11):
    return {n: W.synthetic_head(n, seed=seed + i) for i, n in enumerate(HEADS)}


def _engine(S, family=3, seed=11, emb_seed=3, **kw):
    return StreamEngine(S, _heads(seed), W.synthetic_embedding(seed=emb_seed), use_mfma=family, **kw)


def _audio(S, T, seed):
    """int16 [T, S, 1280], distinct per stream: the fixture clips at several phases and gains, noise at several levels, clip +
    noise, and silence."""
    rng = np.random.default_rng(seed)
    clips = default_calibration_pcm()
    n = T * 1280
    out = np.zeros((S, n), np.int16)
    for s in range(S):
        kind = s % 5
        if kind == 4 and s % 3 == 0:
            continue                                                   # silence
        x = np.zeros(n)
        if kind in (0, 2) and clips is not None:
            x += np.roll(np.resize(clips[s % len(clips)].astype(np.float64), n), 97 * s + 13)
        if kind in (1, 2, 3, 4) or clips is None:
            x += rng.standard_normal(n) * (30.0, 300.0, 3000.0, 9000.0)[s % 4]
        out[s] = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(out.reshape(S, T, 1280).transpose(1, 0, 2))


def _raw(e):
    out = np.empty((e.n_streams, e.n_labels), np.float32)
    _lib.check(e._lib.oww_get_raw(e._h, out.ctypes.data_as(C.c_void_p)))
    return out


def _eq(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, msg
    same = np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    if not same:
        bad = np.argwhere(a != b)
        raise AssertionError(f"{msg}: {len(bad)} of {a.size} values differ, first at {bad[:4].tolist()}")


# ---- 1. cross-handle continuation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,S,mul,before,after", [(3, 96, 5, 20, 40), (1, 96, 5, 20, 40), (2, 40, 7, 8, 34), (0, 40, 7, 8, 34)])
def test_cross_handle_continuation(family, S, mul, before, after):
    perm = (mul * np.arange(S) + 3) % S
    assert len(set(perm.tolist())) == S
    a, b = _engine(S, family), _engine(S, family)
    nb, fp = a.state_info()
    assert (nb, fp) == b.state_info() and nb % 16 == 0 and nb > 20000
    pcm = _audio(S, before + after, seed=family)
    for t in range(before):
        a.step(pcm[t])
    rec = a.export_state(np.arange(S))
    assert rec.shape == (S, nb) and rec.dtype == np.uint8
    hdr = rec[:, :32].view(np.uint32)
    assert (hdr[:, 2] == nb).all() and (hdr[:, 4].astype(np.uint64) | (hdr[:, 5].astype(np.uint64) << np.uint64(32)) == fp).all()
    b.import_state(perm, rec)
    inv = np.empty(S, np.int64)
    inv[perm] = np.arange(S)
    for t in range(before, before + after):
        sa = a.step(pcm[t])
        sb = b.step(pcm[t][inv])                       # stream perm(s) of B hears what stream s of A hears
        _eq(sb[perm], sa, f"family {family} step {t}")
    assert np.abs(sa).max() > 0
    _eq(_raw(b)[perm], _raw(a), "raw scores")
    for s in (0, 1, 7, 8, 15, 16, 31, S - 1):
        _eq(b.get_features(int(perm[s]), 16), a.get_features(s, 16), f"features of stream {s}")
    _eq(b.export_state(perm), a.export_state(np.arange(S)), "second export")
    a.close(); b.close()


# ---- 2. in-handle moves -------------------------------------------------------------------------------------------------------------
SRC = np.array([1, 2, 10, 20, 30, 40, 41, 48], np.int32)       # a swap, a 3-cycle, a chain into free slot 63, a move inside group 48..55
DST = np.array([2, 1, 20, 30, 10, 41, 63, 53], np.int32)


def _twin_of(S, src=SRC, dst=DST):
    """twin_of[j] = the stream of the undisturbed handle that stream j of the moved handle now is."""
    twin = np.arange(S)
    twin[dst] = src
    return twin


@pytest.mark.parametrize("family,graph", [(3, False), (3, True), (1, False)])
def test_moves_inside_a_handle(family, graph):
    S, before, after = 64, 12, 40
    a, b = _engine(S, family), _engine(S, family)
    if graph:
        a.use_graph(True); b.use_graph(True)
    pcm = _audio(S, before + after, seed=20 + family)
    for t in range(before):
        _eq(b.step(pcm[t]), a.step(pcm[t]), "twins before the move")
    b.move_streams(SRC, DST)
    twin = _twin_of(S)
    for t in range(before, before + after):
        sa = a.step(pcm[t])
        sb = b.step(pcm[t][twin])
        _eq(sb, sa[twin], f"step {t}: moved streams and everybody else, group mates included")
    _eq(_raw(b), _raw(a)[twin], "raw")
    _eq(b.export_state(np.arange(S)), a.export_state(twin), "records")
    a.close(); b.close()


# ---- 3. masked steps after a move ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,frac", [(3, 0.3), (3, 0.7), (1, 0.3)])
def test_masked_steps_after_a_move(family, frac):
    S, before, after = 200, 6, 30
    rng = np.random.default_rng(7)
    a, b = _engine(S, family), _engine(S, family)
    pcm = _audio(S, before + after, seed=30)
    for t in range(before):
        a.step(pcm[t]); b.step(pcm[t])
    src = rng.choice(S, 60, replace=False).astype(np.int32)
    dst = np.roll(src, 7)
    b.move_streams(src, dst)
    twin = _twin_of(S, src, dst)
    for t in range(before, before + after):
        on = rng.random(S) < frac
        on[0] = True
        sa = a.step_masked(pcm[t], on)
        sb = b.step_masked(pcm[t][twin], on[twin])
        _eq(sb, sa[twin], f"masked step {t}")
    a.close(); b.close()


# ---- 4. VAD network fused -----------------------------------------------------------------------------------------------------------
def test_vad_state_travels():
    S, before, after = 48, 10, 24
    kw = dict(vad=W.synthetic_vad(seed=9), vad_threshold=0.5)
    a, b, c = _engine(S, **kw), _engine(S, **kw), _engine(S, **kw)
    pcm = _audio(S, before + after, seed=40)
    for t in range(before):
        a.step(pcm[t]); b.step(pcm[t])
    src = np.array([0, 17, 33, 5, 21, 40], np.int32)
    dst = np.array([17, 33, 0, 21, 5, 47], np.int32)
    b.move_streams(src, dst)
    twin = _twin_of(S, src, dst)
    perm = (5 * np.arange(S) + 3) % S
    inv = np.empty(S, np.int64)
    inv[perm] = np.arange(S)
    c.import_state(perm, a.export_state(np.arange(S)))
    for t in range(before, before + after):
        sa, sb, sc = a.step(pcm[t]), b.step(pcm[t][twin]), c.step(pcm[t][inv])
        _eq(sb, sa[twin], f"moved, step {t}")
        _eq(sc[perm], sa, f"imported, step {t}")
        va = a.get_vad()
        _eq(b.get_vad(), va[twin], f"VAD scores, moved, step {t}")
        _eq(c.get_vad()[perm], va, f"VAD scores, imported, step {t}")
    assert np.isfinite(va).all() and va.max() > 0
    a.close(); b.close(); c.close()


# ---- 5. bank subscriptions and per-stream verifiers ---------------------------------------------------------------------------------
def _bank_setup(e, S, K, sub, free):
    rng = np.random.default_rng(3)
    ids = [e.bank_add(W.synthetic_head(f"bank{i}", 50 + i, hidden=(32, 64, 128)[i % 3])) for i in range(4)]
    assert ids == [0, 1, 2, 3]
    e.subscribe(np.arange(S), sub)
    pool = [e.verifier_add((rng.standard_normal(16 * 96) * 0.02).astype(np.float32), float(rng.standard_normal() * 0.1)) for _ in range(6)]
    fixed = np.array([s for s in range(0, S, 3) if s not in free], np.int32)
    e.assign_verifiers(0, fixed, np.array([pool[s % 6] for s in fixed], np.int32), np.zeros(len(fixed), np.float32))
    slot0 = np.array([s for s in range(S) if sub[s, 0] >= 0 and s % 2], np.int32)
    e.assign_verifiers(0, slot0, np.array([pool[(s + 1) % 6] for s in slot0], np.int32), np.zeros(len(slot0), np.float32), bank=True)
    return fixed, slot0, pool


def test_bank_and_verifiers_travel():
    S, K = 64, 2
    free = {63, 53}
    rng = np.random.default_rng(5)
    sub = rng.integers(-1, 4, size=(S, K)).astype(np.int32)
    sub[1], sub[2] = [0, 3], [2, -1]
    for f in free:
        sub[f] = -1
    kw = dict(bank_slots=K, bank_capacity=8, verifier_capacity=8)
    a, b = _engine(S, **kw), _engine(S, **kw)
    _bank_setup(a, S, K, sub, free)
    _bank_setup(b, S, K, sub, free)
    pcm = _audio(S, 40, seed=50)
    before = 3                                          # the move happens during every slot's first five predictions
    for t in range(before):
        _eq(b.step(pcm[t]), a.step(pcm[t]), "twins before")
        _eq(b.bank_scores(), a.bank_scores(), "twin banks before")
    routing, stats = b.bank_routing()["entries"], b.verifier_stats()[0]
    assert sum(routing) > 0 and stats > 0
    b.move_streams(SRC, DST)
    assert b.bank_routing()["entries"] == routing and b.verifier_stats()[0] == stats
    twin = _twin_of(S)
    live = np.array([j for j in range(S) if j not in (set(SRC.tolist()) - set(DST.tolist()))])    # vacated slots are nobody's stream
    seen = 0.0
    for t in range(before, 40):
        sa, sb = a.step(pcm[t]), b.step(pcm[t][twin])
        _eq(sb[live], sa[twin][live], f"fixed scores, step {t}")
        ba, bb = a.bank_scores(), b.bank_scores()
        _eq(bb[live], ba[twin][live], f"bank scores from the first step after the move (step {t}): no slot restarted")
        seen = max(seen, float(np.abs(bb).max()))
    assert seen > 0 and b.verifier_stats()[1] > 0
    # vacated slots ended up unsubscribed
    for j in set(SRC.tolist()) - set(DST.tolist()):
        assert (bb[j] == 0).all()
    # cross-handle: subscribe and assign on the target first, then import
    perm = (5 * np.arange(S) + 3) % S
    inv = np.empty(S, np.int64)
    inv[perm] = np.arange(S)
    c = _engine(S, **kw)
    sub_c = np.empty_like(sub)
    sub_c[perm] = sub
    ids = [c.bank_add(W.synthetic_head(f"bank{i}", 50 + i, hidden=(32, 64, 128)[i % 3])) for i in range(4)]
    c.subscribe(np.arange(S), sub_c)
    rng3 = np.random.default_rng(3)
    pool = [c.verifier_add((rng3.standard_normal(16 * 96) * 0.02).astype(np.float32), float(rng3.standard_normal() * 0.1)) for _ in range(6)]
    fixed = np.array([s for s in range(0, S, 3) if s not in free], np.int32)
    c.assign_verifiers(0, perm[fixed], np.array([pool[s % 6] for s in fixed], np.int32), np.zeros(len(fixed), np.float32))
    slot0 = np.array([s for s in range(S) if sub[s, 0] >= 0 and s % 2], np.int32)
    c.assign_verifiers(0, perm[slot0], np.array([pool[(s + 1) % 6] for s in slot0], np.int32), np.zeros(len(slot0), np.float32), bank=True)
    c.step(pcm[0][inv])                                 # (the target has a past of its own, which the import replaces)
    a2 = _engine(S, **kw)
    _bank_setup(a2, S, K, sub, free)
    for t in range(3):
        a2.step(pcm[t])
    c.import_state(perm, a2.export_state(np.arange(S)))
    for t in range(3, 20):
        sa, sc = a2.step(pcm[t]), c.step(pcm[t][inv])
        _eq(sc[perm], sa, f"imported fixed scores, step {t}")
        _eq(c.bank_scores()[perm], a2.bank_scores(), f"imported bank scores, step {t}")
    for e in (a, b, c, a2):
        e.close()


# ---- 6. refusals leave no trace -----------------------------------------------------------------------------------------------------
def test_refusals_leave_no_trace():
    S = 32
    a, b = _engine(S), _engine(S)
    other_weights, other_family = _engine(S, seed=12), _engine(S, family=1)
    pcm = _audio(S, 24, seed=60)
    t = 0

    def both():
        nonlocal t
        _eq(b.step(pcm[t]), a.step(pcm[t]), f"after a refusal, step {t}")
        t += 1

    for _ in range(6):
        both()
        other_weights.step(pcm[t]); other_family.step(pcm[t])
    ids = np.arange(4)
    good = a.export_state(ids)
    assert other_weights.state_info()[1] != a.state_info()[1] != other_family.state_info()[1]
    for rec in (other_weights.export_state(ids), other_family.export_state(ids)):
        if rec.shape[1] != good.shape[1]:
            rec = np.ascontiguousarray(np.resize(rec, good.shape))
        with pytest.raises(_lib.OwwError, match="error -1.*fingerprint"):
            b.import_state(ids, rec)
        both()
    for byte in (0, 4, 8, 16, 23):                      # magic, layout version, record bytes, fingerprint
        bad = good.copy()
        bad[3, byte] ^= 0x40                            # (the LAST record: nothing of the first three may have been written)
        with pytest.raises(_lib.OwwError, match="error -1"):
            b.import_state(ids, bad)
        both()
    with pytest.raises(_lib.OwwError, match="error -1.*twice"):
        b.import_state(np.array([1, 2, 1, 3]), good)
    both()
    with pytest.raises(_lib.OwwError, match="error -1.*twice"):
        b.move_streams([0, 1], [5, 5])
    both()
    for src, dst in (([0, S], [1, 2]), ([0, 1], [-1, 2]), ([0, 1], [1, S])):
        with pytest.raises(_lib.OwwError, match="error -1.*out of range"):
            b.move_streams(src, dst)
        both()
    with pytest.raises(_lib.OwwError, match="error -1.*out of range"):
        b.import_state([0, 1, 2, S], good)
    both()
    with pytest.raises(_lib.OwwError, match="error -1.*out of range"):
        b.export_state([S])
    both()
    # before oww_commit: OWW_ESTATE from all four
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(0, 8, 1, 0, 3, 0, None)
    _lib.check(lib.oww_create(C.byref(cfg), C.byref(h)))
    i32 = np.zeros(2, np.int32)
    buf = np.zeros(1 << 17, np.uint8)
    nb, fp = C.c_size_t(0), C.c_uint64(0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.oww_state_info(h, C.byref(nb), C.byref(fp)) == -3
    assert lib.oww_state_export(h, p(i32), 1, p(buf), 0) == -3
    assert lib.oww_state_import(h, p(i32), 1, p(buf), 0) == -3
    assert lib.oww_move_streams(h, p(i32), p(i32), 1) == -3
    lib.oww_destroy(h)
    both()
    _eq(b.export_state(np.arange(S)), a.export_state(np.arange(S)), "records after all refusals")
    for e in (a, b, other_weights, other_family):
        e.close()


# ---- 7. device buffers and queued steps ---------------------------------------------------------------------------------------------
def test_device_buffers_and_queued_steps():
    import torch
    S = 64
    a, b, c = _engine(S), _engine(S), _engine(S)
    pcm = _audio(S, 30, seed=70)
    for t in range(8):
        a.step(pcm[t]); b.step(pcm[t])
    nb = a.state_info()[0]
    ids = np.array([3, 9, 8, 40, 41, 42, 43, 44, 45, 46, 47, 63], np.int32)
    host = a.export_state(ids)
    dev = torch.zeros(len(ids) * nb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.export_state_device(ids, dev.data_ptr())
    _eq(dev.cpu().numpy().reshape(len(ids), nb), host, "export to a device buffer")
    to = np.array([5, 6, 7, 16, 17, 18, 19, 20, 21, 22, 23, 0], np.int32)
    c.import_state_device(to, dev.data_ptr())
    b.import_state(to, host)                            # B's own streams ids[i] cloned over its streams to[i], through the host
    twin = np.arange(S)
    twin[to] = ids
    for t in range(8, 14):
        sa, sb, sc = a.step(pcm[t]), b.step(pcm[t][twin]), c.step(pcm[t][twin])
        _eq(sb, sa[twin], f"host import, step {t}")
        _eq(sc[to], sb[to], f"device import equals host import, step {t}")
    # a move issued between submit and collect is ordered behind the queued step
    x = np.ascontiguousarray(pcm[14][twin])
    b.submit(x)
    b.move_streams(SRC, DST)
    _eq(b.collect(), a.step(pcm[14])[twin], "the queued step ran before the move")
    twin2 = twin.copy()
    twin2[DST] = twin[SRC]
    for t in range(15, 30):
        _eq(b.step(pcm[t][twin2]), a.step(pcm[t])[twin2], f"after the queued move, step {t}")
    for e in (a, b, c):
        e.close()


# ---- 8. at scale --------------------------------------------------------------------------------------------------------------------
def test_at_scale_131072():
    S, NP, before, after, n_move = 131072, 64, 16, 24, 16384
    rng = np.random.default_rng(8)
    keep_src_free = {0, 7, 128, S - 1}
    blocks = rng.choice(np.setdiff1d(np.arange(S // 32), [0, 3, 4, S // 32 - 1]), n_move // 32, replace=False)
    dst_all = (blocks[:, None] * 32 + np.arange(32)).ravel()
    in_dst = np.zeros(S, bool)
    in_dst[dst_all] = True
    cand = np.array([s for s in np.nonzero(~in_dst)[0] if s not in keep_src_free and s not in (8, 127)])
    src = np.concatenate([[8, 127], rng.choice(cand, n_move - 2, replace=False)]).astype(np.int32)
    dst = rng.permutation(dst_all).astype(np.int32)
    is_src = np.zeros(S, bool)
    is_src[src] = True
    unmoved = np.nonzero(~in_dst & ~is_src)[0]
    probes = np.concatenate([[0, 7, 8, 127, 128, S - 1], rng.choice(src[2:], 29, replace=False),
                             rng.choice(np.setdiff1d(unmoved, [0, 7, 128, S - 1]), 29, replace=False)]).astype(np.int64)
    assert len(set(probes.tolist())) == NP
    big, small = _engine(S), _engine(NP)
    assert big.state_info() == small.state_info()
    pcm = _audio(NP, before + after, seed=80)
    x = np.ascontiguousarray(np.tile((rng.standard_normal((1024, 1280)) * 2000).astype(np.int16), (S // 1024, 1)))
    out = np.empty((S, big.n_labels), np.float32)
    where = probes.copy()
    new_slot = np.arange(S)
    new_slot[src] = dst
    for t in range(before + after):
        if t == before:
            big.move_streams(src, dst)
            where = new_slot[probes]
            assert (where != probes).sum() == 31
        x[where] = pcm[t]
        big.step(x, out)
        _eq(out[where], small.step(pcm[t]), f"step {t}")
    assert np.abs(out[where]).max() > 0
    big.close(); small.close()
