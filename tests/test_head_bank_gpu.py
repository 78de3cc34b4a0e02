"""Head bank on the GPU (include/owwhip.h: oww_bank_*): bank heads score bit for bit what the same nets score as fixed heads, agree
with the float64 bank oracle, keep Model.predict's per-slot state semantics, refuse what they cannot run, and leave the fixed heads and
the launch list alone."""
import numpy as np
import pytest

from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine

from bank_oracle import BankOracle

pytestmark = pytest.mark.gpu

FIXED = ["alexa", "hey_mycroft", "weather"]
EMB_SEED = 3


def _heads(names=FIXED):
    return {n: W.synthetic_head(n, 1234) for n in names}


def _engine(S, heads=None, K=1, cap=16, **kw):
    return StreamEngine(S, _heads() if heads is None else heads, W.synthetic_embedding(EMB_SEED), bank_slots=K, bank_capacity=cap, **kw)


def _pcm(rng, S, n=1280):
    return (rng.standard_normal((S, n)) * 3000).astype(np.int16)


def _same_as_fixed(S, steps):
    eng = _engine(S)
    ids = [eng.bank_add(W.synthetic_head(n, 1234)) for n in FIXED]
    sub = np.array(ids, dtype=np.int32)[np.arange(S) % 3][:, None]
    eng.subscribe(np.arange(S), sub)
    eng.set_postproc([2, 0, 0], [0.4, np.nan, np.nan], 0)
    eng.bank_set_postproc(ids[0], 2, 0.4)
    rng = np.random.default_rng(S)
    cols = np.arange(S) % 3
    for _ in range(steps):
        fixed = eng.step(_pcm(rng, S))
        bank = eng.bank_scores()
        np.testing.assert_array_equal(bank[:, 0], fixed[np.arange(S), cols])
    assert not eng.range_status()
    eng.close()


def test_bank_equals_fixed_heads_4096():
    _same_as_fixed(4096, 48)


def test_bank_equals_fixed_heads_131072():
    _same_as_fixed(131072, 12)


def _random_bank(n, seed):
    bank = {}
    for i in range(n):
        hidden = (32, 64, 128)[i % 3]
        T = 12 if i % 17 == 5 else 16
        h = W.synthetic_head(f"bank{i}", seed + i, hidden=hidden, layernorm=bool(i % 2), T=T)
        h["net"]["b3"] = (h["net"]["b3"] - np.float32(4.0)).astype(np.float32)   # (scores either side of 0.5)
        bank[i] = h
    return bank


def test_bank_oracle_parity():
    """256 distinct heads (hidden 32 / 64 / 128, LayerNorm on and off, T 16 and 12), 4,096 streams x K = 2 random subscriptions with
    empty slots; a quarter of the streams resubscribe at step 20.  Sampled streams are run on the float64 bank oracle."""
    S, K, steps, n_heads = 4096, 2, 48, 256
    rng = np.random.default_rng(1)
    bank = _random_bank(n_heads, 100)
    eng = _engine(S, K=K, cap=n_heads)
    ids = [eng.bank_add(bank[i]) for i in range(n_heads)]
    assert ids == list(range(n_heads))
    post = {b: (2, 0.3) for b in range(0, n_heads, 2)}
    for b, (pat, thr) in post.items():
        eng.bank_set_postproc(b, pat, thr)
    sub = rng.integers(-1, n_heads, size=(S, K)).astype(np.int32)
    eng.subscribe(np.arange(S), sub)
    noise = W.synthetic_pcm(1, 64000, seed=3, rms=600.0)[0]
    emb = W.synthetic_embedding(EMB_SEED)
    sample = rng.choice(S, 24, replace=False)
    first = BankOracle(bank, emb, K, init_noise=noise)
    eng.reset(None, first.preprocessor.features[-eng.feature_ring:].astype(np.float32))
    oracles = {s: BankOracle(bank, emb, K, features=first.preprocessor.features) for s in sample}
    for s in sample:
        oracles[s].subscribe(sub[s])
    moved = rng.choice(S, S // 4, replace=False)
    moved = np.union1d(moved, sample[:8])
    worst, n_cmp, n_post = 0.0, 0, 0
    for t in range(steps):
        if t == 20:
            new = rng.integers(-1, n_heads, size=(moved.size, K)).astype(np.int32)
            eng.subscribe(moved, new)
            for i, s in enumerate(moved):
                sub[s] = new[i]
                if s in oracles:
                    oracles[s].subscribe(new[i])
        x = _pcm(rng, S)
        eng.step(x)
        got = eng.bank_scores()
        for s in sample:
            _, want = oracles[s].predict(x[s], post)
            for k in range(K):
                if sub[s, k] < 0:
                    assert got[s, k] == 0.0
                    continue
                if len(oracles[s].rings[k]) > 5:
                    worst = max(worst, abs(float(got[s, k]) - want[k]))
                    n_cmp += 1
                    n_post += int(sub[s, k]) in post
    assert n_cmp >= 1024 and n_post >= n_cmp // 3, (n_cmp, n_post)
    assert worst <= 1e-4, worst
    assert not eng.range_status()
    eng.close()


def test_bank_large_routing_no_range_flag():
    """131,072 streams x 1,024 heads (128 streams each): the routed launch runs and raises no range flag."""
    S, n_heads = 131072, 1024
    eng = _engine(S, K=1, cap=n_heads)
    bank = _random_bank(n_heads, 7)
    for i in range(n_heads):
        eng.bank_add(bank[i])
    eng.subscribe(np.arange(S), (np.arange(S) % n_heads)[:, None])
    r = eng.bank_routing()
    assert sum(r["entries"]) == S
    rng = np.random.default_rng(2)
    for _ in range(8):
        eng.step(_pcm(rng, S))
    got = eng.bank_scores()
    assert np.isfinite(got).all() and got.max() > 0.0
    assert not eng.range_status()
    eng.close()


def test_bank_state_semantics():
    S, K = 96, 2
    rng = np.random.default_rng(3)
    pcm = [_pcm(rng, S) for _ in range(40)]
    a, b = _engine(S, K=K), _engine(S, K=K)
    ha, hb = W.synthetic_head("alexa", 1234), W.synthetic_head("weather", 1234)
    for e in (a, b):
        assert [e.bank_add(ha), e.bank_add(hb)] == [0, 1]
        e.subscribe(np.arange(S), np.tile([[0, 1]], (S, 1)))
        e.set_postproc([0, 0, 2], [np.nan, np.nan, 0.4], 0)
        e.bank_set_postproc(1, 2, 0.4)
    for t in range(10):
        fa, fb = a.step(pcm[t]), b.step(pcm[t])
    # resubscription: slot 0 of stream 3 to head 1 in `a`; its slot 1 and the fixed heads do not move
    a.subscribe([3], [[1, 1]])
    for t in range(10, 17):
        fa, fb = a.step(pcm[t]), b.step(pcm[t])
        ga, gb = a.bank_scores(), b.bank_scores()
        np.testing.assert_array_equal(fa, fb)
        np.testing.assert_array_equal(ga[np.arange(S) != 3], gb[np.arange(S) != 3])
        np.testing.assert_array_equal(ga[3, 1], gb[3, 1])
        if t < 15:
            assert ga[3, 0] == 0.0                     # a newly loaded model: five zero frames, then the head's rules on a fresh ring
    # reset(ids) restarts the bank rings and keeps the subscriptions
    a.reset([5]); b.reset([5])
    for t in range(17, 24):
        a.step(pcm[t]); b.step(pcm[t])
        ga, gb = a.bank_scores(), b.bank_scores()
        np.testing.assert_array_equal(ga[5], gb[5])
        if t < 22:
            assert (ga[5] == 0.0).all()
        else:
            assert (ga[5] != 0.0).any()
    # masked step: non-participants keep their bank scores (and rings: the next full step agrees with an engine that saw the same steps)
    on = (np.arange(S) % 3 != 0).astype(np.uint8)
    before = a.bank_scores().copy()
    a.step_masked(pcm[24], on)
    after = a.bank_scores()
    np.testing.assert_array_equal(after[on == 0], before[on == 0])
    # bank_remove empties only the affected slots
    a.bank_remove(0)
    a.bank_set_postproc(1, 0, float("nan"))          # (slot 1 then reads its raw score)
    a.step(pcm[25])
    g = a.bank_scores()
    assert (g[np.arange(S) != 3, 0] == 0.0).all() and (g[:, 1] != 0.0).any()
    a.close(); b.close()


def test_bank_multichunk_max():
    S = 64
    rng = np.random.default_rng(4)
    e3 = _engine(S, K=1, max_chunks=3)
    e3.bank_add(W.synthetic_head("alexa", 1234))
    e3.subscribe(np.arange(S), np.zeros((S, 1), np.int32))
    e3.set_postproc([0, 0, 0], None, 0)
    for _ in range(5):                                  # past the first-5 zeroing
        e3.step(_pcm(rng, S, 3 * 1280))
    fixed = e3.step(_pcm(rng, S, 3 * 1280))
    assert (fixed[:, 0] > 0.0).all()
    np.testing.assert_array_equal(e3.bank_scores()[:, 0], fixed[:, 0])   # fixed = max over the call's chunks (model.py:287-298)
    e3.close()


def test_bank_vad_gate_and_graph():
    S = 64
    rng = np.random.default_rng(5)
    for graph in (False, True):
        e = _engine(S, K=1, vad_threshold=0.5)
        e.bank_add(W.synthetic_head("hey_mycroft", 1234))
        e.subscribe(np.arange(S), np.zeros((S, 1), np.int32))
        if graph:
            e.use_graph(True)
        outs = []
        for t in range(16):
            e.push_vad(rng.random(S).astype(np.float32))
            x = _pcm(rng, S)
            fixed = e.step(x)
            bank = e.bank_scores()
            np.testing.assert_array_equal(bank[:, 0], fixed[:, 1])
            outs.append(bank.copy())
        if not graph:
            ref = outs
        else:
            for o, r in zip(outs, ref):
                np.testing.assert_array_equal(o, r)
        e.close()
        rng = np.random.default_rng(5)


def test_bank_only_handle():
    S = 128
    e = StreamEngine(S, {}, W.synthetic_embedding(EMB_SEED), bank_slots=1, bank_capacity=4)
    ref = _engine(S, K=1)
    assert e._lib.oww_n_labels(e._h) == 0
    for x in (e, ref):
        x.bank_add(W.synthetic_head("weather", 1234))
        x.subscribe(np.arange(S), np.zeros((S, 1), np.int32))
    rng = np.random.default_rng(6)
    for t in range(10):
        x = _pcm(rng, S)
        e.step(x); ref.step(x)
    np.testing.assert_array_equal(e.bank_scores(), ref.bank_scores())
    e.close(); ref.close()


def test_bank_refusals_keep_the_handle_working():
    S = 64
    e = _engine(S, K=2, cap=2)
    lib = e._lib
    from openwakeword_amd.engine import pack_head_blob, _ptr

    def add(h):
        blob = pack_head_blob(h)
        return lib.oww_bank_add(e._h, _ptr(blob), blob.nbytes), lib.oww_last_error().decode()
    for h, word in [(W.synthetic_head("hey_jarvis", 1), "gated"), (W.synthetic_head("timer", 1), "multiclass"),
                    (W.synthetic_head("x", 1, kind="rnn", T=16, n_out=1), "recurrent"), (W.synthetic_head("x", 1, n_blocks=2), "hidden block"),
                    (W.synthetic_head("x", 1, T=20), "feature ring"), (W.synthetic_head("x", 1, hidden=160), "hidden")]:
        rc, msg = add(h)
        assert rc == -1 and word in msg, (rc, msg)
    assert add(W.synthetic_head("alexa", 1234))[0] == 0 and add(W.synthetic_head("weather", 1))[0] == 1
    rc, msg = add(W.synthetic_head("alexa", 2))
    assert rc == -1 and "full" in msg
    ids = np.array([0], np.int32)
    for bad in ([[0, 7]], [[0, 2]]):
        b = np.array(bad, np.int32)
        assert lib.oww_subscribe(e._h, _ptr(ids), 1, _ptr(b)) == -1
    ids2 = np.array([S], np.int32)
    assert lib.oww_subscribe(e._h, _ptr(ids2), 1, _ptr(np.array([[0, 1]], np.int32))) == -1
    assert lib.oww_bank_remove(e._h, 5) == -1 and lib.oww_bank_set_postproc(e._h, 9, 1, 0.5) == -1
    e.bank_remove(1)
    assert lib.oww_subscribe(e._h, _ptr(ids), 1, _ptr(np.array([[0, 1]], np.int32))) == -1      # stale id
    e.subscribe(np.arange(S), np.tile([[0, -1]], (S, 1)))
    rng = np.random.default_rng(7)
    for _ in range(7):
        f = e.step(_pcm(rng, S))
    np.testing.assert_array_equal(e.bank_scores()[:, 0], f[:, 0])
    e.close()
    # the exact-fp32 families have no bank
    with pytest.raises(_lib.OwwError, match="use_mfma = 3"):
        StreamEngine(8, _heads(), W.synthetic_embedding(EMB_SEED), use_mfma=1, bank_slots=1, bank_capacity=2)


def test_bank_no_interference():
    S = 512
    rng = np.random.default_rng(8)
    plain = StreamEngine(S, _heads(), W.synthetic_embedding(EMB_SEED))
    banked = _engine(S, K=2, cap=4)
    idle = _engine(S, K=2, cap=4)
    for n in FIXED:
        banked.bank_add(W.synthetic_head(n, 99))
        idle.bank_add(W.synthetic_head(n, 99))
    banked.subscribe(np.arange(S), np.stack([np.arange(S) % 3, (np.arange(S) + 1) % 3], 1))
    for e in (plain, idle):
        e.enable_timing(True)
    for _ in range(6):
        x = _pcm(rng, S)
        np.testing.assert_array_equal(banked.step(x), plain.step(x))
        idle.step(x)
    tp, ti = plain.kernel_times(), idle.kernel_times()
    assert {k: v["launches"] for k, v in tp.items()} == {k: v["launches"] for k, v in ti.items()}
    for e in (plain, banked, idle):
        e.close()
