"""Head bank, host side: the Python-side refusals of bank heads and subscription arrays, and the float64 bank oracle's sanity check
against OracleModel.predict (with subscriptions that never change, a bank slot is exactly a loaded model)."""
import numpy as np
import pytest

from openwakeword_amd import weights as W
from openwakeword_amd.model import BatchedModel, check_bank_head
from oracle import oww_oracle as O

from bank_oracle import BankOracle


@pytest.mark.parametrize("head,reason", [
    (lambda: W.synthetic_head("hey_jarvis", 1), "gated"),
    (lambda: W.synthetic_head("timer", 1), "multiclass"),
    (lambda: W.synthetic_head("x", 1, kind="rnn", T=16, n_out=1), "recurrent"),
    (lambda: W.synthetic_head("x", 1, n_blocks=2), "one hidden block"),
    (lambda: W.synthetic_head("x", 1, n_blocks=0), "one hidden block"),
    (lambda: W.synthetic_head("x", 1, hidden=160), "128 hidden units"),
    (lambda: W.synthetic_head("x", 1, T=24), "feature ring"),
])
def test_bank_refuses_unsupported_forms(head, reason):
    with pytest.raises(ValueError, match=reason):
        check_bank_head(head(), 16)


@pytest.mark.parametrize("hidden,ln,T", [(32, True, 16), (64, False, 16), (128, True, 12), (100, False, 16)])
def test_bank_accepts_binary_one_block_heads(hidden, ln, T):
    check_bank_head(W.synthetic_head("x", 1, hidden=hidden, layernorm=ln, T=T), 16)


class _Engine:
    def __init__(self):
        self.calls = []

    def subscribe(self, ids, b):
        self.calls.append((ids, b))


def _bare_model(S=8, K=2):
    m = BatchedModel.__new__(BatchedModel)          # (no library, no GPU: the checks run before the engine is reached)
    m.n_streams, m.bank_slots, m.engine, m._debounce_frames = S, K, _Engine(), 0
    return m


@pytest.mark.parametrize("ids,bank,msg", [
    ([0, 1], [[0, 1]], "shape"),
    ([0, 1], [[0, 1, 2], [0, 1, 2]], "shape"),
    ([0, 8], [[0, 1], [0, 1]], "stream ids"),
    ([-1], [[0, 1]], "stream ids"),
    ([0], [[0, -2]], "bank ids"),
    ([0], [[0.5, 1]], "integer"),
    ([[0]], [[0, 1]], "1-D"),
])
def test_bad_subscription_arrays(ids, bank, msg):
    m = _bare_model()
    with pytest.raises(ValueError, match=msg):
        m.subscribe(np.array(ids), np.array(bank))
    assert m.engine.calls == []


def test_subscription_arrays_pass_through():
    m = _bare_model()
    m.subscribe([3, 5], [[0, -1], [2, 2]])
    assert len(m.engine.calls) == 1


def test_bank_postproc_rules():
    m = _bare_model()
    with pytest.raises(ValueError, match="threshold"):
        m.set_bank_postproc(0, patience=3)
    m._debounce_frames = 2
    with pytest.raises(ValueError, match="cannot be used together"):
        m.set_bank_postproc(0, patience=3, threshold=0.5)


def test_bank_needs_fixed_heads_or_a_bank():
    with pytest.raises(ValueError, match="bank"):
        BatchedModel(4, [], weights="synthetic")


def test_bank_oracle_equals_oracle_model():
    """Subscriptions that never change: every slot's raw and post-processed scores are OracleModel.predict's, bit for bit (same
    dtype), with patience on one head and threshold-only on the other."""
    emb = W.synthetic_embedding(7)
    heads = {"alexa": W.synthetic_head("alexa", 1234), "weather": W.synthetic_head("weather", 1234)}
    noise = W.synthetic_pcm(1, 64000, seed=3, rms=600.0)[0]
    pcm = W.synthetic_pcm(2, 1280 * 12, seed=9)
    bank = {0: heads["alexa"], 1: heads["weather"]}
    post = {0: (2, 0.3)}
    for s in range(2):
        model = O.OracleModel(heads, emb, dtype=np.float64, init_noise=noise)
        bo = BankOracle(bank, emb, 2, dtype=np.float64, init_noise=noise)
        bo.subscribe([0, 1] if s == 0 else [1, 0])
        for t in range(12):
            x = pcm[s, 1280 * t:1280 * (t + 1)]
            want = model.predict(x, patience={"alexa": 2}, threshold={"alexa": 0.3})
            _, got = bo.predict(x, post)
            for k, b in enumerate(bo.sub):
                assert got[k] == want["alexa" if b == 0 else "weather"]


def test_bank_oracle_resubscription_restarts_the_ring():
    emb = W.synthetic_embedding(7)
    h = W.synthetic_head("alexa", 1234)
    noise = W.synthetic_pcm(1, 64000, seed=3, rms=600.0)[0]
    pcm = W.synthetic_pcm(1, 1280 * 9, seed=9)[0]
    bo = BankOracle({0: h, 1: h}, emb, 2, dtype=np.float64, init_noise=noise)
    bo.subscribe([0, 0])
    outs = [bo.predict(pcm[1280 * t:1280 * (t + 1)])[1] for t in range(6)]
    assert outs[5][0] != 0.0 and outs[5][1] == outs[5][0]
    bo.subscribe([0, 1])                               # slot 1: a new head (the same net) -> five zero frames again
    for t in range(6, 9):
        raw, out = bo.predict(pcm[1280 * t:1280 * (t + 1)])
        assert out[1] == 0.0 and out[0] == raw[0] and raw[1] == raw[0]
    assert len(bo.rings[1]) == 3 and len(bo.rings[0]) == 9
