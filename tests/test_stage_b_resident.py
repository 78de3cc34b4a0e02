"""Stage B with its weights resident in LDS (owwhip_hx.h: hstage_kernel NS = 1, OWW_RESIDENT_B / OWW_RESIDENT_B_WGS) against the
ring kernels: the same layer bodies in the same order, so a handle pinned to the resident kernel (OWW_RESIDENT_B=1) and one pinned
to the ring kernels (=0) must agree BIT FOR BIT -- the scores of every step, the feature rings of the first, middle and last stream
and the exported state records of all streams.  OWW_RESIDENT_B_WGS caps the grid, so that tiny batches reach the loop in which a
wave claims several groups of its workgroup's range."""
import numpy as np
import pytest

import cases
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine

pytestmark = pytest.mark.gpu

HEADS3 = ("alexa", "hey_mycroft", "hey_jarvis")
SEEDS = (cases.SEED_WEIGHTS, 4321)
STEPS = 8
_weights = {}


def weights(seed):
    if seed not in _weights:
        _weights[seed] = (W.synthetic_embedding(seed), {n: W.synthetic_head(n, seed) for n in HEADS3})
    return _weights[seed]


def plain(e, pcm):
    return {"scores": np.stack([e.step(pcm[:, 1280 * t: 1280 * (t + 1)]) for t in range(STEPS)])}


def run(monkeypatch, S, resident, wgs, seed=SEEDS[0], scenario=plain, pcm_seed=91, **kw):
    """Everything the comparison looks at, from a fresh handle pinned to one kernel."""
    monkeypatch.setenv("OWW_RESIDENT_B", str(resident))
    if wgs is None:
        monkeypatch.delenv("OWW_RESIDENT_B_WGS", raising=False)
    else:
        monkeypatch.setenv("OWW_RESIDENT_B_WGS", str(wgs))
    emb, heads = weights(seed)
    pcm = W.synthetic_pcm(S, 1280 * STEPS, seed=pcm_seed)
    e = StreamEngine(S, heads, emb, **kw)
    try:
        out = scenario(e, pcm)
        out["features"] = np.stack([e.get_features(s, 16) for s in (0, S // 2, S - 1)])
        out["state"] = e.export_state(np.arange(S))
        assert not e.range_status()
        assert out["scores"][-1].max() > 0
        return out
    finally:
        e.close()
        monkeypatch.delenv("OWW_RESIDENT_B")
        monkeypatch.delenv("OWW_RESIDENT_B_WGS", raising=False)


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def compare(monkeypatch, S, wgs_list, **kw):
    ring = run(monkeypatch, S, 0, None, **kw)
    for wgs in wgs_list:
        same(run(monkeypatch, S, 1, wgs, **kw), ring)


@pytest.mark.parametrize("seed", SEEDS)
def test_fewer_groups_than_waves(monkeypatch, seed):
    """5 streams in one workgroup of 12 waves: seven waves take part in the prologue and the barrier, claim nothing and store nothing."""
    compare(monkeypatch, 5, [None], seed=seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("S", [12, 13])
def test_exact_fill_and_one_over(monkeypatch, S, seed):
    """One workgroup: every wave exactly one group (12), and one wave a second one (13)."""
    compare(monkeypatch, S, [1], seed=seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_waves_take_several_groups(monkeypatch, seed):
    """40 streams on one workgroup (waves take 3 or 4 groups) and on two (ranges of 20: 1 or 2 groups, ragged last claims)."""
    compare(monkeypatch, 40, [1, 2], seed=seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_many_workgroups(monkeypatch, seed):
    """2,500 streams, default grid: 209 workgroups with ranges of 11 and 12 groups -- every workgroup's range boundary."""
    compare(monkeypatch, 2500, [None], seed=seed)


def masked(e, pcm):
    S = e.n_streams
    rng = np.random.default_rng(5)
    scores = [e.step(pcm[:, 1280 * t: 1280 * (t + 1)]) for t in range(6)]
    dense = np.ones(S, np.uint8)
    off = rng.choice(S, 4, replace=False)
    dense[off] = 0                                             # 36 of 40: dense launches, the resident kernel when pinned
    before = e.export_state(off)
    scores.append(e.step_masked(pcm[:, 1280 * 6: 1280 * 7], dense))
    np.testing.assert_array_equal(e.export_state(off), before)
    few = np.zeros(S, np.uint8)
    few[rng.choice(S, 10, replace=False)] = 1                  # 10 of 40: group lists, the ring kernels whatever is pinned
    scores.append(e.step_masked(pcm[:, 1280 * 7: 1280 * 8], few))
    return {"scores": np.stack(scores)}


def test_masked_steps(monkeypatch):
    compare(monkeypatch, 40, [2], scenario=masked)


def long_call_and_clips(e, pcm):
    scores = [e.step(pcm[:, 1280 * t: 1280 * (t + 1)]) for t in range(3)]
    scores.append(e.step(pcm[:, 1280 * 3: 1280 * 6]))          # one call of three chunks
    clips = e.embed_clips(W.synthetic_pcm(8, 16000, seed=17))  # borrows streams 0..7 and puts their state back
    scores += [e.step(pcm[:, 1280 * t: 1280 * (t + 1)]) for t in (6, 7)]
    return {"scores": np.stack(scores), "clips": clips}


def test_three_chunk_call_and_embed_clips(monkeypatch):
    compare(monkeypatch, 40, [2], scenario=long_call_and_clips, max_chunks=3)


def graphed(e, pcm):
    e.use_graph(True)
    return plain(e, pcm)


def test_graph_replay(monkeypatch):
    compare(monkeypatch, 40, [2], scenario=graphed)
