"""The schedule, the form table and the submit / collect order of tests/call_forms.py, held to the conditions that make
tests/test_call_forms_gpu.py mean something -- without a GPU."""
import numpy as np
import pytest

import call_forms as CF
from openwakeword_amd import resample as R

SCENARIOS = list(CF.SCENARIOS)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_schedule_shape(scenario):
    calls = CF.schedule(scenario)
    assert 44 <= len(calls) <= 54 and len(calls) == CF.N_CALLS
    assert all(c.kind == "u1" for c in calls[:CF.WARMUP]) and CF.WARMUP >= 8          # the first-five zeroing lies inside the warm-up
    assert [c.index for c in calls] == list(range(len(calls)))
    assert [c.first_chunk for c in calls] == np.concatenate([[0], np.cumsum([c.n_chunks for c in calls])[:-1]]).tolist()
    kmax = CF.SCENARIOS[scenario]["max_chunks"]
    for c in calls:
        assert c.kind in CF.KINDS
        assert (c.mask is None) == (c.kind in ("u1", "u2", "long"))
        assert c.n_chunks == 1 if c.kind not in ("u2", "long") else (c.n_chunks == kmax == 2 if c.kind == "u2" else c.n_chunks > kmax)
    if kmax == 1:
        assert all(c.n_chunks == 1 for c in calls)                                    # the VAD network refuses longer calls
    else:
        assert sorted(c.n_chunks for c in calls if c.kind == "long") == [3, 3, 5]     # slices 2 + 1 and 2 + 2 + 1
        assert sum(c.kind == "u2" for c in calls) >= 2
    for kind in CF.MASKED:
        assert any(c.kind == kind for c in calls)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_every_mask_has_its_density_class(scenario):
    took_part, sat_out = np.zeros(CF.S, bool), np.zeros(CF.S, bool)
    for c in CF.schedule(scenario):
        if c.mask is None:
            continue
        assert c.mask.dtype == np.uint8 and c.mask.shape == (CF.S,) and set(np.unique(c.mask)) <= {0, 1}
        frac, n = float(c.mask.mean()), int(c.mask.sum())
        # which launches a host mask takes: owl::participants (csrc/owwhip_masked_host.h; tests/planners_check.cpp "the 7/8 rule")
        assert CF.takes_full_launches(c.mask) == (8 * n > 7 * CF.S) == (c.kind in CF.FULL_LAUNCH_MASKS)
        assert (c.kind in CF.LIST_MASKS) == (0 < 8 * n <= 7 * CF.S)
        if c.kind == "dense":
            assert 0.55 <= frac <= 0.85, (c.index, frac)                              # most streams, and still the group lists
        elif c.kind == "sparse":
            assert 0 < frac <= 0.30, (c.index, frac)
        elif c.kind == "wide":
            assert 62 <= n <= 69, (c.index, n)                                        # the full launches with somebody sitting out
        elif c.kind == "empty":
            assert frac == 0
        else:
            assert frac == 1
        if c.kind in ("dense", "sparse", "wide"):
            assert c.mask[0] == 1 and c.mask[1] == 0                                  # stream 0 in every mask, stream 1 in none
            took_part |= c.mask != 0
            sat_out |= c.mask == 0
    assert took_part[2:].all() and sat_out[2:].all(), "a stream other than 0 and 1 never takes part or never sits out"
    assert not took_part[1] and not sat_out[0]


def test_every_call_kind_has_two_native_forms_besides_the_base():
    for scenario in SCENARIOS:
        kinds = {c.kind for c in CF.schedule(scenario)}
        assert kinds == (set(CF.KINDS) if CF.SCENARIOS[scenario]["max_chunks"] > 1 else set(CF.KINDS) - {"u2", "long"})
        for kind in kinds:
            native = [f for f in CF.forms_of(scenario) if kind in CF.FORMS[f].native]
            assert len(native) >= 2, (scenario, kind, native)


def test_form_table():
    assert set(CF.FORMS) == {"host", "graph", "timing", "device", "device_mask", "unaligned", "pipe1", "pipe2", "own_stream",
                             "ingest_host", "step_ingest", "submit_ingest1", "submit_ingest2", "ingest_dev"}
    for name, spec in CF.FORMS.items():
        assert spec.native <= set(CF.KINDS) and spec.depth in (0, 1, 2) and spec.drives
        assert bool(spec.fallback) == (spec.native != set(CF.KINDS)), f"{name}: a form that falls back says why, and only such a form"
        assert all(isinstance(k, str) and isinstance(v, str) and v for k, v in spec.exempt.items()), "an exemption carries its reason"
    assert CF.base_form("I") == CF.base_form("II") == CF.base_form("IIe") == "host" and CF.base_form("III") == "ingest_host"
    for scenario in SCENARIOS:
        assert CF.FORMS[CF.base_form(scenario)].native == set(CF.KINDS) and CF.base_form(scenario) not in CF.forms_of(scenario)
    assert set(CF.forms_of("III")) - set(CF.forms_of("II")) == {"step_ingest", "submit_ingest1", "submit_ingest2", "ingest_dev"}
    assert len(CF.CASES) == len(set(CF.CASES)) == sum(len(CF.forms_of(s)) for s in SCENARIOS)


@pytest.mark.parametrize("scenario,form", CF.CASES)
def test_plan(scenario, form):
    calls, ops, spec = CF.schedule(scenario), CF.plan(scenario, form), CF.FORMS[form]
    assert [op.index for op in ops] == list(range(len(calls)))
    native = [op for op in ops if op.native]
    assert len(native) >= 0.6 * len(calls), f"{form} drives {len(native)} of {len(calls)} calls itself"
    assert all(op.native == (calls[op.index].kind in spec.native) for op in ops)
    # every submitted call is collected exactly once, in order, never more than `depth` in flight, and nothing is in flight across a
    # mutation, a checkpoint, a call in the base form or the end
    in_flight, collected, behind = [], [], []                # behind: (the call in flight, the call submitted behind it)
    for op in ops:
        if not op.native or spec.depth == 0:
            assert not in_flight and op.in_flight == 0 and op.drained and (not op.collects or spec.depth)
        if op.index in CF.MUTATIONS:
            assert not in_flight
        if op.native and spec.depth:
            assert op.in_flight == len(in_flight) < spec.depth
            behind += [(in_flight[-1], op.index)] if in_flight else []
            in_flight.append(op.index)
        for j in op.collects:
            assert in_flight and j == in_flight.pop(0)
            collected.append(j)
        assert op.drained == (not in_flight)
        if op.index in CF.CHECKPOINTS:
            assert op.drained
    assert not in_flight and ops[-1].drained
    assert collected == ([op.index for op in native] if spec.depth else [])
    if spec.depth == 2:
        assert 3 * len(behind) >= len(calls), f"{form}: {len(behind)} of {len(calls)} calls are submitted behind another"
        assert any(calls[a].kind == calls[b].kind == "sparse" for a, b in behind), \
            f"{form}: no sparse-masked call is submitted while a sparse-masked call is in flight (the staging lists' turn)"
        assert any({calls[a].kind, calls[b].kind} & set(CF.LIST_MASKS) and "wide" in (calls[a].kind, calls[b].kind) for a, b in behind), \
            f"{form}: no list mask and host-masked full launch follow each other with both in flight"
    else:
        assert not behind


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_mutations_and_checkpoints(scenario):
    calls = CF.schedule(scenario)
    assert [CF.MUTATIONS[k] for k in sorted(CF.MUTATIONS)] == ["A", "B", "B2", "C", "C2", "D", "E", "F", "F2"]
    for at in CF.MUTATIONS:
        assert at >= CF.WARMUP and calls[at].kind == calls[at + 1].kind == "u1", f"mutation before call {at}: a captured graph must be re-captured AND replayed"
    assert len(CF.CHECKPOINTS) == 6 and CF.CHECKPOINTS[-1] == len(calls) - 1 and list(CF.CHECKPOINTS) == sorted(set(CF.CHECKPOINTS))
    unpushed = set()
    for lo, hi in CF.SAT_OUT_BRACKETS:
        assert lo in CF.CHECKPOINTS and hi in CF.CHECKPOINTS and all(c.mask is not None for c in calls[lo + 1:hi + 1])
        assert not any(at in range(lo + 1, hi + 1) for at in CF.MUTATIONS)
        assert all(not calls[i].push_vad for i in range(lo + 1, hi + 1))              # (a pushed VAD score moves every stream's ring)
        unpushed |= set(range(lo + 1, hi + 1))
    # one bracket holds a list mask and the empty mask, the other a host-masked full launch that somebody sits out
    (a, b), (c, d) = CF.SAT_OUT_BRACKETS
    assert [x.kind for x in calls[a + 1:b + 1]] == ["dense", "empty"] and [x.kind for x in calls[c + 1:d + 1]] == ["wide"]
    assert 0 < int((calls[d].mask == 0).sum()) <= 8 and CF.takes_full_launches(calls[d].mask)
    if not CF.SCENARIOS[scenario]["vad_net"]:
        assert sum(x.push_vad for x in calls) == len(calls) - len(unpushed)


def test_stream_lists_of_mutation_d():
    src, dst = CF.MOVE_SRC, CF.MOVE_DST
    assert len(src) == len(dst) and len(set(src)) == len(src) and len(set(dst)) == len(dst) and set(src) == set(dst)
    cycles, seen = [], set()
    nxt = dict(zip(src, dst))
    for s in src:
        if s not in seen:
            n, t = 0, s
            while t not in seen:
                seen.add(t)
                t, n = nxt[t], n + 1
            cycles.append(n)
    assert sorted(cycles) == [2, 3]                                                   # a swap and a 3-cycle
    assert all(CF.CLS[a] == CF.CLS[b] for a, b in zip(src, dst))                      # scenario III: a stream keeps its message format
    assert all(CF.CLS[a] == CF.CLS[b] for a, b in zip(CF.EXPORT_IDS, CF.IMPORT_IDS))
    groups = [CF.RESET_IDS, src, CF.EXPORT_IDS, CF.IMPORT_IDS]
    flat = [s for g in groups for s in g]
    assert len(flat) == len(set(flat)) and all(0 <= s < CF.S for s in flat), "reset, move, export and import lists overlap"
    assert len(CF.RESET_IDS) == 5 and len(CF.EXPORT_IDS) == len(CF.IMPORT_IDS) == 4
    assert CF.RESUBSCRIBED.size in (17, 18)                                           # a quarter of the streams


def test_subscriptions_and_heads():
    sub = CF.subscriptions()
    assert sub.shape == (CF.S, CF.K) and sub.min() == -1 and sub.max() == 2
    assert 0.15 < (sub < 0).mean() < 0.5 and (sub[3] < 0).all() and (sub[0] >= 0).all()
    assert {CF.bank_head(i)["hidden"] for i in range(3)} == {32, 64, 128}
    cur = CF.current_subscriptions()
    assert (cur[CF.NEW_HEAD_IDS, 1] == 1).all() and (cur == 1).sum() == CF.NEW_HEAD_IDS.size and not set(CF.NEW_HEAD_IDS) & set(CF.RESUBSCRIBED)
    for scenario in SCENARIOS:
        heads = CF.fixed_heads(scenario)
        assert [h["kind"] for h in heads.values()] == ["binary", "gated", "multiclass"][:len(heads)]
        assert sum(h["n_out"] for h in heads.values()) == CF.n_labels(scenario)
        assert max([16] + [h["T"] for h in heads.values()]) == CF.t_ring(scenario)
        assert CF.S * (CF.n_labels(scenario) + CF.K) > 256                            # the event kernels run more than one workgroup
        # the in-heads epilogue needs ONE group of narrow nets (up to 64 units): only IIe has it
        assert (scenario == "IIe") == all(h["hidden"] <= 64 and h["kind"] != "multiclass" for h in heads.values())


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_inputs(scenario):
    d, calls = CF.scenario_data(scenario), CF.schedule(scenario)
    key = "rows" if CF.SCENARIOS[scenario]["ingest"] else "pcm"
    assert len(d[key]) == len(calls)
    for c in calls:
        x = d[key][c.index]
        on = np.ones(CF.S, bool) if c.mask is None else c.mask != 0
        if key == "pcm":
            assert x.dtype == np.int16 and x.shape == (CF.S, c.n_chunks * CF.CHUNK)
            assert (x[~on] == CF.JUNK16).all()
        else:
            assert x.dtype == np.uint8 and x.shape == (CF.S, R.class_row_bytes(CF.INGEST_CLASSES, c.n_chunks * CF.CHUNK))
            assert (x[~on] == 0xA5).all()
    if key == "pcm":                                                                  # distinct streams, some of them silent
        whole = np.concatenate([d["pcm"][i] for i in range(CF.WARMUP)], axis=1)
        assert len({row.tobytes() for row in whole}) >= CF.S - 5 and (whole == 0).all(axis=1).any()
    v = d["vad"]
    assert v.shape == (len(calls), CF.S) and ((v < 0.4).mean(axis=1) > 0.2).all() and ((v > 0.6).mean(axis=1) > 0.2).all()


def test_audio_is_the_state_suites():
    from test_stream_state_gpu import _audio                                          # (importing it needs no GPU)
    for n, T, seed in ((7, 2, 5), (33, 3, 104)):
        want = _audio(n, T, seed).transpose(1, 0, 2).reshape(n, T * CF.CHUNK)
        assert np.array_equal(CF._audio(n, T, seed), want)


def test_ulaw_encoder_round_trips():
    codes = np.arange(256, dtype=np.uint8)
    x = R.decode_ulaw(codes)
    assert (R.decode_ulaw(CF.encode_ulaw(x)) == x).all()
    r = np.random.default_rng(0).integers(-32768, 32768, 4096).astype(np.int16)
    err = np.abs(R.decode_ulaw(CF.encode_ulaw(r)).astype(np.int32) - r)
    assert (err <= np.maximum(np.abs(r.astype(np.int32)) // 16, 8) + 700 * (np.abs(r.astype(np.int32)) > 32000)).all()


def test_compare_names_call_observable_and_streams():
    base, got = CF.new_trace(), CF.new_trace()
    a = np.zeros((CF.S, 3), np.float32)
    b = a.copy()
    b[[7, 40], 1] = 1e-9
    base["call"][5] = {"scores": a, "n_total": np.array(2)}
    got["call"][5] = {"scores": b, "n_total": np.array(2)}
    base["drained"][5] = {"raw": a}
    got["checkpoint"][5] = {"state": a}                                               # an observable the form did not record is an error
    base["checkpoint"][5] = {"state": a, "audio": a}
    with pytest.raises(AssertionError, match="recorded"):
        CF.compare(base, got, "graph")
    del got["checkpoint"][5]
    diffs = CF.compare(base, got, "graph")
    assert diffs == ["call 5, scores: 2 streams differ, first [7, 40]"] and got["n_compared"] == 2
    got["call"][5]["scores"] = np.where(a == 0, np.float32(-0.0), a)                   # bits, not values
    assert len(CF.compare(base, got, "graph")) == 1
    got["call"][5]["scores"] = a.copy()
    assert CF.compare(base, got, "graph") == []
