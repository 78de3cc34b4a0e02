"""Every public way of running a step gives the same bits on a handle with everything switched on (tests/call_forms.py: scenarios,
schedule, mutations, forms, trace).  include/owwhip.h promises "Same results as step()" of oww_submit, "exactly oww_step" of a
participating stream of oww_step_masked, "oww_ingest_mixed ... then oww_step" of oww_step_ingest_mixed; the kernels are deterministic
and batch invariant (asserted bit-exactly elsewhere), so equality is the condition: np.array_equal on bits, no tolerance.

Per (scenario, form) one handle makes the scenario's 52 calls in that form and records scores, events, event features, event audio
after every call, bank scores, raw scores, VAD scores and verifier statistics wherever its pipeline is drained, and state records,
audio rings and features of all 70 streams at six checkpoints; the trace must equal the base form's, which is computed once per
scenario.  A failure names the call, the observable and the first differing streams.

The base form itself -- `step` and `step_masked` on host arrays, in scenario III behind `ingest_mixed` to the host -- is not re-derived
here: test_gpu_parity.py, test_masked_step.py, test_head_bank_gpu.py, test_stream_verifiers_gpu.py, test_events_gpu.py,
test_audio_gpu.py, test_postproc_rules_gpu.py, test_vad_regimes.py, test_stream_state_gpu.py and test_ingest_mixed_gpu.py tie it to
float64 and to the reference rules.  What is asserted on the base trace is that it is not vacuous: events (fixed and bank, overflowing
and empty), bank scores, verifier evaluations, the VAD gate and the stream state all move."""
import ctypes as C
import functools

import numpy as np
import pytest

import call_forms as CF
from openwakeword_amd import _lib
from openwakeword_amd import weights as W
from openwakeword_amd.engine import CHUNK, EMB_DIM, EVENT_DTYPE, StreamEngine

pytestmark = pytest.mark.gpu

S, ALL = CF.S, CF.ALL


def _vp(x):
    return None if x is None else (C.c_void_p(int(x)) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))


class Driver:
    """One handle making a scenario's calls in one form."""

    def __init__(self, scenario, form, cal):
        import torch
        self.torch = torch
        self.scenario, self.form, self.cal = scenario, form, cal
        self.cfg, self.spec, self.data = CF.SCENARIOS[scenario], CF.FORMS[form], CF.scenario_data(scenario)
        self.calls, self.ops = CF.schedule(scenario), CF.plan(scenario, form)
        kw = CF.engine_kwargs(scenario)
        if form == "own_stream":
            self.hip_stream = torch.cuda.Stream()
            kw["hip_stream"] = self.hip_stream.cuda_stream
        self.e = StreamEngine(S, CF.fixed_heads(scenario), W.synthetic_embedding(CF.EMB_SEED), **kw)
        self.NL = CF.n_labels(scenario)
        assert self.e.n_labels == self.NL and self.e.feature_ring == CF.t_ring(scenario)
        CF.configure(self.e, scenario, cal)
        if form == "graph":
            self.e.use_graph(True)
        if form == "timing":
            self.e.enable_timing(True)
        self.d_scores = torch.zeros((S, self.NL), dtype=torch.float32, device="cuda")
        self.d_vad = torch.from_numpy(np.ascontiguousarray(self.data["vad"])).cuda()
        torch.cuda.synchronize()
        self.keep = {}                                   # host buffers of submitted steps, until their collect
        self.trace = CF.new_trace()

    def close(self):
        self.e.close()

    # ---- one call -------------------------------------------------------------------------------------------------------------------
    def _push_vad(self, c):
        if not c.push_vad:
            return
        if self.spec.depth == 2:                         # (a host pointer would wait for the step in flight)
            _lib.check(self.e._lib.oww_push_vad(self.e._h, _vp(self.d_vad[c.index].data_ptr()), 1))
        else:
            self.e.push_vad(self.data["vad"][c.index])

    def _pcm(self, c):
        """The call's 16 kHz audio on the host: the scenario's own, or (III) what ingest_mixed makes of the call's messages."""
        if not self.cfg["ingest"]:
            return self.data["pcm"][c.index]
        return self.e.ingest_mixed(self.data["rows"][c.index], n_out=c.n_chunks * CHUNK, stream_on=c.mask)

    def _base(self, c):
        pcm = self._pcm(c)
        return self.e.step(pcm) if c.mask is None else self.e.step_masked(pcm, c.mask)

    def _on_device(self, pcm, offset):
        """pcm on the device, `offset` int16 elements behind a 256-byte aligned address."""
        t = self.torch
        buf = t.zeros(pcm.size + 8, dtype=t.int16, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[offset:offset + pcm.size] = t.from_numpy(np.ascontiguousarray(pcm).ravel()).cuda()
        t.cuda.synchronize()
        return buf, buf.data_ptr() + 2 * offset

    def _device_scores(self):
        self.e.sync()
        return self.d_scores.cpu().numpy().copy()

    def _native(self, c):
        """The call in this form -> scores, or None when it was submitted."""
        e, f, t = self.e, self.form, self.torch
        out = np.empty((S, self.NL), np.float32)
        if f in ("host", "ingest_host", "graph", "timing", "own_stream"):
            return self._base(c)
        if f in ("device", "unaligned"):
            buf, ptr = self._on_device(self._pcm(c), 1 if f == "unaligned" else 0)
            assert ptr % 16 == (2 if f == "unaligned" else 0)
            if c.mask is None:
                e.step_device(ptr, c.n_chunks, self.d_scores.data_ptr())
            else:
                e.step_masked_device(ptr, c.mask, self.d_scores.data_ptr())
            return self._device_scores()
        if f == "device_mask":
            pcm = self._pcm(c)
            d_on = t.from_numpy(np.ones(S, np.uint8) if c.mask is None else np.array(c.mask)).cuda()
            t.cuda.synchronize()
            _lib.check(e._lib.oww_step_masked(e._h, _vp(pcm), 0, _vp(d_on.data_ptr()), 1, _vp(out), 0))
            return out
        if f in ("pipe1", "pipe2"):
            self.keep[c.index] = np.array(self._pcm(c))
            e.submit(self.keep[c.index], stream_on=c.mask)
            return None
        rows = self.data["rows"][c.index]
        if f == "step_ingest":
            return e.step_ingest_mixed(rows, n_out=c.n_chunks * CHUNK, stream_on=c.mask)
        if f in ("submit_ingest1", "submit_ingest2"):
            self.keep[c.index] = np.array(rows)
            e.submit_ingest_mixed(self.keep[c.index], stream_on=c.mask)
            return None
        if f == "ingest_dev":
            d_rows = t.from_numpy(np.array(rows)).cuda()
            t.cuda.synchronize()
            on = None if c.mask is None else np.ascontiguousarray(c.mask)
            _lib.check(e._lib.oww_step_ingest_mixed(e._h, _vp(d_rows.data_ptr()), 1, rows.shape[1], c.n_chunks * CHUNK, _vp(on), 0,
                                                    _vp(out), 0))
            return out
        raise ValueError(f)

    # ---- what is recorded -----------------------------------------------------------------------------------------------------------
    def _record_call(self, i, scores):
        rec, total = self.e.events()
        self.trace["call"][i] = {"scores": scores, "events": rec.view(np.uint8).reshape(len(rec), EVENT_DTYPE.itemsize), "n_total": np.array(total),
                                 "event_streams": rec["stream"].copy(), "event_features": self.e.event_features(),
                                 "event_audio": self.e.event_audio()}

    def _record_drained(self, i):
        e = self.e
        raw = np.empty((S, self.NL), np.float32)
        _lib.check(e._lib.oww_get_raw(e._h, _vp(raw)))
        r = {"bank_scores": e.bank_scores(), "raw": raw, "verifier_stats": np.array(e.verifier_stats())}
        if self.cfg["vad_net"]:
            r["vad"] = e.get_vad()
        self.trace["drained"][i] = r

    def _record_checkpoint(self, i):
        e = self.e
        audio, counts = e.audio(ALL, CF.AUDIO_CHUNKS)
        self.trace["checkpoint"][i] = {"state": e.export_state(ALL), "audio": audio, "audio_counts": counts,
                                       "features": np.stack([e.get_features(s, 16) for s in range(S)])}

    def run(self, n_calls=None):
        for op in self.ops[:n_calls]:
            c = self.calls[op.index]
            if c.index in CF.MUTATIONS:
                self.trace["mutation"][c.index] = CF.mutate(self.e, self.scenario, CF.MUTATIONS[c.index], self.cal)
            self._push_vad(c)
            scores = self._native(c) if op.native else self._base(c)
            if scores is not None:
                self._record_call(c.index, scores)
            for j in op.collects:
                self._record_call(j, self.e.collect())
                self.keep.pop(j, None)
            if op.drained:
                self._record_drained(c.index)
            if c.index in CF.CHECKPOINTS:
                self._record_checkpoint(c.index)
        return self.trace


def _run(scenario, form, cal, n_calls=None):
    d = Driver(scenario, form, cal)
    try:
        return d.run(n_calls)
    finally:
        d.close()


@functools.lru_cache(maxsize=None)
def _base(scenario):
    """(thresholds, base trace) of the scenario, made once."""
    first = min(CF.MUTATIONS)
    probe = _run(scenario, CF.base_form(scenario), None, n_calls=first)
    after = range(CF.WARMUP, first)
    cal = CF.calibrate(np.stack([probe["call"][i]["scores"] for i in after]), np.stack([probe["drained"][i]["bank_scores"] for i in after]))
    return cal, _run(scenario, CF.base_form(scenario), cal)


# ---- the base trace is not vacuous ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", list(CF.SCENARIOS))
def test_base_trace_is_not_vacuous(scenario):
    cal, tr = _base(scenario)
    calls, cfg = CF.schedule(scenario), CF.SCENARIOS[scenario]
    totals = np.array([int(tr["call"][i]["n_total"]) for i in range(CF.N_CALLS)])
    stored = np.array([len(tr["call"][i]["events"]) for i in range(CF.N_CALLS)])
    print(f"scenario {scenario}: n_total per call {totals.tolist()}")
    print(f"scenario {scenario}: {CF.N_CALLS} calls, {int(totals.sum())} hits of which {int(stored.sum())} stored, in {int((totals > 0).sum())} "
          f"calls; {int((totals > CF.EVENT_CAPACITY).sum())} calls overflow, {int((totals[CF.WARMUP:] == 0).sum())} after the warm-up report nothing")
    assert (totals > 0).sum() * 3 >= CF.N_CALLS, "events in fewer than a third of the calls"
    assert (stored == np.minimum(totals, CF.EVENT_CAPACITY)).all()
    assert (totals > CF.EVENT_CAPACITY).any(), "no call overflows the event capacity"
    assert (totals[CF.WARMUP:] == 0).any(), "no call after the warm-up without events"
    assert not totals[:5].any(), "events during the first five predictions"
    columns = np.concatenate([tr["call"][i]["events"].view(EVENT_DTYPE).ravel()["column"] for i in range(CF.N_CALLS)])
    assert (columns >= 0).any() and (columns < 0).any(), "the records do not include both fixed-column and bank-slot records"
    for i in range(CF.N_CALLS):                              # events only of streams that took part
        if calls[i].mask is not None:
            assert calls[i].mask[tr["call"][i]["event_streams"]].all(), f"call {i}: an event of a stream that sat out"
    assert any(tr["call"][i]["event_features"].any() for i in range(CF.N_CALLS)) and any(tr["call"][i]["event_audio"].any() for i in range(CF.N_CALLS))
    # bank scores: exactly 0 on empty slots, non-zero on EVERY subscribed slot that nothing may zero.  Two things may, before mutation
    # C (whose debounce frames are the bank's too): the VAD gate, which zeroes a stream's fixed scores with its bank scores -- so a
    # stream with a non-zero fixed score has its gate open -- and the patience rule that configure() puts on bank head 0.
    # (Between mutations A and D the table is current_subscriptions().)
    at = {v: k for k, v in CF.MUTATIONS.items()}
    assert 12 < at["A"] <= 27 < at["C"] < at["D"]
    for i, sub in ((12, CF.subscriptions()), (27, CF.current_subscriptions())):
        bs, gate_open = tr["drained"][i]["bank_scores"], (tr["call"][i]["scores"] != 0).any(axis=1)
        assert (bs[sub < 0] == 0).all(), f"call {i}: a bank score on an empty slot"
        must = (sub > 0) & gate_open[:, None]
        print(f"scenario {scenario}, call {i}: {int(must.sum())} subscribed slots with an open gate and no patience rule")
        assert must.sum() >= 20 and (bs[must] != 0).all(), f"call {i}: a subscribed slot with an open gate scores nothing"
    # verifiers: evaluations after B, none after F
    b, f = at["B"], at["F2"]                                 # (F removes the handle-wide verifier, F2 every per-stream assignment)
    assert tr["drained"][b]["verifier_stats"][0] > 0 and tr["drained"][b]["verifier_stats"][1] > 0
    assert max(tr["drained"][i]["verifier_stats"][1] for i in range(b, f)) > 0
    assert all(tr["drained"][i]["verifier_stats"][1] == 0 for i in range(f, CF.N_CALLS)) and tr["drained"][f]["verifier_stats"][0] == 0
    assert all(tr["drained"][i]["verifier_stats"][1] == 0 for i in range(b))
    # the VAD gate both zeroes and passes: a stream with a non-zero raw score reads 0 in one place and its score in another.  Counted
    # on the unmasked calls between the warm-up and mutation C only: there no stream is inside its first five predictions (D resets
    # later) and no patience, threshold or debounce rule is set on a fixed column, so nothing but the gate zeroes a row.
    gated = passed = 0
    for i in range(CF.WARMUP, at["C"]):
        if calls[i].mask is None:
            raw, sc = tr["drained"][i]["raw"], tr["call"][i]["scores"]
            gated += int(((raw != 0).all(axis=1) & (sc == 0).all(axis=1)).sum())
            passed += int((sc != 0).any(axis=1).sum())
    print(f"scenario {scenario}: VAD gate zeroed {gated} stream-calls and passed {passed}")
    assert gated > 0 and passed > 0
    if cfg["vad_net"]:
        vad = np.stack([tr["drained"][i]["vad"] for i in range(CF.N_CALLS)])
        assert (vad < 0.5).any() and (vad > 0.5).any(), "get_vad() stays on one side of the gate"
    # state: moves between checkpoints; a stream that sat out kept every bit -- across a dense mask (group lists) and the empty mask
    # (nothing launched), and across a wide mask (full launches whose stores skip the streams that sit out)
    cps = list(CF.CHECKPOINTS)
    for a, b2 in zip(cps[:-1], cps[1:]):
        assert (tr["checkpoint"][a]["state"] != tr["checkpoint"][b2]["state"]).any(), f"the state records after calls {a} and {b2} are equal"
    for lo, hi in CF.SAT_OUT_BRACKETS:
        between = [c for c in calls[lo + 1:hi + 1]]
        assert all(c.mask is not None for c in between)
        on = np.any([c.mask != 0 for c in between], axis=0)
        assert not on.all()
        for name in CF.CHECKPOINT:
            x, y = tr["checkpoint"][lo][name], tr["checkpoint"][hi][name]
            moved = (x != y).reshape(S, -1).any(axis=1)
            assert not moved[~on].any(), f"{name}: streams {np.flatnonzero(moved & ~on)[:6].tolist()} sat out calls {lo + 1} .. {hi} and changed"
            assert moved[on].any(), f"{name}: nobody who took part in calls {lo + 1} .. {hi} changed"
    for i, c in enumerate(calls):                            # a stream that sits a call out repeats its previous scores, whatever the launches
        if c.mask is not None and i:
            off = c.mask == 0
            assert np.array_equal(tr["call"][i]["scores"][off].view(np.uint32), tr["call"][i - 1]["scores"][off].view(np.uint32)), \
                f"call {i} ({c.kind}): a stream that sat out does not repeat its previous scores"
    for i in cps:                                            # junk rows are constant: no such chunk may have reached a ring
        ring = tr["checkpoint"][i]["audio"].reshape(S, -1, CHUNK)
        assert not ((ring == ring[:, :, :1]).all(axis=2) & (ring[:, :, 0] != 0)).any(), f"call {i}: a junk row was read"
    # the dense scoring calls of mutation E returned something
    e = next(k for k, v in CF.MUTATIONS.items() if v == "E")
    assert all(np.asarray(v).any() for v in tr["mutation"][e].values())
    assert tr["mutation"][e]["embed_clips"].shape == (8, 4, EMB_DIM)


# ---- which scenario takes the in-heads epilogue ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,rides", [("II", False), ("IIe", True)])
def test_which_scenario_takes_the_in_heads_epilogue(scenario, rides):
    """postproc_kernel is a launch of its own (kernel class "postproc") unless post-processing rides in the heads launch: one narrow
    group of fixed heads, a one-chunk call, no verifier of either kind.  IIe is that configuration until mutation B and after F2;
    with the multiclass head (I - III) the launch is always there."""
    d = Driver(scenario, "timing", None)
    try:
        e, pcm = d.e, d.data["pcm"][0]

        def launches():
            e.kernel_times()                                 # (reading resets the counters)
            e.step(pcm)
            return e.kernel_times()["postproc"]["launches"]
        plain = launches()
        v = e.verifier_add(d.data["verifier_w"][0], d.data["verifier_b"][0])
        e.assign_verifiers(0, [0], [v], [0.0])
        assigned = launches()
        e.assign_verifiers(0, [0], [-1], [0.0])
        e.set_verifier(1, d.data["verifier_w"][2], d.data["verifier_b"][2], threshold=0.05)
        handle_wide = launches()
        e.set_verifier(1, None)
        assert launches() == plain
        assert assigned == handle_wide == plain + (1 if rides else 0), (plain, assigned, handle_wide)
    finally:
        d.close()


# ---- every form against the base form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,form", CF.CASES)
def test_form_equals_base(scenario, form):
    cal, base = _base(scenario)
    got = _run(scenario, form, cal)
    assert sorted(got["call"]) == list(range(CF.N_CALLS)), "a call's observables were not recorded"
    assert sorted(got["checkpoint"]) == sorted(CF.CHECKPOINTS) and sorted(got["mutation"]) == sorted(CF.MUTATIONS)
    assert sorted(got["drained"]) == [op.index for op in CF.plan(scenario, form) if op.drained], "a drained call's getters were not read"
    diffs = CF.compare(base, got, form)
    print(f"scenario {scenario}, form {form}: {got['n_compared']} comparisons, {len(diffs)} differ")
    assert not diffs, f"scenario {scenario}, form {form}: {len(diffs)} of {got['n_compared']} observables differ from the base form:\n  " + \
        "\n  ".join(diffs[:12])
