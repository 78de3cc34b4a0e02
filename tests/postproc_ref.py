"""Model.predict's post-processing (the reference's model.py:330-381) as two independent restatements, and the call schedule the
post-processing tests drive through them and through the device.

`reference_rules` is the literal form: one `collections.deque(maxlen=30)` per (stream, label) or (stream, slot), one Python list of
voice-activity scores per stream, sliced as `[-patience:]`, `[-n_frames:]` and `[-7:-4]`.  `device_rules` is the form the device code takes
(csrc/owwhip_postproc.h, called by owk::postproc_kernel, the epilogue of owh::heads_hx_kernel, owh::bank_post_kernel): a uint32 count, `ring[cnt % 30]`,
`have = min(cnt, 30)`, a VAD ring of 8 indexed by `L & 7` -- vectorised over streams and labels -- and it takes a named FAULT, one
plausible slip of such a kernel each.  The rules are discrete (a final score is the raw score's bits or 0.0), so the two forms, and the
device, are compared by np.array_equal on the float32 bits; the faults say whether a comparison could have noticed anything.

The batched contract is include/owwhip.h's: thresholds are float32 (so every comparison is made in float32); patience[l] > 0 selects the
patience rule for label l, otherwise debounce_frames > 0 and a non-NaN threshold select the debounce rule; oww_reset empties the
prediction rings of its streams and leaves the VAD history alone, oww_reset_vad empties the VAD history; a slot whose bank head changes
starts a fresh ring; a stream that sits a masked step out is not called (ring and count stay, its row of scores repeats);
oww_push_vad appends for every stream; a multi-chunk call is ONE predict (one append, one count).  What a sat-out stream's bank row
reads right after oww_reset / oww_subscribe cleared it (0.0) is the library's own convention; the schedule never relies on it."""
from collections import deque

import numpy as np

F32 = np.float32
DEPTH = 30

FAULTS = (
    "first5_lt4", "first5_le5",
    "gt_history_patience", "gt_history_debounce", "gt_current_debounce",
    "window_short", "window_long", "ring_slot_slip", "ring_depth_29", "gate_before_append",
    "vad_window_late", "vad_window_early", "vad_warmup_4", "vad_le",
    "nan_threshold_debounced", "masked_stream_counts",
    "slot_keeps_count_on_resubscribe", "slot_uses_stream_count", "count_per_chunk",
)
FAULT_NOTES = {
    "first5_lt4": "first-five zeroing while cnt < 4",
    "first5_le5": "first-five zeroing while cnt <= 5",
    "gt_history_patience": "patience counts ring entries > threshold",
    "gt_history_debounce": "debounce counts ring entries > threshold",
    "gt_current_debounce": "debounce needs the current score > threshold",
    "window_short": "patience / debounce look one entry short",
    "window_long": "patience / debounce look one entry long",
    "ring_slot_slip": "ring read shifted by one slot",
    "ring_depth_29": "ring of 29",
    "gate_before_append": "the ring keeps the VAD-gated value",
    "vad_window_late": "VAD window [-6:-3]",
    "vad_window_early": "VAD window [-8:-5]",
    "vad_warmup_4": "VAD window opens at L = 4 (on entry 0)",
    "vad_le": "VAD gate closes at equality",
    "nan_threshold_debounced": "a NaN threshold debounces as threshold 0",
    "masked_stream_counts": "a sat-out stream's count advances",
    "slot_keeps_count_on_resubscribe": "a resubscribed slot keeps count and ring",
    "slot_uses_stream_count": "bank slots use the stream's count",
    "count_per_chunk": "a k-chunk call counts k times",
}


def ulp(v, n):
    """float32 `v` moved n (-1, 0, 1) representable values."""
    v = F32(v)
    return v if n == 0 else np.nextafter(v, F32(np.inf if n > 0 else -np.inf), dtype=F32)


# ---------------------------------------------------------------------------------------------------------------------------
# the schedule: a list of operations in call order
#   ("post", patience [NL], threshold [NL], debounce_frames)     oww_set_postproc
#   ("bank_post", head, patience, threshold)                       oww_bank_set_postproc
#   ("gate", threshold)                                            oww_set_vad_threshold
#   ("vad", scores [S])                                            oww_push_vad
#   ("reset", ids) / ("reset_vad", ids)                            oww_reset / oww_reset_vad
#   ("sub", ids, bank_ids [n, K])                                  oww_subscribe
#   ("call", k, on)                                                oww_step with k chunks (on None) / oww_step_masked (k = 1, on [S])
# ---------------------------------------------------------------------------------------------------------------------------
class Schedule:
    def __init__(self, S, NL, K, H):
        self.S, self.NL, self.K, self.H = S, NL, K, H
        self.ops = []

    @property
    def calls(self):
        return [op for op in self.ops if op[0] == "call"]

    @property
    def n_calls(self):
        return len(self.calls)

    def without_rules(self):
        """The same calls with no rules and no gate: what the twin handle runs."""
        out = Schedule(self.S, self.NL, self.K, self.H)
        out.ops = [op for op in self.ops if op[0] not in ("post", "bank_post", "gate")]
        return out

    def features(self):
        """What the schedule exercises: decides which faults could show at all."""
        return {"masked": any(op[2] is not None for op in self.calls), "multi": any(op[1] > 1 for op in self.calls),
                "bank": self.K > 0, "fixed": self.NL > 0, "gate": any(op[0] == "gate" and op[1] > 0 for op in self.ops),
                "patience": any(op[0] == "post" and max(op[1], default=0) > 0 for op in self.ops),
                "debounce": any(op[0] == "post" and op[3] > 0 for op in self.ops)}

    def applicable(self):
        f = self.features()
        out = []
        for name in FAULTS:
            if name == "masked_stream_counts" and not f["masked"]:
                continue
            if name == "count_per_chunk" and not f["multi"]:
                continue
            if name.startswith("slot_") and not f["bank"]:
                continue
            out.append(name)
        return out


PATS = (1, 2, 3, 29, 30, 31)
VAD_THR = F32(0.5)
N_CALLS = 70
TWO_CHUNK = (5, 18, 31, 46, 60)
THREE_CHUNK = (24, 53)
MASKED = (9, 15, 16, 27, 38, 45, 56, 64)
DENSE_MASK = 27                       # (almost every stream takes part: the dense launches with a mask)
RESETS = ((7, 4), (41, 5))            # (call, m): streams with s % m == 0 (call 7) / s % m == 2 (call 41) are reset before it
VAD_RESETS = ((20, 3), (50, 4))       # streams with s % m == 0
GATE = ((0, VAD_THR), (26, F32(0.0)), (33, VAD_THR))
DEBOUNCE = ((35, 4), (40, 1), (44, 29), (49, 30), (54, 31), (59, 40))
PATIENCE_2 = 14
FINAL_PATIENCE = 63
SUB_CHANGES = (25, 48)


def _pick_default(kind, idx, q, n=0, calls=None, segments=None):
    return ulp(0.5, n)


def vad_script(S, C=N_CALLS, seed=5):
    """[C, S] scripted voice-activity scores from {0, thr - ulp, thr, thr + ulp, 1}: lows three times in five, and per stream two
    isolated highs (exactly thr, and thr + ulp) in a run of lows, so that each position of the three-entry window decides the gate
    alone as the window slides over them; the pushes right after a VAD reset are 1.0 (a window that opens a push early would read
    them)."""
    r = np.random.default_rng(seed)
    lo, hi = (F32(0.0), ulp(VAD_THR, -1)), (VAD_THR, ulp(VAD_THR, 1), F32(1.0))
    v = np.empty((C, S), F32)
    for c in range(C):
        for s in range(S):
            v[c, s] = lo[r.integers(2)] if r.random() < 0.6 else hi[r.integers(3)]
    for s in range(S):
        for a, val in ((10 + s % 3, VAD_THR), (56 + s % 3, ulp(VAD_THR, 1))):
            for c in range(a - 3, a + 4):
                v[c, s] = lo[(c + s) % 2]
            v[a, s] = val
        for c0, m in VAD_RESETS:
            if s % m == 0:
                v[c0, s] = F32(1.0)
    return v


def make_schedule(S, NL, pick=_pick_default, K=0, H=0, two=TWO_CHUNK, three=THREE_CHUNK, masked=MASKED, n_calls=N_CALLS, vad_seed=5):
    """The 70-call schedule of the post-processing tests.  pick(kind, index, q, n) -> a float32 threshold: the q-quantile ELEMENT of the
    raw table of fixed label / bank head `index`, moved n float32 steps -- so that score == threshold really occurs.
    Two patience phases (calls 0-13 with one rule-free label, 14-34; counts 29, 30, 31 are crossed there), six debounce phases (frames 4, 1, 29, 30, 31, 40; the ring wraps
    the second time in the last), and a final patience phase with the patience values rotated."""
    sc = Schedule(S, NL, K, H)
    ops = sc.ops
    phase = (0, n_calls)
    vad = vad_script(S, n_calls, vad_seed)

    def post_patience(rot, free=None):
        pat = [0 if l % 6 == free else PATS[(l + rot) % 6] for l in range(NL)]
        thr = []
        for l, p in enumerate(pat):
            # 29 and 30 fire only behind a full ring of hits: thresholds 0.0 and negative, where the zeros of the first five frames
            # and of earlier refusals count as hits -- in the reference too.  31 can never fire.
            thr.append(F32(0.0) if p == 29 else F32(-0.25) if p == 30 else pick("fixed", l, 0.5 - 0.1 * (p == 3), (l + rot) % 3 - 1, phase))
        return ("post", pat, np.array(thr, F32), 0)

    def post_debounce(frames):
        thr = [pick("fixed", l, 0.7, (l + frames) % 3 - 1, phase, [(phase[0], phase[1], frames)]) for l in range(NL)]
        if NL:
            thr[NL - 1 if NL < 6 else 5] = F32(np.nan)       # one label without a threshold: never debounced
        if NL > 6:
            thr[6] = F32(0.0)                                 # threshold 0.0 in debounce mode: every entry is a hit
        return ("post", [0] * NL, np.array(thr, F32), frames)

    sub = np.full((S, K), -1, np.int64)
    if K:
        assert K == 3 and H == 2
        for s in range(S):
            sub[s] = ((0, 1, -1), (1, -1, 0), (-1, 0, -1))[s % 3]
        ops.append(("sub", np.arange(S), sub.copy()))
        ops.append(("bank_post", 0, 2, pick("bank", 0, 0.5, 0, (0, 35))))
        ops.append(("bank_post", 1, 0, F32(np.nan)))                                  # (off: first-five zeroing alone)
    starts = sorted([0, PATIENCE_2, FINAL_PATIENCE] + [c0 for c0, _ in DEBOUNCE]) + [n_calls]
    for c in range(n_calls):
        if c in starts:
            phase = (c, starts[starts.index(c) + 1])
        for c0, thr in GATE:
            if c == c0:
                ops.append(("gate", thr))
        if c == 0:
            ops.append(post_patience(0, free=2))       # (one label without a rule: the first-five zeroing shows on its own)
        if c == PATIENCE_2:
            ops.append(post_patience(1))
        for c0, frames in DEBOUNCE:
            if c == c0:
                ops.append(post_debounce(frames))
        if c == FINAL_PATIENCE:
            ops.append(post_patience(3))
        if K and c == 35:
            ops.append(("bank_post", 0, 30, F32(0.0)))
            ops.append(("bank_post", 1, 0, pick("bank", 1, 0.7, 0, (35, 52), [(c0, c1, f) for (c0, f), c1 in zip(DEBOUNCE[:4], (40, 44, 49, 52))])))
            # (debounced with the handle's frames)
        if K and c == 52:
            ops.append(("bank_post", 0, 0, pick("bank", 0, 0.7, 0, (52, n_calls), [(52, 54, 30), (54, 59, 31), (59, 63, 40)])))
            ops.append(("bank_post", 1, 1, pick("bank", 1, 0.5, 1, (52, n_calls))))
        if c == RESETS[0][0]:
            ops.append(("reset", np.array([s for s in range(S) if s % RESETS[0][1] == 0])))
        if c == RESETS[1][0] and S > 2:
            ops.append(("reset", np.array([s for s in range(S) if s % RESETS[1][1] == 2])))
        for c0, m in VAD_RESETS:
            if c == c0:
                ops.append(("reset_vad", np.array([s for s in range(S) if s % m == 0])))
        if K and c in SUB_CHANGES:
            first = c == SUB_CHANGES[0]
            ids = np.array([s for s in range(S) if (s % 2 == 0 if first else s % 3 != 1)])
            new = sub[ids][:, (0, 2, 1) if first else (1, 0, 2)]       # one slot of the three keeps its head
            sub[ids] = new
            ops.append(("sub", ids, new.copy()))
        ops.append(("vad", vad[c]))
        if c in masked:
            on = np.array([s != 5 if c == DENSE_MASK else (s * 7 + c) % 3 != 0 for s in range(S)])
            ops.append(("call", 1, on))
        else:
            ops.append(("call", 2 if c in two else 3 if c in three else 1, None))
    return sc


_HANDOVER_TWO = tuple(c for c in range(N_CALLS) if c % 4 == 1)
_HANDOVER_MASKED = tuple(c for c in range(N_CALLS) if c % 5 == 3 and c % 4 != 1)
# the call shapes of each GPU path (tests/test_postproc_rules_gpu.py); the CPU tier checks on scripted tables that each of them
# lets every applicable fault show
PATHS = {
    "epilogue": dict(NL=3, two=(), three=()),
    "family1": dict(NL=3),
    "family0": dict(NL=3, masked=()),                 # (masked steps need the register-resident families)
    "default6": dict(NL=12),
    "long": dict(NL=3),
    "verifier": dict(NL=3, two=(), three=()),
    "handover": dict(NL=3, two=_HANDOVER_TWO, three=(), masked=_HANDOVER_MASKED),
    "bank": dict(NL=1, K=3, H=2, three=()),
    "graph": dict(NL=3, two=(), three=(), masked=()),
}


def scripted_tables(S, NL, H, C=N_CALLS, seed=0):
    """Raw-score tables without a device: raw [C, S, NL], head_raw [C, S, H], drawn from a few levels -- exact 0.0 and 1.0, and five
    values each with its float32 neighbours either side -- so that a threshold picked from the table meets equal scores and scores one
    ulp above and below it all the time."""
    r = np.random.default_rng(seed)
    levels = [F32(0.0), F32(1.0)]
    for base in (0.2, 0.35, 0.5, 0.65, 0.8):
        levels += [ulp(base, -1), ulp(base, 0), ulp(base, 1)]
    levels = np.array(levels, F32)
    p = np.array([0.03, 0.03] + [0.94 / 15] * 15)
    return (levels[r.choice(len(levels), size=(C, S, NL), p=p)], levels[r.choice(len(levels), size=(C, S, H), p=p)])


def _decisive(tab, segments, cand):
    """For each candidate threshold: how often, over the (first call, end, frames) segments of a debounce phase, a stream's current
    score reaches it while the hits of its last `frames` scores all EQUAL it -- the calls on which `>` for `>=` would show.  Raw
    scores stand in for the ring here (a guide to the choice only; fault_counts judges the schedule)."""
    score = np.zeros(len(cand), np.int64)
    for i, t in enumerate(cand):
        hit, eq = tab >= t, tab == t
        for c0, c1, frames in segments:
            for c in range(max(c0, 6), c1):
                lo = max(c - frames, 0)
                score[i] += int((hit[c] & eq[lo:c].any(0) & ~(hit[lo:c] & ~eq[lo:c]).any(0)).sum())
    return score


def picker(raw=None, head_raw=None, variant=0):
    """pick() over measured tables: raw [C, S, NL], head_raw [C, S, H].  The threshold is an ELEMENT of the table, taken from the calls
    the threshold will be in force for (never the first five: they reach no comparison): the most frequent value among the elements
    ranked within 0.15 of the quantile q -- streams with periodic audio repeat their scores, and a threshold on such a value meets
    equality call after call -- and the q-quantile element itself where no value repeats.  With `segments` (a debounce phase) and
    n = 0 the element of the band on which equality decides most calls (_decisive) is preferred.  `variant` moves every quantile a
    little (-0.12 .. 0.12), for choose_schedule."""
    def pick(kind, idx, q, n=0, calls=None, segments=None):
        tab = np.asarray(raw if kind == "fixed" else head_raw, F32)[:, :, idx]
        c0, c1 = calls if calls is not None else (0, tab.shape[0])
        vals = np.sort(tab[max(c0, 5):c1].ravel())
        q = min(max(q + 0.04 * ((variant * 7 + idx) % 7 - 3) * (variant > 0), 0.0), 1.0)
        lo, hi = int((len(vals) - 1) * max(q - 0.15, 0.0)), int((len(vals) - 1) * min(q + 0.15, 1.0))
        band = vals[lo:hi + 1]
        band = band[(band > 0) & (band < 1)] if ((band > 0) & (band < 1)).any() else band
        u, n_of = np.unique(band, return_counts=True)
        if segments is not None and n == 0:
            wide = np.unique(vals[int((len(vals) - 1) * 0.45):int((len(vals) - 1) * 0.97) + 1])
            wide = wide[(wide > 0) & (wide < 1)]
            wide = wide[::len(wide) // 200 + 1]
            if len(wide):
                score = _decisive(tab, segments, wide)
                if score.max() > 0:
                    return F32(wide[np.argmax(score)])
        v = u[np.argmax(n_of)] if n_of.max() > 1 else vals[int(round(q * (len(vals) - 1)))]
        return ulp(v, n)
    return pick


def choose_schedule(build, raw=None, head_raw=None, tries=8):
    """Thresholds and VAD scores are test inputs: build(pick, vad_seed) -> Schedule is tried with the quantiles of up to `tries` picker
    variants, each with its own draw of the VAD script, until every applicable fault moves a final score on these raw tables (which come
    from the rule-free twin, never from the handle under test).  Returns (schedule, reference result, {fault: scores moved}) of the
    first such variant, else of variant 0."""
    first = None
    for v in range(tries):
        sched = build(picker(raw, head_raw, v), 5 + v)
        want = reference_rules(sched, raw, head_raw)
        counts = fault_counts(sched, raw, head_raw, want)
        if first is None:
            first = (sched, want, counts)
        if all(n > 0 for n in counts.values()):
            return sched, want, counts
    return first


# ---------------------------------------------------------------------------------------------------------------------------
# the literal form
# ---------------------------------------------------------------------------------------------------------------------------
def predict_pair(buffer, vad_buffer, prediction, patience, threshold, n_frames, vad_threshold):
    """model.py:330-381 for one label of one predict(): `buffer` is the label's prediction_buffer (deque(maxlen=30)), `vad_buffer`
    the stream's VAD scores (the current frame's already appended, model.py:370).  Returns the label's final score."""
    prediction = F32(prediction)
    threshold = F32(threshold)
    if len(buffer) < 5:                                                         # 331-333
        prediction = F32(0.0)
    if prediction != 0.0:                                                       # 348
        if patience > 0:                                                        # 349-352
            scores = np.array(buffer, dtype=F32)[-patience:]
            if (scores >= threshold).sum() < patience:
                prediction = F32(0.0)
        elif n_frames > 0 and not np.isnan(threshold):                          # 353-359 ("parent_model in threshold.keys()")
            recent = np.array(buffer, dtype=F32)[-n_frames:]
            if prediction >= threshold and (recent >= threshold).sum() > 0:
                prediction = F32(0.0)
    buffer.append(prediction)                                                   # 362-363
    if vad_threshold > 0:                                                       # 366-381
        frames = list(vad_buffer)[-7:-4]
        vad_max = np.max(frames) if len(frames) > 0 else 0
        if vad_max < F32(vad_threshold):
            prediction = F32(0.0)
    return prediction


def reference_rules(sched, raw=None, head_raw=None):
    """Final scores of every call of `sched`: {"scores" [C, S, NL], "bank" [C, S, K], "bank_count" [C, S, K] (the slot's ring length
    before the call; -1 = empty slot or sat out)}.  raw [C, S, NL] holds the raw score of every fixed label, head_raw [C, S, H] the raw
    score of every bank head on every stream (a slot reads its subscribed head's)."""
    S, NL, K = sched.S, sched.NL, sched.K
    C = sched.n_calls
    out = np.zeros((C, S, NL), F32)
    bank = np.zeros((C, S, K), F32)
    bank_count = np.full((C, S, K), -1, np.int64)
    buf = [[deque(maxlen=DEPTH) for _ in range(NL)] for _ in range(S)]
    bbuf = [[deque(maxlen=DEPTH) for _ in range(K)] for _ in range(S)]
    sub = np.full((S, K), -1, np.int64)
    vad = [[] for _ in range(S)]
    pat, thr, frames, gate = [0] * NL, np.full(NL, np.nan, F32), 0, F32(0.0)
    bpat, bthr = {}, {}
    row, brow = np.zeros((S, NL), F32), np.zeros((S, K), F32)
    c = 0
    for op in sched.ops:
        if op[0] == "post":
            pat, thr, frames = list(op[1]), np.asarray(op[2], F32), int(op[3])
        elif op[0] == "bank_post":
            bpat[op[1]], bthr[op[1]] = int(op[2]), F32(op[3])
        elif op[0] == "gate":
            gate = F32(op[1])
        elif op[0] == "vad":
            for s in range(S):
                vad[s].append(F32(op[1][s]))
        elif op[0] == "reset":
            for s in op[1]:
                buf[s] = [deque(maxlen=DEPTH) for _ in range(NL)]
                bbuf[s] = [deque(maxlen=DEPTH) for _ in range(K)]
                brow[s] = 0.0
        elif op[0] == "reset_vad":
            for s in op[1]:
                vad[s] = []
        elif op[0] == "sub":
            for s, ids in zip(op[1], op[2]):
                for k in range(K):
                    if sub[s, k] != ids[k]:
                        sub[s, k] = ids[k]
                        bbuf[s][k] = deque(maxlen=DEPTH)
                        brow[s, k] = 0.0
        elif op[0] == "call":
            on = op[2]
            for s in range(S):
                if on is not None and not on[s]:
                    continue
                for l in range(NL):
                    row[s, l] = predict_pair(buf[s][l], vad[s], raw[c, s, l], pat[l], thr[l], frames, gate)
                for k in range(K):
                    h = sub[s, k]
                    if h < 0:
                        brow[s, k] = 0.0
                        continue
                    bank_count[c, s, k] = len(bbuf[s][k])
                    brow[s, k] = predict_pair(bbuf[s][k], vad[s], head_raw[c, s, h], bpat.get(h, 0), bthr.get(h, F32(np.nan)), frames, gate)
            out[c], bank[c] = row, brow
            c += 1
    return {"scores": out, "bank": bank, "bank_count": bank_count}


# ---------------------------------------------------------------------------------------------------------------------------
# the device form, with faults
# ---------------------------------------------------------------------------------------------------------------------------
def _rules(raw, cnt, ring, pat, thr, frames, live, gated, fault):
    """One launch of the rule block on [S, M] pairs: cnt / pat / thr [S, M], ring [S, M, D], live [S, M] (the pair runs), gated [S]
    (the stream's VAD gate is closed).  Appends to the ring in place; returns the final scores (only `live` entries mean anything)."""
    D = ring.shape[2]
    have = np.minimum(cnt, D)
    first = 4 if fault == "first5_lt4" else 6 if fault == "first5_le5" else 5
    sc = np.where(cnt < first, F32(0.0), raw).astype(F32)
    is_pat = pat > 0
    thr_d = np.where(np.isnan(thr), F32(0.0), thr) if fault == "nan_threshold_debounced" else thr
    is_deb = ~is_pat & (frames > 0) & ~np.isnan(thr_d)
    n = np.where(is_pat, pat, frames) + (-1 if fault == "window_short" else 1 if fault == "window_long" else 0)
    look = np.minimum(np.maximum(n, 0), have)
    t = np.where(is_pat, thr, thr_d)
    strict = (is_pat & (fault == "gt_history_patience")) | (~is_pat & (fault == "gt_history_debounce"))
    slip = 1 if fault == "ring_slot_slip" else 0
    n_hit = np.zeros(cnt.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(1, int(look.max(initial=0)) + 1):
            v = np.take_along_axis(ring, ((cnt - i - slip) % D)[..., None], 2)[..., 0]
            n_hit += (i <= look) & np.where(strict, v > t, v >= t)
        cur = sc > t if fault == "gt_current_debounce" else sc >= t
    zero = (sc != 0.0) & ((is_pat & (n_hit < pat)) | (is_deb & cur & (n_hit > 0)))
    sc = np.where(zero, F32(0.0), sc).astype(F32)
    fin = np.where(gated[:, None], F32(0.0), sc).astype(F32)
    kept = fin if fault == "gate_before_append" else sc
    idx = (cnt % D)[..., None]
    np.put_along_axis(ring, idx, np.where(live, kept, np.take_along_axis(ring, idx, 2)[..., 0])[..., None], 2)
    return fin


def _gate_closed(vring, nv, gate, fault):
    """[S] bool: the largest of entries L-7 .. L-5 of the L scores pushed so far (none while L < 5: 0) is below the threshold."""
    S = nv.shape[0]
    if not gate > 0:
        return np.zeros(S, bool)
    back = (6, 5, 4) if fault == "vad_window_late" else (8, 7, 6) if fault == "vad_window_early" else (7, 6, 5)
    vmax = np.full(S, -np.inf, F32)
    any_entry = np.zeros(S, bool)
    for j in back:
        ok = nv >= j
        vmax = np.where(ok, np.maximum(vmax, vring[np.arange(S), (nv - j) & 7]), vmax)
        any_entry |= ok
    if fault == "vad_warmup_4":
        early = nv == 4
        vmax = np.where(early, vring[:, 0], vmax)
        any_entry |= early
    vmax = np.where(any_entry, vmax, F32(0.0))
    return vmax <= gate if fault == "vad_le" else vmax < gate


def device_rules(sched, raw=None, head_raw=None, fault=None):
    """reference_rules in the device's form (same arguments, {"scores", "bank"}), with one named fault of FAULTS or none."""
    assert fault is None or fault in FAULTS, fault
    S, NL, K, H = sched.S, sched.NL, sched.K, sched.H
    C = sched.n_calls
    D = 29 if fault == "ring_depth_29" else DEPTH
    out, bank = np.zeros((C, S, NL), F32), np.zeros((C, S, K), F32)
    cnt = np.zeros(S, np.int64)                       # (uint32 on the device; a run is far from its wrap)
    ring = np.zeros((S, NL, D), F32)
    bcnt = np.zeros((S, K), np.int64)
    bring = np.zeros((S, K, D), F32)
    sub = np.full((S, K), -1, np.int64)
    vring, nv = np.zeros((S, 8), F32), np.zeros(S, np.int64)
    pat, thr, frames, gate = np.zeros(NL, np.int64), np.full(NL, np.nan, F32), 0, F32(0.0)
    bpat, bthr = np.zeros(max(H, 1), np.int64), np.full(max(H, 1), np.nan, F32)
    row, brow = np.zeros((S, NL), F32), np.zeros((S, K), F32)
    c = 0
    for op in sched.ops:
        if op[0] == "post":
            pat, thr, frames = np.asarray(op[1], np.int64), np.asarray(op[2], F32), int(op[3])
        elif op[0] == "bank_post":
            bpat[op[1]], bthr[op[1]] = int(op[2]), F32(op[3])
        elif op[0] == "gate":
            gate = F32(op[1])
        elif op[0] == "vad":
            vring[np.arange(S), nv & 7] = op[1]
            nv += 1
        elif op[0] == "reset":
            ids = np.asarray(op[1], np.int64)
            cnt[ids], ring[ids] = 0, 0.0
            bcnt[ids], bring[ids], brow[ids] = 0, 0.0, 0.0
        elif op[0] == "reset_vad":
            ids = np.asarray(op[1], np.int64)
            vring[ids], nv[ids] = 0.0, 0
        elif op[0] == "sub":
            ids = np.asarray(op[1], np.int64)
            changed = sub[ids] != op[2]
            sub[ids] = op[2]
            rows, cols = ids[np.nonzero(changed)[0]], np.nonzero(changed)[1]
            brow[rows, cols] = 0.0
            if fault != "slot_keeps_count_on_resubscribe":
                bcnt[rows, cols], bring[rows, cols] = 0, 0.0
        elif op[0] == "call":
            k = op[1]
            on = np.ones(S, bool) if op[2] is None else np.asarray(op[2], bool)
            gated = _gate_closed(vring, nv, gate, fault)
            step = k if fault == "count_per_chunk" else 1
            if K:                                     # (the bank's launch reads the stream's count before the fixed heads advance it)
                live = on[:, None] & (sub >= 0)
                hd = np.maximum(sub, 0)
                r = np.take_along_axis(head_raw[c], hd, 1) if H else np.zeros((S, K), F32)
                use = np.broadcast_to(cnt[:, None], (S, K)).copy() if fault == "slot_uses_stream_count" else bcnt
                fin = _rules(r, use, bring, bpat[hd], bthr[hd], frames, live, gated, fault)
                brow = np.where(live, fin, np.where(on[:, None], F32(0.0), brow)).astype(F32)
                bcnt += np.where(live, step, 0)
            if NL:
                live = np.broadcast_to(on[:, None], (S, NL))
                fin = _rules(raw[c], np.broadcast_to(cnt[:, None], (S, NL)), ring, np.broadcast_to(pat, (S, NL)),
                             np.broadcast_to(thr, (S, NL)), frames, live, gated, fault)
                row = np.where(live, fin, row).astype(F32)
            cnt += np.where(on, step, 0)
            if fault == "masked_stream_counts":
                cnt += ~on
                bcnt += (~on)[:, None] & (sub >= 0)
            out[c], bank[c] = row, brow
            c += 1
    return {"scores": out, "bank": bank}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def moved(want, got):
    """Final scores a (faulty) form moves: count of differing float32 bit patterns over fixed and bank scores."""
    return int((bits(want["scores"]) != bits(got["scores"])).sum() + (bits(want["bank"]) != bits(got["bank"])).sum())


def fault_counts(sched, raw=None, head_raw=None, want=None):
    """{fault: final scores it moves} for every fault that applies to the schedule."""
    if want is None:
        want = reference_rules(sched, raw, head_raw)
    return {f: moved(want, device_rules(sched, raw, head_raw, fault=f)) for f in sched.applicable()}
