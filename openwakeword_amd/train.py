"""Training bank heads on the device: the step of the reference's train.Model.train_model (train.py:434-510) for the network a bank
head is (train.py:66-83 with n_blocks = 1, n_classes = 1), many heads per call (include/owwhip.h: oww_train_*).
Model.auto_train (train.py:261-366) sits on top of it here: its validation pass (train.py:512-553), its checkpoints and its merge
(average_models, train.py:198-223) run on the device in the step's arithmetic (oww_train_eval, oww_train_snapshot,
oww_train_average), and what stays on the host is policy: when to validate, which checkpoint to keep, which to
merge.  Batches are index tables into one shared window pool, drawn here with a seeded generator, so a run can be replayed against
the reference on the same batches."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

EMB_DIM = 96
FIELDS = ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3")      # the flat record's order (include/owwhip.h)


def record_shapes(T: int, hidden: int) -> List[Tuple[str, Tuple[int, ...]]]:
    F, D = int(T) * EMB_DIM, int(hidden)
    return [("w1", (F, D)), ("b1", (D,)), ("g1", (D,)), ("be1", (D,)), ("w2", (D, D)), ("b2", (D,)), ("g2", (D,)), ("be2", (D,)),
            ("w3", (D, 1)), ("b3", (1,))]


def param_count(T: int, hidden: int) -> int:
    return sum(int(np.prod(s)) for _, s in record_shapes(T, hidden))


def head_to_record(head: dict) -> np.ndarray:
    """A bank head dict (weights.synthetic_head / onnx_ingest.load_head layout, LayerNorm after both layers) -> its flat record."""
    net = head["net"]
    if net.get("ln1") is None or net.get("ln2") is None or net.get("more"):
        raise ValueError("a trainable head has one hidden block and LayerNorm after both linear layers (train.py:66-83)")
    parts = [net["w1"], net["b1"], net["ln1"][0], net["ln1"][1], net["w2"], net["b2"], net["ln2"][0], net["ln2"][1], net["w3"], net["b3"]]
    rec = np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in parts])
    if rec.size != param_count(head["T"], head["hidden"]):
        raise ValueError(f"head fields do not match T = {head['T']}, hidden = {head['hidden']}")
    return rec


def record_to_head(rec: np.ndarray, T: int, hidden: int) -> dict:
    """A flat record -> the head dict bank_add takes unchanged."""
    rec = np.asarray(rec, dtype=np.float32)
    f, o = {}, 0
    for name, shape in record_shapes(T, hidden):
        n = int(np.prod(shape))
        f[name] = rec[o:o + n].reshape(shape).copy()
        o += n
    return {"kind": "binary", "T": int(T), "hidden": int(hidden), "n_out": 1,
            "net": {"w1": f["w1"], "b1": f["b1"], "ln1": (f["g1"], f["be1"]), "w2": f["w2"], "b2": f["b2"], "ln2": (f["g2"], f["be2"]),
                    "w3": f["w3"], "b3": f["b3"]}}


def lr_warmup_cosine_decay(global_step, warmup_steps=0, hold=0, total_steps=0, start_lr=0.0, target_lr=1e-3):
    """train.py:167-190, restated."""
    learning_rate = 0.5 * target_lr * (1 + np.cos(np.pi * (global_step - warmup_steps - hold) / float(total_steps - warmup_steps - hold)))
    warmup_lr = target_lr * (global_step / warmup_steps)
    if hold > 0:
        learning_rate = np.where(global_step > warmup_steps + hold, learning_rate, target_lr)
    learning_rate = np.where(global_step < warmup_steps, warmup_lr, learning_rate)
    return learning_rate


def negative_weight_schedule(steps: int, max_negative_weight: float = 1000) -> List[float]:
    """train.py:274 / 295 / 315: the negative class weight of step k."""
    return np.linspace(1, max_negative_weight, int(steps)).tolist()


def init_head(T: int, hidden: int, seed: int) -> dict:
    """A fresh head with nn.Linear's and nn.LayerNorm's default distributions: weights and biases U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)),
    gamma = 1, beta = 0.  (The same distributions, not torch's generator: a seed here does not reproduce a torch seed.)"""
    r = np.random.default_rng([int(seed), int(T), int(hidden)])
    F, D = int(T) * EMB_DIM, int(hidden)

    def lin(i, o):
        b = 1.0 / np.sqrt(i)
        return r.uniform(-b, b, size=(i, o)).astype(np.float32), r.uniform(-b, b, size=o).astype(np.float32)

    w1, b1 = lin(F, D)
    w2, b2 = lin(D, D)
    w3, b3 = lin(D, 1)
    one, zero = np.ones(D, np.float32), np.zeros(D, np.float32)
    return {"kind": "binary", "T": int(T), "hidden": D, "n_out": 1,
            "net": {"w1": w1, "b1": b1, "ln1": (one.copy(), zero.copy()), "w2": w2, "b2": b2, "ln2": (one.copy(), zero.copy()), "w3": w3, "b3": b3}}


COUNT_FIELDS = ("n_pos", "n_neg", "pos_gt", "neg_gt", "neg_ge")      # oww_train_counts (include/owwhip.h)


def metrics_from_counts(counts: np.ndarray) -> Dict[str, np.ndarray]:
    """counts [U, 5] -> the five count arrays plus what the reference reports from them, in its number formats: "n_fp" (self.fp,
    train.py:100: y - p <= -0.5, i.e. y = 0 and p >= 0.5) = neg_ge, int64; "recall" (binary Recall: pos_gt / n_pos, 0 without
    positives) and "accuracy" (binary Accuracy: (pos_gt + n_neg - neg_gt) / (n_pos + n_neg)), fp32 quotients of the integers as
    torch divides them."""
    c = np.asarray(counts, dtype=np.int64)
    out = {f: c[:, i].astype(np.int32) for i, f in enumerate(COUNT_FIELDS)}
    out["n_fp"] = c[:, 4].copy()
    out["recall"] = np.where(c[:, 0] > 0, c[:, 2].astype(np.float32) / np.maximum(c[:, 0], 1).astype(np.float32), np.float32(0)).astype(np.float32)
    tot = c[:, 0] + c[:, 1]
    out["accuracy"] = np.where(tot > 0, (c[:, 2] + c[:, 1] - c[:, 3]).astype(np.float32) / np.maximum(tot, 1).astype(np.float32),
                               np.float32(0)).astype(np.float32)
    return out


class HeadTrainer:
    """One training session on a BatchedModel's handle (BatchedModel.head_trainer): n_problems heads of one shape side by side."""

    def __init__(self, engine, T: int, hidden: int, n_problems: int, init: Optional[Sequence[dict]] = None, seed: int = 0):
        self.engine, self.T, self.hidden, self.n_problems = engine, int(T), int(hidden), int(n_problems)
        if self.n_problems < 1:
            raise ValueError("n_problems must be at least 1")
        if not 16 <= self.hidden <= 128 or self.hidden % 16:
            raise ValueError(f"hidden must be a multiple of 16 in 16 .. 128 (got {hidden})")
        if not 1 <= self.T <= engine.feature_ring:
            raise ValueError(f"T = {T} outside 1 .. {engine.feature_ring} (the handle's feature ring)")
        heads = [init_head(T, hidden, seed + u) for u in range(self.n_problems)] if init is None else list(init)
        if len(heads) != self.n_problems:
            raise ValueError(f"{len(heads)} initial heads for {self.n_problems} problems")
        for hd in heads:
            if int(hd["T"]) != self.T or int(hd["hidden"]) != self.hidden:
                raise ValueError(f"initial head has T = {hd['T']}, hidden = {hd['hidden']}; the session trains T = {T}, hidden = {hidden}")
        self.n_params = param_count(T, hidden)
        engine.train_begin(np.stack([head_to_record(hd) for hd in heads]), self.T, self.hidden)
        self._open = True
        self.history: Dict[str, np.ndarray] = {"loss": np.empty((self.n_problems, 0), np.float32), "kept": np.empty((self.n_problems, 0), np.int32)}

    def set_pool(self, pool, n_windows: Optional[int] = None, on_device: bool = False) -> None:
        """The shared window pool [P, T, 96] fp32 (host array, or a device address with on_device and n_windows)."""
        if not on_device:
            pool = np.asarray(pool)
            if pool.ndim != 3 or pool.shape[1:] != (self.T, EMB_DIM):
                raise ValueError(f"pool must be [P, {self.T}, 96], got {pool.shape}")
        self.engine.train_set_pool(pool, n_windows, on_device)

    def steps(self, idx, y, lr, neg_weight, on_device: bool = False, shape=None) -> Tuple[np.ndarray, np.ndarray]:
        """K steps: idx / y [n_problems, K, n] or [K, n] (shared), idx = pool rows or -1, y in {0, 1}; lr, neg_weight [K] (a scalar is
        repeated) -> (loss [n_problems, K], NaN where no optimizer step was taken; kept [n_problems, K]); both are appended to history."""
        K = int((shape if on_device else np.shape(idx))[-2])
        lr = np.broadcast_to(np.asarray(lr, dtype=np.float64), (K,))
        nw = np.broadcast_to(np.asarray(neg_weight, dtype=np.float32), (K,))
        loss, m = self.engine.train_steps(self.n_problems, idx, y, lr, nw, on_device, shape)
        self.history["loss"] = np.concatenate([self.history["loss"], loss], axis=1)
        self.history["kept"] = np.concatenate([self.history["kept"], m], axis=1)
        return loss, m

    def records(self) -> np.ndarray:
        return np.stack([self.engine.train_get(u, self.n_params) for u in range(self.n_problems)])

    # ---- what auto_train needs around the step (include/owwhip.h: oww_train_new_sequence .. oww_train_get_slot) ----
    def new_sequence(self) -> None:
        """A new train_model call on the same optimizer: the accumulation counters restart (train.py:443-444); Adam's moments and
        step count, which live in the reference's self.optimizer (train.py:135), stay."""
        self.engine.train_new_sequence()

    def set_eval_pool(self, pool, n_windows: Optional[int] = None, on_device: bool = False) -> None:
        """The validation window pool [P, T, 96] fp32, independent of the training pool."""
        if not on_device:
            pool = np.asarray(pool)
            if pool.ndim != 3 or pool.shape[1:] != (self.T, EMB_DIM):
                raise ValueError(f"eval pool must be [P, {self.T}, 96], got {pool.shape}")
        self.engine.train_set_eval_pool(pool, n_windows, on_device)

    def evaluate(self, idx, y, source: int = -1, scores: bool = False, on_device: bool = False, shape=None) -> Dict[str, np.ndarray]:
        """The forward pass of every problem over the eval-pool rows idx [n_problems, n] or [n] (shared; -1 = empty slot) with labels
        y, on the live parameters (source = -1) or on checkpoint slot `source` -> the five counts n_pos, n_neg, pos_gt, neg_gt,
        neg_ge [n_problems] and what the reference reports from them (metrics_from_counts); "scores" [n_problems, n] if asked."""
        counts, sc = self.engine.train_eval(idx, y, source, scores, on_device, shape)
        out = metrics_from_counts(counts)
        if scores:
            out["scores"] = sc
        return out

    def reserve_checkpoints(self, n_slots: int) -> None:
        self.engine.train_checkpoints(n_slots)

    def snapshot(self, slots) -> None:
        """Problem u's live parameters -> its checkpoint slot slots[u] (-1: none), behind the steps submitted so far."""
        self.engine.train_snapshot(slots)

    def average(self, sel, dst: int) -> None:
        """average_models (train.py:198-223) per problem over the slots sel [n_problems, C] marks, into slot dst; a problem with none
        marked gets its live parameters there (train.py:340-343)."""
        self.engine.train_average(sel, dst)

    def checkpoint_records(self, slot: int) -> np.ndarray:
        return np.stack([self.engine.train_get_slot(u, slot, self.n_params) for u in range(self.n_problems)])

    def checkpoint_heads(self, slot: int) -> List[dict]:
        """Checkpoint slot `slot` of every problem, as dicts bank_add takes unchanged."""
        return [record_to_head(self.engine.train_get_slot(u, slot, self.n_params), self.T, self.hidden) for u in range(self.n_problems)]

    def heads(self) -> List[dict]:
        """The current heads, as dicts bank_add takes unchanged."""
        return [record_to_head(self.engine.train_get(u, self.n_params), self.T, self.hidden) for u in range(self.n_problems)]

    def close(self) -> None:
        if self._open:
            self._open = False
            self.engine.train_end()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


TABLE_CHUNK = 4096       # steps of one drawn chunk = OWW_TRAIN_MAX_STEPS: the unit the tables are defined in


def iter_tables(problems: Sequence[Tuple[np.ndarray, np.ndarray]], steps: int, n_batch: int, seed: int, pos_fraction: float = 0.5):
    """Index and label tables for `problems`, one (positive pool rows, negative pool rows) pair per head, TABLE_CHUNK steps at a time:
    yields (first step, idx [U, k, n_batch] int32, y [U, k, n_batch] uint8).  Every batch holds round(pos_fraction n_batch) positives
    and the rest negatives, drawn with replacement by one generator per problem ([seed, u]) that carries on from chunk to chunk, so a
    run needs one chunk of host memory, not the whole table, and is reproducible from the seed."""
    U = len(problems)
    n_pos = int(round(pos_fraction * n_batch))
    rows = []
    for u, (pos, neg) in enumerate(problems):
        pos, neg = np.asarray(pos, np.int32), np.asarray(neg, np.int32)
        if pos.size == 0 or neg.size == 0:
            raise ValueError(f"problem {u} needs pool rows of both classes")
        rows.append((pos, neg, np.random.default_rng([int(seed), u])))
    for a in range(0, int(steps), TABLE_CHUNK):
        k = min(int(steps), a + TABLE_CHUNK) - a
        idx = np.empty((U, k, n_batch), np.int32)
        y = np.zeros((U, k, n_batch), np.uint8)
        y[:, :, :n_pos] = 1
        for u, (pos, neg, r) in enumerate(rows):
            idx[u, :, :n_pos] = pos[r.integers(0, pos.size, (k, n_pos))]
            idx[u, :, n_pos:] = neg[r.integers(0, neg.size, (k, n_batch - n_pos))]
        yield a, idx, y


def draw_tables(problems: Sequence[Tuple[np.ndarray, np.ndarray]], steps: int, n_batch: int, seed: int, pos_fraction: float = 0.5):
    """iter_tables' chunks in one piece: (idx, y), each [U, steps, n_batch] -- the tables train_heads runs, for replaying a run."""
    chunks = list(iter_tables(problems, steps, n_batch, seed, pos_fraction))
    return np.concatenate([c[1] for c in chunks], axis=1), np.concatenate([c[2] for c in chunks], axis=1)


def train_heads(bm, pool: np.ndarray, problems: Sequence[Tuple[np.ndarray, np.ndarray]], steps: int, hidden: int = 32, n_batch: int = 128,
                lr: float = 1e-4, warmup_steps: Optional[int] = None, hold_steps: Optional[int] = None, max_negative_weight: float = 1000,
                seed: int = 0, init: Optional[Sequence[dict]] = None) -> Tuple[List[dict], Dict[str, np.ndarray]]:
    """One training sequence (train.py:434-510 under auto_train's first schedule, train.py:270-282: warm-up steps / 5, hold steps / 3,
    negative weight 1 -> max_negative_weight) for len(problems) heads at once on `bm`'s device: `pool` [P, T, 96] feature windows,
    problems[u] = (positive pool rows, negative pool rows) -> (heads for bank_add, history).  The tables are drawn by iter_tables
    a chunk of at most 4096 steps at a time and each chunk is one call (draw_tables gives the same tables in one piece)."""
    pool = np.asarray(pool, dtype=np.float32)
    T = pool.shape[1]
    warmup = steps // 5 if warmup_steps is None else int(warmup_steps)
    hold = steps // 3 if hold_steps is None else int(hold_steps)
    k = np.arange(steps)
    lrs = np.asarray(lr_warmup_cosine_decay(k, warmup_steps=warmup, hold=hold, total_steps=steps, target_lr=lr), dtype=np.float64) if warmup > 0 \
        else np.full(steps, lr, np.float64)
    nws = np.asarray(negative_weight_schedule(steps, max_negative_weight), dtype=np.float32)
    with bm.head_trainer(T, hidden, len(problems), init=init, seed=seed) as tr:
        tr.set_pool(pool)
        for a, idx, y in iter_tables(problems, steps, n_batch, seed):      # one call per drawn chunk of at most 4096 steps
            b = a + idx.shape[1]
            tr.steps(idx, y, lrs[a:b], nws[a:b])
        return tr.heads(), tr.history


# ------------------------------------------------------------------------------------------------------------------ auto_train
BEST_VAL_FP = 1000       # train.py: self.best_val_fp is initialised to this and never written (see auto_train's docstring)


def auto_train_plan(steps: int, max_negative_weight: float = 1000, target_fp_per_hour: float = 0.2) -> List[dict]:
    """The three sequences of train.py:261-324 as data: per sequence dict(n_steps, lr [n_steps] float64, neg_weight [n_steps] fp32,
    val_steps: the sorted step indices after which a validation runs, max_negative_weight).  See auto_train for the quirks kept."""
    if int(steps) != steps or steps < 50 or int(steps) % 10:
        raise ValueError("auto_train: steps must be a multiple of 10, at least 50 (train.py:288 runs sequences 2 and 3 for steps / 10 "
                         "steps as a float: any other value walks off the end of its weight list, and under 50 the warm-up is 0 steps long)")
    out = []
    lr, w, n = 0.0001, max_negative_weight, int(steps)
    for seq in range(3):
        if seq == 0:
            val = np.linspace(n - int(n * 0.25), n, 20).astype(np.int64)
            total = n                                          # an int
        else:
            lr = lr / 10
            if seq == 1:
                n = n / 10                                     # train.py:288: a float from here on
            if BEST_VAL_FP > target_fp_per_hour:               # train.py:291 / 311
                w = w * 2
            val = np.linspace(1, n, 20).astype(np.int16)       # train.py:296: int16, wraps above 32,767
            total = n
        ni = int(n)
        k = np.arange(ni)
        lrs = np.asarray(lr_warmup_cosine_decay(k, warmup_steps=total // 5, hold=total // 3, total_steps=total, target_lr=lr), dtype=np.float64)
        nws = np.asarray(np.linspace(1, w, ni).tolist(), dtype=np.float32)
        vs = sorted({int(v) for v in val if 1 < int(v) <= ni - 1})      # train.py:513: step_ndx in val_steps and step_ndx > 1
        out.append(dict(n_steps=ni, lr=lrs, neg_weight=nws, val_steps=vs, max_negative_weight=w))
    return out


def keep_checkpoint(val_n_fp: list, val_recall: list) -> bool:
    """train.py:557-559, the current value already in both histories."""
    return bool(val_n_fp[-1] <= np.percentile(val_n_fp, 50) and val_recall[-1] >= np.percentile(val_recall, 5))


def select_checkpoints(hist: dict, scores: List[dict]) -> List[int]:
    """train.py:326-338: the checkpoints (positions in `scores`) at or above the 90th percentile of accuracy and recall and at or
    below the 10th of false positives per hour, the percentiles taken over the whole histories."""
    if not hist["val_accuracy"]:
        return []
    a, r, f = np.percentile(hist["val_accuracy"], 90), np.percentile(hist["val_recall"], 90), np.percentile(hist["val_fp_per_hr"], 10)
    return [i for i, s in enumerate(scores) if s["val_accuracy"] >= a and s["val_recall"] >= r and s["val_fp_per_hr"] <= f]


class _TableFeed:
    """iter_tables' chunks handed out a few steps at a time, across chunk boundaries"""

    def __init__(self, it):
        self.it, self.idx, self.y, self.at = it, None, None, 0

    def take(self, k: int):
        while k > 0:
            if self.idx is None or self.at == self.idx.shape[1]:
                _, self.idx, self.y = next(self.it)
                self.at = 0
            b = min(self.idx.shape[1], self.at + k)
            yield self.idx[:, self.at:b], self.y[:, self.at:b]
            k -= b - self.at
            self.at = b


def _eval_table(t, U: int, what: str):
    """(idx, y) or idx alone (labels 0) -> int32 / uint8 arrays [n] or [U, n]"""
    if isinstance(t, tuple):
        idx, y = np.asarray(t[0], np.int32), np.asarray(t[1], np.uint8)
    else:
        idx = np.asarray(t, np.int32)
        y = np.zeros(idx.shape, np.uint8)
    if idx.shape != y.shape or idx.ndim not in (1, 2) or (idx.ndim == 2 and idx.shape[0] != U) or idx.shape[-1] < 1:
        raise ValueError(f"auto_train: {what} must be index and label tables [n] or [{U}, n], got {idx.shape} and {y.shape}")
    return idx, y


def auto_train(bm, pool: np.ndarray, problems: Sequence[Tuple[np.ndarray, np.ndarray]], val_pool: np.ndarray, val, fp_val, steps: int = 50000,
               max_negative_weight: float = 1000, target_fp_per_hour: float = 0.2, val_set_hrs: float = 11.3, hidden: int = 32,
               n_batch: int = 128, seed: int = 0, init: Optional[Sequence[dict]] = None) -> Tuple[List[dict], dict]:
    """Model.auto_train (train.py:261-366) for len(problems) heads side by side on `bm`'s device -> (heads for bank_add, report).
    `pool` [P, T, 96] and problems[u] = (positive rows, negative rows) are train_heads'; `val_pool` [Pv, T, 96] holds the validation
    windows; `val` = (idx, y) tables into it, [n] shared or [U, n] (-1 pads), the reference's X_val as ONE batch (the reference keeps
    the last batch's metrics only); `fp_val` the false-positive table (idx, or (idx, y) with y all 0), any length up to 2^20.
    Steps, validation, checkpoints and merge run on the device; decisions are taken here, per problem, each with its own histories,
    checkpoint list and selection.  The tables of all three sequences come from ONE iter_tables generator.

    What the reference does, reproduced as it is:
      * sequence 1: `steps` steps at lr 1e-4, validated after the steps np.linspace(steps - int(0.25 steps), steps, 20).astype(int64);
        the last value, `steps`, is never reached.
      * sequences 2 and 3: steps / 10 steps (a float in the reference) at lr / 10 and lr / 100, validated after the steps
        np.linspace(1, steps / 10, 20).astype(np.int16) (int16: wraps above 32,767 steps) that are > 1 (train.py:513).
      * every sequence: warm-up n // 5, hold n // 3 of its own length n, negative weight np.linspace(1, w, int(n)); a new sequence
        restarts the accumulation counters and keeps Adam's moments and step count (HeadTrainer.new_sequence).
      * a validation runs after the step of its index; a checkpoint is kept when val_n_fp[-1] <= percentile(val_n_fp, 50) and
        val_recall[-1] >= percentile(val_recall, 5), the current values already in the histories, which run on across sequences.
      * best_val_fp is initialised to 1000 and never written, so max_negative_weight doubles before sequence 2 and again before
        sequence 3 whenever target_fp_per_hour < 1000: sequence 3 ramps to 4 x the argument.
      * merge: checkpoints with val_accuracy >= p90, val_recall >= p90 and val_fp_per_hr <= p10 of the histories are averaged
        (average_models: 0 x the first, += in order, one division); with none, the live model is returned.
    report["problems"][u]: the histories (val_recall, val_accuracy, val_n_fp, val_fp_per_hr), counts / fp_counts per validation,
    checkpoint_steps ((sequence, step) pairs), selected (positions in the checkpoint list), combined (the returned model's three
    metrics), live_record (the model as training left it: what is returned, bit for bit, where nothing is selected), loss, kept.
    Not here: _select_best_model (auto_train does not call it), positive_test_clips recall, multiclass and recurrent heads."""
    pool = np.asarray(pool, dtype=np.float32)
    T, U = pool.shape[1], len(problems)
    plan = auto_train_plan(steps, max_negative_weight, target_fp_per_hour)
    v_idx, v_y = _eval_table(val, U, "val")
    f_idx, f_y = _eval_table(fp_val, U, "fp_val")
    if f_y.any():
        raise ValueError("auto_train: the false-positive table's labels are all 0")
    n_val = sum(len(s["val_steps"]) for s in plan)
    hrs = np.float32(val_set_hrs)
    hist = [dict(val_recall=[], val_accuracy=[], val_n_fp=[], val_fp_per_hr=[]) for _ in range(U)]
    counts: List[list] = [[] for _ in range(U)]          # per validation: the five counts of `val`, and fp_val's neg_ge
    fp_counts: List[list] = [[] for _ in range(U)]
    ckpt: List[List[dict]] = [[] for _ in range(U)]
    feed = _TableFeed(iter_tables(problems, sum(s["n_steps"] for s in plan), n_batch, seed))
    with bm.head_trainer(T, hidden, U, init=init, seed=seed) as tr:
        tr.set_pool(pool)
        tr.set_eval_pool(val_pool)
        tr.reserve_checkpoints(max(n_val, 1))
        for si, seq in enumerate(plan):
            if si:
                tr.new_sequence()
            k = 0
            last = seq["n_steps"] - 1
            for v in seq["val_steps"] + ([] if last in seq["val_steps"] else [last]):
                for idx, y in feed.take(v + 1 - k):
                    b = k + idx.shape[1]
                    tr.steps(idx, y, seq["lr"][k:b], seq["neg_weight"][k:b])
                    k = b
                if v not in seq["val_steps"]:
                    continue
                fp, mv = tr.evaluate(f_idx, f_y), tr.evaluate(v_idx, v_y)
                slots = np.full(U, -1, np.int32)
                for u in range(U):
                    h = hist[u]
                    h["val_fp_per_hr"].append(np.float32(fp["n_fp"][u]) / hrs)      # an int64 tensor / a float: fp32 in torch
                    h["val_accuracy"].append(mv["accuracy"][u])
                    h["val_recall"].append(mv["recall"][u])
                    h["val_n_fp"].append(np.int64(mv["n_fp"][u]))
                    counts[u].append([int(mv[f][u]) for f in COUNT_FIELDS])
                    fp_counts[u].append(int(fp["neg_ge"][u]))
                    if keep_checkpoint(h["val_n_fp"], h["val_recall"]):
                        slots[u] = len(ckpt[u])
                        ckpt[u].append(dict(sequence=si, training_step_ndx=v, val_n_fp=h["val_n_fp"][-1], val_recall=h["val_recall"][-1],
                                            val_accuracy=h["val_accuracy"][-1], val_fp_per_hr=h["val_fp_per_hr"][-1]))
                if (slots >= 0).any():
                    tr.snapshot(slots)
        selected = [select_checkpoints(hist[u], ckpt[u]) for u in range(U)]
        sel = np.zeros((U, max(n_val, 1)), np.uint8)
        for u, s in enumerate(selected):
            sel[u, s] = 1
        live = tr.records()                        # the model as training left it: what a problem with nothing selected gets back
        tr.average(sel, 0)
        fp, mv = tr.evaluate(f_idx, f_y, source=0), tr.evaluate(v_idx, v_y, source=0)
        heads = tr.checkpoint_heads(0)
        history = tr.history
    report = []
    for u in range(U):
        h = hist[u]
        report.append(dict({k_: np.asarray(v_) for k_, v_ in h.items()},
                           checkpoint_steps=[(c["sequence"], c["training_step_ndx"]) for c in ckpt[u]], checkpoints=ckpt[u], selected=selected[u],
                           counts=np.asarray(counts[u], np.int32).reshape(-1, 5), fp_counts=np.asarray(fp_counts[u], np.int32),
                           combined=dict(recall=mv["recall"][u], accuracy=mv["accuracy"][u], fp_per_hr=np.float32(fp["n_fp"][u]) / hrs),
                           live_record=live[u], loss=history["loss"][u], kept=history["kept"][u]))
    return heads, {"problems": report, "plan": plan}
