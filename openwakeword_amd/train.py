"""Training bank heads on the device: the step of the reference's train.Model.train_model (train.py:434-510) for the network a bank
head is (train.py:66-83 with n_blocks = 1, n_classes = 1), many heads per call (include/owwhip.h: oww_train_*).
What stays on the host is policy: auto_train's three sequences, checkpoint selection and averaging (train.py:198-366) sit on top
of the step, and validate_bank already gives their false-accepts-per-hour gate.  Batches are index tables into one shared window
pool, drawn here with a seeded generator, so a run can be replayed against the reference on the same batches."""
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
