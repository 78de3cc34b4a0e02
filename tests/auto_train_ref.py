"""The case module of the auto_train tests (no GPU): Model.auto_train (train.py:261-366) restated in numpy on top of the step of
tests/head_train_ref.py, the case tables, and the reference's own class run on the same batches.

  eval_ref(rec, X, y, dtype)                       -- the five counts of oww_train_eval and the scores, on head_train_ref.forward.
  average_ref(records)                             -- average_models (train.py:198-223) in fp32: 0 x the first, += in order, / count.
  Stepper                                          -- head_train_ref.ref_train's step with its state held between calls (ref_train
                                                      opens fresh counters and moments at every call, so a run of three sequences on
                                                      one optimizer cannot be built from it); tests/test_auto_train_cpu.py holds it to
                                                      ref_train bit for bit.
  auto_train_ref(case, dtype, order, defects)      -- the whole policy, float64 (the definition) or fp32 under the four summation orders,
                                                      with switchable defects.
  run_reference_auto_train(case, double)           -- train.Model.auto_train itself (None where the reference checkout is absent).

torchmetrics is not installed where these tests were written.  model.recall / model.accuracy are therefore replaced by two functions
that implement its documented binary rule (predictions already in [0, 1] get no sigmoid and count as positive where > 0.5; Recall =
tp / (tp + fn), 0 without positives; Accuracy = (tp + tn) / all): that rule is taken from the documentation and pinned to nothing.
"""
from __future__ import annotations

import os

import numpy as np

from openwakeword_amd import train as T_

import head_train_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "auto_train.npz")
DEFECTS = ("fp_gt", "acc_not_reset_seq", "moments_reset_seq", "val_before_step", "pct_without_current", "step_gt1_dropped",
           "no_weight_doubling", "avg_divide_first", "fallback_checkpoint")
COUNTS = ("n_pos", "n_neg", "pos_gt", "neg_gt", "neg_ge")
VAL_SET_HRS = 11.3


# ------------------------------------------------------------------------------------------------------------------ eval and average
def hidden_of(n_params, T):
    for D in range(16, 129, 16):
        if T_.param_count(T, D) == n_params:
            return D
    raise ValueError(f"{n_params} parameters fit no hidden size at T = {T}")


def eval_ref(rec, X, y, dtype=np.float64, defects=()):
    """rec: a flat record; X [n, T, 96] the windows of the valid slots; y [n] their labels -> dict(the five counts, p [n] in dtype)."""
    X = np.asarray(X)
    T = X.shape[1]
    D = hidden_of(len(rec), T)
    p = R.forward(R.unpack(rec, T, D, dtype), X.reshape(X.shape[0], -1), dtype)["p"]
    y = np.asarray(y)
    half = dtype(0.5)
    ge = (p > half) if "fp_gt" in defects else (p >= half)
    return dict(n_pos=int((y == 1).sum()), n_neg=int((y == 0).sum()), pos_gt=int(((y == 1) & (p > half)).sum()),
                neg_gt=int(((y == 0) & (p > half)).sum()), neg_ge=int(((y == 0) & ge).sum()), p=p)


def eval_tables(rec, pool, idx, y, dtype=np.float64, defects=()):
    """eval_ref over one problem's table row: idx [n] with -1 = empty -> (counts dict, scores [n] float64 with NaN in empty slots)"""
    idx, y = np.asarray(idx), np.asarray(y)
    valid = idx >= 0
    e = eval_ref(rec, pool[idx[valid]], y[valid], dtype, defects)
    sc = np.full(idx.shape, np.nan)
    sc[valid] = e["p"]
    return e, sc


def metrics(e):
    """what the reference reports from the counts, in its number formats (fp32 quotients of integers, as torch divides them)"""
    f = np.float32
    rec = f(e["pos_gt"]) / f(e["n_pos"]) if e["n_pos"] else f(0)
    acc = f(e["pos_gt"] + e["n_neg"] - e["neg_gt"]) / f(e["n_pos"] + e["n_neg"])
    return rec, acc, np.int64(e["neg_ge"])


def average_ref(records, defects=(), dtype=np.float32):
    recs = [np.asarray(r, dtype) for r in records]
    n = dtype(len(recs))
    if "avg_divide_first" in defects:
        recs = [r / n for r in recs]
    acc = recs[0] * dtype(0)
    for r in recs:
        acc = acc + r
    return acc if "avg_divide_first" in defects else acc / n


# ------------------------------------------------------------------------------------------------------------------ the step, stateful
class Stepper:
    """One problem's training state and head_train_ref.ref_train's step on it (no defects of the step: those are ref_train's)."""

    def __init__(self, rec, T, D, pool, dtype=np.float64, order=0):
        self.dt, self.T, self.D, self.order = dtype, T, D, order
        self.pool = pool.reshape(pool.shape[0], -1)
        F = self.pool.shape[1]
        self.shuffle = np.random.default_rng(5)
        self.fperm = {0: None, 1: np.arange(F)[::-1], 2: None, 3: self.shuffle.permutation(F)}[order] if dtype == np.float32 else None
        self.P = R.unpack(rec, T, D, dtype)
        self.M = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.V = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.acc_steps, self.acc_samples, self.opt = 1, 0, 0

    def record(self):
        return np.concatenate([self.P[f].ravel() for f in T_.FIELDS])

    def new_sequence(self, defects=()):
        if "acc_not_reset_seq" not in defects:
            self.acc_steps, self.acc_samples = 1, 0
        if "moments_reset_seq" in defects:
            self.M = {k: np.zeros_like(v) for k, v in self.P.items()}
            self.V = {k: np.zeros_like(v) for k, v in self.P.items()}
            self.opt = 0

    def step(self, ix, yy, lr, nw):
        """-> (m, stepped, loss or NaN, p of the valid slots)"""
        dt, P_, M, V, order = self.dt, self.P, self.M, self.V, self.order
        valid = ix >= 0
        X = self.pool[ix[valid]].astype(dt)
        y = yy[valid].astype(dt)
        fw = R.forward(P_, X, dt, self.fperm)
        p = fw["p"]
        sel = ((y == 0) & (p >= dt(0.001))) | ((y == 1) & (p < dt(0.999)))
        m = int(sel.sum())
        if m == 0:
            return m, False, np.nan, p
        self.acc_samples += m
        if self.acc_samples < 128:
            self.acc_steps += 1
            return m, False, np.nan, p
        nwk = dt(nw)
        w = np.where(y == 1, dt(1), nwk)
        with np.errstate(divide="ignore"):
            bce = -(y * np.maximum(np.log(p), dt(-100)) + (1 - y) * np.maximum(np.log1p(-p), dt(-100)))
        denom_m, accd = dt(m), dt(self.acc_steps)
        loss = float((w * bce)[sel].sum(dtype=dt) / denom_m / accd)
        sp = (dt(1) - p) * p
        g = np.where(sel, (p - y) / np.maximum(sp, dt(1e-12)) * w * sp, dt(0))
        scale = dt(1) / accd / denom_m
        if dt == np.float64:
            g, scale = g * scale, dt(1)
        g = g[:, None]
        perm = self.shuffle.permutation(len(y)) if order == 3 else None
        o = order if dt == np.float32 else 0
        bs = lambda a: R._bsum(a, o, perm) * scale      # noqa: E731
        G = {}
        G["w3"] = bs(g * fw["h2"])
        G["b3"] = bs(g).reshape(1)
        da2 = np.where(fw["a2"] > 0, g * P_["w3"][None, :], dt(0))
        G["g2"], G["be2"] = bs(da2 * fw["xh2"]), bs(da2)
        dxh = da2 * P_["g2"]
        dz2 = fw["rstd2"] * (dxh - dxh.mean(axis=1, keepdims=True, dtype=dt) - fw["xh2"] * (dxh * fw["xh2"]).mean(axis=1, keepdims=True, dtype=dt))
        G["b2"] = bs(dz2)
        G["w2"] = R._mm_t(fw["h1"], dz2, o, perm) * scale
        da1 = np.where(fw["a1"] > 0, dz2 @ P_["w2"].T, dt(0))
        G["g1"], G["be1"] = bs(da1 * fw["xh1"]), bs(da1)
        dxh = da1 * P_["g1"]
        dz1 = fw["rstd1"] * (dxh - dxh.mean(axis=1, keepdims=True, dtype=dt) - fw["xh1"] * (dxh * fw["xh1"]).mean(axis=1, keepdims=True, dtype=dt))
        G["b1"] = bs(dz1)
        G["w1"] = R._mm_t(X, dz1, o, perm) * scale
        self.opt += 1
        t = self.opt
        step_size = dt(lr / (1.0 - 0.9 ** t))
        bc2 = 1.0 - 0.999 ** t
        for f in T_.FIELDS:
            M[f] = M[f] + (G[f] - M[f]) * dt(1.0 - 0.9)
            V[f] = V[f] * dt(0.999) + dt(1.0 - 0.999) * G[f] * G[f]
            den = np.sqrt(V[f]) / dt(np.sqrt(bc2)) + dt(1e-8)
            P_[f] = P_[f] + (-step_size * M[f]) / den
        self.acc_steps, self.acc_samples = 1, 0
        return m, True, loss, p


# ------------------------------------------------------------------------------------------------------------------ the case tables
#            name          D    T   U  pool shift  output layer x   what it is there for
E2E_TABLE = [("none_sel",  32,  2,  1, 0.3,        12),            # 54 of 55 checkpointed, none selected: the live model is returned
             ("all_t16",   48,  16, 1, 0.3,        12),            # every validation checkpointed, selected and averaged
             ("subset_t1", 16,  1,  1, 0.25,       16),            # some validations not checkpointed, a strict subset averaged
             ("mixed_u3",  32,  2,  3, 0.3,        12),            # three problems that decide differently
             ("varied_d32", 32, 1,  1, 0.2,        16)]            # recall, accuracy and false positives all vary: 52 checkpointed, 17 averaged
E2E_SALT = {"none_sel": 3, "subset_t1": 1, "mixed_u3": 9, "varied_d32": 14}           # generator seeds moved off their default where the default fails admission (test_auto_train_cpu.py)
E2E_STEPS, E2E_BATCH, E2E_VAL, E2E_FP = 200, 160, 300, 2000
GOLDEN_CASES = [t[0] for t in E2E_TABLE]


def make_e2e_case(name):
    _, D, T, U, shift, gain = next(t for t in E2E_TABLE if t[0] == name)
    k = [t[0] for t in E2E_TABLE].index(name)
    r = np.random.default_rng(5000 + k + 100 * E2E_SALT.get(name, 0))
    pool, lab = R._pool(r, 600, T, shift)
    vpool, vlab = R._pool(r, E2E_VAL + E2E_FP, T, shift)
    init = []
    for u in range(U):
        hd = T_.init_head(T, D, 900 + 8 * k + u)
        hd["net"]["w3"] *= np.float32(gain)
        hd["net"]["b3"] *= np.float32(gain)
        init.append(hd)
    problems = []
    for u in range(U):                                             # every problem its own half of the pool's rows of each class
        rows = r.permutation(600)[:400]
        problems.append((rows[lab[rows] == 1].astype(np.int32), rows[lab[rows] == 0].astype(np.int32)))
    val_idx = np.stack([r.permutation(E2E_VAL) for _ in range(U)]).astype(np.int32)
    val_idx[:, ::11] = -1                                          # empty slots
    val_y = np.where(val_idx >= 0, vlab[np.maximum(val_idx, 0)], 0).astype(np.uint8)
    neg = np.flatnonzero(vlab == 0)
    fp_idx = neg[r.integers(0, neg.size, size=E2E_FP)].astype(np.int32)      # one table shared by all problems, with duplicates
    return dict(name=name, D=D, T=T, U=U, steps=E2E_STEPS, n_batch=E2E_BATCH, seed=70 + k, pool=pool, val_pool=vpool, val_idx=val_idx,
                val_y=val_y, fp_idx=fp_idx, problems=problems, init_heads=init, init=np.stack([T_.head_to_record(h) for h in init]),
                max_negative_weight=1000, target_fp_per_hour=0.2)


def tables_of(case):
    """the index / label tables of the whole run, [U, total, n_batch]: one iter_tables generator across the three sequences"""
    total = case["steps"] + 2 * (case["steps"] // 10)
    return T_.draw_tables(case["problems"], total, case["n_batch"], case["seed"])


# ------------------------------------------------------------------------------------------------------------------ the policy
def sequences(case, defects=()):
    """train.py:268-324 restated: per sequence (n_steps, max_steps as the reference passes it, target lr, weights, val_steps array)"""
    steps, w, lr = case["steps"], case["max_negative_weight"], 0.0001
    out = [(int(steps), steps, lr, np.linspace(1, w, int(steps)).tolist(), np.linspace(steps - int(steps * 0.25), steps, 20).astype(np.int64), w)]
    steps = steps / 10
    for _ in range(2):
        lr = lr / 10
        if 1000 > case["target_fp_per_hour"] and "no_weight_doubling" not in defects:      # self.best_val_fp is never written
            w = w * 2
        out.append((int(steps), steps, lr, np.linspace(1, w, int(steps)).tolist(), np.linspace(1, steps, 20).astype(np.int16), w))
    return out


def auto_train_ref(case, dtype=np.float64, order=0, defects=()):
    """-> dict(params [U, n]: the combined records (dtype), live [U, n], per problem lists: counts (one dict of the five per validation,
    X_val's), fp_counts (the false-positive table's neg_ge), val_recall / val_accuracy / val_n_fp / val_fp_per_hr, val_at ((sequence,
    step) of every validation), ckpt_at ((sequence, step) of every checkpoint), selected (positions in the checkpoint list), weights
    (max_negative_weight per sequence), kept [total], stepped [total], loss [total], val_p: per validation the float scores of X_val's
    valid slots)."""
    defects = frozenset(defects)
    assert defects <= set(DEFECTS)
    dt = dtype
    idx, y = tables_of(case)
    seqs = sequences(case, defects)
    hrs = np.float32(VAL_SET_HRS)
    out = dict(params=[], live=[], counts=[], fp_counts=[], val_recall=[], val_accuracy=[], val_n_fp=[], val_fp_per_hr=[], val_at=[],
               ckpt_at=[], selected=[], weights=[s[5] for s in seqs], kept=[], stepped=[], loss=[], val_p=[], combined=[])
    for u in range(case["U"]):
        st = Stepper(case["init"][u], case["T"], case["D"], case["pool"], dt, order)
        H = dict(val_recall=[], val_accuracy=[], val_n_fp=[], val_fp_per_hr=[])
        counts, fp_counts, val_at, ckpts, scores, kept, stepped, loss, val_p = [], [], [], [], [], [], [], [], []
        g = 0

        def validate(si, k):
            ef, _ = eval_tables(st.record(), case["val_pool"], case["fp_idx"], np.zeros_like(case["fp_idx"]), dt, defects)
            ev, _ = eval_tables(st.record(), case["val_pool"], case["val_idx"][u], case["val_y"][u], dt, defects)
            rec, acc, nfp = metrics(ev)
            H["val_fp_per_hr"].append(np.float32(ef["neg_ge"]) / hrs)
            H["val_accuracy"].append(acc)
            H["val_recall"].append(rec)
            H["val_n_fp"].append(nfp)
            counts.append({c: ev[c] for c in COUNTS})
            fp_counts.append(ef["neg_ge"])
            val_at.append((si, k))
            val_p.append(ev["p"].astype(np.float64))
            fps, recs = (H["val_n_fp"][:-1], H["val_recall"][:-1]) if "pct_without_current" in defects and len(H["val_n_fp"]) > 1 else \
                (H["val_n_fp"], H["val_recall"])
            if H["val_n_fp"][-1] <= np.percentile(fps, 50) and H["val_recall"][-1] >= np.percentile(recs, 5):
                ckpts.append(st.record().copy())
                scores.append(dict(at=(si, k), val_recall=rec, val_accuracy=acc, val_fp_per_hr=H["val_fp_per_hr"][-1]))

        for si, (n, max_steps, lr, weights, val_steps, _) in enumerate(seqs):
            if si:
                st.new_sequence(defects)
            warm, hold = max_steps // 5, max_steps // 3
            for k in range(n):
                due = k in val_steps and (k > 1 or "step_gt1_dropped" in defects)
                if due and "val_before_step" in defects:
                    validate(si, k)
                lrk = float(T_.lr_warmup_cosine_decay(k, warmup_steps=warm, hold=hold, total_steps=max_steps, target_lr=lr))
                m, s, ls, _ = st.step(idx[u, g], y[u, g], lrk, np.float32(weights[k]))
                kept.append(m), stepped.append(s), loss.append(ls)
                g += 1
                if due and "val_before_step" not in defects:
                    validate(si, k)
        a, r_, f = np.percentile(H["val_accuracy"], 90), np.percentile(H["val_recall"], 90), np.percentile(H["val_fp_per_hr"], 10)
        sel = [i for i, s in enumerate(scores) if s["val_accuracy"] >= a and s["val_recall"] >= r_ and s["val_fp_per_hr"] <= f]
        if sel:
            comb = average_ref([ckpts[i] for i in sel], defects, dt)
        else:
            comb = ckpts[0] if "fallback_checkpoint" in defects and ckpts else st.record()
        ec, _ = eval_tables(comb, case["val_pool"], case["val_idx"][u], case["val_y"][u], dt, defects)
        efc, _ = eval_tables(comb, case["val_pool"], case["fp_idx"], np.zeros_like(case["fp_idx"]), dt, defects)
        rec, acc, _ = metrics(ec)
        out["combined"].append(dict(recall=rec, accuracy=acc, fp_per_hr=np.float32(efc["neg_ge"]) / hrs))
        out["params"].append(np.asarray(comb)), out["live"].append(st.record())
        out["counts"].append(counts), out["fp_counts"].append(fp_counts), out["val_at"].append(val_at), out["val_p"].append(val_p)
        for k_ in H:
            out[k_].append(np.asarray(H[k_]))
        out["ckpt_at"].append([s["at"] for s in scores]), out["selected"].append(sel)
        out["kept"].append(np.asarray(kept)), out["stepped"].append(np.asarray(stepped)), out["loss"].append(np.asarray(loss))
    out["params"], out["live"] = np.stack(out["params"]), np.stack(out["live"])
    return out


def same_run(a, b):
    """the decisions of two runs agree: kept counts, step / skip, the five counts of every validation, checkpoint steps, selected sets
    -> None, or what differs"""
    for u in range(len(a["kept"])):
        for f in ("kept", "stepped"):
            if not np.array_equal(a[f][u], b[f][u]):
                return f"{f} of problem {u}"
        for f in ("val_at", "counts", "fp_counts", "ckpt_at", "selected"):
            if list(a[f][u]) != list(b[f][u]):
                return f"{f} of problem {u}"
    return None


def half_margin(run):
    """the smallest distance of one of X_val's validation scores from 0.5.  The false-positive table's scores are exempt from the margin
    rule: 2,000 rows x 55 validations are 110,000 scores spread over [0, 1], of which about ten fall within 16 x dp (3e-5 .. 1e-4) of
    0.5 on any seed (mixed_u3: the closest lies 7e-6 away), so no case could be admitted under it.  What holds them instead: their
    counts agree at all 55 validations across the reference in fp32 and double and the restatement in float64 and fp32 under four
    orders (same_run compares fp_counts), and the device is held to those counts exactly, so a flipped score fails a test by name."""
    return min(float(np.abs(p - 0.5).min()) for vp in run["val_p"] for p in vp if p.size)


# ------------------------------------------------------------------------------------------------------------------ the reference's class
def binary_recall(preds, target):
    """torchmetrics.Recall(task='binary') as documented, for predictions in [0, 1]"""
    import torch
    pred, t = preds.reshape(-1) > 0.5, target.reshape(-1) == 1
    tp, fn = (pred & t).sum(), (~pred & t).sum()
    return tp / (tp + fn) if int(tp + fn) else torch.zeros((), dtype=torch.float32)


def binary_accuracy(preds, target):
    pred, t = preds.reshape(-1) > 0.5, target.reshape(-1) == 1
    return (pred == t).sum() / t.numel()


def run_reference_auto_train(case, double=False, fp_batch=768):
    """train.Model.auto_train on the case's batches, model.device = CPU, the initial weights the case's, one shared iterator of batches
    across the three train_model calls -> the dict auto_train_ref returns (None where the reference is absent).  Counts and val_p are
    taken from the outputs the reference's own network produced (a forward hook), its histories from model.history."""
    tr = R.reference_train_module()
    if tr is None:
        return None
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(1)
    tdt = torch.float64 if double else torch.float32
    T, D, U = case["T"], case["D"], case["U"]
    idx, y = tables_of(case)
    total = idx.shape[1]
    seqs = sequences(case)
    out = dict(params=[], live=[], counts=[], fp_counts=[], val_recall=[], val_accuracy=[], val_n_fp=[], val_fp_per_hr=[], val_at=[],
               ckpt_at=[], selected=[], weights=[s[5] for s in seqs], kept=[], stepped=[], loss=[], val_p=[], combined=[])
    fp_rows = [case["fp_idx"][a:a + fp_batch] for a in range(0, len(case["fp_idx"]), fp_batch)]
    fp_data = [(torch.from_numpy(case["val_pool"][r]).to(tdt), torch.zeros(len(r), dtype=torch.int64)) for r in fp_rows]
    for u in range(U):
        model = tr.Model(n_classes=1, input_shape=(T, 96), model_type="dnn", layer_dim=D, n_blocks=1)
        model.device = torch.device("cpu")
        model.recall, model.accuracy = binary_recall, binary_accuracy
        P_ = R.unpack(case["init"][u], T, D, np.float64)
        net = model.model

        def layers(n):
            return (((n.layer1, "w1", "b1"), (n.blocks[0].fcn_layer, "w2", "b2"), (n.last_layer, "w3", "b3")),
                    ((n.layernorm1, "g1", "be1"), (n.blocks[0].layer_norm, "g2", "be2")))

        with torch.no_grad():
            for lin, w, b in layers(net)[0]:
                lin.weight.copy_(torch.from_numpy(P_[w].reshape(-1, lin.weight.shape[0]).T.copy()))
                lin.bias.copy_(torch.from_numpy(P_[b]))
            for ln, g, b in layers(net)[1]:
                ln.weight.copy_(torch.from_numpy(P_[g]))
                ln.bias.copy_(torch.from_numpy(P_[b]))
        if double:
            net.double()
            bce = model.loss
            model.loss = lambda p, t, w, _f=bce: _f(p, t.to(p.dtype), w.to(p.dtype))
        model.optimizer = torch.optim.Adam(net.parameters(), lr=0.0001)

        def record_of(n):
            rec = {}
            for lin, w, b in layers(n)[0]:
                rec[w], rec[b] = lin.weight.detach().numpy().T.copy(), lin.bias.detach().numpy().copy()
            for ln, g, b in layers(n)[1]:
                rec[g], rec[b] = ln.weight.detach().numpy().copy(), ln.bias.detach().numpy().copy()
            return np.concatenate([rec[f].ravel() for f in T_.FIELDS])

        log = []                                   # ("batch", g) markers and ("out", p) of every forward call, in order
        net.register_forward_hook(lambda mod, i, o: log.append(("out", o.detach().squeeze(-1).numpy().copy())))

        def batches():
            for g in range(total):
                valid = idx[u, g] >= 0
                log.append(("batch", g))
                yield torch.from_numpy(case["pool"][idx[u, g][valid]]).to(tdt), torch.from_numpy(y[u, g][valid].astype(np.int64))

        vvalid = case["val_idx"][u] >= 0
        vy = case["val_y"][u][vvalid]
        x_val = [(torch.from_numpy(case["val_pool"][case["val_idx"][u][vvalid]]).to(tdt), torch.from_numpy(vy.astype(np.int64)))]
        picked = []
        avg = model.average_models
        model.average_models = lambda models=None: (picked.extend(next(i for i, b in enumerate(model.best_models) if b is m) for m in models),
                                                    avg(models=models))[1]
        combined = model.auto_train(batches(), x_val, fp_data, steps=case["steps"], max_negative_weight=case["max_negative_weight"],
                                    target_fp_per_hour=case["target_fp_per_hour"])
        # ---- read the log: per batch marker the training forward, then (at a validation) the false-positive batches and X_val ----
        starts = [i for i, e in enumerate(log) if e[0] == "batch"]
        bounds = starts + [len(log)]
        seq_of, g0 = [], 0
        for si, s in enumerate(seqs):
            seq_of += [(si, k) for k in range(s[0])]
        kept, stepped, counts, fp_counts, val_at, val_p = [], [], [], [], [], []
        acc_samples = 0
        for g, a in enumerate(starts):
            outs = [e[1] for e in log[a + 1:bounds[g + 1]]]
            si, k = seq_of[g]
            if k == 0:
                acc_samples = 0
            yy = y[u, g][idx[u, g] >= 0]
            p = outs[0]
            sel = ((yy == 0) & (p >= 0.001)) | ((yy == 1) & (p < 0.999))
            m = int(sel.sum())
            kept.append(m)
            acc_samples += m
            stepped.append(m > 0 and acc_samples >= 128)
            if stepped[-1]:
                acc_samples = 0
            rest = outs[1:]
            if g == total - 1:                     # the merge's own evaluation comes last: X_val, then the false-positive batches
                rest = rest[:len(rest) - 1 - len(fp_data)]
            if rest:
                assert len(rest) == len(fp_data) + 1, (g, len(rest))
                pf, pv = np.concatenate(rest[:-1]), rest[-1]
                fp_counts.append(int((pf >= 0.5).sum()))
                counts.append(dict(n_pos=int((vy == 1).sum()), n_neg=int((vy == 0).sum()), pos_gt=int(((vy == 1) & (pv > 0.5)).sum()),
                                   neg_gt=int(((vy == 0) & (pv > 0.5)).sum()), neg_ge=int(((vy == 0) & (pv >= 0.5)).sum())))
                val_at.append((si, k))
                val_p.append(pv.astype(np.float64))
        assert sum(stepped) == len(model.history["loss"]), "the reference stepped where the counters say it should not"
        H = {f: np.asarray(model.history[f]) for f in ("val_recall", "val_accuracy", "val_n_fp", "val_fp_per_hr")}
        assert len(val_at) == len(H["val_n_fp"])
        # the checkpoints' (sequence, step): training_step_ndx restarts in every sequence; the validations are in order
        ckpt_at, j = [], 0
        for s in model.best_model_scores:
            while not (val_at[j][1] == s["training_step_ndx"] and H["val_n_fp"][j] == s["val_n_fp"] and H["val_recall"][j] == s["val_recall"]):
                j += 1
            ckpt_at.append(val_at[j])
            j += 1
        with torch.no_grad():
            pv = combined(x_val[0][0]).squeeze(-1).numpy()
            pf = np.concatenate([combined(b[0]).squeeze(-1).numpy() for b in fp_data])
        ec = dict(n_pos=int((vy == 1).sum()), n_neg=int((vy == 0).sum()), pos_gt=int(((vy == 1) & (pv > 0.5)).sum()),
                  neg_gt=int(((vy == 0) & (pv > 0.5)).sum()), neg_ge=0)
        rec, acc, _ = metrics(ec)
        out["combined"].append(dict(recall=rec, accuracy=acc, fp_per_hr=np.float32(int((pf >= 0.5).sum())) / np.float32(VAL_SET_HRS)))
        out["params"].append(record_of(combined)), out["live"].append(record_of(net))
        out["counts"].append(counts), out["fp_counts"].append(fp_counts), out["val_at"].append(val_at), out["val_p"].append(val_p)
        for k_ in H:
            out[k_].append(H[k_])
        out["ckpt_at"].append(ckpt_at), out["selected"].append(sorted(picked))
        out["kept"].append(np.asarray(kept)), out["stepped"].append(np.asarray(stepped))
        out["loss"].append(np.asarray([float(v) for v in model.history["loss"]]))
    out["params"], out["live"] = np.stack(out["params"]), np.stack(out["live"])
    return out


# ------------------------------------------------------------------------------------------------------------------ the eval case table
#             name            D    T   U  n    regime      shared
EVAL_TABLE = [("fresh_n1",    16,  1,  1, 1,   "fresh",    False),
              ("fresh_n63",   48,  2,  1, 63,  "fresh",    False),
              ("spread_n64",  16,  2,  3, 64,  "spread",   True),         # one table for all problems
              ("spread_n65",  128, 1,  1, 65,  "spread",   False),
              ("spread_n300", 48,  16, 3, 300, "spread",   False),        # per-problem tables, -1 slots and duplicates
              ("half_n300",   16,  1,  1, 300, "half",     False),        # w3 = 0, b3 = 0: p = 0.5f exactly on every row
              ("sat_n65",     128, 16, 1, 65,  "saturate", False),        # output layer x 400: every score of the table at 0 or 1
              ("fresh_n300",  128, 2,  3, 300, "fresh",    True)]
EVAL_SALT = {}
HALF = "half_n300"
EVAL_POOL = 200


def make_eval_case(name):
    _, D, T, U, n, regime, shared = next(t for t in EVAL_TABLE if t[0] == name)
    k = [t[0] for t in EVAL_TABLE].index(name)
    r = np.random.default_rng(7000 + k + 100 * EVAL_SALT.get(name, 0))
    pool, lab = R._pool(r, EVAL_POOL, T, 0.3)
    init = [T_.init_head(T, D, 300 + 8 * k + u) for u in range(U)]
    for hd in init:
        if regime == "spread":
            hd["net"]["w3"] *= 12
            hd["net"]["b3"] *= 12
        if regime == "half":
            hd["net"]["w3"][:] = 0
            hd["net"]["b3"][:] = 0
        if regime == "saturate":
            hd["net"]["w3"] *= 400
    idx = r.integers(0, EVAL_POOL, size=(n,) if shared else (U, n)).astype(np.int32)
    if n >= 63:
        idx[..., ::7] = -1                                         # empty slots
        idx[..., 1::5] = idx[..., 2::5][..., :idx[..., 1::5].shape[-1]]      # duplicates
    if regime == "saturate":                                       # rows deep in saturation alone (|logit| > 25 in float64), of both signs
        lg = R.forward(R.unpack(T_.head_to_record(init[0]), T, D, np.float64), pool.reshape(EVAL_POOL, -1), np.float64)["lg"]
        deep = np.flatnonzero(np.abs(lg) > 25)
        assert (lg[deep] > 0).any() and (lg[deep] < 0).any() and U == 1
        idx = np.where(idx >= 0, deep[np.maximum(idx, 0) % deep.size], -1).astype(np.int32)
    y = np.where(idx >= 0, lab[np.maximum(idx, 0)], 0).astype(np.uint8)
    return dict(name=name, D=D, T=T, U=U, n=n, regime=regime, shared=shared, pool=pool, idx=idx, y=y, init_heads=init,
                init=np.stack([T_.head_to_record(h) for h in init]))


def eval_case_ref(case, dtype=np.float64, defects=()):
    """-> (counts [U] of dicts, scores [U, n] float64 with NaN in empty slots)"""
    cs, ss = [], []
    for u in range(case["U"]):
        ix, yy = (case["idx"], case["y"]) if case["shared"] else (case["idx"][u], case["y"][u])
        e, sc = eval_tables(case["init"][u], case["pool"], ix, yy, dtype, defects)
        cs.append({c: e[c] for c in COUNTS})
        ss.append(sc)
    return cs, np.stack(ss)


# the mid-accumulation case: batches of 100 fire every second step, sequence 2 has 5 steps, so sequence 3 opens with 100 samples held
MIDACC = dict(name="midacc", D=16, T=1, U=1, steps=50, n_batch=100)


def make_midacc_case():
    r = np.random.default_rng(8100)
    pool, lab = R._pool(r, 400, 1, 0.3)
    vpool, vlab = R._pool(r, 400, 1, 0.3)
    hd = T_.init_head(1, 16, 811)
    rows = np.arange(400)
    val_idx = r.permutation(300)[None, :200].astype(np.int32)
    neg = np.flatnonzero(vlab == 0)
    return dict(MIDACC, seed=81, pool=pool, val_pool=vpool, val_idx=val_idx, val_y=vlab[val_idx].astype(np.uint8),
                fp_idx=neg[r.integers(0, neg.size, size=500)].astype(np.int32),
                problems=[(rows[lab == 1].astype(np.int32), rows[lab == 0].astype(np.int32))], init_heads=[hd],
                init=np.stack([T_.head_to_record(hd)]), max_negative_weight=1000, target_fp_per_hour=0.2)
