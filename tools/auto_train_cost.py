"""Cost of one validation of all heads of a training session: oww_train_eval over the validation set and the
false-positive set, against the two other ways to get the same numbers on the same GPU.

    python tools/auto_train_cost.py --leg eval  --problems 64 [--out FILE]
    python tools/auto_train_cost.py --leg bank  --problems 64 [--out FILE]
    python tools/auto_train_cost.py --leg torch --problems 64 [--out FILE]

Shape: hidden 32, T = 16, validation set 300 rows, false-positive set 65,536 rows, one table shared by all problems.
  eval   HeadTrainer.evaluate twice (validation rows with labels, false-positive rows), live parameters.
  bank   what the library offered before oww_train_eval: heads() (one device-to-host copy per head), bank_add, bank_score_stats on
         the same rows (each window a one-window feature sequence), bank_remove; the f16-split bank kernels, not the trainer's fp32.
  torch  the same forward in PyTorch on cuda tensors, one model after the other, min(U, 8) models timed (linear in the models).
One leg per process, so that each runs under its own time limit; each prints one JSON line and appends it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, D, N_VAL, N_FP, P = 16, 32, 300, 65536, 8192


def _data():
    r = np.random.default_rng(0)
    lab = (np.arange(P) % 2).astype(np.uint8)
    d = r.normal(size=(T, 96)) / np.sqrt(T * 96.0)
    pool = (r.normal(size=(P, T, 96)) + 3.0 * (lab[:, None, None] * 2.0 - 1.0) * d).astype(np.float32)
    val = r.integers(0, P, size=N_VAL).astype(np.int32)
    neg = np.flatnonzero(lab == 0)
    fp = neg[r.integers(0, neg.size, size=N_FP)].astype(np.int32)
    return pool, val, lab[val], fp


def _timed(fn, repeats=3):
    fn()                                             # warm-up: code objects, scratch growth
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return times


def _bm(U):
    from openwakeword_amd import weights as W
    from openwakeword_amd.model import BatchedModel
    return BatchedModel(4, ["alexa"], weights={"heads": {"alexa": W.synthetic_head("alexa", 1234)}, "embedding": W.synthetic_embedding(3)},
                        bank_slots=1, bank_capacity=max(U, 8))


def leg_eval(U):
    bm = _bm(U)
    pool, val, val_y, fp = _data()
    tr = bm.head_trainer(T, D, U)
    tr.set_eval_pool(pool)
    out = {}

    def once():
        out["val"], out["fp"] = tr.evaluate(val, val_y), tr.evaluate(fp, np.zeros_like(fp, dtype=np.uint8))

    times = _timed(once)
    tr.close()
    bm.close()
    return dict(leg="eval", problems=U, validation_s=[round(v, 5) for v in times], ms_per_validation=1e3 * min(times),
                n_fp_first=int(out["fp"]["n_fp"][0]))


def leg_bank(U):
    bm = _bm(U)
    pool, val, val_y, fp = _data()
    tr = bm.head_trainer(T, D, U)
    rows_val, rows_fp = pool[val], pool[fp]          # [n, T, 96]: n one-window sequences (the gather is not timed)
    out = {}

    def once():
        ids = [bm.bank_add(h) for h in tr.heads()]
        out["val"], out["fp"] = bm.bank_score_stats(rows_val, ids), bm.bank_score_stats(rows_fp, ids)
        for i in ids:
            bm.bank_remove(i)

    times = _timed(once)
    tr.close()
    bm.close()
    return dict(leg="bank", problems=U, validation_s=[round(v, 5) for v in times], ms_per_validation=1e3 * min(times),
                n_fp_first=int(out["fp"]["count"][:, 0].sum()))


def leg_torch(U):
    import torch
    from torch import nn
    dev = torch.device("cuda")
    n_models = min(U, 8)
    pool, val, val_y, fp = _data()
    pool_d = torch.from_numpy(pool).to(dev)
    val_d, fp_d = torch.from_numpy(val.astype(np.int64)).to(dev), torch.from_numpy(fp.astype(np.int64)).to(dev)
    y_d = torch.from_numpy(val_y.astype(np.int64)).to(dev)
    models = [nn.Sequential(nn.Flatten(), nn.Linear(T * 96, D), nn.LayerNorm(D), nn.ReLU(), nn.Linear(D, D), nn.LayerNorm(D), nn.ReLU(),
                            nn.Linear(D, 1), nn.Sigmoid()).to(dev) for _ in range(n_models)]
    out = {}

    def once():
        with torch.no_grad():
            for net in models:                       # train.py:514-553: the false-positive batches, then X_val
                n_fp = 0
                for a in range(0, N_FP, 8192):
                    p = net(pool_d[fp_d[a:a + 8192]])
                    n_fp += (0 - p <= -0.5).sum()
                p = net(pool_d[val_d]).squeeze(-1)
                pred = p > 0.5
                rec = (pred & (y_d == 1)).sum() / (y_d == 1).sum()
                acc = (pred == (y_d == 1)).sum() / y_d.numel()
                out["last"] = (int(n_fp), float(rec), float(acc))      # the host reads each model's numbers, as the history does
        torch.cuda.synchronize()

    times = _timed(once)
    return dict(leg="torch", problems=U, models_timed=n_models, validation_s=[round(v, 5) for v in times],
                ms_per_validation=1e3 * min(times) * U / n_models)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("eval", "bank", "torch"), required=True)
    ap.add_argument("--problems", type=int, required=True)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("auto_train_cost needs the GPU: a timing taken elsewhere says nothing about it")
    rec = {"eval": leg_eval, "bank": leg_bank, "torch": leg_torch}[a.leg](a.problems)
    rec.update(hidden=D, T=T, validation_rows=N_VAL, false_positive_rows=N_FP, pool=P)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
