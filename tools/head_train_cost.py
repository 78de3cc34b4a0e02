"""Cost of training bank heads on the device: optimizer steps per second of oww_train_steps at U problems side by
side, against the same step run by PyTorch on the same GPU, one model after the other.

    python tools/head_train_cost.py --leg device --problems 64 [--out FILE]
    python tools/head_train_cost.py --leg torch --problems 64 [--out FILE]

Shape: hidden 32, T = 16, n_batch = 1,124 (the batch of the reference's examples/custom_model.yml), a pool of 20,000 Gaussian windows
with a class shift, half of every batch positive, lr 1e-4, negative weight 1.  One leg per process, so that each runs under its own
time limit; each prints one JSON line and appends it to --out.  The torch leg restates train.py:447-510 for the network of
train.py:66-83 on cuda tensors (batch gathered on the device, as the library does) and times min(U, 8) models in sequence: its cost is
linear in the models, `problem_steps_per_s` is per model either way."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, D, N_BATCH, P, K = 16, 32, 1124, 20000, 50


def _data(U, steps):
    r = np.random.default_rng(0)
    lab = (np.arange(P) % 2).astype(np.uint8)
    d = r.normal(size=(T, 96)) / np.sqrt(T * 96.0)
    pool = (r.normal(size=(P, T, 96)) + 3.0 * (lab[:, None, None] * 2.0 - 1.0) * d).astype(np.float32)
    idx = r.integers(0, P, size=(U, steps, N_BATCH)).astype(np.int32)
    return pool, idx, lab[idx]


def leg_device(U):
    from openwakeword_amd import train as T_
    from openwakeword_amd import weights as W
    from openwakeword_amd.engine import StreamEngine
    e = StreamEngine(4, {"alexa": W.synthetic_head("alexa", 1234)}, W.synthetic_embedding(3))
    pool, idx, y = _data(U, K)
    tr = T_.HeadTrainer(e, T, D, U)
    tr.set_pool(pool)
    tr.steps(idx, y, 1e-4, 1.0)                      # warm-up: code objects, scratch growth
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        loss, m = tr.steps(idx, y, 1e-4, 1.0)        # returns when the K steps are done
        times.append(time.perf_counter() - t0)
    n_opt = int(np.isfinite(loss).sum())
    tr.close()
    e.close()
    t = min(times)
    return dict(leg="device", problems=U, steps_per_call=K, call_s=[round(v, 5) for v in times], optimizer_steps_per_call=n_opt,
                problem_steps_per_s=U * K / t, ms_per_step_all_problems=1e3 * t / K)


def leg_torch(U):
    import torch
    from torch import nn
    dev = torch.device("cuda")
    n_models = min(U, 8)
    pool, idx, y = _data(n_models, K)
    pool_d = torch.from_numpy(pool).to(dev)
    idx_d, y_d = torch.from_numpy(idx.astype(np.int64)).to(dev), torch.from_numpy(y.astype(np.int64)).to(dev)

    def make():
        net = nn.Sequential(nn.Flatten(), nn.Linear(T * 96, D), nn.LayerNorm(D), nn.ReLU(), nn.Linear(D, D), nn.LayerNorm(D), nn.ReLU(),
                            nn.Linear(D, 1), nn.Sigmoid()).to(dev)
        return net, torch.optim.Adam(net.parameters(), lr=1e-4)

    def run(models):
        n_opt = 0
        for u, (net, opt) in enumerate(models):
            acc_steps, acc_samples = 1, 0
            for k in range(K):
                x, yy = pool_d[idx_d[u, k]], y_d[u, k]
                opt.zero_grad()
                p = net(x)
                sel = ((yy == 0) & (p.squeeze() >= 0.001)) | ((yy == 1) & (p.squeeze() < 0.999))
                p, ys = p[sel], yy[sel][..., None].to(torch.float32)
                w = torch.ones_like(ys)
                if p.shape[0] != 0:
                    loss = torch.nn.functional.binary_cross_entropy(p, ys, w) / acc_steps
                    acc_samples += p.shape[0]
                    if acc_samples < 128:
                        acc_steps += 1
                    else:
                        loss.backward()
                        opt.step()
                        acc_steps, acc_samples = 1, 0
                        n_opt += 1
        torch.cuda.synchronize()
        return n_opt

    run([make()])                                    # warm-up
    models = [make() for _ in range(n_models)]
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_opt = run(models)
        times.append(time.perf_counter() - t0)
    t = min(times)
    return dict(leg="torch", problems=U, models_timed=n_models, steps_per_call=K, call_s=[round(v, 5) for v in times], optimizer_steps_per_call=n_opt,
                problem_steps_per_s=n_models * K / t, ms_per_step_all_problems=1e3 * t / K * U / n_models)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("device", "torch"), required=True)
    ap.add_argument("--problems", type=int, required=True)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("head_train_cost needs the GPU: a timing taken elsewhere says nothing about it")
    rec = (leg_device if a.leg == "device" else leg_torch)(a.problems)
    rec.update(hidden=D, T=T, n_batch=N_BATCH, pool=P)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
