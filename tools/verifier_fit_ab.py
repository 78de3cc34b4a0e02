"""Times the device-side verifier fit (oww_verifier_fit) against the reference's scikit-learn pipeline on the same problems.

  python tools/verifier_fit_ab.py [--out profiles/verifier_fit.jsonl] [--repeats 5] [--sklearn-problems 64]

Shapes (T = 16): U = 1024 problems of N = 64, U = 1024 of N = 256, U = 64 of N = 1024; Gaussian(0, 4) windows with a shifted positive
third, resident on the device (windows_on_device = 1), so that the figure is the fit and not the PCIe copy.  The call returns when its
last kernel has finished, so the host clock round the call is the device time plus one launch round trip per slab; one warm-up call
(scratch growth), then `repeats` calls, median and spread reported, the pool emptied in between.  The Gram kernel's executed f16
flops: tiles x 32 x 32 x D x 2 x 3 products (tiles on or above the diagonal only); its time comes from a per-kernel trace
(`rocprofv3 --kernel-trace --stats -- python tools/verifier_fit_ab.py --repeats 1`), which this script does not start itself.
scikit-learn: the pipeline of custom_verifier_model.py:95-113 at its default tolerance, `--sklearn-problems` problems of each shape
over 16 processes, scaled to U."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 64), (1024, 256), (64, 1024)]
T = 16
D = T * 96


def problems(U, N, seed=0):
    r = np.random.default_rng(seed)
    X = r.normal(0, 4.0, (U * N, D)).astype(np.float32)
    y = np.zeros((U, N), np.uint8)
    y[:, :N // 3] = 1
    shift = r.normal(0, 1.2, (U, 1, D)).astype(np.float32)
    X.reshape(U, N, D)[:, :N // 3] += shift
    return X, y.ravel()


def _sk_one(args):
    X, y = args
    import warnings
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        make_pipeline(StandardScaler(), LogisticRegression(random_state=0, max_iter=2000, C=0.001)).fit(X, y)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-problems", type=int, default=64)
    a = ap.parse_args()
    import torch
    from openwakeword_amd import _lib, weights as W
    from openwakeword_amd.engine import StreamEngine
    e = StreamEngine(4, {"alexa": W.synthetic_head("alexa", 1234)}, W.synthetic_embedding(1234), verifier_capacity=1024)
    build = _lib.load().oww_build_info().decode()
    rows = []
    for U, N in SHAPES:
        X, y = problems(U, N)
        off = np.arange(U + 1, dtype=np.int64) * N
        xd = torch.from_numpy(X).cuda()
        torch.cuda.synchronize()
        times = []
        for k in range(a.repeats + 1):
            t0 = time.perf_counter()
            res = e.verifier_fit(xd, off, y, T, 0.001, on_device=True)
            dt = time.perf_counter() - t0
            assert all(r["status"] == 0 for r in res), [r for r in res if r["status"]][:3]
            for r in res:
                e.verifier_remove(r["id"])
            if k:
                times.append(dt)
        tiles = U * ((N + 31) // 32) * ((N + 31) // 32 + 1) // 2
        n_sk = min(U, a.sklearn_problems)
        jobs = [(X[u * N:(u + 1) * N], y[u * N:(u + 1) * N]) for u in range(n_sk)]
        with ProcessPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            list(pool.map(_sk_one, jobs))
            t_sk = (time.perf_counter() - t0) * U / n_sk
        row = dict(U=U, N=N, T=T, build=build, device_s_median=float(np.median(times)), device_s_min=min(times), device_s_max=max(times),
                   iterations_max=max(r["iterations"] for r in res), gram_tiles=tiles, gram_f16_flops=tiles * 32 * 32 * D * 2 * 3,
                   sklearn_16proc_s=t_sk, sklearn_problems_timed=n_sk)
        print(json.dumps(row), flush=True)
        rows.append(row)
    e.close()
    if a.out:
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
