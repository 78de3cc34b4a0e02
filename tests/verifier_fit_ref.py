"""Test infrastructure for the device-side custom-verifier fit (include/owwhip.h: oww_verifier_fit; the reference:
custom_verifier_model.py:95-113, flatten -> StandardScaler -> LogisticRegression(C=0.001)).  HIP-free.

The definition.  Windows X [N, D] fp32, labels y in {0,1}^N:
  1. mu_j = mean_i X_ij, var_j with ddof = 0, s_j = sqrt(var_j), s_j = 1 where var_j == 0 (StandardScaler's rule); Z = (X - mu) / s.
  2. (wt, b) = argmin C sum_i l(y_i, z_i . wt + b) + 1/2 |wt|^2, l the logistic loss, b not penalised.
  3. w = wt / s, bias = b - sum_j w_j mu_j.
Solved in the dual: K = Z Z^T, wt = Z^T a, scores f = K a + b, J(a, b) = C sum l(f_i) + 1/2 a^T K a.  With p = sigmoid(f), g = p - y,
W = p (1 - p) a Newton step solves
      (I + C diag(W) K) da + C W db = -(C g + a),      C (W^T K) da + C sum(W) db = -C sum(g).
At the optimum a = -C (p - y), so res = max_i |a_i + C (p_i - y_i)| / C is a stationarity residual in score units.

  fit64        the float64 definition: the Newton iteration above with a dense solve, stopped at res <= 1e-13.
  fit32        an fp32 restatement of the kernels (owwhip_fit.h) in their order of operations: fp64 statistics, z rounded to fp32 and
               split into f16 hi / lo, Gram matrix hh + hl + lh accumulated in fp32 over 32 x 32 tiles on or above the diagonal and
               mirrored, the fp32 Newton iteration in the kernel's symmetric form (below) with its joint conjugate gradients, stop rule
               and step halving, and the fp64 fold.  `defect` switches one of DEFECTS on.

The kernel's form of the Newton step.  With df = K da + db the first equation reads a + da = -C (g + W df); with S = sqrt(W) and
v = S df that is  (I + C S K S) v = S (-K (C g + a) + db 1),  a symmetric positive definite system whatever K and W are (no division
by W).  v = v1 + db v2 from two solves that share every pass over K, and db follows from the second equation, which says
sum_i (g_i + S_i v_i) = 0:  db = -sum(g + S v1) / sum(S v2).
"""
import functools

import numpy as np

MAX_N = 1024                 # OWW_FIT_MAX_N
TILE = 32                    # rows of a Gram tile (owf::kTile)
NEWTON_CAP = 40              # owf::kNewtonCap
EPS_STOP = 1.5e-6             # owf::kEpsStop: 8 x the largest residual floor of fit32 over CASES (tests/test_verifier_fit_cpu.py prints them)
CG_RTOL2 = 1e-10             # conjugate gradients stop at |r|^2 <= this x |rhs|^2 ...
J_NOISE = 1e-5               # a step is halved only where J rises by more than this x |J|
MAX_HALVINGS = 8

ST_OK, ST_ONE_CLASS, ST_BAD_N, ST_NONFINITE, ST_NOT_CONVERGED = 0, 1, 2, 3, 4

DEFECTS = ("ddof1", "no_const_rule", "intercept_penalised", "hh_only", "no_mirror", "row_overrun", "c_on_regulariser", "fp32_fold", "one_step")


def cg_cap(N):               # ... or after this many steps (owf::cg_cap)
    return 2 * N + 32


def sigmoid(f):
    return 1.0 / (1.0 + np.exp(-f))


def scores(w, bias, A):
    """sigmoid(A . w + bias) in float64: what the verifier kernels compute for window rows A [M, D]"""
    return sigmoid(A.astype(np.float64) @ np.asarray(w, np.float64) + float(bias))


def stats64(X, ddof=0, const_rule=True):
    X64 = X.astype(np.float64)
    mu = X64.mean(0)
    var = ((X64 - mu) ** 2).sum(0) / (X.shape[0] - ddof)
    s = np.sqrt(var)
    if const_rule:
        s[var == 0] = 1.0
    return X64, mu, s


def fit64(X, y, C=1e-3, iters=100):
    """-> (w, bias, iterations, res) in float64"""
    X64, mu, s = stats64(X)
    N = X.shape[0]
    Z = (X64 - mu) / s
    K = Z @ Z.T
    y = np.asarray(y, np.float64)
    a = np.zeros(N)
    b = 0.0
    best = None
    for it in range(1, iters + 1):
        f = K @ a + b
        p = sigmoid(f)
        g = p - y
        W = p * (1 - p)
        A = np.zeros((N + 1, N + 1))
        A[:N, :N] = C * W[:, None] * K + np.eye(N)
        A[:N, N] = C * W
        A[N, :N] = C * (W @ K)
        A[N, N] = C * W.sum()
        d = np.linalg.solve(A, -np.concatenate([C * g + a, [C * g.sum()]]))
        a = a + d[:N]
        b = b + d[N]
        res = np.abs(a + C * (sigmoid(K @ a + b) - y)).max() / C
        if best is None or res < best[0]:
            best = (res, a.copy(), b, it)
        if res <= 1e-13:
            break
    res, a, b, it = best
    w = (Z.T @ a) / s
    return w, b - (w * mu).sum(), it, res


def tile_count(N):
    nt = (N + TILE - 1) // TILE
    return nt * (nt + 1) // 2


def tile_map(Ns):
    """the triangular Gram grid of a slab: (problem, tile row, tile column) of every tile on or above the diagonal, problem-major, row-major"""
    out = []
    for u, N in enumerate(Ns):
        nt = (N + TILE - 1) // TILE
        out += [(u, r, c) for r in range(nt) for c in range(r, nt)]
    return out


def problem_bytes(N, D, on_device):
    """scratch bytes of one problem (owf::problem_bytes): staged windows, the Z halves, the Gram matrix, statistics and vectors"""
    return (0 if on_device else N * D * 4) + 2 * N * D * 2 + N * N * 4 + D * 16 + N * 8


def slab_plan(Ns, D, budget, on_device=False):
    """consecutive whole problems per slab, greedily: a slab takes problems while its bytes stay within `budget` (and always one)"""
    slabs, cur, used = [], [], 0
    for u, N in enumerate(Ns):
        need = problem_bytes(N, D, on_device)
        if cur and used + need > budget:
            slabs.append(cur)
            cur, used = [], 0
        cur.append(u)
        used += need
    if cur:
        slabs.append(cur)
    return slabs


def split16(Z32):
    zh = Z32.astype(np.float16)
    zl = (Z32 - zh.astype(np.float32)).astype(np.float16)
    return zh.astype(np.float32), zl.astype(np.float32)


def gram32(zh, zl, defect=None, neighbour=None):
    """K = hh + hl + lh with fp32 accumulation, tiles on or above the diagonal, mirrored on store"""
    N = zh.shape[0]
    K = zh @ zh.T
    if defect != "hh_only":
        K = K + zh @ zl.T
        K = K + zl @ zh.T
    K = np.triu(K) + np.triu(K, 1).T                  # one value per pair: the stored matrix is exactly symmetric
    K = K.astype(np.float32)
    if defect == "no_mirror":                         # tiles below the diagonal never written (the scratch holds zeros)
        t = np.arange(N) // TILE
        K[t[:, None] > t[None, :]] = 0.0
    if defect == "row_overrun" and N % TILE:          # the tile rows behind the problem's end hold the neighbour's windows and are
        Np = (N + TILE - 1) // TILE * TILE            # stored unmasked into the compact [N][N] matrix: (r, c >= N) lands on (r + 1, c - N)
        nh, nl = neighbour
        ph = np.concatenate([zh, nh[:Np - N]])
        pl = np.concatenate([zl, nl[:Np - N]])
        Kp = (ph @ ph.T + ph @ pl.T + pl @ ph.T).astype(np.float32)
        flat = K.ravel().copy()
        r, c = np.meshgrid(np.arange(N), np.arange(N, Np), indexing="ij")
        at = (r * N + c).ravel()
        ok = at < N * N
        flat[at[ok]] = Kp[:N, N:].ravel()[ok]
        K = flat.reshape(N, N)
    return K


def loss32(y, f):
    return np.maximum(f, 0) + np.log1p(np.exp(-np.abs(f))) - y * f


def newton32(K, y, C, defect=None, eps_stop=EPS_STOP, trace=None):
    """the solver kernel: -> (a, b, iterations, res, converged)"""
    f32 = np.float32
    N = K.shape[0]
    C = f32(C)
    y = y.astype(f32)
    a = np.zeros(N, f32)
    b = f32(0)
    f = np.zeros(N, f32)

    def J_of(a, b, f):
        return float(C) * float(loss32(y, f).astype(np.float64).sum()) + 0.5 * float((a * (f - b)).astype(np.float64).sum())

    J = J_of(a, b, f)
    res, it = np.inf, 0
    for it in range(1, NEWTON_CAP + 1):
        p = sigmoid(f).astype(f32)
        g = p - y
        W = p * (f32(1) - p)
        S = np.sqrt(W)
        kt = K @ (C * g + a)
        rhs = [S * -kt, S.copy()]
        x = [np.zeros(N, f32), np.zeros(N, f32)]
        r = [rhs[0].copy(), rhs[1].copy()]
        d = [r[0].copy(), r[1].copy()]
        rr = [f32(r[0] @ r[0]), f32(r[1] @ r[1])]
        tol = [f32(CG_RTOL2) * rr[0], f32(CG_RTOL2) * rr[1]]
        for _ in range(cg_cap(N)):
            live = [rr[k] > tol[k] for k in range(2)]
            if not any(live):
                break
            for k in range(2):
                if not live[k]:
                    continue
                Ad = d[k] + C * S * (K @ (S * d[k]))
                dAd = f32(d[k] @ Ad)
                if not dAd > 0:
                    rr[k] = f32(0)
                    continue
                al = rr[k] / dAd
                x[k] = x[k] + al * d[k]
                r[k] = r[k] - al * Ad
                rn = f32(r[k] @ r[k])
                d[k] = r[k] + (rn / rr[k]) * d[k]
                rr[k] = rn
        num = f32((g + S * x[0]).sum())
        den = f32((S * x[1]).sum())
        if defect == "intercept_penalised":           # + 1/2 b^2 in the objective: C sum(g + W df) + b + db = 0
            db = -(C * num + b) / (C * den + f32(1))
        else:
            db = -num / den if den > 0 else f32(0)
        v = x[0] + db * x[1]
        an = -C * (g + S * v)
        da = an - a
        t = f32(1)
        fn = K @ an + (b + db)
        df = fn - f
        for h in range(MAX_HALVINGS + 1):
            a2, b2 = (an, b + db) if h == 0 else (a + t * da, b + t * db)
            f2 = fn if h == 0 else f + t * df
            J2 = J_of(a2, b2, f2) + (0.5 * float(b2) ** 2 - 0.5 * float(b) ** 2 if defect == "intercept_penalised" else 0.0)
            if J2 <= J + J_NOISE * abs(J) or h == MAX_HALVINGS:
                break
            t = t * f32(0.5)
        a, b, f = a2.astype(f32), f32(b2), f2.astype(f32)
        J = J_of(a, b, f)
        res = float(np.abs(a + C * (sigmoid(f).astype(f32) - y)).max() / C)
        if trace is not None:
            trace.append(res)
        if res <= eps_stop or defect == "one_step":
            break
    return a, b, it, res, bool(res <= eps_stop)


def fit32(X, y, C=1e-3, defect=None, neighbour=None, eps_stop=EPS_STOP, trace=None):
    """-> dict(w [D] fp32, bias fp32, iterations, res, converged).  neighbour: the windows of the next problem of the batch
    (row_overrun reads them)."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    N = X.shape[0]
    X64, mu, s = stats64(X, ddof=1 if defect == "ddof1" else 0, const_rule=defect != "no_const_rule")
    with np.errstate(all="ignore"):
        Z32 = ((X64 - mu) / s).astype(np.float32)
    zh, zl = split16(Z32)
    nb = None
    if defect == "row_overrun":
        n64, nmu, ns = stats64(neighbour)
        nb = split16(((n64 - nmu) / ns).astype(np.float32))
    with np.errstate(all="ignore"):
        K = gram32(zh, zl, defect, nb)
        a, b, it, res, conv = newton32(K, np.asarray(y), (1.0 / C) if defect == "c_on_regulariser" else C, defect, eps_stop, trace)
        if defect == "fp32_fold":
            w = ((zh + zl).T @ a) / s.astype(np.float32)
            bias = np.float32(b)
            for t in (w * mu.astype(np.float32)).astype(np.float32):
                bias = np.float32(bias - t)
        else:
            w = ((Z32.astype(np.float64).T @ a.astype(np.float64)) / s).astype(np.float32)
            bias = np.float32(float(b) - float((w.astype(np.float64) * mu).sum()))
    return dict(w=w.astype(np.float32), bias=np.float32(bias), iterations=it, res=res, converged=conv)


# ---- the case table ----------------------------------------------------------------------------------------------------------------
REGIMES = ("gauss", "dup", "sep", "imbal", "const", "embed")


def make_case(name, N, T, C, regime, seed, n_pos=None):
    """-> dict(name, X [N, T*96] fp32, y [N] uint8, held [128, T*96] fp32, C, T)"""
    r = np.random.default_rng(seed)
    D = T * 96
    n_pos = max(1, N // 3) if n_pos is None else n_pos
    X = r.normal(0, 4.0, (N, D)).astype(np.float32)
    held = r.normal(0, 4.0, (128, D)).astype(np.float32)
    y = np.zeros(N, np.uint8)
    y[:n_pos] = 1
    dirn = r.normal(0, 4.0, D).astype(np.float32)
    shift = {"sep": 3.0, "imbal": 0.5}.get(regime, 0.3)
    X[:n_pos] += shift * dirn
    held[:64] += shift * dirn
    if regime == "dup":                               # every window twice (and one three times): K is singular
        h = N // 2
        X[h:2 * h] = X[:h]
        y[h:2 * h] = y[:h]
        X[-1] = X[0]
        y[-1] = y[0]
        if y.min() == y.max():
            y[1] = 1 - y[0]
            if 1 + h < N:
                y[1 + h] = y[1]
    if regime == "const":
        X[:, 7] = -1.5
        held[:, 7] = -1.5
    if regime == "embed":                             # the shape of the embedding model's outputs: per-feature offsets far larger than
        off = r.normal(0, 40.0, D).astype(np.float32)             # the spread of a feature, spreads over two decades
        sd = np.exp(r.uniform(np.log(0.01), np.log(1.0), D)).astype(np.float32)
        X = (off + sd * X / 4).astype(np.float32)
        held = (off + sd * held / 4).astype(np.float32)
    perm = r.permutation(N)
    return dict(name=name, X=np.ascontiguousarray(X[perm]), y=np.ascontiguousarray(y[perm]), held=held, C=C, T=T, regime=regime)


def case_table(ring_T=34):
    """every N, T, C and regime of the table at least once; the named cases of DEFECT_CASE among them"""
    rows = [
        ("n2", 2, 1, 1e-3, "gauss", 1), ("n15", 15, 1, 0.1, "gauss", None), ("n16", 16, 16, 1e-3, "gauss", None),
        ("n17", 17, 16, 0.1, "gauss", None), ("n33", 33, 1, 1e-3, "dup", None), ("n64", 64, 16, 0.1, "sep", None),
        ("n65", 65, ring_T, 1e-3, "const", None), ("n65e", 65, 16, 0.1, "embed", None), ("n200", 200, 16, 1e-3, "imbal", 3),
        ("n200c", 200, 16, 0.1, "imbal", 3), ("n33e", 33, 16, 1e-3, "embed", None), ("n64d", 64, 16, 0.1, "dup", None),
        ("n1024", 1024, 16, 1e-3, "gauss", None), ("n17c", 17, ring_T, 0.1, "const", None), ("n200t1", 200, 1, 0.1, "gauss", None),
    ]
    return [make_case(nm, N, T, C, reg, 100 + i, n_pos) for i, (nm, N, T, C, reg, n_pos) in enumerate(rows)]


# the case that must show each defect (beyond 1e-4 in score)
DEFECT_CASE = {"ddof1": "n15", "no_const_rule": "n17c", "intercept_penalised": "n200c", "hh_only": "n200t1", "no_mirror": "n65e",
               "row_overrun": "n17", "c_on_regulariser": "n64", "fp32_fold": "n65e", "one_step": "n64"}


def sklearn_pipeline(X, y, C, tol=None):
    """the reference's pipeline (custom_verifier_model.py:95-113) on flattened windows -> folded (w, bias) in float64"""
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    kw = {} if tol is None else dict(tol=tol)
    pipe = make_pipeline(StandardScaler(), LogisticRegression(random_state=0, max_iter=20000 if tol else 2000, C=C, **kw))
    pipe.fit(X, np.asarray(y).astype(int))
    sc, lr = pipe[0], pipe[1]
    w = lr.coef_[0] / sc.scale_
    return w, lr.intercept_[0] - (lr.coef_[0] * sc.mean_ / sc.scale_).sum(), pipe


RING_T = 34                  # the feature ring of a handle that carries `timer` (weights.py: T = 34)


@functools.lru_cache(maxsize=None)
def table():
    return tuple(case_table(RING_T))


def case(name):
    return next(c for c in table() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per test run and shared: the float64 definition and the fp32 restatement of one case, their scores on the training
    plus the held-out windows, and the distance between the two"""
    c = case(name)
    A = np.concatenate([c["X"], c["held"]])
    w64, b64, it64, res64 = fit64(c["X"], c["y"], c["C"])
    o = fit32(c["X"], c["y"], c["C"])
    s64, s32 = scores(w64, b64, A), scores(o["w"], o["bias"], A)
    return dict(A=A, w64=w64, b64=b64, it64=it64, res64=res64, fit32=o, s64=s64, s32=s32, d32=float(np.abs(s32 - s64).max()))
