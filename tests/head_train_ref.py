"""The case module of the head-training tests (no GPU): the step of train.py:434-510 for the network of train.py:66-83 (n_blocks = 1,
n_classes = 1) restated in numpy, the case table, and the reference's own class run on the same batches.

  ref_train(case, np.float64)                 -- `ref64`: the definition, in double.
  ref_train(case, np.float32, order=0..3)     -- `ref32`: the same arithmetic in fp32 with the kernels' placement of the 1 / (m acc)
                                                 scale (behind the sums), under four summation orders of its reductions (the input axis
                                                 of X W1 and the batch axis of every gradient sum: natural, reversed, tiles of 64 rows
                                                 summed tile by tile as the kernels do, a fixed shuffle), with switchable defects.
  run_reference(case, double=False)           -- train.Model.train_model itself, imported from the reference checkout with stand-in
                                                 modules for its training-only imports (None where the checkout is absent).
"""
from __future__ import annotations

import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np

from openwakeword_amd import train as T_

REFERENCE = os.environ.get("OWW_REFERENCE_DIR", "/root/reference")      # (as tests/test_golden_reproducible.py finds it)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_train.npz")
EPS_LN = 1e-5
DEFECTS = ("bias_k", "eps_in_sqrt", "mean_n", "negw_on_pos", "acc_not_divided", "acc_not_reset", "p_minus_y", "ln_no_means",
           "relu_prenorm", "pad_not_zeroed", "empty_slot_read", "negw_by_opt", "idx_problem0", "moments_frozen_lr0")


# ---------------------------------------------------------------------------------------------------------------- the case table
def schedule(K):
    """(lr [K] float64, neg_weight [K] float32, warmup, hold, total): the reference's own schedule (train.py:167-190) of a run of K + 2
    steps cut after K, target 1e-3: lr[0] = 0 in every case (the first warm-up step); the weights ramp 1 -> 1500 (train.py:274)."""
    warm, hold, total = max(1, K // 5), K // 3, K + 2
    lr = np.array([float(T_.lr_warmup_cosine_decay(k, warm, hold, total, target_lr=1e-3)) for k in range(K)], np.float64)
    nw = np.linspace(1, 1500, K).astype(np.float32) if K > 1 else np.ones(1, np.float32)
    return lr, nw, warm, hold, total


def _pool(r, P, T, shift=1.0):
    lab = (np.arange(P) % 2).astype(np.uint8)
    d = r.normal(size=(T, 96)) / np.sqrt(T * 96.0)
    x = r.normal(size=(P, T, 96)) + shift * 6.0 * (lab[:, None, None] * 2.0 - 1.0) * d
    return x.astype(np.float32), lab


#        name                     D    T   n    K   U  regime
TABLE = [("fresh_n33",            32,  1,  33,  12, 1, "fresh"),          # kept < 128: accumulate, skip, fire every fourth step
         ("fresh_u3",             16,  2,  129, 12, 3, "fresh"),          # per-problem tables
         ("fresh_d128",           128, 1,  300, 2,  1, "fresh"),
         ("fresh_k1",             16,  1,  128, 1,  1, "fresh"),          # lr = 0 alone: only moments and the count move
         ("trained_k12",          32,  2,  129, 12, 1, "trained"),        # output layer x 8: selection drops confident samples
         ("alldrop",              32,  1,  128, 12, 1, "alldrop"),        # m = 0 for the first steps
         ("accum_n127",           32,  2,  127, 12, 1, "fresh"),          # one short of the threshold: fires every second step
         ("saturated",            16,  1,  128, 2,  1, "saturated"),      # one kept negative at p = 1.0f exactly
         ("dead_relu",            16,  1,  128, 12, 1, "dead"),
         ("empty_dup",            32,  1,  300, 12, 1, "empty_dup"),      # -1 slots and duplicated indices
         ("single_n1",            16,  1,  1,   40, 1, "fresh"),          # never reaches 128 in 40 steps
         ("ramp_k40",             32,  2,  128, 40, 1, "fresh"),
         ("faint_pos",            16,  1,  128, 2,  1, "faint"),          # gradients near Adam's eps: positives kept at p = 0.998
         ("t16_u3",               32,  16, 300, 12, 3, "fresh"),
         ("t16_d128",             128, 16, 129, 2,  1, "fresh"),
         ("fresh_d48",            48,  1,  129, 2,  1, "fresh"),          # hidden sizes between the issue's: the other template instances,
         ("fresh_d112",           112, 1,  129, 2,  1, "fresh")]          # D no power of two; D = 112 the largest register footprint
# generator seeds moved off their default where the default draws a sample inside the selection margin (test_head_train_cpu.py: P_MARGIN)
SALT = {"trained_k12": 30}
GOLDEN_CASES = [t[0] for t in TABLE if t[2] <= 2]
SATURATION = "saturated"


def make_case(name):
    _, D, T, n, K, U, regime = next(t for t in TABLE if t[0] == name)
    seed = [t[0] for t in TABLE].index(name)
    r = np.random.default_rng(1000 + seed + 100 * SALT.get(name, 0))
    P = 600 if n >= 128 else 200
    pool, lab = _pool(r, P, T)
    idx = r.integers(0, P, size=(U, K, n)).astype(np.int32)
    init = [T_.init_head(T, D, 77 + seed * 8 + u) for u in range(U)]
    if regime == "trained":
        for hd in init:
            hd["net"]["w3"] *= 8
            hd["net"]["b3"] *= 8
    if regime == "dead":
        for hd in init:
            hd["net"]["ln1"][1][3] = -10.0          # |xhat| <= sqrt(D - 1) < 4: unit 3 never fires
    if regime == "empty_dup":
        idx[:, :, ::7] = -1
        idx[:, :, 1::5] = idx[:, :, 2::5][:, :, :idx[:, :, 1::5].shape[2]]
    y = np.where(idx >= 0, lab[np.maximum(idx, 0)], 0).astype(np.uint8)
    if regime == "alldrop":
        for hd in init:
            hd["net"]["b3"][:] = -20.0              # p < 0.001 on everything: negatives are dropped, positives kept
        neg = np.flatnonzero(lab == 0)
        idx[:, :5] = neg[r.integers(0, neg.size, size=(U, 5, n))]
        y = lab[idx].astype(np.uint8)
    if regime == "faint":
        pos = np.flatnonzero(lab == 1)
        idx = pos[r.integers(0, pos.size, size=(U, K, n))].astype(np.int32)
        y = np.ones_like(idx, dtype=np.uint8)
        for hd in init:                             # every logit within a few hundredths of 6.2: kept, with a gradient of 1e-5 at the logit
            hd["net"]["w3"] *= np.float32(0.1)
            P_ = unpack(T_.head_to_record(hd), T, D, np.float32)
            hd["net"]["b3"][:] += np.float32(6.2 - forward(P_, pool.reshape(P, -1)[pos], np.float32)["lg"].mean())
    lr, nw, warm, hold, total = schedule(K)
    case = dict(name=name, D=D, T=T, n=n, K=K, U=U, regime=regime, pool=pool, idx=idx, y=y, lr=lr, nw=nw, warm=warm, hold=hold, total=total,
                init=np.stack([T_.head_to_record(hd) for hd in init]), probe=r.integers(0, P, size=64))
    if regime == "saturated":
        _saturate(case)
    return case


def _saturate(case):
    """Stretch the output layer and move b3 so that exactly one pool window sits at logit 18 in fp32 (p = 1.0f; its 1 - p is 0) and every
    other at most at 16 (p < 1); that window, labelled 0, goes into slot 0 of every batch."""
    P_ = unpack(case["init"][0], case["T"], case["D"], np.float32)
    X = case["pool"].reshape(case["pool"].shape[0], -1)
    P_["w3"] = P_["w3"] * np.float32(30)
    lg = forward(P_, X, np.float32)["lg"]
    order = np.argsort(lg)
    top = order[-1]
    rest = np.flatnonzero(lg <= lg[top] - 2.5)              # the batches draw from these alone: nothing else comes near saturation
    assert rest.size > 100
    P_["b3"] = P_["b3"] + np.float32(18.0 - lg[top])
    case["init"][0] = np.concatenate([P_[f].ravel() for f in T_.FIELDS]).astype(np.float32)
    case["idx"] = rest[np.random.default_rng(3).integers(0, rest.size, size=case["idx"].shape)].astype(np.int32)
    case["idx"][:, :, 0] = top
    case["y"] = (np.arange(case["pool"].shape[0]) % 2).astype(np.uint8)[case["idx"]]
    case["y"][:, :, 0] = 0
    case["sat_row"] = int(top)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def unpack(rec, T, D, dtype):
    out, o = {}, 0
    for name, shape in T_.record_shapes(T, D):
        n = int(np.prod(shape))
        out[name] = np.asarray(rec[o:o + n], dtype=dtype).reshape(shape if name not in ("w3",) else (D,)).copy()
        o += n
    return out


def _ln(z, g, b, dt):
    mu = z.mean(axis=1, keepdims=True, dtype=dt)
    zc = z - mu
    var = (zc * zc).mean(axis=1, keepdims=True, dtype=dt)
    rstd = dt(1) / np.sqrt(var + dt(EPS_LN))
    xh = zc * rstd
    return xh, rstd, xh * g + b


def forward(P_, X, dt, perm=None):
    X = X.astype(dt)
    z1 = (X @ P_["w1"] if perm is None else X[:, perm] @ P_["w1"][perm]) + P_["b1"]
    xh1, rstd1, a1 = _ln(z1, P_["g1"], P_["be1"], dt)
    h1 = np.maximum(a1, dt(0))
    z2 = h1 @ P_["w2"] + P_["b2"]
    xh2, rstd2, a2 = _ln(z2, P_["g2"], P_["be2"], dt)
    h2 = np.maximum(a2, dt(0))
    lg = h2 @ P_["w3"] + P_["b3"][0]
    p = dt(1) / (dt(1) + np.exp(-lg))
    return dict(z1=z1, xh1=xh1, rstd1=rstd1, a1=a1, h1=h1, z2=z2, xh2=xh2, rstd2=rstd2, a2=a2, h2=h2, lg=lg, p=p)


def score(rec, case, dt=np.float64):
    """p of the 64 probe windows under a flat record."""
    X = case["pool"].reshape(case["pool"].shape[0], -1)[case["probe"]]
    return forward(unpack(rec, case["T"], case["D"], dt), X, dt)["p"]


def _bsum(a, order, rng_perm):
    """sum over axis 0 (the batch) in one of the four orders"""
    if order == 0 or a.shape[0] == 0:
        return a.sum(axis=0, dtype=a.dtype)
    if order == 1:
        return a[::-1].sum(axis=0, dtype=a.dtype)
    if order == 2:
        s = np.zeros(a.shape[1:], a.dtype)
        for t in range(0, a.shape[0], 64):
            s = s + a[t:t + 64].sum(axis=0, dtype=a.dtype)
        return s
    return a[rng_perm].sum(axis=0, dtype=a.dtype)


def ref_train(case, dtype=np.float64, order=0, defects=()):
    """-> dict(params [U, n_params] (dtype), loss [U, K] float64 with NaN where no step, kept [U, K], sets: per (u, k) the bool kept mask over
    the batch's valid slots, p: per (u, k) the scores of the valid slots, steps [U, K] bool)."""
    dt = dtype
    defects = frozenset(defects)
    assert defects <= set(DEFECTS)
    T, D, K, U = case["T"], case["D"], case["K"], case["U"]
    pool = case["pool"].reshape(case["pool"].shape[0], -1)
    F = pool.shape[1]
    shuffle = np.random.default_rng(5)
    fperm = {0: None, 1: np.arange(F)[::-1], 2: None, 3: shuffle.permutation(F)}[order] if dt == np.float32 else None
    out_p, loss, kept_n, sets, ps, stepped = [], np.full((U, K), np.nan), np.zeros((U, K), np.int64), {}, {}, np.zeros((U, K), bool)
    for u in range(U):
        P_ = unpack(case["init"][u], T, D, dt)
        M = {k: np.zeros_like(v) for k, v in P_.items()}
        V = {k: np.zeros_like(v) for k, v in P_.items()}
        acc_steps, acc_samples, opt = 1, 0, 0
        ut = 0 if "idx_problem0" in defects else u
        for k in range(K):
            ix, yy = case["idx"][ut, k], case["y"][ut, k]
            valid = ix >= 0
            if "empty_slot_read" in defects:                     # an empty slot (-1) read as pool row 0 with label 0
                ix, valid = np.maximum(ix, 0), np.ones_like(valid)
                yy = np.where(case["idx"][ut, k] >= 0, yy, 0)
            X = pool[ix[valid]].astype(dt)
            y = yy[valid].astype(dt)
            if "pad_not_zeroed" in defects:                      # the padding rows of the last 64-row tile taking part: all-zero inputs
                n_padding = -len(ix) % 64                        # (the forward pass sees b1 alone), label 0, through selection like any row
                X = np.concatenate([X, np.zeros((n_padding, F), dt)])
                y = np.concatenate([y, np.zeros(n_padding, dt)])
            fw = forward(P_, X, dt, fperm)
            p = fw["p"]
            sel = ((y == 0) & (p >= dt(0.001))) | ((y == 1) & (p < dt(0.999)))
            m = int(sel.sum())
            sets[u, k], ps[u, k], kept_n[u, k] = sel, p, m
            if m == 0:
                continue
            acc_samples += m
            if acc_samples < 128:
                acc_steps += 1
                continue
            nwk = dt(case["nw"][opt if "negw_by_opt" in defects else k])
            w = np.where(y == 1, dt(1), nwk) if "negw_on_pos" not in defects else np.full_like(y, nwk)
            with np.errstate(divide="ignore"):                   # log(0) = -inf is clamped to -100, as binary_cross_entropy does
                bce = -(y * np.maximum(np.log(p), dt(-100)) + (1 - y) * np.maximum(np.log1p(-p), dt(-100)))
            denom_m = dt(int(valid.sum()) if "mean_n" in defects else m)
            accd = dt(1 if "acc_not_divided" in defects else acc_steps)
            loss[u, k] = float((w * bce)[sel].sum(dtype=dt) / denom_m / accd)
            sp = (dt(1) - p) * p
            g = np.where(sel, (p - y) / np.maximum(sp, dt(1e-12)) * w * sp, dt(0))
            if "p_minus_y" in defects:
                g = np.where(sel, (p - y) * w, dt(0))
            scale = dt(1) / accd / denom_m
            if dt == np.float64:
                g, scale = g * scale, dt(1)                      # the definition scales at the logit, as autograd does
            g = g[:, None]
            perm = shuffle.permutation(len(y)) if order == 3 else None
            bs = lambda a: _bsum(a, order if dt == np.float32 else 0, perm) * scale      # noqa: E731
            G = {}
            G["w3"] = bs(g * fw["h2"])
            G["b3"] = bs(g).reshape(1)
            gate2 = (fw["z2"] > 0) if "relu_prenorm" in defects else (fw["a2"] > 0)
            da2 = np.where(gate2, g * P_["w3"][None, :], dt(0))
            G["g2"], G["be2"] = bs(da2 * fw["xh2"]), bs(da2)
            dxh = da2 * P_["g2"]
            if "ln_no_means" in defects:
                dz2 = fw["rstd2"] * dxh
            else:
                dz2 = fw["rstd2"] * (dxh - dxh.mean(axis=1, keepdims=True, dtype=dt) - fw["xh2"] * (dxh * fw["xh2"]).mean(axis=1, keepdims=True, dtype=dt))
            G["b2"] = bs(dz2)
            G["w2"] = _mm_t(fw["h1"], dz2, order if dt == np.float32 else 0, perm) * scale
            gate1 = (fw["z1"] > 0) if "relu_prenorm" in defects else (fw["a1"] > 0)
            da1 = np.where(gate1, dz2 @ P_["w2"].T, dt(0))
            G["g1"], G["be1"] = bs(da1 * fw["xh1"]), bs(da1)
            dxh = da1 * P_["g1"]
            if "ln_no_means" in defects:
                dz1 = fw["rstd1"] * dxh
            else:
                dz1 = fw["rstd1"] * (dxh - dxh.mean(axis=1, keepdims=True, dtype=dt) - fw["xh1"] * (dxh * fw["xh1"]).mean(axis=1, keepdims=True, dtype=dt))
            G["b1"] = bs(dz1)
            G["w1"] = _mm_t(X, dz1, order if dt == np.float32 else 0, perm) * scale
            lr = case["lr"][k]
            if not ("moments_frozen_lr0" in defects and lr == 0):
                opt += 1
                t = k + 1 if "bias_k" in defects else opt
                step_size = dt(lr / (1.0 - 0.9 ** t))
                bc2 = 1.0 - 0.999 ** t
                for f in T_.FIELDS:
                    M[f] = M[f] + (G[f] - M[f]) * dt(1.0 - 0.9)
                    V[f] = V[f] * dt(0.999) + dt(1.0 - 0.999) * G[f] * G[f]
                    den = np.sqrt(V[f] / dt(bc2) + dt(1e-8)) if "eps_in_sqrt" in defects else np.sqrt(V[f]) / dt(np.sqrt(bc2)) + dt(1e-8)
                    P_[f] = P_[f] + (-step_size * M[f]) / den
            stepped[u, k] = True
            if "acc_not_reset" not in defects:
                acc_steps = 1
            acc_samples = 0
        out_p.append(np.concatenate([P_[f].ravel() for f in T_.FIELDS]))
    return dict(params=np.stack(out_p), loss=loss, kept=kept_n, sets=sets, p=ps, steps=stepped)


def _mm_t(A, B, order, perm):
    """A^T B with the batch (axis 0 of both) summed in one of the four orders"""
    if order == 0:
        return A.T @ B
    if order == 1:
        return A[::-1].T @ B[::-1]
    if order == 2:
        s = np.zeros((A.shape[1], B.shape[1]), A.dtype)
        for t in range(0, A.shape[0], 64):
            s = s + A[t:t + 64].T @ B[t:t + 64]
        return s
    return A[perm].T @ B[perm]


def rel_param_error(a, b, case):
    """the largest, over the record's tensors, of max |a - b| / max |b|"""
    worst, o = 0.0, 0
    for _, shape in T_.record_shapes(case["T"], case["D"]):
        n = int(np.prod(shape))
        x, y = np.asarray(a[o:o + n], np.float64), np.asarray(b[o:o + n], np.float64)
        worst = max(worst, float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30)))
        o += n
    return worst


def same_decisions(r1, r2):
    return np.array_equal(r1["kept"], r2["kept"]) and np.array_equal(r1["steps"], r2["steps"]) and \
        all(np.array_equal(r1["sets"][k], r2["sets"][k]) for k in r1["sets"])


# ---------------------------------------------------------------------------------------------------------------- the reference's class
class _Stub(types.ModuleType):
    """a stand-in for a module the reference imports for training data only"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Dummy


class _Dummy:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        import torch
        return torch.zeros(())

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Dummy()


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    NAMES = ("torchinfo", "torchmetrics", "speechbrain", "audiomentations", "torch_audiomentations", "onnxruntime", "mutagen", "acoustics",
             "pronouncing", "onnx", "tflite_runtime", "onnx_tf", "tensorflow", "webrtcvad", "pyaudio", "deep_phonemizer", "dp", "torchaudio",
             "librosa", "soundfile", "resampy", "numba")

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in self.NAMES:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


_train_mod = None


def reference_train_module():
    """openwakeword.train of the reference checkout, or None where it is absent"""
    global _train_mod
    if _train_mod is not None:
        return _train_mod
    if not os.path.isfile(os.path.join(REFERENCE, "openwakeword", "train.py")):
        return None
    finder = _StubFinder()
    before = set(sys.modules)
    sys.meta_path.append(finder)            # behind the real finders: only what is missing is stood in for
    sys.path.insert(0, REFERENCE)
    try:
        import openwakeword.train as tr
    finally:
        # leave the process as it was: no stand-in and no half-real `openwakeword` package stays importable for other tests (the
        # module object in hand keeps working: its globals are bound)
        sys.path.remove(REFERENCE)
        sys.meta_path.remove(finder)
        for name in set(sys.modules) - before:
            if isinstance(sys.modules[name], _Stub) or name.split(".")[0] == "openwakeword":
                del sys.modules[name]
    _train_mod = tr
    return tr


def run_reference(case, double=False):
    """train.Model.train_model on the case's batches -> the dict ref_train returns (None where the reference is absent)."""
    tr = reference_train_module()
    if tr is None:
        return None
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(1)
    tdt = torch.float64 if double else torch.float32
    T, D, K, U = case["T"], case["D"], case["K"], case["U"]
    out_p, loss, kept_n, sets, ps, stepped = [], np.full((U, K), np.nan), np.zeros((U, K), np.int64), {}, {}, np.zeros((U, K), bool)
    for u in range(U):
        model = tr.Model(n_classes=1, input_shape=(T, 96), model_type="dnn", layer_dim=D, n_blocks=1)
        model.device = torch.device("cpu")
        P_ = unpack(case["init"][u], T, D, np.float64)
        net = model.model
        with torch.no_grad():
            for lin, w, b in ((net.layer1, "w1", "b1"), (net.blocks[0].fcn_layer, "w2", "b2"), (net.last_layer, "w3", "b3")):
                lin.weight.copy_(torch.from_numpy(P_[w].reshape(-1, lin.weight.shape[0]).T.copy()))
                lin.bias.copy_(torch.from_numpy(P_[b]))
            for ln, g, b in ((net.layernorm1, "g1", "be1"), (net.blocks[0].layer_norm, "g2", "be2")):
                ln.weight.copy_(torch.from_numpy(P_[g]))
                ln.bias.copy_(torch.from_numpy(P_[b]))
        if double:
            net.double()
            bce = model.loss
            model.loss = lambda p, t, w, _f=bce: _f(p, t.to(p.dtype), w.to(p.dtype))
        model.optimizer = torch.optim.Adam(net.parameters(), lr=0.0001)
        batches, ys, seen = [], [], []
        for k in range(K):
            valid = case["idx"][u, k] >= 0
            ix = case["idx"][u, k][valid]
            batches.append((torch.from_numpy(case["pool"][ix]).to(tdt), torch.from_numpy(case["y"][u, k][valid].astype(np.int64))))
        hook = net.register_forward_hook(lambda mod, i, o: seen.append(o.detach().squeeze(-1).clone()))
        hist0 = 0
        # one step at a time, so that a step's loss can be told from the next one's; the state lives in the model and the optimizer, the
        # accumulation counters are train_model's locals, so the whole run is ONE call and the losses are assigned afterwards
        model.train_model(batches, max_steps=case["total"], warmup_steps=case["warm"], hold_steps=case["hold"],
                          negative_weight_schedule=[float(v) for v in case["nw"]], val_steps=[], lr=1e-3)
        hook.remove()
        acc_samples = 0
        losses = [float(v) for v in model.history["loss"]]
        for k in range(K):
            p = seen[k].numpy()
            y = batches[k][1].numpy()
            pt = seen[k]
            sel = (((batches[k][1] == 0) & (pt >= 0.001)) | ((batches[k][1] == 1) & (pt < 0.999))).numpy()
            sets[u, k], ps[u, k], kept_n[u, k] = sel, p.astype(np.float64), int(sel.sum())
            if sel.sum() == 0:
                continue
            acc_samples += int(sel.sum())
            if acc_samples >= 128:
                stepped[u, k], acc_samples = True, 0
                loss[u, k] = losses[hist0]
                hist0 += 1
        assert hist0 == len(losses), "the reference stepped where the counters say it should not"
        rec = {}
        for lin, w, b in ((net.layer1, "w1", "b1"), (net.blocks[0].fcn_layer, "w2", "b2"), (net.last_layer, "w3", "b3")):
            rec[w], rec[b] = lin.weight.detach().numpy().T.copy(), lin.bias.detach().numpy().copy()
        for ln, g, b in ((net.layernorm1, "g1", "be1"), (net.blocks[0].layer_norm, "g2", "be2")):
            rec[g], rec[b] = ln.weight.detach().numpy().copy(), ln.bias.detach().numpy().copy()
        out_p.append(np.concatenate([rec[f].ravel() for f in T_.FIELDS]))
    return dict(params=np.stack(out_p), loss=loss, kept=kept_n, sets=sets, p=ps, steps=stepped)
