"""Shared by tests/test_head_windows_cpu.py and tests/test_head_windows_gpu.py: the head kernels over feature-window lengths T.

Every head kernel of the default family streams its first layer -- a GEMM with K = 96 T -- through an LDS weight ring of NBUF slots,
one k-step of 32 features at a time (owwhip_hx.h: heads_hx_kernel and, for the bank, heads_gemm1).  KST = 3 T k-steps run as
straight-line groups of NBUF while ks0 + NBUF - 1 + D < KST (D = NBUF - 1), then as conditional groups that end early when KST is no
multiple of NBUF.  Which of these shapes runs depends on T alone; the other head files move weights at T = 16 / 34.  This file holds
the window lengths, the head forms (so that one launch holds NN nets), the inputs, the float64 expectation, the one assertion the
device tests use, and a mirror of the host's launch rule that says which (NBUF, tail shape) a case reaches.  The mirror guards the
coverage of the case table; no expectation is computed from it.  HIP-free."""
import copy
import functools

import numpy as np

from oracle import oww_oracle as O
from openwakeword_amd import weights as W

from test_head_regimes import FP32_CAP, LOUD_ROW, N_ROWS, TOL_SCORE, ZERO_ROW          # noqa: F401  (the project's tolerances, not new ones)

T_EDGE = (1, 2, 3, 5, 7, 19, 22)     # KST = 3, 6, 9, 15, 21, 57, 66: both residues mod 2, residues 1, 2, 3 mod 4, both reachable ones mod 6
T_FULL = 16                          # KST = 48 = 0 mod 2, 4 and 6 (no T of T_EDGE is a multiple of 4): the whole-group shape, same inputs
T_MAX = 120                          # the ABI's longest fixed-head window; single-net forms and side cases only
T_ALL = T_EDGE + (T_FULL,)
SMALL_WGS_HEADS = 2 * 256            # owwhip.hip: kSmallLaunchWgs -- launches of at most this many workgroups run the deep ring
RNN_T = (1, 2, 63, 64)

_B = dict(kind="binary", n_out=1, layernorm=True)
# form -> use_mfma family, the shapes of its heads (weights.synthetic_head keywords; committed in this order), its window lengths,
# and for the forms of the MFMA ring kernels what pack_head_groups must make of one T's heads: hidden tiles per net and nets per launch
FORMS = {
    "narrow1": dict(fam=3, ht=4, nn=1, Ts=T_ALL + (T_MAX,), heads=[dict(_B, hidden=64)]),
    "narrow2": dict(fam=3, ht=4, nn=2, Ts=T_ALL, heads=[dict(_B, kind="gated", hidden=64)]),                 # (net 2 has role 1)
    "narrow3": dict(fam=3, ht=4, nn=3, Ts=T_ALL, heads=[dict(_B, kind="gated", hidden=32), dict(_B, hidden=64, layernorm=False)]),
    "narrow4": dict(fam=3, ht=4, nn=4, Ts=T_ALL, heads=[dict(_B, hidden=64), dict(_B, hidden=64, layernorm=False), dict(_B, hidden=32),
                                                        dict(_B, hidden=20, layernorm=False)]),
    "wide1": dict(fam=3, ht=8, nn=1, Ts=T_ALL + (T_MAX,), heads=[dict(_B, hidden=128)]),
    "wide2": dict(fam=3, ht=8, nn=2, Ts=T_ALL, heads=[dict(kind="multiclass", hidden=100, n_out=5, layernorm=False),
                                                      dict(_B, hidden=65, layernorm=False)]),
    # side cases: the exact-fp32 family's heads64_kernel, the generic kernel, the recurrent kernel
    "fp32_2x64": dict(fam=1, Ts=(1, 19, T_MAX), heads=[dict(_B, hidden=64), dict(_B, hidden=64, layernorm=False)]),
    "generic130": dict(fam=3, Ts=(T_MAX,), heads=[dict(_B, hidden=130)]),
    "rnn1": dict(fam=(3, 0), Ts=RNN_T, heads=[dict(kind="rnn", n_out=1)]),
    "rnn8": dict(fam=(3, 0), Ts=RNN_T, heads=[dict(kind="rnn", n_out=8)]),
}
RING_FORMS = tuple(f for f, spec in FORMS.items() if "nn" in spec)
# bank heads (one binary net each): hidden tiles -> shape; each at one wave per tile (37 subscribers) and at four (133)
BANK_FORMS = {"bank_ht4": dict(_B, hidden=64), "bank_ht8": dict(_B, hidden=128)}
BANK_SUBSCRIBERS = {1: 37, 4: 133}
BANK_RING = 25                       # the bank handle's feature ring: three rows more than the longest window of T_EDGE


# ------------------------------------------------------------------------------------------------ inputs and heads
@functools.lru_cache(maxsize=None)
def windows(T, n_rows=N_ROWS):
    """float32 [n_rows, T, 96]: N(0, 1), one all-zero window, one at 30 x the scale (fixed seed, read-only)."""
    ft = np.random.default_rng(4100 + T).normal(0.0, 1.0, (n_rows, T, 96)).astype(np.float32)
    ft[ZERO_ROW] = 0.0
    ft[LOUD_ROW] *= 30.0
    ft.setflags(write=False)
    return ft


def logits64(head, ft):
    """float64 logits [rows] of each sigmoid output of a head: (net,) / (net, net2) / (the recurrent head's single output,)."""
    if head["kind"] == "rnn":
        p = O.head_stage(ft, head, np.float64)[:, 0]
        return (np.log(p) - np.log1p(-p),)
    return tuple(O._mlp(np.asarray(ft, np.float64), head[k], np.float64)[:, 0] for k in ("net", "net2") if k in head)


def centre(head, ft):
    """A head with one sigmoid output gets each net's output bias moved by minus the median float64 logit over the windows `ft` (in
    place), the way test_head_regimes._bank_head_cached does it: a random head is pinned near 0 or 1 on most windows otherwise, and a
    comparison of scores that are all 1e-9 shows nothing.  Multi-output heads (softmax) are left alone; a gated head's first net is
    centred next to the median, see below."""
    if int(head["n_out"]) != 1:
        return head
    z = logits64(head, ft)
    if head["kind"] == "rnn":
        head["b_out"] = (head["b_out"] - np.float32(np.median(z[0]))).astype(np.float32)
        return head
    for k, zk in zip(("net", "net2"), z):
        c = np.median(zk)
        if head["kind"] == "gated" and k == "net":
            # the first net's score is the gate (> 0.5 hands over to the second net): a median row would sit ON the gate, where fp32 and
            # float64 already disagree.  The gate goes into the widest gap between neighbouring logits of the middle third of the rows.
            zs = np.sort(zk)
            lo, hi = len(zs) // 3, len(zs) - len(zs) // 3
            i = lo + int(np.argmax(np.diff(zs[lo:hi])))
            c = 0.5 * (zs[i] + zs[i + 1])
        head[k]["b3"] = (head[k]["b3"] - np.float32(c)).astype(np.float32)
    return head


GATE_MARGIN = 0.02                   # |logit| of the gating net nearest to the gate: 50 x what TOL_SCORE means for a logit at 0.5 (4e-4)


def draw_head(name, shape, T, seed=0):
    return W.synthetic_head(name, 5000 + 131 * T + seed, T=T, **shape)


@functools.lru_cache(maxsize=None)
def _form_heads(form, T):
    out = {}
    for i, shape in enumerate(FORMS[form]["heads"]):
        name = f"{form}_t{T}_{i}"
        out[name] = centre(draw_head(name, shape, T), windows(T))
    return out


def form_heads(form, T):
    """{name: head} of one (form, T), centred on windows(T); committed side by side they share one launch of NN nets."""
    return copy.deepcopy(_form_heads(form, T))


@functools.lru_cache(maxsize=None)
def _want(form, T, dtype):
    out = {}
    for n, h in _form_heads(form, T).items():
        with np.errstate(over="ignore"):                 # (fp32 exp(-z) of the 30 x window overflows to inf: the score is 0, as on the device)
            w = O.head_stage(windows(T), h, np.dtype(dtype).type).astype(np.float64)
        w.setflags(write=False)
        out[n] = w
    return out


def want(form, T, dtype=np.float64):
    """{name: [37, n_out]} of one (form, T) from the oracle in `dtype` (computed once, read-only)."""
    return _want(form, T, np.dtype(dtype).name)


def is_binary(head):
    return int(head["n_out"]) == 1


def mid_fraction(scores):
    """Share of scores in (0.05, 0.95): the condition that keeps a sigmoid comparison from being vacuous (>= 25 %)."""
    s = np.asarray(scores, np.float64)
    return float(((s > 0.05) & (s < 0.95)).mean())


MID_SHARE = 0.25


def kstep_fault(head, ks, variant):
    """A copy of a dense head whose first layer lost k-step ks (features 32 ks .. 32 ks + 31) the way a broken weight ring would lose
    it: "dropped" = the chunk never arrived (zero rows), "stale" = the slot still held the chunk of k-step ks - 1."""
    h = copy.deepcopy(head)
    for k in ("net", "net2"):
        if k in h:
            w1 = h[k]["w1"].copy()
            w1[32 * ks:32 * ks + 32] = 0.0 if variant == "dropped" else w1[32 * (ks - 1):32 * ks]
            h[k]["w1"] = w1
    return h


def fault_ksteps(T):
    KST = 3 * T
    return sorted({0, KST // 2, max(KST - 2, 0), KST - 1})


# ------------------------------------------------------------------------------------------------ the one assertion
def check_scores(label, got, ref, range_flag, worst=None):
    """Every score finite, within TOL_SCORE of float64, the range flag down.  Prints and returns the worst |score - float64|; `worst`
    (a one-element list) keeps the maximum over a test's calls."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{label}: {got.shape} against {ref.shape}"
    assert np.isfinite(got).all(), f"{label}: non-finite score {got[~np.isfinite(got)][:4]}"
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    print(f"\n{label}: max |score - float64| = {err:.2e}")
    if worst is not None:
        worst[0] = max(worst[0], err)
    assert err <= TOL_SCORE, f"{label}: {err:.3e} from float64 at {np.unravel_index(int(np.argmax(np.abs(got - ref))), got.shape)}"
    assert not range_flag, f"{label}: the range flag is up"
    return err


# ------------------------------------------------------------------------------------------------ mirror of the host's launch rule
def head_groups(heads):
    """owwhip_pack.h::pack_head_groups for the default family: [{T, ht, names, n_nets}] of the MFMA ring launches of `heads` in commit
    order, plus the names left to the generic and recurrent kernels."""
    groups, other = [], []
    for name, h in heads.items():
        if h["kind"] == "rnn":
            other.append(name)
            continue
        nets = 2 if h["kind"] == "gated" else 1
        one_block = len(W.net_blocks(h["net"])) == 1
        fast = h["hidden"] <= 64 and h["n_out"] == 1 and h["kind"] != "multiclass" and one_block
        wide = not fast and nets == 1 and h["hidden"] <= 128 and h["n_out"] <= 8 and one_block
        if not fast and not wide:
            other.append(name)
            continue
        ht = 8 if wide else 4
        g = next((g for g in groups if g["T"] == h["T"] and g["ht"] == ht and g["n_nets"] + nets <= 16 // ht), None)
        if g is None:
            g = dict(T=h["T"], ht=ht, names=[], n_nets=0)
            groups.append(g)
        g["names"].append(name)
        g["n_nets"] += nets
    return groups, other


def heads_nbuf(ht, n_nets, n_rows, small_wgs_heads=SMALL_WGS_HEADS):
    """owwhip.hip::run_heads: the weight-ring depth of one group's launch over n_rows stream positions."""
    deep = (n_rows + 127) // 128 <= small_wgs_heads
    nn = min(n_nets, 4)
    if not deep:
        return 2                                         # HX_NBUF
    if ht == 8:
        return 6 if nn == 1 else 4                       # HeadsDeep<2> / HeadsDeep<4>
    return 6 if nn <= 2 else 4                           # HeadsDeep<NN>


def bank_waves(n_entries, n_groups):
    """owwhip_bank_host.h::route (owb): waves per tile of one width class (the bank kernel's ring always has two slots)."""
    return 4 if n_groups > 0 and n_entries >= 96 * n_groups else 1


BANK_NBUF = 2


def tail_shape(T, nbuf):
    """What the k loop of heads_hx_kernel / heads_gemm1 does with KST = 3 T k-steps on a ring of nbuf slots."""
    KST, D = 3 * T, nbuf - 1
    n_main = 0
    while n_main * nbuf + nbuf - 1 + D < KST:
        n_main += 1
    rest = KST - n_main * nbuf
    return dict(KST=KST, NBUF=nbuf, mod=KST % nbuf, main_groups=n_main, tail_groups=-(-rest // nbuf), partial=rest % nbuf,
                prologue=min(D, KST), kst_le_d=KST <= D, empty_main=n_main == 0, main_then_partial=n_main >= 1 and rest % nbuf != 0)


def reachable_residues(nbuf):
    return sorted({(3 * T) % nbuf for T in range(1, T_MAX + 1)})


def ring_cases():
    """Every (form, T, ring pin) the device tier runs on the MFMA ring kernels -> [(label, tail_shape)], through the mirror."""
    out = []
    for form in RING_FORMS:
        spec = FORMS[form]
        for T in spec["Ts"]:
            groups, other = head_groups(_form_heads(form, T))
            assert not other and len(groups) == 1, (form, T, groups, other)
            g = groups[0]
            assert (g["ht"], g["n_nets"]) == (spec["ht"], spec["nn"]), (form, T, g)
            for pin, small in (("default", SMALL_WGS_HEADS), ("two-slot", 0)):
                out.append((f"{form} T={T} {pin}", tail_shape(T, heads_nbuf(g["ht"], g["n_nets"], N_ROWS, small))))
    for form in BANK_FORMS:
        for waves, n_sub in BANK_SUBSCRIBERS.items():
            assert bank_waves(n_sub * len(T_EDGE), len(T_EDGE)) == waves      # (every stream subscribed to one head per T)
            for T in T_EDGE:
                out.append((f"{form} T={T} waves={waves}", dict(tail_shape(T, BANK_NBUF), waves=waves)))
    return out


def bank_head(form, T, ft=None):
    """The bank head of (form, T); with `ft` ([rows, T, 96], the windows it will meet) centred on them."""
    h = draw_head(f"{form}_t{T}", BANK_FORMS[form], T, seed=7)
    return h if ft is None else centre(h, ft)
