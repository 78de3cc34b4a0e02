"""Both log-mel front ends -- owk::mel_kernel (openwakeword_amd/csrc/owwhip_kernels.h) and the mel phase of owf::hmelA_kernel
(owwhip_fused.h) -- against float64 over the signal regimes and the level-aware budget of tests/mel_budget.py.

Every comparison is |device - float64| <= T0 + T1 * 10^((D - 80) / 20) per value, D = R_pair - u from float64 alone (dB; a tenth of
it for the streaming rows in mel units).  T0, T1 and the regimes are frozen in tests/mel_budget.py and justified on the CPU by
tests/test_mel_budget_cpu.py; nothing here is fitted to a device result.  Each test prints its worst error / budget ratio per regime
(DESIGN.md records them).  int16 input cannot overflow the fp32 power ((32768 * 200)^2 = 4e13), so no regime may be refused:
range_status() stays False throughout."""
import functools

import numpy as np
import pytest
import torch

import mel_budget as MB
from openwakeword_amd import weights as W
from openwakeword_amd.engine import StreamEngine

pytestmark = pytest.mark.gpu
REG = MB.REGIMES
NR = len(REG)
N_SHORT = 1999                   # ten frames: a partial second 8-frame group, and rows of a stacked call that are not 16-byte aligned
STEPS = (1, 1, 1, 1)
QUIET, LOUD = "tone440_quiet", "noise12000"


def _engine(n_streams, **kw):
    return StreamEngine(n_streams, {"alexa": W.synthetic_head("alexa", 1234)}, W.synthetic_embedding(1234), debug_layers=True, **kw)


@pytest.fixture(scope="module")
def eng_rr():
    """Exact-fp32 family: every step takes the separate mel kernel."""
    e = _engine(13, use_mfma=1)
    yield e
    assert e.range_status() is False
    e.close()


@pytest.fixture(scope="module")
def eng_default():
    """Default family: one-chunk steps take the fused kernel, longer calls the separate one (in slices beyond two chunks)."""
    e = _engine(13, max_chunks=2)
    yield e
    assert e.range_status() is False
    e.close()


@functools.lru_cache(maxsize=None)
def _stream_ref(name, calls=STEPS):
    return MB.stream_reference(MB.regimes()[name], calls)


def _run_calls(eng, names, calls=STEPS):
    """Reset, then feed row s the regime names[s] in calls of `calls` chunks -> per call the rows oww_get_mel still reaches,
    float32 [S, rows, 32] (8 rows per chunk; after a call evaluated in slices only the last slice's)."""
    S = eng.n_streams
    assert len(names) == S
    regs = MB.regimes()
    eng.reset()
    out, pos = [], 0
    for k in calls:
        eng.step(np.stack([regs[n][pos:pos + k * 1280] for n in names]))
        pos += k * 1280
        k_last = k if k <= eng.max_chunks else (k % eng.max_chunks or eng.max_chunks)
        out.append(np.stack([eng.get_mel(s, 8 * k_last) for s in range(S)]))
    return out


def _check_stream_rows(got_calls, name, calls=STEPS):
    """Rows [rows, 32] per call of ONE stream fed regime `name` -> worst error / budget; finite everywhere."""
    worst = 0.0
    for i, (got, ref) in enumerate(zip(got_calls, _stream_ref(name, calls))):
        assert np.isfinite(got).all(), f"{name} call {i}: non-finite mel rows"
        rows = got.shape[0]
        part = MB.Ref(ref.clamped[:, -rows:], ref.u[:, -rows:], ref.budget[:, -rows:], ref.R[:, -rows:], ref.floor)
        if i == 0 and rows == ref.clamped.shape[1]:
            assert (got[:3] == 1.0).all(), f"{name}: the first three rows after a reset read 1.0"
        worst = max(worst, MB.worst_ratio(got[None], part))
        if name in MB.LEAKAGE:
            assert part.R.max() - (float(got[got != 1.0].max()) - 2.0) * 10.0 >= 80.0, f"{name} call {i}: energy invented inside the bank"
    return worst


def _report(title, ratios):
    print(f"\n{title}: worst |device - float64| / budget per regime")
    for name in REG:
        if name in ratios:
            print(f"    {name:16s} {ratios[name]:.3f}")
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{title}: over budget: {bad}"


# ------------------------------------------------------------------------------------------------ clip mode
@pytest.mark.parametrize("name", REG)
def test_clip_mode_meets_the_budget(eng_rr, name):
    """oww_mel, one call per regime and length.  The 1,999-sample call stacks the regime twice: the second row is not 16-byte
    aligned and takes the scalar fetch path, and must give the first row's bits."""
    x = MB.regimes()[name]
    ratios = []
    for n, B in ((MB.N_CLIP, 1), (N_SHORT, 2)):
        pcm = np.repeat(x[None, :n], B, axis=0)
        got = eng_rr.mel(pcm)
        ref = MB.reference(pcm)
        assert got.shape == ref.clamped.shape and np.isfinite(got).all()
        if B == 2:
            assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "aligned and unaligned rows differ on the same samples"
        ratios.append(MB.worst_ratio(got, ref))
        if name in MB.LEAKAGE:
            below = float(ref.R.max() - got.max())
            print(f"\n{name} n = {n}: call maximum {below:.1f} dB below R")
            assert below >= 80.0, "energy invented inside the bank"
    print(f"\n{name}: clip mode, worst |device - float64| / budget = {ratios[0]:.3f} (n = {MB.N_CLIP}), {ratios[1]:.3f} (n = {N_SHORT})")
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("n", [MB.N_CLIP, N_SHORT])
def test_clip_mode_floor_comes_from_the_other_row(eng_rr, n):
    """A quiet and a loud regime in one oww_mel call: one call-wide floor, set by the loud row, clamps most of the quiet one."""
    regs = MB.regimes()
    pcm = np.stack([regs[QUIET][:n], regs[LOUD][:n]])
    ref = MB.reference(pcm)
    assert (ref.u[0] < ref.floor[0]).mean() > 0.5 and ref.floor[0] == ref.floor[1]
    got = eng_rr.mel(pcm)
    assert np.isfinite(got).all()
    r = [MB.worst_ratio(got[b:b + 1], MB.Ref(*(a[b:b + 1] for a in ref))) for b in range(2)]
    print(f"\nstacked {QUIET} / {LOUD}, n = {n}: worst error / budget = {r[0]:.3f} / {r[1]:.3f}")
    assert max(r) <= 1.0


@pytest.mark.parametrize("n", [MB.N_CLIP, N_SHORT])
def test_per_clip_floor(eng_default, n):
    """oww_mel_clips on the default family: the same stacked pair, each row with its own floor -- bit for bit its single-row result,
    and inside its own budget."""
    regs = MB.regimes()
    pcm = np.stack([regs[QUIET][:n], regs[LOUD][:n]])
    ref = MB.reference(pcm, per_clip=True)
    assert ref.floor[0] < ref.floor[1] - 30.0                      # (39.7 dB apart: a shared floor would clamp most of the quiet row)
    got = eng_default.mel_clips(pcm)
    assert np.isfinite(got).all()
    for b in range(2):
        alone = eng_default.mel_clips(pcm[b:b + 1])
        assert np.array_equal(got[b].view(np.uint32), alone[0].view(np.uint32)), f"row {b} depends on its neighbour"
    r = [MB.worst_ratio(got[b:b + 1], MB.Ref(*(a[b:b + 1] for a in ref))) for b in range(2)]
    print(f"\nper-clip floor, n = {n}: worst error / budget = {r[0]:.3f} / {r[1]:.3f}")
    assert max(r) <= 1.0


# ------------------------------------------------------------------------------------------------ streaming, fused kernel
def _placement(S, how):
    """Regime index of every row: cyclic, or the cyclic assignment moved through one fixed permutation of the rows."""
    idx = np.arange(S) % NR
    if how == "permuted":
        idx = idx[np.random.default_rng(7).permutation(S)]
    return idx


@functools.lru_cache(maxsize=None)
def _fused_run(S, how):
    """Four one-chunk steps on a fresh default-family handle of S streams -> (regime index per row, rows per step [S, 8, 32])."""
    idx = _placement(S, how)
    eng = _engine(S)
    try:
        got = _run_calls(eng, [REG[i] for i in idx])
        assert eng.range_status() is False
    finally:
        eng.close()
    return idx, got


def _check_fused(S, how, idx, got):
    ratios = {}
    for r, name in enumerate(REG):
        rows = np.nonzero(idx == r)[0]
        if rows.size == 0:
            continue
        rep = rows[0]
        for t, g in enumerate(got):
            differ = rows[(g[rows].view(np.uint32) != g[rep].view(np.uint32)).any(axis=(1, 2))]
            assert differ.size == 0, f"{name} step {t}: rows {differ.tolist()[:8]} differ from row {rep} on the same samples (S = {S}, {how})"
        ratios[name] = _check_stream_rows([g[rep] for g in got], name)
    _report(f"fused kernel, S = {S}, {how}", ratios)


@functools.lru_cache(maxsize=None)
def _big_S():
    return 12 * torch.cuda.get_device_properties(0).multi_processor_count + 13


@pytest.mark.parametrize("how", ["cyclic", "permuted"])
def test_fused_kernel_beyond_one_grid(how):
    """S = 12 CU + 13: one workgroup of 12 waves per CU, so 13 waves take a second trip of the grid-stride loop and the second trip's
    only workgroup is partly filled.  One row per regime meets the budget at every step; every other row of the regime -- rows 0, 11,
    12, 13 and S - 1 among them -- carries the same bits, wherever the placement puts it."""
    S = _big_S()
    idx, got = _fused_run(S, how)
    assert all((idx == r).sum() >= 2 for r in range(NR))
    _check_fused(S, how, idx, got)        # (rows 0, 11, 12, 13 and S - 1 each belong to some regime's rows and are compared there)


def test_fused_kernel_placements_agree():
    """A regime's rows carry the same bits in the cyclic and in the permuted run."""
    S = _big_S()
    (ia, ga), (ib, gb) = _fused_run(S, "cyclic"), _fused_run(S, "permuted")
    assert (ia != ib).mean() > 0.9
    for r, name in enumerate(REG):
        sa, sb = np.nonzero(ia == r)[0][0], np.nonzero(ib == r)[0][0]
        for t in range(len(STEPS)):
            assert np.array_equal(ga[t][sa].view(np.uint32), gb[t][sb].view(np.uint32)), f"{name} step {t}: rows {sa} (cyclic) and {sb} (permuted) differ"


@pytest.mark.parametrize("S", [1, 13])
def test_fused_kernel_small_counts(S):
    """The cyclic run at one stream (a lone wave) and at 13 (a second workgroup of one wave), the regimes in batches of S."""
    eng = _engine(S)
    try:
        ratios = {}
        for base in range(0, NR, S):
            names = [REG[(base + s) % NR] for s in range(S)]
            got = _run_calls(eng, names)
            for s, name in enumerate(names):
                ratios[name] = max(ratios.get(name, 0.0), _check_stream_rows([g[s] for g in got], name))
        assert eng.range_status() is False
    finally:
        eng.close()
    assert len(ratios) == NR
    _report(f"fused kernel, S = {S}", ratios)


# ------------------------------------------------------------------------------------------------ streaming, separate kernel
def _batches(eng, calls=STEPS):
    """Every regime through a 13-stream handle in batches -> name -> rows per call."""
    S, out = eng.n_streams, {}
    for base in range(0, NR, S):
        names = [REG[(base + s) % NR] for s in range(S)]
        got = _run_calls(eng, names, calls)
        for s, name in enumerate(names):
            out.setdefault(name, [g[s] for g in got])
    return out


def test_separate_kernel_streaming(eng_rr, eng_default):
    """The same regimes and steps through owk::mel_kernel (exact-fp32 family), and the two forms against each other: the largest
    |fused - separate| per regime is printed (mel units) and nothing is asserted about it beyond each form's own budget."""
    sep, fused = _batches(eng_rr), _batches(eng_default)
    _report("separate kernel, S = 13", {name: _check_stream_rows(sep[name], name) for name in REG})
    _report("fused kernel, S = 13 (max_chunks = 2 handle)", {name: _check_stream_rows(fused[name], name) for name in REG})
    print("\nlargest |fused - separate| per regime (mel units):")
    for name in REG:
        d = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(fused[name], sep[name]))
        print(f"    {name:16s} {d:.2e}")


@pytest.mark.parametrize("calls", [(2, 3), (3, 2)], ids=["2+3", "3+2"])
def test_multi_chunk_and_sliced_calls(eng_default, calls):
    """Default family, max_chunks = 2: a two-chunk call (one launch, two 8-frame groups) and a three-chunk call, which is evaluated in
    slices of 2 + 1 chunks that share the call's floor (max_only pass, then floor_max).  (3, 2): the long call is the first after a
    reset; silence_noise and the onset regimes put the loud part into the second slice, behind the rows it clamps.  (2, 3): the long
    call follows; noise_silence ends it in silence, which only the first slice's maximum clamps.  oww_get_mel reaches the rows of the
    last slice; all of a two-chunk call's."""
    got = _batches(eng_default, calls)
    k_long = calls.index(3)
    ref = _stream_ref("noise_silence", calls)[k_long]
    assert (ref.u[0, -4:] < ref.floor[0] - 50.0).all(), "the last rows of the long call lie far below a floor only its earlier part sets"
    _report(f"separate kernel, calls of {calls} chunks", {name: _check_stream_rows(got[name], name, calls) for name in REG})


# ------------------------------------------------------------------------------------------------ masked step
@pytest.mark.parametrize("family", ["default", "fp32"])
def test_masked_step_keeps_the_sample_tail(family):
    """oww_step_masked with stream 2 switched off for the second chunk: its rows for the third chunk equal, bit for bit, those of a
    twin handle whose streams never received the second chunk -- the 480-sample tail was kept -- and differ from those of a stream
    that consumed it."""
    kw = {} if family == "default" else {"use_mfma": 1}
    S, off = 13, 2
    regs = MB.regimes()
    names = [REG[s] for s in range(S)]
    chunk = lambda t: np.stack([regs[n][t * 1280:(t + 1) * 1280] for n in names])
    a, b = _engine(S, **kw), _engine(S, **kw)
    try:
        on = np.ones(S, np.uint8)
        on[off] = 0
        a.reset(); b.reset()
        a.step(chunk(0)); a.step_masked(chunk(1), on); a.step(chunk(2))
        b.step(chunk(0)); b.step(chunk(2))
        ga, gb = a.get_mel(off, 8), b.get_mel(off, 8)
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), "the masked stream lost or moved its sample tail"
        x = np.concatenate([regs[names[off]][:1280], regs[names[off]][2560:3840]])
        ref = MB.stream_reference(x, (1, 1))[1]
        r = MB.worst_ratio(ga[None], ref)
        consumed = MB.stream_reference(regs[names[off]], (1, 1, 1))[2]
        assert np.abs(consumed.clamped - ref.clamped).max() > 100 * ref.budget.max()       # a consumed chunk would be seen
        others = [s for s in range(S) if s != off]
        worst = max(MB.worst_ratio(a.get_mel(s, 8)[None], _stream_ref(names[s])[2]) for s in others)
        print(f"\nmasked step ({family}): stream {off} bit-identical to its twin, error / budget {r:.3f}; the other streams {worst:.3f}")
        assert r <= 1.0 and worst <= 1.0
        assert a.range_status() is False and b.range_status() is False
    finally:
        a.close(); b.close()
