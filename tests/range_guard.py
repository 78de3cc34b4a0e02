"""The f16 range guard's test bench (helper module, no tests, no HIP): where the conv histories sit in a stream state record, the
poison that drives one of them out of the f16 range, which wave must report it, and the gain tables of the sweeps.

Record mirror.  Only the eleven conv histories are mirrored (csrc/owwhip_layout.h: kStateLenRr words each, kStateSpgRr streams per
group block).  owwhip.hip::state_layout lists the sections and owwhip_state_host.h::layout (ows) places them: those with one stream
per block right behind the 8-word header, in order, and the grouped sections at the very end of the record, in order, followed only by the VAD's 256-word (h, c) section when the handle
has a VAD.  So every offset comes from one of the two ends and the record size (StreamEngine.state_info()[0]); nothing in the middle
(PCM tail, feature ring, score rings, counters, bank, ingest, audio) is mirrored, and the mirror holds for any head count, ring size,
bank or VAD.

Poison.  A history word of a section stored as fp32 becomes the fp32 value 1.0e5: the consuming layer's operand split
(owwhip_hx.h: split_pair) turns it into hi = f16(1e5) = +inf (0x7C00), lo = f16(1e5 - inf) = -inf (0xFC00), and hi * w + lo * w is
NaN in every output channel of that position.  Stage A keeps its two histories as the split's OUTPUT, so there
the halves are written directly, in the order the kernel stores them (read in owwhip_hx.h: hstageA_stream):
  hist_mel  64 words = 2 rows x 32 bins, one word per value: `hm[lane] = hi | lo << 16`            -> word 0xFC007C00
  hist2     [row 2][parity 2][dword 8][lane 64]: dwords 0..2 hold the hi halves of three channel pairs, dwords 3..5 the lo halves
            of the same pairs (`dst[0..128] = hh[0..2]; dst[192..320] = ll[0..2]`), dwords 6, 7 are never read or written
            -> hi dword 0x7C007C00, its partner 192 words further 0xFC00FC00
A value of hist2 therefore lives in two words; the one-word poison picks a hi dword and writes the partner with it.

One-word poison.  The word is drawn with a fixed seed among the words that are non-zero in a record exported after three steps of
noise audio (hist2: among the non-zero hi dwords): padding words that no kernel reads are zero in every record and are never drawn.
hist19 has one position per stream and eight streams per tile: lanes 8..15 of the tile mirror lanes 0..7 (hstage_kernel: `lanes 8..15
mirror 0..7`), and the record carries both positions of a stream, interleaved (owwhip_state.h: word 2 r + m of run r is position
m * 8 + place).  The mirror's convolution is computed and never stored, so its words (the odd ones) are non-zero and read by nobody
whose result survives: they are not drawn either.

Who reports.  raise_range_flag's n_streams, from the launch code: the fused front end and hstageA_kernel report the stream itself
(owwhip_fused.h:315, owwhip_hx.h: hstageA_kernel), hstage_kernel reports its group `s_first = g * SPT`, `C::SPT` streams (SPT = 1,
2, 4, 8 for stages B, C, D, E = kStateSpgRr of their histories), conv19 has no guard of its own and its NaN embedding is reported
by the heads kernel's wave of 32 streams, the VAD's LSTM by its tile of 16.  oww_range_where clamps the count to the handle's last
stream, so the expected answer is (first, min(n, S - first)) with first = s - s % n."""
import numpy as np

NAMES = ("hist_mel", "hist2", "B:b", "B:d", "C:b", "C:d", "D:b", "D:d", "E:b", "E:d", "hist19")
WORDS = (64, 2048, 1536, 1536, 1280, 1280, 768, 768, 384, 384, 384)            # kStateLenRr
STREAMS_PER_GROUP = (1, 1, 1, 1, 2, 2, 4, 4, 8, 8, 8)                          # kStateSpgRr
HEADER_WORDS = 8
VAD_HC = "vad_hc"
VAD_HC_WORDS = 256
# section -> the n_streams its guard passes to raise_range_flag
REPORTED_STREAMS = {"hist_mel": 1, "hist2": 1, "B:b": 1, "B:d": 1, "C:b": 2, "C:d": 2, "D:b": 4, "D:d": 4, "E:b": 8, "E:d": 8,
                    "hist19": 32, VAD_HC: 16}
# sections stored as f16 operand halves (stage A); every other section is fp32
F16_PAIR_SECTIONS = ("hist_mel", "hist2")
# DESIGN.md 5.16, default handle (3 heads, feature ring 16, no bank, no VAD): the words between the two groups of histories
OTHER_WORDS_DEFAULT = {"pcm_tail": 240, "feature_ring": 1536, "score_ring": 92, "raw": 4, "scores": 4, "frame_counter": 4,
                       "prediction_counter": 4, "vad_ring": 8, "vad_counter": 4}
DEFAULT_RECORD_BYTES = 49344

POISON_F32 = np.float32(1.0e5)
HI_INF, LO_NINF = 0x7C00, 0xFC00                                               # split_pair(1.0e5)
MEL_WORD = np.uint32(HI_INF | (LO_NINF << 16))                                 # hist_mel: hi | lo << 16
H2_HI_WORD = np.uint32(HI_INF | (HI_INF << 16))                                # hist2: two channels' hi halves
H2_LO_WORD = np.uint32(LO_NINF | (LO_NINF << 16))
H2_LO_AFTER = 192                                                              # words from a hi dword to its lo partner

MEL_GAINS = tuple(2.0 ** k for k in range(0, 25, 2))                           # 2^0, 2^2, ... 2^24
FEATURE_GAINS = tuple(2.0 ** k for k in range(0, 21))                          # 2^0 ... 2^20


def offsets(record_bytes, has_vad=False):
    """{section: (first word, words)} of a record of `record_bytes` bytes; with has_vad also the VAD's (h, c) section."""
    assert record_bytes % 4 == 0
    out, off = {}, HEADER_WORDS
    for name, n, spg in zip(NAMES, WORDS, STREAMS_PER_GROUP):
        if spg == 1:
            out[name] = (off, n)
            off += n
    end = record_bytes // 4
    if has_vad:
        end -= VAD_HC_WORDS
        out[VAD_HC] = (end, VAD_HC_WORDS)
    for name, n, spg in reversed(list(zip(NAMES, WORDS, STREAMS_PER_GROUP))):
        if spg > 1:
            end -= n
            out[name] = (end, n)
    assert end >= off, "the record is too small for the eleven histories"
    return out


def _h2_is_hi(idx):
    return (np.asarray(idx) // 64) % 8 < 3


def candidate_words(record, section, has_vad=False):
    """Word indices (within the section) the one-word poison may pick: non-zero in `record` (uint8 [record_bytes], exported after
    warm-up steps); hist2: hi dwords only."""
    first, n = offsets(record.size, has_vad)[section]
    w = np.ascontiguousarray(record).view(np.uint32)[first:first + n]
    idx = np.flatnonzero(w)
    if section == "hist2":
        idx = idx[_h2_is_hi(idx)]
    if section == "hist19":
        idx = idx[idx % 2 == 0]
    return idx


def poison(record, section, words=None, has_vad=False):
    """A copy of `record` (uint8 [record_bytes]) with `section` driven out of the f16 range: the whole section (words = None) or the
    listed word indices within it (hist2: hi dwords; their lo partners are written with them)."""
    rec = np.array(record, dtype=np.uint8, copy=True)
    first, n = offsets(rec.size, has_vad)[section]
    sec = rec.view(np.uint32)[first:first + n]
    idx = np.arange(n) if words is None else np.asarray(words, dtype=np.int64)
    assert idx.size and idx.min() >= 0 and idx.max() < n
    if section == "hist_mel":
        sec[idx] = MEL_WORD
    elif section == "hist2":
        if words is None:
            idx = idx[_h2_is_hi(idx)]
        assert _h2_is_hi(idx).all(), "hist2: pick hi dwords"
        sec[idx] = H2_HI_WORD
        sec[idx + H2_LO_AFTER] = H2_LO_WORD
    else:
        sec.view(np.float32)[idx] = POISON_F32
    return rec


def seeded_words(record, section, seed, has_vad=False):
    """One word of `section` for the one-word poison, drawn with `seed` among candidate_words."""
    cand = candidate_words(record, section, has_vad)
    assert cand.size, f"{section}: every word of the warmed-up record is zero"
    return cand[np.random.default_rng(1000 + seed).integers(cand.size)][None]


def expected_where(section, stream, n_streams_total):
    """(first, n) oww_range_where must name when `stream`'s `section` is out of range on a handle of n_streams_total streams."""
    n = REPORTED_STREAMS[section]
    first = stream - stream % n
    return first, min(n, n_streams_total - first)


# ------------------------------------------------------------------------------------------------ shared cases of the two sweeps
CNN_REGIMES = ("seed1234", "hot", "cold")                                      # cnn_budget.regime names
CNN_INPUT_STREAMS = (0, 5, 7)                                                  # of cnn_budget.mel_inputs(): normal, checker, impulse16

_LN64 = dict(kind="binary", T=16, hidden=64, n_out=1, layernorm=True)
FIXED_SHAPES = {"narrow_ln": _LN64, "narrow_noln": dict(_LN64, layernorm=False), "wide": dict(_LN64, hidden=128)}
GATED_SHAPE = dict(_LN64, kind="gated")
BANK_SHAPES = {"bank64": _LN64, "bank128": dict(_LN64, hidden=128)}
HEAD_SHAPES = {**FIXED_SHAPES, "gated": GATED_SHAPE, **BANK_SHAPES}


def make_head(form):
    """The head of HEAD_SHAPES[form]: tests/test_head_regimes.py's seed1 draw of that shape."""
    import test_head_regimes as HR
    return HR.make_head(HEAD_SHAPES[form], "seed1")


def cnn_inputs():
    """float32 [3, 92, 32]: three of cnn_budget's embed() inputs (three windows each)."""
    import cnn_budget as CB
    return np.ascontiguousarray(CB.mel_inputs()[list(CNN_INPUT_STREAMS)])


def window_ratios(got, e64):
    """cnn_budget's normalisation per WINDOW: [B, n_win, 96] x 2 -> [B * n_win] of max |got - e64| / max |e64|."""
    import cnn_budget as CB
    return CB.ratios(np.asarray(got).reshape(-1, got.shape[-1]), np.asarray(e64).reshape(-1, e64.shape[-1]))
