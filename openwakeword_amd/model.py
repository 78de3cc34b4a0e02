"""
`Model` / `AudioFeatures`: the reference's Python surface for the streaming path, on the HIP library.

Mirrors `openwakeword.Model` (/root/reference/openwakeword/model.py:32-426) and the streaming half of
`openwakeword.utils.AudioFeatures` (utils.py:163-178, 387-463): same constructor keywords, `predict`,
`predict_clip`, `reset`, `prediction_buffer`, `models`, `model_inputs`, `model_outputs`, `class_mapping`,
`preprocessor.get_features`, same exceptions.  `inference_framework="hip"` is the value this package adds
to the reference's `"onnx"` / `"tflite"` selector (model.py:46,112,133).

One `Model` object = one audio stream, like the reference.  The arithmetic (mel, embedding CNN, heads) runs
in libowwhip.so on the GPU through a 1-stream `StreamEngine`; this file only keeps the reference's
host-side control flow: 1280-sample alignment with carry-over (utils.py:409-430), the "repeat the last
prediction" rule for short calls (model.py:299-307), custom verifier hook (model.py:320-328), first-5
zeroing / patience / debounce on the 30-deep `prediction_buffer` (model.py:330-363).  For many streams use
`BatchedModel`, which keeps that post-processing on the device as well.

There is no CPU fallback: constructing a Model without the HIP library or a GPU raises.
"""
from __future__ import annotations

import os
import pickle
import warnings
import wave
from collections import defaultdict, deque
from functools import partial
from typing import Callable, DefaultDict, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import weights as W
from ._lib import FIT_STATUS
from .engine import CHUNK, EMB_DIM, StreamEngine, check_audio_config, check_event_config

# openwakeword/__init__.py:26-60 (names only; the files are release assets that are not in the checkout)
MODELS = {name: {"model_path": os.path.join(os.path.dirname(os.path.abspath(__file__)), "resources", "models",
                                            f"{name}_v0.1.onnx")}
          for name in ("alexa", "hey_mycroft", "hey_jarvis", "hey_rhasspy", "timer", "weather")}
FEATURE_MODELS = {k: {"model_path": os.path.join(os.path.dirname(os.path.abspath(__file__)), "resources", "models", f)}
                  for k, f in (("embedding", "embedding_model.onnx"), ("melspectrogram", "melspectrogram.onnx"))}
# openwakeword/__init__.py:62-71
model_class_mappings = {
    "timer": {"1": "1_minute_timer", "2": "5_minute_timer", "3": "10_minute_timer",
              "4": "20_minute_timer", "5": "30_minute_timer", "6": "1_hour_timer"}
}


def get_pretrained_model_paths(inference_framework: str = "hip") -> List[str]:
    return [MODELS[k]["model_path"] for k in MODELS]


def _load_head(path_or_name: str, synthetic_seed: Optional[int]):
    """Return (model name, head dict).  A path must be an .onnx file readable by onnx_ingest; a bare name is
    looked up among the pretrained files, or generated when synthetic weights were asked for."""
    if os.path.exists(path_or_name):
        if path_or_name.endswith(".tflite"):
            raise ValueError("The hip inference framework is selected, but tflite models were provided!")
        from . import onnx_ingest
        return os.path.splitext(os.path.basename(path_or_name))[0], onnx_ingest.load_head(path_or_name)
    key = path_or_name.replace(" ", "_")
    match = [p for p in get_pretrained_model_paths() if key in p.split(os.path.sep)[-1]]
    if not match:
        raise ValueError("Could not find pretrained model for model name '{}'".format(path_or_name))
    if os.path.exists(match[0]):
        from . import onnx_ingest
        return path_or_name, onnx_ingest.load_head(match[0])
    if synthetic_seed is None:
        raise ValueError(f"Pretrained model file {match[0]} does not exist (the reference downloads it at run "
                         "time, utils.py:625-673). Pass weights='synthetic' to use random-init weights of the "
                         "same architecture, or give the path of an .onnx file.")
    base = [k for k in MODELS if k in os.path.basename(match[0])][0]
    return path_or_name, W.synthetic_head(base, synthetic_seed)


def resolve_weights(weights: Union[str, dict, None]):
    """(seed, embedding or None, given heads) from the `weights` argument shared by Model, BatchedModel and utils.bulk_predict:
    'synthetic' -> seed 1234; a dict may carry 'embedding', 'heads', 'seed'; None -> real files only."""
    if weights is None:
        return None, None, {}
    if isinstance(weights, str):
        if weights != "synthetic":
            raise ValueError("weights must be 'synthetic', a dict {'embedding':..., 'heads':...} or None")
        return 1234, None, {}
    if isinstance(weights, dict):
        return weights.get("seed"), weights.get("embedding"), dict(weights.get("heads", {}))
    raise ValueError("weights must be 'synthetic', a dict {'embedding':..., 'heads':...} or None")


def _verify_melspectrogram(mel_path: str) -> None:
    """Hold a melspectrogram graph file to the analytic HIP front end (onnx_ingest.verify_melspectrogram).  A parameter FOUND to differ
    (window, hop, filter bank, amin, top_db ...) refuses.  A structure the verifier cannot follow (an exporter idiom it does not know)
    is not waved through: the file is then EVALUATED on probe audio (onnx_ingest.probe_melspectrogram) and must reproduce the recipe
    numerically, else it is refused too.  OWW_TRUST_MELSPECTROGRAM=1 is the only way past both checks."""
    if os.environ.get("OWW_TRUST_MELSPECTROGRAM") == "1":
        return
    from . import onnx_ingest
    hint = (".  The HIP front end computes the published recipe only; if this graph is known to be equivalent, set "
            "OWW_TRUST_MELSPECTROGRAM=1 and hold the result to tests/test_real_reference.py")
    try:
        onnx_ingest.verify_melspectrogram(mel_path)
    except onnx_ingest.GraphIdiomUnknown as e:
        try:
            onnx_ingest.probe_melspectrogram(mel_path)
        except ValueError as e2:
            raise ValueError(f"{e}; and the numeric check did not clear it either: {e2}{hint}") from e2
    except ValueError as e:
        raise ValueError(f"{e}{hint}") from e


def resolve_embedding(embedding: Optional[dict], seed: Optional[int], embedding_model_path: str = "",
                      melspec_model_path: str = "") -> dict:
    """The shared speech-embedding network (utils.py:90-93 loads embedding_model.onnx next to the wake-word models): the
    caller's weights, else the file the caller names (the reference's `embedding_model_path` / `melspec_model_path` keyword
    arguments, utils.py:38-44), else the real file in resources/models through onnx_ingest, else -- ONLY when synthetic weights
    were asked for -- the random-init network.  Never silently synthetic: real head files next to a random embedding would score
    nonsense."""
    for given in (embedding_model_path, melspec_model_path):
        if given and given.endswith(".tflite"):                         # utils.py:75-76, for this backend
            raise ValueError("The hip inference framework is selected, but tflite models were provided!")
        if given and not os.path.exists(given):
            raise ValueError(f"{given} does not exist")
    if embedding is not None and not embedding_model_path:
        if melspec_model_path:
            _verify_melspectrogram(melspec_model_path)
        return embedding
    path = embedding_model_path or FEATURE_MODELS["embedding"]["model_path"]
    if os.path.exists(path):
        from . import onnx_ingest
        # real model files: the log-mel front end of the HIP path is analytic, so the melspectrogram graph that sits next to the
        # embedding network is VERIFIED to be that recipe (or the construction fails loudly: onnx_ingest.verify_melspectrogram)
        mel_path = melspec_model_path or FEATURE_MODELS["melspectrogram"]["model_path"]
        if os.path.exists(mel_path):
            _verify_melspectrogram(mel_path)
        return onnx_ingest.load_embedding(path)
    if seed is not None:
        return W.synthetic_embedding(seed)
    raise ValueError(f"{path} does not exist; pass weights='synthetic' for random-init weights of the same architecture")


class VerifierFoldWarning(UserWarning):
    """fold_verifier: the folded verifier's device score is predicted to leave the pipeline's by more than the 1e-4 score class."""


SCORE_CLASS = 1e-4           # the parity class of scores
# max |z_fp32 - z_float64| / (sum |w_i x_i| + |b|) of the verifier kernels' summation order, in units of 2^-24: the largest of
# tests/verifier_budget.py::E32 (tests/test_verifier_budget_cpu.py::test_e32_and_a_are_the_measured_envelope measures it, and
# test_model_constant_is_the_budget_s holds this copy to it)
VERIFIER_E32 = 1.35


def verifier_fold_deviation(w, b, mean, scale):
    """(predicted |device score - pipeline score|, kappa_hat, the three feature indices that carry most of it) of a folded verifier.
    kappa_hat = sum |w_i| (|mean_i| + scale_i) + |b| is the mass the device's fp32 sum has to cancel on data the scaler was fitted
    to; the fp32 rounding of w and b moves the logit by up to 4 * 2^-24 * kappa_hat, the device's summation by 4 * VERIFIER_E32 * 2^-24
    * kappa_hat, and the sigmoid passes on a quarter of that."""
    mass = np.abs(np.asarray(w, np.float64)) * (np.abs(np.asarray(mean, np.float64)) + np.asarray(scale, np.float64))
    kappa_hat = float(mass.sum() + abs(b))
    return 0.25 * (4.0 * VERIFIER_E32 + 4.0) * 2.0 ** -24 * kappa_hat, kappa_hat, np.argsort(-mass, kind="stable")[:3]


def fold_verifier(verifier):
    """(w, bias) of a custom verifier: the reference's scikit-learn pipeline FunctionTransformer(flatten) -> StandardScaler ->
    LogisticRegression (custom_verifier_model.py:95-113) folded into one affine map, or a ready (w, bias) pair.  The fold removes the
    scaler's centring, so the device's fp32 sum has to cancel sum w_i x_i against the bias: where that is predicted to cost more than
    the 1e-4 score class (a feature column that was nearly constant in the training data: a tiny scale_ next to a large mean_), a
    VerifierFoldWarning names the columns.  The result is the same either way."""
    if isinstance(verifier, (tuple, list)) and len(verifier) == 2:
        return np.asarray(verifier[0], np.float32).ravel(), float(verifier[1])
    steps = getattr(verifier, "steps", None)
    if not steps:
        raise ValueError("the device verifier needs the reference's pipeline (flatten -> StandardScaler -> LogisticRegression) or a (w, bias) pair")
    # exactly the reference's structure, nothing skipped in silence: [FunctionTransformer (the flatten)] [StandardScaler] classifier.
    # Any other transformer (PCA, a second scaler, ...) would fold into wrong scores: the caller must then keep the host-side hook
    # of the single-stream Model (model.py:320-328), which runs any pickled object.
    body = [st for _, st in steps]
    clf = body.pop()
    if body and type(body[0]).__name__ == "FunctionTransformer":
        body.pop(0)
    scaler = body.pop(0) if body and type(body[0]).__name__ == "StandardScaler" else None
    if body:
        raise ValueError("the device verifier folds only the reference's pipeline flatten -> StandardScaler -> LogisticRegression; "
                         f"unsupported steps: {[type(st).__name__ for st in body]} (use the host-side hook of openwakeword_amd.Model)")
    if not hasattr(clf, "coef_") or not hasattr(clf, "intercept_") or np.asarray(clf.coef_).shape[0] != 1:
        raise ValueError("the last step of the verifier pipeline must be a fitted binary LogisticRegression")
    coef = np.asarray(clf.coef_, np.float64)[0]
    b = float(np.asarray(clf.intercept_, np.float64)[0])
    if scaler is not None:
        # StandardScaler(with_mean=False) leaves mean_ = None, with_std=False leaves scale_ = None
        scale = np.ones_like(coef) if getattr(scaler, "scale_", None) is None else np.asarray(scaler.scale_, np.float64)
        mean = np.zeros_like(coef) if getattr(scaler, "mean_", None) is None else np.asarray(scaler.mean_, np.float64)
        if scale.shape != coef.shape or mean.shape != coef.shape:
            raise ValueError(f"verifier pipeline: scaler has {scale.size} features, the classifier {coef.size}")
        b -= float(np.sum(coef * mean / scale))
        coef = coef / scale
        dev, kappa_hat, worst = verifier_fold_deviation(coef.astype(np.float32), b, mean, scale)
        if dev > SCORE_CLASS:
            warnings.warn(f"custom verifier: the device score may differ from the pipeline's by about {dev:.1e} (more than {SCORE_CLASS:g}): the "
                          f"folded map has to cancel a mass of {kappa_hat:.3g} in fp32.  Largest contributions: features "
                          f"{', '.join(str(int(i)) for i in worst)} (scale_ = {', '.join(f'{scale[i]:.3g}' for i in worst)}; mean_ = "
                          f"{', '.join(f'{mean[i]:.3g}' for i in worst)}); a column that was nearly constant in training (a tiny scale_ "
                          "next to a large mean_) is the usual cause: drop it before fitting, or keep the host-side hook of "
                          "openwakeword_amd.Model", VerifierFoldWarning, stacklevel=2)
    return coef.astype(np.float32), b


class AudioFeatures:
    """Streaming half of openwakeword.utils.AudioFeatures on one device stream.

    `__call__(x)` buffers audio exactly like utils.py:409-452 and advances the device by whole 1280-sample
    chunks; `get_features(n)` reads the device feature ring (utils.py:454-460)."""

    feature_buffer_max_len = 120        # utils.py:170

    def __init__(self, engine: StreamEngine, stream: int = 0):
        self.engine = engine
        self.sid = int(stream)
        self._pending = np.empty(0, dtype=np.int16)     # samples appended to the raw buffer, not yet processed
        self.accumulated_samples = 0
        self.raw_data_remainder = np.empty(0, dtype=np.int16)
        self.last_scores: Optional[np.ndarray] = None
        self.reset()

    def _get_embeddings(self, x: np.ndarray) -> np.ndarray:
        """utils.py:210-241: mel of the whole clip, 76-row windows every 8 rows, one embedding each."""
        spec = self.engine.mel(np.asarray(x, dtype=np.int16)[None])[0] / 10.0 + 2.0       # utils.py:180,206
        n_win = (spec.shape[0] - 76) // 8 + 1
        if n_win < 1:
            return np.zeros((0, EMB_DIM), np.float32)
        out = self.engine.embed(spec[None, : 76 + 8 * (n_win - 1)].astype(np.float32))[0]
        return out

    # ---- the reference's stateless helpers (training / data-preparation code calls them directly), same shapes -------------
    def _get_melspectrogram(self, x, melspec_transform: Callable = lambda x: x / 10 + 2) -> np.ndarray:
        """utils.py:180-208: int16 samples `[n]` or `[B, n]` -> transformed mel rows `[F, 32]` / `[B, F, 32]`; one clamp floor
        for the whole call, like one run of the melspectrogram graph."""
        x = np.array(x).astype(np.int16) if isinstance(x, list) else np.asarray(x)
        if x.dtype != np.int16:
            raise ValueError("Input data must be 16-bit integers (i.e., 16-bit PCM audio)."
                             f"You provided {x.dtype} data.")
        x = x[None, ] if x.ndim < 2 else x
        return melspec_transform(np.squeeze(self.engine.mel(x)))

    def _batched(self, fn, x):
        cap = self.engine.n_streams_padded
        return np.concatenate([fn(x[o:o + cap]) for o in range(0, x.shape[0], cap)], axis=0)

    def _get_embeddings_from_melspec(self, melspec) -> np.ndarray:
        """utils.py:210-223: one 76-row window `[76, 32(, 1)]` (or a batch of them) -> its embedding, squeezed."""
        m = np.asarray(melspec, dtype=np.float32)
        if m.ndim >= 3 and m.shape[-1] == 1:
            m = m[..., 0]
        if m.ndim == 2:
            m = m[None, ]
        if m.ndim != 3 or m.shape[1:] != (76, 32):
            raise ValueError(f"expected melspectrogram windows of shape [76, 32, 1], got {np.asarray(melspec).shape}")
        return np.squeeze(self._batched(self.engine.embed, m))

    def _get_melspectrogram_batch(self, x, batch_size: int = 128, ncpu: int = 1) -> np.ndarray:
        """utils.py:243-290 (the CPU path: every clip is its own run of the melspectrogram graph, so every clip has its own
        clamp floor): int16 `[N, samples]` -> `[N, ceil(samples/160 - 3), 32]`, transformed (x/10 + 2)."""
        x = np.asarray(x)
        if x.ndim != 2 or x.dtype != np.int16:
            raise ValueError("Input data must be 16-bit integers (i.e., 16-bit PCM audio) of shape (N, samples)")
        return (self._batched(self.engine.mel_clips, x) / 10.0 + 2.0).astype(np.float32)

    def _get_embeddings_batch(self, x, batch_size: int = 128, ncpu: int = 1) -> np.ndarray:
        """utils.py:292-352: mel rows `[N, frames, 32(, 1)]` -> `[N, (frames - 76)//8 + 1, 96]`: 76-row windows every 8 rows;
        rows past the last whole window are ignored."""
        m = np.asarray(x, dtype=np.float32)
        if m.ndim == 4 and m.shape[-1] == 1:
            m = m[..., 0]
        if m.ndim != 3 or m.shape[2] != 32:
            raise ValueError(f"expected melspectrograms of shape (N, frames, 32), got {np.asarray(x).shape}")
        if m.shape[1] < 76:
            raise ValueError("Embedding model requires the input melspectrograms to have at least 76 frames")
        n_win = (m.shape[1] - 76) // 8 + 1
        return self._batched(self.engine.embed, np.ascontiguousarray(m[:, : 76 + 8 * (n_win - 1)]))

    def get_embedding_shape(self, audio_length: float, sr: int = 16000):
        """Shape of `_get_embeddings` for a clip of `audio_length` seconds (utils.py:238-241), from the frame arithmetic
        instead of a trial run: F = (n-512)//160 + 1 mel frames, (F-76)//8 + 1 windows."""
        n = int(audio_length * sr + 1e-6)           # (the float product of an exact sample count may land just below it)
        frames = (n - 512) // 160 + 1 if n >= 512 else 0
        return (max((frames - 76) // 8 + 1, 0), EMB_DIM)

    def embed_clips(self, x: np.ndarray, batch_size: int = 128, ncpu: int = 1) -> np.ndarray:
        """Embeddings of N equally long clips, `[N, samples] int16 -> [N, n_windows, 96]` (utils.py:354-385: mel per clip,
        76-row windows every 8 rows, the embedding model over all windows) -- one `oww_embed_clips` call per batch, PCM in,
        embeddings out, nothing else crosses the bus.  `ncpu` is accepted for signature compatibility; `batch_size` is
        capped by the handle's stream count.  Borrows the streaming state of the first streams: both the engine and this
        object are reset afterwards."""
        x = np.asarray(x)
        if x.ndim != 2 or x.dtype != np.int16:
            raise ValueError("embed_clips expects a 2-D int16 array [N, samples]")
        if x.shape[1] < 512 or (x.shape[1] - 512) // 160 + 1 < 76:          # utils.py:313-314
            raise ValueError("Embedding model requires the input melspectrograms to have at least 76 frames")
        cap = max(1, min(int(batch_size), self.engine.n_streams_padded))
        out = [self.engine.embed_clips(x[o:o + cap]) for o in range(0, x.shape[0], cap)]
        self.engine.reset()                 # borrowed streams back to the start-up state ...
        self.reset()                        # ... and this object's stream re-seeded like a fresh AudioFeatures
        return np.concatenate(out, axis=0) if out else np.zeros((0, 0, EMB_DIM), np.float32)

    def reset(self):
        """utils.py:172-178: the feature ring restarts from the embeddings of 4 s of random audio."""
        self._pending = np.empty(0, dtype=np.int16)
        self.accumulated_samples = 0
        self.raw_data_remainder = np.empty(0, dtype=np.int16)
        noise = np.random.randint(-1000, 1000, 16000 * 4).astype(np.int16)
        feats = self._get_embeddings(noise)                       # [41, 96]; clobbers stream state -> reset below
        ring = np.zeros((self.engine.feature_ring, EMB_DIM), np.float32)
        n = min(len(feats), ring.shape[0])
        ring[ring.shape[0] - n:] = feats[len(feats) - n:]
        self._n_features = n
        self.engine.reset([self.sid], ring)

    def __call__(self, x: np.ndarray) -> int:
        x = np.asarray(x)
        if x.dtype != np.int16:                                     # utils.py:195-197 (lists are cast, 194)
            raise ValueError("Input data must be 16-bit integers (i.e., 16-bit PCM audio)."
                             f"You provided {x.dtype} data.")
        # 1280-sample alignment (utils.py:413-430): samples beyond the last whole chunk wait in `raw_data_remainder`
        # -- but only once at least one whole chunk has accumulated; shorter input simply accumulates
        if self.raw_data_remainder.shape[0]:
            x = np.concatenate((self.raw_data_remainder, x))
            self.raw_data_remainder = np.empty(0, dtype=np.int16)
        total = self.accumulated_samples + x.shape[0]
        take = x.shape[0] - (total % CHUNK if total >= CHUNK else 0)
        self._pending = np.concatenate((self._pending, x[:take]))
        self.raw_data_remainder = x[take:]
        self.accumulated_samples += take

        n = self.accumulated_samples
        if n < CHUNK or n % CHUNK:
            return n                                             # nothing processed yet: the caller repeats its last scores
        k = n // CHUNK
        # one device step: mel over the k chunks (one clamp floor), k embeddings, heads per chunk, max over chunks.  A call
        # longer than max_chunks x 1280 samples (2.56 s by default; the reference takes any length, model.py:287-298) is
        # evaluated by the library in slices of max_chunks chunks that share the CALL's clamp floor (oww_step: one extra pass of
        # the mel kernel finds the call's maximum first), i.e. the reference's single run of the melspectrogram graph
        # (utils.py:387-401); calls beyond the ABI's limit (5.5 minutes in one predict()) are refused by it.
        self.last_scores = self.engine.step_raw(self._pending[None])[0]
        self._n_features = min(self._n_features + k, self.feature_buffer_max_len)
        self._pending = np.empty(0, dtype=np.int16)
        self.accumulated_samples = 0
        return n

    def get_features(self, n_feature_frames: int = 16, start_ndx: int = -1) -> np.ndarray:
        have = min(self._n_features, self.engine.feature_ring)
        buf = self.engine.get_features(self.sid, have)              # the reference's feature_buffer, oldest first
        if start_ndx != -1:                                         # utils.py:455-458
            end_ndx = start_ndx + int(n_feature_frames) if start_ndx + n_feature_frames != 0 else len(buf)
            return buf[start_ndx:end_ndx, :][None, ].astype(np.float32)
        return buf[int(-1 * n_feature_frames):, :][None, ].astype(np.float32)


def check_bank_head(head: dict, feature_ring: int) -> None:
    """The forms the head bank's routed kernel takes (include/owwhip.h: oww_bank_add), checked before the library is touched."""
    kind = head.get("kind")
    if kind == "rnn":
        raise ValueError("recurrent heads cannot go into the head bank; load them as fixed heads (wakeword_models)")
    if kind == "gated":
        raise ValueError("gated heads cannot go into the head bank; load them as fixed heads (wakeword_models)")
    if kind == "multiclass" or int(head["n_out"]) != 1:
        raise ValueError("multiclass heads cannot go into the head bank (a bank head has one sigmoid output); load them as fixed heads")
    if kind != "binary":
        raise ValueError(f"unknown head kind {kind!r}")
    if len(W.net_blocks(head["net"])) != 1:
        raise ValueError("a bank head has exactly one hidden block (train.py:73 n_blocks = 1); load other nets as fixed heads")
    if not 1 <= int(head["hidden"]) <= 128:
        raise ValueError(f"a bank head has at most 128 hidden units (got {head['hidden']})")
    if not 1 <= int(head["T"]) <= int(feature_ring):
        raise ValueError(f"the bank head's T = {head['T']} exceeds the handle's feature ring ({feature_ring} rows)")


def make_engine(n_streams: int, heads: dict, embedding: dict, use_mfma: Optional[int] = None, **kw) -> StreamEngine:
    """The engine behind Model / BatchedModel.  `use_mfma` None = the default fp16-split family (3), and -- when oww_commit refuses
    these weights for it (OWW_ERANGE: the commit-time comparison with the exact-fp32 kernels failed, i.e. the weights' range cannot be
    carried by f16 hi/lo pairs) -- the exact-fp32 family (1) instead, under a loud RuntimeWarning: a custom-trained model must never
    be unloadable.  An explicit value is taken as given (and an explicit 3 raises on such weights)."""
    from ._lib import OwwRangeError
    if use_mfma is not None:
        return StreamEngine(n_streams, heads, embedding, use_mfma=int(use_mfma), **kw)
    try:
        return StreamEngine(n_streams, heads, embedding, use_mfma=3, **kw)
    except OwwRangeError as e:
        import warnings
        warnings.warn(f"{e} -- falling back to the exact-fp32 kernel family (use_mfma=1): same results, about 2.5x slower (masked "
                      "steps -- predict_active, the fan-in server -- run full launches there)", RuntimeWarning)
        return StreamEngine(n_streams, heads, embedding, use_mfma=1, **kw)


class Model:
    """openwakeword.Model on the HIP library (one stream per object)."""

    def __new__(cls, *args, **kwargs):
        """`inference_framework="onnx"` / `"tflite"` (model.py:112-141) keep working where their runtimes exist: the call is
        handed to the reference package unchanged and ITS Model object is returned.  Where `openwakeword` (or the runtime it
        imports at module level, vad.py:48) is not importable this raises the reference's own kind of error (ValueError, cf.
        model.py:141) -- there is no silent fall-back to the HIP path or to anything else."""
        framework = kwargs.get("inference_framework", args[6] if len(args) > 6 else "hip")     # 7th positional parameter, as in the reference
        if framework == "hip":
            return super().__new__(cls)
        if framework not in ("onnx", "tflite"):
            raise ValueError(f"unknown inference_framework '{framework}': 'hip' (this package), or 'onnx' / 'tflite' "
                             "(handed to the reference package)")
        try:
            import openwakeword as reference_package
        except Exception as e:                       # ImportError of the package itself or of onnxruntime / tflite inside it
            raise ValueError(f"inference_framework='{framework}' is served by the reference package, which cannot be imported "
                             f"here ({type(e).__name__}: {e}); use inference_framework='hip'") from e
        passthrough = {k: v for k, v in kwargs.items() if k not in ("weights", "max_chunks", "vad_session", "use_mfma")
                       and not (k == "device" and not isinstance(v, str))}      # (the reference's own device is "cpu" / "gpu")
        return reference_package.Model(*args, **passthrough)

    def __init__(self, wakeword_models: List[str] = [], class_mapping_dicts: List[dict] = [],
                 enable_speex_noise_suppression: bool = False, vad_threshold: float = 0,
                 custom_verifier_models: dict = {}, custom_verifier_threshold: float = 0.1,
                 inference_framework: str = "hip", weights: Union[str, dict, None] = None, device: int = 0,
                 max_chunks: int = 32, wakeword_model_paths: Optional[List[str]] = None, vad_session=None,
                 use_mfma: Optional[int] = None, **kwargs):
        if wakeword_model_paths is not None:            # deprecated alias (model.py:37)
            wakeword_models = wakeword_model_paths
        seed, embedding, given_heads = resolve_weights(weights)
        wakeword_models = list(wakeword_models)
        if wakeword_models == [] and given_heads:
            wakeword_models = list(given_heads)
        if wakeword_models == []:
            wakeword_models = list(MODELS.keys())           # model.py:84-87: all pretrained models
        heads: Dict[str, dict] = {}
        for m in wakeword_models:
            if m in given_heads:
                heads[m] = given_heads[m]
            else:
                name, head = _load_head(m, seed)
                heads[name] = head
        # the keyword arguments the reference hands on to AudioFeatures (model.py:212, utils.py:38-44)
        unknown = sorted(set(kwargs) - {"melspec_model_path", "embedding_model_path", "sr", "ncpu"})
        if unknown:
            raise TypeError(f"AudioFeatures.__init__() got an unexpected keyword argument '{unknown[0]}'")
        if int(kwargs.get("sr", 16000)) != 16000:
            raise ValueError("the HIP path runs the reference's 16 kHz models; resample first (openwakeword_amd.resample)")
        if isinstance(device, str):                     # the reference's device is "cpu" / "gpu" (utils.py:43): this backend has one answer
            device = 0
        embedding = resolve_embedding(embedding, seed, kwargs.get("embedding_model_path", "") or "", kwargs.get("melspec_model_path", "") or "")

        self.models: Dict[str, dict] = heads
        self.model_inputs = {n: int(h["T"]) for n, h in heads.items()}          # model.py:156
        self.model_outputs = {n: int(h["n_out"]) for n, h in heads.items()}     # model.py:157
        self.class_mapping: Dict[str, dict] = {}
        for i, n in enumerate(heads):                                           # model.py:177-182
            if class_mapping_dicts and i < len(class_mapping_dicts) and class_mapping_dicts[i].get(n, None):
                self.class_mapping[n] = class_mapping_dicts[i]
            elif model_class_mappings.get(n, None):
                self.class_mapping[n] = model_class_mappings[n]
            else:
                self.class_mapping[n] = {str(j): str(j) for j in range(0, self.model_outputs[n])}

        self.custom_verifier_models: Dict[str, object] = {}
        self.custom_verifier_threshold = custom_verifier_threshold
        if isinstance(custom_verifier_models, dict):
            for n in heads:
                if custom_verifier_models.get(n, False):
                    self.custom_verifier_models[n] = pickle.load(open(custom_verifier_models[n], "rb"))
            if len(self.custom_verifier_models.keys()) < len(custom_verifier_models.keys()):     # model.py:189-195
                raise ValueError("Custom verifier models were provided, but some were not matched with a base model!"
                                 " Make sure that the keys provided in the `custom_verifier_models` dictionary argument"
                                 " exactly match that of the `.models` attribute of an instantiated openWakeWord Model object"
                                 " that has the same base models but doesn't have custom verifier models.")

        self.prediction_buffer: DefaultDict[str, deque] = defaultdict(partial(deque, maxlen=30))     # model.py:198
        if enable_speex_noise_suppression:                                       # model.py:201-205 (host library)
            from speexdsp_ns import NoiseSuppression
            self.speex_ns = NoiseSuppression.create(160, 16000)
        else:
            self.speex_ns = None
        self.vad_threshold = vad_threshold
        if vad_threshold > 0:                                                    # model.py:208-210
            from .vad import VAD
            self.vad = VAD(session=vad_session)         # raises ValueError without a network (silero_vad.onnx is not in the checkout)

        self._engine = make_engine(1, heads, embedding, use_mfma, device=device, max_chunks=max_chunks,
                                   feature_ring=AudioFeatures.feature_buffer_max_len)
        self._cols = self._engine.head_cols
        self.preprocessor = AudioFeatures(self._engine, 0)

    def close(self):
        self._engine.close()

    # ---- label bookkeeping ---------------------------------------------------------------------------------------
    def get_parent_model_from_label(self, label):
        """Model that owns a prediction label (model.py:215-224): a binary model's label is its own name, a multiclass
        model owns the values of its class mapping.  The last match wins, '' when nothing matches."""
        owner = ""
        for name, mapping in self.class_mapping.items():
            if label in mapping.values() or label == name:
                owner = name
        return owner

    def reset(self):
        """Model.reset (model.py:226-230): empty score history, fresh front-end state (new random feature-ring seed)."""
        self.prediction_buffer = defaultdict(partial(deque, maxlen=30))
        self.preprocessor.reset()

    def _suppress_noise_with_speex(self, x: np.ndarray, frame_size: int = 160):
        # host-side pre-filter exactly as in the reference (model.py:481-504): 10 ms frames through SpeexDSP
        pieces = (self.speex_ns.process(x[o:o + frame_size].tobytes()) for o in range(0, x.shape[0], frame_size))
        return np.frombuffer(b"".join(pieces), np.int16)

    # ---- one predict() call = the reference's model.py:232-386, split into its four phases ------------------------
    def _raw_outputs(self, name: str, n_prepared: int):
        """Per-model output vector of this call: device result when at least one 80 ms chunk was completed (already the
        maximum over chunks for longer calls, model.py:287-298), otherwise the previous prediction / zeros (299-307)."""
        lo, hi = self._cols[name]
        if n_prepared >= CHUNK:
            return self.preprocessor.last_scores[lo:hi]
        if self.model_outputs[name] == 1:
            history = self.prediction_buffer[name]
            return [history[-1] if len(history) else 0]
        return [0] * (max(int(k) for k in self.class_mapping[name]) + 1)

    def _apply_verifiers(self, scores: dict, name: str):
        # model.py:320-328: a pickled scikit-learn classifier re-scores frames the base model already likes
        for label, value in list(scores.items()):
            if value < self.custom_verifier_threshold:
                continue
            verifier = self.custom_verifier_models.get(self.get_parent_model_from_label(label), False)
            if verifier:
                scores[label] = verifier.predict_proba(self.preprocessor.get_features(self.model_inputs[name]))[0][-1]

    def _gate(self, scores: dict, n_prepared: int, patience: dict, threshold: dict, debounce_time: float):
        # model.py:340-359 -- the rules look at scores buffered BEFORE this call
        if not patience and not debounce_time > 0:
            return
        if threshold == {}:
            raise ValueError("Error! When using the `patience` argument, threshold "
                             "values must be provided via the `threshold` argument!")
        if patience != {} and debounce_time > 0:
            raise ValueError("Error! The `patience` and `debounce_time` arguments cannot be used together!")
        for label in scores:
            if scores[label] == 0.0:
                continue
            owner = self.get_parent_model_from_label(label)
            past = np.array(self.prediction_buffer[label])
            if owner in patience:
                need = patience[owner]
                if (past[-need:] >= threshold[owner]).sum() < need:
                    scores[label] = 0.0
            elif debounce_time > 0 and owner in threshold:
                span = int(np.ceil(debounce_time / (n_prepared / 16000)))
                if scores[label] >= threshold[owner] and (past[-span:] >= threshold[owner]).sum() > 0:
                    scores[label] = 0.0

    def predict(self, x: np.ndarray, patience: dict = {}, threshold: dict = {}, debounce_time: float = 0.0,
                timing: bool = False):
        if not isinstance(x, np.ndarray):
            raise ValueError(f"The input audio data (x) must by a Numpy array, instead received an object of type {type(x)}.")
        import time
        clock = {"models": {}}
        t0 = time.time()
        n_prepared = self.preprocessor(self._suppress_noise_with_speex(x) if self.speex_ns else x)
        clock["models"]["preprocessor"] = time.time() - t0          # mel, embedding AND every head run in this one device call

        scores: dict = {}
        for name in self.models:
            t1 = time.time()
            out = self._raw_outputs(name, n_prepared)
            if self.model_outputs[name] == 1:
                scores[name] = out[0]
            else:
                scores.update({cls: out[int(idx)] for idx, cls in self.class_mapping[name].items()})
            if self.custom_verifier_models:
                self._apply_verifiers(scores, name)
            for label in scores:                                    # model.py:331-333: warm-up, first five frames
                if len(self.prediction_buffer[label]) < 5:
                    scores[label] = 0.0
            clock["models"][name] = time.time() - t1
        self._gate(scores, n_prepared, patience, threshold, debounce_time)
        for label, value in scores.items():                         # model.py:362-363
            self.prediction_buffer[label].append(value)
        if self.vad_threshold > 0:                                  # model.py:366-381: after the ring append, on the raw x
            t2 = time.time()
            self.vad(x)
            clock["models"]["vad"] = time.time() - t2
            from .vad import gate_value
            if gate_value(self.vad.prediction_buffer, self.vad_threshold):
                for label in scores:
                    scores[label] = 0.0
        return (scores, clock) if timing else scores

    # ---- conveniences on top of predict() --------------------------------------------------------------------------
    @staticmethod
    def _read_wav(path: str) -> np.ndarray:
        with wave.open(path, mode="rb") as f:
            return np.frombuffer(f.readframes(f.getnframes()), dtype=np.int16)

    def predict_clip(self, clip: Union[str, np.ndarray], padding: int = 1, chunk_size=1280, **kwargs):
        """Stream a whole clip through predict() (model.py:388-426): `padding` seconds of silence either side, calls of
        `chunk_size` samples; like the reference the final partial chunk (and one full one) is not fed."""
        data = self._read_wav(clip) if isinstance(clip, str) else clip
        if padding:
            silence = np.zeros(16000 * padding, dtype=np.int16)
            data = np.concatenate((silence, data, silence))
        starts = range(0, data.shape[0] - chunk_size, chunk_size)
        return [self.predict(data[o:o + chunk_size], **kwargs) for o in starts]

    def _get_positive_prediction_frames(self, file: str, threshold: float = 0.5, return_type: str = "features", **kwargs):
        """Features (or 4 s of audio) behind every frame scoring >= threshold (model.py:428-479; false-positive mining)."""
        data = self._read_wav(file)
        found = defaultdict(list)
        for o in range(0, data.shape[0] - CHUNK, CHUNK):
            for label, value in self.predict(data[o:o + CHUNK], **kwargs).items():
                if value < threshold:
                    continue
                if return_type == "features":
                    found[label].append(self.preprocessor.get_features(self.model_inputs[self.get_parent_model_from_label(label)]))
                elif return_type == "audio":
                    context = data[max(0, o - 3 * 16000):o + 16000]
                    if len(context) == 4 * 16000:
                        found[label].append(context)
        return {label: np.vstack(v) for label, v in found.items()}


class BatchedModel:
    """S independent streams behind one object: `predict_batch(pcm[S, 1280*k])` -> fp32 scores [S, n_labels].

    This is the many-stream form the reference lacks (one Python object per stream, utils.py:502-536 forks
    processes for scale-out).  Post-processing (first-5 zeroing, patience, debounce, 30-deep score ring) runs
    on the device per stream; `labels` names the score columns in `Model.predict`'s key order."""

    def __init__(self, n_streams: int, wakeword_models: Sequence[str], weights: Union[str, dict, None] = None,
                 device: int = 0, max_chunks: int = 1, hip_stream: int = 0, vad_weights: Optional[dict] = None,
                 vad_threshold: float = 0.0, use_mfma: Optional[int] = None, calibration_pcm="default",
                 embedding_model_path: str = "", melspec_model_path: str = "", bank_slots: int = 0, bank_capacity: int = 1024,
                 verifier_capacity: int = 0, event_capacity: int = 0, event_features: int = 0, audio_chunks: int = 0,
                 event_audio: int = 0):
        # bank_slots > 0: a head bank (bank_add / subscribe / bank_scores): every stream is scored by the bank heads it subscribed to,
        # up to bank_slots of them, beside the fixed `wakeword_models` (which may then be empty)
        # verifier_capacity > 0: a pool of per-stream custom verifiers (add_verifier / assign_verifiers / assign_bank_verifiers)
        # event_capacity > 0: detections as ordered device-side events, each with the stream's last event_features feature rows
        # (set_event_thresholds / events / event_features / event_label)
        # audio_chunks > 0: every stream's last audio_chunks chunks of 16 kHz audio stay on the device (the reference's raw_data_buffer
        # holds 125), every event with its stream's last event_audio chunks (audio / event_audio)
        if not wakeword_models and int(bank_slots) <= 0:
            raise ValueError("BatchedModel needs wakeword_models, or a head bank (bank_slots > 0)")
        check_event_config(event_capacity, event_features, 1 << 30)       # (the ring itself is known once the heads are loaded)
        check_audio_config(audio_chunks, event_audio, event_capacity)
        self._weights = weights
        self._debounce_frames = 0
        # same weight resolution as Model: real .onnx files (heads AND the shared embedding network) unless synthetic
        # weights are asked for explicitly -- never a random-init embedding under real heads
        seed, emb, given = resolve_weights(weights)
        heads = {}
        for m in wakeword_models:
            if m in given:
                heads[m] = given[m]
            else:
                name, head = _load_head(m, seed)
                heads[name] = head
        emb = resolve_embedding(emb, seed, embedding_model_path, melspec_model_path)       # (as Model: utils.py:38-44)
        # vad_weights: the on-device voice-activity network (weights.synthetic_vad layout) -- BASELINE configs[4]: network + gate
        # fused into every step.  With a gate asked for and no weights given, a silero_vad.onnx next to the package is ingested
        # when its graph is the architecture the kernels implement (onnx_ingest.load_vad); a graph it refuses, or no file, leaves
        # the gate to externally pushed scores (push_vad) -- said loudly, never a silently different network.
        if vad_weights is None and vad_threshold > 0:
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resources", "models", "silero_vad.onnx")
            if os.path.exists(path):
                from . import onnx_ingest
                try:
                    vad_weights = onnx_ingest.load_vad(path)
                except Exception as e:               # refused by name (ValueError) or unreadable in a way the reader did not foresee
                    import warnings
                    warnings.warn(f"{e} -- the VAD gate of this BatchedModel waits for push_vad() scores", RuntimeWarning)
        # calibration_pcm: audio of the deployment's domain for the commit-time calibration / self-test of the fp16-split kernels
        # (StreamEngine); "default" = speech shipped with the package
        self.engine = make_engine(n_streams, heads, emb, use_mfma, device=device, max_chunks=max_chunks, hip_stream=hip_stream,
                                  vad=vad_weights, vad_threshold=vad_threshold, calibration_pcm=calibration_pcm,
                                  bank_slots=int(bank_slots), bank_capacity=int(bank_capacity),
                                  verifier_capacity=int(verifier_capacity), event_capacity=int(event_capacity),
                                  event_features=int(event_features), audio_chunks=int(audio_chunks), event_audio=int(event_audio))
        self.event_capacity, self.event_rows = int(event_capacity), int(event_features)
        self.audio_chunks, self.event_audio_chunks = int(audio_chunks), int(event_audio)
        self.bank_slots = int(bank_slots)
        self.verifier_capacity = int(verifier_capacity)
        self._model_T = {n: int(h["T"]) for n, h in heads.items()}
        self._verifier_T: Dict[int, int] = {}
        self.labels: List[str] = []
        self._keep: List[int] = []
        col = 0
        for n, h in heads.items():
            if h["n_out"] == 1:
                self.labels.append(n)
                self._keep.append(col)
            else:
                for int_label, cls in model_class_mappings.get(n, {str(j): str(j) for j in range(h["n_out"])}).items():
                    self.labels.append(cls)
                    self._keep.append(col + int(int_label))
            col += h["n_out"]
        self._event_thr = np.full(self.engine.n_labels, 0.5, dtype=np.float32)
        self._parent = {}
        col = 0
        for n, h in heads.items():
            for j in range(h["n_out"]):
                self._parent[col + j] = n
            col += h["n_out"]
        self.n_streams = n_streams

    def set_postproc(self, patience: dict = {}, threshold: dict = {}, debounce_time: float = 0.0, chunk_samples: int = 1280):
        """Same rules and errors as Model.predict's keyword arguments (model.py:340-359), applied to every stream."""
        if patience != {} or debounce_time > 0:
            if threshold == {}:
                raise ValueError("Error! When using the `patience` argument, threshold "
                                 "values must be provided via the `threshold` argument!")
            if patience != {} and debounce_time > 0:
                raise ValueError("Error! The `patience` and `debounce_time` arguments cannot be used together!")
        NL = self.engine.n_labels
        pat = [int(patience.get(self._parent[c], 0)) for c in range(NL)]
        thr = [float(threshold.get(self._parent[c], np.nan)) for c in range(NL)]
        frames = int(np.ceil(debounce_time / (chunk_samples / 16000))) if debounce_time > 0 else 0
        self.engine.set_postproc(pat, thr, frames)
        self._debounce_frames = frames

    def score_clips(self, clips: np.ndarray, return_features: bool = False):
        """Dense scores of equally long clips: int16 [B, n] -> {label: [B, n_win]}, one raw score per 80 ms window position of every
        clip (model.py:428-479 scans long audio like this, one window at a time).  Window w ends at embedding row w + t_max - 1 of the
        clip, t_max the longest window of the fixed models.  Batches larger than the stream count run in several calls.  These are
        embed_clips-path scores: one mel clamp floor per clip, no seeded feature ring and no post-processing -- not the streaming path's.
        With return_features also the embeddings [B, n_out, 96]."""
        clips = np.ascontiguousarray(np.atleast_2d(clips))
        cap = self.engine.n_streams_padded
        parts = [self.engine.score_clips(clips[lo:lo + cap], return_features=True) for lo in range(0, clips.shape[0], cap)]
        raw = np.concatenate([p[0] for p in parts], axis=0)
        out = {lab: raw[:, :, c] for lab, c in zip(self.labels, self._keep)}
        return (out, np.concatenate([p[1] for p in parts], axis=0)) if return_features else out

    # ---- dense scoring: ordered hit lists (include/owwhip.h: oww_score_hits, oww_score_clip_hits, oww_bank_score_hits) ----
    def _label_thresholds(self, threshold):
        """A number, or {label: value} (labels not named: 0.5) -> one threshold per score column of the engine."""
        if not isinstance(threshold, dict):
            return threshold
        thr = np.full(self.engine.n_labels, 0.5, dtype=np.float32)
        for lab, v in threshold.items():
            thr[self._keep[self.labels.index(lab)]] = np.float32(v)
        return thr

    def score_hits(self, feats: np.ndarray, threshold=0.5, cap: int = 4096, return_windows: bool = True) -> Dict[str, dict]:
        """The frames of feature sequences [B, n_rows, 96] that score at least `threshold` (a number, or {label: value}), found on the
        device (Model._get_positive_prediction_frames, model.py:428-479) -> {label: {"seq", "window", "score", "n_total",
        "windows"}}: positions in ascending (seq, window) order, the first `cap` of them per label; their raw scores; the count without
        the cap; and each hit's own [T, 96] feature window.  The score matrix is never written."""
        cols = self.engine.score_hits(feats, self._label_thresholds(threshold), cap, return_windows)
        return {lab: cols[c] for lab, c in zip(self.labels, self._keep)}

    def score_clip_hits(self, clips: np.ndarray, threshold=0.5, cap: int = 4096, return_windows: bool = True) -> Dict[str, dict]:
        """score_hits over equally long int16 clips [B, n], as score_clips scores them: the embeddings stay on the device, only the
        hits and their windows come back.  Batches larger than the stream count run in several calls; `seq` counts over all clips and
        `cap` bounds the merged list of a label."""
        clips = np.ascontiguousarray(np.atleast_2d(clips))
        per = self.engine.n_streams_padded
        thr = self._label_thresholds(threshold)
        out: Dict[str, dict] = {}
        for lo in range(0, clips.shape[0], per):
            cols = self.engine.score_clip_hits(clips[lo:lo + per], thr, cap, return_windows)
            for lab, c in zip(self.labels, self._keep):
                col = cols[c]
                col["seq"] = col["seq"] + np.int32(lo)
                if lab not in out:
                    out[lab] = col
                    continue
                acc = out[lab]
                room = max(int(cap) - acc["seq"].size, 0)
                for k in ("seq", "window", "score") + (("windows",) if return_windows else ()):
                    acc[k] = np.concatenate([acc[k], col[k][:room]], axis=0)
                acc["n_total"] += col["n_total"]
        return out

    def bank_score_hits(self, feats: np.ndarray, ids: Sequence[int], thresholds=None, cap: int = 4096, return_windows: bool = True) -> List[dict]:
        """score_hits over the listed bank heads: one dict per listed id, in the list's order (None thresholds = 0.5, train.py:100).
        Says where a head false-accepts and on what, where bank_score_stats says how often."""
        return self.engine.bank_score_hits(feats, ids, thresholds, cap, return_windows)

    # ---- head bank: per-stream subscriptions to wake-word heads (include/owwhip.h: oww_bank_*) ----
    def bank_add(self, model: Union[str, dict], weights: Union[str, dict, None] = None) -> int:
        """Add a head to the bank while the streams run -> bank id.  `model` is resolved like an entry of `wakeword_models`: a
        pretrained name, an .onnx path (onnx_ingest.load_head), or a head dict; `weights` as in the constructor (default: the
        constructor's).  A bank head is binary (one sigmoid output), ungated, with one hidden block of <= 128 units and T <= the
        handle's feature ring; other forms raise ValueError (they remain available as fixed heads)."""
        if isinstance(model, dict):
            head = model
        else:
            seed, _, given = resolve_weights(self._weights if weights is None else weights)
            head = given[model] if model in given else _load_head(model, seed)[1]
        check_bank_head(head, self.engine.feature_ring)
        return self.engine.bank_add(head)

    def head_trainer(self, T: int, hidden: int, n_problems: int, init: Optional[Sequence[dict]] = None, seed: int = 0):
        """A training session for `n_problems` bank heads of T feature rows and `hidden` units on this model's device (train.HeadTrainer:
        set_pool, steps(idx, y, lr, neg_weight), history, heads() -> dicts for bank_add, close()): the step of train.py:434-510, many
        heads per call.  `init`: one head dict per problem (default: train.init_head(T, hidden, seed + u)).  One session per model."""
        from .train import HeadTrainer
        return HeadTrainer(self.engine, T, hidden, n_problems, init=init, seed=seed)

    def bank_remove(self, bank_id: int) -> None:
        """Drop a bank head; the slots subscribed to it become empty (score 0)."""
        self.engine.bank_remove(bank_id)

    def subscribe(self, stream_ids: Sequence[int], bank_ids) -> None:
        """bank_ids [len(stream_ids), bank_slots]: the bank heads of each listed stream, -1 = empty slot.  A slot whose head changes
        starts afresh (an empty prediction buffer, as a model newly loaded into that stream's Model); nothing else of the stream moves."""
        if self.bank_slots <= 0:
            raise ValueError("this BatchedModel has no head bank (bank_slots = 0)")
        ids = np.asarray(stream_ids)
        b = np.asarray(bank_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("stream_ids must be a 1-D integer sequence")
        if b.dtype.kind not in "iu" or b.shape != (ids.size, self.bank_slots):
            raise ValueError(f"bank_ids must be an integer array of shape ({ids.size}, {self.bank_slots}), got {b.dtype} {b.shape}")
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.n_streams):
            raise ValueError(f"stream ids must lie in 0 .. {self.n_streams - 1}")
        if b.size and int(b.min()) < -1:
            raise ValueError("bank ids are >= 0, or -1 for an empty slot")
        self.engine.subscribe(ids, b)

    def set_bank_postproc(self, bank_id: int, patience: int = 0, threshold: Optional[float] = None) -> None:
        """Model.predict's `patience` / `threshold` for one bank head, with the same errors (model.py:340-345); the debounce time
        is the one of set_postproc, shared with the fixed heads."""
        if patience and threshold is None:
            raise ValueError("Error! When using the `patience` argument, threshold "
                             "values must be provided via the `threshold` argument!")
        if patience and self._debounce_frames > 0:
            raise ValueError("Error! The `patience` and `debounce_time` arguments cannot be used together!")
        self.engine.bank_set_postproc(bank_id, int(patience), float("nan") if threshold is None else float(threshold))

    def bank_scores(self) -> np.ndarray:
        """float32 [n_streams, bank_slots]: the post-processed bank scores of the last predict_batch / predict_active /
        collect_batch (an empty slot reads 0.0)."""
        return self.engine.bank_scores()

    # ---- dense scoring over the bank: validate heads on a corpus (include/owwhip.h: oww_bank_score_*) ----
    def bank_score_shape(self, ids: Sequence[int], n_rows: int):
        """(n_win, t_max) of sequences of n_rows feature rows under the listed bank heads (t_max = their longest window)."""
        return self.engine.bank_score_shape(ids, n_rows)

    def bank_score_features(self, feats: np.ndarray, ids: Sequence[int]) -> np.ndarray:
        """Every window of feature sequences [B, n_rows, 96] through the listed bank heads -> raw scores [B, n_win, n_ids]; window w
        ends at row w + t_max - 1 and each head reads its own last T rows.  The live streams and their subscriptions do not notice."""
        return self.engine.bank_score_features(feats, ids)

    def bank_score_stats(self, feats: np.ndarray, ids: Sequence[int], thresholds: Optional[Sequence[float]] = None) -> Dict[str, np.ndarray]:
        """{"count", "max", "argmax"}, each [B, n_ids]: the windows with score >= thresholds[i] (None = 0.5, train.py:100), the
        largest score and the first window that attains it -- reduced on the device, the score matrix is never written."""
        return self.engine.bank_score_stats(feats, ids, thresholds)

    # ---- detection events: the hits of a call as ordered records with feature snapshots (include/owwhip.h: oww_events_*) ----
    def set_event_thresholds(self, thresholds: Optional[dict] = None, bank: Optional[float] = None) -> None:
        """Event thresholds by label ({label: value}; labels not named keep theirs, NaN = the label never reports) and for the bank
        slots (`bank`; None = keep).  Default 0.5 everywhere."""
        if self.event_capacity <= 0:
            raise ValueError("this BatchedModel reports no events (event_capacity = 0)")
        thresholds = thresholds or {}
        unknown = [k for k in thresholds if k not in self.labels]
        if unknown:
            raise ValueError(f"unknown labels {unknown}; this model's labels are {self.labels}")
        for label, v in thresholds.items():
            self._event_thr[self._keep[self.labels.index(label)]] = np.float32(v)
        self.engine.set_event_thresholds(self._event_thr if thresholds else None, bank)

    def events(self) -> Tuple[np.ndarray, int]:
        """(records, n_total) of the last predict_batch / predict_active / collect_batch: a structured array (engine.EVENT_DTYPE:
        stream, column, bank_id, score, frame, feature_index) of the stored detections in ascending (stream, column, slot) order, and
        the number of detections the call had; fewer records than that = the call overflowed event_capacity."""
        return self.engine.events()

    def event_features(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """float32 [n, event_features, 96]: the feature window behind stored events first .. first + n - 1, taken on the device in the
        step that detected (what Model._get_positive_prediction_frames collects, model.py:428-476)."""
        return self.engine.event_features(first, n)

    def audio(self, stream_ids: Sequence[int], n_chunks: int) -> Tuple[np.ndarray, np.ndarray]:
        """(int16 [n, n_chunks * 1280], uint32 counts [n]): the newest n_chunks chunks of 16 kHz audio of the listed streams, oldest
        first, zero where a stream has received less since its reset, and the chunks each has received (needs audio_chunks > 0)."""
        return self.engine.audio(stream_ids, n_chunks)

    def event_audio(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """int16 [n, event_audio * 1280]: the audio behind stored events first .. first + n - 1, taken on the device in the detecting
        step and ending with the detecting chunk."""
        return self.engine.event_audio(first, n)

    check_audio_config = staticmethod(check_audio_config)

    def event_label(self, record) -> Union[str, int]:
        """The label of a fixed-head event (as in `labels`), the bank id of a bank event."""
        col = int(record["column"])
        if col < 0:
            return int(record["bank_id"])
        if col in self._keep:
            return self.labels[self._keep.index(col)]
        return self.engine.event_label(record)

    # ---- stream state records: a live stream's state as a portable record (include/owwhip.h: oww_state_*, oww_move_streams) ----
    def _stream_ids(self, ids, what: str = "stream_ids") -> np.ndarray:
        a = np.asarray(ids)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError(f"{what} must be a 1-D integer sequence")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= self.n_streams):
            raise ValueError(f"stream ids must lie in 0 .. {self.n_streams - 1}")
        return a

    def export_streams(self, stream_ids: Sequence[int]) -> np.ndarray:
        """uint8 [len(stream_ids), record_bytes]: everything the listed streams' future scores depend on (in the reference: the
        stream's Model object, model.py:226-230, utils.py:163-171).  Records are only meaningful to a BatchedModel with the same
        kernel family, ring sizes, bank slots, VAD and weights (engine.state_info's fingerprint; import refuses any other)."""
        return self.engine.export_state(self._stream_ids(stream_ids))

    def import_streams(self, stream_ids: Sequence[int], records: np.ndarray) -> None:
        """Put exported records into the listed streams: each continues bit for bit where its source stopped.  Subscriptions and
        verifier assignments are not part of a record: subscribe() first (which restarts the slot), then import."""
        ids = self._stream_ids(stream_ids)
        if not isinstance(records, np.ndarray) or records.dtype != np.uint8:
            raise ValueError(f"records must be a uint8 array (export_streams), got {getattr(records, 'dtype', type(records).__name__)}")
        nb = self.engine.state_info()[0]
        if records.ndim != 2 or records.shape != (ids.size, nb):
            raise ValueError(f"records must have shape ({ids.size}, {nb}), got {records.shape}")
        if np.unique(ids).size != ids.size:
            raise ValueError("stream_ids holds a stream twice")
        self.engine.import_state(ids, records)

    def move_streams(self, src: Sequence[int], dst: Sequence[int]) -> None:
        """Stream src[i] becomes stream dst[i] inside this model: state, bank subscriptions and verifier assignments travel; swaps,
        cycles and chains are legal (all reads happen before any write), `dst` holds no duplicates.  Source slots that are nobody's
        destination keep their device state (reset() them when they are reused) and end up unsubscribed."""
        s, d = self._stream_ids(src, "src"), self._stream_ids(dst, "dst")
        if s.size != d.size:
            raise ValueError(f"src and dst must have the same length ({s.size} != {d.size})")
        if np.unique(d).size != d.size:
            raise ValueError("dst holds a stream twice")
        self.engine.move_streams(s, d)

    def reset(self, stream_ids: Optional[Sequence[int]] = None, init_features: Optional[np.ndarray] = None,
              reset_vad: bool = False):
        """Model.reset for the listed streams (None = all).  Like the reference (model.py:226-230) this leaves the VAD state
        alone; pass reset_vad=True when a stream slot is handed to a NEW caller, so that it does not inherit the previous
        caller's voice-activity history."""
        self.engine.reset(stream_ids, init_features)
        if reset_vad:
            self.engine.reset_vad(stream_ids)

    def predict_batch(self, pcm: np.ndarray, sample_rate: int = 16000) -> np.ndarray:
        """`sample_rate` != 16000: every stream's message is converted on the device first (engine.resample; e.g. 640 samples at 8 kHz,
        3840 at 48 kHz or 3528 at 44.1 kHz make one 1280-sample chunk)."""
        if not isinstance(pcm, np.ndarray):
            raise ValueError(f"The input audio data (x) must by a Numpy array, instead received an object of type {type(pcm)}.")
        if int(sample_rate) != 16000:
            pcm = self.engine.resample(pcm, sample_rate)
        return self.engine.step(pcm)[:, self._keep]

    def configure_ingest(self, sample_rate: int, encoding: str = "pcm16") -> None:
        """Streams that arrive as `encoding` ("pcm16", "ulaw", "alaw") at `sample_rate` Hz: decode and continuous rate conversion per
        stream on the device (engine.configure_ingest); feed them with predict_ingest."""
        self.engine.configure_ingest(sample_rate, encoding)

    def predict_ingest(self, data: np.ndarray, active=None) -> np.ndarray:
        """predict_batch on one encoded message per stream (e.g. uint8 [n_streams, 640] of 8 kHz G.711 = one 80 ms step).  Unlike
        predict_batch(sample_rate=...), the conversion filter runs on across messages, so no frame starts or ends in its transient;
        `active` ([n_streams] bool): only those streams are fed, as in predict_active."""
        if not isinstance(data, np.ndarray):
            raise ValueError(f"The input audio data (x) must by a Numpy array, instead received an object of type {type(data)}.")
        return self.engine.step_ingest(data, active)[:, self._keep]

    def configure_ingest_classes(self, formats) -> None:
        """Streams in different formats on one model: `formats` is a list of (sample_rate, encoding), at most 16 (engine.
        configure_ingest_classes).  Every stream starts in class 0; assign_ingest moves it, predict_ingest_mixed feeds all of them."""
        self.engine.configure_ingest_classes(formats)

    def assign_ingest(self, stream_ids, class_ids) -> None:
        """The listed streams take the listed classes and start from silence."""
        self.engine.assign_ingest(stream_ids, class_ids)

    def predict_ingest_mixed(self, rows: np.ndarray, active=None) -> np.ndarray:
        """predict_ingest with every stream in its own class: rows uint8 [n_streams, row_bytes] (engine.pack_ingest_rows), one 80 ms
        message per stream in the stream's own format; `active` as in predict_ingest."""
        if not isinstance(rows, np.ndarray):
            raise ValueError(f"The input audio data (x) must by a Numpy array, instead received an object of type {type(rows)}.")
        return self.engine.step_ingest_mixed(rows, stream_on=active)[:, self._keep]

    def submit_ingest_mixed(self, rows: np.ndarray, active=None) -> None:
        """Pipelined predict_ingest_mixed, beside submit_batch: the scores come back from collect_batch() in submission order."""
        if not isinstance(rows, np.ndarray):
            raise ValueError(f"The input audio data (x) must by a Numpy array, instead received an object of type {type(rows)}.")
        self.engine.submit_ingest_mixed(rows, active)

    def predict_active(self, pcm: np.ndarray, active) -> np.ndarray:
        """predict_batch for the streams flagged in `active` ([n_streams] bool) only; the others do not advance at all and
        repeat their previous scores (the reference's per-client behaviour: no audio, no predict() call)."""
        if not isinstance(pcm, np.ndarray):
            raise ValueError(f"The input audio data (x) must by a Numpy array, instead received an object of type {type(pcm)}.")
        return self.engine.step_masked(pcm, active)[:, self._keep]

    def set_custom_verifier(self, model_name: str, verifier, threshold: float = 0.1) -> None:
        """`Model(custom_verifier_models=..., custom_verifier_threshold=...)` for every stream, on the device (model.py:320-328).
        `verifier` is the scikit-learn pipeline custom_verifier_model.train_verifier_model returns (flatten -> StandardScaler ->
        LogisticRegression; custom_verifier_model.py:95-113), or an already folded (w [T*96], bias) pair, or None to remove it.
        Anything else -- an arbitrary object with predict_proba -- cannot run on the device: use the single-stream Model, which
        keeps the reference's host-side hook."""
        if model_name not in self._parent.values():
            raise ValueError("Custom verifier models were provided, but some were not matched with a base model!")
        cols = [c for c, n in self._parent.items() if n == model_name]
        if verifier is None:
            for c in cols:
                self.engine.set_verifier(c, None)
            return
        w, b = fold_verifier(verifier)
        for c in cols:
            self.engine.set_verifier(c, w, b, threshold)

    # ---- per-stream custom verifiers (include/owwhip.h: oww_verifier_*) ----
    def add_verifier(self, verifier) -> int:
        """Put one user's custom verifier into the pool -> verifier id.  `verifier` is what set_custom_verifier takes: the reference's
        scikit-learn pipeline (custom_verifier_model.py:95-113) or a folded (w [T*96], bias) pair.  Needs verifier_capacity > 0."""
        if self.verifier_capacity <= 0:
            raise ValueError("this BatchedModel has no verifier pool (verifier_capacity = 0)")
        w, b = fold_verifier(verifier)
        if w.size == 0 or w.size % 96:
            raise ValueError(f"a verifier has T x 96 weights, got {w.size}")
        T = w.size // 96
        if T > self.engine.feature_ring:
            raise ValueError(f"the verifier reads T = {T} feature rows, more than the feature ring holds ({self.engine.feature_ring})")
        vid = self.engine.verifier_add(w, b)
        self._verifier_T[vid] = T
        return vid

    def fit_verifiers(self, features, labels, C: float = 0.001) -> List[int]:
        """custom_verifier_model.train_verifier_model (custom_verifier_model.py:95-113: flatten -> StandardScaler ->
        LogisticRegression(C)) on the device, for one user or many in one call: `features` one [N, T, 96] array with `labels` [N] in
        {0, 1}, or lists of them -> the pool ids of the fitted verifiers, ready for assign_verifiers.  What is fitted is the optimum
        of scikit-learn's objective, N = 2 .. 1024 windows per user.  Raises ValueError with scikit-learn's wording
        where it would raise (one class; NaN or infinity); any other failure names the status."""
        if self.verifier_capacity <= 0:
            raise ValueError("this BatchedModel has no verifier pool (verifier_capacity = 0)")
        single = isinstance(features, np.ndarray) and features.ndim == 3
        feats = [features] if single else list(features)
        labs = [labels] if single else list(labels)
        if len(feats) != len(labs) or not feats:
            raise ValueError(f"{len(feats)} feature arrays and {len(labs)} label arrays")
        feats = [np.ascontiguousarray(f, dtype=np.float32) for f in feats]
        labs = [np.asarray(y).ravel() for y in labs]
        T = feats[0].shape[1] if feats[0].ndim == 3 else 0
        for f, y in zip(feats, labs):
            if f.ndim != 3 or f.shape[1] != T or f.shape[2] != 96 or y.size != f.shape[0]:
                raise ValueError(f"features must be [N, {T}, 96] with N labels each, got {f.shape} and {y.size} labels")
            if y.size and not np.isin(y, (0, 1)).all():
                raise ValueError("labels must be 0 or 1")
        if not 1 <= T <= self.engine.feature_ring:
            raise ValueError(f"the verifiers read T = {T} feature rows, the feature ring holds {self.engine.feature_ring}")
        off = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])]).astype(np.int64)
        res = self.engine.verifier_fit(np.concatenate(feats, axis=0), off, np.concatenate(labs).astype(np.uint8), T, C)
        bad = [(u, r) for u, r in enumerate(res) if r["status"] != 0]
        for r in res:
            if r["status"] == 0:
                self._verifier_T[r["id"]] = T
        if bad:
            u, r = bad[0]
            name = FIT_STATUS[r["status"]]
            if name == "ONE_CLASS":
                cls = 1 if r["n_pos"] else 0
                raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: {cls} (problem {u})")
            if name == "NONFINITE":
                raise ValueError(f"Input X contains NaN or infinity. (problem {u})")
            raise ValueError(f"verifier fit of problem {u} failed: {name} (N = {int(off[u + 1] - off[u])}, {r['iterations']} iterations, residual {r['residual']:.3g}); "
                             f"{len(res) - len(bad)} of {len(res)} problems were fitted")
        return [r["id"] for r in res]

    def get_verifier(self, verifier_id: int) -> Tuple[np.ndarray, float]:
        """Pool verifier read back from the device: the folded (w [T*96] fp32, bias) pair add_verifier takes."""
        if int(verifier_id) not in self._verifier_T:
            raise ValueError(f"{verifier_id} is not a verifier of this BatchedModel's pool")
        return self.engine.verifier_get(int(verifier_id), self._verifier_T[int(verifier_id)])

    def remove_verifier(self, verifier_id: int) -> None:
        """Drop a pool verifier; every stream assigned to it falls back to the default (the handle-wide set_custom_verifier)."""
        if int(verifier_id) not in self._verifier_T:
            raise ValueError(f"{verifier_id} is not a verifier of this BatchedModel's pool")
        self.engine.verifier_remove(int(verifier_id))
        del self._verifier_T[int(verifier_id)]

    def _verifier_args(self, stream_ids, verifier_ids, threshold, T: Optional[int]):
        ids = np.asarray(stream_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("stream_ids must be a 1-D integer sequence")
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.n_streams):
            raise ValueError(f"stream ids must lie in 0 .. {self.n_streams - 1}")
        v = np.asarray(verifier_ids)
        if v.dtype.kind not in "iu" or v.ndim > 1 or (v.ndim == 1 and v.size != ids.size):
            raise ValueError(f"verifier_ids must be one integer or {ids.size} of them, got {v.dtype} {v.shape}")
        v = np.broadcast_to(v, ids.shape).astype(np.int64)
        if v.size and int(v.min()) < -2:
            raise ValueError("verifier ids are >= 0, or -1 (default) / -2 (none)")
        for x in np.unique(v[v >= 0]):
            if int(x) not in self._verifier_T:
                raise ValueError(f"{int(x)} is not a verifier of this BatchedModel's pool")
            if T is not None and self._verifier_T[int(x)] != T:
                raise ValueError(f"verifier {int(x)} reads T = {self._verifier_T[int(x)]} feature rows, the model has T = {T}")
        t = np.asarray(threshold)
        if t.dtype.kind not in "iuf" or t.ndim > 1 or (t.ndim == 1 and t.size != ids.size):
            raise ValueError(f"threshold must be one number or {ids.size} of them, got {t.dtype} {t.shape}")
        return ids, v, np.broadcast_to(t, ids.shape).astype(np.float32)

    def assign_verifiers(self, stream_ids: Sequence[int], model_name: str, verifier_ids, threshold=0.1) -> None:
        """`Model(custom_verifier_models={model_name: ...}, custom_verifier_threshold=threshold)` per stream: the listed streams'
        columns of `model_name` (every class of a multiclass model) are re-scored by their own pool verifier.  verifier_ids /
        threshold: one value or one per stream; id -1 = the model's set_custom_verifier setting (if any), -2 = no verifier at all."""
        if self.verifier_capacity <= 0:
            raise ValueError("this BatchedModel has no verifier pool (verifier_capacity = 0)")
        if model_name not in self._parent.values():
            raise ValueError("Custom verifier models were provided, but some were not matched with a base model!")
        ids, v, t = self._verifier_args(stream_ids, verifier_ids, threshold, self._model_T[model_name])
        for c in [c for c, n in self._parent.items() if n == model_name]:
            self.engine.assign_verifiers(c, ids, v, t)

    def assign_bank_verifiers(self, stream_ids: Sequence[int], slot: int, verifier_ids, threshold=0.1) -> None:
        """assign_verifiers for bank slot `slot` of the listed streams (the slot must hold a head whose T matches; a slot whose head
        changes drops its verifier); id -1 and -2 both mean none here."""
        if self.verifier_capacity <= 0:
            raise ValueError("this BatchedModel has no verifier pool (verifier_capacity = 0)")
        if self.bank_slots <= 0:
            raise ValueError("this BatchedModel has no head bank (bank_slots = 0)")
        if not 0 <= int(slot) < self.bank_slots:
            raise ValueError(f"slot {slot} outside 0 .. {self.bank_slots - 1}")
        ids, v, t = self._verifier_args(stream_ids, verifier_ids, threshold, None)
        self.engine.assign_verifiers(int(slot), ids, v, t, bank=True)

    def verifier_stats(self) -> Tuple[int, int]:
        """(pairs of (stream, column / slot) with a per-stream assignment, verifier evaluations of the last step)."""
        return self.engine.verifier_stats()

    def set_vad_threshold(self, threshold: float) -> None:
        """The VAD gate of `Model(vad_threshold=...)` (model.py:366-381) for every stream; 0 switches it off."""
        self.engine.set_vad_threshold(threshold)

    def push_vad(self, vad_scores: np.ndarray) -> None:
        """Voice-activity score of each stream for the frame about to be predicted (the value `VAD.__call__` appends to its
        ring, vad.py:98-130); the network that produces it is the caller's (see openwakeword_amd.vad)."""
        self.engine.push_vad(vad_scores)

    def submit_batch(self, pcm: np.ndarray) -> None:
        """Pipelined `predict_batch` for host-fed serving: enqueue one step (upload on its own stream) and return; the
        scores come back from `collect_batch()` in submission order, at most two steps in flight.  Page-locked buffers
        (`engine.pinned_empty`) make the upload overlap the previous step's kernels."""
        if not isinstance(pcm, np.ndarray):
            raise ValueError(f"The input audio data (x) must by a Numpy array, instead received an object of type {type(pcm)}.")
        self.engine.submit(pcm)

    def collect_batch(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        return self.engine.collect(out)[:, self._keep]

    def close(self):
        self.engine.close()
