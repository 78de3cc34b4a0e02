"""Custom verifier training on the device: the reference's custom_verifier_model.py with the fit (custom_verifier_model.py:95-113:
flatten -> StandardScaler -> LogisticRegression(C=0.001)) done by oww_verifier_fit for one user or for many at once.  The result is
not a scikit-learn pipeline but a verifier in the BatchedModel's pool -- a pool id for assign_verifiers; get_verifier(id) reads the
folded (w, bias) pair back.  What is fitted is the optimum of scikit-learn's objective; its own iterate at the default tol = 1e-4
sits up to 1e-3 in score from that optimum."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def flatten_features(x):                        # custom_verifier_model.py:91-92
    return [i.flatten() for i in x]


def train_verifier_model(features: np.ndarray, labels: np.ndarray, model=None, C: float = 0.001) -> int:
    """custom_verifier_model.train_verifier_model (custom_verifier_model.py:95-113) on the device: `features` [N, T, 96], `labels` [N]
    in {0, 1}, `model` the BatchedModel whose pool takes the verifier -> its pool id."""
    if model is None:
        raise ValueError("train_verifier_model needs model=<a BatchedModel with verifier_capacity > 0>: the verifier is fitted on its device")
    return model.fit_verifiers(np.asarray(features), np.asarray(labels), C=C)[0]


def train_custom_verifiers(bm, model_name: str, users: Sequence[Tuple[np.ndarray, np.ndarray]], C: float = 0.001) -> List[int]:
    """custom_verifier_model.train_custom_verifier (custom_verifier_model.py:116-177) for many users in one fit: `users` holds one
    (positive_clips, negative_clips) pair of equally long int16 clip arrays [B, n] per user.  As in the reference, the positive
    windows are those where `model_name` scores >= 0.5 on a positive clip and the negative windows are every window of the negative
    clips (threshold 0.0); they are captured with score_clip_hits and all users are fitted by one oww_verifier_fit -> one pool id per
    user.  These are windows of the bulk path (embed_clips: every clip embedded on its own, left-aligned), not of the streaming
    feature ring, exactly as mine_windows' docstring says; and where the reference draws N random start offsets per clip, the caller
    supplies them as shifted copies of the clips.  A user needs 2 .. 1024 windows in all, of both classes."""
    if model_name not in bm.labels and model_name not in getattr(bm, "_parent", {}).values():
        raise ValueError(f"{model_name} is not a model of this BatchedModel")
    feats, labs = [], []
    for u, (pos, neg) in enumerate(users):
        p = bm.score_clip_hits(np.asarray(pos), threshold=0.5)[model_name]["windows"]
        n = bm.score_clip_hits(np.asarray(neg), threshold=0.0)[model_name]["windows"]
        if p.shape[0] == 0:                     # custom_verifier_model.py:140-143
            raise ValueError(f"The positive features were created with no samples! Make sure that the positive clips of user {u} contain the wake word")
        if n.shape[0] == 0:
            raise ValueError(f"The negative features were created with no samples (user {u})")
        feats.append(np.concatenate([p, n], axis=0))
        labs.append(np.concatenate([np.ones(p.shape[0], np.uint8), np.zeros(n.shape[0], np.uint8)]))
    return bm.fit_verifiers(feats, labs, C=C)
