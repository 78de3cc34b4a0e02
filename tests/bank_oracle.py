"""Float64 reference of the head bank (include/owwhip.h: oww_bank_*), composed only of oracle/oww_oracle.py pieces: one
OracleAudioFeatures per stream, head_stage per subscribed bank head, and Model.predict's post-processing (model.py:330-363) per
(stream, slot) with the slot's own 30-deep ring, which restarts when the slot's head changes."""
from collections import deque
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from oracle import oww_oracle as O

CHUNK = 1280


class BankOracle:
    """One stream: K slots, each subscribed to a bank head id (-1 = empty) of `bank` (id -> head dict)."""

    def __init__(self, bank: Dict[int, dict], emb: dict, K: int, dtype=np.float64, init_noise: Optional[np.ndarray] = None,
                 features: Optional[np.ndarray] = None):
        self.bank = bank
        self.dtype = dtype
        self.K = K
        self.preprocessor = O.OracleAudioFeatures(emb, dtype=dtype, init_noise=init_noise)
        if features is not None:                      # (a precomputed clip_embeddings of the same init noise)
            self.preprocessor.features = np.array(features, copy=True)
        self.sub = [-1] * K
        self.rings = [deque(maxlen=30) for _ in range(K)]

    def subscribe(self, ids: Sequence[int]) -> None:
        for k, b in enumerate(ids):
            if int(b) != self.sub[k]:                 # a model newly loaded into this stream's Model: empty prediction_buffer
                self.sub[k] = int(b)
                self.rings[k] = deque(maxlen=30)

    def reset(self) -> None:                          # model.py:226-230: the loaded models (subscriptions) stay
        self.preprocessor.reset()
        self.rings = [deque(maxlen=30) for _ in range(self.K)]

    def predict(self, x: np.ndarray, post: Dict[int, Tuple[int, float]] = {}, debounce_frames: int = 0):
        """-> (raw [K], scores [K]); post: bank id -> (patience, threshold); debounce_frames shared by every slot."""
        n_ready = self.preprocessor(x)
        raw = np.zeros(self.K)
        out = np.zeros(self.K)
        for k in range(self.K):
            b = self.sub[k]
            if b < 0:
                continue
            head = self.bank[b]
            T = int(head["T"])
            if n_ready > CHUNK:                                                  # model.py:287-298
                r = max(float(O.head_stage(self.preprocessor.get_features(T, start_ndx=-T - back), head, self.dtype)[0, 0])
                        for back in range(n_ready // CHUNK - 1, -1, -1))
            else:                                                                # model.py:299-302
                r = float(O.head_stage(self.preprocessor.get_features(T), head, self.dtype)[0, 0])
            raw[k] = r
            ring = self.rings[k]
            sc = 0.0 if len(ring) < 5 else r                                     # model.py:331-333
            pat, thr = post.get(b, (0, float("nan")))
            if sc != 0.0:                                                        # model.py:340-359
                if pat > 0:
                    hist = np.array(ring)[-pat:]
                    if (hist >= thr).sum() < pat:
                        sc = 0.0
                elif debounce_frames > 0 and thr == thr:
                    hist = np.array(ring)[-debounce_frames:]
                    if sc >= thr and (hist >= thr).sum() > 0:
                        sc = 0.0
            ring.append(sc)                                                      # model.py:362-363
            out[k] = sc
        return raw, out
