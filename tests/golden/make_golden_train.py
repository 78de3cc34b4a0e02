"""Writes tests/golden/head_train.npz: the reference's own train.Model.train_model (imported from the reference checkout with stand-in
modules for its training-only imports, tests/head_train_ref.py: run_reference) run in fp32, as it stands, on the batches of every
case of the table with T <= 2.  Per case: the final parameters as flat records [U, n], history["loss"] laid out per step [U, K] (NaN
where no optimizer step was taken) and the kept count of every step [U, K].

    python tests/golden/make_golden_train.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import head_train_ref as R  # noqa: E402


def main(out):
    arrays = {}
    for name in R.GOLDEN_CASES:
        ref = R.run_reference(R.make_case(name))
        if ref is None:
            raise SystemExit(f"no reference checkout at {R.REFERENCE}")
        arrays[name + "/params"] = ref["params"].astype(np.float32)
        arrays[name + "/loss"] = ref["loss"].astype(np.float32)
        arrays[name + "/kept"] = ref["kept"].astype(np.int32)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {len(R.GOLDEN_CASES)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else R.GOLDEN)
