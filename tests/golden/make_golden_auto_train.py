"""Writes tests/golden/auto_train.npz: per end-to-end case of tests/auto_train_ref.py and per problem, what the reference's own
train.Model.auto_train (fp32, CPU) left on the case's batches -- the validation histories, the (sequence, step) of every validation
and of every checkpoint, the selected set, the five counts of every validation, the kept counts and step decisions, and the final
record.  Results only: the inputs are regenerated from seeds by the case module.  Needs the reference checkout (OWW_REFERENCE_DIR).

    python tests/golden/make_golden_auto_train.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import auto_train_ref as A  # noqa: E402
from test_auto_train_cpu import golden_entries  # noqa: E402


def main():
    out = {}
    for name in A.GOLDEN_CASES:
        run = A.run_reference_auto_train(A.make_e2e_case(name), double=False)
        if run is None:
            raise SystemExit("the reference checkout is not here")
        out.update(golden_entries(name, run))
    np.savez_compressed(A.GOLDEN, **out)
    print(A.GOLDEN, os.path.getsize(A.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
