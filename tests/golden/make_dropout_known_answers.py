"""Writes tests/golden/dropout_known_answers.npz: (seed, step, layer, row, col, p) -> (hash, keep) from the SCALAR
implementation of oracle/dropout.py, so that a later edit of the replica cannot drift silently
(tests/test_dropout_cases_cpu.py).  Run from the repository root: python tests/golden/make_dropout_known_answers.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import dropout as drp  # noqa: E402

SEEDS = (5, 123456789012345, 2 ** 62 - 1)
# (seed index, step, layer, row, col, p): first element, both halves of a pair, pair index >= 128, rows past 2^16 and
# 2^31, later steps, the four probabilities of dropout_cases.py
INPUTS = [(0, 0, 0, 0, 0, 0.1), (0, 0, 0, 0, 64, 0.1), (0, 0, 0, 0, 128, 0.1), (0, 0, 0, 1, 0, 0.1),
          (0, 1, 0, 0, 0, 0.1), (0, 0, 1, 0, 0, 0.1), (1, 0, 2, 299, 63, 0.1), (1, 0, 2, 299, 127, 0.1),
          (1, 2, 7, 4096, 15, 0.1), (1, 2, 7, 16320, 175, 0.1), (2, 0, 0, 65536, 256, 0.1), (2, 3, 1, 65537, 319, 0.1),
          (2, 1000, 3, 2 ** 31 + 5, 200, 0.1), (0, 5, 0, 77, 77, 0.25), (1, 5, 1, 77, 141, 0.25), (2, 5, 2, 77, 13, 0.5),
          (0, 9, 4, 123456, 100, 0.5), (1, 0, 0, 41389, 69, 1e-5), (2, 2, 6, 8160, 47, 1e-5), (0, 1, 1, 300, 39, 0.1),
          (2, 2 ** 31 - 1, 5, 12, 255, 0.1)]

if __name__ == "__main__":
    rows = [(SEEDS[i], st, l, r, c, p) for i, st, l, r, c, p in INPUTS]
    np.savez(os.path.join(HERE, "dropout_known_answers.npz"),
             seed=np.array([r[0] for r in rows], np.uint64), step=np.array([r[1] for r in rows], np.int64),
             layer=np.array([r[2] for r in rows], np.int64), row=np.array([r[3] for r in rows], np.int64),
             col=np.array([r[4] for r in rows], np.int64), p=np.array([r[5] for r in rows], np.float64),
             hash=np.array([drp.hash_scalar(*r[:5]) for r in rows], np.uint32),
             keep=np.array([drp.keep_scalar(*r) for r in rows], np.bool_))
    print(f"{len(rows)} known answers written")
