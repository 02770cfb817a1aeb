"""Writes the two fixtures of the run-length tests (tests/test_gpu_rle_pairhmm.py), inputs and the restatement's answers only:

tests/golden/repeat_matrix_r94_g507.npz    log_prob_F [4, 51, 51]: the values of the four repeatCountLogProbabilities_{A,C,G,T}_F
    arrays of a shipped polish parameter file (params/polish/ont/r9.4/allParams.np.human.r94-g507.json of the reference), given as
    the first argument; without an argument the committed file is kept.
tests/golden/posterior/rle_classes.npz     the lists of tests/rle_pairhmm_oracle.py for one unanchored pair in the launch class of
    1 024 cells (widest diagonal 257) and one in the class of 2 048, and the forward probability of one pair beyond 2 048 cells, all
    with the shipped matrix and the counts of tests/rle_cases.py's rle_pair, which the restatement is too slow to produce inside a test.

Run from the repository root:  python -m tests.make_rle_posterior_golden [allParams.json]
The run that wrote the committed fixture took MEASURED_SECONDS (below) on one CPU core.
"""
import json
import os
import sys
import time

import numpy as np

from tests import posterior_cases as pc
from tests import rle_cases as rc
from tests import rle_pairhmm_oracle as ro

# name -> seed, lx, ly, strand, options, threshold
POSTERIOR = {"w257": (1257, 256, 268, 0, dict(expansion=20, min_diags=30, traceback_diagonals=4), 0.01),
             "w1101": (33, 1100, None, 1, dict(expansion=20, min_diags=1000, traceback_diagonals=40), 0.01)}
FORWARD = {"w2060": (34, 2060, None, 1)}
MEASURED_SECONDS = 46  # the run that wrote the committed fixture: 1 s, 19 s and 26 s for the three pairs


def matrix_from_params(path):
    m = json.load(open(path))["polish"]["repeatCountSubstitutionMatrix"]
    a = np.array([m[f"repeatCountLogProbabilities_{b}_F"] for b in "ACGT"], np.float64)
    return a.reshape(4, rc.R_SHIPPED, rc.R_SHIPPED)


def pair_with_counts(seed, lx, ly):
    return rc.rle_pair(seed, lx, rc.R_SHIPPED, ly)


def main():
    if len(sys.argv) > 1:
        np.savez_compressed(os.path.join(rc.GOLDEN, "repeat_matrix_r94_g507.npz"), log_prob_F=matrix_from_params(sys.argv[1]))
    table = rc.shipped_matrix()
    t0 = time.time()
    out = {}
    for name, (seed, lx, ly, strand, kw, threshold) in POSTERIOR.items():
        sx, cx, sy, cy = pair_with_counts(seed, lx, ly)
        lists, info = rc.want_posterior(pc.model(), table, strand, (sx, cx, sy, cy, []), kw, threshold)
        out.update({name + "_x": sx, name + "_cx": cx, name + "_y": sy, name + "_cy": cy,
                    name + "_total": np.array([rc.total_of(info, len(sx) + len(sy))], np.float64)})
        for k, tag in enumerate(("match", "gapx", "gapy")):
            a = pc.as_arrays([lists[k]])
            for f in ("x", "y", "weight", "log_posterior"):
                out[f"{name}_{tag}_{f}"] = a[f]
        print(name, len(sx), len(sy), [len(l) for l in lists], f"{time.time() - t0:.0f} s", flush=True)
    for name, (seed, lx, ly, strand) in FORWARD.items():
        sx, cx, sy, cy = pair_with_counts(seed, lx, ly)
        assert min(len(sx), len(sy)) + 1 > 2048
        rsm = ro.RepeatSubMatrix(table, strand)
        total = ro.forward_probability(pc.model(), ro.symbols(sx, cx, rc.R_SHIPPED), ro.symbols(sy, cy, rc.R_SHIPPED), [], expansion=20, rsm=rsm)
        out.update({name + "_x": sx, name + "_cx": cx, name + "_y": sy, name + "_cy": cy, name + "_total": np.array([total], np.float64)})
        print(name, len(sx), len(sy), total, f"{time.time() - t0:.0f} s", flush=True)
    path = os.path.join(rc.GOLDEN, "posterior")
    os.makedirs(path, exist_ok=True)
    np.savez_compressed(os.path.join(path, "rle_classes.npz"), **out)


if __name__ == "__main__":
    main()
