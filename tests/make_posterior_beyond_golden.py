"""Writes tests/golden/posterior/beyond_2048.npz: the restatement's lists (tests/posterior_oracle.py) for one unanchored pair whose
widest diagonal holds more than 2 048 cells, the first size that mrp_posterior_aligned_pairs takes only with posterior wide pairs on
(tests/test_gpu_posterior_beyond.py).  The reference's defaults, with gaps: one traceback over every diagonal.  The restatement walks
the 4.2 M cells of the band twice; on one CPU core that took MEASURED_SECONDS (below).  Run from the repository root:
python -m tests.make_posterior_beyond_golden
"""
import os
import time

import numpy as np

from margin_amd import synth
from tests import posterior_cases as pc
from tests import posterior_oracle as po

NAME, SEED, LX = "w2060", 34, 2060
KW = dict(expansion=20, min_diags=1000, traceback_diagonals=40)  # the reference's defaults
THRESHOLD = 0.01
MEASURED_SECONDS = 55  # the run that wrote the committed fixture (2060 x 2057 symbols; 3227 / 798 / 763 list entries)


def main():
    rng = np.random.default_rng(SEED)
    sx = synth.random_sequence(rng, LX)
    sy = synth.evolve_sequence(rng, sx, 0.05, 0.05, 0.05)
    assert min(len(sx), len(sy)) + 1 > 2048, (len(sx), len(sy))
    t0 = time.time()
    lists, info = po.posterior(pc.model(), sx, sy, [], threshold=THRESHOLD, with_gaps=True, **KW)
    out = {NAME + "_x": sx, NAME + "_y": sy, NAME + "_total": np.array([info[-1][4][0][1]], np.float64)}
    for k, tag in enumerate(("match", "gapx", "gapy")):
        a = pc.as_arrays([lists[k]])
        for f in ("x", "y", "weight", "log_posterior"):
            out[f"{NAME}_{tag}_{f}"] = a[f]
    print(NAME, len(sx), len(sy), [len(l) for l in lists], f"{time.time() - t0:.0f} s")
    path = os.path.join(os.path.dirname(__file__), "golden", "posterior")
    os.makedirs(path, exist_ok=True)
    np.savez_compressed(os.path.join(path, "beyond_2048.npz"), **out)


if __name__ == "__main__":
    main()
