"""Writes tests/golden/posterior/wide_classes.npz: the restatement's lists (tests/posterior_oracle.py) for three unanchored pairs whose
widest diagonals fall into the launch classes of 1 024 and 2 048 cells (and one of 256), which the restatement is too slow to produce
inside a test (a minute for the largest).  Run from the repository root:  python -m tests.make_posterior_golden
"""
import os

import numpy as np

from margin_amd import synth
from tests import posterior_cases as pc
from tests import posterior_oracle as po

SHAPES = (("w256", 31, 200), ("w1024", 32, 300), ("w2048", 33, 1100))
KW = dict(expansion=20, min_diags=1000, traceback_diagonals=40)  # the reference's defaults
THRESHOLD = 0.01


def main():
    out = {}
    for name, seed, lx in SHAPES:
        rng = np.random.default_rng(seed)
        sx = synth.random_sequence(rng, lx)
        sy = synth.evolve_sequence(rng, sx, 0.05, 0.05, 0.05)
        lists, info = po.posterior(pc.model(), sx, sy, [], threshold=THRESHOLD, with_gaps=True, **KW)
        out[name + "_x"], out[name + "_y"] = sx, sy
        for k, tag in enumerate(("match", "gapx", "gapy")):
            a = pc.as_arrays([lists[k]])
            for f in ("x", "y", "weight", "log_posterior"):
                out[f"{name}_{tag}_{f}"] = a[f]
        print(name, len(sx), len(sy), [len(l) for l in lists])
    path = os.path.join(os.path.dirname(__file__), "golden", "posterior")
    os.makedirs(path, exist_ok=True)
    np.savez_compressed(os.path.join(path, "wide_classes.npz"), **out)


if __name__ == "__main__":
    main()
