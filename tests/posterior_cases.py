"""The pairs the posterior tests share (tests/test_posterior_plan.py, tests/test_gpu_posterior.py): the smallest shapes at which each
rule of getPosteriorProbsWithBanding (impl/pairwiseAligner.c:706-844) can go wrong, and the restatement's answer for each, computed
once per process."""
from __future__ import annotations

import functools

import numpy as np

from margin_amd import capi, synth
from tests import posterior_oracle as po


def _fit(rng, s, length):
    """s cut or padded with random symbols to the given length"""
    s = list(s[:length])
    while len(s) < length:
        s.append(int(rng.integers(0, 4)))
    return np.array(s, dtype=np.uint8)


def _pair(seed, lx, ly=None):
    """x random, y = x mutated at about 15 % (5 % substitutions, insertions, deletions each); ly given: y cut or padded to it"""
    rng = np.random.default_rng(seed)
    sx = synth.random_sequence(rng, lx)
    sy = synth.evolve_sequence(rng, sx, 0.05, 0.05, 0.05)
    return sx, (sy if ly is None else _fit(rng, sy, ly))


def random_anchors(rng, lx, ly):
    """getRandomAnchorPairs, tests/pairwiseAlignerTest.c:344-360 (without the per-anchor expansion of the dynamic band)"""
    out, x, y = [], -1, -1
    while True:
        x += int(rng.integers(1, 21))
        y += int(rng.integers(1, 21))
        if x >= lx or y >= ly:
            return out
        out.append((x, y))


def _anchored(seed, lx, step):
    sx, sy = _pair(seed, lx)
    anchors = [(i, min(i, len(sy) - 1)) for i in range(step - 5, min(len(sx), len(sy)) - 5, step)]
    return sx, sy, anchors


# name -> (sx, sy, anchors, dict of expansion / min_diags / traceback_diagonals / ragged_left / ragged_right).  The seeds are the first
# whose pair gives the restatement a non-empty match, gap-x and gap-y list at both thresholds, so that no comparison is of nothing.
def _cases():
    c = {}
    sx, sy = _pair(18, 12, 9)  # a traceback every 3 diagonals: the boundaries, the kept traceBack + 2 forward diagonals
    c["1_12x9"] = (sx, sy, [], dict(expansion=10, min_diags=6, traceback_diagonals=2))
    sx, sy = _pair(3, 12, 13)  # the width rule postpones a traceback
    c["2_12x13"] = (sx, sy, [], dict(expansion=2, min_diags=4, traceback_diagonals=1))
    sx, sy = _pair(1, 30, 29)  # tracebacks of exactly 10 posterior diagonals: the edge of the every-tenth-total rule
    c["3_30x29"] = (sx, sy, [], dict(expansion=20, min_diags=14, traceback_diagonals=3))
    sx, sy = _pair(1, 70, 65)  # 18 diagonals per traceback, two totals each; diagonals wider than a wave (66)
    c["4_70x65"] = (sx, sy, [], dict(expansion=40, min_diags=24, traceback_diagonals=5))
    sx, sy = _pair(3, 100)  # the reference's defaults: one traceback of ~197 diagonals and 20 totals
    c["5_100"] = (sx, sy, [], dict(expansion=20, min_diags=1000, traceback_diagonals=40))
    sx, sy, an = _anchored(16, 160, 25)  # band limits from anchors, ragged start and end states, eight tracebacks
    c["6_160_e4"] = (sx, sy, an, dict(expansion=4, min_diags=30, traceback_diagonals=8, ragged_left=True, ragged_right=True))
    c["6_160_e10"] = (sx, sy, an, dict(expansion=10, min_diags=30, traceback_diagonals=8, ragged_left=True, ragged_right=True))
    return c


CASES = _cases()
THRESHOLDS = (0.01, 0.2)


def model():
    return capi.PairHmm.default_nucleotide()


@functools.lru_cache(maxsize=None)
def expected(name, threshold):
    """the restatement with gaps: ((match, gap_x, gap_y), info); the match list does not depend on with_gaps"""
    sx, sy, anchors, kw = CASES[name]
    return po.posterior(model(), sx, sy, anchors, threshold=threshold, with_gaps=True, **kw)


def options(kw, threshold, with_gaps):
    return capi.PosteriorOptions(threshold=threshold, expansion=kw["expansion"], min_diags_between_traceback=kw["min_diags"],
                                 traceback_diagonals=kw["traceback_diagonals"], ragged_left=kw.get("ragged_left", False),
                                 ragged_right=kw.get("ragged_right", False), with_gaps=with_gaps)


def pack(pairs):
    """[(sx, sy, anchors)] -> pool, x_off, x_len, y_off, y_len, anchor_off, anchors as the entries take them"""
    pool, xo, xl, yo, yl, ao, an = [], [], [], [], [], [0], []
    at = 0
    for sx, sy, anchors in pairs:
        xo.append(at); xl.append(len(sx)); at += len(sx)
        yo.append(at); yl.append(len(sy)); at += len(sy)
        pool += [np.asarray(sx, dtype=np.uint8), np.asarray(sy, dtype=np.uint8)]
        an += [v for a in anchors for v in a]
        ao.append(len(an) // 2)
    pool = np.concatenate(pool) if pool else np.zeros(0, np.uint8)
    return (pool, np.array(xo, np.int64), np.array(xl, np.int32), np.array(yo, np.int64), np.array(yl, np.int32), np.array(ao, np.int64),
            np.array(an, np.int64))


def as_arrays(lists):
    """the restatement's lists of several pairs -> first / x / y / weight / log_posterior as the entry returns them"""
    first, x, y, w, v = [0], [], [], [], []
    for lst in lists:
        for p in lst:
            w.append(p[0]); x.append(p[1]); y.append(p[2]); v.append(p[3])
        first.append(len(x))
    return {"first": np.array(first, np.int64), "x": np.array(x, np.int32), "y": np.array(y, np.int32), "weight": np.array(w, np.int32),
            "log_posterior": np.array(v, np.float64)}


def assert_lists_equal(got, want):
    """exactly: the log posteriors as bit patterns"""
    for k in ("first", "x", "y", "weight"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["log_posterior"].view(np.int64), want["log_posterior"].view(np.int64))
