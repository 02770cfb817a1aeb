"""The downsampling to maxDepth, restated in Python.  TEST INFRASTRUCTURE ONLY.

Restates downsampleBamChunkReadWithVcfEntrySubstringsViaFullReadLengthLikelihood (impl/htsIntegration.c:1141-1216) branch by branch on
the inputs include/margin_rphmm.h names: per read its status, l = the variants it saved a substring for and
h = alnReadLength; per chunk V = its variant count.  The LP of computeReadProbsByLengthAndSecondMetric (:957-1011) is solved in exact
rationals (fractions.Fraction), and `certificate` checks a candidate optimum without sharing a line with the greedy that makes one.
The draws are the library's counter-based ones (sonLib's st_random cannot be reproduced), restated in integers."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

KEPT = 1  # MRP_READ_KEPT
MASK = (1 << 64) - 1


def mix(z: int) -> int:
    """the splitmix64 finaliser"""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed: int, overlap_start: int, overlap_end: int, k: int) -> float:
    """u_k of a chunk: three nested finalisers, the top 53 bits times 2^-53 (exact in a double)"""
    z = mix(mix(mix((seed ^ overlap_start) & MASK) ^ (overlap_end & MASK)) ^ (k & MASK))
    return (z >> 11) / float(1 << 53)


def lp_optimum(l, h, T: int):
    """maximise sum p h subject to sum p l = T, 0 <= p <= 1, over reads with l > 0 and sum l > T: the fractional knapsack's greedy,
    by h / l descending, equal ratios by ascending index -> list of Fraction"""
    order = sorted(range(len(l)), key=lambda i: (-Fraction(int(h[i]), int(l[i])), i))
    p = [Fraction(0)] * len(l)
    before = 0
    for i in order:
        if before + int(l[i]) <= T:
            p[i] = Fraction(1)
        elif before < T:
            p[i] = Fraction(T - before, int(l[i]))
        before += int(l[i])
    return p


def certificate(l, h, T: int, p) -> None:
    """asserts that p is AN optimum of the LP over reads with l > 0: feasible, and some threshold ratio has p = 1 above it and p = 0
    below it (an exchange argument: moving weight from a lower ratio to a higher one at constant sum p l cannot lower the objective,
    and no such move is left)"""
    assert all(0 <= q <= 1 for q in p)
    assert sum(q * int(li) for q, li in zip(p, l)) == T
    ratio = [Fraction(int(hi), int(li)) for hi, li in zip(h, l)]
    not_full = [r for r, q in zip(ratio, p) if q < 1]
    not_empty = [r for r, q in zip(ratio, p) if q > 0]
    if not_full and not_empty:
        assert max(not_full) <= min(not_empty)


def objective(h, p) -> Fraction:
    return sum((Fraction(q) * int(hi) for q, hi in zip(p, h)), Fraction(0))


def downsample(status, l, h, V: int, D: int, seed: int, overlap_start: int, overlap_end: int):
    """-> (keep uint8 [n], prob float64 [n], downsampled bool, exact probabilities of the kept reads with l > 0 or None)"""
    n = len(status)
    kept = [r for r in range(n) if status[r] == KEPT]                       # :1153-1161 `reads`, in list order
    total = sum(int(l[r]) for r in kept)
    keep, prob = np.zeros(n, np.uint8), np.zeros(n, np.float64)
    if V > 0 and float(total) / float(V) < float(D):                         # :1163-1170 (V == 0: inf or nan, never below D)
        for r in kept:
            keep[r], prob[r] = 1, 1.0
        return keep, prob, False, None
    if V == 0:                                                               # :1174-1186 everybody is discarded
        return keep, prob, True, None
    T = D * V                                                                # :964 total_cov
    pos = [r for r in kept if l[r] > 0]
    exact = None
    if total <= T:
        p = {r: Fraction(1) for r in kept}
    else:
        exact = lp_optimum([l[r] for r in pos], [h[r] for r in pos], T)
        certificate([l[r] for r in pos], [h[r] for r in pos], T, exact)
        p = {r: (Fraction(1) if h[r] > 0 else Fraction(0)) for r in kept}   # l == 0: a free variable, its coefficient decides
        p.update(dict(zip(pos, exact)))
    for k, r in enumerate(kept):                                             # :1199-1207 one draw per read, in list order
        prob[r] = p[r].numerator / p[r].denominator                          # (int / int: the correctly rounded quotient)
        keep[r] = draw(seed, overlap_start, overlap_end, k) < prob[r]
    return keep, prob, True, exact
