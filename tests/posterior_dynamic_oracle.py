"""The dynamic anchor band for the posterior restatement.  TEST INFRASTRUCTURE ONLY.

band_dynamic restates band_constructDynamic (impl/pairwiseAligner.c:120-173) with band_setCurrentDiagonal (:86-114) and
diagonal_construct (:22-35), loop for loop and assert for assert: a violated assert or the exception of :23-27 is a ValueError.
posterior_dynamic and tracebacks_dynamic run tests/posterior_oracle.py's posterior and tracebacks over that band: the restatement asks
oracle.pairhmm.band for its band, and for the duration of one call that name answers with the dynamic band instead.  What
getPosteriorProbsWithBanding reads of `diagonalExpansion` beside the band (the width rule of :748) stays the scalar.
"""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import pairhmm as ph
from tests import posterior_oracle as po


def _need(ok):
    if not ok:
        raise ValueError("band_constructDynamic: assertion")


def _x(xay, xmy):
    """diagonal_getXCoordinate, :53-56"""
    _need((xay + xmy) % 2 == 0)
    return (xay + xmy) // 2


def _y(xay, xmy):
    """diagonal_getYCoordinate, :62-65"""
    _need((xay - xmy) % 2 == 0)
    return (xay - xmy) // 2


def _set_current_diagonal(xay, xL, yL, xU, yU):
    """band_setCurrentDiagonal, :96-114"""
    xmyL, xmyR = xL - yL, xU - yU
    _need(xay >= xL + yU)
    _need(xay <= xU + yL)
    xmyL = xmyL if (xay + xmyL) % 2 == 0 else xmyL + 1  # band_avoidOffByOne
    xmyR = xmyR if (xay + xmyR) % 2 == 0 else xmyR + 1

    def p(xmy, i, j, k):  # band_setCurrentDiagonalP
        return xmy + 2 * (j - i) * k if i < j else xmy

    xmyL = p(xmyL, _x(xay, xmyL), xL, 1)
    xmyL = p(xmyL, yL, _y(xay, xmyL), 1)
    xmyR = p(xmyR, xU, _x(xay, xmyR), -1)
    xmyR = p(xmyR, _y(xay, xmyR), yU, -1)
    if (xay + xmyL) % 2 != 0 or (xay + xmyR) % 2 != 0 or xmyL > xmyR:  # diagonal_construct
        raise ValueError("invalid diagonal")
    return xmyL, xmyR


def band_dynamic(anchors, expansions, lx, ly):
    """band_constructDynamic, :120-173: anchors [(x, y)], expansions one per anchor -> (xmyL, xmyR), int64 [lx + ly + 1] each"""
    anchors, expansions = [(int(x), int(y)) for x, y in anchors], [int(e) for e in expansions]
    _need(len(anchors) == len(expansions))
    _need(lx >= 0 and ly >= 0)
    n = lx + ly
    lo, hi = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    bound = lambda z, lz: 0 if z < 0 else (lz if z > lz else z)  # band_boundCoordinate
    index = 0
    xay = 0
    pxay = pxmy = nxay = nxmy = 0
    xL = yL = xU = yU = expansion = 0
    while xay <= n:
        lo[xay], hi[xay] = _set_current_diagonal(xay, xL, yL, xU, yU)
        at_next = nxay == xay
        xay += 1
        if at_next:
            pxay, pxmy = nxay, nxmy
            x, y = lx, ly
            if index < len(anchors):
                x, y = anchors[index][0] + 1, anchors[index][1] + 1
                expansion = expansions[index]
                index += 1
                _need(x > _x(pxay, pxmy))
                _need(y > _y(pxay, pxmy))
                _need(x <= lx and y <= ly and x > 0 and y > 0)
                _need(expansion >= 0)
                _need(expansion % 2 == 0)
            nxay, nxmy = x + y, x - y
            xL = bound(_x(pxay, pxmy - expansion), lx)
            yL = bound(_y(nxay, nxmy - expansion), ly)
            xU = bound(_x(nxay, nxmy + expansion), lx)
            yU = bound(_y(pxay, pxmy + expansion), ly)
    return lo, hi


@contextlib.contextmanager
def _band_replaced(expansions):
    """oracle.pairhmm.band answers with the dynamic band; the scalar expansion it is called with is not the band's business"""
    saved = ph.band
    ph.band = lambda anchors, lx, ly, expansion: band_dynamic(anchors, expansions, lx, ly)
    try:
        yield
    finally:
        ph.band = saved


def posterior_dynamic(model, sx, sy, anchors, expansions, **kw):
    """posterior_oracle.posterior over the dynamic band; kw as there (expansion = the scalar of :748)"""
    with _band_replaced(expansions):
        return po.posterior(model, sx, sy, anchors, **kw)


def tracebacks_dynamic(lx, ly, anchors, expansions, **kw):
    with _band_replaced(expansions):
        return po.tracebacks(lx, ly, anchors, **kw)


def random_expansions(rng, n):
    """one even expansion per anchor, 0 .. 20 (getRandomAnchorPairs, tests/pairwiseAlignerTest.c:351, draws 0 .. 8: a wider range here)"""
    return [2 * int(rng.integers(0, 11)) for _ in range(n)]
