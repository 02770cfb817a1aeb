"""A Python restatement of the posterior half of the reference's pairwise aligner.  TEST INFRASTRUCTURE ONLY.

getPosteriorProbsWithBanding (impl/pairwiseAligner.c:706-844) with diagonalCalculationPosteriorMatchProbs (:610-635) or
diagonalCalculationPosteriorProbs (:637-681), addPosteriorProb (:598-608) and diagonalCalculationTotalProbability (:578-596).  It runs
sequentially as the reference does: forward diagonal by diagonal, a traceback where the reference has one, diagonals created and
deleted where the reference creates and deletes them, and it asserts what the reference asserts at :782-787 and :824-837.

Python floats are IEEE doubles, every operation below is a single + or * (no contraction), the float literals of lookup() are rounded
to float first as a C compiler does, and math.exp is the C library's exp: the lists are the reference's bit for bit.  The band comes
from oracle.pairhmm (band_construct); log_add below is pinned against oracle.pairhmm.log_add by tests/test_posterior_oracle.py.
"""
from __future__ import annotations

import math
import struct

from oracle import pairhmm as ph

NEG = float("-inf")
MATCH, GAP_X, GAP_Y = 0, 1, 2  # stateMachine.h: match, shortGapX, shortGapY
PAIR_ALIGNMENT_PROB_1 = 10000000  # inc/pairwiseAligner.h


def _f(v: float) -> float:
    """a float literal (0.693203116424741f) widened to double"""
    return struct.unpack("f", struct.pack("f", v))[0]


_C = [[_f(c) for c in row] for row in ((-0.009350833524763, 0.130659527668286, 0.498799810682272, 0.693203116424741),
                                       (-0.014532321752540, 0.139942324101744, 0.495635523139337, 0.692140569840976),
                                       (-0.004605031767994, 0.063427417320019, 0.695956496475118, 0.514272634594009),
                                       (-0.000458661602210, 0.009695946122598, 0.930734667215156, 0.168037164329057))]


def lookup(x: float) -> float:
    """lookup, impl/pairwiseAligner.c:282-293"""
    c = _C[0] if x <= 1.0 else (_C[1] if x <= 2.5 else (_C[2] if x <= 4.5 else _C[3]))
    return ((c[0] * x + c[1]) * x + c[2]) * x + c[3]


def log_add(x: float, y: float) -> float:
    """logAdd, impl/pairwiseAligner.c:295-299"""
    if x < y:
        return y if (x == NEG or y - x >= 7.5) else lookup(y - x) + x
    return x if (y == NEG or x - y >= 7.5) else lookup(x - y) + y


class Model:
    """StateMachine3 + nucleotide emissions as Python floats, from a capi.PairHmm or an oracle.pairhmm.Model"""

    def __init__(self, m):
        self.mc, self.mfx, self.mfy = float(m.match_continue), float(m.match_from_gap_x), float(m.match_from_gap_y)
        self.gox, self.goy, self.gex, self.gey = float(m.gap_open_x), float(m.gap_open_y), float(m.gap_extend_x), float(m.gap_extend_y)
        self.gsx, self.gsy = float(m.gap_switch_to_x), float(m.gap_switch_to_y)
        self.em, self.ex, self.ey = [float(v) for v in m.e_match], [float(v) for v in m.e_gap_x], [float(v) for v in m.e_gap_y]


def gap_prob(t, c):
    """emissions_symbol_getGapProb, impl/stateMachine.c:363-368"""
    return -1.386294361 if c >= 4 else t[c]


def match_prob(m: Model, a, b):
    """emissions_symbol_getMatchProb, impl/stateMachine.c:378-383"""
    return -2.772588722 if (a >= 4 or b >= 4) else m.em[a * 4 + b]


def fwd(fr, to, f, t, eP, tP):
    """doTransitionForward, impl/pairwiseAligner.c:311-314"""
    to[t] = log_add(to[t], fr[f] + (eP + tP))


def bwd(fr, to, f, t, eP, tP):
    """doTransitionBackward, impl/pairwiseAligner.c:322-325"""
    fr[f] = log_add(fr[f], to[t] + (eP + tP))


def cell(m: Model, cur, lower, middle, upper, cX, cY, go):
    """stateMachine3_cellCalculate, impl/stateMachine.c:562-586"""
    if lower is not None:
        eP = gap_prob(m.ex, cX)
        go(lower, cur, MATCH, GAP_X, eP, m.gox)
        go(lower, cur, GAP_X, GAP_X, eP, m.gex)
        go(lower, cur, GAP_Y, GAP_X, eP, m.gsx)
    if middle is not None:
        eP = match_prob(m, cX, cY)
        go(middle, cur, MATCH, MATCH, eP, m.mc)
        go(middle, cur, GAP_X, MATCH, eP, m.mfx)
        go(middle, cur, GAP_Y, MATCH, eP, m.mfy)
    if upper is not None:
        eP = gap_prob(m.ey, cY)
        go(upper, cur, MATCH, GAP_Y, eP, m.goy)
        go(upper, cur, GAP_Y, GAP_Y, eP, m.gey)
        go(upper, cur, GAP_X, GAP_Y, eP, m.gsy)


def start_prob(ragged, s):
    """stateMachine3_startStateProb / raggedStartStateProb, impl/stateMachine.c:521-530"""
    return (0.0 if s in (GAP_X, GAP_Y) else NEG) if ragged else (0.0 if s == MATCH else NEG)


def end_prob(m: Model, ragged, s):
    """stateMachine3_endStateProb / raggedEndStateProb, impl/stateMachine.c:532-560"""
    if ragged:
        return (m.gox + m.goy) / 2.0 if s == MATCH else (m.gex if s == GAP_X else m.gey)
    return m.mc if s == MATCH else (m.mfx if s == GAP_X else m.mfy)


class Diag:
    """DpDiagonal, impl/pairwiseAligner.c:383-448: created with LOG_ZERO (dpDiagonal_zeroValues) or with init(state) in every cell"""

    def __init__(self, xay, l, r, init=None):
        self.xay, self.l, self.r = xay, l, r
        self.c = [[NEG] * 3 if init is None else [init(k) for k in range(3)] for _ in range((r - l) // 2 + 1)]

    def cell(self, xmy):
        """dpDiagonal_getCell, impl/pairwiseAligner.c:425-431"""
        return None if (xmy < self.l or xmy > self.r) else self.c[(xmy - self.l) // 2]


def diagonal_calculation(m, d, m1, m2, sx, sy, go):
    """diagonalCalculation, impl/pairwiseAligner.c:547-564 (getXCharacter / getYCharacter :535-545)"""
    for xmy in range(d.l, d.r + 1, 2):
        x, y = (d.xay + xmy) // 2, (d.xay - xmy) // 2
        cX = sx[x - 1] if x > 0 else 4
        cY = sy[y - 1] if y > 0 else 4
        cell(m, d.cell(xmy), m1.cell(xmy - 1) if m1 else None, m2.cell(xmy) if m2 else None, m1.cell(xmy + 1) if m1 else None, cX, cY, go)


def cell_dot(a, b):
    """cell_dotProduct, impl/pairwiseAligner.c:333-339"""
    t = a[0] + b[0]
    for i in (1, 2):
        t = log_add(t, a[i] + b[i])
    return t


def diag_dot(a, b):
    """dpDiagonal_dotProduct, impl/pairwiseAligner.c:450-461"""
    t = NEG
    for xmy in range(a.l, a.r + 1, 2):
        t = log_add(t, cell_dot(a.cell(xmy), b.cell(xmy)))
    return t


def total_probability(m, xay, F, B, sx, sy):
    """diagonalCalculationTotalProbability, impl/pairwiseAligner.c:578-596"""
    t = diag_dot(F[xay], B[xay])
    f1, b1 = F.get(xay - 1), B.get(xay + 1)
    if f1 is not None and b1 is not None:
        md = Diag(b1.xay, b1.l, b1.r)
        diagonal_calculation(m, md, None, f1, sx, sy, fwd)
        t = log_add(t, diag_dot(md, b1))
    return t


def _exp(v):
    return math.exp(v) if v == v else v  # exp(NaN) = NaN; math.exp(+-inf) is C's


def posterior(model, sx, sy, anchors=(), expansion=20, threshold=0.01, min_diags=1000, traceback_diagonals=40, ragged_left=False,
              ragged_right=False, with_gaps=False):
    """getPosteriorProbsWithBanding, impl/pairwiseAligner.c:706-844.  Returns ((match, gap_x, gap_y), info): each list holds
    (weight, x, y, v) in the order of generation, v the argument of exp(); info one (d, tracedBackTo, tracedBackFrom, diagonals taken,
    [(diagonal, total) recomputed]) per traceback."""
    m = model if isinstance(model, Model) else Model(model)
    sx, sy = [int(c) for c in sx], [int(c) for c in sy]
    assert traceback_diagonals >= 1 and expansion >= 0 and expansion % 2 == 0 and min_diags >= 2 and traceback_diagonals + 1 < min_diags  # :714-718
    lX, lY = len(sx), len(sy)
    n = lX + lY
    out, info = ([], [], []), []
    if n == 0:  # :721-723
        return out, info
    L, R = ph.band(anchors, lX, lY, expansion)  # band_construct :175-226
    L, R = [int(v) for v in L], [int(v) for v in R]
    F = {0: Diag(0, L[0], R[0], lambda k: start_prob(ragged_left, k))}  # :730-732
    B = {}

    def add(lst, x, y, v):
        """addPosteriorProb, impl/pairwiseAligner.c:598-608"""
        p = _exp(v)
        if p >= threshold:
            lst.append((int(math.floor(min(p, 1.0) * PAIR_ALIGNMENT_PROB_1)), x - 1, y - 1, v))

    traced_to = 0
    total_calcs = 0
    for d in range(1, n + 1):  # :739-744
        F[d] = Diag(d, L[d], R[d])
        diagonal_calculation(m, F[d], F.get(d - 1), F.get(d - 2), sx, sy, fwd)
        at_end = d == n  # :746
        width = (R[d] - L[d]) // 2 + 1
        if not (at_end or (d >= traced_to + min_diags and width <= expansion * 2 + 1)):  # :747-752
            continue
        B[d] = Diag(d, L[d], R[d], lambda k: end_prob(m, at_end and ragged_right, k))  # :754-756
        if d > traced_to + 1:  # :757-762
            assert F.get(d - 1) is not None
            B[d - 1] = Diag(d - 1, L[d - 1], R[d - 1])
        traced_from = d - (0 if at_end else traceback_diagonals + 1)  # :768
        total, k, d2, recomputed = NEG, 0, d, []
        while d2 > traced_to:  # :771
            if d2 > traced_to + 2:  # :773-777
                assert F.get(d2 - 2) is not None
                B[d2 - 2] = Diag(d2 - 2, L[d2 - 2], R[d2 - 2])
            if d2 > traced_to + 1:  # :778-780
                diagonal_calculation(m, B[d2], B.get(d2 - 1), B.get(d2 - 2), sx, sy, bwd)
            if d2 <= traced_from:  # :781
                assert F.get(d2) is not None and F.get(d2 - 1) is not None and B.get(d2) is not None  # :782-784
                if d2 != n:
                    assert B.get(d2 + 1) is not None  # :785-787
                if k % 10 == 0:  # :788-803
                    new_total = total_probability(m, d2, F, B, sx, sy)
                    if k != 0:
                        assert total + 1.0 > new_total and new_total + 1.0 > new_total  # :799-800
                    recomputed.append((d2, new_total))
                    total = new_total
                k += 1
                fd, bd = F[d2], B[d2]
                for xmy in range(fd.l, fd.r + 1, 2):  # :610-681
                    x, y = (d2 + xmy) // 2, (d2 - xmy) // 2
                    cf, cb = fd.cell(xmy), bd.cell(xmy)
                    if x > 0 and y > 0:
                        add(out[0], x, y, (cf[MATCH] + cb[MATCH]) - total)
                    if with_gaps and x > 0:
                        add(out[1], x, y, (cf[GAP_X] + cb[GAP_X]) - total)
                    if with_gaps and y > 0:
                        add(out[2], x, y, (cf[GAP_Y] + cb[GAP_Y]) - total)
                if d2 < traced_from or at_end:  # :808-811
                    del F[d2]
            if d2 + 1 <= n:  # :813-816
                B.pop(d2 + 1, None)
            d2 -= 1
        info.append((d, traced_to, traced_from, k, recomputed))
        traced_to = traced_from  # :819
        B.pop(d2 + 1, None)  # :821
        F.pop(d2, None)  # :822
        assert len(B) == 0  # :824
        total_calcs += k
        if not at_end:
            assert len(F) == traceback_diagonals + 2  # :826-828
    assert total_calcs == n and traced_to == n and not F and not B  # :835-838
    return out, info


def tracebacks(lx, ly, anchors=(), expansion=20, min_diags=1000, traceback_diagonals=40):
    """the (d, tracedBackTo, tracedBackFrom) of the loop above without its arithmetic (:746-749, :768, :819)"""
    n = lx + ly
    if n == 0:
        return []
    L, R = ph.band(anchors, lx, ly, expansion)
    out, traced_to = [], 0
    for d in range(1, n + 1):
        at_end = d == n
        width = (int(R[d]) - int(L[d])) // 2 + 1
        if not (at_end or (d >= traced_to + min_diags and width <= expansion * 2 + 1)):
            continue
        traced_from = d - (0 if at_end else traceback_diagonals + 1)
        out.append((d, traced_to, traced_from))
        traced_to = traced_from
    return out


def check_aligned_pairs(pairs, lx, ly, x_gaps=False, y_gaps=False):
    """checkAlignedPairs, tests/pairwiseAlignerTest.c:362-397, over (weight, x, y, ...) tuples"""
    seen = set()
    for p in pairs:
        w, x, y = int(p[0]), int(p[1]), int(p[2])
        assert 0 < w <= PAIR_ALIGNMENT_PROB_1
        assert x >= (-1 if y_gaps else 0) and y >= (-1 if x_gaps else 0)
        assert x < lx and y < ly
        assert (x, y) not in seen
        seen.add((x, y))
