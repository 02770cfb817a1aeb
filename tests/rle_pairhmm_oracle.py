"""A Python restatement of the reference's run-length emissions for the pairwise aligner.  TEST INFRASTRUCTURE ONLY.

rleNucleotideEmissions_construct (impl/stateMachine.c:716-752), which polishParams_finishParsing (impl/parser.c:510-524) gives both
read-to-reference state machines when useRepeatCountsInAlignment is set:

  symbol_getRepeatLength / symbol_stripRepeatCount / symbol_addRepeatCount      impl/stateMachine.c:116-131
  repeatSubMatrix_getLogProb's index, with its N -> A and strand rules           impl/repeatSubMatrix.c:11-43
  getRleNucleotideGapProbX / ...GapProbY / ...MatchProb                          impl/stateMachine.c:722-738
  rleString_construct and the clamp of rleString_constructSymbolString           impl/rle.c:7-38, impl/stateMachine.c:133-146
  computeForwardProbability                                                      impl/pairwiseAligner.c:849-903

Everything that is not an emission is tests/posterior_oracle.py's and tests/posterior_dynamic_oracle.py's: their cell() asks the module
for gap_prob and match_prob at every call, and for the duration of one call here those two names answer with the run-length functions.
A symbol is the reference's Symbol, (count << 8) | base; the symbol before the first stays the literal 4 of
impl/pairwiseAligner.c:535-545, N with count 0.

The reference's own tests hold no vector for these emissions: tests/pairwiseAlignerTest.c:560-600 draws random strings and checks
properties of the result.  So parity with the reference is pinned by this restatement alone, line by line against the cited code.

Arithmetic: 2.3025 * log_prob is one IEEE multiply and the sum with the nucleotide term one IEEE add, as a C compiler without
contraction into a fused multiply-add evaluates impl/stateMachine.c:735-737.
"""
from __future__ import annotations

import contextlib

import numpy as np

from tests import posterior_dynamic_oracle as pdo
from tests import posterior_oracle as po


def symbol_get_repeat_length(s: int) -> int:
    """symbol_getRepeatLength, impl/stateMachine.c:116-118"""
    return s >> 8


def symbol_strip_repeat_count(s: int) -> int:
    """symbol_stripRepeatCount, impl/stateMachine.c:120-122"""
    return s & 255


def symbol_add_repeat_count(character: int, run_length: int, max_repeat_exclusive: int) -> int:
    """symbol_addRepeatCount, impl/stateMachine.c:124-131"""
    assert character <= 255
    if run_length >= max_repeat_exclusive:
        run_length = max_repeat_exclusive - 1
    assert run_length <= 255
    return (run_length << 8) | character


def symbols(bases, counts, max_repeat_exclusive):
    """rleString_constructSymbolString with includeRepeatCounts, impl/stateMachine.c:133-146, over bases already converted"""
    return [symbol_add_repeat_count(int(b), int(c), max_repeat_exclusive) for b, c in zip(bases, counts)]


class RepeatSubMatrix:
    """RepeatSubMatrix: logProbabilities [alphabetSize][R][R] flat, of which the parameter files fill the bases A..T"""

    ALPHABET_SIZE = 5  # the nucleotide alphabet, N last

    def __init__(self, log_prob, strand):
        lp = np.asarray(log_prob, dtype=np.float64)
        assert lp.ndim == 3 and lp.shape[0] == 4 and lp.shape[1] == lp.shape[2]
        self.R = int(lp.shape[1])
        self.flat = [float(v) for v in lp.reshape(-1)]
        self.strand = bool(strand)

    def index(self, base, strand, observed, underlying):
        """repeatSubMatrix_setLogProb, impl/repeatSubMatrix.c:11-35"""
        if base >= self.ALPHABET_SIZE - 1:
            assert base == self.ALPHABET_SIZE - 1  # beyond N the reference aborts (:22)
            base = 0
        idx = (base if strand else 3 - base) * self.R * self.R + underlying * self.R + observed
        assert 0 <= idx < len(self.flat)
        return idx

    def log_prob(self, base, strand, observed, underlying):
        """repeatSubMatrix_getLogProb, impl/repeatSubMatrix.c:37-43"""
        return self.flat[self.index(base, strand, observed, underlying)]


def rle_gap_prob_x(m: po.Model, x: int) -> float:
    """getRleNucleotideGapProbX, impl/stateMachine.c:722-724"""
    return _nucleotide_gap_prob(m.ex, symbol_strip_repeat_count(x))


def rle_gap_prob_y(m: po.Model, y: int) -> float:
    """getRleNucleotideGapProbY, impl/stateMachine.c:726-731 (the base prior is commented out there)"""
    return _nucleotide_gap_prob(m.ey, symbol_strip_repeat_count(y))


def rle_match_prob(m: po.Model, rsm: RepeatSubMatrix, x: int, y: int) -> float:
    """getRleNucleotideMatchProb, impl/stateMachine.c:733-738"""
    x_base = symbol_strip_repeat_count(x)
    return _nucleotide_match_prob(m, x_base, symbol_strip_repeat_count(y)) + 2.3025 * rsm.log_prob(x_base, rsm.strand, symbol_get_repeat_length(y),
                                                                                                   symbol_get_repeat_length(x))


_nucleotide_gap_prob, _nucleotide_match_prob = po.gap_prob, po.match_prob  # impl/stateMachine.c:363-383


@contextlib.contextmanager
def _emissions_replaced(rsm: RepeatSubMatrix):
    """posterior_oracle.cell reads gap_prob(table, symbol) and match_prob(model, x, y) from its module: the run-length ones for one call.
    The gap functions strip the count and are otherwise the nucleotide ones, for x and y alike, so one function serves both tables."""
    saved = po.gap_prob, po.match_prob
    po.gap_prob = lambda table, c: _nucleotide_gap_prob(table, symbol_strip_repeat_count(c))
    po.match_prob = lambda m, a, b: rle_match_prob(m, rsm, a, b)
    try:
        yield
    finally:
        po.gap_prob, po.match_prob = saved


def posterior(model, rsm: RepeatSubMatrix, sx, sy, anchors=(), **kw):
    """posterior_oracle.posterior with run-length emissions; sx, sy: Symbols with counts"""
    with _emissions_replaced(rsm):
        return po.posterior(model, sx, sy, anchors, **kw)


def posterior_dynamic(model, rsm: RepeatSubMatrix, sx, sy, anchors, expansions, **kw):
    """posterior_dynamic_oracle.posterior_dynamic with run-length emissions"""
    with _emissions_replaced(rsm):
        return pdo.posterior_dynamic(model, sx, sy, anchors, expansions, **kw)


def forward_probability(model, sx, sy, anchors=(), expansion=20, ragged_left=False, ragged_right=False, rsm: RepeatSubMatrix = None, band=None):
    """computeForwardProbability, impl/pairwiseAligner.c:849-903: the forward diagonals, then diagonalCalculationTotalProbability at the
    last diagonal, where no diagonal lies beyond it: dpDiagonal_dotProduct with the end states.  rsm None: the nucleotide emissions.
    band: (L, R) in place of band_construct's."""
    m = model if isinstance(model, po.Model) else po.Model(model)
    sx, sy = [int(c) for c in sx], [int(c) for c in sy]
    n = len(sx) + len(sy)
    if n == 0:  # :860-862
        return 0.0
    L, R = band if band is not None else po.ph.band(anchors, len(sx), len(sy), expansion)
    L, R = [int(v) for v in L], [int(v) for v in R]
    with (_emissions_replaced(rsm) if rsm is not None else contextlib.nullcontext()):
        d2, d1 = None, po.Diag(0, L[0], R[0], lambda k: po.start_prob(ragged_left, k))  # :868-870
        for d in range(1, n + 1):  # :874-879
            cur = po.Diag(d, L[d], R[d])
            po.diagonal_calculation(m, cur, d1, d2, sx, sy, po.fwd)
            d2, d1 = d1, cur
        back = po.Diag(n, L[n], R[n], lambda k: po.end_prob(m, ragged_right, k))  # :884-886
        return po.diag_dot(d1, back)  # :887, :578-596 with no backward diagonal n + 1


def rle_string(s: str):
    """rleString_construct, impl/rle.c:7-38 -> (rleString, repeatCounts)"""
    chars, counts = [], []
    k = 1
    for i in range(len(s)):
        if i + 1 == len(s) or s[i] != s[i + 1]:
            chars.append(s[i])
            counts.append(k)
            k = 1
        else:
            k += 1
    return "".join(chars), counts


def char_to_symbol(c: str) -> int:
    """convertNucleotideCharToSymbol, impl/stateMachine.c:25-42"""
    return {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3}.get(c, 4)


def rle_compress(s: str, max_repeat_exclusive: int):
    """rleString_construct, then rleString_constructSymbolString over the whole string: (bases, clamped counts)"""
    chars, counts = rle_string(s)
    sym = [symbol_add_repeat_count(char_to_symbol(c), k, max_repeat_exclusive) for c, k in zip(chars, counts)]
    return [symbol_strip_repeat_count(v) for v in sym], [symbol_get_repeat_length(v) for v in sym]
