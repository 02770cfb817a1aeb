"""The Python restatement of getPosteriorProbsWithBanding (tests/posterior_oracle.py) against the pins that exist without it: the
oracle's complete matrices (pho_full_matrices: bwd_t, the total of every diagonal, the posteriors) and the reference's own test of
AGCG / AGTTCG (tests/pairwiseAlignerTest.c:257-340, checkAlignedPairs :362-397)."""
import math

import numpy as np

from margin_amd import capi, synth
from oracle import pairhmm as ph
from tests import posterior_oracle as po


def omodel(m):
    return ph.Model.from_buffer_copy(bytes(m))


def test_log_add_is_the_oracles():
    rng = np.random.default_rng(3)
    vals = [-math.inf, 0.0, -7.5, 7.5, 1.0, 2.5, 4.5] + [float(v) for v in rng.normal(0, 5, 400)]
    for a in vals:
        for b in vals[:60]:
            assert po.log_add(a, b) == ph.log_add(a, b) or (math.isnan(po.log_add(a, b)) and math.isnan(ph.log_add(a, b)))


def test_totals_and_posteriors_equal_the_complete_matrices():
    """unanchored, not ragged, one traceback: every total the restatement recomputes is pho_full_matrices' diag_totals at that
    diagonal bit for bit; for n <= 10 (one total, taken at the last diagonal, which is the forward total) every exp(v) is its posterior"""
    rng = np.random.default_rng(21)
    m = capi.PairHmm.default_nucleotide()
    shapes = [(4, 6), (3, 3), (1, 1), (5, 5), (2, 7), (12, 9), (30, 29), (41, 37)]
    for lx, ly in shapes:
        sx = synth.random_sequence(rng, lx)
        sy = synth.evolve_sequence(rng, sx, 0.05, 0.05, 0.05)
        sy = np.array((list(sy) + [0] * ly)[:ly], dtype=np.uint8)
        e = 2 * (max(lx, ly) + 1)  # the whole matrix in the oracle's band
        tf, tb, diag, post = ph.full_matrices(omodel(m), sx, sy, e)
        (match, _, _), info = po.posterior(m, sx, sy, [], expansion=e, threshold=1e-300, min_diags=1000, traceback_diagonals=40)
        assert len(info) == 1 and info[0][:3] == (lx + ly, 0, lx + ly)
        assert [d for d, _ in info[0][4]] == list(range(lx + ly, 0, -10))
        for d, total in info[0][4]:
            assert total == diag[d], (lx, ly, d)
        if lx + ly <= 10:
            assert len(match) == lx * ly
            for w, x, y, v in match:
                assert math.exp(v) == post[x, y]


def test_agcg_agttcg():
    """test_diagonalDPCalculations (:257-340): the four match pairs; checkAlignedPairs' invariants (:362-397)"""
    sx, sy = capi.symbols_from_chars("AGCG"), capi.symbols_from_chars("AGTTCG")
    m = capi.PairHmm.default_nucleotide()
    for thr in (0.2, 0.01):
        (match, gx, gy), _ = po.posterior(m, sx, sy, [], expansion=2, threshold=thr, with_gaps=True)
        po.check_aligned_pairs(match, 4, 6)
        po.check_aligned_pairs(gx, 4, 6, x_gaps=True)
        po.check_aligned_pairs(gy, 4, 6, y_gaps=True)
        got = {(x, y) for _, x, y, _ in match}
        assert {(0, 0), (1, 1), (2, 4), (3, 5)} <= got
        if thr == 0.2:
            assert got == {(0, 0), (1, 1), (2, 4), (3, 5)}


def test_empty_pair_and_one_symbol():
    m = capi.PairHmm.default_nucleotide()
    assert po.posterior(m, [], []) == (([], [], []), [])
    (match, gx, gy), info = po.posterior(m, [], [0, 1, 2, 3, 0], with_gaps=True)
    assert match == [] and gx == [] and len(gy) == 5 and len(info) == 1
