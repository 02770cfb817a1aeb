"""The ML repeat counts of a run-length consensus from its reads' posterior matches: a sequential restatement of the reference
(/impl of MarginPolish), the definition mrp_ml_repeat_counts is held to bit for bit.

    poa_augment's match loop                               impl/poa.c:324-340        observations()
    getAlignedPairsWithIndelsCroppingReference (x_shift)   impl/poa.c:621-665, the read loop :682-707
    pairCoordinateCorrectionFn pops from the end           impl/pairwiseAligner.c:1109-1123   (walk_backwards)
    repeatSubMatrix_getLogProb (index, N as A)             impl/repeatSubMatrix.c:11-43      table_slice()
    repeatSubMatrix_getLogProbForGivenRepeatCount          impl/repeatSubMatrix.c:65-84      log_probs()
    repeatSubMatrix_getMinAndMaxRepeatCountObservations    impl/repeatSubMatrix.c:86-113     min_and_max()
    repeatSubMatrix_getMLRepeatCount                       impl/repeatSubMatrix.c:124-143    ml_repeat_count()
    getRepeatLengthProbForHaplotype, getMax                impl/repeatSubMatrix.c:145-167
    repeatSubMatrix_getPhasedMLRepeatCount                 impl/repeatSubMatrix.c:169-238    phased_ml_repeat_count()
    poa_estimateRepeatCountsUsingBayesianModel             impl/poa.c:1715-1727              estimate()
    poa_estimatePhasedRepeatCountsUsingBayesianModel       impl/poa.c:1729-1756, called from polish.c:736-739
    rleString_expand                                       impl/rle.c:145-155                rle_expand()

Every sum is taken in list order with a multiply and an add as two IEEE double operations (numpy's elementwise ufuncs never fuse them);
the candidates u of one node are the elements of one vector, which changes no element's arithmetic.

Out of scope, as in the library: getRunLengthMode (repeatSubMatrix == NULL, "for an experiment", poa.c:1703-1706), poaNode_getPhasedMLBase
(never called), and the base weights, inserts and deletes of poa_augment."""
from __future__ import annotations

import math

import numpy as np

PAIR_ALIGNMENT_PROB_1 = 10000000.0
LOG_ZERO = -math.inf


def observations(n_nodes, read_matches, x_shift=None, walk_backwards=False):
    """read_matches[r] = [(x, y, weight)] in the order given -> per node its list of (read, y, weight) (poa.c:324-340): reads ascending
    (:682-707), a read's matches in the order poa_augment receives them -- the reverse of the given order with walk_backwards"""
    obs = [[] for _ in range(n_nodes)]
    for r, matches in enumerate(read_matches):
        shift = 0 if x_shift is None else int(x_shift[r])
        for x, y, w in (reversed(matches) if walk_backwards else matches):
            obs[int(x) + shift].append((r, int(y), int(w)))
    return obs


def table_slice(table, base, strand):
    """repeatSubMatrix_setLogProb, :11-35: N (4) as A, then the strand picks the base or its complement -> [underlying, observed]"""
    if base >= 4:
        base = 0
    return table[base if strand else 3 - base]


def min_and_max(R, obs, read_counts):
    """:86-113 -- min starts at R, so an overlong count never lowers it; a max of R or more becomes R - 1"""
    mn, mx = R, 0
    for r, y, _ in obs:
        c = int(read_counts[r][y])
        if c < mn:
            mn = c
        if c > mx:
            mx = c
    if mx >= R:
        mx = R - 1
    return mn, mx


def log_probs(table, R, base, obs, read_counts, strands, mn, mx):
    """:115-122 over :65-84 -- logProbabilities[u - mn] for u = mn..mx, each LOG_ONE plus the terms in list order, then / 1e7"""
    lp = np.zeros(mx - mn + 1)
    for r, y, w in obs:
        o = min(int(read_counts[r][y]), R - 1)  # :76-77
        lp = lp + table_slice(table, base, bool(strands[r]))[mn:mx + 1, o] * float(w)
    return lp / PAIR_ALIGNMENT_PROB_1


def get_max(values):
    """:153-167 -- the first that is strictly greater"""
    best, at = values[0], 0
    for i in range(1, len(values)):
        if values[i] > best:
            best, at = values[i], i
    return at, float(best)


def ml_repeat_count(table, R, base, obs, read_counts, strands):
    """:124-143 -> (count, log probability, candidates)"""
    mn, mx = min_and_max(R, obs, read_counts)
    if mn == R:
        return 0, LOG_ZERO, 0
    at, best = get_max(log_probs(table, R, base, obs, read_counts, strands, mn, mx))
    return at + mn, best, mx - mn + 1


def phased_ml_repeat_count(table, R, base, obs, read_counts, strands, read_in_hap, log_het_substitution):
    """:169-238 -> (count, log probability, candidates)"""
    mn, mx = min_and_max(R, obs, read_counts)
    if mn == R:
        return 0, LOG_ZERO, 0
    hap1 = [o for o in obs if read_in_hap[o[0]]]  # :185-190, in list order
    hap2 = [o for o in obs if not read_in_hap[o[0]]]
    lp1 = log_probs(table, R, base, hap1, read_counts, strands, mn, mx)
    lp2 = log_probs(table, R, base, hap2, read_counts, strands, mn, mx)
    _, ml2 = get_max(lp2)
    s = float(log_het_substitution)

    def p(i):  # getRepeatLengthProbForHaplotype, :145-151
        same = float(lp2[i])
        return float(lp1[i]) + (same if same > ml2 + s else ml2 + s)

    best, at = p(0), 0
    for i in range(1, mx - mn + 1):  # :212-220: the last that is not smaller
        v = p(i)
        if v >= best:
            best, at = v, i
    return at + mn, best, mx - mn + 1


def estimate(table, symbols, read_counts, strands, read_matches, x_shift=None, walk_backwards=False, read_in_hap=None, log_het_substitution=None):
    """poa.c:1715-1756 for one consensus -> dict(count int32 [nodes] (a 0 stored as 1, :1721-1723), log_prob float64 [nodes],
    non_rle_length, observations, nodes_observed, candidates)"""
    table = np.asarray(table, dtype=np.float64)
    R = table.shape[1]
    obs = observations(len(symbols), read_matches, x_shift, walk_backwards)
    count, lp, cands = np.zeros(len(symbols), np.int32), np.zeros(len(symbols)), 0
    for k, base in enumerate(symbols):
        if read_in_hap is None:
            c, v, n = ml_repeat_count(table, R, int(base), obs[k], read_counts, strands)
        else:
            c, v, n = phased_ml_repeat_count(table, R, int(base), obs[k], read_counts, strands, read_in_hap, log_het_substitution)
        count[k], lp[k] = (1 if c == 0 else c), v
        cands += n
    return dict(count=count, log_prob=lp, non_rle_length=int(count.sum()), observations=sum(len(o) for o in obs),
                nodes_observed=sum(1 for o in obs if o), candidates=cands)


def rle_expand(symbols, counts):
    """rleString_expand, rle.c:145-155"""
    return "".join("ACGTN"[int(b)] * int(c) for b, c in zip(symbols, counts))
