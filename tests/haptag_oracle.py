"""The reference's filtered-read haplotagging and filtered-variant phasing, restated in Python.  TEST INFRASTRUCTURE ONLY.

Restates bubbleGraph_partitionFilteredReadsFromVcfEntries (impl/bubbleGraph.c:1749-1943), its twin
bubbleGraph_partitionFilteredReadsFromPhasedVcfEntries (:1945-2138) and bubbleGraph_phaseVcfEntriesFromHaplotaggedReads
(:2140-2351) on the inputs the C-ABI takes (include/margin_rphmm.h, mrp_haptag_sites): a site is
(alleles, (i, j), entries) with alleles a list of uint8 symbol arrays, (i, j) the two compared allele indices and entries a
list of (read index, uint8 symbol array) in the order buildVcfEntryToReadSubstringsMap (:1281-1323) lists them.  The
pair-HMM forward probability is oracle/pairhmm.py's; logAddExact uses math.log / math.exp.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import pairhmm as ph

NOT_VISITED, CIS, TRANS, TIE = 0, 1, 2, 3  # MRP_VARIANT_*


def log_add_exact(x: float, y: float) -> float:
    """sonLib stMath_logAddExact (the formula mrp_kernels.hip and rphmm_frame.c state)"""
    if x == -math.inf:
        return y
    if y == -math.inf:
        return x
    return x + math.log(1.0 + math.exp(y - x)) if x > y else y + math.log(1.0 + math.exp(x - y))


def _f32(v: float) -> float:
    return float(np.float32(v))


def partition_filtered_reads(fwd: ph.Model, rev: ph.Model, sites, n_reads: int, read_forward_strand, expansion: int = 4):
    """bubbleGraph_partitionFilteredReadsFromVcfEntries -> (hap int32 [n_reads], h1, h2 float64 [n_reads]).
    (i, j) of a site = gF->haplotypeString1 / 2 at the primary bubble (:1765-1766)."""
    h1, h2 = [0.0] * n_reads, [0.0] * n_reads                       # :1753-1758 every read starts at 0
    for alleles, (i, j), entries in sites:                          # :1763 primary bubbles of the fragment, in order
        if i == j:                                                  # :1780 hap1 == hap2: the same allele pointer
            continue
        if not entries:                                             # :1797-1801 nothing to phase with
            continue
        reads = [entries[q] for q in range(len(entries) - 1, -1, -1)]  # :1816-1819 b->reads[j] = stList_pop(...): reversed
        cache, sup = {}, []
        for r, sub in reads:                                        # :1841-1874 in b->reads order
            key = bytes(np.asarray(sub, dtype=np.uint8))            # cachedScores is keyed by the substring alone
            if key in cache:                                        # :1847-1853 copy the first scored (= LAST listed) read's
                sup.append(cache[key])
                continue
            m = fwd if read_forward_strand[r] else rev              # :1843-1845 the owner's strand picks the state machine
            # :1832 anchorPairs is always empty; :1869 the support is stored as a float
            s = tuple(_f32(ph.forward_probability(m, alleles[a], sub, (), expansion)) for a in (i, j))
            cache[key] = s
            sup.append(s)
        for (r, _), (s1, s2) in zip(reads, sup):                    # :1877-1889 in fp64, float operands widened
            h1[r] += s1 - log_add_exact(s1, s2)
            h2[r] += s2 - log_add_exact(s2, s1)
    hap = [1 if a > b else (2 if b > a else 0) for a, b in zip(h1, h2)]  # :1913-1925
    return np.array(hap, dtype=np.int32), np.array(h1), np.array(h2)


def partition_filtered_reads_from_phased_vcf(fwd, rev, sites, n_reads, read_forward_strand, expansion: int = 4):
    """bubbleGraph_partitionFilteredReadsFromPhasedVcfEntries (:1945-2138, called at tools/tagFromPhasedVcf.c:308): the same
    body, (i, j) = (gt1, gt2) of the phased VCF entry instead of the fragment's alleles."""
    return partition_filtered_reads(fwd, rev, sites, n_reads, read_forward_strand, expansion)


def phase_filtered_variants(fwd: ph.Model, rev: ph.Model, variants, n_reads: int, read_forward_strand, read_hap, expansion: int = 4,
                            sv_threshold: int = 512):
    """bubbleGraph_phaseVcfEntriesFromHaplotaggedReads -> (state int32, cis, trans float64) per variant; (i, j) = (gt1, gt2);
    read_hap[r] in (1, 2) for a tagged read (the name sets of :2145-2158), anything else untagged.  The chunk filter on the
    root entry's position (:2179) is the caller's: variants outside the chunk are not passed."""
    n = len(variants)
    state, cis, trans = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
    for v, (alleles, (g1, g2), entries) in enumerate(variants):
        if g1 == g2:                                                # :2174 no homozygous
            continue
        if not entries:                                             # :2186-2192 no reads: not updated
            continue
        a_sym, b_sym = alleles[g1], alleles[g2]                     # :2195-2205
        c = t = 0.0
        cache = {}
        for r, sub in entries:                                      # :2220-2289 in list order
            h = int(read_hap[r])
            if h not in (1, 2):                                     # :2226-2235 untagged: neither scored nor cached
                continue
            key = bytes(np.asarray(sub, dtype=np.uint8))
            if key in cache:                                        # :2238-2241 the FIRST tagged read with it owns the scores
                sa, sb = cache[key]
            else:
                m = fwd if read_forward_strand[r] else rev          # :2248-2250

                def score(al):                                      # :2253-2263 anchored past referenceExpansionForStructuralVariants
                    long = len(sub) > sv_threshold or len(al) > sv_threshold
                    return ph.forward_probability(m, al, sub, ph.kmer_anchors(al, sub) if long else (), expansion)
                sa, sb = score(a_sym), score(b_sym)                 # supports stay double
                cache[key] = (sa, sb)
            l = log_add_exact(sa, sb)                               # :2280-2287
            c += (sa - l) if h == 1 else (sb - l)
            t += (sb - l) if h == 1 else (sa - l)
        cis[v], trans[v] = c, t
        state[v] = CIS if c > t else (TRANS if t > c else TIE)      # :2295-2328 (a tie sets gt to -1 | -1)
    return state, cis, trans


def assert_margins_decisive(a, b, what: str = ""):
    """every |a - b| is exactly 0 or larger than 1e-6 * max(1, |a|, |b|): a decision compared across two implementations
    whose totals may differ by ~1e-12 cannot then flip"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    ok = (d == 0) | (d > 1e-6 * np.maximum(1.0, np.maximum(np.abs(a), np.abs(b))))
    assert ok.all(), f"{what}: {int((~ok).sum())} margins too close to call"
