"""Inputs of the downsampling tests (host and device).  TEST INFRASTRUCTURE ONLY.

A case is one chunk as the definition sees it: per read its status, l (the variants it saved a substring for) and h (alnReadLength), and
V, the chunk's variant count.  Every case is made for max_depth D = 4, so one call of the seam can hold them all."""
from __future__ import annotations

import numpy as np

D = 4
DROPPED, KEPT, FILTERED = 0, 1, 2


def case(name, l, h, V, status=None):
    l, h = np.asarray(l, np.int32), np.asarray(h, np.int32)
    status = np.full(len(l), KEPT, np.uint8) if status is None else np.asarray(status, np.uint8)
    return dict(name=name, status=status, l=l, h=h, V=int(V))


def edge_cases():
    """-> [(case, expected probabilities of its reads as (numerator, denominator) or None where only the oracle is asked)]"""
    return [
        (case("no read at all", [], [], 2), []),
        (case("no kept read", [5, 5, 5], [9, 9, 9], 2, status=[DROPPED, FILTERED, DROPPED]), [(0, 1)] * 3),
        (case("one kept read", [9], [100], 2), [(8, 9)]),
        (case("two kept reads", [5, 5], [10, 20], 2), [(3, 5), (1, 1)]),
        (case("shallow: total < D V", [3, 4], [10, 20], 2), [(1, 1), (1, 1)]),
        (case("shallow: no substring at all", [0, 0], [10, 0], 3), [(1, 1), (1, 1)]),
        # 8 / 2 is not below 4: downsampled, and the constraint takes every read whole -- the read with l == 0 and h == 0 too
        (case("total == D V exactly", [4, 0, 4], [7, 0, 9], 2), [(1, 1), (1, 1), (1, 1)]),
        (case("B == T exactly at a read", [4, 4, 4], [30, 20, 10], 2), [(1, 1), (1, 1), (0, 1)]),
        (case("equal ratios straddle the threshold", [3, 3, 3, 3], [6, 6, 6, 6], 2), [(1, 1), (1, 1), (2, 3), (0, 1)]),
        (case("equal ratios, unequal lengths", [2, 4, 6, 1], [1, 2, 3, 9], 2), [(1, 1), (1, 1), (1, 6), (1, 1)]),
        (case("l == 0 with h > 0 and with h == 0", [0, 0, 5, 6], [5, 0, 10, 10], 2), [(1, 1), (0, 1), (1, 1), (1, 2)]),
        # rank differs from index: the draw of a kept read is numbered among the kept reads
        (case("dropped and low-mapq reads between kept ones", [7, 5, 3, 5, 9, 5], [1, 10, 1, 20, 1, 5], 2,
              status=[DROPPED, KEPT, FILTERED, KEPT, DROPPED, KEPT]), [(0, 1), (3, 5), (0, 1), (1, 1), (0, 1), (0, 1)]),
        # chunkSize == 0 (htsIntegration.c:1174): never an extraction's result, the seam and the host function take it all the same
        (case("no variants", [1, 2], [5, 5], 0), [(0, 1), (0, 1)]),
        (case("no variants, no substring", [0, 0], [5, 5], 0), [(0, 1), (0, 1)]),
    ]


def random_case(rng, n_kept: int, downsampled: bool, ties: bool = False):
    """n_kept kept reads with dropped and low-mapq reads between them; V is chosen so that the chunk is (not) downsampled"""
    n = n_kept + int(rng.integers(0, max(2, n_kept // 3 + 2)))
    status = np.zeros(n, np.uint8)
    status[rng.permutation(n)[:n_kept]] = KEPT
    other = np.flatnonzero(status != KEPT)
    status[other] = rng.choice([DROPPED, FILTERED], size=len(other))
    l = rng.integers(0, 40, size=n).astype(np.int32)
    l[rng.random(n) < 0.05] = 0
    # with ties: few distinct ratios, so that equal ratios straddle the threshold
    h = (l * rng.integers(1, 4, size=n) if ties else rng.integers(1, 60_000, size=n)).astype(np.int32)
    h[(l == 0) & (rng.random(n) < 0.5)] = 0
    total = int(l[status == KEPT].sum())
    if downsampled:
        V = max(1, total // (D * int(rng.integers(2, 5)))) if total >= D else 0
    else:
        V = total // D + 1 + int(rng.integers(0, 3))
    return case(f"random {n_kept} {'deep' if downsampled else 'shallow'}{' ties' if ties else ''}", l, h, V, status)


def extracted(c):
    """the case as the arrays of one mrp_extracted_chunk (capi.extracted_struct): only n_variants, read_status and read_n_substrings are
    read by the downsampling, so the variants carry no allele and no entry"""
    V, z = c["V"], np.zeros
    return dict(ref_aln_start=z(V, np.int64), ref_aln_stop_incl=z(V, np.int64), allele_first=z(V + 1, np.int64), allele_off=z(0, np.int64),
                allele_len=z(0, np.int32), read_status=c["status"], read_n_substrings=c["l"], entry_first=z(V + 1, np.int64), entry_read=z(0, np.int32),
                entry_off=z(0, np.int64), entry_len=z(0, np.int32), pool=z(0, np.uint8))
