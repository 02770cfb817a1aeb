"""The reference's extraction with indelSizeForSVHandling > 0, restated over tests/extract_oracle.py.  TEST INFRASTRUCTURE ONLY.

Restates extractReadSubstringsAtVariantPositions (impl/htsIntegration.c:1725-1755) and nothing more: the variants are divided
into small and structural by isStructuralVariant (:1727-1732), extractReadSubstringsAtVariantPositions2 -- extract_oracle's
extract_chunk -- walks each class alone (:1741-1742), and mergeVariantTypeSeparatedReadLists (:1675-1719) joins the two results
per read: a read either walk lists is listed, with the substrings of both.

Two assumptions: the reference lists the merged reads in the iteration order of a hash over read names,
which nothing in it determines -- here reads keep their index; and it merges by read name, here by read index.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import extract_oracle as eo


def sub_chunk(chunk, which):
    """the chunk over the variants `which` (ascending indices) alone, same reads"""
    return dataclasses.replace(chunk, variant_pos=np.asarray(chunk.variant_pos, np.int64)[which], alleles=[chunk.alleles[v] for v in which],
                               is_sv=np.asarray(chunk.is_sv, np.uint8)[which])


def extract_chunk(chunk, opts):
    """extract_oracle.extract_chunk's result for the split walk: variants in the chunk's order, the status and substrings merged"""
    is_sv = np.asarray(chunk.is_sv) != 0
    n_reads = len(chunk.read_pos)
    variants = [None] * len(is_sv)
    status = np.zeros(n_reads, np.uint8)
    subs = [[] for _ in range(n_reads)]
    for which in (np.flatnonzero(~is_sv), np.flatnonzero(is_sv)):  # :1741-1742 small, then sv
        x = eo.extract_chunk(sub_chunk(chunk, which), opts)
        for k, v in enumerate(which):
            variants[v] = x["variants"][k]
        for r in range(n_reads):
            if x["status"][r] != eo.DROPPED:
                # every filter before :1852 ignores the variants: two walks that list a read agree on its list
                assert status[r] in (eo.DROPPED, x["status"][r])
                status[r] = x["status"][r]
            subs[r] += [(int(which[k]), a, b) for k, a, b in x["subs"][r]]
    return dict(variants=variants, status=status, subs=subs)


def extract(chunks, opts):
    """extract_oracle.extract for the split walk: per chunk the arrays mrp_extracted_chunk holds"""
    out = []
    for ch in chunks:
        x = extract_chunk(ch, opts)
        entries = [[] for _ in x["variants"]]
        for r, lst in enumerate(x["subs"]):
            for v, a, b in lst:
                entries[v].append((r, eo.substring_symbols(ch, r, a, b)))
        out.append(dict(ref_aln_start=np.array([w["aln_start"] for w in x["variants"]], np.int64),
                        ref_aln_stop_incl=np.array([w["aln_stop"] for w in x["variants"]], np.int64),
                        alleles=[w["alleles"] for w in x["variants"]], read_status=x["status"],
                        read_n_substrings=np.array([len(s) for s in x["subs"]], np.int32), entries=entries))
    return out
