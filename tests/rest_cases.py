"""The rest of an extracted chunk (mrp_string_chunk_rest_from_extracted), restated in Python from the rules in
include/margin_rphmm.h, and the inputs of its tests.  TEST INFRASTRUCTURE ONLY.

A chunk's variants are split with dataclasses.replace into the primary set and the filtered set; both are extracted over the same
reads (tests/extract_oracle.py, so no device is needed); the rest follows from the two extractions, the caller's keep mask, the
reads' strands and the bubbles' variants."""
from __future__ import annotations

import dataclasses

import numpy as np

from margin_amd import synth
from tests import extract_cases as ec
from tests import extract_oracle as xo

DROPPED, KEPT, FILTERED = xo.DROPPED, xo.KEPT, xo.FILTERED


def subset(chunk, idx):
    """chunk with the variants idx only (ascending), everything else as it was"""
    idx = [int(i) for i in idx]
    return dataclasses.replace(chunk, variant_pos=np.ascontiguousarray(chunk.variant_pos[idx], np.int64), alleles=[chunk.alleles[i] for i in idx],
                               is_sv=np.ascontiguousarray(chunk.is_sv[idx], np.uint8))


def split_variants(chunk, every: int = 5):
    """one variant in `every` goes to the filtered set, and the chunk's first pair of variants at one position goes there whole
    -> (primary chunk, filtered chunk, filtered indices)"""
    n = len(chunk.variant_pos)
    pick = np.zeros(n, bool)
    pick[every // 2::every] = True
    pos = np.asarray(chunk.variant_pos)
    same = np.flatnonzero(pos[1:] == pos[:-1])
    if len(same):
        pick[same[0]] = pick[same[0] + 1] = True
    fidx = np.flatnonzero(pick)
    return subset(chunk, np.flatnonzero(~pick)), subset(chunk, fidx), fidx


def genotypes(fchunk, seed: int) -> np.ndarray:
    """a gt per filtered variant: two distinct alleles mostly, every fourth variant homozygous"""
    rng = np.random.default_rng([seed, 31])
    gt = np.zeros((len(fchunk.alleles), 2), np.int32)
    for v, al in enumerate(fchunk.alleles):
        g = rng.choice(len(al), size=2, replace=False)
        gt[v] = (g[0], g[0]) if v % 4 == 3 else g
    return gt


def keep_mask(x, seed: int, share: float) -> np.ndarray:
    """the caller's downsampling as a mask over every read of the chunk"""
    return np.ascontiguousarray(np.random.default_rng([seed, 37]).random(len(x["read_status"])) < share, np.uint8)


def rest_reference(x, xf, keep, strand, bubble_variant, fvariant_pos, gt, chunk_start: int, chunk_end: int):
    """x, xf: extract_oracle.extract results of one chunk over its primary and its filtered variants.
    -> (filtered_read list, rest dict as capi.string_chunk_rest_struct takes it, or None for the empty rest)"""
    n = len(x["read_status"])
    sx, sf = x["read_status"], xf["read_status"]
    kept = np.ones(n, bool) if keep is None else np.asarray(keep) != 0
    primary = [sx[r] == KEPT and kept[r] for r in range(n)]
    low_mapq = [r for r in range(n) if sx[r] == FILTERED]                    # (i)
    masked = [r for r in range(n) if sx[r] == KEPT and not kept[r]]          # (ii)
    only_there = [r for r in range(n) if sx[r] == DROPPED and sf[r] == KEPT]  # (iii)
    flist = low_mapq + masked + only_there
    nv = len(xf["alleles"])
    if not flist and nv == 0:
        return [], None
    findex = {r: f for f, r in enumerate(flist)}
    taggable = set(low_mapq) | set(masked)
    fsubs = [sorted(((findex[r], s) for r, s in x["entries"][int(v)] if r in taggable), key=lambda t: t[0]) for v in bubble_variant]
    variants = []
    for v in range(nv):
        entries = []
        if chunk_start <= int(fvariant_pos[v]) < chunk_end:
            for r, s in xf["entries"][v]:  # ascending reads
                if sf[r] == KEPT:
                    entries.append((r if primary[r] else n + findex[r], s))
        variants.append((list(xf["alleles"][v]), (int(gt[v][0]), int(gt[v][1])), entries))
    return flist, dict(forward_strand=np.array([strand[r] for r in flist], np.uint8), fsubs=fsubs, variants=variants)


def assert_rest_equal(got, flist, want):
    """got: capi.ExtractedRest"""
    if want is None:
        assert got.rest is None and got.block is None and len(got.filtered_read) == 0
        return
    assert got.rest is not None
    assert got.filtered_read.tolist() == list(flist)
    assert got.rest["forward_strand"].tolist() == want["forward_strand"].tolist()
    assert len(got.rest["fsubs"]) == len(want["fsubs"])
    for b, (g, w) in enumerate(zip(got.rest["fsubs"], want["fsubs"])):
        assert [f for f, _ in g] == [f for f, _ in w], b
        assert all((s == t).all() if len(s) == len(t) else False for (_, s), (_, t) in zip(g, w)), b
    assert len(got.rest["variants"]) == len(want["variants"])
    for v, ((ga, gg, ge), (wa, wg, we)) in enumerate(zip(got.rest["variants"], want["variants"])):
        assert gg == wg, v
        assert len(ga) == len(wa) and all(len(a) == len(b) and (a == b).all() for a, b in zip(ga, wa)), v
        assert [r for r, _ in ge] == [r for r, _ in we], v
        assert all(len(s) == len(t) and (s == t).all() for (_, s), (_, t) in zip(ge, we)), v


# ---- hand-built chunks (tests/extract_cases.py: the overlap slice is genome 100..139, windows of +-2) ----

def _alts(rel: int):
    return [c for c in "ACGT" if c != ec.REF[rel]]


SNP110 = ec.SNP110
SNP125 = (125, [ec.REF[25], _alts(25)[0]], 0)   # window [23, 28)
TRI126 = (126, [ec.REF[26]] + _alts(26)[:2], 0)
SNP134 = (134, [ec.REF[34], _alts(34)[0]], 0)   # outside a chunk that ends at 130


def hand_cases():
    """-> list of (name, chunk of all variants, indices of the filtered ones, gt of those, keep mask or None)"""
    rd = [(100, "40M", 3, 0),       # 0: low mapq                                   -> (i)
          (100, "40M", 60, 0),      # 1: primary
          (100, "40M", 60, 0x10),   # 2: kept, masked out by the caller, reverse    -> (ii)
          (115, "20M", 60, 0),      # 3: no primary variant at or after its start   -> (iii)
          (100, "40M", 60, 0x10)]   # 4: primary, reverse
    return [
        # every kind of filtered read; the masked read's entries at the filtered variants carry n_reads + f; the variant at 134 lies
        # outside [100, 130) and is listed without entries; a homozygous gt; a three-allele variant with gt (2, 1)
        ("kinds", ec.make([SNP110, SNP125, TRI126, SNP134], rd, chunk_start=100, chunk_end=130), [1, 2, 3], [(0, 1), (2, 1), (1, 1)],
         np.array([1, 1, 0, 1, 1], np.uint8)),
        # a read of kind (iii) is the only entry of the filtered variant: read 0 ends before it, read 1 starts behind the primary one
        ("only_iii", ec.make([SNP110, SNP125], [(100, "14M", 60, 0), (115, "20M", 60, 0x10)]), [1], [(1, 0)], None),
        # filtered variants, no filtered read
        ("no_filtered_read", ec.make([SNP110, SNP125], [(100, "40M", 60, 0), (100, "40M", 60, 0x10)]), [1], [(0, 1)], None),
        # filtered reads, no filtered variant
        ("no_filtered_variant", ec.make([SNP110], [(100, "40M", 60, 0), (100, "40M", 2, 0), (100, "40M", 60, 0)]), [], [], np.array([1, 1, 0], np.uint8)),
        # the empty rest
        ("empty", ec.make([SNP110], [(100, "40M", 60, 0), (100, "40M", 60, 0x10)]), [], [], None),
    ]


def split_hand(chunk, fidx):
    n = len(chunk.variant_pos)
    return subset(chunk, [v for v in range(n) if v not in fidx]), subset(chunk, list(fidx))


def synthetic(seed: int):
    """the issue's synthetic input: an 8 kb / 8x aligned chunk with one variant in five filtered"""
    return synth.make_aligned_chunk(seed, overlap_bp=8_000, coverage=8.0)
