"""Hand-built chunks for the SV split of the extraction: small and structural variants whose windows
interact, over a reference long enough for the shipped expansions.  Reads are tests/extract_cases.py's: (pos, CIGAR text, mapq,
flag), bases cycling A C G T."""
from __future__ import annotations

import dataclasses

import numpy as np

from margin_amd import capi, synth
from tests import extract_cases as ec

SV_SIZE = 50  # indelSizeForSVHandling of params/phase/allParams.phase_vcf.ont.sv.json
OPTS = dict(capi.shipped_extract_options(), expansion_small=12, expansion_sv=64, indel_size_for_sv_handling=SV_SIZE)
UNSPLIT = dict(OPTS, indel_size_for_sv_handling=0)


def reference(n: int, seed: int = 5) -> str:
    return "".join(np.random.default_rng([seed, 43]).choice(list("ACGT"), size=n))


def snp(ref: str, pos: int):
    """(pos, [REF, another base], small)"""
    return (pos, [ref[pos], "ACGT"[("ACGT".index(ref[pos]) + 1) % 4]], 0)


def ins(ref: str, pos: int, n: int = 60):
    """(pos, [REF, REF + n bases], structural for n >= SV_SIZE)"""
    return (pos, [ref[pos], ref[pos] + ("GATTACA" * (n // 7 + 1))[:n]], 1 if n + 1 > SV_SIZE else 0)


def make(ref: str, variants, reads, chunk_start: int = 0, chunk_end=None):
    """extract_cases.make over the overlap [0, len(ref)) of a reference of one's own"""
    c = ec.make([], reads)
    c = dataclasses.replace(c, overlap_start=0, overlap_end=len(ref), chunk_start=chunk_start, chunk_end=len(ref) if chunk_end is None else chunk_end,
                            reference=ref, variant_pos=np.array([v[0] for v in variants], np.int64), alleles=[list(v[1]) for v in variants],
                            is_sv=np.array([v[2] for v in variants], np.uint8))
    assert capi.mark_structural_variants(c, SV_SIZE).tolist() == c.is_sv.tolist()  # the flags are those the reference would set
    return c


REF = reference(1200)


def delayed_start(sv_at: int = 620):
    """a small variant at 600 (window [588, 613]) before a structural one (sv_at 620: window [556, 685]), one read 1000M from 100"""
    return make(REF, [snp(REF, 600), ins(REF, sv_at)], [(100, "1000M", 60, 0)])


def interleaved(n_small: int = 150, n_sv: int = 70, length: int = 4000):
    """one read over n_small small variants interleaved with n_sv structural ones: more than one 64-entry trip per class"""
    ref = reference(length + 400, seed=9)
    pos_small = np.linspace(210, length + 100, n_small).astype(int)
    pos_sv = np.linspace(230, length + 90, n_sv).astype(int) + 3
    variants = sorted([snp(ref, int(p)) for p in pos_small] + [ins(ref, int(p)) for p in pos_sv], key=lambda v: (v[0], v[2]))
    return make(ref, variants, [(200, f"{length}M", 60, 0)])


def synthetic(seed: int):
    """a 20 kb aligned chunk at about 8x with a variant every 500 bases, about a quarter of them structural by the loader's rule"""
    c = synth.make_aligned_chunk(seed, overlap_bp=20_000, coverage=8.0, variant_every=500, sv_share=0.25)
    return dataclasses.replace(c, is_sv=capi.mark_structural_variants(c, SV_SIZE))
