"""Seeded synthetic chunks for the stRPHmm hot path (inputs only -- no algorithm lives here).

Generators of profile-byte chunks:

* :func:`make_ont_chunk` -- BASELINE.json config 2 as restated in SURVEY.md section 8(d): a region
  with biallelic het sites at uniform positions, 30x log-normal reads, 50/50 strand and
  haplotype, 8 % allele error, profile bytes ``min(255, round(30*delta))`` with the supported
  allele at 0 (the encoding of bubbleGraph.c:2423-2435).
* :func:`make_unit_test_chunk` -- the shape used by the reference's own randomised system tests
  (tests/stRPHmmTest.c:13-160): 1..9 alleles per site, chosen allele 0 and every other allele 100.

A chunk is plain numpy: the site table, one packed uint8 profile pool and a per-read table.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np


@dataclass
class Read:
    name: str
    ref_start: int      # first site (stProfileSeq.refStart)
    length: int         # number of sites (stProfileSeq.length)
    strand: int         # 1 = forward
    hap: int            # true haplotype (0/1), for scoring only
    pool_off: int       # offset of profileProbs in Chunk.pool
    nbytes: int


@dataclass
class Chunk:
    allele_number: np.ndarray            # uint32[n_sites]
    allele_offset: np.ndarray            # int64[n_sites + 1]
    sub: np.ndarray                      # uint16[sum A^2]  (site-major, [from*A+to])
    prior: np.ndarray                    # uint16[sum A]
    pool: np.ndarray                     # uint8[pool_bytes]
    reads: List[Read] = field(default_factory=list)
    hap1: Optional[np.ndarray] = None
    hap2: Optional[np.ndarray] = None

    @property
    def n_sites(self) -> int:
        return int(self.allele_number.shape[0])

    @property
    def units(self) -> int:
        """het-sites x reads: sum of stProfileSeq.length (the metric's unit of work)."""
        return int(sum(r.length for r in self.reads))


def _finish(allele_number, reads_raw, hap1, hap2, sub=None) -> Chunk:
    allele_number = np.asarray(allele_number, dtype=np.uint32)
    off = np.zeros(len(allele_number) + 1, dtype=np.int64)
    np.cumsum(allele_number, out=off[1:])
    n_sub = int((allele_number.astype(np.int64) ** 2).sum())
    sub_arr = np.zeros(n_sub, dtype=np.uint16) if sub is None else np.asarray(sub, dtype=np.uint16)
    prior = np.zeros(int(off[-1]), dtype=np.uint16)
    pool_parts, reads, pos = [], [], 0
    for name, start, length, strand, hap, probs in reads_raw:
        probs = np.ascontiguousarray(probs, dtype=np.uint8)
        assert probs.shape[0] == off[start + length] - off[start]
        reads.append(Read(name, int(start), int(length), int(strand), int(hap), pos, int(probs.shape[0])))
        pool_parts.append(probs)
        pos += int(probs.shape[0])
    pool = np.concatenate(pool_parts) if pool_parts else np.zeros(0, dtype=np.uint8)
    return Chunk(allele_number, off, sub_arr, prior, pool, reads, hap1, hap2)


def make_ont_chunk(seed: int = 1, region_bp: int = 1_000_000, n_sites: int = 2000, coverage: float = 30.0,
                   median_len: float = 15_000.0, sigma: float = 0.6, min_len: int = 1000,
                   max_len: int = 100_000, allele_error: float = 0.08,
                   allele_choices: Sequence[int] = (2,), allele_probs: Sequence[float] = (1.0,),
                   length_model: str = "lognormal", normal_sd: float = 3000.0) -> Chunk:
    """SURVEY.md 8(d) config 2 generator (and configs 3-5 by changing the arguments)."""
    r_sites = np.random.default_rng([seed, 1])
    r_reads = np.random.default_rng([seed, 2])
    r_err = np.random.default_rng([seed, 3])
    r_prof = np.random.default_rng([seed, 4])
    pos = np.sort(r_sites.integers(0, region_bp, size=n_sites))
    A = r_sites.choice(np.asarray(allele_choices), size=n_sites, p=np.asarray(allele_probs)).astype(np.uint32)
    hap1 = (r_sites.random(n_sites) * A).astype(np.int64)
    shift = 1 + (r_sites.random(n_sites) * (A - 1)).astype(np.int64)
    hap2 = (hap1 + shift) % A
    off = np.zeros(n_sites + 1, dtype=np.int64)
    np.cumsum(A, out=off[1:])
    target = coverage * region_bp
    total, reads_raw, idx = 0.0, [], 0
    while total < target:
        if length_model == "lognormal":
            ln = float(np.exp(r_reads.normal(np.log(median_len), sigma)))
        else:
            ln = float(r_reads.normal(median_len, normal_sd))
        ln = int(min(max(ln, min_len), max_len))
        start_bp = int(r_reads.integers(-ln + 1, region_bp))
        strand = int(r_reads.random() < 0.5)
        hap = int(r_reads.random() < 0.5)
        lo, hi = max(start_bp, 0), min(start_bp + ln, region_bp)
        total += hi - lo
        s0, s1 = int(np.searchsorted(pos, lo, "left")), int(np.searchsorted(pos, hi, "left"))
        if s1 <= s0:
            continue
        truth = (hap1 if hap == 0 else hap2)[s0:s1]
        a_loc = A[s0:s1].astype(np.int64)
        wrong = r_err.random(s1 - s0) < allele_error
        alt = (truth + 1 + (r_err.random(s1 - s0) * (a_loc - 1)).astype(np.int64)) % a_loc
        observed = np.where(wrong, alt, truth)
        nb = int(off[s1] - off[s0])
        delta = np.abs(r_prof.normal(4.0, 2.0, size=nb))
        probs = np.minimum(255, np.rint(30.0 * delta)).astype(np.uint8)
        probs[(off[s0:s1] - off[s0]) + observed] = 0
        reads_raw.append((f"read_{idx:06d}", s0, s1 - s0, strand, hap, probs))
        idx += 1
    return _finish(A, reads_raw, hap1, hap2)


def make_unit_test_chunk(seed: int, ref_length: int, coverage: int, min_read: int, max_read: int,
                         error_rate: float, max_alleles: int = 9) -> Chunk:
    """Shape of tests/stRPHmmTest.c simulateReads (:106-160) with a fixed seed."""
    rng = np.random.default_rng([seed, 7])
    A = rng.integers(1, max_alleles + 1, size=ref_length).astype(np.uint32)
    hap1 = (rng.random(ref_length) * A).astype(np.int64)
    hap2 = (rng.random(ref_length) * A).astype(np.int64)
    off = np.zeros(ref_length + 1, dtype=np.int64)
    np.cumsum(A, out=off[1:])
    remaining, reads_raw, idx = coverage * ref_length, [], 0
    while remaining > 0:
        hap = int(rng.random() > 0.5)
        ln = int(rng.integers(min_read, max_read + 1))
        start = int(rng.integers(0, ref_length - ln + 1))
        truth = (hap1 if hap == 0 else hap2)[start:start + ln]
        a_loc = A[start:start + ln].astype(np.int64)
        err = rng.random(ln) < error_rate
        observed = np.where(err, (rng.random(ln) * a_loc).astype(np.int64), truth)
        nb = int(off[start + ln] - off[start])
        probs = np.full(nb, 100, dtype=np.uint8)
        probs[(off[start:start + ln] - off[start]) + observed] = 0
        reads_raw.append((f"read_{idx:06d}", start, ln, int(rng.random() < 0.5), hap, probs))
        idx += 1
        remaining -= ln
    return _finish(A, reads_raw, hap1, hap2)


def shipped_phase_params() -> dict:
    """params/base_params.json 'phase' block: the values every BASELINE config runs with."""
    return dict(maxNotSumTransitions=1, minPartitionsInAColumn=100, maxPartitionsInAColumn=100,
                minPosteriorProbabilityForPartition=0.0, maxCoverageDepth=64,
                minReadCoverageToSupportPhasingBetweenHeterozygousSites=2, includeInvertedPartitions=1,
                roundsOfIterativeRefinement=10, includeAncestorSubProb=1)


def unit_test_params(max_partitions: int = 50, max_not_sum: int = 0, min_cov: int = 0) -> dict:
    """tests/stRPHmmTest.c:91-104 getHmmParams (calloc'd, so every other field is 0)."""
    return dict(maxNotSumTransitions=max_not_sum, minPartitionsInAColumn=0, maxPartitionsInAColumn=max_partitions,
                minPosteriorProbabilityForPartition=0.0, maxCoverageDepth=64,
                minReadCoverageToSupportPhasingBetweenHeterozygousSites=min_cov, includeInvertedPartitions=1,
                roundsOfIterativeRefinement=0, includeAncestorSubProb=0)


# ---- read x allele alignment pairs (pair-HMM forward probability) ----

def random_sequence(rng, length: int, n_rate: float = 0.0) -> np.ndarray:
    """uint8 symbols 0..3 (ACGT), 4 = N with probability n_rate"""
    s = rng.integers(0, 4, size=length).astype(np.uint8)
    if n_rate > 0:
        s[rng.random(length) < n_rate] = 4
    return s


def evolve_sequence(rng, s: np.ndarray, sub: float = 0.05, ins: float = 0.03, dele: float = 0.03) -> np.ndarray:
    """substitutions, insertions and deletions at ONT-like rates (the role of evolveSequence in tests/pairwiseAlignerTest.c)"""
    out = []
    for c in s:
        r = rng.random()
        if r < dele:
            continue
        out.append(int(rng.integers(0, 4)) if r < dele + sub else int(c))
        while rng.random() < ins:
            out.append(int(rng.integers(0, 4)))
    return np.array(out, dtype=np.uint8)


def margin_phase_pair_hmm_arrays():
    """"hmmForwardStrandReadGivenReference" of the reference's params/base_params.json (type, transitions, emissions)"""
    transitions = [0.8, 0.1, 0.1, 0.5, 0.5, 0.0, 0.5, 0.0, 0.5]
    emissions = [0.969, 0.005, 0.017, 0.009, 0.008, 0.973, 0.007, 0.012, 0.021, 0.007, 0.967, 0.006, 0.008, 0.008, 0.004, 0.98,
                 1.0, 1.0, 1.0, 1.0, 0.25, 0.25, 0.25, 0.25]
    return 2, transitions, emissions


def make_bubble_strings(seed: int = 1, n_sites: int = 2000, coverage: int = 30, expansion: int = 12, allele_error=(0.05, 0.03, 0.03),
                        duplicate_rate: float = 0.0):
    """The strings margin phase aligns for one chunk of config 2: per het SNP site two alleles (the reference window of
    referenceExpansionForSmallVariants = 12 either side, the site substituted) and ~coverage read substrings, each a noisy
    copy of one allele, strand Bernoulli(0.5).  Returns a list of (alleles, reads, forward_strand) bubbles."""
    rng = np.random.default_rng(seed)
    bubbles = []
    for _ in range(n_sites):
        ref = random_sequence(rng, 2 * expansion + 1)
        alt = ref.copy()
        alt[expansion] = (alt[expansion] + 1 + rng.integers(0, 3)) % 4
        n = max(1, int(rng.poisson(coverage)))
        reads, strands = [], []
        for _k in range(n):
            if reads and rng.random() < duplicate_rate:
                reads.append(reads[int(rng.integers(0, len(reads)))].copy())
            else:
                reads.append(evolve_sequence(rng, ref if rng.random() < 0.5 else alt, *allele_error))
            strands.append(bool(rng.random() < 0.5))
        bubbles.append(([ref, alt], reads, strands))
    return bubbles


def pairs_from_bubbles(bubbles):
    """flatten bubbles into (pool, x_off, x_len, y_off, y_len, model_index): every allele x read pair, model 0 = forward strand"""
    strings, xo, xl, yo, yl, mi = [], [], [], [], [], []
    pos = 0
    for alleles, reads, fwd in bubbles:
        a_at = []
        for a in alleles:
            strings.append(a); a_at.append((pos, len(a))); pos += len(a)
        for r, f in zip(reads, fwd):
            strings.append(r)
            for (ao, al) in a_at:
                xo.append(ao); xl.append(al); yo.append(pos); yl.append(len(r)); mi.append(0 if f else 1)
            pos += len(r)
    pool = np.concatenate(strings) if strings else np.zeros(0, dtype=np.uint8)
    return (pool, np.array(xo, dtype=np.int64), np.array(xl, dtype=np.int32), np.array(yo, dtype=np.int64), np.array(yl, dtype=np.int32),
            np.array(mi, dtype=np.uint8))


# ---- chunks as the strings margin phase aligns (input of mrp_phase_string_chunks) ----

@dataclass
class StringChunk:
    """One chunk before the alignment: per bubble (alleles, reads, substrings) with alleles / substrings uint8 symbol arrays and
    reads the index of each substring's read; per read its name and strand.  hap / truth are for scoring only."""
    bubbles: list
    read_names: List[str]
    read_forward_strand: np.ndarray  # uint8 [n_reads]
    hap: np.ndarray                  # int [n_reads]: the haplotype each read was drawn from
    truth: List[int]                 # per bubble: the allele of haplotype 0


def _noisy_copy(rng, s: np.ndarray, sub: float, ins: float, dele: float) -> np.ndarray:
    """evolve_sequence's three error kinds in one vectorised pass (at most one inserted symbol after a position)"""
    n = len(s)
    r = rng.random(n)
    base = rng.integers(0, 4, size=2 * n).astype(np.uint8)
    out = np.where(r < dele + sub, base[:n], s).astype(np.uint8)
    ins_after = rng.random(n) < ins
    keep = r >= dele
    pieces = np.stack([out, base[n:]], axis=1).reshape(-1)
    mask = np.stack([keep, ins_after], axis=1).reshape(-1)
    return np.ascontiguousarray(pieces[mask], dtype=np.uint8)


def make_string_chunk(seed: int, n_sites: int = 130, coverage: int = 30, allele_len: int = 25, span=(4, 40), multi_allelic: float = 0.0,
                      duplicate_rate: float = 0.0, sv_sites: int = 0, sv_len: int = 600, orphan_reads: int = 0, empty_bubbles: int = 0,
                      error=(0.04, 0.02, 0.02), name_prefix: str = "read") -> StringChunk:
    """Spanning reads over consecutive het sites: each read carries one haplotype and one strand over a run of `span` sites and
    appears in every bubble of that run with a noisy copy of its haplotype's allele.  Options: a share of multi-allelic sites
    (3-4 alleles: every allele a substitution of the reference window at its own position), substrings copied verbatim from
    another read of the bubble (duplicate_rate), sv_sites bubbles whose second allele inserts sv_len symbols (longer than the
    shipped sv_threshold of 512: the pair-HMM anchors them), orphan_reads reads listed in no bubble, and empty_bubbles bubbles
    (placed at random) that list no substring.  Deterministic per seed."""
    rng = np.random.default_rng([seed, 11])
    n_reads = max(1, int(round(coverage * n_sites / ((span[0] + span[1]) / 2))))
    hap = rng.integers(0, 2, size=n_reads)
    strand = rng.integers(0, 2, size=n_reads).astype(np.uint8)
    spans = []
    for _ in range(n_reads):
        ln = int(rng.integers(span[0], span[1] + 1))
        a = int(rng.integers(-ln + 1, n_sites))
        spans.append((max(a, 0), min(a + ln, n_sites) - 1))
    empty = set(rng.choice(n_sites, size=min(empty_bubbles, n_sites), replace=False).tolist()) if empty_bubbles else set()
    sv = set(rng.choice(n_sites, size=min(sv_sites, n_sites), replace=False).tolist()) if sv_sites else set()
    bubbles, truth = [], []
    mid = allele_len // 2
    for i in range(n_sites):
        ref = random_sequence(rng, allele_len)
        if i in sv:
            alleles = [ref, np.concatenate([ref[:mid], random_sequence(rng, sv_len), ref[mid:]])]
        else:
            n_all = int(rng.integers(3, 5)) if rng.random() < multi_allelic else 2
            alleles = [ref]
            for k in range(1, n_all):
                alt = ref.copy()
                p = (mid + 2 * (k - 1)) % allele_len
                alt[p] = (alt[p] + k) % 4
                alleles.append(alt)
        t0 = int(rng.integers(0, len(alleles)))
        t1 = (t0 + 1 + int(rng.integers(0, len(alleles) - 1))) % len(alleles)
        truth.append(t0)
        reads, subs = [], []
        if i not in empty:
            for r in range(n_reads):
                a, b = spans[r]
                if not a <= i <= b:
                    continue
                if subs and rng.random() < duplicate_rate:
                    subs.append(subs[int(rng.integers(0, len(subs)))].copy())
                else:
                    subs.append(_noisy_copy(rng, alleles[t0 if hap[r] == 0 else t1], *error))
                reads.append(r)
        bubbles.append((alleles, reads, subs))
    names = [f"{name_prefix}_{seed}_{r:05d}" for r in range(n_reads + orphan_reads)]
    hap = np.concatenate([hap, rng.integers(0, 2, size=orphan_reads)]) if orphan_reads else hap
    strand = np.concatenate([strand, rng.integers(0, 2, size=orphan_reads).astype(np.uint8)]) if orphan_reads else strand
    if orphan_reads:  # the orphans take random positions among the reads
        perm = rng.permutation(len(names))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        bubbles = [(al, [int(inv[r]) for r in rs], sb) for al, rs, sb in bubbles]
        names = [names[int(p)] for p in perm]
        hap, strand = hap[perm], strand[perm]
    return StringChunk(bubbles=bubbles, read_names=names, read_forward_strand=np.ascontiguousarray(strand, dtype=np.uint8), hap=np.asarray(hap), truth=truth)


def split_filtered(full: StringChunk, seed: int, filtered_share: float = 0.5, variant_share: float = 0.1):
    """A chunk as margin phase sees it after downsampling (polish.maxDepth): a share of the reads of `full` become filtered reads,
    the others stay primary, and variant_share * n_bubbles filtered variants (three alleles, a heterozygous genotype along the two
    haplotypes, an entry per read of a random bubble) are added.  Returns (StringChunk of the primary reads, rest): rest a dict with
    forward_strand (per filtered read), fsubs (per bubble a list of (filtered read, symbols), ascending reads) and variants (a list
    of (alleles, (gt1, gt2), entries), entries (read, symbols) with filtered reads numbered behind the primary ones) -- what
    capi.string_chunk_rest_struct takes.  Deterministic per seed."""
    rng = np.random.default_rng([seed, 29])
    n = len(full.read_names)
    is_f = rng.random(n) < filtered_share
    idx = np.zeros(n, dtype=np.int64)
    idx[~is_f] = np.arange(int((~is_f).sum()))
    idx[is_f] = np.arange(int(is_f.sum()))
    n_primary = int((~is_f).sum())
    bubbles, fsubs = [], []
    for alleles, reads, subs in full.bubbles:
        bubbles.append((alleles, [int(idx[r]) for r in reads if not is_f[r]], [s for r, s in zip(reads, subs) if not is_f[r]]))
        fsubs.append(sorted(((int(idx[r]), s) for r, s in zip(reads, subs) if is_f[r]), key=lambda x: x[0]))
    primary = StringChunk(bubbles=bubbles, read_names=[nm for nm, f in zip(full.read_names, is_f) if not f],
                          read_forward_strand=np.ascontiguousarray(full.read_forward_strand[~is_f]), hap=full.hap[~is_f], truth=full.truth)
    variants = []
    with_reads = [b for b in range(len(full.bubbles)) if full.bubbles[b][1]]
    for _ in range(int(round(variant_share * len(full.bubbles))) if with_reads else 0):
        b = with_reads[int(rng.integers(0, len(with_reads)))]
        ref = random_sequence(rng, 25)
        alleles = [ref]
        for k in (1, 2):
            alt = ref.copy()
            alt[10 + 3 * k] = (alt[10 + 3 * k] + k) % 4
            alleles.append(alt)
        g = rng.choice(3, size=2, replace=False).tolist()
        entries = [(int(idx[r]) + (n_primary if is_f[r] else 0), _noisy_copy(rng, alleles[g[int(full.hap[r])]], 0.04, 0.02, 0.02)) for r in full.bubbles[b][1]]
        variants.append((alleles, (int(g[0]), int(g[1])), entries))
    return primary, dict(forward_strand=np.ascontiguousarray(full.read_forward_strand[is_f]), fsubs=fsubs, variants=variants)


# ---- alignments before the extraction of read substrings at variant sites ----

@dataclass
class AlignedChunk:
    """One chunk as htslib holds it (the fields of mrp_aligned_chunk): coordinates (0-based genome), the overlap slice of the
    reference, variants ascending by position with their alleles as strings (allele 0 = REF) and an SV flag, and reads as
    bam1_t fields: pos, flag, mapq, l_qseq, the CIGAR as BAM uint32 words and the sequence in bam_get_seq's 4-bit packing
    (both in CSR).  read_names / read_forward_strand are for the string chunk that follows."""
    overlap_start: int
    overlap_end: int
    chunk_start: int
    chunk_end: int
    reference: str
    variant_pos: np.ndarray   # int64
    alleles: list             # per variant: list of str
    is_sv: np.ndarray         # uint8
    read_pos: np.ndarray      # int64
    flag: np.ndarray          # uint16
    mapq: np.ndarray          # uint8
    l_qseq: np.ndarray        # int32
    cigar_first: np.ndarray   # int64 [n_reads + 1]
    cigar: np.ndarray         # uint32
    seq_first: np.ndarray     # int64 [n_reads + 1]
    seq: np.ndarray           # uint8
    read_names: List[str] = field(default_factory=list)

    @property
    def read_forward_strand(self) -> np.ndarray:
        return np.ascontiguousarray((self.flag & 0x10) == 0, dtype=np.uint8)


_NT16 = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN")}


def pack_seq(codes: Sequence[int]) -> np.ndarray:
    """4-bit codes (seq_nt16_table values) -> bam_get_seq's layout, high nibble first"""
    c = np.asarray(codes, dtype=np.uint8)
    if len(c) % 2:
        c = np.concatenate([c, np.zeros(1, np.uint8)])
    return np.ascontiguousarray((c[0::2] << 4) | c[1::2], dtype=np.uint8)


def _run_length(ops: Sequence[int]) -> List[int]:
    words, k = [], 0
    while k < len(ops):
        j = k
        while j < len(ops) and ops[j] == ops[k]:
            j += 1
        words.append(((j - k) << 4) | ops[k])
        k = j
    return words


def make_aligned_chunk(seed: int, overlap_bp: int = 12_000, margin_bp: int = 1_000, coverage: float = 12.0, read_len=(600, 4000),
                       variant_every: int = 150, sv_share: float = 0.08, sv_len=(60, 400), error=(0.04, 0.03, 0.03),
                       oddities: bool = True, genome_start: Optional[int] = None) -> AlignedChunk:
    """Haplotype reads aligned to a random reference, base by base: ONT-like substitutions, insertions and deletions, the
    het variants of the read's haplotype (SNPs, indels, multi-allelic sites, SV-flagged long insertions / deletions, some
    sites a few bases apart and some at the same position), soft and hard clips, M or =/X CIGARs, N ops, IUPAC and '='
    bases, windows deleted whole in some reads, reads crossing the chunk and overlap edges.  With oddities, also low-mapq,
    secondary, supplementary and unmapped records, a read without CIGAR and a secondary without sequence.  Deterministic
    per seed; the other generators' outputs are untouched (own generator stream)."""
    rng = np.random.default_rng([seed, 29])
    g0 = int(genome_start if genome_start is not None else 1_000_000 + 7_919 * (seed % 1000))
    pad = read_len[1] + 2 * sv_len[1]
    genome = "".join(rng.choice(list("ACGT"), size=overlap_bp + 2 * pad))  # genome[k] is position g0 - pad + k
    low = rng.random(len(genome)) < 0.05
    genome = "".join(c.lower() if m else c for c, m in zip(genome, low))
    genome = "".join("N" if rng.random() < 0.002 else c for c in genome)
    base = g0 - pad
    ovl_s, ovl_e = g0, g0 + overlap_bp
    ch_s, ch_e = ovl_s + margin_bp, ovl_e - margin_bp
    ref = genome[ovl_s - base:ovl_e - base]

    # variants (REF taken from the reference)
    vpos, valleles, vsv = [], [], []
    p = ovl_s + int(rng.integers(0, 20))
    while p < ovl_e - 2:
        r = rng.random()
        g = genome[p - base]
        if r < sv_share:
            ln = int(rng.integers(sv_len[0], sv_len[1] + 1))
            if rng.random() < 0.5:
                alleles = [g, g + "".join(rng.choice(list("ACGT"), size=ln))]
            else:
                ln = min(ln, ovl_e - p - 1)
                alleles = [genome[p - base:p - base + ln + 1], g]
            vsv.append(1)
        else:
            kind = rng.random()
            if kind < 0.55:
                alleles = [g, "ACGT"[("ACGT".find(g.upper()) + 1) % 4]]
            elif kind < 0.7:
                alleles = [g] + ["ACGT"[("ACGT".find(g.upper()) + k) % 4] for k in (1, 2)]
            elif kind < 0.85:
                alleles = [g, g + "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 6))))]
            else:
                ln = int(rng.integers(1, 6))
                alleles = [genome[p - base:p - base + ln + 1], g]
            vsv.append(0)
        vpos.append(p)
        valleles.append(alleles)
        q = rng.random()
        p += 0 if q < 0.03 else int(rng.integers(1, 8)) if q < 0.15 else int(rng.integers(variant_every // 2, 2 * variant_every))
    hap_alt = [[int(rng.integers(1, len(a))) if rng.random() < 0.85 else 0, 0] for a in valleles]  # hap 0 alt, hap 1 REF mostly
    for h in hap_alt:
        if rng.random() < 0.5:
            h.reverse()

    # reads
    n_reads = max(1, int(coverage * (overlap_bp + read_len[1]) / ((read_len[0] + read_len[1]) / 2)))
    pos_l, flag_l, mapq_l, lq_l, cig_l, seq_l, names = [], [], [], [], [], [], []
    var_at = {}
    for k, q in enumerate(vpos):
        var_at.setdefault(q, k)
    sub, ins, dele = error
    for r in range(n_reads):
        hap = int(rng.integers(0, 2))
        start = int(rng.integers(ovl_s - read_len[1], ovl_e))
        length = int(rng.integers(read_len[0], read_len[1] + 1))
        eq_style = rng.random() < 0.3
        ops, codes = [], []
        g = start
        wipe = rng.random() < 0.3
        while g < start + length and g - base < len(genome) - pad // 2:
            v = var_at.get(g)
            if v is not None and hap_alt[v][hap] != 0 and g > start:
                a_ref, a_alt = valleles[v][0], valleles[v][hap_alt[v][hap]]
                common = 0
                while common < min(len(a_ref), len(a_alt)) and a_ref[common].upper() == a_alt[common].upper():
                    common += 1
                for t in range(min(len(a_ref), len(a_alt))):
                    c = a_alt[t]
                    same = c.upper() == genome[g - base + t].upper()
                    ops.append((7 if same else 8) if eq_style else 0)
                    codes.append(_NT16[c.upper()])
                if len(a_alt) > len(a_ref):
                    ops += [1] * (len(a_alt) - len(a_ref))
                    codes += [_NT16[c.upper()] for c in a_alt[len(a_ref):]]
                elif len(a_ref) > len(a_alt):
                    ops += [2] * (len(a_ref) - len(a_alt))
                g += len(a_ref)
                continue
            if v is not None and wipe and rng.random() < 0.1 and g > start:  # a deletion over a whole small window
                ln = int(rng.integers(20, 40))
                ops += [3 if rng.random() < 0.3 else 2] * ln
                g += ln
                continue
            x = rng.random()
            if x < dele:
                ops.append(2)
                g += 1
                continue
            c = genome[g - base].upper()
            if x < dele + sub:
                c = "ACGT"[int(rng.integers(0, 4))]
            code = _NT16.get(c, 15)
            if rng.random() < 0.003:
                code = int(rng.choice([0, 3, 5, 6, 9, 15]))  # '=', M, R, S, W, N
            same = c == genome[g - base].upper() and code in (1, 2, 4, 8)
            ops.append((7 if same else 8) if eq_style else 0)
            codes.append(code)
            g += 1
            while rng.random() < ins:
                ops.append(1)
                codes.append([1, 2, 4, 8][int(rng.integers(0, 4))])
        if rng.random() < 0.05:  # an N run inside the read (spliced-looking)
            cut = int(rng.integers(1, max(2, len(ops) - 1)))
            if ops[cut - 1] not in (1,) and ops[cut] not in (1,):
                ops = ops[:cut] + [3] * int(rng.integers(5, 60)) + ops[cut:]
        while ops and ops[0] in (2, 3):  # an alignment starts and ends on a base
            ops.pop(0)
            start += 1
        while ops and ops[-1] in (2, 3):
            ops.pop()
        if not ops:
            continue
        words = _run_length(ops)
        lead = [1, 2, 4, 8]
        sc0 = int(rng.integers(1, 200)) if rng.random() < 0.4 else 0
        sc1 = int(rng.integers(1, 200)) if rng.random() < 0.4 else 0
        if sc0:
            words = [(sc0 << 4) | 4] + words
            codes = [lead[int(rng.integers(0, 4))] for _ in range(sc0)] + codes
        if sc1:
            words = words + [(sc1 << 4) | 4]
            codes = codes + [lead[int(rng.integers(0, 4))] for _ in range(sc1)]
        if rng.random() < 0.15:
            words = [(int(rng.integers(1, 500)) << 4) | 5] + words
        if rng.random() < 0.15:
            words = words + [(int(rng.integers(1, 500)) << 4) | 5]
        flag = 0x10 if rng.random() < 0.5 else 0
        mapq = 60 if rng.random() < 0.85 else int(rng.integers(0, 12))
        if oddities:
            o = rng.random()
            flag |= 0x100 if o < 0.04 else 0x800 if o < 0.08 else 0x4 if o < 0.1 else 0
        pos_l.append(start)
        flag_l.append(flag)
        mapq_l.append(mapq)
        lq_l.append(len(codes))
        cig_l.append(np.array(words, np.uint32))
        seq_l.append(pack_seq(codes))
        names.append(f"aln_{seed}_{r:05d}")
    if oddities:  # a mapped read without CIGAR, a secondary without sequence (SEQ '*')
        for w, lq in (([], 40), ([(40 << 4) | 0], 0)):
            pos_l.append(ch_s + int(rng.integers(0, 100)))
            flag_l.append(0 if lq else 0x100)
            mapq_l.append(60)
            lq_l.append(lq)
            cig_l.append(np.array(w, np.uint32))
            seq_l.append(pack_seq([1] * lq))
            names.append(f"aln_{seed}_odd{len(names)}")
    cf = np.zeros(len(cig_l) + 1, np.int64)
    np.cumsum([len(c) for c in cig_l], out=cf[1:])
    sf = np.zeros(len(seq_l) + 1, np.int64)
    np.cumsum([len(s) for s in seq_l], out=sf[1:])
    return AlignedChunk(overlap_start=ovl_s, overlap_end=ovl_e, chunk_start=ch_s, chunk_end=ch_e, reference=ref,
                        variant_pos=np.array(vpos, np.int64), alleles=valleles, is_sv=np.array(vsv, np.uint8),
                        read_pos=np.array(pos_l, np.int64), flag=np.array(flag_l, np.uint16), mapq=np.array(mapq_l, np.uint8),
                        l_qseq=np.array(lq_l, np.int32), cigar_first=cf,
                        cigar=np.concatenate(cig_l) if cig_l else np.zeros(0, np.uint32), seq_first=sf,
                        seq=np.concatenate(seq_l) if seq_l else np.zeros(0, np.uint8), read_names=names)
