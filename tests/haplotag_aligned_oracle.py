"""tools/tagFromPhasedVcf.c's chunk loop restated in Python.  TEST INFRASTRUCTURE ONLY.

Per chunk (tools/tagFromPhasedVcf.c:284-309): updateVcfEntriesWithSubstringsAndPositions and
extractReadSubstringsAtVariantPositions with filteredReads = NULL (tests/extract_oracle.py; with a NULL list the
reference skips a low-mapq read at impl/htsIntegration.c:1825, so only the KEPT reads are in `reads`), then
bubbleGraph_partitionFilteredReadsFromPhasedVcfEntries (impl/bubbleGraph.c:1945-2138, tests/haptag_oracle.py) with
(gt1, gt2) of every phased VCF entry as the two compared alleles.

Also the site building of mrp_haptag_sites_from_extracted (include/margin_rphmm.h), array for array.
"""
from __future__ import annotations

import numpy as np

from tests import extract_oracle as eo
from tests import haptag_oracle as ho


def draw_genotypes(chunk, seed: int) -> np.ndarray:
    """phased genotypes of a synthetic chunk's variants, int32 [n_variants, 2]: mostly heterozygous, 15 % homozygous"""
    rng = np.random.default_rng([seed, 77])
    out = np.zeros((len(chunk.alleles), 2), np.int32)
    for v, al in enumerate(chunk.alleles):
        na = len(al)
        g1 = int(rng.integers(0, na))
        g2 = g1 if (na < 2 or rng.random() < 0.15) else (g1 + 1 + int(rng.integers(0, na - 1))) % na
        out[v] = (g1, g2)
    return out


def sites_from_extracted(xs, gts):
    """mrp_haptag_sites_from_extracted on eo.as_arrays dicts -> (dict of the mrp_haptag_sites arrays, read_first).
    Raises ValueError naming chunk and variant for a genotype outside the variant's alleles."""
    a_first, a_off, a_len, cmp_, e_first, e_read, e_off, e_len, pools = [0], [], [], [], [0], [], [], [], []
    read_first, base = [0], 0
    for c, (x, gt) in enumerate(zip(xs, gts)):
        nv = len(x["entry_first"]) - 1
        gt = np.zeros((0, 2), np.int32) if gt is None else np.asarray(gt).reshape(-1, 2)
        for v in range(nv):
            lo, hi = int(x["allele_first"][v]), int(x["allele_first"][v + 1])
            for g in gt[v]:
                if not 0 <= int(g) < hi - lo:
                    raise ValueError(f"chunk {c}, variant {v}: genotype {int(g)} outside its {hi - lo} alleles")
            for a in range(lo, hi):
                a_off.append(base + int(x["allele_off"][a]))
                a_len.append(int(x["allele_len"][a]))
            cmp_ += [int(gt[v][0]), int(gt[v][1])]
            for e in range(int(x["entry_first"][v]), int(x["entry_first"][v + 1])):
                r = int(x["entry_read"][e])
                if x["read_status"][r] != eo.KEPT:            # filteredReads == NULL: htsIntegration.c:1825
                    continue
                e_read.append(read_first[c] + r)
                e_off.append(base + int(x["entry_off"][e]))
                e_len.append(int(x["entry_len"][e]))
            a_first.append(len(a_off))
            e_first.append(len(e_read))
        pools.append(np.asarray(x["pool"], np.uint8))
        base += len(x["pool"])
        read_first.append(read_first[c] + len(x["read_status"]))
    out = dict(allele_first=np.array(a_first, np.int64), allele_off=np.array(a_off, np.int64), allele_len=np.array(a_len, np.int32),
               compare=np.array(cmp_, np.int32), entry_first=np.array(e_first, np.int64), entry_read=np.array(e_read, np.int64),
               entry_off=np.array(e_off, np.int64), entry_len=np.array(e_len, np.int32),
               pool=np.concatenate(pools).astype(np.uint8) if pools else np.zeros(0, np.uint8), n_sites=len(cmp_) // 2)
    return out, np.array(read_first, np.int64)


def chunk_sites(x, gt):
    """one chunk of eo.extract() -> the sites haptag_oracle takes: (alleles, (gt1, gt2), entries of KEPT reads in read order)"""
    gt = np.asarray(gt).reshape(-1, 2)
    return [(list(x["alleles"][v]), (int(gt[v][0]), int(gt[v][1])), [(r, s) for r, s in ents if x["read_status"][r] == eo.KEPT])
            for v, ents in enumerate(x["entries"])]


def facts(sites, strand) -> dict:
    """what an input exercises at its heterozygous sites: entries that copy an owner's scores, and such pairs on opposite strands"""
    dup = mixed = 0
    for _, (i, j), ents in sites:
        if i == j:
            continue
        dup += len(ents) - len({bytes(s) for _, s in ents})
        mixed += sum(1 for k, (a, s) in enumerate(ents) for b, t in ents[k + 1:] if bytes(s) == bytes(t) and strand[a] != strand[b])
    return dict(duplicates=dup, mixed_strand=mixed)


def haplotag(chunks, gts, opts, fwd, rev, expansion: int = 4):
    """the chunk loop -> per chunk dict(hap int8 [n_reads]: 1, 2, 0 (in `reads`, unclassified) or -1 (not in `reads`), h1, h2
    float64 (0 for reads not in `reads`), extracted (eo.extract's dict), sites, facts)"""
    out = []
    for ch, gt, x in zip(chunks, gts, eo.extract(chunks, opts)):
        n = len(ch.read_pos)
        strand = ch.read_forward_strand                              # bam_is_rev(aln): flag 0x10
        sites = chunk_sites(x, gt)
        hap, h1, h2 = ho.partition_filtered_reads_from_phased_vcf(fwd, rev, sites, n, strand, expansion)
        kept = x["read_status"] == eo.KEPT
        assert (h1[~kept] == 0).all() and (h2[~kept] == 0).all()
        low = sum(1 for ents in x["entries"] for r, _ in ents if x["read_status"][r] == eo.FILTERED)
        out.append(dict(hap=np.where(kept, hap, -1).astype(np.int8), h1=h1, h2=h2, extracted=x, sites=sites,
                        facts=dict(facts(sites, strand), low_mapq_entries=low)))
    return out
