"""What margin phase writes into the root VCF entries of a chunk, and how writePhasedVcf picks them up, restated in plain Python over
dicts and sets: updateOriginalVcfEntriesWithBubbleData (vcf.c:511-592), the update that ends
bubbleGraph_phaseVcfEntriesFromHaplotaggedReads (bubbleGraph.c:2298-2343) and updateHaplotypeSwitchingInVcfEntries (vcf.c:595-650).
TEST INFRASTRUCTURE ONLY: the definition the C functions mrp_variant_records_from_extracted and mrp_variants_from_records are held to.

A root entry is a dict: gt1, gt2, the three probabilities as LOG values (np.float32: the reference applies fromLog, vcf.c:560-562, a
monotone map the records leave to the caller; probability 0 is -inf), wasUpdated, state (UNTOUCHED / UPDATED / CLEARED: whether and how
the reference wrote to it), alleleIdxToReads (a set of the chunk's read indices per allele) and, beside the reference's sets, the two
lists hap1Reads / hap2Reads the sets were filled from (a homozygous call puts both into one set; the record keeps them apart).
Extractions are tests/extract_oracle.extract results: read_status, alleles, entries[v] = [(read, symbols)] in ascending read order."""
from __future__ import annotations

import numpy as np

from tests import extract_oracle as xo

UNTOUCHED, UPDATED, CLEARED = 0, 1, 2
NOT_VISITED, CIS, TRANS, TIE = 0, 1, 2, 3
NEG_INF = np.float32(-np.inf)


def root_entry(n_alleles: int, pos: int) -> dict:
    """a root VCF entry margin has not touched (gt -2 | -2 stands for "whatever the VCF said")"""
    return dict(pos=int(pos), gt1=-2, gt2=-2, genotypeProb=np.float32(0), haplotype1Prob=np.float32(0), haplotype2Prob=np.float32(0), wasUpdated=False,
                state=UNTOUCHED, alleleIdxToReads=[set() for _ in range(n_alleles)], hap1Reads=[], hap2Reads=[])


def is_primary(x, keep, r: int) -> bool:
    """a read of `reads` after the caller's downsampling (phase.c:360-382)"""
    return x["read_status"][r] == xo.KEPT and (keep is None or bool(keep[r]))


def update_with_bubble_data(x, keep, bubble_variant, gf, hap, variant_pos, chunk_start: int, chunk_end: int):
    """vcf.c:511-592.  gf: dict(ref_start, length, hap1, hap2, genotype_probs, hap_probs1, hap_probs2); hap[r] = 1 / 2 for a read in
    hap1Reads / hap2Reads (the phasing's own tags: the sets hold the chunk's BamChunkRead pointers, genomeFragment.c:237-238).
    -> the root entry of every variant of the chunk"""
    roots = [root_entry(len(x["alleles"][v]), variant_pos[v]) for v in range(len(x["alleles"]))]
    # :516 buildVcfEntryToBamChunkReadMap over bamChunkReads: the reads of the chunk that saved a substring for the entry
    entry_to_reads = [[r for r, _ in x["entries"][v] if is_primary(x, keep, r)] for v in range(len(x["alleles"]))]
    hap1_reads = {r for r in range(len(hap)) if hap[r] == 1}
    hap2_reads = {r for r in range(len(hap)) if hap[r] == 2}
    for i in range(int(gf["length"])):                               # :520
        b = int(gf["ref_start"]) + i                                 # :522
        hap1_allele, hap2_allele = int(gf["hap1"][i]), int(gf["hap2"][i])   # :523-524
        v = int(bubble_variant[b])                                   # :532-533
        root = roots[v]
        assert hap1_allele < len(root["alleleIdxToReads"]) and hap2_allele < len(root["alleleIdxToReads"])  # :537
        if root["pos"] < chunk_start or root["pos"] >= chunk_end:    # :538-540 not in chunk
            continue
        bcrs = entry_to_reads[v]                                     # :543
        if len(bcrs) == 0:                                           # :546-555 nothing to phase with (never for a bubble)
            root.update(gt1=-1, gt2=-1, genotypeProb=NEG_INF, haplotype1Prob=NEG_INF, haplotype2Prob=NEG_INF, state=CLEARED)
            continue
        root.update(gt1=hap1_allele, gt2=hap2_allele,                # :558-559
                    genotypeProb=np.float32(gf["genotype_probs"][i]),         # :560, before fromLog
                    haplotype1Prob=np.float32(gf["hap_probs1"][i]),           # :561
                    haplotype2Prob=np.float32(gf["hap_probs2"][i]),           # :562
                    wasUpdated=True, state=UPDATED)                  # :563
        for r in bcrs:                                               # :572-582
            if r in hap1_reads:                                      # :576
                root["alleleIdxToReads"][hap1_allele].add(r)
                root["hap1Reads"].append(r)
            elif r in hap2_reads:                                    # :578
                root["alleleIdxToReads"][hap2_allele].add(r)
                root["hap2Reads"].append(r)
    return roots


def update_filtered(x, xf, keep, hap, fvariant_pos, gt, variant_state, chunk_start: int, chunk_end: int):
    """the end of bubbleGraph_phaseVcfEntriesFromHaplotaggedReads, bubbleGraph.c:2298-2343, given each variant's cis / trans decision
    (variant_state); readNamesBelongingToHap1/2 are the primary reads the phasing tagged (phase.c:413).  -> the root entries"""
    roots = [root_entry(len(xf["alleles"][v]), fvariant_pos[v]) for v in range(len(xf["alleles"]))]
    for v, root in enumerate(roots):
        state = int(variant_state[v])
        assert state in (NOT_VISITED, CIS, TRANS, TIE)
        if state == NOT_VISITED:                                     # :2174 homozygous, :2179 outside the chunk, :2186-2192 no substrings
            continue
        computed_gt1, computed_gt2 = -1, -1                          # :2298-2299
        if state == CIS:                                             # :2303-2305
            computed_gt1, computed_gt2 = int(gt[v][0]), int(gt[v][1])
        elif state == TRANS:                                         # :2306-2309
            computed_gt1, computed_gt2 = int(gt[v][1]), int(gt[v][0])
        root.update(gt1=computed_gt1, gt2=computed_gt2, genotypeProb=NEG_INF, haplotype1Prob=NEG_INF, haplotype2Prob=NEG_INF)  # :2312-2316, probability 0
        if computed_gt1 == -1:                                       # :2317-2321
            root["state"] = CLEARED
            continue
        root.update(wasUpdated=True, state=UPDATED)                  # :2327
        # :2331-2343 over the variant's read substrings: the reads the second extraction kept (buildVcfEntryToReadSubstringsMap)
        substrings = [r for r, _ in xf["entries"][v] if xf["read_status"][r] == xo.KEPT] if chunk_start <= root["pos"] < chunk_end else []
        for r in substrings:
            tagged = is_primary(x, keep, r)                          # (only primary reads are in the two name sets)
            if tagged and hap[r] == 1:                               # :2337
                root["alleleIdxToReads"][computed_gt1].add(r)
                root["hap1Reads"].append(r)
            elif tagged and hap[r] == 2:                             # :2339
                root["alleleIdxToReads"][computed_gt2].add(r)
                root["hap2Reads"].append(r)
    return roots


def records_arrays(primary_roots, filtered_roots) -> dict:
    """the root entries of one chunk in mrp_variant_records' layout"""
    roots = list(primary_roots) + list(filtered_roots)
    first, reads = [0], []
    for e in roots:
        reads += sorted(e["hap1Reads"]) + sorted(e["hap2Reads"])
        first.append(len(reads))
    return dict(n_primary=len(primary_roots), n_filtered=len(filtered_roots), state=np.array([e["state"] for e in roots], np.uint8),
                gt=np.array([(e["gt1"], e["gt2"]) for e in roots], np.int32).reshape(len(roots), 2),
                genotype_log_prob=np.array([e["genotypeProb"] for e in roots], np.float32),
                hap1_log_prob=np.array([e["haplotype1Prob"] for e in roots], np.float32),
                hap2_log_prob=np.array([e["haplotype2Prob"] for e in roots], np.float32), read_first=np.array(first, np.int64),
                n_hap1=np.array([len(e["hap1Reads"]) for e in roots], np.int32), n_hap2=np.array([len(e["hap2Reads"]) for e in roots], np.int32),
                reads=np.array(reads, np.int32))


def assert_records_equal(got: dict, want: dict, where=""):
    """array for array; floats as bits"""
    assert (got["n_primary"], got["n_filtered"]) == (want["n_primary"], want["n_filtered"]), where
    for k in ("state", "gt", "read_first", "n_hap1", "n_hap2", "reads"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    for k in ("genotype_log_prob", "hap1_log_prob", "hap2_log_prob"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (where, k)


def switch_haplotypes(chunk_ranges, switched, roots):
    """updateHaplotypeSwitchingInVcfEntries, vcf.c:595-650: roots = the contig's root entries ordered by position"""
    idx = 0
    for (chunk_start, chunk_end), was_switched in zip(chunk_ranges, switched):
        while idx < len(roots) and roots[idx]["pos"] < chunk_start:   # :611 binarySearchVcfListForFirstIndexAtOrAfterRefPos, :622-628
            idx += 1
        while idx < len(roots) and roots[idx]["pos"] < chunk_end:     # :620-621
            e = roots[idx]
            if was_switched:                                          # :631-637
                e["gt1"], e["gt2"] = e["gt2"], e["gt1"]
                e["haplotype1Prob"], e["haplotype2Prob"] = e["haplotype2Prob"], e["haplotype1Prob"]
            idx += 1


def contig_variants(chunk_roots, chunk_ranges, switched, read_id):
    """chunk_roots[c] = (primary roots, filtered roots) of chunk c, in genome order.  A root entry belongs to the one chunk whose
    [chunk_start, chunk_end) holds its position (the others leave it untouched).  -> the variants writePhasedVcf considers
    (wasUpdated, vcf.c:863-868) in position order -- ties by chunk, primary before filtered, site -- as frame_oracle.phase_sets takes
    them, alleleIdxToReads as sets of the caller's read ids (readIdToIdx), each with chunk, site and the three log values"""
    roots = []
    for c, (prim, filt) in enumerate(chunk_roots):
        for s, e in enumerate(list(prim) + list(filt)):
            if e["state"] == UNTOUCHED:
                continue
            assert chunk_ranges[c][0] <= e["pos"] < chunk_ranges[c][1]
            g = dict(e, chunk=c, site=s, alleleIdxToReads=[{int(read_id[c][r]) for r in a} for a in e["alleleIdxToReads"]])
            roots.append(g)
    roots.sort(key=lambda e: (e["pos"], e["chunk"], e["site"]))
    switch_haplotypes(chunk_ranges, switched, roots)
    return [e for e in roots if e["wasUpdated"]]
