"""The reference's extraction of read substrings at variant sites, restated in Python.  TEST INFRASTRUCTURE ONLY.

Restates, on the inputs mrp_extract_read_substrings takes (include/margin_rphmm.h, mrp_aligned_chunk):

* getAlleleSubstrings2 (impl/vcf.c:394-462) as updateVcfEntriesWithSubstringsAndPositions (:476-486) calls it:
  each VCF entry's allele strings with reference context and its window refAlnStart / refAlnStopIncl;
* binarySearchVcfListForFirstIndexAtOrAfterRefPos (impl/vcf.c:238-258);
* getAlignedReadLength3 with boundaryAtMatch = FALSE (impl/htsIntegration.c:37-111) and countIndels (:113-120);
* extractReadSubstringsAtVariantPositions2 (impl/htsIntegration.c:1758-1989) with saveStartingVcfEntries (:1589-1607)
  and saveFinishedVcfEntries (:1610-1680): the walk goes one CIGAR step at a time, exactly as the reference's does;
* bubbleGraph_constructFromVCFAndBamChunkReadVcfEntrySubstrings (impl/bubbleGraph.c:1338-1400) over
  buildVcfEntryToReadSubstringsMap (:1281-1323): the bubbles margin phase builds from the kept reads.

A chunk is a margin_amd.synth.AlignedChunk (or any object with the same fields).  Symbols are those of
mrp_symbols_from_chars: A/C/G/T (either case) -> 0..3, everything else -> 4.
"""
from __future__ import annotations

import numpy as np

DROPPED, KEPT, FILTERED = 0, 1, 2  # MRP_READ_*
M, I, D, N, S, H, P, EQ, X = range(9)  # BAM_CIGAR ops
SEQ_NT16 = "=ACMGRSVTWYHKDBN"  # htslib seq_nt16_str


def symbols(chars) -> np.ndarray:
    lut = np.full(256, 4, np.uint8)
    for k, c in enumerate("ACGT"):
        lut[ord(c)] = lut[ord(c.lower())] = k
    b = np.frombuffer(chars.encode() if isinstance(chars, str) else bytes(chars), np.uint8)
    return lut[b]


def seqi(packed: np.ndarray, i: int) -> int:
    """bam_seqi: high nibble first"""
    return (int(packed[i >> 1]) >> ((~i & 1) << 2)) & 0xF


def allele_substrings(ref: str, rel: int, alleles, expansion: int):
    """getAlleleSubstrings2 (vcf.c:394-462) with putRefPosInPOASpace = FALSE: pos = refPos - 1 = rel (0-based in the overlap
    slice) -> (allele strings, refAlnStart, refAlnStopIncl); raises ValueError where the reference asserts (:423)"""
    n = len(ref)
    ref_allele = alleles[0]
    ref_len = len(ref_allele)
    for i in range(len(ref_allele)):                          # :416-424 a REF past the slice stops at its end
        if rel + i >= n:
            ref_len = i
            break
        rc, ac = ref[rel + i].upper(), ref_allele[i].upper()
        if not (rc == ac or rc not in "ACGT"):
            raise ValueError(f"REF allele disagrees with the reference at {rel + i}")
    p_start = rel - expansion                                 # :428-435
    s_start = rel + ref_len
    s_len = n - s_start if s_start + expansion >= n else expansion
    if s_start >= n:
        s_start, s_len = n - 1, 0
    aln_start = 0 if p_start < 0 else p_start
    aln_stop = n - 1 if s_start + expansion >= n else s_start + expansion
    prefix = ref[aln_start:aln_start + (rel if p_start < 0 else expansion)]  # :439-440 stString_getSubString
    suffix = ref[s_start:s_start + s_len]
    return [prefix + a + suffix for a in alleles], aln_start, aln_stop


def variant_windows(chunk, opts):
    """updateVcfEntriesWithSubstringsAndPositions (vcf.c:476-486) -> per variant dict(ref_pos (1-based, chunk relative),
    aln_start, aln_stop, alleles (uint8 symbol arrays))"""
    out = []
    for v in range(len(chunk.variant_pos)):
        rel = int(chunk.variant_pos[v]) - chunk.overlap_start
        e = opts["expansion_sv"] if chunk.is_sv[v] else opts["expansion_small"]
        strings, a, b = allele_substrings(chunk.reference, rel, chunk.alleles[v], e)
        out.append(dict(ref_pos=rel + 1, aln_start=a, aln_stop=b, alleles=[symbols(s) for s in strings]))
    return out


def first_index_at_or_after(ref_pos, want: int) -> int:
    """binarySearchVcfListForFirstIndexAtOrAfterRefPos (vcf.c:238-258), recursion included"""
    n = len(ref_pos)
    if n == 0 or ref_pos[n - 1] < want:
        return -1
    if ref_pos[0] >= want:
        return 0

    def rec(start, end_incl):
        if end_incl - start == 1:
            return start if ref_pos[start] >= want else end_incl
        mid = start + (end_incl - start) // 2
        return rec(mid, end_incl) if ref_pos[mid] < want else rec(start, mid)
    return rec(0, n - 1)


def aligned_read_length(cigar, l_qseq: int):
    """getAlignedReadLength3(boundaryAtMatch = FALSE) (htsIntegration.c:37-111) -> (alnReadLength, start soft clip)"""
    start_clip = end_clip = 0
    k = 0
    while k < len(cigar):                                     # :52-73 stop at the first M, =, X, D, N or I
        op, ln = cigar[k] & 0xF, cigar[k] >> 4
        if op in (M, EQ, X, D, N, I):
            break
        if op == S:
            start_clip += ln
        k += 1
    k = len(cigar) - 1
    while k > 0:                                              # :76-97 never looks at the first op
        op, ln = cigar[k] & 0xF, cigar[k] >> 4
        if op in (M, EQ, X, D, N, I):
            break
        if op == S:
            end_clip += ln
        k -= 1
    ins = sum(c >> 4 for c in cigar if c & 0xF == I)          # countIndels :113-120: N is not a deletion
    dels = sum(c >> 4 for c in cigar if c & 0xF == D)
    return l_qseq - start_clip - end_clip + dels - ins, start_clip


def extract_chunk(chunk, opts):
    """extractReadSubstringsAtVariantPositions2 for one chunk -> dict(variants (variant_windows), status [n_reads],
    subs: per read the list of (variant, seq start, seq end) in the order the reference saves them)"""
    vw = variant_windows(chunk, opts)
    ref_pos = [w["ref_pos"] for w in vw]
    ovl = chunk.overlap_start
    n_reads = len(chunk.read_pos)
    status = np.zeros(n_reads, np.uint8)
    subs = [[] for _ in range(n_reads)]
    for r in range(n_reads):
        cigar = [int(c) for c in chunk.cigar[chunk.cigar_first[r]:chunk.cigar_first[r + 1]]]
        l_qseq, flag, pos = int(chunk.l_qseq[r]), int(chunk.flag[r]), int(chunk.read_pos[r])
        if l_qseq <= 0 or not cigar or flag & 0x4:            # :1816-1819
            continue
        if not opts["include_secondary"] and flag & 0x100:
            continue
        if not opts["include_supplementary"] and flag & 0x800:
            continue
        filtered = int(chunk.mapq[r]) < opts["min_mapq"]      # :1825-1828 filteredReads is never NULL in phase.c
        aln_len, clip = aligned_read_length(cigar, l_qseq)
        if aln_len <= 0:
            continue
        if pos >= chunk.chunk_end or pos + aln_len <= chunk.chunk_start:  # :1840-1842
            continue
        nxt = first_index_at_or_after(ref_pos, pos - ovl + 1)  # :1852-1855
        if nxt == -1:
            continue
        current = {}                                          # currentVcfEntries: entry -> seq start
        saved = subs[r]

        def save_starting(ref_here, seq_here):                # :1589-1607 only the next entry in list order
            nonlocal nxt
            while nxt < len(vw) and vw[nxt]["aln_start"] <= ref_here - ovl:
                current[nxt] = seq_here + clip
                nxt += 1

        def save_finished(rel_ref, seq_here, end_of_read):    # :1610-1680
            for v in sorted(current):
                if end_of_read or vw[v]["aln_stop"] <= rel_ref:
                    start, end = current[v], seq_here + clip
                    if not (end - start == 0 or (end_of_read and rel_ref < vw[v]["ref_pos"])):
                        saved.append((v, start, end))
                    del current[v]

        seq_i, ref_i = 0, pos
        k, in_op, op, ln = 0, 0, -1, -1
        if clip == 0:                                         # :1895-1899
            save_starting(ref_i, seq_i)
        i = 0
        while i <= aln_len:                                   # :1901 the loop bound ignores N ops
            if k == len(cigar):
                break
            if in_op == 0:
                op, ln = cigar[k] & 0xF, cigar[k] >> 4
            if op in (M, EQ, X):
                seq_i += 1
                ref_i += 1
            elif op in (D, N):
                ref_i += 1
            elif op == I:
                seq_i += 1
                i -= 1
            else:                                             # S, H, P: the whole op in one step
                in_op = ln - 1
                i -= 1
            save_starting(ref_i, seq_i)
            save_finished(ref_i - ovl, seq_i, False)
            in_op += 1
            if in_op == ln:
                k += 1
                in_op = 0
            i += 1
        save_finished(ref_i - ovl, seq_i, True)               # :1961-1962
        status[r] = FILTERED if filtered else KEPT
    return dict(variants=vw, status=status, subs=subs)


def substring_symbols(chunk, r: int, a: int, b: int) -> np.ndarray:
    packed = chunk.seq[chunk.seq_first[r]:chunk.seq_first[r + 1]]
    return symbols("".join(SEQ_NT16[seqi(packed, i)] for i in range(a, b)))


def extract(chunks, opts):
    """-> per chunk the arrays mrp_extracted_chunk holds: ref_aln_start, ref_aln_stop_incl, allele lists, read_status,
    read_n_substrings, per variant entry lists [(read, symbols)] in ascending read order"""
    out = []
    for ch in chunks:
        x = extract_chunk(ch, opts)
        nv = len(x["variants"])
        entries = [[] for _ in range(nv)]
        for r, lst in enumerate(x["subs"]):
            for v, a, b in lst:
                entries[v].append((r, substring_symbols(ch, r, a, b)))
        out.append(dict(ref_aln_start=np.array([w["aln_start"] for w in x["variants"]], np.int64),
                        ref_aln_stop_incl=np.array([w["aln_stop"] for w in x["variants"]], np.int64),
                        alleles=[w["alleles"] for w in x["variants"]], read_status=x["status"],
                        read_n_substrings=np.array([len(s) for s in x["subs"]], np.int32), entries=entries))
    return out


def bubbles_from_extracted(x, keep=None):
    """bubbleGraph_constructFromVCFAndBamChunkReadVcfEntrySubstrings (bubbleGraph.c:1338-1400) over the kept reads (and
    keep[r], the caller's downsampling) -> (bubbles [(alleles, reads, substrings)], bubble -> variant)"""
    bubbles, variant_of = [], []
    for v, ents in enumerate(x["entries"]):
        ents = [(r, s) for r, s in ents if x["read_status"][r] == KEPT and (keep is None or keep[r])]
        if not ents:                                          # :1366-1371 nothing to phase with
            continue
        ents = ents[::-1]                                     # :1391-1393 b->reads filled by stList_pop
        bubbles.append((list(x["alleles"][v]), [r for r, _ in ents], [s for _, s in ents]))
        variant_of.append(v)
    return bubbles, variant_of


def as_arrays(x) -> dict:
    """one chunk of extract() in mrp_extracted_chunk's layout (alleles then substrings in one pool, entry CSR by variant)"""
    a_first, a_off, a_len, e_first, e_read, e_off, e_len, parts, at = [0], [], [], [0], [], [], [], [], 0
    for al in x["alleles"]:
        for a in al:
            a_off.append(at); a_len.append(len(a)); parts.append(a); at += len(a)
        a_first.append(len(a_off))
    for ents in x["entries"]:
        for r, s in ents:
            e_read.append(r); e_off.append(at); e_len.append(len(s)); parts.append(s); at += len(s)
        e_first.append(len(e_read))
    return dict(ref_aln_start=x["ref_aln_start"], ref_aln_stop_incl=x["ref_aln_stop_incl"], allele_first=np.array(a_first, np.int64),
                allele_off=np.array(a_off, np.int64), allele_len=np.array(a_len, np.int32), read_status=np.asarray(x["read_status"], np.uint8),
                read_n_substrings=np.asarray(x["read_n_substrings"], np.int32), entry_first=np.array(e_first, np.int64),
                entry_read=np.array(e_read, np.int32), entry_off=np.array(e_off, np.int64), entry_len=np.array(e_len, np.int32),
                pool=np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8))
