"""Hand-built alignments, one per rule of DESIGN.md section 9.3, each with the substrings the reference's walk saves for it
written out (read -> [(variant, first seq index, end seq index)], indices into the read's bases, soft clip included)."""
from __future__ import annotations

import numpy as np

from margin_amd import synth

REF = "ACGTTGCAAC" * 4                     # the overlap slice: genome 100..139
OPTS = dict(expansion_small=2, expansion_sv=6, min_mapq=5, include_secondary=0, include_supplementary=0)
OPS = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}


def cigar(text: str):
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num) << 4) | OPS[ch])
            num = ""
    return out


def qlen(words):
    return sum(w >> 4 for w in words if (w & 15) in (0, 1, 4, 7, 8))


def make(variants, reads, chunk_start=100, chunk_end=140):
    """variants: [(genome pos, alleles, is_sv)]; reads: [(pos, cigar text, mapq, flag)]; bases cycle A C G T"""
    cf, sf, cig, seq, pos, flag, mapq, lq = [0], [0], [], [], [], [], [], []
    for p, text, mq, fl in reads:
        w = cigar(text)
        n = qlen(w)
        packed = synth.pack_seq([(1, 2, 4, 8)[i % 4] for i in range(n)])
        cig += w
        seq.append(packed)
        cf.append(cf[-1] + len(w))
        sf.append(sf[-1] + len(packed))
        pos.append(p); flag.append(fl); mapq.append(mq); lq.append(n)
    return synth.AlignedChunk(overlap_start=100, overlap_end=140, chunk_start=chunk_start, chunk_end=chunk_end, reference=REF,
                              variant_pos=np.array([v[0] for v in variants], np.int64), alleles=[list(v[1]) for v in variants],
                              is_sv=np.array([v[2] for v in variants], np.uint8), read_pos=np.array(pos, np.int64),
                              flag=np.array(flag, np.uint16), mapq=np.array(mapq, np.uint8), l_qseq=np.array(lq, np.int32),
                              cigar_first=np.array(cf, np.int64), cigar=np.array(cig, np.uint32), seq_first=np.array(sf, np.int64),
                              seq=np.concatenate(seq) if seq else np.zeros(0, np.uint8),
                              read_names=[f"hand{k}" for k in range(len(reads))])


SNP110 = (110, [REF[10], "A" if REF[10] != "A" else "C"], 0)  # window [8, 13): refAlnStart 8, refAlnStopIncl 13


def cases():
    """-> list of (name, chunk, expected substrings per read, expected status per read)"""
    K, F, X = 1, 2, 0
    return [
        # 1. start: the step that reaches refAlnStart, so an insertion just before it is in; a read starting inside the
        #    window starts at its soft clip
        ("start", make([SNP110], [(100, "8M2I10M", 60, 0), (109, "3S10M", 60, 0)]),
         [[(0, 8, 15)], [(0, 3, 7)]], [K, K]),
        # 2. end: the base aligned to refAlnStopIncl and an insertion after the last included base are out; deletion
        #    steps start and end windows
        ("end", make([SNP110], [(100, "13M3I7M", 60, 0), (100, "9M6D8M", 60, 0), (100, "5M6D10M", 60, 0)]),
         [[(0, 8, 13)], [(0, 8, 9)], [(0, 5, 7)]], [K, K, K]),
        # 3. delayed start: the SV entry (window [15, 28)) starts only once the small one before it (window [18, 23)) has
        ("delayed", make([(120, [REF[20], "G"], 0), (121, [REF[21], "T"], 1)], [(100, "30M", 60, 0)]),
         [[(0, 18, 23), (1, 18, 28)]], [K]),
        # 4. dropped windows: deleted whole; open at the end of the read, kept (walk reached refPos 11) and dropped (9 < 11);
        #    a read starting on the window's last position without clip keeps its first base, with a clip it has none
        ("dropped", make([SNP110], [(100, "7M7D10M", 60, 0), (100, "11M", 60, 0), (100, "9M", 60, 0)]),
         [[], [(0, 8, 11)], []], [K, K, K]),
        ("slice_end", make([(139, [REF[39], "A"], 0)], [(139, "3M", 60, 0), (139, "1S3M", 60, 0)]),
         [[(0, 0, 1)], []], [K, K]),
        # 5. loop bound: alnReadLength leaves N out, so the walk stops after 15 reference steps (reaching rel 15):
        #    the entry at 114 (refPos 15) is kept open-ended, the one at 116 (refPos 17) dropped
        ("loop_bound", make([(114, [REF[14], "A"], 0), (116, [REF[16], "C"], 0)], [(100, "4M10N10M", 60, 0)]),
         [[(0, 4, 5)]], [K]),
        # ... and the chunk-span test uses the same length: 100 + 4 <= 105
        ("span", make([SNP110], [(100, "2M20N2M", 60, 0)], chunk_start=105), [[]], [X]),
        # 6. read lists: low mapq filtered (with its substring), nothing at or after the read not listed, listed without substring
        ("lists", make([SNP110], [(100, "20M", 3, 0), (111, "20M", 60, 0), (100, "9M", 60, 0)]),
         [[(0, 8, 13)], [], []], [F, X, K]),
    ]
