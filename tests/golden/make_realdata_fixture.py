"""Write tests/golden/realdata_extract.npz: one window of margin's real-data test set (HG002 ONT reads on chr20:59M+100k,
tests/data/realData in the margin repository) for the extraction of read substrings at variant sites.

Usage: python tests/golden/make_realdata_fixture.py <margin tests/data/realData directory>

Only the standard library and numpy: BGZF is multi-member gzip, and a BAM record is read with struct.  Kept: every read
whose alignment overlaps the window (full alignment: CIGAR and packed bases as bam1_t holds them), the VCF records inside
the window (alleles of REF and ALT) and the reference slice of the window.
"""
import gzip
import os
import struct
import sys

import numpy as np

OVERLAP = (75_000, 80_000)   # chunkOverlapStart / End (0-based, the contig of the test set)
CHUNK = (75_500, 79_500)     # chunkStart / End
REF_SPAN_OPS = (0, 2, 3, 7, 8)


def read_bam(path):
    data = gzip.open(path, "rb").read()
    assert data[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", data, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", data, at)[0]
    at += 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", data, at)[0]
        at += 4 + l_name + 4
    while at < len(data):
        block = struct.unpack_from("<i", data, at)[0]
        rec = data[at + 4:at + 4 + block]
        at += 4 + block
        ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 0)
        o = 32
        name = rec[o:o + l_name - 1].decode()
        o += l_name
        cigar = np.frombuffer(rec, np.uint32, n_cig, o).copy()
        o += 4 * n_cig
        seq = np.frombuffer(rec, np.uint8, (l_seq + 1) // 2, o).copy()
        if n_cig == 2 and (cigar[0] & 15) == 4 and (cigar[1] & 15) == 3:
            raise SystemExit(f"{name}: CIGAR in the CG tag (more than 65535 ops) is not handled")
        yield dict(name=name, pos=pos, mapq=mapq, flag=flag, l_qseq=l_seq, cigar=cigar, seq=seq)


def main(src):
    ref = "".join(l.strip() for l in open(os.path.join(src, "hg38.chr20_59M_100k.fa")) if not l.startswith(">"))
    reads = []
    for r in read_bam(os.path.join(src, "HG002.r94g360.chr20_59M_100k.bam")):
        span = int(sum(int(c) >> 4 for c in r["cigar"] if int(c) & 15 in REF_SPAN_OPS))
        if r["pos"] < OVERLAP[1] and r["pos"] + max(span, 1) > OVERLAP[0]:
            reads.append(r)
    vpos, alleles = [], []
    for line in open(os.path.join(src, "HG002.r94g360.chr20_59M_100k.vcf")):
        if line.startswith("#"):
            continue
        f = line.split("\t")
        p = int(f[1]) - 1
        if OVERLAP[0] <= p < OVERLAP[1]:
            vpos.append(p)
            alleles.append(",".join([f[3]] + f[4].split(",")))
    cf = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r["cigar"]) for r in reads], out=cf[1:])
    sf = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r["seq"]) for r in reads], out=sf[1:])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "realdata_extract.npz")
    np.savez_compressed(out, coords=np.array([*OVERLAP, *CHUNK], np.int64), reference=np.array(ref[OVERLAP[0]:OVERLAP[1]]),
                        variant_pos=np.array(vpos, np.int64), alleles=np.array(alleles), is_sv=np.zeros(len(vpos), np.uint8),
                        read_pos=np.array([r["pos"] for r in reads], np.int64), flag=np.array([r["flag"] for r in reads], np.uint16),
                        mapq=np.array([r["mapq"] for r in reads], np.uint8), l_qseq=np.array([r["l_qseq"] for r in reads], np.int32),
                        cigar_first=cf, cigar=np.concatenate([r["cigar"] for r in reads]), seq_first=sf,
                        seq=np.concatenate([r["seq"] for r in reads]), read_names=np.array([r["name"] for r in reads]))
    print(f"{out}: {len(reads)} reads, {int(sf[-1]) * 2} bases, {int(cf[-1])} CIGAR ops, {len(vpos)} variants, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
