"""mrp_haplotag_aligned_chunks on the device: against tools/tagFromPhasedVcf.c's chunk loop restated in Python
(tests/haplotag_aligned_oracle.py), bit for bit against the chain mrp_extract_read_substrings ->
mrp_haptag_sites_from_extracted -> mrp_partition_reads_by_haplotype, the owner rule at its edges on a hand-built site
with more entries than a wave has lanes, degenerate inputs, repeat calls and host-thread counts.

Tolerance of the totals against the oracle: 1e-9 * max(1, |oracle|), as tests/test_gpu_haptag.py (device log / exp are not
glibc's; the pair-HMM values themselves are bit-identical).  Against the chain nothing may differ: the same kernels run
over the same pairs."""
import numpy as np
import pytest

from margin_amd import capi, synth
from oracle import pairhmm as ph
from tests import extract_cases as ec
from tests import extract_oracle as eo
from tests import haplotag_aligned_oracle as hao
from tests import haptag_oracle as ho
from tests.test_gpu_extract import OPTION_SETS

pytestmark = pytest.mark.gpu


def models():
    f = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    r = f.reverse_complement()
    return f, r, ph.Model.from_buffer_copy(bytes(f)), ph.Model.from_buffer_copy(bytes(r))


def close(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return bool((np.abs(got - ref) <= 1e-9 * np.maximum(1.0, np.abs(ref))).all())


@pytest.fixture(scope="module")
def synthetic():
    chunks = [synth.make_aligned_chunk(seed, overlap_bp=8_000, coverage=8.0) for seed in range(6)]
    return chunks, [hao.draw_genotypes(c, seed) for seed, c in enumerate(chunks)]


def chain(ctx, chunks, gts, opts, f, r):
    """the three calls the composite joins -> per chunk dict(hap int8 with -1 for reads that are not kept, h1, h2)"""
    got, _ = capi.extract_read_substrings(ctx, chunks, opts)
    sites, first = capi.haptag_sites_from_extracted(got, gts)
    n = int(first[-1])
    strand = np.concatenate([c.read_forward_strand for c in chunks]) if chunks else np.zeros(0, np.uint8)
    hap, h1, h2, _ = capi.partition_reads_from_site_arrays(ctx, f, r, sites, n, strand)
    out = []
    for c, g in enumerate(got):
        a, b = int(first[c]), int(first[c + 1])
        out.append(dict(hap=np.where(g["read_status"] == capi.READ_KEPT, hap[a:b], -1).astype(np.int8), h1=h1[a:b], h2=h2[a:b]))
    return out


def assert_identical(got, want, where=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["hap"].dtype == np.int8 and np.array_equal(g["hap"], w["hap"]), f"{where} chunk {i} hap"
        for k in ("h1", "h2"):
            assert np.array_equal(g[k].view(np.uint64), w[k].view(np.uint64)), f"{where} chunk {i} {k}"


def assert_matches_oracle(got, want, where=""):
    for i, (g, w) in enumerate(zip(got, want)):
        ho.assert_margins_decisive(w["h1"], w["h2"], f"{where} chunk {i}")
        assert np.array_equal(g["hap"], w["hap"]), f"{where} chunk {i} hap"
        assert close(g["h1"], w["h1"]) and close(g["h2"], w["h2"]), f"{where} chunk {i} totals"


def test_oracle_parity(gpu_ctx, synthetic):
    f, r, of, orv = models()
    seeds = (1, 2, 4)
    chunks, gts = [synthetic[0][s] for s in seeds], [synthetic[1][s] for s in seeds]
    opts = capi.shipped_extract_options()
    want = hao.haplotag(chunks, gts, opts, of, orv)
    got, st = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r, opts)
    assert_matches_oracle(got, want)
    # what the input exercises
    for w in want:
        assert w["facts"]["duplicates"] > 0 and w["facts"]["mixed_strand"] > 0 and w["facts"]["low_mapq_entries"] > 0
        assert (w["hap"] == -1).any() and (w["hap"] == 1).any() and (w["hap"] == 2).any()
    assert st.pairhmm.pairs_lane > 0 and st.pairhmm.pairs_wave > 0
    het = [[s for s in w["sites"] if s[1][0] != s[1][1] and s[2]] for w in want]
    assert st.sites == sum(len(c.alleles) for c in chunks) and st.active_sites == sum(len(h) for h in het)
    assert st.entries == sum(len(s[2]) for h in het for s in h)
    assert st.owners == sum(len({bytes(x) for _, x in s[2]}) for h in het for s in h)
    assert st.pairhmm.pairs_lane + st.pairhmm.pairs_wave == 2 * st.owners
    assert st.extract.entries == sum(len(e) for w in want for e in w["extracted"]["entries"])
    # what comes back: the extraction's one total (16 B), the entry CSR, per entry its length (8 B), read and owner (4 B each), per
    # read its status and its three results (1 + 4 + 8 + 8 B) -- and not the substrings' symbols
    n_reads, n_ent = sum(len(c.read_pos) for c in chunks), st.extract.entries
    n_bases = sum(len(s) for w in want for e in w["extracted"]["entries"] for _, s in e)
    assert st.bytes_downloaded == 16 + 8 * (st.sites + 1) + 16 * n_ent + 21 * n_reads and n_bases > 16 * n_ent
    assert st.total_ms > 0 and st.owners_ms > 0 and st.pairhmm.kernel_ms > 0 and st.extract.kernel_ms > 0


@pytest.mark.parametrize("k", range(len(OPTION_SETS)))
def test_composite_equals_the_chain(gpu_ctx, synthetic, k):
    f, r, _, _ = models()
    chunks, gts = synthetic[0] * 3, synthetic[1] * 3
    got, st = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r, OPTION_SETS[k])
    assert_identical(got, chain(gpu_ctx, chunks, gts, OPTION_SETS[k], f, r), f"options {k}")
    assert st.owners > 0 and st.entries > st.owners
    # six calls of one chunk give what one call of six gives
    for c in range(6):
        one, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks[c:c + 1], gts[c:c + 1], f, r, OPTION_SETS[k])
        assert_identical(one, got[c:c + 1], f"options {k}, chunk {c} alone")
        assert_identical(got[6 + c:7 + c], got[c:c + 1], f"options {k}, chunk {c} again")


def owner_rule_chunk():
    """One SNP site (window of 5 reference bases) with 75 entries.  Reads 0..69 are the same alignment on alternating strands
    (read 0 forward), so their substrings are equal; read 69, on the reverse strand, has low mapq: it takes no part, the owner
    is read 68 and its forward strand decides.  Then reads with other substrings: 70 (forward) and 71 (reverse) start one base
    later -- same length, other symbols, owner 71 --, 72 has an insertion inside the window -- longer, with the 70 reads'
    substring as its prefix --, 73 a deletion -- shorter, a prefix of it --, and 74 is a low-mapq copy of 70."""
    reads = [(100, "20M", 3 if i == 69 else 60, 0x10 if i % 2 else 0) for i in range(70)]
    reads += [(101, "19M", 60, 0), (101, "19M", 60, 0x10), (100, "10M2I8M", 60, 0), (100, "11M1D8M", 60, 0x10), (101, "19M", 2, 0)]
    # the reads' bases cycle A C G T from their first base: 20M reads carry ACGTA over the window; REF there is ACACG
    alleles = [ec.REF[10], "G"]
    return ec.make([(110, alleles, 0)], reads), np.array([[1, 0]], np.int32)


def test_owner_rule_at_the_edges(gpu_ctx):
    f, r, of, orv = models()
    chunk, gt = owner_rule_chunk()
    want = hao.haplotag([chunk], [gt], ec.OPTS, of, orv)
    ents = want[0]["extracted"]["entries"][0]
    subs = {rd: bytes(s) for rd, s in ents}
    assert len(ents) == 75 and len({subs[i] for i in range(70)}) == 1                       # more entries than a wave has lanes
    assert len(subs[70]) == len(subs[0]) and subs[70] != subs[0] and subs[71] == subs[70] == subs[74]
    assert len(subs[72]) > len(subs[0]) and subs[72].startswith(subs[0]) and len(subs[73]) < len(subs[0]) and subs[0].startswith(subs[73])
    assert want[0]["extracted"]["read_status"].tolist() == [1] * 69 + [2] + [1] * 4 + [2]
    got, st = capi.haplotag_aligned_chunks(gpu_ctx, [chunk], [gt], f, r, ec.OPTS)
    assert_matches_oracle(got, want, "owner rule")
    assert got[0]["hap"][69] == -1 and got[0]["hap"][74] == -1 and (got[0]["hap"][:69] == got[0]["hap"][0]).all()
    assert st.entries == 73 and st.owners == 4 and st.active_sites == 1
    # the strand of the owner decides, not that of the first entry, of the low-mapq entry behind it or of the read itself:
    # reads 70 and 71 both carry read 71's scores (reverse strand), reads 0..68 read 68's (forward)
    sub70, sub0 = np.frombuffer(subs[70], np.uint8), np.frombuffer(subs[0], np.uint8)
    al = want[0]["sites"][0][0]
    s_rev = [ph.forward_probability(orv, al[a], sub70, (), 4) for a in (1, 0)]
    s_fwd = [ph.forward_probability(of, al[a], sub70, (), 4) for a in (1, 0)]
    assert np.float32(s_rev[0]) != np.float32(s_fwd[0]) or np.float32(s_rev[1]) != np.float32(s_fwd[1])
    assert got[0]["h1"][70] == got[0]["h1"][71] and got[0]["h2"][70] == got[0]["h2"][71]
    o_rev = [ph.forward_probability(orv, al[a], sub0, (), 4) for a in (1, 0)]
    o_fwd = [ph.forward_probability(of, al[a], sub0, (), 4) for a in (1, 0)]
    assert np.float32(o_rev[0]) != np.float32(o_fwd[0]) or np.float32(o_rev[1]) != np.float32(o_fwd[1])
    assert_identical(got, chain(gpu_ctx, [chunk], [gt], ec.OPTS, f, r), "owner rule")


def test_degenerate_inputs(gpu_ctx, synthetic):
    f, r, _, _ = models()
    got, st = capi.haplotag_aligned_chunks(gpu_ctx, [], [], f, r)
    assert got == [] and st.sites == 0 and st.entries == 0
    no_variants = ec.make([], [(100, "20M", 60, 0)])
    no_reads = ec.make([ec.SNP110], [])
    both = ec.make([], [])
    hom = synthetic[0][0]
    hom_gt = np.zeros((len(hom.alleles), 2), np.int32)
    lists = ec.cases()[-1][1]  # a low-mapq read, a read with nothing at or after it, a read without substring
    chunks = [no_variants, no_reads, both, hom, lists]
    gts = [None, np.array([[0, 1]], np.int32), None, hom_gt, np.array([[0, 1]], np.int32)]
    structs = [capi.aligned_chunk_struct(c) for c in chunks]
    got, st = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r, ec.OPTS, structs=structs)
    assert got[0]["hap"].tolist() == [-1] and got[1]["hap"].size == 0 and got[2]["hap"].size == 0
    status = eo.extract([hom], ec.OPTS)[0]["read_status"]
    assert (status == eo.KEPT).any() and (status != eo.KEPT).any()
    assert np.array_equal(got[3]["hap"], np.where(status == eo.KEPT, 0, -1))
    assert (got[3]["h1"] == 0).all() and (got[3]["h2"] == 0).all()
    assert got[4]["hap"].tolist() == [-1, -1, 0] and got[4]["h1"].tolist() == [0.0] * 3   # the only entry is the low-mapq read's
    assert st.active_sites == 0 and st.owners == 0 and st.pairhmm.pairs_lane + st.pairhmm.pairs_wave == 0
    assert_identical(got, chain(gpu_ctx, chunks, gts, ec.OPTS, f, r), "degenerate")
    # h1_out / h2_out NULL
    chunks, gts = synthetic[0][:2], synthetic[1][:2]
    full, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r)
    tags, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r, totals=False)
    for a, b in zip(tags, full):
        assert a["h1"] is None and a["h2"] is None and np.array_equal(a["hap"], b["hap"])


def test_diagonal_limit_is_raised_before_the_pair_hmm(gpu_ctx):
    # an SV-flagged variant whose window (expansion_sv = 2200) and a read spanning it make a pair of 2 000+ x 2 000+ symbols
    f, r, _, _ = models()
    rng = np.random.default_rng(5)
    n = 6_000
    ref = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))
    packed = synth.pack_seq([(1, 2, 4, 8)["ACGT".index(c)] for c in ref])
    chunk = synth.AlignedChunk(overlap_start=0, overlap_end=n, chunk_start=0, chunk_end=n, reference=ref, variant_pos=np.array([3_000], np.int64),
                               alleles=[[ref[3_000], "A" if ref[3_000] != "A" else "C"]], is_sv=np.array([1], np.uint8),
                               read_pos=np.array([0], np.int64), flag=np.array([0], np.uint16), mapq=np.array([60], np.uint8),
                               l_qseq=np.array([n], np.int32), cigar_first=np.array([0, 1], np.int64), cigar=np.array([n << 4], np.uint32),
                               seq_first=np.array([0, len(packed)], np.int64), seq=packed, read_names=["long"])
    opts = dict(capi.shipped_extract_options(), expansion_sv=2_200)
    with pytest.raises(capi.MrpError) as e:
        capi.haplotag_aligned_chunks(gpu_ctx, [chunk], [np.array([[0, 1]], np.int32)], f, r, opts)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "diagonal" in str(e.value)
    # the context is fine afterwards
    ok, _ = capi.haplotag_aligned_chunks(gpu_ctx, [chunk], [np.array([[0, 1]], np.int32)], f, r)
    assert ok[0]["hap"].tolist() in ([1], [2])


def test_repeat_and_host_threads(gpu_ctx, synthetic):
    f, r, _, _ = models()
    lib = capi.load()
    chunks, gts = synthetic
    first, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r)
    try:
        for threads in (1, 3, 0):
            lib.mrp_set_host_threads(threads)
            again, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r)
            assert_identical(again, first, f"threads {threads}")
    finally:
        lib.mrp_set_host_threads(0)
