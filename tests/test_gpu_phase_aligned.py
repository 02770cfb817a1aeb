"""mrp_phase_aligned_chunks on the device: bit for bit against the chain it joins, mrp_extract_read_substrings ->
mrp_string_chunk_from_extracted (keep, names, strand from the flag) -> mrp_phase_string_chunks -- every output, float bits included.
Nothing may differ: the same pair-HMM, phasing and HP kernels run over the same pairs, and what the composite makes on the device
instead of the host (the owners of equal substrings under the mask, the k-mer anchors) is exact integer work.  So there is no
tolerance anywhere in this file."""
import struct

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests.test_gpu_extract import OPTION_SETS

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("ref_start", "length", "hap1", "hap2", "genotype", "ancestor", "genotype_probs", "hap_probs1", "hap_probs2", "support1", "support2",
               "reads1", "reads2", "hmm_forward", "hmm_backward", "n_sweeps")
PROFILE_KEYS = ("read_of_seq", "pool", "allele_number", "sub", "prior")


def models():
    f = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    return f, f.reverse_complement()


def params(pd=None):
    return capi.Params.from_reference_names(pd or synth.shipped_phase_params())


@pytest.fixture(scope="module")
def synthetic():
    return [synth.make_aligned_chunk(seed, overlap_bp=8_000, coverage=8.0) for seed in range(6)]


def chain(ctx, chunks, keeps, opts, p, **kw):
    """the three calls the composite joins -> (per chunk the dict phase_aligned_chunks gives, symbol bytes of all entries)"""
    f, r = models()
    got, _ = capi.extract_read_substrings(ctx, chunks, opts)
    scs, bvs = [], []
    for c, g, k in zip(chunks, got, keeps or [None] * len(chunks)):
        sc, bv, _ = capi.string_chunk_from_extracted(g, c.read_names, c.read_forward_strand, keep=k)
        scs.append(sc)
        bvs.append(bv)
    out, st = capi.phase_string_chunks(ctx, scs, f, r, p, profiles=True, **kw)
    for d, bv in zip(out, bvs):
        d["bubble_variant"] = bv
    return out, st, sum(int(g["entry_len"].sum()) for g in got)


def bits(v):
    return v.tobytes() if isinstance(v, np.ndarray) else struct.pack("<d", v) if isinstance(v, float) else v


def assert_identical(got, want, where=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in RESULT_KEYS:
            a, b = g["result"][k], w["result"][k]
            assert type(a) is type(b) and (not isinstance(a, np.ndarray) or (a.dtype == b.dtype and a.shape == b.shape)), (where, i, k)
            assert bits(a) == bits(b), (where, i, k)
        assert g["hap"].dtype == np.int8 and np.array_equal(g["hap"], w["hap"]), (where, i, "hap")
        assert g["phred"].tobytes() == w["phred"].tobytes(), (where, i, "phred")
        assert g["bubble_variant"].dtype == np.int64 and np.array_equal(g["bubble_variant"], w["bubble_variant"]), (where, i, "bubble_variant")
        assert g["profile"]["seqs"] == w["profile"]["seqs"], (where, i, "seqs")
        for k in PROFILE_KEYS:
            a, b = g["profile"][k], w["profile"][k]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, i, k)


def composite(ctx, chunks, keeps, opts, p, **kw):
    f, r = models()
    return capi.phase_aligned_chunks(ctx, chunks, f, r, p, options=opts, keeps=keeps, profiles=True, **kw)


@pytest.mark.parametrize("k", range(len(OPTION_SETS)))
def test_composite_equals_the_chain(gpu_ctx, synthetic, k):
    p = params()
    got, st = composite(gpu_ctx, synthetic, None, OPTION_SETS[k], p, min_phred=3)
    want, cst, symbol_bytes = chain(gpu_ctx, synthetic, None, OPTION_SETS[k], p, min_phred=3)
    assert_identical(got, want, f"options {k}")
    # what the input exercises: duplicates, SV pairs that are anchored, both pair-HMM kernels, tagged and untagged reads
    assert st.entries_used > st.owners > 0 and st.bubbles > 0 and st.pairs == cst.pairhmm.pairs_lane + cst.pairhmm.pairs_wave
    assert st.chunks.pairhmm.pairs_lane == cst.pairhmm.pairs_lane > 0 and st.chunks.pairhmm.pairs_wave == cst.pairhmm.pairs_wave > 0
    assert st.chunks.pairhmm.cells == cst.pairhmm.cells and st.chunks.phase.resident == 1
    if OPTION_SETS[k]["expansion_sv"] >= 512:
        assert st.pairs_anchored > 0 and st.anchors > 0
    assert st.bubbles == sum(len(g["bubble_variant"]) for g in got) <= st.variants == sum(len(c.alleles) for c in synthetic)
    assert any((g["hap"] == -1).any() and (g["hap"] == 1).any() and (g["hap"] == 2).any() for g in got)
    # what came back before the pair-HMM launch: the extraction's totals, the entry CSR, per entry its length (8 B), read and owner
    # (4 B each), per read its status, per anchored pair a count, the anchors as diagonal runs (12 B each) -- and not the substrings'
    # symbols.  That is less than the symbols where the windows have the shipped width: with windows of a few symbols (the other
    # option sets) the 16 B of indices per entry alone exceed them.
    n_reads = sum(len(c.read_pos) for c in synthetic)
    assert st.entries == st.extract.entries and st.extract.reads == n_reads
    assert st.front_bytes_downloaded == 16 + 8 * (st.variants + 1) + 16 * st.entries + n_reads + 4 * st.pairs_anchored + 12 * st.anchor_runs
    assert st.anchor_runs <= st.anchors
    if k == 0:
        assert st.front_bytes_downloaded < symbol_bytes
    assert st.total_ms > 0 and st.owners_ms > 0 and st.chunks.pairhmm.kernel_ms > 0 and st.extract.kernel_ms > 0
    # each chunk alone gives its share of the joint call
    for c in range(len(synthetic)):
        one, _ = composite(gpu_ctx, synthetic[c:c + 1], None, OPTION_SETS[k], p, min_phred=3)
        assert_identical(one, got[c:c + 1], f"options {k}, chunk {c} alone")


def test_keep_masks_and_repeat(gpu_ctx, synthetic):
    p = params()
    chunks = synthetic[:4]
    rng = np.random.default_rng(8)
    keeps = [None, (rng.random(len(chunks[1].read_pos)) < 0.7).astype(np.uint8), None, (rng.random(len(chunks[3].read_pos)) < 0.4).astype(np.uint8)]
    opts = capi.shipped_extract_options()
    got, st = composite(gpu_ctx, chunks, keeps, opts, p)
    want, _, _ = chain(gpu_ctx, chunks, keeps, opts, p)
    assert_identical(got, want, "masks")
    unmasked, ust = composite(gpu_ctx, chunks, None, opts, p)
    assert st.entries == ust.entries and st.entries_used < ust.entries_used and st.pairs_anchored > 0 and st.anchors > 0
    for c in (1, 3):
        assert (got[c]["hap"][keeps[c] == 0] == -1).all() and (unmasked[c]["hap"][keeps[c] == 0] != -1).any()
    again, ast = composite(gpu_ctx, chunks, keeps, opts, p)
    assert_identical(again, got, "repeat")
    assert ast.front_bytes_downloaded == st.front_bytes_downloaded and ast.anchors == st.anchors and ast.anchor_runs == st.anchor_runs


def owner_rule_chunk():
    """One SNP site with 75 entries, as tests/test_gpu_haplotag_aligned.py builds it: reads 0..69 are the same alignment on alternating
    strands (read 0 forward), so their substrings are equal.  Read 69 would own their scores (the last listed); the mask takes it out,
    read 68 behind it has low mapq, so read 67, on the reverse strand, owns them.  70 (forward) and 71 (reverse) share another
    substring, 72 and 73 have their own, 74 is a low-mapq copy of 70."""
    reads = [(100, "20M", 3 if i == 68 else 60, 0x10 if i % 2 else 0) for i in range(70)]
    reads += [(101, "19M", 60, 0), (101, "19M", 60, 0x10), (100, "10M2I8M", 60, 0), (100, "11M1D8M", 60, 0x10), (101, "19M", 2, 0)]
    keep = np.ones(75, np.uint8)
    keep[69] = 0
    return ec.make([(110, [ec.REF[10], "G"], 0)], reads), keep


def test_owner_rule_under_the_mask(gpu_ctx):
    p = params()
    chunk, keep = owner_rule_chunk()
    got, st = composite(gpu_ctx, [chunk], [keep], ec.OPTS, p)
    want, _, _ = chain(gpu_ctx, [chunk], [keep], ec.OPTS, p)
    assert_identical(got, want, "owner rule")
    assert st.entries == 75 and st.entries_used == 72 and st.owners == 4 and st.bubbles == 1 and st.pairs == 8
    hap = got[0]["hap"]
    assert hap[69] == -1 and hap[68] == -1 and hap[74] == -1 and (hap[:68] != -1).all() and (hap[70:74] != -1).all()
    # with read 67 masked out as well the forward read 66 owns the scores
    keep2 = keep.copy()
    keep2[67] = 0
    other, ost = composite(gpu_ctx, [chunk], [keep2], ec.OPTS, p)
    assert_identical(other, chain(gpu_ctx, [chunk], [keep2], ec.OPTS, p)[0], "owner rule, forward owner")
    assert ost.entries_used == 71 and ost.owners == 4 and other[0]["hap"][67] == -1


def test_lowered_sv_threshold(gpu_ctx, synthetic):
    # the windows of small variants (25 symbols) are anchored too: most pairs of the call go through the anchors kernel and the banded pair-per-wave kernel
    p = params()
    chunks = synthetic[:3]
    opts = capi.shipped_extract_options()
    got, st = composite(gpu_ctx, chunks, None, opts, p, sv_threshold=20)
    want, cst, _ = chain(gpu_ctx, chunks, None, opts, p, sv_threshold=20)
    assert_identical(got, want, "sv_threshold 20")
    normal, nst = composite(gpu_ctx, chunks, None, opts, p)
    assert st.pairs == nst.pairs and st.pairs_anchored > 4 * nst.pairs_anchored and st.anchors > nst.anchors
    assert st.chunks.pairhmm.pairs_wave == cst.pairhmm.pairs_wave > nst.chunks.pairhmm.pairs_wave


def test_degenerate_inputs(gpu_ctx, synthetic):
    p = params()
    got, st = composite(gpu_ctx, [], None, ec.OPTS, p)
    assert got == [] and st.variants == 0 and st.entries == 0 and st.pairs == 0
    no_variants = ec.make([], [(100, "20M", 60, 0)])
    no_reads = ec.make([ec.SNP110], [])
    both = ec.make([], [])
    lists = ec.cases()[-1][1]  # a low-mapq read, a read with nothing at or after it, a read without substring: no bubble
    chunks = [no_variants, no_reads, both, lists]
    got, st = composite(gpu_ctx, chunks, None, ec.OPTS, p)
    # (the chain without the chunk that has a variant and no entry: the binding hands mrp_string_chunk_from_extracted NULL for its
    # empty entry arrays, which that call refuses; what the composite gives for it is asserted below)
    want, _, _ = chain(gpu_ctx, chunks[:1] + chunks[2:], None, ec.OPTS, p)
    assert_identical(got[:1] + got[2:], want, "degenerate")
    assert got[1]["result"]["reads1"] == [] and got[1]["result"]["reads2"] == [] and got[1]["profile"]["seqs"] == []
    assert got[0]["hap"].tolist() == [-1] and got[1]["hap"].size == 0 and got[3]["hap"].tolist() == [-1, -1, -1]
    assert st.bubbles == 0 and st.pairs == 0 and st.entries == 1 and st.entries_used == 0
    assert all(len(g["bubble_variant"]) == 0 and g["result"]["length"] == 0 for g in got)
    # every read masked out: the entries are there, none takes part
    chunks = synthetic[:2]
    keeps = [np.zeros(len(c.read_pos), np.uint8) for c in chunks]
    got, st = composite(gpu_ctx, chunks, keeps, capi.shipped_extract_options(), p)
    want, _, _ = chain(gpu_ctx, chunks, keeps, capi.shipped_extract_options(), p)
    assert_identical(got, want, "all masked")
    assert st.entries > 0 and st.entries_used == 0 and st.bubbles == 0 and all((g["hap"] == -1).all() for g in got)
    # a masked chunk beside an unmasked one
    keeps[1] = None
    got, st = composite(gpu_ctx, chunks, keeps, capi.shipped_extract_options(), p)
    assert_identical(got, chain(gpu_ctx, chunks, keeps, capi.shipped_extract_options(), p)[0], "one masked")
    assert len(got[0]["bubble_variant"]) == 0 and len(got[1]["bubble_variant"]) > 0


def test_outside_the_resident_range(gpu_ctx, synthetic):
    # the unit tests' parameters in sum mode: the per-chunk path, over the host copy of the device-built profile pool
    p = params(synth.unit_test_params(max_partitions=50, max_not_sum=0))
    chunks = synthetic[2:3]
    got, st = composite(gpu_ctx, chunks, None, capi.shipped_extract_options(), p)
    want, cst, _ = chain(gpu_ctx, chunks, None, capi.shipped_extract_options(), p)
    assert st.chunks.phase.resident == 0 and cst.phase.resident == 0
    assert_identical(got, want, "per-chunk path")


def long_window_chunk():
    """an SV-flagged variant whose window (expansion_sv = 2 200) and a read spanning it make pairs of 4 000+ x 4 000+ symbols"""
    rng = np.random.default_rng(5)
    n = 6_000
    ref = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))
    packed = synth.pack_seq([(1, 2, 4, 8)["ACGT".index(c)] for c in ref])
    return synth.AlignedChunk(overlap_start=0, overlap_end=n, chunk_start=0, chunk_end=n, reference=ref, variant_pos=np.array([3_000], np.int64),
                              alleles=[[ref[3_000], "A" if ref[3_000] != "A" else "C"]], is_sv=np.array([1], np.uint8),
                              read_pos=np.array([0], np.int64), flag=np.array([0], np.uint16), mapq=np.array([60], np.uint8),
                              l_qseq=np.array([n], np.int32), cigar_first=np.array([0, 1], np.int64), cigar=np.array([n << 4], np.uint32),
                              seq_first=np.array([0, len(packed)], np.int64), seq=packed, read_names=["long"])


def test_diagonal_limit_is_raised_before_the_pair_hmm(gpu_ctx):
    p = params()
    chunk = long_window_chunk()
    opts = dict(capi.shipped_extract_options(), expansion_sv=2_200)
    # unanchored (sv_threshold above the lengths) the pairs cover their whole matrix: a diagonal beyond 2 048 cells.  The binding checks
    # that no output was written.
    with pytest.raises(capi.MrpError) as e:
        composite(gpu_ctx, [chunk], None, opts, p, sv_threshold=100_000)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "diagonal" in str(e.value)
    with pytest.raises(capi.MrpError) as e:
        chain(gpu_ctx, [chunk], None, opts, p, sv_threshold=100_000)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED
    # the context is fine afterwards; anchored, the same pairs are banded around some 4 000 anchors each and go through
    got, st = composite(gpu_ctx, [chunk], None, opts, p)
    want, _, _ = chain(gpu_ctx, [chunk], None, opts, p)
    assert_identical(got, want, "long window, anchored")
    assert st.pairs == 2 and st.pairs_anchored == 2 and st.anchors > 8_000
