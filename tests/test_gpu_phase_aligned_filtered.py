"""mrp_phase_aligned_chunks_with_filtered on the device: bit for bit against the chain it joins -- mrp_extract_read_substrings over
the chunk's variants and over the rest's (one call), mrp_string_chunk_from_extracted, mrp_string_chunk_rest_from_extracted,
mrp_phase_string_chunks_with_filtered -- every output, float bits included.  The composite runs the same kernels over the same pairs;
what it makes on the device instead of the host (owners, classes of equal substrings, k-mer anchors) is exact integer work, and a
different numbering of the classes only reorders pairs inside the launch.  So there is no tolerance anywhere in this file."""
import dataclasses

import numpy as np
import pytest

from margin_amd import capi
from tests import extract_cases as ec
from tests import rest_cases as rc
from tests import string_filtered_cases as sf
from tests import test_gpu_phase_aligned as pa
from tests.test_gpu_extract import OPTION_SETS

pytestmark = pytest.mark.gpu

MIN_PHRED = sf.MIN_PHRED  # leaves primary reads untagged: the partition then tags some of them
NOT_VISITED, CIS, TRANS = capi.VARIANT_NOT_VISITED, capi.VARIANT_CIS, capi.VARIANT_TRANS


@pytest.fixture(scope="module")
def synthetic():
    """six 8 kb / 8x chunks, one variant in five filtered -> (chunks of the primary variants, rests (filtered chunk, gt))"""
    chunks, rests = [], []
    for seed in range(6):
        primary, filtered, _ = rc.split_variants(rc.synthetic(seed))
        chunks.append(primary)
        rests.append((filtered, rc.genotypes(filtered, seed)))
    return chunks, rests


def chain(ctx, chunks, rests, keeps, opts, p, **kw):
    """-> (per chunk the dict phase_aligned_chunks_with_filtered gives, StringFilteredStats, symbol bytes of both extractions, the rests
    as dicts)"""
    f, r = pa.models()
    n = len(chunks)
    twice = list(chunks) + [dataclasses.replace(c, variant_pos=fl.variant_pos, alleles=fl.alleles, is_sv=fl.is_sv) for c, (fl, _) in zip(chunks, rests)]
    got, _ = capi.extract_read_substrings(ctx, twice, opts)  # both extractions in one call
    scs, bvs, ers = [], [], []
    for c in range(n):
        ch, (fl, gt), k = chunks[c], rests[c], (keeps or [None] * n)[c]
        sc, bv, _ = capi.string_chunk_from_extracted(got[c], ch.read_names, ch.read_forward_strand, keep=k)
        ers.append(capi.string_chunk_rest_from_extracted(got[c], got[n + c], ch.read_forward_strand, bv, fl.variant_pos, gt, ch.chunk_start, ch.chunk_end, k))
        scs.append(sc)
        bvs.append(bv)
    out, st = capi.phase_string_chunks_with_filtered(ctx, scs, [None] * n, f, r, p, profiles=True, rest_structs=[(e.struct, e) for e in ers], **kw)
    for d, bv, e in zip(out, bvs, ers):
        d["bubble_variant"] = bv
        d["filtered_read"] = e.filtered_read
    return out, st, sum(int(g["entry_len"].sum()) for g in got), [e.rest for e in ers]


def composite(ctx, chunks, rests, keeps, opts, p, **kw):
    f, r = pa.models()
    return capi.phase_aligned_chunks_with_filtered(ctx, chunks, rests, f, r, p, options=opts, keeps=keeps, profiles=True, **kw)


def assert_identical(got, want, where=""):
    pa.assert_identical(got, want, where)
    sf.assert_back_identical(got, [w["filtered"] for w in want])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["filtered_read"].dtype == np.int32 and np.array_equal(g["filtered_read"], w["filtered_read"]), (where, i)


def assert_stats_equal(st, cst):
    """the pair counts of the one launch equal the chain's"""
    for k in ("pairs_scored", "pairs_speculative", "pairs_read_by_results"):
        assert getattr(st, k) == getattr(cst, k), k
    a, b = st.aligned.chunks.pairhmm, cst.chunks.pairhmm
    assert (a.pairs_lane, a.pairs_wave, a.cells) == (b.pairs_lane, b.pairs_wave, b.cells)
    assert st.aligned.pairs == st.pairs_scored == a.pairs_lane + a.pairs_wave


@pytest.mark.parametrize("k", range(len(OPTION_SETS)))
def test_composite_equals_the_chain(gpu_ctx, synthetic, k):
    chunks, rests = synthetic
    p = pa.params()
    # one chunk is downsampled by the caller: with min_mapq 0 (the third option set) no read is of low mapq, and the discards of the
    # downsampling are then the call's only filtered reads
    keeps = [None] * 4 + [(np.random.default_rng(4).random(len(chunks[4].read_pos)) < 0.8).astype(np.uint8), None]
    got, st = composite(gpu_ctx, chunks, rests, keeps, OPTION_SETS[k], p, min_phred=MIN_PHRED)
    want, cst, symbol_bytes, rdicts = chain(gpu_ctx, chunks, rests, keeps, OPTION_SETS[k], p, min_phred=MIN_PHRED)
    # ---- conditions on the inputs, decided by the chain alone
    states = np.concatenate([w["filtered"]["variant_state"] for w in want])
    assert (states == CIS).any() and (states == TRANS).any() and (states == NOT_VISITED).any()
    fhap = np.concatenate([w["filtered"]["read_hap"][len(c.read_pos):] for c, w in zip(chunks, want)])
    assert (fhap == 1).any() and (fhap == 2).any()
    rescued = sum(int((((w["hap"] != 1) & (w["hap"] != 2)) & (w["filtered"]["read_hap"][:len(c.read_pos)] > 0)).sum()) for c, w in zip(chunks, want))
    assert rescued > 0  # a primary read the phasing left untagged and the partition then tags
    assert cst.pairs_speculative > 0 and cst.pairs_read_by_results > 0
    if OPTION_SETS[k]["expansion_sv"] >= 512:  # an anchored pair of a filtered variant: heterozygous, an entry of a primary read, a string past 512
        anchored = 0
        for c, rd in zip(chunks, rdicts):
            for alleles, gt, entries in rd["variants"]:
                if gt[0] != gt[1]:
                    anchored += sum(1 for q, s in entries if q < len(c.read_pos) and (len(s) > 512 or max(len(alleles[gt[0]]), len(alleles[gt[1]])) > 512))
        assert anchored > 0
    # ---- the composite
    assert_identical(got, want, f"options {k}")
    assert_stats_equal(st, cst)
    n_reads = sum(len(c.read_pos) for c in chunks)
    A = st.aligned
    assert st.filtered_variants == sum(len(fl.alleles) for fl, _ in rests) and A.variants == sum(len(c.alleles) for c in chunks) + st.filtered_variants
    assert st.filtered_reads == sum(len(g["filtered_read"]) for g in got) and A.extract.reads == 2 * n_reads
    assert 0 < st.filtered_entries < A.entries == A.extract.entries
    # what came back before the pair-HMM launch, to the byte; no symbol among it
    assert A.front_bytes_downloaded == 16 + 8 * (A.variants + 1) + 20 * A.entries + A.extract.reads + 4 * A.pairs_anchored + 12 * A.anchor_runs
    if k == 0:  # the shipped window widths
        assert A.front_bytes_downloaded < symbol_bytes
        assert A.pairs_anchored > 0
    assert st.classes_ms > 0 and st.filtered_ms > 0 and A.total_ms > 0
    # each chunk alone gives its share of the joint call
    for c in range(len(chunks)):
        one, _ = composite(gpu_ctx, chunks[c:c + 1], rests[c:c + 1], keeps[c:c + 1], OPTION_SETS[k], p, min_phred=MIN_PHRED)
        assert_identical(one, got[c:c + 1], f"options {k}, chunk {c} alone")
    # a repeat equals the first call
    again, ast = composite(gpu_ctx, chunks, rests, keeps, OPTION_SETS[k], p, min_phred=MIN_PHRED)
    assert_identical(again, got, f"options {k}, repeat")
    assert ast.aligned.front_bytes_downloaded == A.front_bytes_downloaded and ast.pairs_scored == st.pairs_scored


def test_mixed_call(gpu_ctx, synthetic):
    """keep masks, a chunk with an empty rest, one with filtered variants and no filtered read, one with no variants at all, and the
    hand-built chunk with every kind of filtered read"""
    chunks, rests = synthetic
    p = pa.params()
    rng = np.random.default_rng(8)
    hand = {name: (rc.split_hand(ch, fidx), gt, keep) for name, ch, fidx, gt, keep in rc.hand_cases()}
    nothing = ec.make([], [(100, "20M", 60, 0)])
    call = [(chunks[1], rests[1], (rng.random(len(chunks[1].read_pos)) < 0.7).astype(np.uint8)),
            (chunks[3], rests[3], (rng.random(len(chunks[3].read_pos)) < 0.4).astype(np.uint8)),
            (chunks[2], (rc.subset(chunks[2], []), []), None)]  # no filtered variant, no mask: low-mapq reads only
    for name in ("empty", "no_filtered_read", "kinds", "only_iii"):
        (primary, filtered), gt, keep = hand[name]
        call.append((primary, (filtered, gt), keep))
    call.append((nothing, (nothing, []), None))
    cs, rs, ks = [c for c, _, _ in call], [r for _, r, _ in call], [k for _, _, k in call]
    got, st = composite(gpu_ctx, cs, rs, ks, ec.OPTS, p, min_phred=MIN_PHRED)
    want, cst, _, rdicts = chain(gpu_ctx, cs, rs, ks, ec.OPTS, p, min_phred=MIN_PHRED)
    assert rdicts[3] is None and rdicts[7] is None                                       # the empty rests
    assert len(rdicts[4]["forward_strand"]) == 0 and len(rdicts[4]["variants"]) == 1    # filtered variants, no filtered read
    assert got[5]["filtered_read"].tolist() == [0, 2, 3] and got[6]["filtered_read"].tolist() == [1]
    assert_identical(got, want, "mixed")
    assert_stats_equal(st, cst)
    for c in (0, 1):  # a masked read is a filtered read of its chunk
        assert set(np.flatnonzero(ks[c] == 0)) & set(got[c]["filtered_read"].tolist())
    assert got[3]["filtered"]["read_hap"].size == len(cs[3].read_pos) and got[3]["filtered"]["variant_state"].size == 0
    # no chunk at all
    none, nst = composite(gpu_ctx, [], [], None, ec.OPTS, p)
    assert none == [] and nst.pairs_scored == 0 and nst.filtered_reads == 0


def test_owner_rule(gpu_ctx):
    """the 75-entry site of test_gpu_phase_aligned.owner_rule_chunk() and a filtered SNP four bases on: read 69, the would-be
    last-listed owner of the 70 equal substrings, is masked out, so it is a filtered read -- listed first in the partition, where the
    last-listed participant owns; the class spans kept, low-mapq (68) and masked reads on both strands"""
    p = pa.params()
    chunk, keep = pa.owner_rule_chunk()
    filtered = dataclasses.replace(chunk, variant_pos=np.array([114], np.int64), alleles=[[ec.REF[14], [c for c in "ACGT" if c != ec.REF[14]][0]]],
                                   is_sv=np.zeros(1, np.uint8))
    rests = [(filtered, [(0, 1)])]
    got, st = composite(gpu_ctx, [chunk], rests, [keep], ec.OPTS, p, min_phred=MIN_PHRED)
    want, cst, _, rdicts = chain(gpu_ctx, [chunk], rests, [keep], ec.OPTS, p, min_phred=MIN_PHRED)
    assert got[0]["filtered_read"].tolist() == [68, 74, 69]  # low mapq ascending, then the masked read
    assert [fr for fr, _ in rdicts[0]["fsubs"][0]] == [0, 1, 2]
    assert_identical(got, want, "owner rule")
    assert_stats_equal(st, cst)
    assert st.aligned.entries_used == 72 and st.aligned.owners == 4 and st.filtered_variants == 1 and st.filtered_reads == 3
    # with read 67 masked out as well
    keep2 = keep.copy()
    keep2[67] = 0
    other, ost = composite(gpu_ctx, [chunk], rests, [keep2], ec.OPTS, p, min_phred=MIN_PHRED)
    want2, cst2, _, _ = chain(gpu_ctx, [chunk], rests, [keep2], ec.OPTS, p, min_phred=MIN_PHRED)
    assert_identical(other, want2, "owner rule, two masked")
    assert_stats_equal(ost, cst2)
    assert other[0]["filtered_read"].tolist() == [68, 74, 67, 69]
