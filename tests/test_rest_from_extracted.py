"""mrp_string_chunk_rest_from_extracted against its Python restatement (tests/rest_cases.py), without a device: the two
extractions come from tests/extract_oracle.py."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import extract_oracle as xo
from tests import rest_cases as rc

SEEDS = (3, 5, 8)
MASKS = {3: None, 5: 0.7, 8: 0.4}


def build(chunk, primary, filtered, gt, keep, opts):
    """-> dict(x, xf (oracle results), got (capi.ExtractedRest), want (flist, rest), sc (the string chunk), bv)"""
    x, = xo.extract([primary], opts)
    xf, = xo.extract([filtered], opts)
    strand = chunk.read_forward_strand
    sc, bv, _ = capi.string_chunk_from_extracted(xo.as_arrays(x), chunk.read_names, strand, keep)
    got = capi.string_chunk_rest_from_extracted(xo.as_arrays(x), xo.as_arrays(xf), strand, bv, filtered.variant_pos, gt, chunk.chunk_start,
                                                chunk.chunk_end, keep)
    want = rc.rest_reference(x, xf, keep, strand, bv, filtered.variant_pos, gt, chunk.chunk_start, chunk.chunk_end)
    return dict(x=x, xf=xf, got=got, want=want, sc=sc, bv=bv, keep=keep, n_reads=len(strand))


@pytest.fixture(scope="module")
def synthetic():
    out = {}
    for seed in SEEDS:
        chunk = rc.synthetic(seed)
        primary, filtered, fidx = rc.split_variants(chunk)
        opts = capi.shipped_extract_options()
        x0, = xo.extract([primary], opts)
        keep = None if MASKS[seed] is None else rc.keep_mask(x0, seed, MASKS[seed])
        out[seed] = dict(build(chunk, primary, filtered, rc.genotypes(filtered, seed), keep, opts), chunk=chunk, filtered=filtered, fidx=fidx)
    return out


@pytest.fixture(scope="module")
def hand():
    out = {}
    for name, chunk, fidx, gt, keep in rc.hand_cases():
        primary, filtered = rc.split_hand(chunk, fidx)
        out[name] = dict(build(chunk, primary, filtered, np.array(gt, np.int32).reshape(-1, 2), keep, ec.OPTS), chunk=chunk, filtered=filtered)
    return out


def through_the_string_call(case):
    """the C-made rest, unchanged, into mrp_phase_string_chunks_with_filtered with a NULL context"""
    lib = capi.load()
    S, hold = capi.string_chunk_struct(case["sc"])
    arr, rarr = (capi.StringChunk * 1)(S), (capi.StringChunkRest * 1)(case["got"].struct)
    hap = np.zeros(max(case["n_reads"], 1), np.int8)
    hp = (C.c_void_p * 1)(hap.ctypes.data)
    res = (C.POINTER(capi.PhaseResult) * 1)()
    fout = (capi.FilteredOut * 1)()
    m = capi.PairHmm.default_nucleotide()
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    return lib.mrp_phase_string_chunks_with_filtered(None, 1, arr, rarr, C.byref(m), C.byref(m), 4, 512, 0.0, C.byref(p), 0, res, hp, None, None, fout, None)


@pytest.mark.parametrize("seed", SEEDS)
def test_synthetic_chunks(synthetic, seed):
    case = synthetic[seed]
    flist, want = case["want"]
    rc.assert_rest_equal(case["got"], flist, want)
    assert through_the_string_call(case) == capi.MRP_ERR_NO_DEVICE, capi.load().mrp_last_error()


def test_the_synthetic_inputs_cover_the_rules(synthetic):
    """so that a pass means something: low-mapq and masked reads (a read of kind (iii) needs the primary variants to end before the
    chunk does: the hand-built chunks have one), a pair of filtered variants at one position, filtered variants
    outside the chunk with entries in xf, a homozygous gt, entries of masked and of primary reads at filtered variants"""
    kinds, same_pos, outside, hom, masked_entry, primary_entry = set(), 0, 0, 0, 0, 0
    for case in synthetic.values():
        x, xf, keep, ch, fl = case["x"], case["xf"], case["keep"], case["chunk"], case["filtered"]
        flist, want = case["want"]
        n = case["n_reads"]
        for r in flist:
            kinds.add("i" if x["read_status"][r] == rc.FILTERED else "ii" if x["read_status"][r] == rc.KEPT else "iii")
        pos = np.asarray(fl.variant_pos)
        same_pos += int((pos[1:] == pos[:-1]).sum())
        for v, (_al, g, entries) in enumerate(want["variants"]):
            if not ch.chunk_start <= pos[v] < ch.chunk_end:
                assert not entries
                outside += len(xf["entries"][v]) > 0
            hom += g[0] == g[1]
            masked_entry += sum(1 for r, _ in entries if r >= n and keep is not None and x["read_status"][flist[r - n]] == rc.KEPT)
            primary_entry += sum(1 for r, _ in entries if r < n)
    assert kinds >= {"i", "ii"} and same_pos and outside and hom and masked_entry and primary_entry


@pytest.mark.parametrize("name", ["kinds", "only_iii", "no_filtered_read", "no_filtered_variant", "empty"])
def test_hand_built_chunks(hand, name):
    case = hand[name]
    flist, want = case["want"]
    rc.assert_rest_equal(case["got"], flist, want)
    assert through_the_string_call(case) == capi.MRP_ERR_NO_DEVICE, capi.load().mrp_last_error()


def test_list_order_and_indices(hand):
    """(i) low mapq, (ii) masked, (iii) only at a filtered variant; a masked read's entries carry n_reads + f; the variant outside the
    chunk has no entries; a homozygous gt is kept as given"""
    case = hand["kinds"]
    got, n = case["got"], case["n_reads"]
    assert got.filtered_read.tolist() == [0, 2, 3]
    assert got.rest["forward_strand"].tolist() == [1, 0, 1]
    assert [[f for f, _ in b] for b in got.rest["fsubs"]] == [[0, 1]]  # the bubble at 110: the low-mapq and the masked read, not read 3
    v125, v126, v134 = got.rest["variants"]
    assert [r for r, _ in v125[2]] == [1, n + 1, n + 2, 4] and [r for r, _ in v126[2]] == [1, n + 1, n + 2, 4]  # read 0 (low mapq) not listed
    assert v126[1] == (2, 1) and len(v126[0]) == 3
    assert v134[1] == (1, 1) and v134[2] == [] and len(case["xf"]["entries"][2]) > 0
    raw = got.raw  # xf's symbols first, its offsets as they are; the copied substrings behind them
    fx = xo.as_arrays(case["xf"])
    assert (raw["pool"][:len(fx["pool"])] == fx["pool"]).all() and (raw["valle_off"] == fx["allele_off"]).all()
    assert (raw["fsub_off"] >= len(fx["pool"])).all() and raw["pool"].size == len(fx["pool"]) + int(raw["fsub_len"].sum())


def test_a_read_only_at_a_filtered_variant(hand):
    case = hand["only_iii"]
    got, n = case["got"], case["n_reads"]
    assert case["x"]["read_status"].tolist() == [rc.KEPT, rc.DROPPED] and case["xf"]["read_status"].tolist() == [rc.KEPT, rc.KEPT]
    assert got.filtered_read.tolist() == [1] and got.rest["forward_strand"].tolist() == [0]
    assert got.rest["fsubs"] == [[]]
    (alleles, g, entries), = got.rest["variants"]
    assert g == (1, 0) and [r for r, _ in entries] == [n + 0]


def test_partial_and_empty_rests(hand):
    a = hand["no_filtered_read"]["got"]
    assert a.struct.n_filtered == 0 and a.struct.n_variants == 1 and [r for r, _ in a.rest["variants"][0][2]] == [0, 1]
    b = hand["no_filtered_variant"]["got"]
    assert b.filtered_read.tolist() == [1, 2] and b.struct.n_variants == 0 and [[f for f, _ in s] for s in b.rest["fsubs"]] == [[0, 1]]
    e = hand["empty"]["got"]
    assert e.rest is None and e.block is None and bytes(e.struct) == bytes(capi.StringChunkRest())


def test_argument_errors(hand):
    case = hand["kinds"]
    ch, fl = case["chunk"], case["filtered"]
    xa, xfa = xo.as_arrays(case["x"]), xo.as_arrays(case["xf"])
    args = (ch.read_forward_strand, case["bv"], fl.variant_pos)
    good = np.array([(0, 1), (2, 1), (1, 1)], np.int32)

    def err(gt=good, x=xa, xf=xfa, **kw):
        with pytest.raises(capi.MrpError) as e:
            capi.string_chunk_rest_from_extracted(x, xf, *args, gt, ch.chunk_start, ch.chunk_end, case["keep"], **kw)
        return e.value.code

    for bad in ([(0, 2), (2, 1), (1, 1)], [(0, 1), (3, 1), (1, 1)], [(0, 1), (2, 1), (-1, 1)]):  # a gt outside the variant's alleles
        assert err(np.array(bad, np.int32)) == capi.MRP_ERR_ARG
    for null in ("x", "xf", "out", "filtered_read", "block", "gt", "fvariant_pos", "strand", "bubble_variant"):
        assert err(nulls=(null,)) == capi.MRP_ERR_ARG, null
    fewer = dict(xfa, read_status=xfa["read_status"][:-1], read_n_substrings=xfa["read_n_substrings"][:-1])  # not the same reads
    assert err(xf=fewer) == capi.MRP_ERR_ARG
    with pytest.raises(capi.MrpError):
        capi.string_chunk_rest_from_extracted(xa, xfa, ch.read_forward_strand, np.array([7], np.int64), fl.variant_pos, good, 100, 130, case["keep"])
