"""The phased variant records on the host: mrp_variant_records_from_extracted and mrp_variants_from_records against the plain-Python
restatement of the reference (tests/variant_records_oracle.py), mrp_phase_sets over their result, and the argument checks of
mrp_phase_aligned_chunks_with_records without a device.  Every comparison is exact: integers, and floats as bits -- nothing is
recomputed in floating point."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

from margin_amd import capi, synth
from oracle import frame_oracle as fo
from tests import extract_cases as ec
from tests import extract_oracle as xo
from tests import rest_cases as rc
from tests import variant_records_oracle as vo


def alts(rel):
    return [c for c in "ACGT" if c != ec.REF[rel]]


def snp(pos, n_alt=1):
    return (pos, [ec.REF[pos - 100]] + alts(pos - 100)[:n_alt], 0)


# ---- the hand-built chunk: the overlap slice is genome 100..139, windows of +-2, the chunk itself [106, 134) -----------------------
# reads 0, 1, 4, 5, 7: primary, a deletion over the window of the variant at 120 (no substring there); read 6: primary, ends at 116;
# read 2: low mapq; read 3: kept by the extraction, masked out by the caller
READS = [(100, "17M7D16M", 60, 0), (100, "17M7D16M", 60, 0x10), (100, "40M", 3, 0), (100, "40M", 60, 0), (100, "17M7D16M", 60, 0),
         (100, "17M7D16M", 60, 0x10), (100, "17M", 60, 0), (100, "17M7D16M", 60, 0)]
KEEP = np.array([1, 1, 1, 0, 1, 1, 1, 1], np.uint8)
HAP = np.array([1, 2, 1, 2, 0, -1, 1, 2], np.int8)  # (the tags of reads 2 and 3 must not count: they are not primary)
PRIMARY = [snp(104), snp(108), snp(110), snp(114, 2), snp(120), snp(128), snp(132), snp(136)]
FILTERED = [snp(112), snp(116), snp(126), snp(130), snp(135)]
FGT = [(0, 1), (1, 0), (0, 1), (1, 1), (0, 1)]
FSTATE = [vo.CIS, vo.TRANS, vo.TIE, vo.NOT_VISITED, vo.NOT_VISITED]  # (135 lies outside the chunk: the back half never visits it)
START, END = 106, 134


@pytest.fixture(scope="module")
def hand():
    ch = ec.make(PRIMARY, READS, chunk_start=START, chunk_end=END)
    fl = ec.make(FILTERED, READS, chunk_start=START, chunk_end=END)
    x, xf = xo.extract([ch, fl], ec.OPTS)
    _, bv = xo.bubbles_from_extracted(x, KEEP)
    return dict(x=x, xf=xf, bv=bv, vpos=ch.variant_pos, fpos=fl.variant_pos)


def fragment(ref_start, length, hap1, hap2, seed=1):
    rng = np.random.default_rng(seed)
    probs = lambda: (-rng.random(length) * 9).astype(np.float32)
    return dict(ref_start=ref_start, length=length, hap1=np.array(hap1, np.uint64), hap2=np.array(hap2, np.uint64), genotype_probs=probs(),
                hap_probs1=probs(), hap_probs2=probs())


def both(h, gf, keep=KEEP, hap=HAP, state=FSTATE, gt=FGT, start=START, end=END, **kw):
    """-> (the C function's records, the oracle's)"""
    got = capi.variant_records_from_extracted(xo.as_arrays(h["x"]), xo.as_arrays(h["xf"]), keep, h["bv"], gf, hap, h["vpos"], h["fpos"], start, end, gt,
                                              state, **kw)
    prim = vo.update_with_bubble_data(h["x"], keep, h["bv"], gf, hap, h["vpos"], start, end)
    filt = vo.update_filtered(h["x"], h["xf"], keep, hap, h["fpos"], gt, state, start, end)
    return got, vo.records_arrays(prim, filt)


def test_hand_chunk_every_branch(hand):
    h = hand
    # the inputs are what the comments say: the variant at 120 has substrings of reads 2 and 3 only, so it makes no bubble
    assert [r for r, _ in h["x"]["entries"][4]] == [2, 3] and list(h["bv"]) == [0, 1, 2, 3, 5, 6, 7]
    assert h["x"]["read_status"][2] == xo.FILTERED and h["x"]["read_status"][3] == xo.KEPT
    # the fragment over all seven bubbles; a homozygous call at 128 (bubble 4); the third allele at 114
    gf = fragment(0, 7, [0, 1, 0, 2, 1, 0, 1], [1, 0, 1, 0, 1, 1, 0])
    got, want = both(h, gf)
    vo.assert_records_equal(got, want, "whole fragment")
    U, D, Cl = vo.UNTOUCHED, vo.UPDATED, vo.CLEARED
    #                         104 margin, 108, 110, 114, 120 no bubble, 128, 132, 136 margin | CIS, TRANS, TIE, NOT_VISITED x 2
    assert got["state"].tolist() == [U, D, D, D, U, D, D, U, D, D, Cl, U, U]
    assert got["gt"].tolist() == [[-2, -2], [1, 0], [0, 1], [2, 0], [-2, -2], [1, 1], [0, 1], [-2, -2], [0, 1], [0, 1], [-1, -1], [-2, -2], [-2, -2]]
    # masked (3) and low-mapq (2) reads are listed nowhere, nor are tags 0 (read 4) and -1 (read 5); read 6 ends before 128
    lists = lambda s: (got["reads"][got["read_first"][s]:][:got["n_hap1"][s]].tolist(), got["reads"][got["read_first"][s] + got["n_hap1"][s]:got["read_first"][s + 1]].tolist())
    assert lists(1) == ([0, 6], [1, 7]) and lists(5) == ([0], [1, 7]) and lists(8) == ([0, 6], [1, 7]) and lists(10) == ([], [])
    assert got["genotype_log_prob"][1].view(np.uint32) == gf["genotype_probs"][1].view(np.uint32)
    assert np.isneginf(got["hap1_log_prob"][8:11]).all() and (got["hap1_log_prob"][11:] == 0).all()
    # a fragment that leaves bubbles out on both sides: 108 (bubble 1) is inside the chunk and outside the fragment
    gf2 = fragment(2, 3, [0, 2, 1], [1, 0, 0], seed=2)
    got2, want2 = both(h, gf2)
    vo.assert_records_equal(got2, want2, "inner fragment")
    assert got2["state"][:8].tolist() == [U, U, D, D, U, D, U, U]
    # an empty fragment; no mask; every read tagged; each state at each filtered variant inside the chunk
    vo.assert_records_equal(*both(h, fragment(0, 0, [], [])), "no fragment")
    vo.assert_records_equal(*both(h, gf, keep=None), "no mask")
    vo.assert_records_equal(*both(h, gf, keep=None, hap=np.array([1, 2, 1, 2, 1, 2, 1, 2], np.int8)), "all tagged")
    for k in range(4):
        state = [(k + v) % 4 for v in range(4)] + [vo.NOT_VISITED]
        got3, want3 = both(h, gf, state=state)
        vo.assert_records_equal(got3, want3, f"states {state}")
    # the chunk's limits move: each margin variant is updated once its position is inside
    got4, want4 = both(h, gf, start=100, end=140, state=[vo.CIS] * 5)
    vo.assert_records_equal(got4, want4, "whole slice")
    assert got4["state"].tolist() == [D, D, D, D, U, D, D, D, D, D, D, D, D]


@pytest.mark.parametrize("seed", [0, 1])
def test_synthetic_chunk_random_outcome(seed):
    """an 8 kb / 8x chunk through the extraction oracle, with a made-up phasing: fragment, tags, states"""
    primary, filtered, _ = rc.split_variants(rc.synthetic(seed))
    x, xf = xo.extract([primary, filtered], capi.shipped_extract_options())
    rng = np.random.default_rng([seed, 5])
    keep = rc.keep_mask(x, seed, 0.8)
    _, bv = xo.bubbles_from_extracted(x, keep)
    nb = len(bv)
    f0, f1 = nb // 7, nb - nb // 9
    na = [len(x["alleles"][v]) for v in bv[f0:f1]]
    gf = fragment(f0, f1 - f0, [rng.integers(k) for k in na], [rng.integers(k) for k in na], seed)
    hap = rng.choice(np.array([1, 2, 0, -1], np.int8), len(x["read_status"]), p=[0.4, 0.4, 0.1, 0.1])
    gt = rc.genotypes(filtered, seed)
    state = rng.integers(0, 4, len(gt))
    h = dict(x=x, xf=xf, bv=bv, vpos=primary.variant_pos, fpos=filtered.variant_pos)
    got, want = both(h, gf, keep=keep, hap=hap, state=state, gt=gt, start=primary.chunk_start, end=primary.chunk_end)
    vo.assert_records_equal(got, want, f"seed {seed}")
    assert set(got["state"].tolist()) == {0, 1, 2} and (got["n_hap1"] > 0).any() and (got["n_hap2"] > 0).any()


def test_records_errors_leave_the_output_unwritten(hand):
    h = hand
    gf = fragment(0, 7, [0, 1, 0, 2, 1, 0, 1], [1, 0, 1, 0, 1, 1, 0])

    def code(**kw):
        args = dict(h=h, gf=gf)
        args.update(kw)
        with pytest.raises(capi.MrpError) as e:  # (the binding asserts that the output struct is unwritten)
            both(args.pop("h"), args.pop("gf"), **args)
        return e.value.code
    for what in ("x", "xf", "result", "out", "bubble_variant", "hap", "variant_pos", "fvariant_pos", "gt", "variant_state"):
        assert code(nulls=(what,)) == capi.MRP_ERR_ARG, what
    # extractions over different read counts
    fewer = ec.make(FILTERED, READS[:-1], chunk_start=START, chunk_end=END)
    assert code(h=dict(h, xf=xo.extract([fewer], ec.OPTS)[0])) == capi.MRP_ERR_ARG
    # a bubble out of range
    assert code(h=dict(h, bv=[0, 1, 2, 3, 5, 6, 8])) == capi.MRP_ERR_ARG
    assert code(h=dict(h, bv=[0, 1, 2, 3, 5, 6, -1])) == capi.MRP_ERR_ARG
    # an entry's read out of range, in either extraction
    for which in ("x", "xf"):
        bad = copy.deepcopy(h[which])
        bad["entries"][1][0] = (len(READS), bad["entries"][1][0][1])
        assert code(h=dict(h, **{which: bad})) == capi.MRP_ERR_ARG, which
    # a fragment that leaves the bubbles
    assert code(gf=fragment(1, 7, [0] * 7, [0] * 7)) == capi.MRP_ERR_ARG
    assert code(gf=fragment(-1, 3, [0] * 3, [0] * 3)) == capi.MRP_ERR_ARG
    # a fragment allele the variant lacks (114 has three alleles, the others two)
    assert code(gf=fragment(0, 7, [0, 1, 2, 2, 1, 0, 1], [1, 0, 1, 0, 1, 1, 0])) == capi.MRP_ERR_ARG
    assert code(gf=fragment(0, 7, [0, 1, 0, 2, 1, 0, 1], [1, 0, 1, 3, 1, 1, 0])) == capi.MRP_ERR_ARG
    # a gt outside the variant's alleles, a state outside 0..3
    assert code(gt=[(0, 2)] + FGT[1:]) == capi.MRP_ERR_ARG
    assert code(state=[4] + FSTATE[1:]) == capi.MRP_ERR_ARG
    assert code(state=[-1] + FSTATE[1:]) == capi.MRP_ERR_ARG


# ---- from the records of three chunks to mrp_phase_sets ------------------------------------------------------------------------------

CORE, MARGIN, N_IDS = 100, 20, 24


def made_up_chunks(seed):
    """three chunks of one contig, cores [100 c, 100 c + 100), each seeing 20 positions of its neighbours; the root entries as the two
    updates leave them: untouched outside the chunk's core, otherwise any of the three states; reads shared across the overlaps"""
    rng = np.random.default_rng(seed)
    chunk_roots, ranges, read_id, pos_tables = [], [], [], []
    for c in range(3):
        lo, hi = CORE * c, CORE * (c + 1)
        nr = 14
        read_id.append(rng.choice(N_IDS, nr, replace=False).astype(np.int32))
        sets = []
        for n, filtered in ((12, False), (6, True)):
            pos = np.sort(rng.integers(max(lo - MARGIN, 0), hi + MARGIN, n))
            pos[1] = pos[0]  # two variants at one position
            roots = []
            for p in pos:
                k = int(rng.integers(2, 4))
                e = vo.root_entry(k, p)
                if lo <= p < hi:
                    state = int(rng.choice([vo.UNTOUCHED, vo.UPDATED, vo.UPDATED, vo.UPDATED, vo.CLEARED]))
                    if state == vo.CLEARED:
                        e.update(gt1=-1, gt2=-1, genotypeProb=vo.NEG_INF, haplotype1Prob=vo.NEG_INF, haplotype2Prob=vo.NEG_INF, state=state)
                    elif state == vo.UPDATED:
                        g1 = int(rng.integers(k))
                        g2 = g1 if rng.random() < 0.2 else int(rng.integers(k))
                        logs = [vo.NEG_INF] * 3 if filtered else [np.float32(-rng.random() * 5) for _ in range(3)]
                        e.update(gt1=g1, gt2=g2, genotypeProb=logs[0], haplotype1Prob=logs[1], haplotype2Prob=logs[2], wasUpdated=True, state=state)
                        tags = rng.choice([0, 1, 2], nr, p=[0.3, 0.35, 0.35])
                        e["hap1Reads"], e["hap2Reads"] = np.flatnonzero(tags == 1).tolist(), np.flatnonzero(tags == 2).tolist()
                        e["alleleIdxToReads"][g1] |= set(e["hap1Reads"])
                        e["alleleIdxToReads"][g2] |= set(e["hap2Reads"])
                roots.append(e)
            sets.append(roots)
        chunk_roots.append(tuple(sets))
        ranges.append((lo, hi))
        pos_tables.append(tuple((np.array([e["pos"] for e in s], np.int64), np.array([len(e["alleleIdxToReads"]) for e in s], np.int32)) for s in sets))
    return chunk_roots, ranges, read_id, pos_tables


@pytest.mark.parametrize("switched", [(0, 0, 0), (0, 1, 0), (1, 0, 1)])
@pytest.mark.parametrize("seed", [3, 4])
def test_variants_from_records_and_phase_sets(seed, switched):
    chunk_roots, ranges, read_id, tables = made_up_chunks(seed)
    records = [vo.records_arrays(p, f) for p, f in chunk_roots]
    got = capi.variants_from_records(records, [t[0][0] for t in tables], [t[0][1] for t in tables], [t[1][0] for t in tables], [t[1][1] for t in tables],
                                     switched, read_id)
    want = vo.contig_variants(copy.deepcopy(chunk_roots), ranges, switched, read_id)
    assert len(got) == len(want) > 10
    assert any(w["gt1"] == w["gt2"] and w["hap1Reads"] and w["hap2Reads"] for w in want)  # a homozygous call: the union of its two lists
    assert any(a["pos"] == b["pos"] for a, b in zip(want, want[1:]))                         # the tie-break is exercised
    for g, w in zip(got, want):
        assert (g["pos"], g["gt1"], g["gt2"], g["chunk"], g["site"]) == (w["pos"], w["gt1"], w["gt2"], w["chunk"], w["site"])
        assert g["alleleIdxToReads"] == [sorted(s) for s in w["alleleIdxToReads"]]
        for k, kw in (("genotype_log_prob", "genotypeProb"), ("hap1_log_prob", "haplotype1Prob"), ("hap2_log_prob", "haplotype2Prob")):
            assert np.float32(g[k]).view(np.uint32) == np.float32(w[kw]).view(np.uint32), k
    if any(switched):
        plain = capi.variants_from_records(records, [t[0][0] for t in tables], [t[0][1] for t in tables], [t[1][0] for t in tables],
                                           [t[1][1] for t in tables], (0, 0, 0), read_id)
        assert any((a["gt1"], a["gt2"]) != (b["gt1"], b["gt2"]) for a, b in zip(got, plain))
        assert all(a["alleleIdxToReads"] == b["alleleIdxToReads"] for a, b in zip(got, plain))  # the lists stay with their allele
    # mrp_phase_sets over the result, unchanged, against the oracle's rules over the oracle's variants
    reasons = {"Same": 0, "NoHet": 1, "MissingConcordancy": 2, "UnlikelyConcordancy": 3, "Discordancy": 4}
    for rules in ((2, 0.05, 0.5), (1, 0.0, 0.3)):
        ps = capi.phase_sets(got, *rules)
        ref = fo.phase_sets(want, *rules)
        assert ps == [(p, reasons[r]) for p, r in ref]
    assert len({p for p, _ in ps}) > 2


def test_variants_from_records_errors():
    chunk_roots, ranges, read_id, tables = made_up_chunks(3)
    records = [vo.records_arrays(p, f) for p, f in chunk_roots]
    args = lambda recs: (recs, [t[0][0] for t in tables], [t[0][1] for t in tables], [t[1][0] for t in tables], [t[1][1] for t in tables], (0, 0, 0), read_id)
    s = int(np.flatnonzero(records[1]["state"] == vo.UPDATED)[0])
    for field, value in (("state", 3), ("gt", 9), ("n_hap1", 99)):
        bad = copy.deepcopy(records)
        bad[1][field].reshape(-1)[2 * s if field == "gt" else s] = value
        with pytest.raises(capi.MrpError) as e:
            capi.variants_from_records(*args(bad))
        assert e.value.code == capi.MRP_ERR_ARG and "chunk 1" in str(e.value), field
    assert capi.variants_from_records([], [], [], [], [], [], []) == []


# ---- the device call's argument checks, without a device ---------------------------------------------------------------------------------

def test_symbols_exported_and_transcribed():
    lib = capi.load()
    for name in ("mrp_variant_records_from_extracted", "mrp_phase_aligned_chunks_with_records", "mrp_variants_from_records"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6  # additions only
    assert C.sizeof(capi.VariantRecords) == 11 * 8 and C.sizeof(capi.RecordVariants) == 7 * 8
    assert C.sizeof(capi.PhaseAlignedRecordsStats) == C.sizeof(capi.PhaseAlignedFilteredStats) + 5 * 8
    assert len(capi.load().mrp_phase_aligned_chunks_with_records.argtypes) == len(capi.load().mrp_phase_aligned_chunks_with_filtered.argtypes) + 1


def test_device_call_errors_in_order():
    chunks, rests = [], []
    for seed in range(2):
        primary, filtered, _ = rc.split_variants(rc.synthetic(seed))
        chunks.append(primary)
        rests.append((filtered, rc.genotypes(filtered, seed)))
    f = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    r, p = f.reverse_complement(), capi.Params.from_reference_names(synth.shipped_phase_params())

    def code_of(*args, **kw):
        with pytest.raises(capi.MrpError) as e:  # (the binding asserts: no output written, filtered_out and records_out zeroed)
            capi.phase_aligned_chunks_with_records(None, *args, **kw)
        return e.value.code, str(e.value)
    # MRP_ERR_ARG first: the call's own null arguments, records_out among them, and with_filtered's checks
    for what in ("records_out", "rest", "filtered_out", "filtered_read_out", "gt[0]", "options", "out", "hap_out", "read_names", "hap_out[0]", "read_names[0][0]"):
        code, msg = code_of(chunks, rests, f, r, p, nulls=(what,))
        assert code == capi.MRP_ERR_ARG and "mrp_phase_aligned_chunks_with_records" in msg, (what, msg)
    assert code_of(chunks, rests, None, r, p)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, rests, f, r, p, expansion=3)[0] == capi.MRP_ERR_ARG
    fl, gt = rests[1]
    g = gt.copy()
    g[0, 0] = len(fl.alleles[0])
    code, msg = code_of(chunks, [rests[0], (fl, g)], f, r, p)
    assert code == capi.MRP_ERR_ARG and "chunk 1" in msg and "filtered variant 0" in msg
    swapped = dataclasses.replace(fl, variant_pos=np.ascontiguousarray(fl.variant_pos[::-1]))
    assert code_of(chunks, [rests[0], (swapped, gt)], f, r, p)[0] == capi.MRP_ERR_ARG
    # then the refused extraction modes, without a context; an argument error of the same call still comes first
    for mode in ("indel_size_for_sv_handling", "use_run_length_encoding"):
        opts = dict(capi.shipped_extract_options(), **{mode: 1})
        assert code_of(chunks, rests, f, r, p, options=opts)[0] == capi.MRP_ERR_UNSUPPORTED
        assert code_of(chunks, rests, f, r, None, options=opts)[0] == capi.MRP_ERR_ARG
        assert code_of(chunks, rests, f, r, p, options=opts, nulls=("records_out",))[0] == capi.MRP_ERR_ARG
    # well-formed: only now is the context looked at
    code, msg = code_of(chunks, rests, f, r, p)
    assert code == capi.MRP_ERR_NO_DEVICE and "no CPU fallback" in msg
    assert code_of([], [], f, r, p)[0] == capi.MRP_ERR_NO_DEVICE
    assert code_of(chunks[:1], [(rc.subset(chunks[0], []), [])], f, r, p)[0] == capi.MRP_ERR_NO_DEVICE  # an empty rest
