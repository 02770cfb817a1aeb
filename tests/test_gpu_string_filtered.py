"""mrp_phase_string_chunks_with_filtered on the device: the back half of the chunk loop (filtered variants phased with the tagged
primary reads, filtered and untagged primary reads haplotagged against the fragment's alleles) inside the string-chunk call,
against the chain of the existing calls (tests/string_filtered_cases.py) -- decisions identical, totals bit for bit: the pair-HMM
results are the same numbers and the sums run over the same fp64 operations in the same order."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi
from tests import haptag_oracle as ho
from tests import string_filtered_cases as sf
from tests.test_gpu_string_chunks import models, params
from tests.test_gpu_string_queue import assert_identical

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(gpu_ctx):
    f, r = models()
    chunks, rests = sf.filtered_chunks(26)
    p = params()
    front, back = sf.chain(gpu_ctx, chunks, rests, f, r, p)
    return dict(f=f, r=r, p=p, chunks=chunks, rests=rests, front=front, back=back)


def classes_of(entries):
    out = {}
    for pos, (q, sub) in enumerate(entries):
        out.setdefault(bytes(np.asarray(sub, np.uint8)), []).append((pos, q))
    return out


def test_the_inputs_make_the_owner_rules_bite(case):
    """every special case the comparison below is meant to cover occurs in the input"""
    chunks, rests, front, back = case["chunks"], case["rests"], case["front"], case["back"]
    assert len(chunks) >= 24 and sum(r is None for r in rests) >= 1 and any(r is None and c.bubbles for c, r in zip(chunks, rests))
    owner_differs = untagged_owner = not_01 = hom_site = sv_bubble = sv_variant = no_tagged = 0
    for c, rest, g, b in zip(chunks, rests, front, back):
        if rest is None:
            continue
        n_primary = len(c.read_names)
        strands = np.concatenate([c.read_forward_strand, rest["forward_strand"]])
        res = g["result"]
        for j, (alleles, cmp_, entries) in enumerate(b["psites"]):
            bub = c.bubbles[int(res["ref_start"]) + j]
            if cmp_[0] == cmp_[1]:
                hom_site += bool(entries)
                continue
            if len(alleles) > 2 and set(cmp_) != {0, 1}:
                not_01 += bool(entries)
            if max(len(a) for a in alleles) > 512 and entries:
                sv_bubble += 1
            first_primary = {}  # the front's rule: the first-listed primary substring of the bubble owns
            for q, sub in zip(bub[1], bub[2]):
                first_primary.setdefault(bytes(np.asarray(sub, np.uint8)), q)
            for key, members in classes_of(entries).items():
                last = members[-1][1]
                if len({bool(strands[q]) for _pos, q in members}) == 2 and key in first_primary and strands[first_primary[key]] != strands[last]:
                    owner_differs += 1
                if len(members) >= 2 and last < n_primary:  # (a primary read is listed only when the phasing left it untagged)
                    untagged_owner += 1
        for (alleles, gt, entries), state in zip(rest["variants"], b["variant_state"]):
            if gt[0] != gt[1] and entries and not any(b["tagged"][q] for q, _ in entries):
                assert state == ho.TIE
                no_tagged += 1
            if max(len(a) for a in alleles) > 512 and gt[0] != gt[1] and any(b["tagged"][q] for q, _ in entries):
                sv_variant += 1
    print(dict(owner_differs=owner_differs, untagged_owner=untagged_owner, not_01=not_01, hom_site=hom_site, sv_bubble=sv_bubble, sv_variant=sv_variant,
               no_tagged=no_tagged))
    assert owner_differs >= 3 and untagged_owner >= 3 and not_01 >= 3 and hom_site >= 3 and sv_bubble >= 1 and sv_variant >= 1 and no_tagged >= 3
    states = np.concatenate([b["variant_state"] for b in back])
    assert {int(x) for x in states} == {ho.NOT_VISITED, ho.CIS, ho.TRANS, ho.TIE}
    haps = np.concatenate([b["read_hap"][len(c.read_names):] for c, r, b in zip(chunks, rests, back) if r is not None])
    assert (haps == 1).sum() > 50 and (haps == 2).sum() > 50
    untagged = sum(int((b["tagged"][:len(c.read_names)] == 0).sum()) for c, b in zip(chunks, back))
    assert untagged > 20
    for b in back:
        ho.assert_margins_decisive(b["h1"], b["h2"], "partition")
        ho.assert_margins_decisive(b["cis"], b["trans"], "phasing")


def test_one_call_equals_the_chain(gpu_ctx, case):
    f, r, p, chunks, rests = case["f"], case["r"], case["p"], case["chunks"], case["rests"]
    got, st = capi.phase_string_chunks_with_filtered(gpu_ctx, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED, profiles=True)
    assert_identical(got, case["front"], chunks)  # every array of mrp_phase_string_chunks: as without a rest
    sf.assert_back_identical(got, case["back"])
    _, plain = capi.phase_string_chunks(gpu_ctx, chunks, f, r, p, min_phred=sf.MIN_PHRED)
    n_plain = plain.pairhmm.pairs_lane + plain.pairhmm.pairs_wave
    assert st.pairs_scored == st.chunks.pairhmm.pairs_lane + st.chunks.pairhmm.pairs_wave == n_plain + st.pairs_speculative
    assert 0 < st.pairs_read_by_results <= st.pairs_speculative and st.filtered_ms > 0
    print(dict(pairs_scored=st.pairs_scored, speculative=st.pairs_speculative, read=st.pairs_read_by_results, filtered_ms=st.filtered_ms))


def test_anchoring_differs_between_the_two_halves(gpu_ctx, case):
    """an SV-length pair is anchored when variants are phased and not when reads are partitioned: the call equals the chain with the
    shipped threshold and with the threshold out of reach, and between the two the variants' totals at the long alleles move"""
    f, r, p = case["f"], case["r"], case["p"]
    idx = [i for i, (c, rest) in enumerate(zip(case["chunks"], case["rests"])) if rest is not None and any(max(len(a) for a in al) > 512 for al, _g, _e in rest["variants"])]
    assert idx
    chunks, rests = [case["chunks"][i] for i in idx], [case["rests"][i] for i in idx]
    a, _ = capi.phase_string_chunks_with_filtered(gpu_ctx, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED)
    sf.assert_back_identical(a, [case["back"][i] for i in idx])
    moved = 0
    front, back = sf.chain(gpu_ctx, chunks, rests, f, r, p, sv_threshold=10 ** 6)
    b, _ = capi.phase_string_chunks_with_filtered(gpu_ctx, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED, sv_threshold=10 ** 6)
    sf.assert_back_identical(b, back)
    for x, y, rest in zip(a, b, rests):
        for v, (al, g, e) in enumerate(rest["variants"]):
            if max(len(s) for s in al) > 512 and x["filtered"]["variant_state"][v] != ho.NOT_VISITED and x["filtered"]["cis"][v] != 0:
                moved += x["filtered"]["cis"][v] != y["filtered"]["cis"][v]
    assert moved >= 1


def test_through_the_queue(gpu_ctx, case):
    f, r, p, chunks, rests = case["f"], case["r"], case["p"], case["chunks"], case["rests"]
    ref, _ = capi.phase_string_chunks_with_filtered(gpu_ctx, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED, profiles=True)
    q = capi.Queue([0, 0])
    try:
        for per_batch in (1, 5, len(chunks)):
            got, st = capi.queue_phase_string_chunks_with_filtered(q, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED, chunks_per_batch=per_batch, profiles=True)
            assert_identical(got, ref, chunks)
            sf.assert_back_identical(got, [g["filtered"] for g in ref])
            assert st.batches == -(-len(chunks) // per_batch) and sum(st.chunks_per_device[:2]) == len(chunks)
    finally:
        q.close()
    got, st = capi.phase_string_chunks_with_filtered_on_devices([0], chunks[:7], rests[:7], f, r, p, min_phred=sf.MIN_PHRED, chunks_per_batch=3)
    sf.assert_back_identical(got, [g["filtered"] for g in ref[:7]])
    assert st.batches == 3


def test_a_lane_error_leaves_the_outputs_zeroed_and_the_queue_usable(gpu_ctx, case):
    """the refusal is injected (mrp_context_set_test_hooks bit 2: the device's next allocation of at least 1 MB is refused once): with
    every chunk in one batch that is the batch's symbol pool, before anything is launched"""
    f, r, p, chunks, rests = case["f"], case["r"], case["p"], case["chunks"], case["rests"]
    L = capi.load()
    ref, _ = capi.phase_string_chunks_with_filtered(gpu_ctx, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED)
    q = capi.Queue([0, 0])
    try:
        a = capi.StringFilteredArgs(chunks, rests, True)
        symbols = sum(b[1]["pool"].size for b in a.built + a.rbuilt if "pool" in b[1])
        assert symbols > 3 << 19  # 1.5 MB in the batch's one pool: its size class is above the hook's 1 MB
        st = capi.QueueStats()
        gpu_ctx.set_test_hooks(4)
        try:
            rc = L.mrp_queue_phase_string_chunks_with_filtered(q.h, a.n, a.arr, a.rarr, C.byref(f), C.byref(r), 4, 512, 0.0, C.byref(p), sf.MIN_PHRED,
                                                               len(chunks), a.res, a.hp, a.pp, a.prof, a.fout, C.byref(st))
        finally:
            gpu_ctx.set_test_hooks(0)
        assert rc != capi.MRP_OK
        assert all(not a.res[i] for i in range(a.n)) and all(not P.pool and not P.seqs for P in a.prof)
        for O in a.fout:
            assert O.n_reads == 0 and O.n_variants == 0 and not O.read_hap and not O.h1 and not O.h2 and not O.variant_state and not O.cis and not O.trans
        got, _ = capi.queue_phase_string_chunks_with_filtered(q, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED, chunks_per_batch=5)
        sf.assert_back_identical(got, [g["filtered"] for g in ref])
    finally:
        q.close()


def test_a_call_without_pairs(gpu_ctx):
    """no substring at any bubble and the one filtered variant homozygous: nothing is scored, the back half's kernels run over
    records that are all dead -- the filtered read stays untagged, the variant is not visited, as in the chain"""
    from margin_amd import synth
    f, r = models()
    p = params()
    chunks = sf.no_pair_chunks()
    rng = np.random.default_rng(13)
    allele = synth.random_sequence(rng, 25)
    filtered_read = len(chunks[1].read_names)  # the rest's only read, behind the chunk's primary ones
    rest = dict(forward_strand=np.ones(1, np.uint8), fsubs=[[], []], variants=[([allele, allele[::-1].copy()], (1, 1), [(filtered_read, allele.copy())])])
    rests = [None, rest]
    got, st = capi.phase_string_chunks_with_filtered(gpu_ctx, chunks, rests, f, r, p, min_phred=sf.MIN_PHRED, profiles=True)
    front, back = sf.chain(gpu_ctx, chunks, rests, f, r, p)
    assert st.pairs_scored == 0 and st.pairs_speculative == 0 and st.pairs_read_by_results == 0
    assert all((g["hap"] == -1).all() for g in got)
    assert_identical(got, front, chunks)
    sf.assert_back_identical(got, back)
    o = got[1]["filtered"]
    assert o["read_hap"].tolist() == [0, 0, 0] and (o["h1"] == 0).all() and (o["h2"] == 0).all()
    assert o["variant_state"].tolist() == [ho.NOT_VISITED] and o["cis"].tolist() == [0.0] and o["trans"].tolist() == [0.0]


def test_oversize_unanchored_pair_of_the_back_half_is_refused(gpu_ctx):
    """a primary substring and an allele beyond the diagonal limit, anchored by the front: with a rest the partition may align them
    unanchored, so the call refuses; with an empty rest it goes through"""
    from margin_amd import synth
    f, r = models()
    rng = np.random.default_rng(8)
    big = synth.random_sequence(rng, 2100)
    alt = big.copy()
    alt[1000] = (alt[1000] + 1) % 4
    chunk = synth.StringChunk(bubbles=[([big, alt], [0], [big.copy()])], read_names=["long"], read_forward_strand=np.ones(1, np.uint8),
                              hap=np.zeros(1, int), truth=[0])
    p = params()
    got, _ = capi.phase_string_chunks_with_filtered(gpu_ctx, [chunk], [None], f, r, p)
    assert got[0]["filtered"]["read_hap"].shape == (1,)
    rest = dict(forward_strand=np.ones(1, np.uint8), fsubs=[[(0, synth.random_sequence(rng, 30))]], variants=[])
    with pytest.raises(capi.MrpError) as e:
        capi.phase_string_chunks_with_filtered(gpu_ctx, [chunk], [rest], f, r, p)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED
    q = capi.Queue([0])
    try:
        with pytest.raises(capi.MrpError) as e:
            capi.queue_phase_string_chunks_with_filtered(q, [chunk], [rest], f, r, p)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "2101 cells" in str(e.value)
    finally:
        q.close()
