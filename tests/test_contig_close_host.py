"""Closing a contig on the host: mrp_final_read_tags, mrp_stitch_values, mrp_close_contig and mrp_close_contigs against the plain-Python
restatement of the reference (tests/contig_oracle.py), on per-chunk results made without a device.  Every comparison is exact: integers,
and floats as bits.  The conditions that keep a test from passing vacuously are asserted on the oracle's side alone."""
import copy
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi
from tests import contig_oracle as co
from tests import variant_records_oracle as vo
from tests.test_variant_records_host import made_up_chunks

RECORD_SEED = 5           # the three made-up chunks of tests/test_variant_records_host.py: 14 reads each out of 24 ids
RULES = (2, 0.3, 0.25)    # with them every reason of a phase set break occurs among the seed's variants (asserted below)
ODD_PHRED = 12.3456006    # as a float 12.34560013; "%f" prints 12.345601, which strtof reads as the next float up, 12.34560108


def name_of(read_id):
    return f"read_{int(read_id):03d}"


def designed_contig(seed=RECORD_SEED, n_chunks=3):
    """the made-up records, and tags made for the stitching: a read's true haplotype is its id's parity; chunk 0 and chunk 2 tag by it,
    chunk 1 the other way round (so it is switched); in every chunk the phasing leaves a few reads untagged, of which the back half tags
    some -- a filtered read among them, whose result lies behind the chunk's reads; one read of chunks 0 and 1 is tagged against the
    others in chunk 1 with the higher score, so it changes sets there; one score is ODD_PHRED"""
    chunk_roots, ranges, read_id, tables = made_up_chunks(seed)
    rng = np.random.default_rng([seed, 41])
    shared01 = sorted(set(read_id[0].tolist()) & set(read_id[1].tolist()))
    assert len(shared01) >= 6
    mover, back_only = shared01[0], shared01[1:4]
    chunks = []
    for c in range(n_chunks):
        ids = read_id[c]
        n = len(ids)
        truth = np.array([1 + int(i) % 2 for i in ids], np.int8)
        hap = truth.copy() if c != 1 else (3 - truth).astype(np.int8)
        phred = np.round(rng.uniform(5.0, 40.0, n), 9)
        filtered_read, read_hap = [], np.zeros(n, np.int32)
        for r, i in enumerate(ids.tolist()):
            if i == mover:
                hap[r] = truth[r] if c == 0 else (truth[r] if c == 1 else hap[r])  # chunk 1: against its chunk's other reads
                phred[r] = 10.0 if c == 0 else 30.0
            elif i in back_only and c <= 1:
                # the phasing leaves it alone; the back half tags it as the chunk's other reads are tagged.  The first of them is a
                # filtered read (its own index holds 0, its result lies at n + k), the second an untagged primary read, the third has no fragment tag at all
                side = int(hap[r])
                hap[r] = (0, 0, -1)[back_only.index(i)]
                if back_only.index(i) == 0:
                    filtered_read.append(r)
                else:
                    read_hap[r] = side
        for r in range(n):  # the phasing's own tags are repeated by the back half's output (include/margin_rphmm.h, mrp_filtered_out)
            if hap[r] in (1, 2):
                read_hap[r] = hap[r]
        # a second filtered read that stays untagged, and one the back half tags, where the chunk has reads to spare
        spare = [r for r, i in enumerate(ids.tolist()) if i != mover and i not in back_only]
        for k, r in enumerate(spare[:2]):
            hap[r], read_hap[r] = (-1, 0)[k], 0
            filtered_read.append(r)
        filtered_read.sort()
        tail = []
        for r in filtered_read:
            i = int(ids[r])
            tail.append((3 - truth[r] if c == 1 else truth[r]) if (i in back_only or r == spare[1]) else 0)
        if c == 0:
            first_tagged = int(np.flatnonzero((hap == 1) | (hap == 2))[1])
            phred[first_tagged] = ODD_PHRED
        prim, filt = chunk_roots[c]
        chunks.append(dict(read_names=[name_of(i) for i in ids], read_id=ids, hap=hap, phred=phred,
                           filtered=dict(read_hap=np.concatenate([read_hap, np.array(tail, np.int32)]), variant_state=np.zeros(len(filt), np.int32)),
                           filtered_read=np.array(filtered_read, np.int32), records=vo.records_arrays(prim, filt),
                           variant_pos=tables[c][0][0], n_alleles=tables[c][0][1], fvariant_pos=tables[c][1][0], fn_alleles=tables[c][1][1],
                           roots=(prim, filt), range=ranges[c]))
    return chunks


def oracle(chunks, **kw):
    return co.close_contig(copy.deepcopy(chunks), **kw)  # (the switching edits the root entries)


@pytest.fixture(scope="module")
def contig():
    return designed_contig()


def test_symbols_exported_and_transcribed():
    lib = capi.load()
    for name in ("mrp_final_read_tags", "mrp_stitch_values", "mrp_close_contig", "mrp_close_contigs", "mrp_contig_out_clear"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and (name == "mrp_contig_out_clear" or getattr(lib, name).argtypes is not None)
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6  # additions only
    assert C.sizeof(capi.ContigChunk) == 14 * 8 and C.sizeof(capi.ContigRules) == 4 * 8 and C.sizeof(capi.ContigOut) == 6 * 8 + C.sizeof(capi.RecordVariants)
    assert callable(capi.final_read_tags) and callable(capi.stitch_values) and callable(capi.close_contig) and callable(capi.close_contigs)


def test_the_inputs_are_what_the_docstrings_say(contig):
    """decided by the oracle alone"""
    want = oracle(contig, rules=RULES)
    assert want["switched"] == [0, 1, 0]                                                    # at least one chunk is switched
    only_back = [(c, r) for c, ch in enumerate(contig) for r, t in enumerate(co.final_tags(ch)) if t in (1, 2) and ch["hap"][r] not in (1, 2)]
    assert any(r in contig[c]["filtered_read"] for c, r in only_back) and any(r not in contig[c]["filtered_read"] for c, r in only_back)
    primary = oracle(contig, rules=RULES, primary_reads_only=True)
    assert primary["counts"] != want["counts"]                                              # ... a read only the back half tagged counts in one of them
    assert sum(primary["counts"][1]) < sum(want["counts"][1])
    assert np.float32(co.printed(ODD_PHRED)).view(np.uint32) != np.float32(ODD_PHRED).view(np.uint32)  # "%f" changes the float
    assert any(ODD_PHRED in ch["phred"][np.isin(ch["hap"], (1, 2))] for ch in contig)
    assert want["moved"]                                                                    # addToHapReadsSeen moves a read of two chunks
    assert {why for _, why in want["phase_sets"]} == {0, 1, 2, 3, 4}                        # a phase set break of every reason
    assert any(len(ch["filtered_read"]) > 0 and (ch["filtered"]["read_hap"][len(ch["read_names"]):] > 0).any() for ch in contig)


@pytest.mark.parametrize("primary_reads_only", [False, True])
@pytest.mark.parametrize("prevent_switching", [False, True])
def test_close_contig_equals_the_oracle(contig, primary_reads_only, prevent_switching):
    kw = dict(primary_reads_only=primary_reads_only, prevent_switching=prevent_switching, rules=RULES)
    want = oracle(contig, **kw)
    got = capi.close_contig(contig, **kw)
    co.assert_closed_equal(got, want, str(kw))
    if prevent_switching:
        assert got["switched"] == [0, 0, 0]
        if not primary_reads_only:  # it would have switched (among the primary reads alone chunk 1 is a tie, which never switches)
            assert sum(want["counts"][1][:2]) < sum(want["counts"][1][2:])
    # the same name in two chunks gets the same final tag
    seen = {}
    for ch, fh in zip(contig, got["final_hap"]):
        for nm, h in zip(ch["read_names"], fh):
            assert seen.setdefault(nm, int(h)) == int(h)
    assert {1, 2} <= set(seen.values())


def test_tags_and_values_per_chunk(contig):
    for c, ch in enumerate(contig):
        tags = capi.final_read_tags(ch["hap"], ch["filtered"], ch["filtered_read"])
        assert tags.tolist() == co.final_tags(ch), c
        values = capi.stitch_values(ch["hap"], ch["phred"], tags)
        l1, l2 = co.partition_lines(ch)
        for r, nm in enumerate(ch["read_names"]):
            want = l1.get(nm, l2.get(nm, 0.0))
            assert np.float64(values[r]).view(np.uint64) == np.float64(want).view(np.uint64), (c, r, values[r], want)
        assert (values[(tags > 0) & ~np.isin(ch["hap"], (1, 2))] == -1.0).all() and (values[tags == 0] == 0.0).all()
    # scores "%f" and strtof take apart: large, tiny, negative (a read of the wrong side), zero
    phred = np.array([ODD_PHRED, 1234567.891, 1e-7, -0.25, 0.0, 99.9999995, 3.0000001], np.float64)
    hap = np.array([1, 2, 1, 2, 1, 2, 0], np.int8)
    got = capi.stitch_values(hap, phred, np.array([1, 2, 1, 2, 1, 2, 2], np.int8))
    assert got[:6].tolist() == [co.printed(p) for p in phred[:6]] and got[6] == -1.0
    assert got[0] != ODD_PHRED and got[2] == 0.0 and got[5] == 100.0


def test_the_haplotag_form(contig):
    """tagFromPhasedVcf.c: no fragment, every value -1.0, switching prevented"""
    chunks = [dict(read_names=ch["read_names"], read_id=ch["read_id"], hap=np.where(ch["hap"] == 0, -1, ch["hap"]).astype(np.int8), phred=None, filtered=None)
              for ch in contig]
    assert capi.final_read_tags(chunks[0]["hap"]).tolist() == [max(int(h), 0) for h in chunks[0]["hap"]]
    assert set(capi.stitch_values(None, None, capi.final_read_tags(chunks[0]["hap"])).tolist()) == {-1.0, 0.0}
    for kw in (dict(prevent_switching=True), dict(prevent_switching=True, primary_reads_only=True), dict()):
        want = oracle(chunks, **kw)
        got = capi.close_contig(chunks, **kw)
        co.assert_closed_equal(got, want, str(kw))
        assert got["variants"] == [] and got["phase_sets"] == []
    assert capi.close_contig(chunks, prevent_switching=True)["switched"] == [0, 0, 0]
    assert capi.close_contig(chunks, prevent_switching=True, primary_reads_only=True)["counts"][1] == (0, 0, 0, 0)  # every value is negative


def test_edges(contig):
    # a one-chunk contig; no chunk at all
    co.assert_closed_equal(capi.close_contig(contig[:1], rules=RULES), oracle(contig[:1], rules=RULES), "one chunk")
    none = capi.close_contig([], rules=RULES)
    assert none == dict(switched=[], counts=[], variants=[], phase_sets=[], final_hap=[])
    # a chunk without reads in the middle: its records still count
    empty = dict(contig[1], read_names=[], read_id=np.zeros(0, np.int32), hap=np.zeros(0, np.int8), phred=np.zeros(0),
                 filtered=dict(read_hap=np.zeros(0, np.int32), variant_state=contig[1]["filtered"]["variant_state"]), filtered_read=np.zeros(0, np.int32))
    prim, filt = copy.deepcopy(empty["roots"])
    for e in prim + filt:
        e["hap1Reads"], e["hap2Reads"], e["alleleIdxToReads"] = [], [], [set() for _ in e["alleleIdxToReads"]]
    empty.update(records=vo.records_arrays(prim, filt), roots=(prim, filt))
    chunks = [contig[0], empty, contig[2]]
    want = oracle(chunks, rules=RULES)
    got = capi.close_contig(chunks, rules=RULES)
    co.assert_closed_equal(got, want, "a chunk without reads")
    assert got["counts"][1] == (0, 0, 0, 0) and got["final_hap"][1].size == 0 and any(v["chunk"] == 1 for v in got["variants"])
    # records == NULL: the stitching alone
    bare = [{k: v for k, v in ch.items() if k not in ("records", "roots")} for ch in contig]
    got = capi.close_contig(bare, rules=RULES)
    co.assert_closed_equal(got, oracle(bare, rules=RULES), "no records")
    assert got["variants"] == [] and got["phase_sets"] == [] and got["switched"] == [0, 1, 0]


@pytest.mark.parametrize("threads", [1, 4])
def test_two_contigs_each_equal_to_its_own_close(contig, threads):
    second = designed_contig(seed=4)
    contigs = [contig, second[:2], [], second]
    lib = capi.load()
    try:
        lib.mrp_set_host_threads(threads)
        got = capi.close_contigs(contigs, rules=RULES, primary_reads_only=True)
    finally:
        lib.mrp_set_host_threads(16)
    assert len(got) == 4
    for k, chunks in enumerate(contigs):
        alone = capi.close_contig(chunks, rules=RULES, primary_reads_only=True)
        want = oracle(chunks, rules=RULES, primary_reads_only=True)
        co.assert_closed_equal(got[k], want, f"contig {k}")
        co.assert_closed_equal(alone, want, f"contig {k} alone")
        assert got[k]["switched"] == alone["switched"] and got[k]["phase_sets"] == alone["phase_sets"]


def test_every_argument_error_leaves_the_output_unwritten(contig):
    def code(call, *args, **kw):
        with pytest.raises(capi.MrpError) as e:  # (the bindings assert that nothing was written)
            call(*args, **kw)
        return e.value.code
    ch = contig[0]
    n = len(ch["read_names"])
    hap, F, fr = ch["hap"], ch["filtered"], ch["filtered_read"]
    # ---- mrp_final_read_tags
    assert code(capi.final_read_tags, hap, F, fr, nulls=("hap",)) == capi.MRP_ERR_ARG
    assert code(capi.final_read_tags, hap, F, fr, nulls=("out",)) == capi.MRP_ERR_ARG
    for bad in (3, -2):
        h = hap.copy()
        h[2] = bad
        assert code(capi.final_read_tags, h, F, fr) == capi.MRP_ERR_ARG
        assert code(capi.final_read_tags, h) == capi.MRP_ERR_ARG
    for bad in (3, -1):
        rh = F["read_hap"].copy()
        rh[-1] = bad
        assert code(capi.final_read_tags, hap, dict(F, read_hap=rh), fr) == capi.MRP_ERR_ARG
    assert code(capi.final_read_tags, hap, dict(F, read_hap=F["read_hap"][:-1]), fr) == capi.MRP_ERR_ARG   # fewer entries than reads + filtered reads
    assert code(capi.final_read_tags, hap, F, fr[:-1]) == capi.MRP_ERR_ARG
    assert code(capi.final_read_tags, hap, F, np.concatenate([fr[:-1], [n]])) == capi.MRP_ERR_ARG           # a filtered read outside the chunk
    assert code(capi.final_read_tags, hap, F, np.concatenate([fr[:-1], fr[:1]])) == capi.MRP_ERR_ARG        # ... named twice
    # ---- mrp_stitch_values
    tags = capi.final_read_tags(hap, F, fr)
    for what in ("phred", "final_tag", "out"):
        assert code(capi.stitch_values, hap, ch["phred"], tags, nulls=(what,)) == capi.MRP_ERR_ARG, what
    t = tags.copy()
    t[0] = 3
    assert code(capi.stitch_values, hap, ch["phred"], t) == capi.MRP_ERR_ARG
    t = tags.copy()
    r = int(np.flatnonzero(hap == 1)[0])
    t[r] = 2  # the phasing's tag with another final tag
    assert code(capi.stitch_values, hap, ch["phred"], t) == capi.MRP_ERR_ARG
    # ---- mrp_close_contig / mrp_close_contigs
    for one in (True, False):
        for what in ("chunks", "rules", "out", "read_names", "read_names[0]", "hap", "phred", "read_id", "variant_pos", "n_alleles", "fvariant_pos", "fn_alleles"):
            assert code(capi.close_contigs, [contig], one=one, nulls=(what,)) == capi.MRP_ERR_ARG, (one, what)
        edits = [("hap", lambda c: c["hap"].__setitem__(1, 5)),                                  # a tag outside its range
                 ("read_hap", lambda c: c["filtered"]["read_hap"].__setitem__(0, 7)),
                 ("state", lambda c: c["records"]["state"].__setitem__(0, 3)),                    # a record state outside its range
                 ("sites", lambda c: c.__setitem__("variant_pos", c["variant_pos"][:-1])),        # records and position arrays disagree
                 ("fsites", lambda c: c.__setitem__("fn_alleles", np.append(c["fn_alleles"], 2)) or c.__setitem__("fvariant_pos", np.append(c["fvariant_pos"], 1)))]
        for what, edit in edits:
            bad = copy.deepcopy(contig)
            edit(bad[1])
            assert code(capi.close_contigs, [bad], one=one) == capi.MRP_ERR_ARG, (one, what)
            if not one:  # a bad contig behind a good one: nothing of the good one is handed over
                assert code(capi.close_contigs, [contig, bad]) == capi.MRP_ERR_ARG, what
    assert code(capi.close_contigs, [contig], nulls=("first_chunk",)) == capi.MRP_ERR_ARG
    lib = capi.load()
    first = np.array([0, 2, 1, 3], np.int64)  # a contig that ends before it starts
    built = [capi.contig_chunk_struct(c) for c in contig]
    arr = (capi.ContigChunk * 3)(*[b[0] for b in built])
    outs = (capi.ContigOut * 3)()
    rules = capi.ContigRules(0, 0, 2, 0.05, 0.5)
    assert lib.mrp_close_contigs(3, first.ctypes.data, arr, C.byref(rules), outs) == capi.MRP_ERR_ARG and bytes(outs) == bytes((capi.ContigOut * 3)())
    first[0] = 1
    assert lib.mrp_close_contigs(1, first.ctypes.data, arr, C.byref(rules), outs) == capi.MRP_ERR_ARG
    assert lib.mrp_close_contig(-1, arr, C.byref(rules), outs) == capi.MRP_ERR_ARG
