"""The work queue over aligned chunks with the phased variant records (mrp_queue_phase_aligned_chunks_with_records and its *_on_devices
form), and a contig from the queue through mrp_close_contig.  At every chunk's own position the queue returns, bit for bit and records
array for array, what ONE mrp_phase_aligned_chunks_with_records call over all chunks returns -- whatever the batch size, the lanes, or
which worker took which batch.  A chunk's kernels see the same operands in whatever batch it travels, so there is no tolerance anywhere in
this file.  Two workers share device 0 (the device listed twice), as in tests/test_gpu_aligned_queue.py."""
import numpy as np
import pytest

from margin_amd import capi
from tests import contig_oracle as co
from tests import extract_cases as ec
from tests import rest_cases as rc
from tests import string_filtered_cases as sf
from tests import sv_split_cases as svc
from tests import test_gpu_phase_aligned as pa
from tests import test_gpu_variant_records as vr
from tests import variant_records_oracle as vo
from tests.test_aligned_queue_args import built
from tests.test_aligned_records_queue_args import RecordsCall
from tests.test_gpu_aligned_queue import check_stats, units_of
from tests.test_gpu_downsample import DEPTH, SEED
from tests.test_gpu_phase_aligned_filtered import synthetic  # noqa: F401  (the six 8 kb / 8x chunks and their rests)

pytestmark = pytest.mark.gpu

MIN_PHRED = sf.MIN_PHRED
OPTS = capi.shipped_extract_options()


def one_call(ctx, chunks, rests, keeps=None, options=OPTS, min_phred=MIN_PHRED):
    f, r = pa.models()
    return capi.phase_aligned_chunks_with_records(ctx, chunks, rests, f, r, pa.params(), options=options, keeps=keeps, profiles=True, min_phred=min_phred)


def queued(q, chunks, rests, per_batch, keeps=None, options=OPTS, min_phred=MIN_PHRED):
    f, r = pa.models()
    return q.phase_aligned_chunks_with_records(chunks, rests, f, r, pa.params(), options=options, keeps=keeps, profiles=True, min_phred=min_phred,
                                               chunks_per_batch=per_batch)


def check_records_stats(rs, got, one=None):
    """the sums over the batches are the one call's: a site, a list and a downloaded slot belong to one chunk"""
    recs = [g["records"] for g in got]
    assert rs.records_sites == sum(len(R["state"]) for R in recs)
    assert rs.records_updated == sum(int((R["state"] == capi.RECORD_UPDATED).sum()) for R in recs)
    assert rs.reads_listed == sum(len(R["reads"]) for R in recs)
    assert rs.records_bytes_downloaded >= 20 * rs.records_sites + 4 * rs.reads_listed and (rs.records_sites == 0 or rs.records_ms > 0)
    if one is not None:
        assert (rs.records_sites, rs.records_updated, rs.reads_listed, rs.records_bytes_downloaded) == \
            (one.records_sites, one.records_updated, one.reads_listed, one.records_bytes_downloaded)


def test_parity_across_batchings(gpu_ctx, synthetic):  # noqa: F811
    chunks, rests = synthetic
    hand = {name: (rc.split_hand(ch, fidx), gt) for name, ch, fidx, gt, _keep in rc.hand_cases()}
    (e_primary, e_filtered), e_gt = hand["empty"]
    nothing = ec.make([], [(100, "20M", 60, 0)])
    b_primary, b_rest, b_keep = vr.boundary_chunk()
    # the six chunks, chunk 1 again (a tie in the cost order), a chunk with an empty rest, a chunk without variants, and the chunk of the
    # wave and pass boundaries three times: it costs more than any other and ties keep the input order, so its last copy is third in the
    # cost order -- third of the first batch of four, second of device 0's batch when the queue deals a short queue out in stripes
    cs = list(chunks) + [chunks[1], e_primary, nothing] + [b_primary] * 3
    rs = list(rests) + [rests[1], (e_filtered, e_gt), (nothing, [])] + [b_rest] * 3
    keeps = [None] * 9 + [b_keep] * 3
    keeps[4] = (np.random.default_rng(4).random(len(chunks[4].read_pos)) < 0.8).astype(np.uint8)
    units = units_of(cs, rs)
    order, batch = capi.queue_plan(units, 4)
    assert order[:3].tolist() == [9, 10, 11] and batch[11] == batch[9] == 0 and units[6] == units[1] > 0 and units[8] == 0
    ref, rst = one_call(gpu_ctx, cs, rs, keeps)
    # ---- conditions on the inputs, decided by the one call alone
    states = np.concatenate([w["filtered"]["variant_state"] for w in ref])
    assert (states == capi.VARIANT_CIS).any() and (states == capi.VARIANT_TRANS).any() and (states == capi.VARIANT_NOT_VISITED).any()
    assert rst.filtered.filtered_reads > 0 and rst.filtered.aligned.chunks.phase.resident == 1
    B = ref[11]["records"]
    assert ((B["state"] == capi.RECORD_UPDATED) & (B["n_hap1"] + B["n_hap2"] > 64)).any()  # a site past one 64-entry pass
    assert all((w["records"]["state"] == capi.RECORD_UPDATED).any() for w in ref[:7]) and ref[8]["records"]["state"].size == 0
    q = capi.Queue([0, 0])
    try:
        for per_batch in (1, 4, 0):
            got, st = queued(q, cs, rs, per_batch, keeps)
            vr.assert_identical(got, ref, f"chunks_per_batch {per_batch}")
            check_stats(st, units, per_batch)
            check_records_stats(st.records, got, rst)
    finally:
        q.close()


def test_downsampling_on_the_queue(synthetic):  # noqa: F811
    chunks, rests = synthetic
    chunks, rests = chunks[:4], rests[:4]
    ctx = capi.Context(0)
    q = capi.Queue([0])
    try:
        ctx.set_downsampling(DEPTH, SEED)
        q.set_downsampling(DEPTH, SEED)
        ref, rst = one_call(ctx, chunks, rests)
        assert ctx.last_downsampling().reads_discarded > 0
        got, st = queued(q, chunks, rests, 2)
        vr.assert_identical(got, ref, "downsampling")
        assert st.batches == 2
        check_records_stats(st.records, got, rst)
    finally:
        q.close()
        ctx.close()


def test_sv_split_on_the_queue():
    """the SV case of tests/test_gpu_variant_records.py::test_sv_split, twice: one chunk per batch"""
    primary, filtered, _ = rc.split_variants(svc.synthetic(0))
    assert primary.is_sv.any() and not primary.is_sv.all()
    chunks, rests = [primary, primary], [(filtered, rc.genotypes(filtered, 0))] * 2
    ctx = capi.Context(0)
    q = capi.Queue([0, 0])
    try:
        with pytest.raises(capi.MrpError) as e:  # off: refused before a lane starts, nothing written (the binding asserts it)
            queued(q, chunks, rests, 1, options=svc.OPTS)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED
        ctx.set_sv_split(1)
        q.set_sv_split(1)
        ref, rst = one_call(ctx, chunks, rests, options=svc.OPTS)
        assert (ref[0]["records"]["state"] == capi.RECORD_UPDATED).any() and len(ref[0]["records"]["reads"]) > 0
        got, st = queued(q, chunks, rests, 1, options=svc.OPTS)
        vr.assert_identical(got, ref, "sv split")
        assert st.batches == 2
        check_records_stats(st.records, got, rst)
    finally:
        q.close()
        ctx.close()


def test_the_one_device_form(gpu_ctx, synthetic):  # noqa: F811
    chunks, rests = synthetic
    chunks, rests = chunks[:4], rests[:4]
    f, r = pa.models()
    p = pa.params()
    keeps = [None, (np.random.default_rng(8).random(len(chunks[1].read_pos)) < 0.7).astype(np.uint8), None, None]
    ref, rst = one_call(gpu_ctx, chunks, rests, keeps)
    got, st = capi.phase_aligned_chunks_with_records_on_devices([0], chunks, rests, f, r, p, options=OPTS, keeps=keeps, profiles=True, min_phred=MIN_PHRED,
                                                                chunks_per_batch=3)
    vr.assert_identical(got, ref, "on_devices")
    check_stats(st, units_of(chunks, rests), 3, n_devices=1)
    check_records_stats(st.records, got, rst)
    with pytest.raises(capi.MrpError) as e:  # a device that does not exist
        capi.phase_aligned_chunks_with_records_on_devices([99], chunks[:1], rests[:1], f, r, p, options=OPTS)
    assert e.value.code == capi.MRP_ERR_ARG
    # no chunk: MRP_OK, zeroed stats
    none, nst = capi.phase_aligned_chunks_with_records_on_devices([0], [], [], f, r, p, options=OPTS)
    assert none == [] and nst.batches == 0 and nst.n_devices == 1 and sum(nst.chunks_per_device) == 0
    assert bytes(nst.records) == bytes(capi.QueueRecordsStats())


def test_diagonal_refusal_inside_a_lane(gpu_ctx, synthetic):  # noqa: F811
    """the 2 048-cell refusal is a lane's error (an error code, no device fault): the records handed out by the batches that were done are
    released, records_out comes back zeroed, and the queue then gives the right answer for the good chunks"""
    chunks, rests = synthetic
    long_chunk = pa.long_window_chunk()
    good, good_rests = list(chunks[:4]), list(rests[:4])
    cs = good[:2] + [long_chunk] + good[2:]
    rs = good_rests[:2] + [(rc.subset(long_chunk, []), [])] + good_rests[2:]
    wide = dict(OPTS, expansion_sv=2_200)
    q = capi.Queue([0, 0])
    try:
        structs, rest_structs = built(cs, rs)
        call = RecordsCall(cs, structs, rest_structs, options=wide)
        call.sv_threshold, call.per_batch = 100_000, 1  # unanchored (sv_threshold above the lengths): a diagonal beyond 2 048 cells
        rc_ = call.run("queue", q=q.h)
        assert rc_ == capi.MRP_ERR_UNSUPPORTED and b"diagonal" in capi.load().mrp_last_error()
        n = len(cs)
        assert all(not call.res[i] and not call.bv[i] and not call.fr[i] for i in range(n))
        assert bytes(call.prof) == bytes((capi.ProfileOut * n)()) and bytes(call.fout) == bytes((capi.FilteredOut * n)())
        assert bytes(call.recs) == bytes((capi.VariantRecords * n)()) and bytes(call.rstats) == bytes(capi.QueueRecordsStats())
        assert call.stats.batches == n
        # the queue stays usable
        got, st = queued(q, good, good_rests, 1)
        ref, rst = one_call(gpu_ctx, good, good_rests)
        vr.assert_identical(got, ref, "after the refusal")
        assert st.batches == 4
        check_records_stats(st.records, got, rst)
    finally:
        q.close()


def contig_chunks(results, chunks, rests, ids):
    """the chunk dicts capi.close_contig and tests/contig_oracle.py take, from per-chunk results of the one call's layout"""
    na = lambda c: np.array([len(a) for a in c.alleles], np.int32)
    return [dict(read_names=list(c.read_names), read_id=ids[i], hap=d["hap"], phred=d["phred"], filtered=d["filtered"], filtered_read=d["filtered_read"],
                 records=d.get("records"), variant_pos=c.variant_pos, n_alleles=na(c), fvariant_pos=fl.variant_pos, fn_alleles=na(fl), range=vr.CORES[i])
            for i, (d, c, (fl, _)) in enumerate(zip(results, chunks, rests))]


def test_a_contig_from_the_queue_to_phase_sets_and_final_tags(gpu_ctx):
    chunks, rests, ids = vr.contig(vr.CONTIG_SEED)
    rules = (2, 0.05, 0.5)
    # ---- the queue, one chunk per batch -> mrp_close_contig
    q = capi.Queue([0, 0])
    try:
        got, st = queued(q, chunks, rests, 1)
    finally:
        q.close()
    assert st.batches == 3
    closed = capi.close_contig(contig_chunks(got, chunks, rests, ids), rules=rules)
    # ---- the oracle chain of test_three_adjacent_chunks_to_phase_sets: the single calls, then the reference's updates, stitching (with
    # the values tests/contig_oracle.py reads out of stitching.c) and phase set rules restated in Python
    want, xs, xfs = vr.chain(gpu_ctx, chunks, rests, None, OPTS, pa.params())
    ochunks = contig_chunks(want, chunks, rests, ids)
    for o, w, x, xf, c, (fl, gt) in zip(ochunks, want, xs, xfs, chunks, rests):
        ox, oxf = vr.oracle_view(x, c.alleles), vr.oracle_view(xf, fl.alleles)
        g = w["result"]
        gf = dict(ref_start=g["ref_start"], length=g["length"], hap1=g["hap1"], hap2=g["hap2"], genotype_probs=g["genotype_probs"], hap_probs1=g["hap_probs1"],
                  hap_probs2=g["hap_probs2"])
        o["roots"] = (vo.update_with_bubble_data(ox, None, w["bubble_variant"], gf, w["hap"], c.variant_pos, c.chunk_start, c.chunk_end),
                      vo.update_filtered(ox, oxf, None, w["hap"], fl.variant_pos, gt, w["filtered"]["variant_state"], c.chunk_start, c.chunk_end))
    owant = co.close_contig(ochunks, rules=rules)
    print("switched", owant["switched"], "counts", owant["counts"], "variants", len(owant["variants"]))
    # ---- conditions, on the oracle's side
    assert any(owant["switched"])  # at least one chunk trades its haplotypes
    assert len(owant["variants"]) > 40 and {v["chunk"] for v in owant["variants"]} == {0, 1, 2}
    assert set(ids[0]) & set(ids[1]) and set(ids[1]) & set(ids[2])  # reads shared across the overlaps
    assert {1, 2} <= set(owant["final"].values())
    assert any(v["gt1"] != v["gt2"] for v in owant["variants"]) and sum(1 for s, why in owant["phase_sets"] if why == 0 and s >= 0) > 0
    # ---- equal: switches, counts, variants (positions, genotypes, read lists, float bits), phase sets and reasons, final HP tags
    co.assert_closed_equal(closed, owant, "contig")
    for c, ch in enumerate(chunks):
        assert closed["final_hap"][c].tolist() == [owant["final"].get(nm, 0) for nm in ch.read_names]
