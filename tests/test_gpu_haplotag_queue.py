"""The work queue over haplotagging aligned chunks on the device (mrp_queue_haplotag_aligned_chunks, mrp_haplotag_aligned_chunks_on_devices):
at every chunk's own position the queue returns, bit for bit, what ONE mrp_haplotag_aligned_chunks call over all chunks returns -- whatever
the batch size, the lanes, or which worker took which batch.  A chunk's kernels see the same operands in the same order in whatever batch
it travels, so there is no tolerance anywhere against the one call: hap is compared as int8, h1 / h2 as uint64 views.  Only the oracle test
carries tests/test_gpu_haplotag_aligned.py's rule (tags equal, totals within 1e-9 * max(1, |oracle|), margins decisive).  Two workers share
device 0 (the device listed twice), as in tests/test_gpu_aligned_queue.py."""
import dataclasses

import numpy as np
import pytest

from margin_amd import capi
from tests import haplotag_aligned_oracle as hao
from tests import rest_cases as rc
from tests import test_gpu_haplotag_aligned as ha
from tests import test_gpu_phase_aligned as pa
from tests.test_gpu_aligned_queue import check_stats
from tests.test_gpu_haplotag_aligned import synthetic  # noqa: F401  (the six 8 kb / 8x chunks with drawn genotypes)
from tests.test_haplotag_queue_args import Call, built

pytestmark = pytest.mark.gpu

OPTS = capi.shipped_extract_options()


def units_of(chunks, gts):
    return np.array([capi.haplotag_chunk_units(c, g) for c, g in zip(chunks, gts)], dtype=np.int64)


def without_reads(chunk):
    e = lambda t: np.zeros(0, t)
    return dataclasses.replace(chunk, read_pos=e(np.int64), flag=e(np.uint16), mapq=e(np.uint8), l_qseq=e(np.int32), cigar_first=np.zeros(1, np.int64),
                               cigar=e(np.uint32), seq_first=np.zeros(1, np.int64), seq=e(np.uint8), read_names=[])


def test_parity_across_batchings(gpu_ctx, synthetic):  # noqa: F811
    chunks, gts = synthetic
    f, r, _, _ = ha.models()
    # the six chunks, chunk 1 again (a tie in the cost order), a chunk without variants, a chunk without reads, an all-homozygous chunk
    cs = list(chunks) + [chunks[1], rc.subset(chunks[2], []), without_reads(chunks[3]), chunks[0]]
    gs = list(gts) + [gts[1], None, gts[3], np.zeros_like(gts[0])]
    ref, rst = capi.haplotag_aligned_chunks(gpu_ctx, cs, gs, f, r, OPTS)
    # ---- conditions on the inputs, decided by the one call alone
    tags = np.concatenate([w["hap"] for w in ref])
    assert (tags == 1).any() and (tags == 2).any() and (tags == -1).any()
    assert rst.pairhmm.pairs_lane > 0 and rst.pairhmm.pairs_wave > 0
    assert ref[7]["hap"].size > 0 and ref[8]["hap"].size == 0
    hom = ref[9]
    assert (hom["hap"] == 0).any() and set(hom["hap"].tolist()) <= {0, -1}  # every kept read of the homozygous chunk: 0 / 0.0 / 0.0
    assert (hom["h1"] == 0).all() and (hom["h2"] == 0).all()
    units = units_of(cs, gs)
    assert units[6] == units[1] > 0 and units[7] == units[8] == units[9] == 0 and (units[:6] > 0).all()
    q = capi.Queue([0, 0])
    try:
        for per_batch in (1, 4, 0):
            got, st = q.haplotag_aligned_chunks(cs, gs, f, r, OPTS, chunks_per_batch=per_batch)
            ha.assert_identical(got, ref, f"chunks_per_batch {per_batch}")
            check_stats(st, units, per_batch, fallback=0)
    finally:
        q.close()


def test_the_one_device_form_and_the_defaults(gpu_ctx, synthetic):  # noqa: F811
    chunks, gts = synthetic
    chunks, gts = chunks[:4], gts[:4]
    f, r, _, _ = ha.models()
    ref, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r)
    got, st = capi.haplotag_aligned_chunks_on_devices([0], chunks, gts, f, r, chunks_per_batch=3)
    ha.assert_identical(got, ref, "on_devices")
    assert st.batches == 2 and st.n_devices == 1
    check_stats(st, units_of(chunks, gts), 3, n_devices=1)
    tags, tst = capi.haplotag_aligned_chunks_on_devices([0], chunks, gts, f, r, totals=False, chunks_per_batch=3)
    for a, b in zip(tags, ref):
        assert a["h1"] is None and a["h2"] is None and a["hap"].dtype == np.int8 and np.array_equal(a["hap"], b["hap"])
    assert tst.batches == 2
    with pytest.raises(capi.MrpError) as e:
        capi.haplotag_aligned_chunks_on_devices([99], chunks[:1], gts[:1], f, r)
    assert e.value.code == capi.MRP_ERR_ARG
    # no chunk: MRP_OK, zeroed stats
    none, nst = capi.haplotag_aligned_chunks_on_devices([0], [], [], f, r)
    assert none == [] and nst.batches == 0 and nst.n_devices == 1 and sum(nst.chunks_per_device) == 0 and sum(nst.units_per_device) == 0
    assert nst.fallback_chunks == 0 and max(nst.busy_ms_per_device) == 0


def test_oracle_parity_through_the_queue(gpu_ctx, synthetic):  # noqa: F811
    f, r, of, orv = ha.models()
    seeds = (1, 2, 4)
    chunks, gts = [synthetic[0][s] for s in seeds], [synthetic[1][s] for s in seeds]
    want = hao.haplotag(chunks, gts, OPTS, of, orv)
    q = capi.Queue([0, 0])
    try:
        got, st = q.haplotag_aligned_chunks(chunks, gts, f, r, OPTS, chunks_per_batch=1)
    finally:
        q.close()
    ha.assert_matches_oracle(got, want, "queue")
    assert st.batches == 3


def test_one_queue_several_kinds_of_work(gpu_ctx, synthetic):  # noqa: F811
    """the lanes' contexts are kept between calls, shared by the inputs of the queue and left clean by each"""
    chunks, gts = synthetic
    f, r, _, _ = ha.models()
    p = pa.params()
    ref, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r, OPTS)
    others = chunks[4:6]
    phased, _ = capi.phase_aligned_chunks(gpu_ctx, others, f, r, p, options=OPTS, profiles=True, min_phred=3)
    q = capi.Queue([0, 0])
    try:
        a, st_a = q.haplotag_aligned_chunks(chunks, gts, f, r, OPTS, chunks_per_batch=2)
        b, st_b = q.haplotag_aligned_chunks(chunks, gts, f, r, OPTS, chunks_per_batch=3)
        ha.assert_identical(a, ref, "two per batch")
        ha.assert_identical(b, ref, "three per batch")
        assert st_a.batches == 3 and st_b.batches == 2
        c, st_c = q.phase_aligned_chunks(others, f, r, p, options=OPTS, profiles=True, min_phred=3, chunks_per_batch=1)
        pa.assert_identical(c, phased, "phasing, behind haplotagging")
        assert st_c.batches == 2
        d, st_d = q.haplotag_aligned_chunks(chunks, gts, f, r, OPTS, chunks_per_batch=1)
        ha.assert_identical(d, ref, "haplotagging, behind phasing")
        assert st_d.batches == 6
    finally:
        q.close()


def test_diagonal_refusal_inside_a_lane(gpu_ctx, synthetic):  # noqa: F811
    """the lengths exist only after a batch's extraction: the 2 048-cell refusal is a lane's error (an error code raised before any pair-HMM
    launch, no device fault).  The queue stops, its outputs are unspecified, and it stays usable."""
    chunks, gts = synthetic
    f, r, _, _ = ha.models()
    long_chunk = pa.long_window_chunk()  # the one-read 6 000-base chunk of test_diagonal_limit_is_raised_before_the_pair_hmm
    good, good_gts = list(chunks[:4]), list(gts[:4])
    cs = good[:2] + [long_chunk] + good[2:]
    gs = good_gts[:2] + [np.array([[0, 1]], np.int32)] + good_gts[2:]
    wide = dict(OPTS, expansion_sv=2_200)
    q = capi.Queue([0, 0])
    try:
        with pytest.raises(capi.MrpError) as e:
            q.haplotag_aligned_chunks(cs, gs, f, r, wide, chunks_per_batch=1)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "diagonal" in str(e.value)
        # the same through the C entry, to look at the stats
        call = Call(built(cs), gs, options=wide)
        call.fwd, call.rev, call.per_batch = f, r, 1
        rc_, msg = call.run("queue", q=q.h)
        assert rc_ == capi.MRP_ERR_UNSUPPORTED and b"diagonal" in msg
        assert call.stats.batches == len(cs) and call.stats.n_devices == 2 and call.stats.fallback_chunks == 0
        # the queue stays usable
        got, st = q.haplotag_aligned_chunks(good, good_gts, f, r, OPTS, chunks_per_batch=1)
        ref, _ = capi.haplotag_aligned_chunks(gpu_ctx, good, good_gts, f, r, OPTS)
        ha.assert_identical(got, ref, "after the refusal")
        assert st.batches == 4
    finally:
        q.close()


def test_host_threads(gpu_ctx, synthetic):  # noqa: F811
    chunks, gts = synthetic
    f, r, _, _ = ha.models()
    lib = capi.load()
    ref, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r)
    try:
        for threads in (1, 3, 0):
            lib.mrp_set_host_threads(threads)
            q = capi.Queue([0, 0])  # (a queue sizes its pools when it is created)
            try:
                got, st = q.haplotag_aligned_chunks(chunks, gts, f, r, chunks_per_batch=2)
            finally:
                q.close()
            ha.assert_identical(got, ref, f"threads {threads}")
            assert st.batches == 3
    finally:
        lib.mrp_set_host_threads(0)
