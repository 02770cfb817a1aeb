"""The work queue over aligned chunks on the device (mrp_queue_phase_aligned_chunks, mrp_queue_phase_aligned_chunks_with_filtered and
their *_on_devices forms): at every chunk's own position the queue returns, bit for bit, what ONE mrp_phase_aligned_chunks /
mrp_phase_aligned_chunks_with_filtered call over all chunks returns -- whatever the batch size, the lanes, or which worker took which
batch.  A chunk's kernels see the same operands in the same order in whatever batch it travels, so there is no tolerance anywhere in
this file.  Two workers share device 0 (the device listed twice), as in tests/test_gpu_string_queue.py."""
import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import rest_cases as rc
from tests import string_filtered_cases as sf
from tests import test_gpu_phase_aligned as pa
from tests import test_gpu_phase_aligned_filtered as pf
from tests import test_gpu_string_queue as sq
from tests.test_aligned_queue_args import Call, built
from tests.test_gpu_phase_aligned_filtered import synthetic  # noqa: F401  (the six 8 kb / 8x chunks and their rests)

pytestmark = pytest.mark.gpu

MIN_PHRED = sf.MIN_PHRED
OPTS = capi.shipped_extract_options()


def units_of(chunks, rests=None):
    return np.array([capi.aligned_chunk_units(c, None if rests is None else rests[i]) for i, c in enumerate(chunks)], dtype=np.int64)


def check_stats(st, units, chunks_per_batch, n_devices=2, fallback=0):
    """tests/test_gpu_string_queue.check_stats over mrp_aligned_chunk_units"""
    n = len(units)
    _order, batch = capi.queue_plan(units, chunks_per_batch)
    assert st.n_devices == n_devices
    assert sum(st.chunks_per_device[:n_devices]) == n and sum(st.chunks_per_device[n_devices:]) == 0
    assert sum(st.units_per_device[:n_devices]) == int(units.sum())
    if chunks_per_batch >= 1:
        assert st.batches == int(batch.max()) + 1 == -(-n // chunks_per_batch)
    else:  # the library's cut: a short queue is one batch per device
        assert st.batches == min(n, n_devices)
    assert st.fallback_chunks == fallback
    assert max(st.busy_ms_per_device[:n_devices]) > 0


def test_parity_across_batchings_with_filtered(gpu_ctx, synthetic):  # noqa: F811
    chunks, rests = synthetic
    f, r = pa.models()
    p = pa.params()
    hand = {name: (rc.split_hand(ch, fidx), gt) for name, ch, fidx, gt, _keep in rc.hand_cases()}
    (e_primary, e_filtered), e_gt = hand["empty"]
    nothing = ec.make([], [(100, "20M", 60, 0)])
    # the six chunks, chunk 1 again (a tie in the cost order), a chunk with an empty rest, a chunk without variants
    cs = list(chunks) + [chunks[1], e_primary, nothing]
    rs = list(rests) + [rests[1], (e_filtered, e_gt), (nothing, [])]
    keeps = [None] * len(cs)
    keeps[4] = (np.random.default_rng(4).random(len(chunks[4].read_pos)) < 0.8).astype(np.uint8)
    ref, rst = capi.phase_aligned_chunks_with_filtered(gpu_ctx, cs, rs, f, r, p, options=OPTS, keeps=keeps, profiles=True, min_phred=MIN_PHRED)
    # ---- conditions on the inputs, decided by the one call alone
    states = np.concatenate([w["filtered"]["variant_state"] for w in ref])
    assert (states == capi.VARIANT_CIS).any() and (states == capi.VARIANT_TRANS).any() and (states == capi.VARIANT_NOT_VISITED).any()
    assert rst.aligned.pairs_anchored > 0 and rst.filtered_reads > 0 and rst.aligned.chunks.phase.resident == 1
    units = units_of(cs, rs)
    assert len(set(units.tolist())) < len(cs) and units[6] == units[1] > 0 and units[8] == 0
    q = capi.Queue([0, 0])
    try:
        for per_batch in (1, 4, 0):
            got, st = q.phase_aligned_chunks_with_filtered(cs, rs, f, r, p, options=OPTS, keeps=keeps, profiles=True, min_phred=MIN_PHRED,
                                                           chunks_per_batch=per_batch)
            pf.assert_identical(got, ref, f"chunks_per_batch {per_batch}")
            check_stats(st, units, per_batch)
    finally:
        q.close()


def test_the_plain_twin_and_the_one_device_form(gpu_ctx, synthetic):  # noqa: F811
    chunks, _rests = synthetic
    chunks = chunks[:4]
    f, r = pa.models()
    p = pa.params()
    keeps = [None, (np.random.default_rng(8).random(len(chunks[1].read_pos)) < 0.7).astype(np.uint8), None, None]
    ref, _ = capi.phase_aligned_chunks(gpu_ctx, chunks, f, r, p, options=OPTS, keeps=keeps, profiles=True, min_phred=3)
    got, st = capi.phase_aligned_chunks_on_devices([0], chunks, f, r, p, options=OPTS, keeps=keeps, profiles=True, min_phred=3, chunks_per_batch=3)
    pa.assert_identical(got, ref, "on_devices")
    check_stats(st, units_of(chunks), 3, n_devices=1)
    with pytest.raises(capi.MrpError) as e:
        capi.phase_aligned_chunks_on_devices([99], chunks[:1], f, r, p, options=OPTS)
    assert e.value.code == capi.MRP_ERR_ARG
    # no chunk: MRP_OK, zeroed stats
    none, nst = capi.phase_aligned_chunks_on_devices([0], [], f, r, p, options=OPTS)
    assert none == [] and nst.batches == 0 and nst.n_devices == 1 and sum(nst.chunks_per_device) == 0


def test_the_same_queue_twice_and_then_strings(gpu_ctx, synthetic):  # noqa: F811
    """the lanes' contexts are kept between calls, and the inputs of the queue share them"""
    chunks, rests = synthetic
    f, r = pa.models()
    p = pa.params()
    ref, _ = capi.phase_aligned_chunks_with_filtered(gpu_ctx, chunks, rests, f, r, p, options=OPTS, profiles=True, min_phred=MIN_PHRED)
    plain, _ = capi.phase_aligned_chunks(gpu_ctx, chunks, f, r, p, options=OPTS, profiles=True, min_phred=3)
    strings = sq.queue_chunks(6)
    sf_, sr_ = sq.models()
    sp = sq.params()
    sref, _ = capi.phase_string_chunks(gpu_ctx, strings, sf_, sr_, sp, min_phred=3, profiles=True)
    q = capi.Queue([0, 0])
    try:
        a, st_a = q.phase_aligned_chunks_with_filtered(chunks, rests, f, r, p, options=OPTS, profiles=True, min_phred=MIN_PHRED, chunks_per_batch=2)
        b, st_b = q.phase_aligned_chunks_with_filtered(chunks, rests, f, r, p, options=OPTS, profiles=True, min_phred=MIN_PHRED, chunks_per_batch=3)
        pf.assert_identical(a, ref, "two per batch")
        pf.assert_identical(b, ref, "three per batch")
        assert st_a.batches == 3 and st_b.batches == 2
        s, st_s = q.phase_string_chunks(strings, sf_, sr_, sp, min_phred=3, chunks_per_batch=2, profiles=True)
        sq.assert_identical(s, sref, strings)
        assert st_s.batches == 3
        c, st_c = q.phase_aligned_chunks(chunks, f, r, p, options=OPTS, profiles=True, min_phred=3, chunks_per_batch=1)
        pa.assert_identical(c, plain, "plain, behind strings")
        assert st_c.batches == 6
    finally:
        q.close()


def test_diagonal_refusal_inside_a_lane(gpu_ctx, synthetic):  # noqa: F811
    """the lengths exist only after a batch's extraction: the 2 048-cell refusal is a lane's error (an error code, no device fault).  The
    queue stops, returns nothing and stays usable."""
    chunks, rests = synthetic
    f, r = pa.models()
    p = pa.params()
    long_chunk = pa.long_window_chunk()
    good, good_rests = list(chunks[:4]), list(rests[:4])
    cs = good[:2] + [long_chunk] + good[2:]
    rs = good_rests[:2] + [(rc.subset(long_chunk, []), [])] + good_rests[2:]
    wide = dict(OPTS, expansion_sv=2_200)
    q = capi.Queue([0, 0])
    try:
        with pytest.raises(capi.MrpError) as e:  # unanchored (sv_threshold above the lengths): a diagonal beyond 2 048 cells
            q.phase_aligned_chunks_with_filtered(cs, rs, f, r, p, options=wide, profiles=True, sv_threshold=100_000, chunks_per_batch=1)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "diagonal" in str(e.value)
        # the same through the C entry, to look at the outputs
        structs, rest_structs = built(cs, rs)
        call = Call(cs, structs, rest_structs, options=wide)
        call.sv_threshold, call.per_batch = 100_000, 1
        rc_ = call.run("queue", True, q=q.h)
        assert rc_ == capi.MRP_ERR_UNSUPPORTED and b"diagonal" in capi.load().mrp_last_error()
        n = len(cs)
        assert all(not call.res[i] and not call.bv[i] and not call.fr[i] for i in range(n))
        assert bytes(call.prof) == bytes((capi.ProfileOut * n)()) and bytes(call.fout) == bytes((capi.FilteredOut * n)())
        assert call.stats.batches == n
        # the queue stays usable
        got, st = q.phase_aligned_chunks_with_filtered(good, good_rests, f, r, p, options=OPTS, profiles=True, min_phred=MIN_PHRED, chunks_per_batch=1)
        ref, _ = capi.phase_aligned_chunks_with_filtered(gpu_ctx, good, good_rests, f, r, p, options=OPTS, profiles=True, min_phred=MIN_PHRED)
        pf.assert_identical(got, ref, "after the refusal")
        assert st.batches == 4
    finally:
        q.close()


def test_outside_the_resident_range(gpu_ctx, synthetic):  # noqa: F811
    """the unit tests' parameters in sum mode: every batch takes the one call's per-chunk path"""
    chunks, _rests = synthetic
    chunks = chunks[2:4]
    f, r = pa.models()
    p = pa.params(synth.unit_test_params(max_partitions=50, max_not_sum=0))
    ref, rst = capi.phase_aligned_chunks(gpu_ctx, chunks, f, r, p, options=OPTS, profiles=True)
    assert rst.chunks.phase.resident == 0
    q = capi.Queue([0, 0])
    try:
        got, st = q.phase_aligned_chunks(chunks, f, r, p, options=OPTS, profiles=True, chunks_per_batch=1)
    finally:
        q.close()
    pa.assert_identical(got, ref, "per-chunk path")
    check_stats(st, units_of(chunks), 1, fallback=2)
    assert st.batches == 2
