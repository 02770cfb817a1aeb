"""The downsampling to maxDepth on the device.  The kernel's seam, mrp_downsample_reads, against the host
definition, mrp_downsample_keep_from_extracted: probabilities as fp64 bits, the mask byte for byte.  Each composite with
mrp_context_set_downsampling on against the same composite given keep[c] from the host definition over the chunk's primary extraction:
every output, float bits included.  The kernel does exact integer work and correctly rounded fp64 operations on exact integers, and the
composites run the same kernels over the same reads either way, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest

from margin_amd import capi, synth
from tests import downsample_cases as dc
from tests import rest_cases as rc
from tests import sv_split_cases as svc
from tests import test_gpu_phase_aligned as pa
from tests import test_gpu_phase_aligned_filtered as pf
from tests import test_gpu_variant_records as vr
from tests.test_gpu_extract import OPTION_SETS

pytestmark = pytest.mark.gpu

DEPTH, SEED = 4, 0xD0C5
OPTS = OPTION_SETS[0]  # the shipped windows


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the seam against the host definition -------------------------------------------------------------------------------------------

def seam_call():
    """about 300 chunks in one call: the edge cases, kept-read counts that cross one wave (63 / 64 / 65), one workgroup (255 / 256 /
    257), one LDS tile (1 025) and four of them (4 097), each deep and shallow, and random chunks, deep and shallow interleaved;
    dropped and low-mapq reads sit between the kept ones, so a read's rank differs from its index"""
    rng = np.random.default_rng(13)
    cases = [c for c, _ in dc.edge_cases()]
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1025):
        cases += [dc.random_case(rng, n, downsampled=True), dc.random_case(rng, n, downsampled=False), dc.random_case(rng, n, downsampled=True, ties=True)]
    cases.append(dc.random_case(rng, 4097, downsampled=True))
    k = 0
    while len(cases) < 300:
        cases.append(dc.random_case(rng, int(rng.integers(0, 140)), downsampled=k % 2 == 0, ties=k % 7 == 0))
        k += 1
    order = rng.permutation(len(cases))
    return [cases[i] for i in order]


def test_seam_equals_the_host_definition(gpu_ctx):
    cases = seam_call()
    n = len(cases)
    n_reads = np.array([len(c["l"]) for c in cases], np.int64)
    first = np.concatenate([[0], np.cumsum(n_reads)[:-1]]).astype(np.int64)
    V = np.array([c["V"] for c in cases], np.int64)
    ostart = 10_000 * np.arange(n, dtype=np.int64) + 7
    oend = ostart + 9_000 + np.arange(n, dtype=np.int64)
    l, h, status = (np.concatenate([c[k] for c in cases]) for k in ("l", "h", "status"))
    want = [capi.downsample_keep_from_extracted(dc.extracted(c), c["h"], dc.D, SEED, int(ostart[i]), int(oend[i])) for i, c in enumerate(cases)]
    wkeep, wprob = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    did = np.array([w[2] for w in want])
    kept = status == dc.KEPT
    # ---- conditions on the inputs, decided by the host definition alone
    n_kept = np.array([int((c["status"] == dc.KEPT).sum()) for c in cases])
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 4097} <= set(n_kept.tolist()) and n >= 300
    assert did.any() and (~did).any() and (did[1:] != did[:-1]).sum() > 50  # deep and shallow chunks interleaved
    assert ((wprob > 0) & (wprob < 1)).sum() > 50 and (kept & (wkeep == 0)).sum() > 1000 and (kept & (wkeep == 1) & np.repeat(did, n_reads)).sum() > 1000
    assert (status[:-1] != dc.KEPT).any() and (np.cumsum(kept)[kept] - 1 != np.flatnonzero(kept)).any()  # rank differs from index
    # ---- the kernel
    keep, prob, st = capi.downsample_reads(gpu_ctx, n_reads, first, l, h, status, V, dc.D, SEED, ostart, oend)
    assert np.array_equal(bits(prob), bits(wprob)), np.flatnonzero(bits(prob) != bits(wprob))[:10]
    assert keep.dtype == np.uint8 and np.array_equal(keep, wkeep), np.flatnonzero(keep != wkeep)[:10]
    assert (st.chunks, st.chunks_downsampled, st.reads_discarded) == (n, int(did.sum()), int((kept & (wkeep == 0)).sum()))
    assert st.bytes_downloaded == 9 * len(l) + 4 * n and st.downsample_ms > 0
    last = gpu_ctx.last_downsampling()
    assert (last.chunks, last.chunks_downsampled, last.reads_discarded, last.bytes_downloaded) == (st.chunks, st.chunks_downsampled, st.reads_discarded, st.bytes_downloaded)
    # a chunk alone gives its share of the joint call: its draws depend on the chunk alone
    for i in (int(np.argmax(n_kept == 257)), int(np.argmax(did & (n_kept > 20)))):
        c = cases[i]
        k1, p1, _ = capi.downsample_reads(gpu_ctx, [len(c["l"])], [0], c["l"], c["h"], c["status"], [c["V"]], dc.D, SEED, [ostart[i]], [oend[i]])
        assert np.array_equal(k1, want[i][0]) and np.array_equal(bits(p1), bits(want[i][1])), i
    # no chunk at all
    k0, p0, st0 = capi.downsample_reads(gpu_ctx, [], [], [], [], [], [], dc.D, SEED, [], [])
    assert k0.size == 0 and st0.chunks == 0 and st0.bytes_downloaded == 0


# ---- the composites -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def call():
    """three of the 8 kb / 8x chunks of tests/rest_cases.py, one variant in five filtered, and one thin chunk (2x)"""
    chunks, rests = [], []
    for seed in range(3):
        primary, filtered, _ = rc.split_variants(rc.synthetic(seed))
        chunks.append(primary)
        rests.append((filtered, rc.genotypes(filtered, seed)))
    primary, filtered, _ = rc.split_variants(synth.make_aligned_chunk(11, overlap_bp=8_000, coverage=2.0))
    chunks.append(primary)
    rests.append((filtered, rc.genotypes(filtered, 11)))
    return chunks, rests


@pytest.fixture()
def on_ctx():
    ctx = capi.Context(0)
    ctx.set_downsampling(DEPTH, SEED)
    yield ctx
    ctx.close()


def host_keeps(ctx, chunks, opts, seed, depth=DEPTH, xs=None):
    """the contract: per chunk mrp_downsample_keep_from_extracted over its primary extraction (xs: made before) -> (keeps, probabilities,
    downsampled, the extractions)"""
    got = xs if xs is not None else capi.extract_read_substrings(ctx, chunks, opts)[0]
    out = [capi.downsample_keep_from_extracted(x, capi.aln_read_lengths(c), depth, seed, c.overlap_start, c.overlap_end) for x, c in zip(got, chunks)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], got


COMPOSITES = {
    "plain": (lambda ctx, chunks, rests, keeps, opts, p: pa.composite(ctx, chunks, keeps, opts, p, min_phred=pf.MIN_PHRED), pa.assert_identical),
    "with_filtered": (lambda ctx, chunks, rests, keeps, opts, p: pf.composite(ctx, chunks, rests, keeps, opts, p, min_phred=pf.MIN_PHRED), pf.assert_identical),
    "with_records": (lambda ctx, chunks, rests, keeps, opts, p: vr.composite(ctx, chunks, rests, keeps, opts, p), vr.assert_identical),
}


def aligned_stats(st):
    return st.filtered.aligned if hasattr(st, "records_sites") else st.aligned if hasattr(st, "aligned") else st


def on_formula(A, chunks, with_rest=True):
    """front_bytes_downloaded with the setting on: what it was (include/margin_rphmm.h; with a rest the classes add 4 B per entry) plus
    1 B per read of the call's chunks and 4 B per chunk"""
    return (16 + 8 * (A.variants + 1) + (20 if with_rest else 16) * A.entries + A.extract.reads + 4 * A.pairs_anchored + 12 * A.anchor_runs
            + sum(len(c.read_pos) for c in chunks) + 4 * len(chunks))


@pytest.mark.parametrize("which", list(COMPOSITES))
def test_composite_equals_the_composite_given_keep(gpu_ctx, on_ctx, call, which):
    run, assert_identical = COMPOSITES[which]
    chunks, rests = call
    p = pa.params()
    keeps, probs, did, xs = host_keeps(gpu_ctx, chunks, OPTS, SEED)
    # ---- conditions on the inputs, decided by the chain alone
    print("downsampled", did, "discarded", [int(((x["read_status"] == capi.READ_KEPT) & (k == 0)).sum()) for x, k in zip(xs, keeps)])
    assert any(did) and not all(did) and not did[3]  # the thin chunk is shallow
    assert any(((pr > 0) & (pr < 1)).any() for pr in probs)  # a fractional p
    discarded = [np.flatnonzero((x["read_status"] == capi.READ_KEPT) & (k == 0)) for x, k in zip(xs, keeps)]
    assert sum(len(d) for d in discarded) > 0
    want, wst = run(gpu_ctx, chunks, rests, keeps, OPTS, p)
    if which != "plain":  # a discarded read comes back as a filtered read of kind (ii), and some of them with an HP tag
        tagged = 0
        for c, (w, d) in enumerate(zip(want, discarded)):
            fr = w["filtered_read"].tolist()
            assert set(d.tolist()) <= set(fr), c
            tags = w["filtered"]["read_hap"][len(chunks[c].read_pos):]
            tagged += sum(1 for r in d if tags[fr.index(int(r))] in (1, 2))
        assert tagged > 0
    # ---- the composite with the setting on
    got, st = run(on_ctx, chunks, rests, None, OPTS, p)
    assert_identical(got, want, which)
    ds = on_ctx.last_downsampling()
    assert (ds.chunks, ds.chunks_downsampled, ds.reads_discarded) == (len(chunks), sum(did), sum(len(d) for d in discarded))
    assert ds.bytes_downloaded == sum(len(c.read_pos) for c in chunks) + 4 * len(chunks) and ds.downsample_ms > 0
    A, W = aligned_stats(st), aligned_stats(wst)
    assert A.front_bytes_downloaded == on_formula(A, chunks, which != "plain") == W.front_bytes_downloaded + ds.bytes_downloaded
    assert (A.entries_used, A.owners, A.pairs) == (W.entries_used, W.owners, W.pairs)
    # each chunk alone gives its share of the joint call
    for c in range(len(chunks)):
        one, _ = run(on_ctx, chunks[c:c + 1], rests[c:c + 1], None, OPTS, p)
        assert_identical(one, got[c:c + 1], f"{which}, chunk {c} alone")
    # a repeat equals the first call
    again, ast = run(on_ctx, chunks, rests, None, OPTS, p)
    assert_identical(again, got, f"{which}, repeat")
    assert aligned_stats(ast).front_bytes_downloaded == A.front_bytes_downloaded
    # another seed, another mask: the first seed whose host masks differ (a vertex of the LP leaves one read per chunk to the draw)
    other = next(s for s in range(1, 64) if any(not np.array_equal(a, b) for a, b in zip(host_keeps(None, chunks, OPTS, s, xs=xs)[0], keeps)))
    keeps2 = host_keeps(None, chunks, OPTS, other, xs=xs)[0]
    on_ctx.set_downsampling(DEPTH, other)
    got2, _ = run(on_ctx, chunks, rests, None, OPTS, p)
    want2, _ = run(gpu_ctx, chunks, rests, keeps2, OPTS, p)
    assert_identical(got2, want2, f"{which}, seed {other}")
    assert any(not np.array_equal(a["hap"], b["hap"]) for a, b in zip(got2, got))


def test_off_after_on_is_as_never_set(gpu_ctx, call):
    chunks, rests = call
    p = pa.params()
    never, nst = pf.composite(gpu_ctx, chunks, rests, None, OPTS, p, min_phred=pf.MIN_PHRED)
    N = nst.aligned
    assert N.front_bytes_downloaded == 16 + 8 * (N.variants + 1) + 20 * N.entries + N.extract.reads + 4 * N.pairs_anchored + 12 * N.anchor_runs
    ctx = capi.Context(0)
    try:
        ctx.set_downsampling(DEPTH, SEED)
        on, ost = pf.composite(ctx, chunks, rests, None, OPTS, p, min_phred=pf.MIN_PHRED)
        assert ost.aligned.front_bytes_downloaded == on_formula(ost.aligned, chunks)
        assert ctx.last_downsampling().reads_discarded > 0 and any(not np.array_equal(a["hap"], b["hap"]) for a, b in zip(on, never))
        ctx.set_downsampling(0, SEED)
        off, fst = pf.composite(ctx, chunks, rests, None, OPTS, p, min_phred=pf.MIN_PHRED)
        pf.assert_identical(off, never, "off after on")
        assert fst.aligned.front_bytes_downloaded == N.front_bytes_downloaded and fst.aligned.entries_used == N.entries_used
        ds = ctx.last_downsampling()
        assert (ds.chunks, ds.chunks_downsampled, ds.reads_discarded, ds.bytes_downloaded, ds.downsample_ms) == (0, 0, 0, 0, 0.0)
        # a caller's mask is taken again
        keeps = [rc.keep_mask(dict(read_status=np.zeros(len(c.read_pos))), 3, 0.7) for c in chunks]
        a, _ = pf.composite(ctx, chunks, rests, keeps, OPTS, p, min_phred=pf.MIN_PHRED)
        b, _ = pf.composite(gpu_ctx, chunks, rests, keeps, OPTS, p, min_phred=pf.MIN_PHRED)
        pf.assert_identical(a, b, "a caller's mask after off")
    finally:
        ctx.close()


def test_argument_errors(gpu_ctx, call):
    chunks, rests = call
    p = pa.params()
    f, r = pa.models()
    keeps = [None, np.ones(len(chunks[1].read_pos), np.uint8), None, None]
    ctx = capi.Context(0)
    q = capi.Queue([0])
    try:
        for setter in (ctx.set_downsampling, q.set_downsampling):  # a negative depth
            with pytest.raises(capi.MrpError) as e:
                setter(-1, 0)
            assert e.value.code == capi.MRP_ERR_ARG
        ctx.set_downsampling(DEPTH, SEED)
        q.set_downsampling(DEPTH, SEED)
        # a keep mask together with the setting: an argument error, raised before the refused extraction modes
        rle = dict(OPTS, use_run_length_encoding=1)
        calls = [lambda o: pa.composite(ctx, chunks, keeps, o, p), lambda o: pf.composite(ctx, chunks, rests, keeps, o, p),
                 lambda o: vr.composite(ctx, chunks, rests, keeps, o, p),
                 lambda o: q.phase_aligned_chunks(chunks, f, r, p, options=o, keeps=keeps, chunks_per_batch=2),
                 lambda o: q.phase_aligned_chunks_with_filtered(chunks, rests, f, r, p, options=o, keeps=keeps, chunks_per_batch=2)]
        for fn in calls:
            for o in (OPTS, rle):
                with pytest.raises(capi.MrpError) as e:
                    fn(o)
                assert e.value.code == capi.MRP_ERR_ARG and "chunk 1" in str(e.value) and "keep" in str(e.value), str(e.value)
        # an array of NULL masks is no mask
        got, _ = pa.composite(ctx, chunks[:1], [None], OPTS, p)
        want, _ = pa.composite(ctx, chunks[:1], None, OPTS, p)
        pa.assert_identical(got, want, "NULL masks")
        # the haplotagging ignores the setting
        gts = [rc.genotypes(c, 5) for c in chunks[:2]]
        a, _ = capi.haplotag_aligned_chunks(ctx, chunks[:2], gts, f, r, OPTS)
        b, _ = capi.haplotag_aligned_chunks(gpu_ctx, chunks[:2], gts, f, r, OPTS)
        for x, y in zip(a, b):
            assert np.array_equal(x["hap"], y["hap"])
    finally:
        q.close()
        ctx.close()


def test_sv_split_and_downsampling_together():
    """the SV split on: l is the one count over both classes of variant, and the primary extraction alone decides"""
    ctx, plain = capi.Context(0), capi.Context(0)
    try:
        for c in (ctx, plain):
            c.set_sv_split(1)
        ctx.set_downsampling(DEPTH, SEED)
        primary, filtered, _ = rc.split_variants(svc.synthetic(0))
        assert primary.is_sv.any() and not primary.is_sv.all()
        chunks, rests = [primary], [(filtered, rc.genotypes(filtered, 0))]
        p = pa.params()
        keeps, probs, did, xs = host_keeps(plain, chunks, svc.OPTS, SEED)
        per_variant = np.diff(xs[0]["entry_first"])  # both classes' walks saved substrings: l counts over both
        assert per_variant[primary.is_sv != 0].sum() > 0 and per_variant[primary.is_sv == 0].sum() > 0
        assert int(xs[0]["read_n_substrings"].sum()) == int(per_variant.sum())
        assert did[0] and ((xs[0]["read_status"] == capi.READ_KEPT) & (keeps[0] == 0)).any()
        got, _ = pf.composite(ctx, chunks, rests, None, svc.OPTS, p, min_phred=pf.MIN_PHRED)
        want, _ = pf.composite(plain, chunks, rests, keeps, svc.OPTS, p, min_phred=pf.MIN_PHRED)
        pf.assert_identical(got, want, "sv split")
        assert ctx.last_downsampling().reads_discarded == int(((xs[0]["read_status"] == capi.READ_KEPT) & (keeps[0] == 0)).sum())
    finally:
        ctx.close()
        plain.close()


def test_queue_equals_the_one_call(on_ctx):
    """six chunks, two per batch: every chunk's outputs equal one call over all six -- a chunk's draws depend on the chunk alone"""
    chunks, rests = [], []
    for seed in range(6):
        primary, filtered, _ = rc.split_variants(rc.synthetic(seed))
        chunks.append(primary)
        rests.append((filtered, rc.genotypes(filtered, seed)))
    f, r = pa.models()
    p = pa.params()
    q = capi.Queue([0])
    try:
        q.set_downsampling(DEPTH, SEED)
        ref, _ = pa.composite(on_ctx, chunks, None, OPTS, p, min_phred=pf.MIN_PHRED)
        assert on_ctx.last_downsampling().reads_discarded > 0
        got, st = q.phase_aligned_chunks(chunks, f, r, p, options=OPTS, profiles=True, min_phred=pf.MIN_PHRED, chunks_per_batch=2)
        pa.assert_identical(got, ref, "aligned queue")
        assert st.batches == 3
        ref, _ = pf.composite(on_ctx, chunks, rests, None, OPTS, p, min_phred=pf.MIN_PHRED)
        got, st = q.phase_aligned_chunks_with_filtered(chunks, rests, f, r, p, options=OPTS, profiles=True, min_phred=pf.MIN_PHRED, chunks_per_batch=2)
        pf.assert_identical(got, ref, "aligned queue with filtered")
        assert st.batches == 3
        # off again: the queue gives what a context that never had it set gives
        q.set_downsampling(0, 0)
        never = capi.Context(0)
        try:
            ref, _ = pa.composite(never, chunks[:2], None, OPTS, p, min_phred=pf.MIN_PHRED)
        finally:
            never.close()
        got, _ = q.phase_aligned_chunks(chunks[:2], f, r, p, options=OPTS, profiles=True, min_phred=pf.MIN_PHRED, chunks_per_batch=1)
        pa.assert_identical(got, ref, "aligned queue, off again")
    finally:
        q.close()
