"""Wide pairs on the device (mrp_context_set_wide_pairs / mrp_queue_set_wide_pairs): pairs whose widest diagonal
exceeds the pair-per-wave kernel's 2 048 cells go to the pair-per-workgroup kernel instead of being refused.  The kernel runs the same
cell arithmetic in the same order, so the log probabilities are compared bit for bit with oracle/pairhmm_oracle.c and the composites
bit for bit with their chains on the same context: no tolerance on any pair-HMM value.  The two scoring loops compared with
tests/haptag_oracle.py keep that file's own rule for their TOTALS (decisions equal, totals within 1e-9 * max(1, |oracle|), margins
decisive, as tests/test_gpu_haptag.py: the device's log / exp in the reduction are not glibc's).

Every test makes its own context or queue with the setting on and closes it; the session's gpu_ctx is never switched."""
import numpy as np
import pytest

from margin_amd import capi, synth
from oracle import pairhmm as ph
from tests import haptag_oracle as ho
from tests import string_filtered_cases as sf
from tests import test_gpu_haplotag_aligned as ha
from tests import test_gpu_phase_aligned as pa
from tests.test_gpu_pairhmm import models3, pack
from tests.test_gpu_string_queue import assert_identical as assert_strings_identical
from tests.test_pairhmm import omodel

pytestmark = pytest.mark.gpu

RAGGED = [(False, False), (True, False), (False, True), (True, True)]
LONG_OPTS = dict(capi.shipped_extract_options(), expansion_sv=2_200)


@pytest.fixture()
def wide_ctx():
    ctx = capi.Context(0)
    ctx.set_wide_pairs(1)
    yield ctx
    ctx.close()


@pytest.fixture()
def wide_queue():
    q = capi.Queue([0])
    q.set_wide_pairs(1)
    yield q
    q.close()


def related(rng, lx, ly, n_rate=0.0):
    """an x string and a y string of exactly ly symbols that resembles it"""
    a = synth.random_sequence(rng, lx, n_rate=n_rate)
    b = synth.evolve_sequence(rng, a, 0.02, 0.01, 0.01)
    b = b[:ly] if len(b) >= ly else np.concatenate([b, synth.random_sequence(rng, ly - len(b))])
    return a, np.ascontiguousarray(b)


def cells_of(xl, yl):
    return int(((np.asarray(xl, np.int64) + 1) * (np.asarray(yl, np.int64) + 1)).sum())


def test_edges_of_the_class_unanchored(wide_ctx):
    """width 2 049 is the first wide pair and width 2 048 stays on the wave kernel in the same call; a plateau of full-width diagonals in
    both orientations; more than four cells per thread and diagonal.  The ragged combination is the call's, so every call scores all five
    pairs and pair i is compared with the oracle under combination i % 4; the three models are spread over the pairs."""
    rng = np.random.default_rng(2049)
    shapes = [(2048, 2048), (2047, 2047), (2048, 2300), (2300, 2048), (4100, 4100)]
    pairs = [related(rng, lx, ly, n_rate=0.002) for lx, ly in shapes]
    pool, xo, xl, yo, yl = pack(pairs)
    mi = np.array([0, 1, 2, 1, 0], np.uint8)
    ms = models3()
    oms = [omodel(m) for m in ms]
    wide = [i for i, (lx, ly) in enumerate(shapes) if min(lx, ly) + 1 > 2048]
    assert wide == [0, 2, 3, 4] and capi.pair_diagonal_width([], 2047, 2047, 4)[0] == 2048
    for k, (rl, rr) in enumerate(RAGGED):
        before = wide_ctx.wide_pair_count()
        out, st = capi.forward_probabilities(wide_ctx, ms, pool, xo, xl, yo, yl, mi, ragged_left=rl, ragged_right=rr)
        after = wide_ctx.wide_pair_count()
        assert (after[0] - before[0], after[1] - before[1]) == (4, cells_of(xl[wide], yl[wide]))
        assert st.pairs_wave == 5 and st.pairs_lane == 0 and st.cells == cells_of(xl, yl)
        assert np.isfinite(out).all()
        mine = [i for i in range(len(shapes)) if i % 4 == k]
        ref = ph.forward_batch(oms, pool, xo[mine], xl[mine], yo[mine], yl[mine], mi[mine], ragged_left=rl, ragged_right=rr)
        assert np.isfinite(ref).all() and (out[mine] == ref).all(), (k, out[mine], ref)


def test_anchored_and_wide(wide_ctx):
    """two distant anchors: the band between them is as wide as the gap.  A second pair with N symbols and unequal lengths."""
    rng = np.random.default_rng(3000)
    pairs = [related(rng, 3000, 3000), related(rng, 2600, 3100, n_rate=0.01)]
    assert (pairs[1][0] == 4).any()
    anchors = [[(200, 200), (2800, 2800)], [(100, 150), (2500, 2950)]]
    pool, xo, xl, yo, yl = pack(pairs)
    aoff = np.array([0, 2, 4], np.int64)
    an = np.array(anchors[0] + anchors[1], np.int64)
    mi = np.array([0, 1], np.uint8)
    ms = models3()
    oms = [omodel(m) for m in ms]
    for expansion in (4, 20):
        widths = [capi.pair_diagonal_width(anchors[i], int(xl[i]), int(yl[i]), expansion) for i in range(2)]
        assert all(w > 2048 for w, _ in widths)
        before = wide_ctx.wide_pair_count()
        out, st = capi.forward_probabilities(wide_ctx, ms, pool, xo, xl, yo, yl, mi, aoff, an, expansion=expansion)
        after = wide_ctx.wide_pair_count()
        assert (after[0] - before[0], after[1] - before[1]) == (2, sum(c for _, c in widths)) and st.cells == sum(c for _, c in widths)
        ref = ph.forward_batch(oms, pool, xo, xl, yo, yl, mi, aoff, an, expansion=expansion)
        assert np.isfinite(ref).all() and (out == ref).all(), (expansion, out, ref)


def test_one_workgroup_reuses_its_workspace_slice(wide_ctx):
    """test hook bit 6: the wide kernel's grid is one workgroup, so the three wide pairs run one after the other in one slice, largest
    first: stale cells of the larger pair must not leak into the smaller.  Lane-class and wave-class pairs travel in the same call and
    every output sits at its own index."""
    rng = np.random.default_rng(2600)
    small = [(synth.random_sequence(rng, int(rng.integers(0, 60))), synth.random_sequence(rng, int(rng.integers(0, 80)))) for _ in range(50)]
    medium = [related(rng, n, n + 7) for n in rng.integers(120, 400, size=10).tolist()]
    wide = [related(rng, 2600, 2600), related(rng, 2100, 2100), related(rng, 2048, 2500)]
    pairs = small[:20] + [wide[1]] + medium[:5] + small[20:] + [wide[0]] + medium[5:] + [wide[2]]
    where = [20, 56, 62]
    pool, xo, xl, yo, yl = pack(pairs)
    mi = rng.integers(0, 3, size=len(pairs)).astype(np.uint8)
    ms = models3()
    ref = ph.forward_batch([omodel(m) for m in ms], pool, xo, xl, yo, yl, mi)
    wide_ctx.set_test_hooks(64)
    out, st = capi.forward_probabilities(wide_ctx, ms, pool, xo, xl, yo, yl, mi)
    wide_ctx.set_test_hooks(0)
    assert st.pairs_lane == 50 and st.pairs_wave == 13 and wide_ctx.wide_pair_count() == (3, cells_of(xl[where], yl[where]))
    assert np.isfinite(ref).all() and (out == ref).all(), np.nonzero(out != ref)
    again, _ = capi.forward_probabilities(wide_ctx, ms, pool, xo, xl, yo, yl, mi)  # a workgroup per pair: the same numbers
    assert (again == ref).all()


def wide_site(rng):
    """two 2 100-symbol alleles and three read substrings, the third a copy of the first on the other strand"""
    a0 = synth.random_sequence(rng, 2100)
    a1 = a0.copy()
    a1[1000] = (a1[1000] + 1) % 4
    s0 = synth.evolve_sequence(rng, a0, 0.01, 0.005, 0.005)
    s1 = synth.evolve_sequence(rng, a1, 0.01, 0.005, 0.005)
    return [a0, a1], [s0, s1, s0.copy()], [True, False, False]


def test_the_never_anchored_loops(wide_ctx):
    rng = np.random.default_rng(2100)
    f, r, of, orv = ha.models()
    alleles, subs, strands = wide_site(rng)
    assert min(len(s) for s in subs) > 2048
    site = [(alleles, (0, 1), [(q, s) for q, s in enumerate(subs)])]
    # the partition never anchors (bubbleGraph.c:1832)
    hap, h1, h2, st = capi.partition_reads_by_haplotype(wide_ctx, f, r, site, 3, strands)
    rhap, rh1, rh2 = ho.partition_filtered_reads(of, orv, site, 3, strands)
    assert st.pairs_wave == 4 and wide_ctx.wide_pair_count()[0] == 4
    ho.assert_margins_decisive(rh1, rh2, "partition")
    assert (hap == rhap).all() and ha.close(h1, rh1) and ha.close(h2, rh2)
    assert set(rhap.tolist()) == {1, 2}
    # the variants with the threshold above the lengths
    read_hap = np.array([1, 2, 2], np.int32)
    state, cis, trans, st = capi.phase_variants_from_tagged_reads(wide_ctx, f, r, site, 3, strands, read_hap, sv_threshold=100_000)
    rstate, rcis, rtrans = ho.phase_filtered_variants(of, orv, site, 3, strands, read_hap, sv_threshold=100_000)
    assert st.pairs_wave == 4 and wide_ctx.wide_pair_count()[0] == 8
    ho.assert_margins_decisive(rcis, rtrans, "phasing")
    assert (state == rstate).all() and ha.close(cis, rcis) and ha.close(trans, rtrans)


def test_allele_read_supports_with_a_wide_bubble(wide_ctx):
    rng = np.random.default_rng(2101)
    f, r, of, orv = ha.models()
    bubbles = synth.make_bubble_strings(seed=5, n_sites=20, coverage=10)
    alleles, subs, strands = wide_site(rng)
    bubbles.insert(7, (alleles, subs[1:], strands[1:]))
    got, st = capi.allele_read_supports(wide_ctx, f, r, bubbles, sv_threshold=100_000)
    assert wide_ctx.wide_pair_count()[0] == 4 and st.pairs_wave == 4 and st.pairs_lane > 0
    for (al, reads, fs), sup in zip(bubbles, got):
        ref = ph.allele_read_supports(of, orv, al, reads, fs, sv_threshold=100_000)
        assert np.isfinite(ref).all() and sup.shape == ref.shape and (sup == ref).all()


def oversize_string_chunk():
    """the chunk and the rest of tests/test_gpu_string_filtered.py::test_oversize_unanchored_pair_of_the_back_half_is_refused"""
    rng = np.random.default_rng(8)
    big = synth.random_sequence(rng, 2100)
    alt = big.copy()
    alt[1000] = (alt[1000] + 1) % 4
    chunk = synth.StringChunk(bubbles=[([big, alt], [0], [big.copy()])], read_names=["long"], read_forward_strand=np.ones(1, np.uint8),
                              hap=np.zeros(1, int), truth=[0])
    rest = dict(forward_strand=np.ones(1, np.uint8), fsubs=[[(0, synth.random_sequence(rng, 30))]], variants=[])
    return chunk, rest


def test_string_composite_equals_its_chain(wide_ctx):
    from tests.test_gpu_string_chunks import models, params
    f, r = models()
    p = params()
    chunk, rest = oversize_string_chunk()
    got, st = capi.phase_string_chunks_with_filtered(wide_ctx, [chunk], [rest], f, r, p, min_phred=sf.MIN_PHRED, profiles=True)
    assert wide_ctx.wide_pair_count()[0] > 0 and st.pairs_scored == st.chunks.pairhmm.pairs_lane + st.chunks.pairhmm.pairs_wave
    front, back = sf.chain(wide_ctx, [chunk], [rest], f, r, p)
    assert_strings_identical(got, front, [chunk])
    sf.assert_back_identical(got, back)
    assert back[0]["psites"] and len(back[0]["psites"][0][2]) >= 1  # the partition did align against the 2 100-symbol alleles


def test_aligned_composites_equal_their_chains(wide_ctx):
    p = pa.params()
    chunk = pa.long_window_chunk()
    got, st = pa.composite(wide_ctx, [chunk], None, LONG_OPTS, p, sv_threshold=100_000)
    n_wide = wide_ctx.wide_pair_count()[0]
    assert st.pairs == 2 and st.pairs_anchored == 0 and n_wide == 2 and st.chunks.pairhmm.pairs_wave == 2
    want, _, _ = pa.chain(wide_ctx, [chunk], None, LONG_OPTS, p, sv_threshold=100_000)
    pa.assert_identical(got, want, "long window, unanchored")
    # the same chunk haplotagged from a phased genotype: never anchored (tools/tagFromPhasedVcf.c)
    f, r, _, _ = ha.models()
    gts = [np.array([[0, 1]], np.int32)]
    before = wide_ctx.wide_pair_count()[0]
    tags, hst = capi.haplotag_aligned_chunks(wide_ctx, [chunk], gts, f, r, LONG_OPTS)
    assert wide_ctx.wide_pair_count()[0] - before == 2 and hst.pairhmm.pairs_wave == 2
    ha.assert_identical(tags, ha.chain(wide_ctx, [chunk], gts, LONG_OPTS, f, r), "haplotag, long window")
    assert tags[0]["hap"].tolist() != [-1]


def test_queues_equal_the_one_call(wide_ctx, wide_queue):
    """the long chunk beside two ordinary ones, a chunk per batch: bit for bit the one call over the same chunks on a wide context"""
    p = pa.params()
    f, r = pa.models()
    ordinary = [synth.make_aligned_chunk(seed, overlap_bp=6_000, coverage=6.0, sv_share=0.0) for seed in (11, 12)]
    cs = [ordinary[0], pa.long_window_chunk(), ordinary[1]]
    ref, _ = pa.composite(wide_ctx, cs, None, LONG_OPTS, p, sv_threshold=100_000, min_phred=3)
    got, st = wide_queue.phase_aligned_chunks(cs, f, r, p, options=LONG_OPTS, profiles=True, sv_threshold=100_000, min_phred=3, chunks_per_batch=1)
    pa.assert_identical(got, ref, "aligned queue")
    assert st.batches == 3 and wide_queue.wide_pair_count()[0] == 2
    from tests import haplotag_aligned_oracle as hao
    gts = [hao.draw_genotypes(cs[0], 11), np.array([[0, 1]], np.int32), hao.draw_genotypes(cs[2], 12)]
    href, _ = capi.haplotag_aligned_chunks(wide_ctx, cs, gts, f, r, LONG_OPTS)
    hgot, hst = wide_queue.haplotag_aligned_chunks(cs, gts, f, r, LONG_OPTS, chunks_per_batch=1)
    ha.assert_identical(hgot, href, "haplotag queue")
    assert hst.batches == 3 and wide_queue.wide_pair_count()[0] == 4
    # strings: the up-front check no longer refuses, the fronts are made on the prefetch thread
    from tests.test_gpu_string_chunks import models, params
    sf_, sr_ = models()
    sp = params()
    big, big_rest = oversize_string_chunk()
    a, ar = sf.split_chunk(431, n_sites=30, coverage=24)
    b, br = sf.split_chunk(432, n_sites=40, coverage=24, duplicate_rate=0.25)
    scs, srs = [a, big, b], [ar, big_rest, br]
    sref, _ = capi.phase_string_chunks_with_filtered(wide_ctx, scs, srs, sf_, sr_, sp, min_phred=sf.MIN_PHRED, profiles=True)
    sgot, sst = capi.queue_phase_string_chunks_with_filtered(wide_queue, scs, srs, sf_, sr_, sp, min_phred=sf.MIN_PHRED, chunks_per_batch=1, profiles=True)
    assert_strings_identical(sgot, sref, scs)
    sf.assert_back_identical(sgot, [g["filtered"] for g in sref])
    pairs, cells = wide_queue.wide_pair_count()
    assert sst.batches == 3 and pairs > 4 and cells > 0


def test_the_switch_and_the_caps():
    ms = models3()
    ctx = capi.Context(0)
    try:
        big = np.zeros(2 * 2100, np.uint8)
        args = (ms, big, [0], [2100], [2100], [2100])
        with pytest.raises(capi.MrpError) as e:  # off by default
            capi.forward_probabilities(ctx, *args)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED
        ctx.set_wide_pairs(1)
        out, st = capi.forward_probabilities(ctx, *args)
        assert np.isfinite(out).all() and st.pairs_wave == 1 and ctx.wide_pair_count() == (1, 2101 * 2101)
        ctx.set_wide_pairs(0)
        with pytest.raises(capi.MrpError) as e:  # off again: the old refusal with the old message
            capi.forward_probabilities(ctx, *args)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED
        assert "diagonal" in str(e.value) and "2101 cells" in str(e.value) and "limit 2048" in str(e.value)
        ctx.set_wide_pairs(1)
        count = ctx.wide_pair_count()
        zeros = np.zeros(2 * 32768, np.uint8)
        with pytest.raises(capi.MrpError) as e:  # the width cap
            capi.forward_probabilities(ctx, ms, zeros, [0], [32768], [32768], [32768])
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "diagonal" in str(e.value) and "32769" in str(e.value) and "32768" in str(e.value)
        zeros = np.zeros(230_000, np.uint8)
        with pytest.raises(capi.MrpError) as e:  # the cells cap: width 30 001 is allowed, 6e9 cells are not
            capi.forward_probabilities(ctx, ms, zeros, [0], [30_000], [30_000], [200_000])
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "diagonal" in str(e.value) and str(2 ** 31) in str(e.value)
        # a refused pair stops the whole call before anything is launched, also beside pairs that would run
        with pytest.raises(capi.MrpError):
            capi.forward_probabilities(ctx, ms, zeros, [0, 0], [2100, 30_000], [30_000, 30_000], [2100, 200_000])
        assert ctx.wide_pair_count() == count
        # the context then scores an ordinary batch correctly
        rng = np.random.default_rng(1)
        pairs = [(synth.random_sequence(rng, int(n)), synth.random_sequence(rng, int(n) + 3)) for n in rng.integers(0, 300, size=40)]
        pool, xo, xl, yo, yl = pack(pairs)
        mi = rng.integers(0, 3, size=len(pairs)).astype(np.uint8)
        out, st = capi.forward_probabilities(ctx, ms, pool, xo, xl, yo, yl, mi)
        assert (out == ph.forward_batch([omodel(m) for m in ms], pool, xo, xl, yo, yl, mi)).all()
        assert st.pairs_lane > 0 and st.pairs_wave > 0 and ctx.wide_pair_count() == count
    finally:
        ctx.close()
