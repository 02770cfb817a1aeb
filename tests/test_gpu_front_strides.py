"""The kernels of the alignment front on inputs that make them take a second trip (tests/stride_cases.py; what each case exhibits is
asserted without a device in tests/test_stride_cases.py): a wave's lanes striding over more than 64 parts of one work item -- a
read's candidate entries and CIGAR ops, a variant's substrings, a k-mer chain's walk back over the records in the workspace -- and
the waves striding over more work items than the grid cap -- variants, entries, sites, pairs.

A. mrp_extract_read_substrings against tests/extract_oracle.py, byte for byte;
B. mrp_haplotag_aligned_chunks (ha_owners_kernel over more than 65 536 sites) against tests/haplotag_aligned_oracle.py (totals
   within 1e-9 * max(1, |oracle|), tags equal) and bit for bit against the chain of three calls; mrp_equal_substring_classes
   over 65 536 + 40 sites against the host grouping;
C. mrp_kmer_alignment_anchors_many against oracle.pairhmm.kmer_anchors, pair by pair, counts and values;
D. mrp_forward_probabilities with every pair in the pair-per-wave kernel, bit for bit against oracle.pairhmm.forward_batch."""
import numpy as np
import pytest

from margin_amd import capi
from oracle import pairhmm as ph
from tests import extract_oracle as eo
from tests import stride_cases as sc
from tests.test_gpu_extract import assert_same
from tests.test_gpu_haplotag_aligned import assert_identical, assert_matches_oracle, chain
from tests.test_gpu_kmer_anchors import layout
from tests.test_gpu_substring_classes import arrays, host_classes
from tests.test_pairhmm import omodel

pytestmark = pytest.mark.gpu


# ---- A. extraction ----

def check_extraction(ctx, chunks, opts, want):
    """want: eo.extract's dict per chunk"""
    got, st = capi.extract_read_substrings(ctx, chunks, opts)
    assert len(got) == len(chunks) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w if "pool" in w else eo.as_arrays(w), f"chunk {i}")
    return got, st


def test_entry_and_cigar_boundaries(gpu_ctx):
    """A1 and A2 in one call, and each chunk alone: reads with 63 .. 200 entries, the delayed start carried from one pass of 64
    candidates into the next, buckets of 63 .. 129 substrings, CIGARs of 63 .. 129 ops with clips on both sides"""
    chunks = [sc.boundary_chunk(), sc.cigar_chunk()]
    want = [sc.boundary_oracle(), eo.extract([sc.cigar_chunk()], sc.OPTS)[0]]
    got, _ = check_extraction(gpu_ctx, chunks, sc.OPTS, want)
    f = sc.boundary_facts()
    assert got[0]["read_n_substrings"].tolist() == f["entries_per_read"] and got[0]["read_status"].tolist() == f["status"]
    for c in f["carry"]:                                      # the SV entry of read 0: its length comes from the carried maximum
        v = sc.LONG_START + c["candidate"]
        lo, hi = int(got[0]["entry_first"][v]), int(got[0]["entry_first"][v + 1])
        e = lo + got[0]["entry_read"][lo:hi].tolist().index(0)
        assert got[0]["entry_len"][e] == c["from_carry"] != c["own_window"]
    for i in range(2):
        check_extraction(gpu_ctx, chunks[i:i + 1], sc.OPTS, want[i:i + 1])
    check_extraction(gpu_ctx, chunks[::-1], sc.OPTS, want[::-1])


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", sc.DENSE_SEEDS)
def test_dense_chunks(gpu_ctx, seed, k):
    """A3: 90x coverage, a variant every 24 bases: reads with up to 157 entries, variants with up to 90 substrings"""
    _, st = check_extraction(gpu_ctx, [sc.dense_chunk(seed)], sc.option_sets()[k], [sc.dense_oracle(seed, k)])
    assert st.entries > 5_000


def test_more_entries_than_the_grid(gpu_ctx):
    """A4 (i): the dense chunk six times in one call, more than 65 536 entries: ex_gather_kernel's waves stride over them"""
    want = eo.as_arrays(sc.dense_oracle(0, 0))
    _, st = check_extraction(gpu_ctx, [sc.dense_chunk(0)] * 6, capi.shipped_extract_options(), [want] * 6)
    assert st.entries == 6 * len(want["entry_read"]) > sc.GRID_CAP


def test_more_variants_than_the_grid(gpu_ctx):
    """A4 (ii): 66 000 variants in one chunk, with entries on both sides of variant 65 536: ex_rank_kernel's waves stride on"""
    got, st = check_extraction(gpu_ctx, [sc.wide_chunk()], sc.OPTS, [sc.wide_oracle()])
    assert st.entries == 440 and (np.diff(got[0]["entry_first"])[sc.GRID_CAP:] > 0).sum() >= 100


# ---- B. owners and classes ----

def test_owners_past_the_grid(gpu_ctx):
    """B1: every variant of the 66 000 heterozygous: ha_owners_kernel's waves stride over the sites, and past site 65 536 some
    entries are owned by another read's entry"""
    f, r, _, _ = sc.pair_hmm_models()
    chunks, gts = [sc.wide_chunk()], [sc.wide_genotypes()]
    want = sc.wide_haplotag_oracle()
    got, st = capi.haplotag_aligned_chunks(gpu_ctx, chunks, gts, f, r, sc.OPTS)
    assert_matches_oracle(got, [want], "66 000 sites")
    sites = [s for s in want["sites"] if s[2]]
    assert st.sites == sc.WIDE_BP and st.active_sites == len(sites) and st.entries == sum(len(s[2]) for s in sites)
    assert st.owners == sum(len({bytes(x) for _, x in s[2]}) for s in sites) < st.entries
    assert_identical(got, chain(gpu_ctx, chunks, gts, sc.OPTS, f, r), "66 000 sites")


def test_classes_past_the_grid(gpu_ctx):
    """B2: 65 536 sites of no or one entry, then 40 of every shape: ec_classes_kernel's waves stride over the sites"""
    sites = sc.class_sites()
    want = host_classes(sites)
    first, pool, off, length = arrays(sites)
    got = capi.equal_substring_classes(gpu_ctx, first, pool, off, length)
    assert got.dtype == np.int32 and len(got) == len(want)
    assert (got == want).all(), np.flatnonzero(got != want)[:10]
    tail = int(first[sc.GRID_CAP])
    assert len(want) - tail > 2_000 and (want[tail:] != np.arange(tail, len(want))).any()


# ---- C. k-mer anchors ----

def check_anchors(ctx, pairs):
    pool, off = layout([s for x, y in pairs for s in (x, y)])
    aoff, anchors, _ = capi.kmer_alignment_anchors_many(ctx, pool, off[0::2], [len(x) for x, _ in pairs], off[1::2], [len(y) for _, y in pairs])
    assert aoff[0] == 0 and aoff[-1] == len(anchors)
    for i, (x, y) in enumerate(pairs):
        want = ph.kmer_anchors(x, y)
        got = anchors[aoff[i]:aoff[i + 1]]
        assert len(got) == len(want), (i, len(got), len(want))
        assert np.array_equal(got, want), i
    return aoff, anchors


def test_walk_back_through_the_workspace(gpu_ctx):
    """C1-C3: walks over more than 256 records that find their stop in every lane of a workspace pass, a best score that lies
    beyond the 64 records in registers, and a tie between the registers and the workspace; each pair alone, all in one call, and
    with x and y swapped"""
    pairs = [(x, y) for _, x, y in sc.anchor_cases()]
    for p in pairs:
        check_anchors(gpu_ctx, [p])
    check_anchors(gpu_ctx, pairs + [(y, x) for x, y in pairs] + pairs[::-1])


def test_more_pairs_than_the_grid(gpu_ctx):
    """C4: 65 536 + 64 pairs: each of the first 64 waves runs two real pairs one after the other, with short pairs in between"""
    pool, x_off, x_len, y_off, y_len, idx, real = sc.many_pairs()
    aoff, anchors, _ = capi.kmer_alignment_anchors_many(gpu_ctx, pool, x_off, x_len, y_off, y_len)
    assert aoff[0] == 0 and aoff[-1] == len(anchors)
    n_each = np.diff(aoff)
    short = np.ones(len(x_off), bool)
    short[idx] = False
    assert (n_each[short] == 0).all()                         # too short for a k-mer
    for i, (x, y) in zip(idx, real):
        want = ph.kmer_anchors(x, y)
        assert n_each[i] == len(want), (i, int(n_each[i]), len(want))
        assert np.array_equal(anchors[aoff[i]:aoff[i + 1]], want), i


# ---- D. pair-per-wave kernel ----

def test_more_wave_pairs_than_the_grid(gpu_ctx):
    """16 384 + 200 short pairs and twelve long ones under 200 models: no pair fits the pair-per-lane kernel, and the first launch
    class of the pair-per-wave kernel holds more pairs than its grid has workgroups"""
    ms = sc.many_models()
    pool, xo, xl, yo, yl, mi = sc.wave_pairs()
    out, st = capi.forward_probabilities(gpu_ctx, ms, pool, xo, xl, yo, yl, mi, expansion=4, ragged_left=True)
    ref = ph.forward_batch([omodel(m) for m in ms], pool, xo, xl, yo, yl, mi, expansion=4, ragged_left=True)
    assert st.pairs_lane == 0 and st.pairs_wave == len(xo)
    assert not np.isnan(ref).any()
    assert (out == ref).all(), np.flatnonzero(out != ref)[:10]
