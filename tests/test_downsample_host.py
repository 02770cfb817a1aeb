"""The downsampling to maxDepth on the host, no device: mrp_downsample_keep_from_extracted against the Python
restatement of the reference's branches with the LP solved in exact rationals (tests/downsample_oracle.py) -- probabilities as fp64 bits,
the mask byte for byte; the draw and alnReadLength against their restatements; the argument errors that need no context.  The fixtures
of tests/golden/downsample/ hold what the reference's own solver, lp_solve, returns for the same LP."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import downsample_cases as dc
from tests import downsample_oracle as do
from tests import extract_cases as ec
from tests import extract_oracle as xo

SYMBOLS = ["mrp_context_set_downsampling", "mrp_queue_set_downsampling", "mrp_context_last_downsampling", "mrp_downsample_draw", "mrp_aln_read_lengths",
           "mrp_downsample_keep_from_extracted", "mrp_downsample_reads"]
SEED, OS, OE = 0x5EED, 1_000_000, 1_012_000
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "downsample")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host(c, max_depth=dc.D, seed=SEED):
    return capi.downsample_keep_from_extracted(dc.extracted(c), c["h"], max_depth, seed, OS, OE)


def assert_equals_oracle(c, max_depth=dc.D, seed=SEED):
    keep, prob, did = host(c, max_depth, seed)
    wkeep, wprob, wdid, _ = do.downsample(c["status"], c["l"], c["h"], c["V"], max_depth, seed, OS, OE)
    assert did == wdid, c["name"]
    assert np.array_equal(bits(prob), bits(wprob)), (c["name"], prob, wprob)
    assert keep.dtype == np.uint8 and np.array_equal(keep, wkeep), c["name"]
    return keep, prob, did


def test_symbols_and_bindings():
    lib = capi.load()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS, s
    assert callable(capi.Context.set_downsampling) and callable(capi.Queue.set_downsampling) and callable(capi.Context.last_downsampling)
    assert capi.ABI_VERSION == 6 == lib.mrp_abi_version()  # nothing existing changes


def test_edge_cases():
    for c, expected in dc.edge_cases():
        keep, prob, did = assert_equals_oracle(c)
        want = np.array([n / d for n, d in expected], np.float64)  # (int / int: the correctly rounded quotient)
        assert np.array_equal(bits(prob), bits(want)), (c["name"], prob.tolist())
        kept = c["status"] == dc.KEPT
        assert not keep[~kept].any() and keep[kept & (prob == 1.0)].all() and not keep[prob == 0.0].any(), c["name"]
        assert did == (not c["name"].startswith(("shallow", "no kept read", "no read at all"))), c["name"]


def test_the_edge_cases_are_what_they_claim():
    cases = {c["name"]: (c, e) for c, e in dc.edge_cases()}
    c, _ = cases["total == D V exactly"]
    assert int(c["l"].sum()) == dc.D * c["V"]
    c, e = cases["B == T exactly at a read"]
    assert int(c["l"][:2].sum()) == dc.D * c["V"] and e[2] == (0, 1)
    c, e = cases["equal ratios straddle the threshold"]
    assert len({Fraction(int(h), int(l)) for h, l in zip(c["h"], c["l"])}) == 1 and e[1] == (1, 1) and e[3] == (0, 1) and 0 < e[2][0] < e[2][1]
    assert any(0 < n < d for _, e in cases.values() for n, d in e)  # a fractional p


def test_random_chunks():
    rng = np.random.default_rng(20)
    n_deep = n_fraction = n_discarded = 0
    for i in range(150):
        c = dc.random_case(rng, int(rng.integers(0, 90)), downsampled=i % 3 != 0, ties=i % 5 == 0)
        keep, prob, did = assert_equals_oracle(c, seed=i)
        n_deep += did
        n_fraction += int(((prob > 0) & (prob < 1)).sum())
        n_discarded += int(((c["status"] == dc.KEPT) & (keep == 0)).sum())
    assert n_deep > 60 and n_fraction > 40 and n_discarded > 200


def test_other_depths_and_the_seed():
    rng = np.random.default_rng(21)
    c = dc.random_case(rng, 60, downsampled=True)
    masks = []
    for depth in (1, 2, 32, 64, 1 << 40):
        keep, prob, did = assert_equals_oracle(c, max_depth=depth)
        masks.append((did, int(keep.sum())))
    assert masks[0][0] and not masks[-1][0]  # from deep to shallow as the depth grows
    # the probabilities do not depend on the seed; the mask does, at the one read a vertex of the LP leaves fractional
    c = dc.case("twenty reads of five", [5] * 20, [1000 + i for i in range(20)], 6)
    runs = [host(c, seed=s) for s in range(16)]
    frac = np.flatnonzero((runs[0][1] > 0) & (runs[0][1] < 1))
    assert len(frac) == 1
    assert all(np.array_equal(bits(r[1]), bits(runs[0][1])) for r in runs)
    assert {int(r[0][frac[0]]) for r in runs} == {0, 1}
    assert all(np.array_equal(np.delete(r[0], frac), np.delete(runs[0][0], frac)) for r in runs)


def test_sv_split_count():
    """in the SV split read_n_substrings is the one count over both classes (the merged read's vcfEntries, htsIntegration.c:1675-1719):
    the definition reads that sum and nothing per class"""
    rng = np.random.default_rng(22)
    small, sv = rng.integers(0, 20, size=30), rng.integers(0, 4, size=30)
    h = rng.integers(100, 9000, size=30)
    c = dc.case("both classes", small + sv, h, 12)
    keep, prob, did = assert_equals_oracle(c)
    assert did and ((prob > 0) & (prob < 1)).any()
    only_small = dc.case("small alone", small, h, 12)
    assert not np.array_equal(bits(host(only_small)[1]), bits(prob))


def test_draw():
    for seed, a, b, k in [(0, 0, 0, 0), (1, 2, 3, 4), (2**64 - 1, 2**62, 2**62 + 5, 10**9), (0x5EED, 1_000_000, 1_012_000, 17), (7, -5, -1, 0)]:
        u = capi.downsample_draw(seed, a, b, k)
        assert u == do.draw(seed, a, b, k) and 0.0 <= u < 1.0, (seed, a, b, k)
    us = np.array([capi.downsample_draw(3, 100, 200, k) for k in range(4000)])
    assert (us >= 0).all() and (us < 1).all() and len(set(us.tolist())) == 4000 and 0.45 < us.mean() < 0.55
    # a chunk's draws depend on the chunk alone: another chunk, another stream
    assert capi.downsample_draw(3, 100, 200, 5) != capi.downsample_draw(3, 100, 201, 5) != capi.downsample_draw(3, 101, 200, 5)
    assert do.mix(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0


def test_aln_read_lengths():
    chunks = [synth.make_aligned_chunk(seed, overlap_bp=4_000, coverage=6.0) for seed in range(3)] + [c for _, c, *_ in ec.cases()]
    n_clipped = 0
    for ch in chunks:
        got = capi.aln_read_lengths(ch)
        assert got.dtype == np.int32 and len(got) == len(ch.read_pos)
        for r in range(len(ch.read_pos)):
            cig = [int(w) for w in ch.cigar[ch.cigar_first[r]:ch.cigar_first[r + 1]]]
            if ch.l_qseq[r] <= 0 or not cig:
                assert got[r] == 0
                continue
            want, clip = xo.aligned_read_length(cig, int(ch.l_qseq[r]))
            assert got[r] == want, r
            n_clipped += clip > 0
    assert n_clipped > 0


def test_argument_errors():
    lib = capi.load()
    c = dc.edge_cases()[3][0]
    X, hold = capi.extracted_struct(dc.extracted(c))
    h = np.ascontiguousarray(c["h"], np.int32)
    keep, prob = np.zeros(2, np.uint8), np.zeros(2, np.float64)
    f = lib.mrp_downsample_keep_from_extracted
    assert f(C.byref(X), h.ctypes.data, 4, 0, 0, 10, keep.ctypes.data, prob.ctypes.data, None) == capi.MRP_OK
    assert f(C.byref(X), h.ctypes.data, 4, 0, 0, 10, keep.ctypes.data, None, None) == capi.MRP_OK  # prob_out and downsampled_out are optional
    for depth in (0, -1):
        assert f(C.byref(X), h.ctypes.data, depth, 0, 0, 10, keep.ctypes.data, None, None) == capi.MRP_ERR_ARG
    assert f(None, h.ctypes.data, 4, 0, 0, 10, keep.ctypes.data, None, None) == capi.MRP_ERR_ARG
    assert f(C.byref(X), None, 4, 0, 0, 10, keep.ctypes.data, None, None) == capi.MRP_ERR_ARG
    assert f(C.byref(X), h.ctypes.data, 4, 0, 0, 10, None, None, None) == capi.MRP_ERR_ARG
    bad = dc.extracted(dc.case("negative count", [3, -1], [5, 5], 2))
    Xb, hold_b = capi.extracted_struct(bad)
    assert f(C.byref(Xb), h.ctypes.data, 4, 0, 0, 10, keep.ctypes.data, None, None) == capi.MRP_ERR_ARG
    assert lib.mrp_aln_read_lengths(None, None) == capi.MRP_ERR_ARG
    S, hold_s = capi.aligned_chunk_struct(ec.make([ec.SNP110], [(100, "20M", 60, 0)]))
    assert lib.mrp_aln_read_lengths(C.byref(S), None) == capi.MRP_ERR_ARG
    # the setters and the getter without their object
    assert lib.mrp_context_set_downsampling(None, 4, 0) == lib.mrp_queue_set_downsampling(None, 4, 0) == capi.MRP_ERR_ARG
    assert lib.mrp_context_last_downsampling(None, None) == capi.MRP_ERR_ARG
    # the seam: its argument errors come before the context is looked at, then MRP_ERR_NO_DEVICE
    one = lambda v: np.array([v], np.int64)
    args = dict(n_reads=one(2), first=one(0), l=c["l"], h=c["h"], status=c["status"], V=one(2), max_depth=4, seed=0, overlap_start=one(0), overlap_end=one(9))
    with pytest.raises(capi.MrpError) as e:
        capi.downsample_reads(None, **args)
    assert e.value.code == capi.MRP_ERR_NO_DEVICE
    for change in (dict(max_depth=0), dict(max_depth=-3), dict(V=one(-1)), dict(l=np.array([1, -1], np.int32)), dict(n_reads=one(-1))):
        with pytest.raises(capi.MrpError) as e:
            capi.downsample_reads(None, **dict(args, **change))
        assert e.value.code == capi.MRP_ERR_ARG, change
    two = lambda a, b: np.array([a, b], np.int64)
    with pytest.raises(capi.MrpError) as e:  # the second chunk's reads begin inside the first's
        capi.downsample_reads(None, **dict(args, n_reads=two(2, 1), first=two(0, 1), V=two(2, 2), overlap_start=two(0, 0), overlap_end=two(9, 9)))
    assert e.value.code == capi.MRP_ERR_ARG


def fixtures():
    path = os.path.join(GOLDEN, "lp_solve_cases.json")
    with open(path) as f:
        return json.load(f)


def test_against_lp_solve():
    """computeReadProbsByLengthAndSecondMetric (htsIntegration.c:957-1011) run through the reference's vendored lp_solve: where the
    optimum is unique the library's p agrees within ten times the largest difference the fixtures themselves show (simplex arithmetic
    and scaling are no exact quotient); where ratios tie only the objective is compared, within the same margin"""
    fx = fixtures()
    tol = 10 * fx["largest_difference_observed"]
    assert 0 <= tol < 1e-9
    assert sum(1 for c in fx["cases"] if 8 <= len(c["l"]) <= 40) >= 12 and any(c["tied"] for c in fx["cases"]) and any(not c["tied"] for c in fx["cases"])
    for c in fx["cases"]:
        l, h, D_, V = c["l"], c["h"], c["max_depth"], c["V"]
        assert len(l) <= 40 and sum(l) > D_ * V
        keep, prob, did = capi.downsample_keep_from_extracted(dc.extracted(dc.case(c["name"], l, h, V)), h, D_, 0, 0, 1)
        assert did
        lp = np.array(c["lp_solve"], np.float64)
        if not c["tied"]:
            assert np.abs(prob - lp).max() <= tol, (c["name"], np.abs(prob - lp).max())
        scale = float(sum(h))
        assert abs(float(np.dot(prob, h)) - float(np.dot(lp, h))) <= tol * scale, c["name"]
        assert abs(float(np.dot(lp, l)) - D_ * V) <= tol * sum(l), c["name"]  # lp_solve's answer is feasible
