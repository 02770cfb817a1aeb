"""The dynamic anchor band on the host (band_constructDynamic, impl/pairwiseAligner.c:120-173): mrp_band_diagonals_dynamic,
mrp_pair_diagonal_width_dynamic and mrp_posterior_tracebacks_dynamic against the restatement of tests/posterior_dynamic_oracle.py, and
what mrp_posterior_aligned_pairs_dynamic and the posterior wide switch decide without a device."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi
from tests import posterior_cases as pc
from tests import posterior_dynamic_oracle as pdo
from tests import posterior_oracle as po

N_DRAWS = 300


def draws(seed=120, n=N_DRAWS):
    """lengths 0 .. 100, anchors as getRandomAnchorPairs draws them, an even expansion 0 .. 20 per anchor"""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        lx, ly = int(rng.integers(0, 101)), int(rng.integers(0, 101))
        anchors = pc.random_anchors(rng, lx, ly)
        yield lx, ly, anchors, pdo.random_expansions(rng, len(anchors))


def test_band_agrees_with_the_restatement():
    anchored = 0
    for lx, ly, anchors, exps in draws():
        lo, hi = pdo.band_dynamic(anchors, exps, lx, ly)
        got_lo, got_hi = capi.band_diagonals_dynamic(anchors, lx, ly, exps)
        assert np.array_equal(got_lo, lo) and np.array_equal(got_hi, hi), (lx, ly, anchors, exps)
        widths = (hi - lo) // 2 + 1
        assert capi.pair_diagonal_width_dynamic(anchors, lx, ly, exps) == (int(widths.max()), int(widths.sum()))
        anchored += len(anchors) > 0
    assert anchored > N_DRAWS // 2


def test_equal_expansions_give_the_constant_band():
    for lx, ly, anchors, _ in draws(seed=121, n=100):
        for e in (0, 2, 8, 20):
            lo, hi = capi.band_diagonals(anchors, lx, ly, e)
            got = capi.band_diagonals_dynamic(anchors, lx, ly, [e] * len(anchors))
            assert np.array_equal(got[0], lo) and np.array_equal(got[1], hi), (lx, ly, anchors, e)
    for lx, ly in ((0, 0), (0, 7), (9, 0), (13, 11)):  # no anchors at all: expansion 0, still the whole matrix, as every constant band is
        got = capi.band_diagonals_dynamic([], lx, ly, [])
        for e in (0, 4, 20):
            lo, hi = capi.band_diagonals([], lx, ly, e)
            assert np.array_equal(got[0], lo) and np.array_equal(got[1], hi)
        assert capi.pair_diagonal_width_dynamic([], lx, ly, []) == (min(lx, ly) + 1, (lx + 1) * (ly + 1))


def test_some_band_differs_from_every_constant_band():
    """the per-anchor path is really taken: a drawn band no single expansion gives"""
    found = 0
    for lx, ly, anchors, exps in draws():
        if len(set(exps)) < 2:
            continue
        lo, hi = capi.band_diagonals_dynamic(anchors, lx, ly, exps)
        constant = [capi.band_diagonals(anchors, lx, ly, e) for e in range(0, 22, 2)]
        found += all(not (np.array_equal(lo, cl) and np.array_equal(hi, ch)) for cl, ch in constant)
    assert found > 0


def test_the_expansion_belongs_to_the_stretch_that_ends_at_its_anchor():
    """two anchors on the main diagonal of a 40 x 40 matrix: the first stretch has anchor 0's expansion, everything behind anchor 1 has anchor 1's"""
    lo, hi = capi.band_diagonals_dynamic([(9, 9), (24, 24)], 40, 40, [0, 12])
    c0, c12 = capi.band_diagonals([(9, 9), (24, 24)], 40, 40, 0), capi.band_diagonals([(9, 9), (24, 24)], 40, 40, 12)
    assert np.array_equal(lo[:21], c0[0][:21]) and np.array_equal(hi[:21], c0[1][:21])      # diagonals 0 .. 20, up to anchor 0 at (10, 10)
    assert np.array_equal(lo[21:], c12[0][21:]) and np.array_equal(hi[21:], c12[1][21:])    # the rest, the tail behind the last anchor included
    assert not np.array_equal(lo, c0[0]) and not np.array_equal(lo, c12[0])


def test_tracebacks_agree_with_the_restatement():
    rng = np.random.default_rng(122)
    several = 0
    for lx, ly, anchors, exps in draws(seed=123, n=150):
        tb = int(rng.integers(1, 11))
        kw = dict(traceback_diagonals=tb, min_diags=tb + int(rng.integers(2, 11)), expansion=2 * int(rng.integers(0, 11)))
        want = pdo.tracebacks_dynamic(lx, ly, anchors, exps, **kw)
        got = capi.posterior_tracebacks_dynamic(anchors, exps, lx, ly, pc.options(kw, 0.01, False))
        assert [tuple(r) for r in got.tolist()] == want, (lx, ly, anchors, exps, kw)
        several += len(want) > 2
    assert several > 20


def test_restatement_runs_over_the_dynamic_band_and_puts_the_band_back():
    from oracle import pairhmm as ph
    saved = ph.band
    sx, sy, anchors, kw = pc.CASES["6_160_e4"]
    exps = [0, 8, 2, 12, 4, 6][:len(anchors)]
    assert len(exps) == len(anchors)
    dyn, _ = pdo.posterior_dynamic(pc.model(), sx, sy, anchors, exps, threshold=0.01, with_gaps=True, **kw)
    assert ph.band is saved
    const, _ = po.posterior(pc.model(), sx, sy, anchors, threshold=0.01, with_gaps=True, **kw)
    assert dyn != const and len(dyn[0]) > 0


def expect_arg(fn, *a):
    with pytest.raises(capi.MrpError) as e:
        fn(*a)
    assert e.value.code == capi.MRP_ERR_ARG, str(e.value)
    return str(e.value)


def test_argument_errors():
    for bad in (3, -2, -1, 7):  # odd or negative where the reference asserts (:157-158), whichever anchor carries it
        for exps in ([bad, 4], [4, bad]):
            assert "expansion" in expect_arg(capi.band_diagonals_dynamic, [(2, 2), (6, 7)], 10, 10, exps)
            assert "expansion" in expect_arg(capi.pair_diagonal_width_dynamic, [(2, 2), (6, 7)], 10, 10, exps)
            assert "expansion" in expect_arg(capi.posterior_tracebacks_dynamic, [(2, 2), (6, 7)], exps, 10, 10, capi.PosteriorOptions())
    # the anchor checks are mrp_band_diagonals': not increasing, outside the matrix, left over behind (lx, ly)
    for anchors in ([(4, 4), (4, 6)], [(4, 4), (3, 6)], [(10, 3)], [(3, 10)], [(9, 9), (10, 10)]):
        expect_arg(capi.band_diagonals, anchors, 10, 10, 4)
        expect_arg(capi.band_diagonals_dynamic, anchors, 10, 10, [4] * len(anchors))
    L = capi.load()
    lo = np.zeros(21, np.int32)
    a, e = np.array([2, 2], np.int64), np.array([4], np.int64)
    assert L.mrp_band_diagonals_dynamic(a.ctypes.data, 1, 10, 10, None, lo.ctypes.data, lo.ctypes.data) == capi.MRP_ERR_ARG
    assert L.mrp_band_diagonals_dynamic(None, 1, 10, 10, e.ctypes.data, lo.ctypes.data, lo.ctypes.data) == capi.MRP_ERR_ARG
    assert L.mrp_band_diagonals_dynamic(a.ctypes.data, 1, 10, 10, e.ctypes.data, None, lo.ctypes.data) == capi.MRP_ERR_ARG
    assert L.mrp_band_diagonals_dynamic(a.ctypes.data, -1, 10, 10, e.ctypes.data, lo.ctypes.data, lo.ctypes.data) == capi.MRP_ERR_ARG
    assert L.mrp_pair_diagonal_width_dynamic(a.ctypes.data, 1, 10, 10, None, None, None) == capi.MRP_ERR_ARG
    assert L.mrp_pair_diagonal_width_dynamic(a.ctypes.data, 1, 10, 10, e.ctypes.data, None, None) == capi.MRP_OK
    # the options keep their checks in dynamic mode: opt->expansion is still what :748 reads
    assert "diagonalExpansion" in expect_arg(capi.posterior_tracebacks_dynamic, [], [], 10, 10, capi.PosteriorOptions(expansion=3))


SMALL = [(np.array([0, 1, 2, 3], np.uint8), np.array([0, 1, 3, 3, 2], np.uint8), [(1, 1)])]
WIDE = [(np.zeros(2048, np.uint8), np.zeros(2048, np.uint8), [])]  # the diagonal x + y = 2048 holds 2 049 cells


def entry_error(pairs, expansions, options=None, dynamic=True, model_index=None):
    pool, xo, xl, yo, yl, ao, an = pc.pack(pairs)
    with pytest.raises(capi.MrpError) as e:
        capi.posterior_aligned_pairs(None, [pc.model()], pool, xo, xl, yo, yl, model_index, ao, an, options or capi.PosteriorOptions(),
                                     anchor_expansion=expansions, dynamic=dynamic)
    return e.value.code, str(e.value)


def test_entry_error_order_without_a_device():
    code, text = entry_error(SMALL, [4], capi.PosteriorOptions(expansion=3))
    assert code == capi.MRP_ERR_ARG and "diagonalExpansion" in text and "mrp_posterior_aligned_pairs_dynamic" in text
    for bad in (3, -2):
        code, text = entry_error(WIDE + SMALL, [bad])  # an argument error behind a wide pair comes first
        assert code == capi.MRP_ERR_ARG and "pair 1" in text and "expansion" in text
    code, text = entry_error(SMALL + WIDE, [4], model_index=np.array([0, 3], np.uint8))
    assert code == capi.MRP_ERR_ARG and "names model" in text
    code, text = entry_error(SMALL + WIDE, [4])
    assert code == capi.MRP_ERR_UNSUPPORTED and "2049 cells (limit 2048" in text
    code, text = entry_error(SMALL, [4])
    assert code == capi.MRP_ERR_NO_DEVICE and "no context" in text
    # anchors without their expansions
    L = capi.load()
    pool, xo, xl, yo, yl, ao, an = pc.pack(SMALL)
    m, o, match = pc.model(), capi.PosteriorOptions(), capi.PosteriorPairs()
    p = lambda a: a.ctypes.data
    rc = L.mrp_posterior_aligned_pairs_dynamic(None, C.addressof(m), 1, 1, p(pool), pool.size, p(xo), p(xl), p(yo), p(yl), None, p(ao), p(an), None, C.byref(o),
                                               C.byref(match), None, None, None, None)
    assert rc == capi.MRP_ERR_ARG and not match.first


def test_wide_pair_is_refused_with_a_null_context_as_before():
    """a NULL context counts as the posterior wide switch off: the 2 049-cell pair of tests/test_posterior_args.py, both entries"""
    for dynamic in (False, True):
        code, text = entry_error(WIDE, [] if dynamic else None, dynamic=dynamic)
        assert code == capi.MRP_ERR_UNSUPPORTED and "2049 cells (limit 2048; wide pairs are not extended to this entry)" in text
    L = capi.load()
    assert L.mrp_context_set_posterior_wide_pairs(None, 1) == capi.MRP_ERR_ARG
    assert L.mrp_context_posterior_wide_count(None, None, None) == capi.MRP_ERR_ARG


def test_symbols_and_abi():
    L = capi.load()
    for name in ("mrp_band_diagonals_dynamic", "mrp_pair_diagonal_width_dynamic", "mrp_posterior_tracebacks_dynamic", "mrp_posterior_aligned_pairs_dynamic",
                 "mrp_context_set_posterior_wide_pairs", "mrp_context_posterior_wide_count"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    assert capi.ABI_VERSION == L.mrp_abi_version() == 6
