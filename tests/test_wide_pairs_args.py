"""Wide pairs (mrp_context_set_wide_pairs), CPU side: the five symbols are exported under the unchanged ABI, and
mrp_pair_diagonal_width -- host only, what decides a pair's kernel -- against the oracle's band."""
import numpy as np
import pytest

from margin_amd import capi
from oracle import pairhmm as ph
from tests.test_pairhmm import random_anchors

SYMBOLS = ["mrp_context_set_wide_pairs", "mrp_context_wide_pair_count", "mrp_queue_set_wide_pairs", "mrp_queue_wide_pair_count",
           "mrp_pair_diagonal_width"]


def test_symbols_are_exported_and_the_abi_is_unchanged():
    lib = capi.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTED_SYMBOLS, s
    assert capi.ABI_VERSION == 6 and lib.mrp_abi_version() == 6
    for name in ("set_wide_pairs", "wide_pair_count"):
        assert callable(getattr(capi.Context, name)) and callable(getattr(capi.Queue, name))
    assert capi.WIDE_MAX_WIDTH == 32768 and capi.WIDE_MAX_CELLS == 2 ** 31


def test_the_setters_refuse_a_null_handle():
    lib = capi.load()
    assert lib.mrp_context_set_wide_pairs(None, 1) == capi.MRP_ERR_ARG
    assert lib.mrp_context_wide_pair_count(None, None, None) == capi.MRP_ERR_ARG
    assert lib.mrp_queue_set_wide_pairs(None, 1) == capi.MRP_ERR_ARG
    assert lib.mrp_queue_wide_pair_count(None, None, None) == capi.MRP_ERR_ARG


def test_width_and_cells_equal_the_oracles_band():
    rng = np.random.default_rng(31)
    n_anchored = 0
    for _ in range(300):
        lx, ly = int(rng.integers(0, 160)), int(rng.integers(0, 160))
        anchors = random_anchors(rng, lx, ly) if rng.random() < 0.8 else []
        n_anchored += bool(anchors)
        e = 2 * int(rng.integers(0, 12))
        lo, hi = ph.band(anchors, lx, ly, e)
        widths = (hi.astype(np.int64) - lo) // 2 + 1
        assert capi.pair_diagonal_width(anchors, lx, ly, e) == (int(widths.max()), int(widths.sum()))
    assert n_anchored > 100


def test_without_anchors_it_is_the_whole_matrix():
    for lx, ly in ((0, 0), (0, 9), (9, 0), (1, 1), (7, 4), (4, 7), (2047, 2047), (2048, 2048), (2048, 2300), (30_000, 200_000)):
        assert capi.pair_diagonal_width([], lx, ly, 4) == (min(lx, ly) + 1, (lx + 1) * (ly + 1))
        assert capi.pair_diagonal_width(None, lx, ly, 0) == (min(lx, ly) + 1, (lx + 1) * (ly + 1))
    lo, hi = ph.band([], 7, 4, 4)
    assert capi.pair_diagonal_width([], 7, 4, 4) == (int(((hi - lo) // 2 + 1).max()), int(((hi - lo) // 2 + 1).sum()))


def test_either_output_may_be_null():
    import ctypes as C
    lib = capi.load()
    w, c = C.c_int32(), C.c_int64()
    assert lib.mrp_pair_diagonal_width(None, 0, 5, 3, 4, C.byref(w), None) == capi.MRP_OK and w.value == 4
    assert lib.mrp_pair_diagonal_width(None, 0, 5, 3, 4, None, C.byref(c)) == capi.MRP_OK and c.value == 24


def test_bad_arguments_as_band_diagonals():
    for anchors, e in (([], 3), ([(1, 1)], 5),                                            # odd expansion, pairwiseAligner.c:179
                       ([(3, 3), (3, 4)], 2), ([(2, 2), (1, 5)], 2), ([(6, 0)], 2), ([(0, 5)], 2)):  # asserts :206-211
        with pytest.raises(capi.MrpError) as err:
            capi.pair_diagonal_width(anchors, 6, 5, e)
        assert err.value.code == capi.MRP_ERR_ARG
        with pytest.raises(capi.MrpError):
            capi.band_diagonals(anchors, 6, 5, e)
    with pytest.raises(capi.MrpError) as err:
        capi.pair_diagonal_width([], -1, 5, 2)
    assert err.value.code == capi.MRP_ERR_ARG
