"""mrp_posterior_aligned_pairs without a device: every MRP_ERR_ARG, then both MRP_ERR_UNSUPPORTED, then MRP_ERR_NO_DEVICE, in the
order include/margin_rphmm.h states; nothing is written on an error."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi
from tests import posterior_cases as pc


def call(pairs, options=None, models=None, model_index=None, ctx=None, **kw):
    pool, xo, xl, yo, yl, ao, an = pc.pack(pairs)
    for k, v in kw.items():  # overrides of the packed arrays
        if k == "x_off": xo = v
        elif k == "y_len": yl = v
        elif k == "anchor_off": ao = v
    return capi.posterior_aligned_pairs(ctx, models or [pc.model()], pool, xo, xl, yo, yl, model_index, ao, an, options or capi.PosteriorOptions())


def expect(code, text, *a, **kw):
    with pytest.raises(capi.MrpError) as e:
        call(*a, **kw)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value), str(e.value)


SMALL = [(np.array([0, 1, 2, 3], np.uint8), np.array([0, 1, 3, 3, 2], np.uint8), [])]
WIDE = [(np.zeros(2048, np.uint8), np.zeros(2048, np.uint8), [])]  # the diagonal x + y = 2048 holds 2 049 cells


def test_arg_errors():
    O = capi.PosteriorOptions
    expect(capi.MRP_ERR_ARG, "reserved", SMALL, O(reserved=1))
    expect(capi.MRP_ERR_ARG, "every cell of the band", SMALL, O(threshold=0.0))
    expect(capi.MRP_ERR_ARG, "threshold", SMALL, O(threshold=1.5))
    expect(capi.MRP_ERR_ARG, "threshold", SMALL, O(threshold=float("nan")))
    expect(capi.MRP_ERR_ARG, "diagonalExpansion", SMALL, O(expansion=3))
    expect(capi.MRP_ERR_ARG, "diagonalExpansion", SMALL, O(expansion=-2))
    expect(capi.MRP_ERR_ARG, "traceBackDiagonals must be >= 1", SMALL, O(traceback_diagonals=0))
    expect(capi.MRP_ERR_ARG, "minDiagsBetweenTraceBack", SMALL, O(min_diags_between_traceback=1, traceback_diagonals=1))
    expect(capi.MRP_ERR_ARG, "traceBackDiagonals + 1", SMALL, O(min_diags_between_traceback=5, traceback_diagonals=4))
    expect(capi.MRP_ERR_ARG, "outside the symbol pool", SMALL, x_off=np.array([7], np.int64))
    expect(capi.MRP_ERR_ARG, "outside the symbol pool", SMALL, y_len=np.array([6], np.int32))
    expect(capi.MRP_ERR_ARG, "outside the symbol pool", SMALL, y_len=np.array([-1], np.int32))
    expect(capi.MRP_ERR_ARG, "names model 1 of 1", SMALL, model_index=np.array([1], np.uint8))
    expect(capi.MRP_ERR_ARG, "invalid anchors", [(SMALL[0][0], SMALL[0][1], [(2, 2), (2, 3)])])
    expect(capi.MRP_ERR_ARG, "invalid anchors", [(SMALL[0][0], SMALL[0][1], [(4, 1)])])
    expect(capi.MRP_ERR_ARG, "anchor offsets", SMALL, anchor_off=np.array([1, 0], np.int64))


def test_null_arguments_and_gap_outputs():
    L = capi.load()
    pool, xo, xl, yo, yl, ao, an = pc.pack(SMALL)
    m = pc.model()
    o = capi.PosteriorOptions()
    match, gx, gy = capi.PosteriorPairs(), capi.PosteriorPairs(), capi.PosteriorPairs()
    p = lambda a: a.ctypes.data
    args = lambda **r: [r.get("ctx"), r.get("models", C.addressof(m)), 1, 1, p(pool), pool.size, r.get("xo", p(xo)), p(xl), p(yo), p(yl), None, None, None,
                        r.get("opt", C.byref(o)), r.get("match", C.byref(match)), r.get("gx"), r.get("gy"), None, None]
    for r in (dict(models=None), dict(opt=None), dict(match=None), dict(xo=None), dict(gx=C.byref(gx)), dict(gx=C.byref(gx), gy=C.byref(gy))):
        assert L.mrp_posterior_aligned_pairs(*args(**r)) == capi.MRP_ERR_ARG, r
    og = capi.PosteriorOptions(with_gaps=True)
    for r in (dict(opt=C.byref(og)), dict(opt=C.byref(og), gx=C.byref(gx))):
        assert L.mrp_posterior_aligned_pairs(*args(**r)) == capi.MRP_ERR_ARG, r
    assert L.mrp_posterior_aligned_pairs(*args(opt=C.byref(og), gx=C.byref(gx), gy=C.byref(gy))) == capi.MRP_ERR_NO_DEVICE
    assert not match.first and not gx.first and not gy.first  # nothing was written
    L.mrp_posterior_pairs_free(C.byref(match))  # zeroed: fine
    L.mrp_posterior_pairs_free(None)
    assert L.mrp_context_set_posterior_workspace(None, 1 << 20) == capi.MRP_ERR_ARG


def test_order_arg_then_unsupported_then_no_device():
    # a bad pair behind a wide one: the argument error comes first
    expect(capi.MRP_ERR_ARG, "invalid anchors", WIDE + [(SMALL[0][0], SMALL[0][1], [(4, 1)])])
    expect(capi.MRP_ERR_ARG, "names model", SMALL + WIDE, model_index=np.array([0, 3], np.uint8))
    # a 2 049-cell diagonal is refused before the context is looked at; 2 048 cells pass on to the next check
    expect(capi.MRP_ERR_UNSUPPORTED, "2049 cells (limit 2048", SMALL + WIDE)
    expect(capi.MRP_ERR_NO_DEVICE, "no context", [(np.zeros(2047, np.uint8), np.zeros(2047, np.uint8), [])])
    expect(capi.MRP_ERR_NO_DEVICE, "no context", SMALL)


def test_workspace_refusal_without_a_device():
    """a pair whose forward diagonals exceed the default workspace, its diagonals within 2 048 cells"""
    lx = 16000
    anchors = [(i, i) for i in range(500, lx - 100, 500)]
    o = capi.PosteriorOptions(expansion=1400)
    w, cells = capi.pair_diagonal_width(anchors, lx, lx, 1400)
    assert w <= 2048 and cells * 24 > capi.POSTERIOR_DEFAULT_WORKSPACE, (w, cells)
    s = np.zeros(lx, np.uint8)
    expect(capi.MRP_ERR_UNSUPPORTED, f"limit {capi.POSTERIOR_DEFAULT_WORKSPACE} bytes", [(s, s, anchors)], o)
    # ... and an argument error still comes first
    expect(capi.MRP_ERR_ARG, "names model", [(s, s, anchors)], o, model_index=np.array([2], np.uint8))
