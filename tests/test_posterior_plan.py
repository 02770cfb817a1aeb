"""mrp_posterior_tracebacks (host only): where getPosteriorProbsWithBanding traces back (impl/pairwiseAligner.c:746-749, :768, :819),
against the sequential restatement, on the shapes of the GPU tests and on random bands."""
import numpy as np
import pytest

from margin_amd import capi
from tests import posterior_cases as pc
from tests import posterior_oracle as po


def plan(anchors, lx, ly, kw):
    return [tuple(int(v) for v in t) for t in capi.posterior_tracebacks(anchors, lx, ly, pc.options(kw, 0.01, False))]


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_plan_of_the_cases(name):
    sx, sy, anchors, kw = pc.CASES[name]
    want = po.tracebacks(len(sx), len(sy), anchors, kw["expansion"], kw["min_diags"], kw["traceback_diagonals"])
    assert plan(anchors, len(sx), len(sy), kw) == want
    # the restatement's own loop, with its arithmetic and its asserts, traces back at the same places
    assert [i[:3] for i in pc.expected(name, 0.2)[1]] == want


def test_plan_known_answers():
    """a traceback every 3 diagonals; the width rule postponing one"""
    assert [t[0] for t in plan([], 12, 9, dict(expansion=10, min_diags=6, traceback_diagonals=2))] == [6, 9, 12, 15, 18, 21]
    assert plan([], 12, 9, dict(expansion=10, min_diags=6, traceback_diagonals=2))[:2] == [(6, 0, 3), (9, 3, 6)]
    assert [t[0] for t in plan([], 12, 13, dict(expansion=2, min_diags=4, traceback_diagonals=1))] == [4, 21, 23, 25]
    assert plan([], 0, 0, dict(expansion=2, min_diags=4, traceback_diagonals=1)) == []
    assert plan([], 1, 0, dict(expansion=2, min_diags=4, traceback_diagonals=1)) == [(1, 0, 1)]
    assert len(plan(pc.CASES["6_160_e4"][2], 160, len(pc.CASES["6_160_e4"][1]), pc.CASES["6_160_e4"][3])) == 8


def test_plan_random():
    """lx, ly <= 100, parameters as tests/pairwiseAlignerTest.c:433-435 draws them, random valid anchors"""
    rng = np.random.default_rng(77)
    for _ in range(200):
        lx, ly = int(rng.integers(0, 101)), int(rng.integers(0, 101))
        tb = int(rng.integers(1, 11))
        kw = dict(traceback_diagonals=tb, min_diags=tb + int(rng.integers(2, 11)), expansion=2 * int(rng.integers(0, 11)))
        anchors = pc.random_anchors(rng, lx, ly) if rng.random() < 0.7 else []
        want = po.tracebacks(lx, ly, anchors, kw["expansion"], kw["min_diags"], kw["traceback_diagonals"])
        assert plan(anchors, lx, ly, kw) == want
        if want:
            assert want[-1][0] == lx + ly and want[-1][2] == lx + ly and want[0][1] == 0
            assert all(a[2] == b[1] for a, b in zip(want, want[1:]))


def test_plan_capacity_and_errors():
    o = capi.PosteriorOptions(expansion=10, min_diags_between_traceback=6, traceback_diagonals=2)
    import ctypes as C
    n = C.c_int64()
    out = np.zeros((2, 3), dtype=np.int64)
    L = capi.load()
    assert L.mrp_posterior_tracebacks(None, 0, 12, 9, C.byref(o), out.ctypes.data, 2, C.byref(n)) == 0
    assert n.value == 6 and out.tolist() == [[6, 0, 3], [9, 3, 6]]
    assert L.mrp_posterior_tracebacks(None, 0, 12, 9, C.byref(o), None, 0, C.byref(n)) == 0 and n.value == 6
    for bad in (dict(expansion=3), dict(min_diags_between_traceback=3, traceback_diagonals=2), dict(traceback_diagonals=0), dict(threshold=0.0),
                dict(reserved=1)):
        with pytest.raises(capi.MrpError) as e:
            capi.posterior_tracebacks([], 5, 5, capi.PosteriorOptions(**bad))
        assert e.value.code == capi.MRP_ERR_ARG
    with pytest.raises(capi.MrpError) as e:
        capi.posterior_tracebacks([(3, 3), (3, 4)], 6, 5, capi.PosteriorOptions())
    assert e.value.code == capi.MRP_ERR_ARG
