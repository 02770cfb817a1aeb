"""mrp_ml_repeat_counts and mrp_rle_expand without a device: the exports and their transcription, every MRP_ERR_ARG (raised before the
context is looked at, nothing written: capi.ml_repeat_counts asserts that its pre-filled outputs come back untouched), the NULL context
behind them, mrp_rle_expand against mrp_rle_compress, and the properties of the restatement (tests/repeat_count_oracle.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from margin_amd import capi
from tests import repeat_count_cases as cases
from tests import repeat_count_oracle as rco
from tests import rle_cases as rc
from tests import rle_pairhmm_oracle as ro

WHO = "mrp_ml_repeat_counts"


def test_symbols_exported_and_transcribed():
    lib = capi.load()
    for name in ("mrp_ml_repeat_counts", "mrp_rle_expand"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6  # additions only
    assert C.sizeof(capi.RepeatCountOptions) == 24 and C.sizeof(capi.RepeatCountStats) == 9 * 8


# ---- the argument errors ------------------------------------------------------------------------------------------------------------

def small():
    """two consensus strings: 3 nodes under 2 reads, 2 nodes under 1 read"""
    a = cases.consensus([0, 1, 4], [[1, 2, 3], [2, 9]], [1, 0], [[(0, 0, 5), (1, 1, 7), (2, 2, 1)], [(0, 0, 3), (1, 1, 4)]], [0, 1])
    b = cases.consensus([2, 3], [[1, 1]], [1], [[(0, 0, 9), (1, 1, 9)]])
    return [a, b]


def call(p=None, table=None, ctx=None, **kw):
    p = dict(cases.pack(small()) if p is None else p)
    p.update({k: kw.pop(k) for k in list(kw) if k in p})
    return capi.ml_repeat_counts(ctx, np.zeros((4, 4, 4)) if table is None else table, **p, **kw)


def expect(code, text, **kw):
    with pytest.raises(capi.MrpError) as e:
        call(**kw)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value) and WHO in str(e.value), str(e.value)


def test_null_context_comes_after_the_checks():
    expect(capi.MRP_ERR_NO_DEVICE, "no context")
    expect(capi.MRP_ERR_NO_DEVICE, "no context", read_in_hap=np.array([1, 0, 1], np.uint8), log_het_substitution=-math.inf, walk_backwards=True)
    expect(capi.MRP_ERR_NO_DEVICE, "no context", table=np.full((4, 255, 255), -np.inf))  # -inf is a log probability
    expect(capi.MRP_ERR_NO_DEVICE, "no context", p=cases.pack([]))


@pytest.mark.parametrize("name", ["log_prob", "node_first", "read_first", "matches", "first", "opt", "symbols", "repeat_count_out", "non_rle_length_out", "y_off",
                                  "y_len", "read_forward_strand", "x", "counts"])
def test_null_arguments(name):
    expect(capi.MRP_ERR_ARG, "null", nulls=(name,))


def test_sizes_table_and_options():
    for R in (1, 0, -2, 256):
        expect(capi.MRP_ERR_ARG, f"max_repeat {R} outside [2, 255]", max_repeat=R)
    t = np.zeros((4, 4, 4))
    t[2, 1, 3] = np.nan
    expect(capi.MRP_ERR_ARG, "log_prob[2][1][3] is NaN", table=t)
    t[2, 1, 3] = np.inf
    expect(capi.MRP_ERR_ARG, "log_prob[2][1][3] is +inf", table=t)
    expect(capi.MRP_ERR_ARG, "reserved", reserved=1)
    expect(capi.MRP_ERR_ARG, "reserved", reserved2=-1)
    expect(capi.MRP_ERR_ARG, "walk_backwards", walk_backwards=2)
    expect(capi.MRP_ERR_ARG, "log_het_substitution is NaN", read_in_hap=np.zeros(3, np.uint8), log_het_substitution=math.nan)
    expect(capi.MRP_ERR_NO_DEVICE, "no context", log_het_substitution=math.nan)  # unphased: s is not read


def test_offsets():
    p = cases.pack(small())
    expect(capi.MRP_ERR_ARG, "begin at 0", node_first=p["node_first"] + 1)
    expect(capi.MRP_ERR_ARG, "begin at 0", read_first=p["read_first"] + 1)
    expect(capi.MRP_ERR_ARG, "consensus 1: node_first or read_first descends", node_first=np.array([0, 3, 2], np.int64))
    expect(capi.MRP_ERR_ARG, "consensus 0: node_first or read_first descends", read_first=np.array([0, -1, 3], np.int64))
    m = dict(p["matches"])
    m["first"] = p["matches"]["first"] + 1
    expect(capi.MRP_ERR_ARG, "matches->first must begin at 0", matches=m)
    m["first"] = np.array([0, 3, 2, 7], np.int64)
    expect(capi.MRP_ERR_ARG, "read 1: matches->first descends", matches=m)
    expect(capi.MRP_ERR_ARG, "outside the pool", y_off=np.array([0, 3, 6], np.int64))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1: its counts lie outside the pool", y_len=np.array([3, -1, 2], np.int32))
    expect(capi.MRP_ERR_ARG, "node 1: symbol 5 above 4", symbols=np.array([0, 5, 4, 2, 3], np.uint8))


def test_matches_are_checked_and_named():
    p = cases.pack(small())

    def changed(key, at, value):
        m = {k: v.copy() for k, v in p["matches"].items()}
        m[key][at] = value
        return m

    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, match 4: y 2 outside the read (2 counts)", matches=changed("y", 4, 2))
    expect(capi.MRP_ERR_ARG, "consensus 1, read 2, match 5: y -1 outside the read", matches=changed("y", 5, -1))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, match 4: x 2 + x_shift 1 outside the consensus (3 nodes)", matches=changed("x", 4, 2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, match 0: x -1 + x_shift 0 outside", matches=changed("x", 0, -1))
    expect(capi.MRP_ERR_ARG, "consensus 1, read 2, match 6: x 2 + x_shift 0 outside the consensus (2 nodes)", matches=changed("x", 6, 2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, match 2: x 2 + x_shift 1 outside", x_shift=np.array([1, 1, 0], np.int32))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, match 1: negative weight -7", matches=changed("weight", 1, -7))
    expect(capi.MRP_ERR_NO_DEVICE, "no context", matches=changed("weight", 1, 0), x_shift=None)  # a weight of 0 and a NULL x_shift are fine
    expect(capi.MRP_ERR_NO_DEVICE, "no context", counts=np.array([255, 4, 200, 0, 9, 1, 1], np.uint8))  # counts of R and more are accepted


# ---- mrp_rle_expand -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", ["", "A", "GGGGGGGGGT", "CCCAAAACCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCC", "ACGTNNNACGT", "T" * 255 + "ACGT" * 20])
def test_rle_expand_round_trips_rle_compress(s):
    sym, cnt = capi.rle_compress(s, 256)
    assert capi.rle_expand(sym, cnt) == s == rco.rle_expand(sym, cnt)
    assert capi.rle_expand(sym, cnt.astype(np.int32)) == s  # the int32 counts of repeat_count_out
    assert ro.rle_compress(s, 256) == (sym.tolist(), cnt.tolist())


def test_rle_expand_refuses():
    L = capi.load()
    sym, c8, c32 = np.array([0, 5], np.uint8), np.array([1, 1], np.uint8), np.array([1, -1], np.int32)
    ok = np.array([0, 4], np.uint8)
    out = C.create_string_buffer(b"zzzz", 4)
    assert L.mrp_rle_expand(ok.ctypes.data, c8.ctypes.data, None, -1, out, 4) == -1
    assert L.mrp_rle_expand(None, c8.ctypes.data, None, 2, out, 4) == -1
    assert L.mrp_rle_expand(ok.ctypes.data, None, None, 2, out, 4) == -1
    assert L.mrp_rle_expand(ok.ctypes.data, c8.ctypes.data, c32.ctypes.data, 2, out, 4) == -1
    assert L.mrp_rle_expand(sym.ctypes.data, c8.ctypes.data, None, 2, out, 4) == -1  # a symbol above 4
    assert L.mrp_rle_expand(ok.ctypes.data, None, c32.ctypes.data, 2, out, 4) == -1  # a negative count
    assert L.mrp_rle_expand(ok.ctypes.data, c8.ctypes.data, None, 2, out, 1) == -1  # too small
    assert out.raw == b"zzzz"
    assert L.mrp_rle_expand(ok.ctypes.data, c8.ctypes.data, None, 2, None, 0) == 2  # a sizing call
    assert L.mrp_rle_expand(None, None, None, 0, None, 0) == 0
    assert L.mrp_rle_expand(ok.ctypes.data, c8.ctypes.data, None, 2, out, 4) == 2 and out.raw == b"ANzz"


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def diagonal_table(R):
    """every row's maximum on the diagonal, every base"""
    t = -np.abs(np.arange(R)[:, None] - np.arange(R)[None, :]) * 0.7 - 0.1
    return np.broadcast_to(t, (4, R, R)).copy()


def test_single_observation_on_a_diagonal_table_gives_its_count():
    R = 9
    for c in range(R):
        for strand in (0, 1):
            one = cases.consensus([2], [[c]], [strand], [[(0, 0, 1234567)]])
            w = cases.want(diagonal_table(R), [one])
            assert w["count"].tolist() == [max(c, 1)] and w["candidates"] == 1
            assert w["log_prob"][0] == (0.0 + -0.1 * 1234567.0) / 1e7


def test_node_without_observations_and_overlong_only():
    R = 6
    c = cases.consensus([0, 1, 2], [[7, 6, 200]], [1], [[(1, 0, 5), (1, 1, 5), (1, 2, 5)]])
    for hap in (None, [np.array([1], np.uint8)]):
        w = cases.want(diagonal_table(R), [c], hap=hap, s=cases.S_SHIPPED)
        assert w["count"].tolist() == [1, 1, 1] and np.isneginf(w["log_prob"]).all()
        assert (w["non_rle_length"].tolist(), w["observations"], w["nodes_observed"], w["candidates"]) == ([3], 3, 1, 0)


def test_mixed_overlong_is_clamped_and_min_ignores_it():
    R = 6
    obs = [(0, 0, 1), (0, 1, 1), (0, 2, 1)]
    assert rco.min_and_max(R, obs, [[9, 3, 4]]) == (3, 5)
    assert rco.min_and_max(R, obs, [[3, 3, 3]]) == (3, 3)
    assert rco.min_and_max(R, [], [[]]) == (R, 0)


def test_strand_picks_the_complement_slice_and_n_counts_as_a():
    t = np.arange(4 * 3 * 3, dtype=np.float64).reshape(4, 3, 3)
    assert rco.table_slice(t, 1, True) is not None and (rco.table_slice(t, 1, True) == t[1]).all() and (rco.table_slice(t, 1, False) == t[2]).all()
    assert (rco.table_slice(t, 4, True) == t[0]).all() and (rco.table_slice(t, 4, False) == t[3]).all()


def test_walk_backwards_reverses_inside_a_read_only():
    m = [[(0, 0, 1), (0, 1, 2), (1, 2, 3)], [(0, 0, 4), (0, 1, 5)]]
    assert rco.observations(2, m)[0] == [(0, 0, 1), (0, 1, 2), (1, 0, 4), (1, 1, 5)]
    assert rco.observations(2, m, walk_backwards=True)[0] == [(0, 1, 2), (0, 0, 1), (1, 1, 5), (1, 0, 4)]
    assert rco.observations(3, m, x_shift=[1, 0])[1] == [(0, 0, 1), (0, 1, 2)]


def test_phased_with_everybody_in_the_hap_is_the_unphased_argmax_but_for_ties():
    # s = -inf and an empty other side: lp2 = 0.0 throughout, ml2 + s = -inf, p(u) = lp1[u] + 0.0
    table, call = cases.edge_table(), cases.edge_call()
    all_in = [np.ones(len(c["read_counts"]), np.uint8) for c in call]
    un = cases.want_cached("edge", table, call)
    ph = cases.want_cached("edge", table, call, hap=all_in, s=-math.inf)
    twins = cases.EDGE_NODES["twins"]
    differ = np.flatnonzero(un["count"] != ph["count"]).tolist()
    # an exact tie: the candidates 4 and 5 have identical rows -- > keeps the first, >= takes the last
    assert un["count"][twins] == 4 and ph["count"][twins] == 5 and un["log_prob"][twins] == ph["log_prob"][twins]
    for k in differ:  # whatever else differs is a tie too (all candidates at -inf)
        assert un["log_prob"][k] == ph["log_prob"][k]
    assert twins in differ
    same = np.ones(len(un["count"]), bool)
    same[differ] = False
    assert np.array_equal((un["log_prob"] + 0.0)[same].view(np.int64), ph["log_prob"][same].view(np.int64))


def test_the_edge_call_holds_its_edges():
    table, call = cases.edge_table(), cases.edge_call()
    assert [len(c["symbols"]) for c in call] == [0, len(cases.EDGE_NODES), 5] and [len(c["read_counts"]) for c in call] == [0, 1129, 0]
    main, N = call[1], cases.EDGE_NODES
    obs = rco.observations(len(main["symbols"]), main["matches"], main["x_shift"])
    assert [len(obs[N[k]]) for k in ("none", "one", "n63", "n64", "n65", "n129", "n1000")] == [0, 1, 63, 64, 65, 129, 1000]
    assert sorted(r for r, _, _ in obs[N["same_x"]]) == [0, 0, 1, 1, 1, 2, 3] and main["symbols"][N["n_base"]] == 4
    assert len({int(main["strands"][r]) for r, _, _ in obs[N["n_base"]]}) == 2
    w = cases.want_cached("edge", table, call)
    assert w["count"][N["zero"]] == 1 and np.isfinite(w["log_prob"][N["zero"]])
    assert w["count"][N["overlong"]] == 1 and np.isneginf(w["log_prob"][N["overlong"]])
    assert rco.min_and_max(cases.EDGE_R, obs[N["mixed"]], main["read_counts"]) == (2, cases.EDGE_R - 1)
    assert w["count"][len(N):].tolist() == [1] * 5 and w["non_rle_length"][0] == 0 and w["non_rle_length"][2] == 5
    assert not np.isnan(w["log_prob"]).any()
