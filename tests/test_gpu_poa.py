"""mrp_poa_augment on the device against the sequential restatement (tests/poa_oracle.py): every weight as a bit pattern, the picks, the
inserts and deletes of every node in the reference's order of creation with their strings, the totals and the stats' counts
(tests/poa_cases.py's assert_equal), and mrp_poa_consensus over the device's arrays, at the smallest shapes at which the kernels can go
wrong."""
import json
import os

import numpy as np
import pytest

from margin_amd import capi
from tests import poa_cases as cases
from tests import poa_edge_cases as edge
from tests import posterior_cases as pc
from tests import rle_cases as rc

pytestmark = pytest.mark.gpu


def test_the_references_vector(gpu_ctx):
    with open(os.path.join(os.path.dirname(__file__), "golden", "poa", "augment_example.json")) as f:
        v = json.load(f)
    swap = lambda l: [(x, y, w) for w, x, y in l]
    call = [cases.consensus(cases.SYM(v["reference"]), None,
                            [cases.read(cases.SYM(v["read"]), [1] * len(v["read"]), 1, swap(v["matches"]), swap(v["deletes"]), swap(v["inserts"]))])]
    got = cases.run(gpu_ctx, call, 51, merge=False)
    w, _, st = cases.want(call, 51, merge=False)
    cases.assert_equal(got, w, st)
    for k, node in enumerate(v["nodes"]):
        assert got["base_weight"][k].tolist() == node["base_weights"]
        lo, hi = got["insert_first"][k], got["insert_first"][k + 1]
        strings = ["".join("ACGTN"[b] for b in got["pool_symbols"][o:o + n]) for o, n in zip(got["insert_str_off"][lo:hi], got["insert_str_len"][lo:hi])]
        assert [[s, wt] for s, wt in zip(strings, got["insert_weight_forward"][lo:hi].tolist())] == node["inserts"]
        lo, hi = got["delete_first"][k], got["delete_first"][k + 1]
        assert [[n, wt] for n, wt in zip(got["delete_length"][lo:hi].tolist(), got["delete_weight_forward"][lo:hi].tolist())] == node["deletes"]


# ---- runs, shifts, grouping and order, weights: one call of three consensus strings per option set (what each case claims is asserted
# on the restatement's own trace by tests/test_poa_host.py::test_the_edge_call_holds_what_it_claims) ----

@pytest.mark.parametrize("compare,merge", [(True, True), (False, True), (True, False), (False, False)])
def test_edges_in_one_call_of_three_consensus_strings(gpu_ctx, compare, merge):
    call = edge.edge_call()
    w, poas, st, _ = cases.want_cached("edge", call, edge.EDGE_R, compare, merge)
    got = cases.run(gpu_ctx, call, edge.EDGE_R, compare, merge, want_rcw=True)
    cases.assert_equal(got, w, st)
    assert got["n_nodes"] == 1 + (len(call[1]["symbols"]) + 1) + (len(call[2]["symbols"]) + 1)
    assert got["insert_first"][1] == 0 and got["totals"][0].tolist() == [0.0] * 4  # the consensus without a node: a prefix node alone
    lean = cases.run(gpu_ctx, call, edge.EDGE_R, compare, merge, want_rcw=False)
    assert lean["repeat_count_weight"] is None and np.array_equal(lean["repeat_count_pick"], got["repeat_count_pick"])
    cases.assert_equal(lean, w, st)
    for use_rle in (True, False):
        cases.assert_consensus(got, poas, call, use_rle)


def test_runs_of_65_entries_and_nodes_of_200_distinct_inserts(gpu_ctx):
    call = edge.big_call()
    w, poas, st, _ = cases.want_cached("big", call, edge.EDGE_R)
    assert st["longest_run"] == 65 and st["complete_inserts"] >= 2145 + 200 and st["complete_deletes"] >= 2145
    per_node = np.diff(w["insert_first"])
    assert {1, 63, 64, 65, 200} <= set(per_node.tolist())
    got = cases.run(gpu_ctx, call, edge.EDGE_R)
    cases.assert_equal(got, w, st)
    cases.assert_consensus(got, poas, call, True)


def test_deletes_only_more_distinct_deletes_than_complete_inserts(gpu_ctx):
    """no insert list at all and several hundred distinct (node, length) deletes: the leaders of the deletes need room of their own"""
    n = 1600
    sym = np.tile(np.array([0, 1, 2, 3], np.uint8), n // 4)
    reads = []
    for r in range(390):
        x, length = 2 + 4 * r, 1 + r % 3  # positions x .. x + length - 1 deleted after the read's first symbol
        reads.append(cases.read([sym[x - 1], sym[x + length]], [1, 1], r % 2, [(x - 1, 0, 1000 + r), (x + length, 1, 2000 + r)],
                                [(x + q, 0, 500 + r + q) for q in range(length)], []))
    call = cases.random_shifts([cases.consensus(sym, None, reads)], 5)
    w, poas, st = cases.want(call, 12)
    assert st["complete_inserts"] == 0 and st["complete_deletes"] == 390 and len(w["delete_length"]) == 390 and len(w["insert_str_len"]) == 0
    assert len(set(zip(np.repeat(np.arange(n + 1), np.diff(w["delete_first"])).tolist(), w["delete_length"].tolist()))) == 390
    got = cases.run(gpu_ctx, call, 12)
    cases.assert_equal(got, w, st)
    cases.assert_consensus(got, poas, call, True)


def test_the_longest_run_may_start_at_the_first_coordinate(gpu_ctx):
    """an insert run at x = -1 from y = 0 and a delete run at x = 0 with y = -1 have no predecessor to look up"""
    sym = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8)
    for kind in ("inserts", "deletes"):
        if kind == "inserts":  # three symbols before the reference, then a match of position 0; elsewhere runs of one
            rd = cases.read([2, 3, 2, 0, 1, 1], [1, 2, 3, 1, 1, 1], 1, [(0, 3, 900), (1, 5, 800)], [], [(-1, 0, 50), (-1, 1, 60), (-1, 2, 70), (0, 4, 30)])
        else:  # positions 0 .. 3 deleted before the read's first symbol, then a match of position 4; elsewhere a run of one
            rd = cases.read([0, 2], [1, 1], 0, [(4, 0, 900), (6, 1, 800)], [(0, -1, 50), (1, -1, 60), (2, -1, 70), (3, -1, 40), (5, 0, 30)], [])
        call = [cases.consensus(sym, None, [rd])]
        w, _, st = cases.want(call, 12)
        assert st["longest_run"] == (3 if kind == "inserts" else 4) and st["complete_" + kind] == 2
        cases.assert_equal(cases.run(gpu_ctx, call, 12), w, st)


def test_penalties(gpu_ctx):
    call = edge.edge_call()
    picks = []
    for penalty in (0.0, 0.5, 1.0, 3.0):
        w, _, st, _ = cases.want_cached("edge", call, edge.EDGE_R, True, True, penalty)
        got = cases.run(gpu_ctx, call, edge.EDGE_R, penalty=penalty)
        cases.assert_equal(got, w, st)
        picks.append(got["base_pick"].tolist())
    assert picks[0] != picks[1] and picks[1] != picks[3]  # the penalty decides some node either way


# ---- refusals raised on the device ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["matches", "deletes", "inserts"])
def test_a_duplicate_key_is_an_argument_error(gpu_ctx, which):
    call = [dict(c, reads=[dict(r) for r in c["reads"]]) for c in cases.random_call()]
    rd = call[2]["reads"][3]
    assert len(rd[which]) > 2
    x, y, wt = rd[which][1]
    rd[which] = rd[which] + [(x, y, wt + 1)]
    with pytest.raises(capi.MrpError) as e:
        cases.run(gpu_ctx, call, 12)  # (capi.poa_augment asserts that the outputs came back untouched)
    assert e.value.code == capi.MRP_ERR_ARG and f"twice in the {which}" in str(e.value)


def test_a_total_beyond_2_53_is_refused(gpu_ctx):
    """An accumulator is a sum of int32 weights over the entries at one node, so a few hundred entries stay far below 2^53.  The bound that
    is reachable in a quick test is a total: 33 reads match every one of 131 072 nodes with the largest weight, 33 * 131 072 * (2^31 - 1) >=
    2^53.  One read fewer stays below and is accepted.  Nothing faults either way: it is an integer compare."""
    n, wmax = 131072, 2**31 - 1
    sym = np.tile(np.array([0, 1, 2, 3], np.uint8), n // 4)
    x = np.arange(n, dtype=np.int32)

    def call_of(n_reads):
        reads = n_reads
        lists = [dict(first=np.arange(reads + 1, dtype=np.int64) * n, x=np.tile(x, reads), y=np.tile(x, reads), weight=np.full(reads * n, wmax, np.int32))]
        empty = dict(first=np.zeros(reads + 1, np.int64), x=np.zeros(0, np.int32), y=np.zeros(0, np.int32), weight=np.zeros(0, np.int32))
        return [np.array([0, n]), sym, np.ones(n, np.uint8), np.array([0, reads]), np.tile(sym, reads), np.ones(reads * n, np.uint8),
                np.arange(reads, dtype=np.int64) * n, np.full(reads, n, np.int32), np.ones(reads, np.uint8), lists[0], empty, empty]

    assert 33 * n * wmax >= 2**53 > 32 * n * wmax
    with pytest.raises(capi.MrpError) as e:
        capi.poa_augment(gpu_ctx, 12, *call_of(33))
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "2^53" in str(e.value)
    got = capi.poa_augment(gpu_ctx, 12, *call_of(32))
    assert got["totals"][0].tolist() == [float(32 * n * wmax), 0.0, 0.0, 0.0] and got["base_weight"][1].tolist()[0] == float(32 * wmax)


# ---- determinism, a random call, the chain ----------------------------------------------------------------------------------------------

def test_determinism_on_one_context_and_across_contexts(gpu_ctx):
    call = cases.random_call()
    runs = [cases.run(gpu_ctx, call, 12, want_rcw=True) for _ in range(2)]
    with capi.Context(0) as other:
        runs.append(cases.run(other, call, 12, want_rcw=True))
    for r in runs[1:]:
        cases.assert_equal(r, runs[0])
        assert np.array_equal(cases.bits(r["repeat_count_weight"]), cases.bits(runs[0]["repeat_count_weight"]))


def test_a_random_call(gpu_ctx):
    call = cases.random_call()
    w, poas, st, _ = cases.want_cached("random", call, 12)
    got = cases.run(gpu_ctx, call, 12, want_rcw=True)
    cases.assert_equal(got, w, st)
    assert st["complete_inserts"] > 300 and st["complete_deletes"] > 300 and got["stats"].matches > 12000
    assert len(set(rd["x_shift"] for c in call for rd in c["reads"])) > 3
    for use_rle in (True, False):
        cases.assert_consensus(got, poas, call, use_rle)


def test_the_chain_from_posteriors_to_the_consensus(gpu_ctx):
    from tests.test_gpu_repeat_counts import chain_reads
    R, table = rc.R_SHIPPED, rc.shipped_matrix()
    kw = dict(expansion=20, min_diags=1000, traceback_diagonals=40)
    sx, cx, reads = chain_reads(91, 40, 6, R)
    strands = [1, 0, 1, 1, 0, 0]
    models = [pc.model(), pc.model().reverse_complement()]
    repeat = [capi.RepeatModel(table, 1), capi.RepeatModel(table, 0)]
    pairs = [(sx, cx, sy, cy, []) for sy, cy in reads]
    model_index = np.array([0 if s else 1 for s in strands], np.uint8)
    pool, counts, xo, xl, yo, yl, ao, an = rc.pack(pairs)
    match, gap_x, gap_y = capi.posterior_aligned_pairs_rle(gpu_ctx, models, repeat, pool, counts, xo, xl, yo, yl, model_index, ao, an, pc.options(kw, 0.01, True))[:3]
    got = capi.poa_augment(gpu_ctx, R, [0, len(sx)], sx, cx, [0, len(reads)], pool, counts, yo, yl, strands, match, gap_x, gap_y, pool_bytes=len(pool))
    # the restatements: rle_pairhmm_oracle, then poa_oracle
    lists = [rc.want_posterior(models[0 if s else 1], table, s, p, kw, 0.01)[0] for s, p in zip(strands, pairs)]
    flip = lambda l: [(x, y, w) for w, x, y, _ in l]
    call = [cases.consensus(sx, cx, [cases.read(sy, cy, s, flip(l[0]), flip(l[1]), flip(l[2])) for (sy, cy), s, l in zip(reads, strands, lists)])]
    assert all(len(l[1]) > 3 and len(l[2]) > 3 for l in lists)
    w, poas, st = cases.want(call, R)
    cases.assert_equal(got, w, st)
    cases.assert_consensus(got, poas, call, True)
    s, c, _ = capi.poa_consensus(got, 0, len(sx), True)
    assert len(capi.rle_expand(s, c)) > 40
