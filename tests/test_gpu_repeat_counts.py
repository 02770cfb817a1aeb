"""mrp_ml_repeat_counts on the device against the sequential restatement (tests/repeat_count_oracle.py): the stored counts, the winning
log probabilities as bit patterns, the lengths, and the stats' three counts (tests/repeat_count_cases.py's assert_equal), at the smallest
shapes at which the kernels can go wrong."""
import math

import numpy as np
import pytest

from margin_amd import capi
from tests import posterior_cases as pc
from tests import repeat_count_cases as cases
from tests import repeat_count_oracle as rco
from tests import rle_cases as rc

pytestmark = pytest.mark.gpu


def test_edges_in_one_call_of_three_consensus_strings(gpu_ctx):
    table, call = cases.edge_table(), cases.edge_call()
    for backwards in (False, True):
        got = cases.run(gpu_ctx, table, call, walk_backwards=backwards)
        cases.assert_equal(got, cases.want_cached("edge", table, call, backwards))
    N, base = cases.EDGE_NODES, 0  # (the first consensus has no node)
    count, lp = got[0], got[1]
    assert count[base + N["none"]] == 1 and np.isneginf(lp[base + N["none"]])
    assert count[base + N["overlong"]] == 1 and np.isneginf(lp[base + N["overlong"]])
    assert count[base + N["zero"]] == 1 and np.isfinite(lp[base + N["zero"]])
    assert count[base + N["twins"]] == 4  # two identical candidate rows: the first wins
    assert got[2].tolist()[0] == 0 and got[2].tolist()[2] == 5
    assert got[3].observations == 1 + 63 + 64 + 65 + 129 + 1000 + 7 + 20 + 5 + 4 + 5 + 12 + 9


def test_candidate_range_beyond_a_wave(gpu_ctx):
    (call, spans), table = cases.wide_call(), cases.wide_table()
    assert spans[:4] == [1, 64, 65, 130]
    w = cases.want_cached("wide", table, call)
    got = cases.run(gpu_ctx, table, call)
    cases.assert_equal(got, w)
    assert got[3].candidates == sum(spans) == w["candidates"]
    assert len(set(got[0].tolist())) > 4


def test_the_order_inside_a_read_has_teeth(gpu_ctx):
    table, call = rc.shipped_matrix(), cases.order_call()
    fwd, bwd = (cases.want_cached("order", table, call, b) for b in (False, True))
    differ = int((fwd["log_prob"].view(np.int64) != bwd["log_prob"].view(np.int64)).sum())
    assert fwd["observations"] == 200 * 40 and differ > 20  # the two orders of the restatement differ in bits
    for backwards, w in ((False, fwd), (True, bwd)):
        cases.assert_equal(cases.run(gpu_ctx, table, call, walk_backwards=backwards), w)


def test_determinism_on_one_context_and_across_contexts(gpu_ctx):
    table, call = cases.edge_table(), cases.edge_call()
    hap = cases.random_hap(call, 7)
    runs = [cases.run(gpu_ctx, table, call, hap=hap, s=cases.S_SHIPPED) for _ in range(2)]
    with capi.Context(0) as other:
        runs.append(cases.run(other, table, call, hap=hap, s=cases.S_SHIPPED))
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1].view(np.int64), runs[0][1].view(np.int64)) and np.array_equal(r[2], runs[0][2])


def test_phased(gpu_ctx):
    table, call = cases.edge_table(), cases.edge_call()
    sizes = [len(c["read_counts"]) for c in call]
    haps = dict(random=cases.random_hap(call, 7), all_in=[np.ones(n, np.uint8) for n in sizes], all_other=[np.zeros(n, np.uint8) for n in sizes])
    for name, hap in haps.items():
        for s in (cases.S_SHIPPED, -math.inf):
            for backwards in (False, True) if name == "random" else (False,):
                got = cases.run(gpu_ctx, table, call, walk_backwards=backwards, hap=hap, s=s)
                cases.assert_equal(got, cases.want_cached("edge", table, call, backwards, hap, s))
                assert got[0][cases.EDGE_NODES["twins"]] == 5  # two identical candidate rows: the last wins
    # a NULL vector is the unphased path, whatever s says
    got = cases.run(gpu_ctx, table, call, hap=None, s=cases.S_SHIPPED)
    cases.assert_equal(got, cases.want_cached("edge", table, call))
    un, ph = cases.want_cached("edge", table, call), cases.want_cached("edge", table, call, False, haps["random"], cases.S_SHIPPED)
    assert not np.array_equal(un["log_prob"].view(np.int64), ph["log_prob"].view(np.int64))


def test_shipped_matrix(gpu_ctx):
    table, call = rc.shipped_matrix(), cases.shipped_call()
    hap = cases.random_hap(call, 8)
    for h, s in ((None, 0.0), (hap, cases.S_SHIPPED)):
        w = cases.want_cached("shipped", table, call, False, h, None if h is None else s)
        got = cases.run(gpu_ctx, table, call, hap=h, s=s)
        cases.assert_equal(got, w)
        assert got[3].observations == 2000 * 30 and got[3].nodes_observed == 2000  # the test's own counts
        assert len(set(call[0]["strands"].tolist())) == 2 and got[0].max() > 3 and got[3].bytes_uploaded > 12 * 60000


def chain_reads(seed, n_nodes, n_reads, R):
    """a run-length consensus and reads of it with about 5 % substitutions, insertions and deletions each and noisy run lengths"""
    rng = np.random.default_rng(seed)
    sx = rng.integers(0, 4, size=n_nodes).astype(np.uint8)
    sx[1:][sx[1:] == sx[:-1]] ^= 1  # neighbouring runs differ
    cx = rc.geometric_counts(rng, n_nodes, R)
    reads = []
    for _ in range(n_reads):
        sy, cy = [], []
        for b, c in zip(sx.tolist(), cx.tolist()):
            u = rng.random()
            if u < 0.05:
                continue
            if u < 0.10:
                sy.append(int(rng.integers(0, 4))); cy.append(int(rc.geometric_counts(rng, 1, R)[0]))
            sy.append(int(rng.integers(0, 4)) if u >= 0.95 else b)
            cy.append(c if rng.random() < 0.8 else min(R - 1, max(1, c + int(rng.choice((-1, 1))))))
        reads.append((np.array(sy, np.uint8), np.array(cy, np.uint8)))
    return sx, cx, reads


def test_the_chain_from_posteriors_to_the_polished_sequence(gpu_ctx):
    R, table = rc.R_SHIPPED, rc.shipped_matrix()
    kw = dict(expansion=20, min_diags=1000, traceback_diagonals=40)
    sx, cx, reads = chain_reads(91, 40, 6, R)
    strands = [1, 0, 1, 1, 0, 0]
    models = [pc.model(), pc.model().reverse_complement()]
    repeat = [capi.RepeatModel(table, 1), capi.RepeatModel(table, 0)]
    pairs = [(sx, cx, sy, cy, []) for sy, cy in reads]
    model_index = np.array([0 if s else 1 for s in strands], np.uint8)
    # the device: posteriors, then the estimate straight from match_out
    pool, counts, xo, xl, yo, yl, ao, an = rc.pack(pairs)
    match = capi.posterior_aligned_pairs_rle(gpu_ctx, models, repeat, pool, counts, xo, xl, yo, yl, model_index, ao, an, pc.options(kw, 0.01, True))[0]
    got = capi.ml_repeat_counts(gpu_ctx, table, [0, len(sx)], sx, [0, len(reads)], counts, yo, yl, strands, match, walk_backwards=True)
    # the restatements: rle_pairhmm_oracle, then repeat_count_oracle
    lists = [rc.want_posterior(models[0 if s else 1], table, s, p, kw, 0.01)[0][0] for s, p in zip(strands, pairs)]
    assert all(len(l) > 20 for l in lists)
    cons = cases.consensus(sx, [cy for _, cy in reads], strands, [[(x, y, w) for w, x, y, _ in l] for l in lists])
    cases.assert_equal(got, cases.want(table, [cons], walk_backwards=True))
    assert np.array_equal(match["x"], np.array([x for l in lists for _, x, _, _ in l], np.int32))
    polished = capi.rle_expand(sx, got[0])
    assert polished == rco.rle_expand(sx, cases.want(table, [cons], walk_backwards=True)["count"]) and len(polished) == got[2][0]
