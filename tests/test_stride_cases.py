"""What the cases of tests/stride_cases.py exhibit, asserted from the references alone (no device): every boundary the kernels of
the alignment front cross on a second trip is really in the inputs tests/test_gpu_front_strides.py runs.  Where two references of
one function exist (the oracle's k-mer chain, the Python restatement of its walk, the product's host function) they are pinned
against each other on the same cases."""
import numpy as np
import pytest

from margin_amd import capi
from oracle import pairhmm as ph
from tests import extract_oracle as eo
from tests import stride_cases as sc


# ---- A. extraction ----

def test_boundary_chunk_entries_per_read():
    f = sc.boundary_facts()
    per = f["entries_per_read"]
    assert per[0] == 200 and set(sc.BOUNDARY_COUNTS) <= set(per)
    c = sc.boundary_chunk()
    text = lambda r: [(int(w) & 15, int(w) >> 4) for w in c.cigar[c.cigar_first[r]:c.cigar_first[r + 1]]]
    by_count = {n: [r for r, k in enumerate(per) if k == n] for n in sc.BOUNDARY_COUNTS}
    assert any(text(r)[0][0] == eo.S for r in by_count[64]) and any(text(r)[-1][0] == eo.S for r in by_count[65])
    assert any(f["status"][r] == eo.FILTERED for r in by_count[127])                    # low mapq: filtered, entries kept
    eqx = [r for r in by_count[129] if {op for op, _ in text(r)} == {eo.EQ, eo.X, eo.I, eo.D}]
    assert eqx
    ops = text(eqx[0])
    ref_before_indel = sum(n for op, n in ops[:[op for op, _ in ops].index(eo.I)])
    assert ref_before_indel > 64 and (eo.I, 2) in ops and (eo.D, 3) in ops              # both past the read's 64th entry


def test_boundary_chunk_delayed_start_crosses_a_pass():
    """the SV entries are the first candidates of the second and third pass of 64; each starts at the maximum carried over from the
    pass before, which its substring's length shows"""
    carry = sc.boundary_facts()["carry"]
    assert [c["candidate"] for c in carry] == [64, 128]
    for c in carry:
        assert c["own_start"] < c["predecessor_start"] == c["before"]
        assert c["length"] == c["from_carry"] < c["own_window"]


def test_boundary_chunk_buckets():
    b = sc.boundary_facts()["buckets"]
    assert set(b) == set(sc.BUCKET_SIZES)
    for size, per in b.items():
        assert len(per) == sc.BUCKET_READ
        for v in per:
            assert v["n"] == size and v["ascending"] and v["statuses"] == {eo.KEPT, eo.FILTERED}


def test_cigar_chunk_block_edges():
    f = sc.cigar_facts()
    for n in sc.CIGAR_OPS:
        assert f["n_ops"].count(n) >= 2
    assert all(k > 0 for k in f["entries_per_read"])
    # the read with an N op has 65 ops, and the loop bound (alnReadLength + 1 steps, N left out) ends its walk before its CIGAR does
    (r,) = f["n_read"]
    assert f["n_ops"][r] == 65 and f["n_read_aligned"][0] + 1 < f["n_read_ref_steps"][0]
    assert f["entries_per_read"][r] < f["n_read_ref_steps"][0] - 10
    c = sc.cigar_chunk()
    # the last op of the first block of 64, whose advance is carried into the second: a sequence op in some reads, a reference op in others
    at_edge = {int(c.cigar[c.cigar_first[r] + 63]) & 15 for r, n in enumerate(f["n_ops"]) if n >= 128}
    assert eo.I in at_edge and (eo.M in at_edge or eo.D in at_edge)
    lead = [[int(w) & 15 for w in c.cigar[c.cigar_first[r]:c.cigar_first[r] + 2]] for r in range(len(f["n_ops"]))]
    tail = [[int(w) & 15 for w in c.cigar[c.cigar_first[r + 1] - 2:c.cigar_first[r + 1]]] for r in range(len(f["n_ops"]))]
    assert sum(a == [eo.H, eo.S] and b == [eo.S, eo.H] for a, b in zip(lead, tail)) == len(sc.CIGAR_OPS)
    assert any(a == [eo.H, eo.S] and b[1] == eo.M for a, b in zip(lead, tail))


@pytest.mark.parametrize("seed", sc.DENSE_SEEDS)
def test_dense_chunks(seed):
    f = sc.dense_facts(seed)
    assert f["max_per_read"] > 128 and f["reads_over_64"] >= 10 and f["max_per_variant"] > 64
    if seed == 0:
        assert 6 * f["entries"] > sc.GRID_CAP                 # six copies in one call pass the grid cap of the entry-wide kernels


def test_wide_chunk_passes_the_variant_grid():
    f = sc.wide_facts()
    assert f["variants"] == sc.WIDE_BP > sc.GRID_CAP
    assert f["with_entries_past_cap"] >= 100 and f["with_entries_below_cap"] >= 100
    assert f["entries_per_read"] == [150, 100, 100, 90]


# ---- B. owners and classes ----

def test_wide_chunk_has_owners_past_the_cap():
    f = sc.wide_owner_facts()
    assert 0 < f["owners"] < f["entries"]
    assert all(90 <= n <= 150 for n in f["sites_per_read"])
    w = sc.wide_haplotag_oracle()
    assert set(w["hap"].tolist()) <= {1, 2} and w["facts"]["mixed_strand"] >= 0


def test_class_sites():
    sites = sc.class_sites()
    assert len(sites) == sc.GRID_CAP + sc.TAIL_SITES
    head = [len(s) for s in sites[:sc.GRID_CAP]]
    assert set(head) == {0, 1} and 0.3 < np.mean(head) < 0.7
    assert {1, 2, 63, 64, 65, 130} <= {len(s) for s in sites[sc.GRID_CAP:]}
    from tests.test_gpu_substring_classes import host_classes
    tail = sites[sc.GRID_CAP:]
    rep = host_classes(tail)
    first = np.concatenate([[0], np.cumsum([len(s) for s in tail])])
    own = [rep[first[i]:first[i + 1]] - first[i] for i in range(len(tail))]
    assert any(len(o) > 64 and (o == 0).all() for o in own) and any(len(o) > 64 and (o == np.arange(len(o))).all() for o in own)
    assert sum(1 for s in tail if len(s) >= 5 and len({bytes(x) for x in s[-5:]}) == 3 and len(s[-5]) == 8) >= 4


# ---- C. k-mer anchors ----

def test_walk_restatement_equals_the_oracle_and_the_host_function():
    for name, x, y in sc.anchor_cases():
        want = ph.kmer_anchors(x, y)
        assert len(want) > 0 and np.array_equal(sc.walk_anchors(sc.walk(x, y)), want), name
        assert np.array_equal(capi.kmer_alignment_anchors(x, y), want), name


def test_long_walk_reaches_every_lane_of_a_workspace_pass():
    recs = sc.walk(*sc.long_walk_pair())
    assert all(r["stopped"] and r["stop_dist"] == i for i, r in enumerate(recs) if i > 0)   # every walk ends at record 0
    assert max(r["passed"] for r in recs) > 256
    d = np.array([r["stop_dist"] for r in recs])
    assert ((d > 64) & (d <= 128)).any() and ((d > 128) & (d <= 192)).any() and (d > 192).any()
    lanes = {int(k) for k in (d[d > 64] - 65) % 64}
    assert {0, 63} <= lanes and any(0 < k < 63 for k in lanes)


def test_far_best_lies_beyond_the_registers():
    recs = sc.walk(*sc.far_best_pair())
    last = recs[-1]
    near = recs[-65:-1]
    assert len(near) == 64 and all(r["x"] < last["x"] and r["score"] == 1 and not r["high"] for r in near)
    assert last["best_dist"] > 64 and last["score"] == 41 and last["stopped"] and last["stop_dist"] == last["best_dist"]


def test_tie_between_registers_and_workspace():
    x, y, pos = sc.tie_pair()
    recs = sc.walk(x, y)
    at = {r["x"]: i for i, r in enumerate(recs)}
    f, pn, pf = at[pos["F"]], at[pos["Pn"]], at[pos["Pf"]]
    assert recs[pn]["score"] == recs[pf]["score"] == 2 and recs[pn]["x"] < recs[f]["x"] and recs[pf]["x"] < recs[f]["x"]
    assert f - pn <= 64 < f - pf
    assert not any(r["high"] and r["x"] < recs[f]["x"] for r in recs[pf:f])                 # no stop between them
    assert not recs[f]["stopped"] and recs[f]["passed"] == f and recs[f]["score"] == 3
    assert recs[f]["back"] == pn
    chain = {tuple(a) for a in ph.kmer_anchors(x, y).tolist()}
    centre = lambda i: (recs[i]["x"] + sc.K // 2, recs[i]["y"] + sc.K // 2)
    assert centre(f) in chain and centre(pn) in chain and centre(pf) not in chain


def test_many_pairs():
    pool, x_off, x_len, y_off, y_len, idx, real = sc.many_pairs()
    n = len(x_off)
    assert n == sc.GRID_CAP + sc.N_REAL and idx == list(range(sc.N_REAL)) + list(range(sc.GRID_CAP, n))
    short = np.ones(n, bool)
    short[idx] = False
    assert (np.minimum(x_len, y_len)[short] < sc.K).all() and (x_len[short] >= 0).all() and x_len[short].max() == sc.K - 1
    assert (x_off + x_len <= len(pool)).all() and (y_off + y_len <= len(pool)).all()
    assert len({x.tobytes() + b"|" + y.tobytes() for x, y in real}) == 2 * sc.N_REAL          # mutually different
    assert all(len(x) >= 60 and len(y) >= 40 for x, y in real)
    n_anchors = [len(ph.kmer_anchors(x, y)) for x, y in real]
    assert sum(k > 0 for k in n_anchors[:sc.N_REAL]) > 50 and sum(k > 0 for k in n_anchors[sc.N_REAL:]) > 50
    for i in list(range(sc.N_REAL, sc.GRID_CAP, 997)):                                      # a short pair has no anchor
        assert len(ph.kmer_anchors(pool[x_off[i]:x_off[i] + x_len[i]], pool[y_off[i]:y_off[i] + y_len[i]])) == 0
    for x, y in real[:8] + real[sc.N_REAL:sc.N_REAL + 8]:
        assert np.array_equal(capi.kmer_alignment_anchors(x, y), ph.kmer_anchors(x, y))


# ---- D. pair-per-wave kernel ----

def test_wave_pairs_fill_more_than_one_grid():
    f = sc.wave_facts()
    assert f["first_class"] > sc.PHM_GRID_CAP and f["second_class"] > 0 and f["second_class"] + f["wider"] == sc.N_LONG == f["long_pairs"]
    _, _, x_len, _, y_len, mi = sc.wave_pairs()
    big = np.maximum(x_len, y_len) > 100
    assert (x_len[big] >= 101).all() and (np.maximum(x_len, y_len)[big] <= 300).all() and (np.maximum(x_len, y_len)[~big] <= 30).all()
    assert (x_len == 0).any() and (y_len == 0).any() and len(set(mi.tolist())) == sc.N_MODELS
