"""What the tests of mrp_ml_repeat_counts share (tests/test_repeat_counts_host.py, tests/test_gpu_repeat_counts.py,
tools/repeat_count_probe.py): the cases, their packing into one call, the expected values from the restatement
(tests/repeat_count_oracle.py), computed once per (case, order, phasing), and the comparison on bit patterns.

A consensus is a dict: symbols uint8 [nodes]; read_counts a list of uint8 arrays (a read's run lengths); strands; matches, per read a
list of (x, y, weight) in the order given to the call; x_shift int32 per read.  A call is a list of them."""
from __future__ import annotations

import functools
import math

import numpy as np

from margin_amd import capi
from tests import repeat_count_oracle as rco
from tests import rle_cases as rc

S_SHIPPED = math.log(0.0001)  # log(hetRunLengthSubstitutionProbability), the shipped default


def consensus(symbols, read_counts=(), strands=(), matches=(), x_shift=None):
    n = len(read_counts)
    return dict(symbols=np.asarray(symbols, np.uint8), read_counts=[np.asarray(c, np.uint8) for c in read_counts],
                strands=np.asarray(strands, np.uint8), matches=[list(m) for m in matches],
                x_shift=np.zeros(n, np.int32) if x_shift is None else np.asarray(x_shift, np.int32))


class Builder:
    """a consensus from observations: observe(node, read, count, weight) appends a symbol with that count to the read and a match of it"""

    def __init__(self, rng, symbols, n_reads):
        self.rng, self.symbols = rng, np.asarray(symbols, np.uint8)
        self.counts = [[] for _ in range(n_reads)]
        self.obs = [[] for _ in range(n_reads)]  # (node, y, weight)

    def observe(self, node, read, count, weight=None):
        w = int(self.rng.integers(1, 10_000_001)) if weight is None else weight
        self.obs[read].append((node, len(self.counts[read]), w))
        self.counts[read].append(count)

    def build(self, shuffle=True, shift=True):
        """a read's matches in a random order (the order given is the definition's), a random crop x_shift per read"""
        matches, shifts = [], []
        for o in self.obs:
            s = int(self.rng.integers(0, min(n for n, _, _ in o) + 1)) if (o and shift) else 0
            m = [(n - s, y, w) for n, y, w in o]
            if shuffle:
                m = [m[i] for i in self.rng.permutation(len(m))]
            matches.append(m)
            shifts.append(s)
        strands = self.rng.integers(0, 2, size=len(self.counts))
        return consensus(self.symbols, self.counts, strands, matches, shifts)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

EDGE_R = 12
EDGE_NODES = dict(none=0, one=1, n63=2, n64=3, n65=4, n129=5, n1000=6, same_x=7, n_base=8, zero=9, overlong=10, mixed=11, twins=12, minus_inf=13)


@functools.lru_cache(maxsize=None)
def edge_table():
    """R = 12, random; the candidates 4 and 5 have identical rows (every base, every observed count); [., 7, 2] is -inf"""
    t = rc.random_table(np.random.default_rng(41), EDGE_R)
    t[:, 5, :] = t[:, 4, :]
    t[:, 7, 2] = -np.inf
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def edge_call():
    """three consensus strings: one without a node (and so without a read), the edges, one without a read"""
    rng = np.random.default_rng(42)
    N, R = EDGE_NODES, EDGE_R
    sym = rng.integers(0, 4, size=len(N)).astype(np.uint8)
    sym[N["n_base"]] = 4
    b = Builder(rng, sym, 129 + 1000)
    some = lambda: int(rng.integers(0, R))
    b.observe(N["one"], 0, some())
    for name, n in (("n63", 63), ("n64", 64), ("n65", 65), ("n129", 129)):
        for r in range(n):
            b.observe(N[name], r, some())
    for r in range(1000):  # one node under 1 000 one-symbol reads
        b.observe(N["n1000"], 129 + r, some())
    for r, k in ((0, 2), (1, 3), (2, 1), (3, 1)):  # the same x matched by several y of one read
        for _ in range(k):
            b.observe(N["same_x"], r, some())
    for r in range(20):  # an N node under both strands (20 random strands)
        b.observe(N["n_base"], r, some())
    for r in range(5):  # candidate 0 alone: it wins and is stored as 1
        b.observe(N["zero"], r, 0)
    for r, c in enumerate((R, 200, 255, R + 1)):  # nothing below R: 1 / -inf
        b.observe(N["overlong"], r, c)
    for r, c in enumerate((3, R + 5, 2, 255, 6)):  # clamped, max = R - 1
        b.observe(N["mixed"], r, c)
    for r in range(12):  # the two candidates with identical rows
        b.observe(N["twins"], r, 4 + r % 2)
    for r in range(9):  # candidate 7 under an observed 2 is -inf
        b.observe(N["minus_inf"], r, (2, 7, 5)[r % 3])
    main = b.build()
    assert len(set(main["strands"][:20].tolist())) == 2 and main["x_shift"].max() > 0
    return [consensus([]), main, consensus(rng.integers(0, 5, size=5))]


WIDE_R = 130


@functools.lru_cache(maxsize=None)
def wide_table():
    t = rc.random_table(np.random.default_rng(43), WIDE_R)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def wide_call():
    """R = 130: candidate ranges of 1, 64, 65 and 130, and eight random ones"""
    rng = np.random.default_rng(44)
    spans = [(17, 17), (10, 73), (10, 74), (0, 129)] + [tuple(sorted(rng.integers(0, WIDE_R, size=2).tolist())) for _ in range(8)]
    b = Builder(rng, rng.integers(0, 4, size=len(spans)), 24)
    for node, (lo, hi) in enumerate(spans):
        cs = [lo, hi] + rng.integers(lo, hi + 1, size=22).tolist()
        for r in range(24):
            b.observe(node, r, cs[r])
    return [b.build()], [hi - lo + 1 for lo, hi in spans]


def noisy_counts(rng, truth):
    """a read's run lengths over nodes with the run lengths truth: kept at 80 %, one more or less otherwise, never below 0"""
    noise = rng.choice((-1, 0, 1), size=len(truth), p=(0.1, 0.8, 0.1))
    return np.clip(truth.astype(np.int64) + noise, 0, 255).astype(np.uint8)


def spanning_consensus(rng, n_nodes, n_reads, per_read=1, secondary=0.0):
    """every read spans the consensus: per_read matches of every node (y = per_read * node + j), run lengths 1 + geometric(0.5) with the
    noise above, random strands and weights; `secondary`: that many more matches per read and node, of a neighbouring node"""
    truth = np.minimum(rng.geometric(0.5, size=n_nodes), 255)
    sym = rng.integers(0, 4, size=n_nodes).astype(np.uint8)
    counts, matches = [], []
    for _ in range(n_reads):
        counts.append(noisy_counts(rng, np.repeat(truth, per_read)))
        y = np.arange(n_nodes * per_read)
        x = y // per_read
        n_sec = int(secondary * n_nodes)
        if n_sec:
            ys = rng.integers(0, n_nodes * per_read, size=n_sec)
            x = np.concatenate([x, np.clip(ys // per_read + rng.choice((-1, 1), size=n_sec), 0, n_nodes - 1)])
            y = np.concatenate([y, ys])
        w = rng.integers(1, 10_000_001, size=len(x))
        matches.append(np.stack([x, y, w], axis=1))
    return consensus(sym, counts, rng.integers(0, 2, size=n_reads), [[]] * n_reads), matches


def with_matches(cons, matches):
    """(spanning_consensus keeps its matches as arrays: lists of tuples only where the oracle needs them)"""
    out = dict(cons)
    out["matches"] = [[tuple(int(v) for v in row) for row in m] for m in matches]
    return out


@functools.lru_cache(maxsize=None)
def shipped_call():
    """2 000 nodes under 30 spanning reads on the shipped r9.4 g507 matrix"""
    return [with_matches(*spanning_consensus(np.random.default_rng(45), 2000, 30))]


@functools.lru_cache(maxsize=None)
def order_call():
    """200 nodes with 40 observations each, four of every one of 10 reads: the walk order inside a read decides the order of the sum"""
    return [with_matches(*spanning_consensus(np.random.default_rng(46), 200, 10, per_read=4))]


def random_hap(call, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2, size=len(c["read_counts"])).astype(np.uint8) for c in call]


# ---- packing, expectation, comparison ---------------------------------------------------------------------------------------------------

def pack(call):
    """-> the arguments of capi.ml_repeat_counts behind ctx and log_prob"""
    node_first, read_first = [0], [0]
    sym, counts, y_off, y_len, strand, shift = [], [], [], [], [], []
    first, mx, my, mw, at = [0], [], [], [], 0
    for c in call:
        sym.append(c["symbols"])
        node_first.append(node_first[-1] + len(c["symbols"]))
        read_first.append(read_first[-1] + len(c["read_counts"]))
        for r, cnt in enumerate(c["read_counts"]):
            counts.append(cnt); y_off.append(at); y_len.append(len(cnt)); at += len(cnt)
            m = np.asarray(c["matches"][r], np.int64).reshape(-1, 3)
            mx.append(m[:, 0]); my.append(m[:, 1]); mw.append(m[:, 2])
            first.append(first[-1] + len(m))
        strand.append(c["strands"]); shift.append(c["x_shift"])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    matches = dict(first=np.array(first, np.int64), x=cat(mx, np.int32), y=cat(my, np.int32), weight=cat(mw, np.int32))
    return dict(node_first=np.array(node_first, np.int64), symbols=cat(sym, np.uint8), read_first=np.array(read_first, np.int64), counts=cat(counts, np.uint8),
                y_off=np.array(y_off, np.int64), y_len=np.array(y_len, np.int32), read_forward_strand=cat(strand, np.uint8), matches=matches,
                x_shift=cat(shift, np.int32))


def want(table, call, walk_backwards=False, hap=None, s=None):
    """the restatement over a call -> dict(count, log_prob, non_rle_length [consensus], observations, nodes_observed, candidates)"""
    parts = [rco.estimate(table, c["symbols"], c["read_counts"], c["strands"], c["matches"], c["x_shift"], walk_backwards,
                          None if hap is None else hap[i], s) for i, c in enumerate(call)]
    return dict(count=np.concatenate([p["count"] for p in parts]), log_prob=np.concatenate([p["log_prob"] for p in parts]),
                non_rle_length=np.array([p["non_rle_length"] for p in parts], np.int64),
                **{k: sum(p[k] for p in parts) for k in ("observations", "nodes_observed", "candidates")})


_WANT = {}


def want_cached(name, table, call, walk_backwards=False, hap=None, s=None):
    """want(), once per (case name, order, phasing): the expectation is shared among the tests and never changed"""
    key = (name, bool(walk_backwards), None if hap is None else tuple(h.tobytes() for h in hap), s)
    if key not in _WANT:
        w = want(table, call, walk_backwards, hap, s)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def run(ctx, table, call, walk_backwards=False, hap=None, s=0.0):
    p = pack(call)
    return capi.ml_repeat_counts(ctx, table, walk_backwards=walk_backwards, log_het_substitution=s,
                                 read_in_hap=None if hap is None else (np.concatenate(hap) if hap else np.zeros(0, np.uint8)), **p)


def assert_equal(got, w):
    """counts, log probabilities (bit patterns), lengths and the stats' three counts"""
    count, lp, length, st = got
    assert np.array_equal(count, w["count"])
    assert np.array_equal(lp.view(np.int64), w["log_prob"].view(np.int64))
    assert np.array_equal(length, w["non_rle_length"])
    assert (st.observations, st.nodes_observed, st.candidates) == (w["observations"], w["nodes_observed"], w["candidates"])
    assert (count >= 1).all()
