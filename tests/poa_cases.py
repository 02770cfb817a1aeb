"""What the tests of mrp_poa_augment and mrp_poa_consensus share (tests/test_poa_host.py, tests/test_gpu_poa.py, tools/poa_probe.py): the
cases, their packing into one call, the expected values from the restatement (tests/poa_oracle.py), computed once per (case, options),
and the comparison on bit patterns.

A consensus is a dict: symbols, counts (uint8 per reference position) and reads, each a dict with symbols, counts, strand, x_shift and the
three lists matches / deletes / inserts of (x, y, weight) in call coordinates (x before x_shift is added).  A call is a list of them."""
from __future__ import annotations

import functools

import numpy as np

from margin_amd import capi
from tests import poa_oracle as po

FIELDS_F64 = ("base_weight", "insert_weight_forward", "insert_weight_reverse", "delete_weight_forward", "delete_weight_reverse", "totals")
FIELDS_INT = ("base_pick", "repeat_count_pick", "insert_first", "insert_str_off", "insert_str_len", "insert_n_observations", "pool_symbols",
              "pool_counts", "delete_first", "delete_length", "delete_n_observations")
SYM = lambda s: ["ACGTN".index(c) for c in s]


def read(symbols, counts, strand=1, matches=(), deletes=(), inserts=(), x_shift=0):
    return dict(symbols=np.asarray(symbols, np.uint8), counts=np.asarray(counts, np.uint8), strand=int(strand), x_shift=int(x_shift),
                matches=list(matches), deletes=list(deletes), inserts=list(inserts))


def consensus(symbols, counts=None, reads=()):
    symbols = np.asarray(symbols, np.uint8)
    return dict(symbols=symbols, counts=np.ones(len(symbols), np.uint8) if counts is None else np.asarray(counts, np.uint8), reads=list(reads))


def shifted(rd, shift):
    """the same read under a crop: x_shift = shift, every x lowered by it"""
    low = lambda l: [(x - shift, y, w) for x, y, w in l]
    return dict(rd, x_shift=rd["x_shift"] + shift, matches=low(rd["matches"]), deletes=low(rd["deletes"]), inserts=low(rd["inserts"]))


def random_shifts(call, seed):
    """a random crop per read: x_shift in [0, the smallest x of its lists] (an insert's -1 stays reachable)"""
    rng = np.random.default_rng(seed)
    out = []
    for c in call:
        reads = []
        for rd in c["reads"]:
            xs = [x for k in ("matches", "deletes", "inserts") for x, _, _ in rd[k]]
            reads.append(shifted(rd, int(rng.integers(0, max(0, min(xs)) + 1)) if xs else 0))
        out.append(dict(c, reads=reads))
    return out


def pack(call):
    """-> the positional arguments of capi.poa_augment behind max_repeat, and x_shift"""
    node_first = np.cumsum([0] + [len(c["symbols"]) for c in call]).astype(np.int64)
    read_first = np.cumsum([0] + [len(c["reads"]) for c in call]).astype(np.int64)
    reads = [rd for c in call for rd in c["reads"]]
    cat = lambda arrs, dt: np.concatenate([np.asarray(a, dt) for a in arrs]) if arrs else np.zeros(0, dt)
    y_len = np.array([len(rd["symbols"]) for rd in reads], np.int32)
    y_off = (np.cumsum(np.concatenate([[0], y_len]))[:-1]).astype(np.int64)
    lists = []
    for k in ("matches", "deletes", "inserts"):
        first = np.cumsum([0] + [len(rd[k]) for rd in reads]).astype(np.int64)
        flat = [t for rd in reads for t in rd[k]]
        lists.append(dict(first=first, x=np.array([t[0] for t in flat], np.int32), y=np.array([t[1] for t in flat], np.int32),
                          weight=np.array([t[2] for t in flat], np.int32)))
    return ([node_first, cat([c["symbols"] for c in call], np.uint8), cat([c["counts"] for c in call], np.uint8), read_first,
             cat([rd["symbols"] for rd in reads], np.uint8), cat([rd["counts"] for rd in reads], np.uint8), y_off, y_len,
             np.array([rd["strand"] for rd in reads], np.uint8), *lists], np.array([rd["x_shift"] for rd in reads], np.int32))


def run(ctx, call, R, compare=True, merge=True, penalty=0.5, want_rcw=False, **kw):
    args, x_shift = pack(call)
    return capi.poa_augment(ctx, R, *args, x_shift=x_shift, compare_repeat_counts=compare, merge_ends=merge, reference_base_penalty=penalty,
                            want_repeat_count_weight=want_rcw, **kw)


def flatten(poas, tots, R):
    """the oracle's per-consensus graphs as the arrays of mrp_poa"""
    nodes = [n for p in poas for n in p["nodes"]]
    ins = [e for n in nodes for e in n["inserts"]]
    dels = [e for n in nodes for e in n["deletes"]]
    f64, i32, i64 = (lambda v: np.array(v, np.float64)), (lambda v: np.array(v, np.int32)), (lambda v: np.array(v, np.int64))
    return dict(
        n_nodes=len(nodes), n_consensus=len(poas), max_repeat=R,
        base_weight=f64([n["base_weights"] for n in nodes]).reshape(len(nodes), 5), repeat_count_weight=f64([n["repeat_count_weights"] for n in nodes]).reshape(len(nodes), R),
        base_pick=i32([n["base_pick"] for n in nodes]), repeat_count_pick=i32([n["repeat_count_pick"] for n in nodes]),
        insert_first=i64(np.cumsum([0] + [len(n["inserts"]) for n in nodes])), insert_str_len=i32([len(e["symbols"]) for e in ins]),
        insert_str_off=i64(np.cumsum([0] + [len(e["symbols"]) for e in ins])[:-1]), insert_weight_forward=f64([e["forward"] for e in ins]),
        insert_weight_reverse=f64([e["reverse"] for e in ins]), insert_n_observations=i64([e["observations"] for e in ins]),
        pool_symbols=np.array([b for e in ins for b in e["symbols"]], np.uint8), pool_counts=i32([c for e in ins for c in e["counts"]]),
        delete_first=i64(np.cumsum([0] + [len(n["deletes"]) for n in nodes])), delete_length=i32([e["length"] for e in dels]),
        delete_weight_forward=f64([e["forward"] for e in dels]), delete_weight_reverse=f64([e["reverse"] for e in dels]),
        delete_n_observations=i64([e["observations"] for e in dels]), totals=f64(tots).reshape(len(poas), 4))


def want(call, R, compare=True, merge=True, penalty=0.5, trace=None):
    """the restatement over every consensus of the call -> (arrays as capi.poa_augment returns them, the graphs, stats)"""
    poas, tots, stats = [], [], dict(complete_inserts=0, complete_deletes=0, longest_run=0)
    for c in call:
        t = None if trace is None else []
        poa, tot, st = po.augment_call(c["symbols"], c["counts"], R, c["reads"], compare, merge, penalty, t)
        if trace is not None:
            trace.append(t)
        poas.append(poa)
        tots.append(tot)
        stats = dict(complete_inserts=stats["complete_inserts"] + st["complete_inserts"], complete_deletes=stats["complete_deletes"] + st["complete_deletes"],
                     longest_run=max(stats["longest_run"], st["longest_run"]))
    return flatten(poas, tots, R), poas, stats


_CACHE = {}


def want_cached(name, call, R, compare=True, merge=True, penalty=0.5):
    key = (name, R, compare, merge, penalty)
    if key not in _CACHE:
        trace = []
        _CACHE[key] = want(call, R, compare, merge, penalty, trace) + (trace,)
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_equal(got, w, stats=None):
    for k in ("n_nodes", "n_consensus", "max_repeat"):
        assert got[k] == w[k], k
    for k in FIELDS_INT:
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(w[k], np.int64)), (k, got[k], w[k])
    for k in FIELDS_F64:
        assert np.array_equal(bits(got[k]), bits(w[k])), (k, got[k], w[k])
    if got["repeat_count_weight"] is not None:
        assert np.array_equal(bits(got["repeat_count_weight"]), bits(w["repeat_count_weight"]))
    if stats is not None:
        st = got["stats"]
        assert (st.complete_inserts, st.complete_deletes, st.longest_run) == (stats["complete_inserts"], stats["complete_deletes"], stats["longest_run"])
        assert st.distinct_inserts == len(w["insert_str_len"]) and st.distinct_deletes == len(w["delete_length"])


def assert_consensus(got, poas, call, use_rle):
    """mrp_poa_consensus over the call's arrays against the restatement, consensus by consensus"""
    first = 0
    for c, poa in zip(call, poas):
        L = len(c["symbols"])
        s, cnt, cmap = capi.poa_consensus(got, first, L, use_rle)
        ws, wc, wm = po.consensus(poa, use_rle)
        assert s.tolist() == ws and cnt.tolist() == wc and cmap.tolist() == wm, (first, use_rle)
        first += L + 1


# ---- the noise model ------------------------------------------------------------------------------------------------------------------

def noisy_consensus(rng, n_nodes, n_reads, R, spanning=True):
    """a run-length reference and reads of it under substitutions, short indels and homopolymer-length errors, with the three lists a
    posterior aligner would give: the path's cells with high weights and, beside many matched cells, a low-weight gap of either kind or
    a low-weight match of the next reference position.  No (x, y) occurs twice in a list: a reference position gives at most one delete
    and one extra match, a read position at most one insert."""
    sx = rng.integers(0, 4, size=n_nodes).astype(np.uint8)
    sx[1:][sx[1:] == sx[:-1]] ^= 1  # neighbouring runs mostly differ
    cx = np.minimum(rng.geometric(0.5, size=n_nodes), R - 1).astype(np.uint8)
    reads = []
    for _ in range(n_reads):
        lo, hi = (0, n_nodes) if spanning else sorted(int(v) for v in rng.choice(n_nodes + 1, size=2, replace=False))
        n = hi - lo
        u, v = rng.random(n).tolist(), rng.random(n).tolist()
        sub, keep, noise = rng.integers(0, 4, n).tolist(), (rng.random(n) < 0.8).tolist(), rng.choice((-1, 1, 2), n).tolist()
        n_ins, ins_b = rng.integers(1, 4, n).tolist(), rng.integers(0, 4, (n, 3)).tolist()
        ins_c = np.minimum(rng.geometric(0.5, (n, 3)), 255).tolist()
        high, low = rng.integers(5_000_000, 10_000_001, (n, 4)).tolist(), rng.integers(1, 2_000_000, n).tolist()
        ref_b, ref_c = sx[lo:hi].tolist(), cx[lo:hi].tolist()
        sy, cy, m, d, i = [], [], [], [], []
        for k in range(n):
            x = lo + k
            if u[k] < 0.04:  # the reference symbol is deleted after the read's last symbol
                d.append((x, len(sy) - 1, high[k][0]))
                continue
            if u[k] < 0.08:  # one to three read symbols inserted after reference x - 1
                for q in range(n_ins[k]):
                    i.append((x - 1, len(sy), high[k][q]))
                    sy.append(ins_b[k][q])
                    cy.append(ins_c[k][q])
            y = len(sy)
            m.append((x, y, high[k][3]))
            if v[k] < 0.15:
                d.append((x, y - 1, low[k]))
            elif v[k] < 0.30:
                i.append((x - 1, y, low[k]))
            elif v[k] < 0.35 and x + 1 < hi:
                m.append((x + 1, y, low[k]))
            sy.append(sub[k] if u[k] >= 0.96 else ref_b[k])
            cy.append(ref_c[k] if keep[k] else max(1, ref_c[k] + noise[k]))
        order = lambda l: [l[q] for q in rng.permutation(len(l)).tolist()]
        reads.append(read(sy, cy, int(rng.integers(0, 2)), order(m), order(d), order(i)))
    return consensus(sx, cx, reads)


@functools.lru_cache(maxsize=None)
def random_call(seed=5, n_nodes=300, n_reads=20, R=12):
    rng = np.random.default_rng(seed)
    return random_shifts([noisy_consensus(rng, n_nodes + 7 * k, n_reads, R, spanning=(k != 1)) for k in range(3)], seed + 1)
