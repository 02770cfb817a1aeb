"""The edge cases of mrp_poa_augment (tests/test_gpu_poa.py, tests/test_poa_host.py): one call of three consensus strings -- one without a
node (a single prefix node), the edges, one without a read -- under a random crop per read, and a second call with the large shapes.  The
edges' reference is a chain of segments, each closed by an N that no walk crosses; a segment has reads of its own (a read need not span:
the alignment-end tests compare against the whole read and the whole reference).  assert_claims() checks on the restatement's own trace
that every case does what its name says."""
from __future__ import annotations

import functools

import numpy as np

from tests import poa_cases as cases

EDGE_R = 12
A, C, G, T, N = 0, 1, 2, 3, 4


class Chain:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.s, self.c, self.reads, self.at, self.read_of = [], [], [], {}, {}

    def w(self):
        return int(self.rng.integers(1, 10_000_001))

    def segment(self, name, symbols, counts=None, last=False):
        x0 = len(self.s)
        self.at[name] = x0
        self.s += list(symbols) + ([] if last else [N])
        self.c += list(counts if counts is not None else [1] * len(symbols)) + ([] if last else [1])
        return x0

    def add(self, name, rd):
        self.read_of.setdefault(name, []).append(len(self.reads))
        self.reads.append(rd)

    def aligned(self, name, x, ops, strand=1, weight=None):
        """a read along a path from reference x: "m" matches the reference symbol as it is, ("M", symbol, count) matches another,
        ("I", symbol, count) inserts, "D" deletes"""
        sy, cy, m, d, i = [], [], [], [], []
        for op in ops:
            wt = self.w() if weight is None else weight
            if op == "D":
                d.append((x, len(sy) - 1, wt))
                x += 1
            elif op[0] == "I":
                i.append((x - 1, len(sy), wt))
                sy.append(op[1]); cy.append(op[2])
            else:
                b, c = (self.s[x], self.c[x]) if op == "m" else op[1:]
                m.append((x, len(sy), wt))
                sy.append(b); cy.append(c)
                x += 1
        self.add(name, cases.read(sy, cy, strand, m, d, i))

    def insert_run(self, name, n, inner=True, holes=(), strand=1):
        """reference G T; a read G, n inserted symbols of A / C, T; with inner every flank of the run is a match"""
        x0 = self.segment(name, [G, T])
        sy = [G] + [int(v) for v in self.rng.integers(0, 2, size=n)] + [T]
        cy = [1] + [int(v) for v in self.rng.integers(1, 256, size=n)] + [1]
        ys = [y for y in range(1, n + 1) if y not in holes]
        left = range(0, n) if inner else [0] + [h for h in holes]
        right = range(2, n + 2) if inner else [n + 1] + [h for h in holes]
        m = [(x0, y, self.w()) for y in left] + [(x0 + 1, y, self.w()) for y in right]
        self.add(name, cases.read(sy, cy, strand, m, [], [(x0, y, self.w()) for y in ys]))

    def delete_run(self, name, n, inner=True, strand=0):
        """reference G, n symbols of A / C, T; a read G T that deletes them"""
        mid = [int(v) for v in self.rng.integers(0, 2, size=n)]
        x0 = self.segment(name, [G] + mid + [T], [1] + [int(v) for v in self.rng.integers(1, EDGE_R, size=n)] + [1])
        left = range(x0, x0 + n) if inner else [x0]
        right = range(x0 + 2, x0 + n + 2) if inner else [x0 + n + 1]
        m = [(x, 0, self.w()) for x in left] + [(x, 1, self.w()) for x in right]
        self.add(name, cases.read([G, T], [1, 1], strand, m, [(x, 0, self.w()) for x in range(x0 + 1, x0 + n + 1)], []))

    def one_symbol(self, name, x, symbol, count, weight, strand=1):
        self.add(name, cases.read([symbol], [count], strand, [(x, 0, weight)], [], []))

    def build(self):
        return cases.consensus(self.s, self.c, self.reads)


def _edges():
    ch = Chain(77)
    # the reference's start: ATATAT
    x0 = ch.segment("start", [A, T, A, T, A, T])
    ch.aligned("at_walks_to_node_0", x0, ["m"] * 6 + [("I", A, 1), ("I", T, 1)])  # and: a run reaching the read's end
    ch.aligned("insert_before_the_reference", x0, [("I", G, 2), "m", "m", "m"], strand=0)  # y = 0 at x = -1
    ch.aligned("insert_at_read_start", x0 + 2, [("I", C, 1), "m", "m"])  # y = 0 at x >= 0
    ch.aligned("delete_before_the_read", x0, ["D"] + ["m"] * 5)  # x = 0 with y = -1
    # runs
    for n in (1, 2, 3):
        ch.insert_run(f"insert_run_{n}", n)
        ch.delete_run(f"delete_run_{n}", n)
    ch.insert_run("insert_inner_flanks_fail", 4, inner=False)
    ch.delete_run("delete_inner_flanks_fail", 4, inner=False)
    ch.insert_run("two_runs_and_a_hole", 5, inner=False, holes=(3,))
    # shifts
    x0 = ch.segment("mismatch", [C, A, T, A, T])
    ch.aligned("stopped_by_a_mismatch", x0, ["m"] * 5 + [("I", A, 1), ("I", T, 1), ("M", G, 1)])
    x0 = ch.segment("counts", [A, T, A, T], [1, 1, 2, 1])
    ch.aligned("stopped_by_a_count", x0, ["m"] * 4 + [("I", A, 2), ("I", T, 1), ("M", G, 1)])
    x0 = ch.segment("length_one", [C, A], [1, 2])
    ch.aligned("length_one_rule", x0, ["m", "m", ("I", A, 3), ("M", G, 1)])
    x0 = ch.segment("rotation", [T, C, A], [1, 2, 3])
    ch.aligned("merged_ends", x0, ["m"] * 3 + [("I", A, 255), ("I", C, 2), ("I", A, 255), ("M", G, 1)])
    x0 = ch.segment("delete_both", [G, C, A, C, A, C, T])
    ch.aligned("delete_shifted_by_both_rules", x0, ["m"] * 4 + ["D", "D", "m"])
    # grouping and order
    x0 = ch.segment("rotated_equal", [T, C, A, G])
    ch.aligned("equal_after_rotation", x0, ["m"] * 3 + [("I", C, 1), ("I", A, 1), "m"], strand=1)
    ch.aligned("equal_after_rotation", x0, ["m"] * 2 + [("I", A, 1), ("I", C, 1), "m", "m"], strand=0)
    x0 = ch.segment("order", [G, T])
    for (b, c), wt in zip(((C, 2), (A, 1), (A, 7), (C, 2)), (500, 900, 100, 50)):
        ch.aligned("first_appearance_order", x0, ["m", ("I", b, c), "m"], weight=wt, strand=b == C)
    x0 = ch.segment("forty", [G, A, T])
    for r in range(40):
        ch.aligned("forty_equal_deletes", x0, ["m", "D", "m"], strand=r % 3 != 0)
    x0 = ch.segment("both", [G, C, T])
    ch.aligned("inserts_and_deletes_at_one_node", x0, ["m", ("I", A, 4), "m", "m"])
    ch.aligned("inserts_and_deletes_at_one_node", x0, ["m", "D", "m"], strand=0)
    # weights
    x0 = ch.segment("heavy", [A], [3])
    for r in range(4):
        n = 250
        ch.add("a_node_under_1000_matches", cases.read(ch.rng.integers(0, 5, size=n), ch.rng.integers(0, 256, size=n), r % 2,
                                                       [(x0, int(y), ch.w()) for y in ch.rng.permutation(n)], [], []))
    x0 = ch.segment("odd", [C, T], [1, 5])
    ch.aligned("read_symbol_n_and_an_overlong_count", x0, [("M", N, 1), ("M", T, 200)])
    x0 = ch.segment("zero", [G], [2])
    for r in range(3):
        ch.one_symbol("a_pick_of_count_0", x0, G, 0, 9_000_000)
    x0 = ch.segment("picks", [G, C, T, A])
    for x, b, wt in ((0, G, 100), (0, A, 200), (1, C, 100), (1, A, 40), (2, T, 10), (2, A, 300), (2, G, 300)):
        ch.one_symbol("picks", x0 + x, b, 1, wt)
    # the reference's end
    x0 = ch.segment("end", [G, C, T, A], last=True)
    ch.aligned("delete_run_reaching_the_end", x0, ["m", "m", "D", "D"], strand=0)
    return ch


@functools.lru_cache(maxsize=None)
def edge_chain():
    return _edges()


@functools.lru_cache(maxsize=None)
def edge_call():
    rng = np.random.default_rng(78)
    call = [cases.consensus([]), edge_chain().build(), cases.consensus(rng.integers(0, 5, size=5), rng.integers(1, EDGE_R, size=5))]
    return cases.random_shifts(call, 79)


def assert_claims():
    ch, call = edge_chain(), edge_call()
    name_of = {r: k for k, v in ch.read_of.items() for r in v}

    def traces(compare, merge):
        w, poas, st, tr = cases.want_cached("edge", call, EDGE_R, compare, merge)
        by = {}
        for t in tr[1]:
            by.setdefault(name_of[t["read"]], []).append(t)
        return w, poas[1], by

    w, poa, by = traces(True, True)
    node = lambda seg, k=0: poa["nodes"][ch.at[seg] + k]
    one = lambda name: by[name][0]
    assert len(by["at_walks_to_node_0"]) == 1 and one("at_walks_to_node_0")["start"] == 6 and one("at_walks_to_node_0")["shifted"] == 0
    assert one("insert_before_the_reference")["key"][1:3] == (-1, 0) and one("insert_at_read_start")["key"][1:3] == (1, 0)
    assert one("delete_before_the_read")["key"][1:3] == (-1, 0)
    for n in (1, 2, 3):
        assert len(by[f"insert_run_{n}"]) == len(by[f"delete_run_{n}"]) == n * (n + 1) // 2
    assert len(by["insert_inner_flanks_fail"]) == len(by["delete_inner_flanks_fail"]) == 1
    assert sorted(t["key"][2:] for t in by["two_runs_and_a_hole"]) == [(1, 2), (4, 5)]
    t = one("stopped_by_a_mismatch")
    assert t["start"] - t["shifted"] == 4 and t["stopped_by"] == "symbol"
    t = one("stopped_by_a_count")
    assert t["stopped_by"] == "count" and t["start"] - t["shifted"] - t["suffix"] == 2
    assert one("length_one_rule").get("length_one_rule") and one("length_one_rule")["start"] - one("length_one_rule")["shifted"] == 1
    t = one("delete_shifted_by_both_rules")
    assert t["kind"] == "delete" and t["suffix"] == 1 and t["start"] - t["shifted"] == 3
    e = call[1]["reads"][ch.read_of["delete_run_reaching_the_end"][0]]
    assert e["x_shift"] > 0 and one("delete_run_reaching_the_end")["length"] == 2
    a, b = by["equal_after_rotation"]
    assert a["shifted"] == b["shifted"] and a["string"] == b["string"] and a["start"] != b["start"] and (a["suffix"] > 0) != (b["suffix"] > 0)
    (e,) = [e for e in poa["nodes"][a["shifted"]]["inserts"] if e["key"] == a["string"]]
    assert e["forward"] > 0 and e["reverse"] > 0 and e["observations"] == 2
    ins = node("order", 1)["inserts"]
    strings, weights = [e["key"] for e in ins], [e["forward"] + e["reverse"] for e in ins]
    assert len(ins) == 3 and strings != sorted(strings) and weights != sorted(weights) and weights != sorted(weights, reverse=True)
    assert ins[0]["observations"] == 2 and ins[0]["forward"] == 550.0
    (d,) = node("forty", 1)["deletes"]
    assert d["observations"] == 40 and d["forward"] > 0 and d["reverse"] > 0
    assert node("both", 1)["inserts"] and node("both", 1)["deletes"]
    assert sum(node("heavy", 1)["base_weights"]) > 0 and sum(1 for t in call[1]["reads"][ch.read_of["a_node_under_1000_matches"][0]]["matches"]) == 250
    assert node("odd", 1)["base_weights"][N] > 0 and node("odd", 2)["repeat_count_weights"][EDGE_R - 1] > 0
    assert node("zero", 1)["repeat_count_pick"] == 0
    assert [node("picks", k)["base_pick"] for k in (1, 2, 3, 4)] == [A, C, G, A]
    for penalty, picks in ((0.0, [A, A, G, A]), (3.0, [G, C, G, A])):
        _, poas, _, _ = cases.want_cached("edge", call, EDGE_R, True, True, penalty)
        assert [poas[1]["nodes"][ch.at["picks"] + k]["base_pick"] for k in (1, 2, 3, 4)] == picks
    # the count stops the walk with compare_repeat_counts on, not off
    _, _, off = traces(False, True)
    assert off["stopped_by_a_count"][0]["start"] - off["stopped_by_a_count"][0]["shifted"] == 4
    # the ends merge into 255 + 255 with merge_ends on and stay apart with it off (the counts differ from the reference's, so the common
    # suffix exists only without compare_repeat_counts)
    t = off["merged_ends"][0]
    assert t["suffix"] == 2 and t["merged"] and t["string"] == ((C, A), (2, 510))
    _, _, apart = traces(False, False)
    assert apart["merged_ends"][0]["string"] == ((C, A, A), (2, 255, 255)) and by["merged_ends"][0]["suffix"] == 0


@functools.lru_cache(maxsize=None)
def big_call():
    """runs of 64 and 65 entries with every flank a match (65: 2 145 complete indels from one run, past a wave and past a tile), and nodes
    with 1, 63, 64, 65 and 200 distinct inserts"""
    ch = Chain(80)
    for n in (64, 65):
        ch.insert_run(f"insert_run_{n}", n, strand=n % 2)
        ch.delete_run(f"delete_run_{n}", n, strand=n % 2)
    for n in (1, 63, 64, 65, 200):
        x0 = ch.segment(f"distinct_{n}", [G, T])
        for r in ch.rng.permutation(n):
            ch.aligned(f"distinct_{n}", x0, ["m", ("I", int(r) % 2, 1 + int(r) // 2), "m"], strand=int(r) % 3 == 0)
            if r % 5 == 0:  # and some of them twice
                ch.aligned(f"distinct_{n}", x0, ["m", ("I", int(r) % 2, 1 + int(r) // 2), "m"], strand=1)
    ch.segment("tail", [A], last=True)
    return cases.random_shifts([ch.build()], 81)
