"""The POA weights, inserts, deletes and consensus of a run-length reference from its reads' posterior lists: a sequential restatement
of the reference (/impl of MarginPolish), the definition mrp_poa_augment and mrp_poa_consensus are held to bit for bit.

    poa_getReferenceGraph (prefix node 'N', count 1)       impl/poa.c:112-127                Poa
    isMatch                                                impl/poa.c:168-174
    addToInserts, addToDeletes                             impl/poa.c:176-233                add_insert(), add_delete()
    matchesReferenceSubstring, hasInternalRepeat           impl/poa.c:235-267
    getShift                                               impl/poa.c:269-298                get_shift()
    getMaxCommonSuffixLength                               impl/poa.c:300-315                common_suffix()
    rleString_rotateString                                 impl/rle.c:157-176                rotate()
    rleString_eq                                           impl/rle.c:115-128
    poa_augment                                            impl/poa.c:317-543                augment()
    getAlignedPairsWithIndelsCroppingReference (x_shift)   impl/poa.c:612-666                augment_call()
    which list is which                                    impl/pairwiseAligner.c:637-681, impl/poa.c:651-653
    the four totals                                        impl/poa.c:794-844                totals()
    getMaxWeight                                           impl/poa.c:1335-1348              get_max_weight()
    poa_getConsensus                                       impl/poa.c:1350-1588              consensus()
    logAdd                                                 impl/pairwiseAligner.c:282-299    posterior_oracle.log_add

Lists.  A gap-x entry (x, y) is a DELETE: reference x deleted after read y (y may be -1).  A gap-y entry (x, y) is an INSERT: read y
inserted after reference x (x may be -1).  An entry's x is shifted by the read's x_shift first (:662-665); the "alignment end" tests then
compare against the whole read and the whole reference (:399, :497).

Weights are integers (floor(p * 1e7)) and every accumulator is a sum of them (a complete indel's weight is a minimum of them), so the
reference's doubles are exact in any order while they stay below 2^53.  The restatement accumulates Python ints, asserts the bound and
converts at the end.  What is order dependent is where a node's distinct insert or delete first appears: node["inserts"] and
node["deletes"] are in the reference's order of creation (reads ascending; inside a read inserts by (x, y_k, y_l), deletes by (y, x_k, x_l)).

Strings are (symbol 0..4, count) sequences: 'a' equals 'A' here, where the reference compares chars.  Counts are whatever the caller
gives (the library gives bytes saturated at 255).

Out of scope, as in the library: poa_getAnchorAlignments (:545-599), poa_polish, the bubble graph, the observation lists (counted only)."""
from __future__ import annotations

import math

from tests.posterior_oracle import log_add

LOG_ZERO = -math.inf
UINT_MAX = 4294967295
LIMIT = 1 << 53


def new_poa(symbols, counts, R):
    """:112-127 -- node 0 is the prefix node ('N', count 1), node i + 1 reference position i"""
    node = lambda b, c: dict(base=int(b), count=int(c), base_weights=[0] * 5, repeat_count_weights=[0] * R, inserts=[], deletes=[])
    return dict(R=R, symbols=[int(b) for b in symbols], counts=[int(c) for c in counts],
                nodes=[node(4, 1)] + [node(b, c) for b, c in zip(symbols, counts)])


def _eq(sa, ca, i, sb, cb, j, compare_counts):
    return sa[i] == sb[j] and (not compare_counts or ca[i] == cb[j])


def has_internal_repeat(s, c, n, compare_counts):
    """:250-267"""
    if len(s) % n != 0:
        return False
    for i in range(n, len(s), n):
        for j in range(n):
            if not _eq(s, c, j, s, c, j + i, compare_counts):
                return False
    return True


def get_shift(ref_s, ref_c, start, s, c, compare_counts, trace=None):
    """:269-298 -> the shifted position"""
    n = 0
    while True:  # while (minRepeatLength++ < str->length): leaves length + 1 when nothing was found (never: n = length always is one)
        n += 1
        if n - 1 >= len(s) or has_internal_repeat(s, c, n, compare_counts):
            break
    k = start - n
    while k >= 0:
        if not all(_eq(ref_s, ref_c, k + l, s, c, l, compare_counts) for l in range(n)):  # matchesReferenceSubstring, :235-248
            if trace is not None:
                trace["stopped_by"] = "symbol" if any(ref_s[k + l] != s[l] for l in range(n)) else "count"
            break
        start = k
        k -= n
    if len(s) == 1 and compare_counts and start > 0 and ref_s[start - 1] == s[0]:  # :292-295
        start -= 1
        if trace is not None:
            trace["length_one_rule"] = True
    return start


def common_suffix(ref_s, ref_c, length1, s, c, compare_counts):
    """:300-315"""
    i = 0
    while length1 - i - 1 >= 0 and len(s) - i - 1 >= 0:
        if not _eq(ref_s, ref_c, length1 - 1 - i, s, c, len(s) - 1 - i, compare_counts):
            break
        i += 1
    return i


def rotate(s, c, rotation, merge_ends):
    """rle.c:157-176 -> (symbols, counts); with merge_ends equal neighbours of the rotated string merge and their counts add"""
    n = len(s)
    rs, rc = [0] * n, [0] * n
    for i in range(n):
        rs[(i + rotation) % n], rc[(i + rotation) % n] = s[i], c[i]
    os_, oc = [], []
    for i in range(n):
        if not merge_ends or i == 0 or rs[i] != rs[i - 1]:
            os_.append(rs[i])
            oc.append(rc[i])
        else:
            oc[-1] += rc[i]
    return os_, oc


def add_insert(node, s, c, weight, strand):
    """:176-204 (rleString_eq: lengths, symbols and counts)"""
    key = (tuple(s), tuple(c))
    for e in node["inserts"]:
        if e["key"] == key:
            break
    else:
        e = dict(key=key, symbols=list(s), counts=list(c), forward=0, reverse=0, observations=0)
        node["inserts"].append(e)
    e["forward" if strand else "reverse"] += weight
    e["observations"] += 1


def add_delete(node, length, weight, strand):
    """:206-233"""
    for e in node["deletes"]:
        if e["length"] == length:
            break
    else:
        e = dict(length=length, forward=0, reverse=0, observations=0)
        node["deletes"].append(e)
    e["forward" if strand else "reverse"] += weight
    e["observations"] += 1


def augment(poa, read_s, read_c, strand, matches, inserts, deletes, compare_counts=True, merge_ends=True, trace=None, read_no=0):
    """:317-543 for one read; the lists hold (x, y, weight) with x already shifted.  trace (a list) receives one dict per complete indel."""
    R, ref_s, ref_c, nodes = poa["R"], poa["symbols"], poa["counts"], poa["nodes"]
    L, M = len(ref_s), len(read_s)
    for x, y, w in matches:  # :324-340
        node = nodes[x + 1]
        node["base_weights"][read_s[y]] += w
        node["repeat_count_weights"][read_c[y] if read_c[y] < R else R - 1] += w
    match_set = set()
    for x, y, _ in matches:  # :344-350
        assert (x, y) not in match_set, "duplicate match (the reference asserts)"
        match_set.add((x, y))
    stats = dict(complete_inserts=0, complete_deletes=0, longest_run=0)

    ins = sorted(inserts, key=lambda t: (t[0], t[1]))  # :355
    i = 0
    while i < len(ins):  # :362-449
        x0, y0 = ins[i][0], ins[i][1]
        j = i + 1
        while j < len(ins) and ins[j][0] == x0 and y0 + j - i == ins[j][1]:
            j += 1
        stats["longest_run"] = max(stats["longest_run"], j - i)
        for k in range(i, j):
            if (x0, y0 + k - i - 1) not in match_set and y0 + k - i - 1 > -1:  # :389-392
                continue
            for l in range(k, j):
                if (x0 + 1, y0 + l - i + 1) not in match_set and y0 + l - i + 1 < M:  # :397-401
                    continue
                yk = ins[k][1]
                s, c = list(read_s[yk:yk + l + 1 - k]), list(read_c[yk:yk + l + 1 - k])
                weight = UINT_MAX
                for m in range(k, l + 1):
                    weight = weight if weight < ins[m][2] else ins[m][2]
                t = None if trace is None else dict(kind="insert", read=read_no, start=x0 + 1, key=(read_no, x0, yk, ins[l][1]))
                pos = get_shift(ref_s, ref_c, x0 + 1, s, c, compare_counts, t)
                suffix = common_suffix(ref_s, ref_c, pos, s, c, compare_counts)
                if suffix > 0:
                    before = len(s)
                    s, c = rotate(s, c, suffix, merge_ends)
                    pos -= suffix
                    if t is not None:
                        t["merged"] = len(s) < before
                if t is not None:
                    t.update(shifted=pos, suffix=suffix, string=(tuple(s), tuple(c)), weight=weight)
                    trace.append(t)
                add_insert(nodes[pos], s, c, weight, strand)
                stats["complete_inserts"] += 1
        i = j

    dels = sorted(deletes, key=lambda t: (t[1], t[0]))  # :454
    i = 0
    while i < len(dels):  # :461-539
        x0, y0 = dels[i][0], dels[i][1]
        j = i + 1
        while j < len(dels) and dels[j][1] == y0 and x0 + j - i == dels[j][0]:
            j += 1
        stats["longest_run"] = max(stats["longest_run"], j - i)
        for k in range(i, j):
            if (x0 + k - i - 1, y0) not in match_set and x0 + k - i - 1 > -1:  # :487-490
                continue
            for l in range(k, j):
                if (x0 + l - i + 1, y0 + 1) not in match_set and x0 + l - i + 1 < L:  # :495-499
                    continue
                length = l - k + 1
                weight = UINT_MAX
                for m in range(k, l + 1):
                    weight = weight if weight < dels[m][2] else dels[m][2]
                start = x0 + k - i
                s, c = ref_s[start:start + length], ref_c[start:start + length]
                t = None if trace is None else dict(kind="delete", read=read_no, start=start, key=(read_no, y0, start, start + length - 1))
                pos = get_shift(ref_s, ref_c, start, s, c, compare_counts, t)
                suffix = common_suffix(ref_s, ref_c, pos, s, c, compare_counts)
                pos -= suffix
                if t is not None:
                    t.update(shifted=pos, suffix=suffix, length=length, weight=weight)
                    trace.append(t)
                add_delete(nodes[pos], length, weight, strand)
                stats["complete_deletes"] += 1
        i = j
    return stats


def get_max_weight(weights, reference_index, penalty):
    """:1335-1348 over doubles"""
    max_weight, max_index = 0.0, -1
    for j, w in enumerate(weights):
        if j != reference_index and w >= max_weight:
            max_weight, max_index = w, j
    assert max_index != -1
    return reference_index if weights[reference_index] * penalty >= max_weight else max_index


def totals(poa):
    """:794-839 -> [reference match weight, disagreement, insert total, delete total] as doubles (exact: asserted below 2^53)"""
    t = [0, 0, 0, 0]
    for node in poa["nodes"]:
        t[0] += node["base_weights"][node["base"]]
        t[1] += sum(w for j, w in enumerate(node["base_weights"]) if j != node["base"])
        t[2] += sum((e["forward"] + e["reverse"]) * len(e["symbols"]) for e in node["inserts"])
        t[3] += sum((e["forward"] + e["reverse"]) * e["length"] for e in node["deletes"])
    assert all(v < LIMIT for v in t)
    return [float(v) for v in t]


def finish(poa, penalty):
    """ints -> the reference's doubles, and getMaxWeight per node as :1481-1490 calls it (the raw result)"""
    for node in poa["nodes"]:
        assert all(w < LIMIT for w in node["base_weights"] + node["repeat_count_weights"])
        node["base_weights"] = [float(w) for w in node["base_weights"]]
        node["repeat_count_weights"] = [float(w) for w in node["repeat_count_weights"]]
        for e in node["inserts"] + node["deletes"]:
            assert e["forward"] < LIMIT and e["reverse"] < LIMIT and e["forward"] + e["reverse"] < LIMIT
            e["forward"], e["reverse"] = float(e["forward"]), float(e["reverse"])
        node["base_pick"] = get_max_weight(node["base_weights"], node["base"], penalty)
        node["repeat_count_pick"] = get_max_weight(node["repeat_count_weights"], node["count"], penalty)
    return poa


def augment_call(symbols, counts, R, reads, compare_counts=True, merge_ends=True, penalty=0.5, trace=None):
    """poa_realign's loop (:682-713) over one reference.  reads: dicts with symbols, counts, strand, x_shift, matches, inserts,
    deletes -- (x, y, weight) lists in call coordinates.  -> (poa with doubles and picks, totals, stats)"""
    poa = new_poa(symbols, counts, R)
    stats = dict(complete_inserts=0, complete_deletes=0, longest_run=0)
    for r, rd in enumerate(reads):
        sh = int(rd.get("x_shift", 0))
        lists = [[(int(x) + sh, int(y), int(w)) for x, y, w in rd[k]] for k in ("matches", "inserts", "deletes")]
        st = augment(poa, [int(b) for b in rd["symbols"]], [int(c) for c in rd["counts"]], bool(rd["strand"]), *lists,
                     compare_counts=compare_counts, merge_ends=merge_ends, trace=trace, read_no=r)
        stats = dict(complete_inserts=stats["complete_inserts"] + st["complete_inserts"],
                     complete_deletes=stats["complete_deletes"] + st["complete_deletes"], longest_run=max(stats["longest_run"], st["longest_run"]))
    tot = totals(poa)
    return finish(poa, penalty), tot, stats


def _log(v):
    """the C library's log: log(0) = -inf, log of a negative or NaN = NaN"""
    if v != v or v < 0.0:
        return math.nan
    return LOG_ZERO if v == 0.0 else math.log(v)


def rle_construct(expanded):
    """rleString_construct, rle.c:8-38 -> (symbols, counts)"""
    s, c = [], []
    for b in expanded:
        if s and s[-1] == b:
            c[-1] += 1
        else:
            s.append(b)
            c.append(1)
    return s, c


def consensus(poa, use_rle=True):
    """:1350-1588 over a finished poa -> (symbols, counts, poa_to_consensus_map).  ValueError where the reference dereferences NULL."""
    nodes = poa["nodes"]
    n = len(nodes)
    weight = lambda e: e["forward"] + e["reverse"]
    total_out = [0.0] * n
    fwd = [0.0] + [LOG_ZERO] * n
    match_fwd = [0.0] * n
    incoming = [[] for _ in range(n + 1)]
    for i, node in enumerate(nodes):  # :1377-1383
        for e in node["deletes"]:
            incoming[i + e["length"] + 1].append((i, e))
    for i, node in enumerate(nodes):  # :1387-1458
        indel = 0.0
        for e in node["inserts"]:
            indel += weight(e)
        for e in node["deletes"]:
            indel += weight(e)
        mt = 0.0
        if i == 0:
            if n == 1:
                mt = 1.0
            else:
                for nn in nodes[1:]:
                    for k in range(5):
                        mt += nn["base_weights"][k]
                mt /= float(n) - 1
                mt -= indel
        else:
            for k in range(5):
                mt += node["base_weights"][k]
            mt -= indel
        mt = 0.0001 if mt <= 0.0 else mt
        total_out[i] = mt + indel
        for e in node["inserts"]:
            fwd[i + 1] = log_add(fwd[i + 1], fwd[i] + _log(weight(e) / total_out[i]))
        for e in node["deletes"]:
            to = i + e["length"] + 1
            fwd[to] = log_add(fwd[to], fwd[i] + _log(weight(e) / total_out[i]))
        match_fwd[i] = fwd[i] + _log(mt / total_out[i])
        fwd[i + 1] = log_add(fwd[i + 1], match_fwd[i])
    cmap = [-1] * (n - 1)
    strings = []  # (symbol, count) pieces, backwards
    running, previous = 0, -1  # previousBase = '-'
    i = n
    while i > 0:  # :1473-1563
        if i < n:
            node = nodes[i]
            base = node["base_pick"]
            if use_rle:
                count = node["repeat_count_pick"]
                count = 1 if count == 0 else count
                strings.append([(base, count)])
                if previous != base:
                    cmap[i - 1] = running
                    running += 1
                previous = base
            else:
                strings.append([(base, 1)])
                cmap[i - 1] = running
                running += 1
        max_ins_p, tot_ins, max_ins = LOG_ZERO, LOG_ZERO, None
        for e in nodes[i - 1]["inserts"]:
            p = _log(weight(e) / total_out[i - 1]) + fwd[i - 1]
            if p > max_ins_p:
                max_ins_p, max_ins = p, e
            tot_ins = log_add(tot_ins, p)
        max_del_p, tot_del, max_del = LOG_ZERO, LOG_ZERO, None
        for src, e in incoming[i]:
            p = _log(weight(e) / total_out[src]) + fwd[src]
            if p > max_del_p:
                max_del_p, max_del = p, e
            tot_del = log_add(tot_del, p)
        if match_fwd[i - 1] >= tot_del and match_fwd[i - 1] >= tot_ins:
            i -= 1
        elif tot_ins >= tot_del:
            if max_ins is None:
                raise ValueError(f"node {i - 1}: no maximal insert (the reference dereferences NULL)")
            strings.append(list(zip(max_ins["symbols"], max_ins["counts"])))
            if use_rle:
                base = max_ins["symbols"][-1]
                running += len(max_ins["symbols"]) + (0 if base != previous else -1)
                previous = max_ins["symbols"][0]
            else:
                running += sum(max_ins["counts"])
            i -= 1
        else:
            if max_del is None:
                raise ValueError(f"node {i}: no maximal delete (the reference dereferences NULL)")
            i -= max_del["length"] + 1
    expanded = [b for piece in reversed(strings) for b, c in piece for _ in range(c)]
    s, c = rle_construct(expanded) if use_rle else (expanded, [1] * len(expanded))
    for k in range(n - 1):  # :1573-1578
        if cmap[k] != -1:
            cmap[k] = len(s) - 1 - cmap[k]
    return s, c, cmap
